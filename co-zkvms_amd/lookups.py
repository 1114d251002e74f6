"""Instruction-lookups harness over the C ABI (`cozk_lookups_*`): SURVEY 8(f)1 restated synthetically -- the toggled /
sparse batched grand product of Lasso's read / write memory checking (co-jolt/src/subprotocols/sparse_grand_product.rs)
on the GPU(s), coordinator + verifier on the calling thread -- and thin wrappers of the toggle-layer entry points
(`cozk_toggle_*`, `cozk_toggle_group_*`) and of the primary sumcheck's (`cozk_primary_*`) for the kernel-level parity tests."""
import ctypes

import numpy as np

from . import _lib as L
from .engine import Vec, fr_to_mont_limbs, mont_limbs_to_int


class LookupsConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("log_n", ctypes.c_int), ("n_pairs", ctypes.c_int), ("density_pct", ctypes.c_int),
                ("devices", ctypes.c_int * 3), ("seed", ctypes.c_uint64), ("log_workers", ctypes.c_int), ("primary", ctypes.c_int), ("mix", ctypes.c_int)]


class LookupsResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_primary_ms", ctypes.c_double), ("t_construct_ms", ctypes.c_double),
                ("t_prove_ms", ctypes.c_double),
                ("t_worker_ms", ctypes.c_double), ("bytes_star_up", ctypes.c_uint64), ("bytes_star_down", ctypes.c_uint64),
                ("bytes_ring", ctypes.c_uint64), ("star_messages", ctypes.c_uint64), ("proof_len", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32)]


LOOKUPS_SYMBOLS = ["cozk_lookups_create", "cozk_lookups_error", "cozk_lookups_destroy", "cozk_lookups_prove", "cozk_lookups_proof_bytes",
                   "cozk_toggle_create", "cozk_toggle_free", "cozk_toggle_batch", "cozk_toggle_len", "cozk_toggle_layer_output", "cozk_toggle_bind",
                   "cozk_toggle_round", "cozk_toggle_final_claims", "cozk_toggle_download", "cozk_lookups_get_sparse_stats",
                   "cozk_lookups_reset_sparse_stats", "cozk_primary_create", "cozk_primary_free", "cozk_primary_degree", "cozk_primary_len",
                   "cozk_primary_round_begin", "cozk_primary_level", "cozk_primary_round_finish", "cozk_primary_final_evals"]

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_toggle_create.restype = _i
    l.cozk_toggle_create.argtypes = [_vp, _i, _vp, _sz, _vp, _vp, _i, ctypes.POINTER(_vp)]
    l.cozk_toggle_free.restype = _i
    l.cozk_toggle_free.argtypes = [_vp]
    l.cozk_toggle_batch.restype = _sz
    l.cozk_toggle_batch.argtypes = [_vp]
    l.cozk_toggle_len.restype = _sz
    l.cozk_toggle_len.argtypes = [_vp]
    l.cozk_toggle_layer_output.restype = _i
    l.cozk_toggle_layer_output.argtypes = [_vp, _vp, _i, ctypes.POINTER(_vp)]
    l.cozk_toggle_bind.restype = _i
    l.cozk_toggle_bind.argtypes = [_vp, _vp, _vp]
    l.cozk_toggle_round.restype = _i
    l.cozk_toggle_round.argtypes = [_vp, _vp, _vp, _vp, _i, _vp]
    l.cozk_toggle_final_claims.restype = _i
    l.cozk_toggle_final_claims.argtypes = [_vp, _vp, _vp, _vp, _vp]
    l.cozk_toggle_download.restype = _i
    l.cozk_toggle_download.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    l.cozk_primary_create.restype = _i
    l.cozk_primary_create.argtypes = [_vp, _i, _i, _vp, _sz, _vp, _vp, _sz, _vp, _vp, ctypes.POINTER(_vp)]
    l.cozk_primary_free.restype = _i
    l.cozk_primary_free.argtypes = [_vp]
    l.cozk_primary_degree.restype = _i
    l.cozk_primary_degree.argtypes = [_vp]
    l.cozk_primary_len.restype = _sz
    l.cozk_primary_len.argtypes = [_vp]
    l.cozk_primary_round_begin.restype = _i
    l.cozk_primary_round_begin.argtypes = [_vp, _vp, _vp, ctypes.POINTER(_sz), ctypes.POINTER(_i)]
    l.cozk_primary_level.restype = _i
    l.cozk_primary_level.argtypes = [_vp, _vp, _i, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz)]
    l.cozk_primary_round_finish.restype = _i
    l.cozk_primary_round_finish.argtypes = [_vp, _vp, _vp]
    l.cozk_primary_final_evals.restype = _i
    l.cozk_primary_final_evals.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
    return l


class SparseStats(ctypes.Structure):
    """cozk_sparse_stats: the per-context counters of the sparse pair layers"""
    _fields_ = [("layers_sparse", ctypes.c_uint64), ("layers_scattered", ctypes.c_uint64), ("sparse_rounds", ctypes.c_uint64),
                ("handovers", ctypes.c_uint64), ("bytes_sparse", ctypes.c_uint64), ("bytes_dense_equivalent", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class LookupsHarness(L.HarnessHandle):
    PREFIX, CONFIG, RESULT = "cozk_lookups", LookupsConfig, LookupsResult
    EXTRA = {"cozk_lookups_get_sparse_stats": (_i, [_vp, _i, _vp]), "cozk_lookups_reset_sparse_stats": (_i, [_vp])}

    def __init__(self, mode="plain", log_n=6, n_pairs=2, density_pct=25, devices=(0, 0, 0), seed=1, primary=False, log_workers=0, mix="uniform"):
        cfg = LookupsConfig()
        cfg.mix = 1 if mix == "sha2" else 0
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.log_n, cfg.n_pairs, cfg.density_pct = log_n, n_pairs, density_pct
        cfg.devices = (ctypes.c_int * 3)(*devices)
        cfg.seed = seed
        cfg.primary = 1 if primary else 0
        cfg.log_workers = log_workers
        self._open(cfg)

    def sparse_stats(self, party=0):
        """the sparse pair layer counters of one party's context (all zero unless a prove ran with COZK_TOGGLE_SPARSE=1)"""
        st = SparseStats()
        if self._l.cozk_lookups_get_sparse_stats(self.h, party, ctypes.byref(st)) != L.OK:
            raise L.CozkError(-1, "lookups_get_sparse_stats")
        return st

    def reset_sparse_stats(self):
        self._l.cozk_lookups_reset_sparse_stats(self.h)


class ToggleLayer:
    """Rep3BatchedGrandProductToggleLayer on the device (`cozk_toggle`): `flags` = one list of 0/1 per PAIR of circuits,
    `fingerprints` = one list per circuit of ints (plain) or (a, b) tuples (Rep3)"""

    def __init__(self, ctx, flags, fingerprints):
        from .poly import Rep3DenseInterleavedPolynomial, SplitEqPolynomial  # noqa: F401 - same module family
        self._l = _decl()
        self.ctx = ctx
        self.mode = L.MODE_REP3 if isinstance(fingerprints[0][0], tuple) else L.MODE_PLAIN
        self._flag_vecs = [Vec.from_ints(ctx, f, kind=L.SCALAR_U8) for f in flags]
        flat = [v for row in fingerprints for v in row]
        if self.mode == L.MODE_REP3:
            fa, fb = Vec.from_ints(ctx, [v[0] for v in flat]), Vec.from_ints(ctx, [v[1] for v in flat])
        else:
            fa, fb = Vec.from_ints(ctx, flat), None
        arr = (_vp * len(flags))(*[v.h for v in self._flag_vecs])
        h = _vp()
        ctx.check(self._l.cozk_toggle_create(ctx.h, self.mode, arr, len(flags), fa.h, fb.h if fb is not None else None, 0, ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_vecs(cls, ctx, flag_vecs, fp_a, fp_b=None):
        """the same layer from device vectors (no host lists): one U8 Vec of N entries per pair of circuits, the fingerprints as FR
        Vecs of 2 x pairs x N entries (fp_b: the second Rep3 component)"""
        self = cls.__new__(cls)
        self._l = _decl()
        self.ctx = ctx
        self.mode = L.MODE_REP3 if fp_b is not None else L.MODE_PLAIN
        self._flag_vecs = list(flag_vecs)
        self._fp_vecs = (fp_a, fp_b)
        arr = (_vp * len(flag_vecs))(*[v.h for v in flag_vecs])
        h = _vp()
        ctx.check(self._l.cozk_toggle_create(ctx.h, self.mode, arr, len(flag_vecs), fp_a.h, fp_b.h if fp_b is not None else None, 0, ctypes.byref(h)))
        self.h = h
        return self

    def layer_output(self, party=0):
        from .poly import Rep3DenseInterleavedPolynomial
        h = _vp()
        self.ctx.check(self._l.cozk_toggle_layer_output(self.ctx.h, self.h, party, ctypes.byref(h)))
        return Rep3DenseInterleavedPolynomial(self.ctx, h, self.mode)

    def bind(self, r):
        rr = fr_to_mont_limbs([r])[0]
        self.ctx.check(self._l.cozk_toggle_bind(self.ctx.h, self.h, rr.ctypes.data))

    def round(self, eq, r=None, party=0):
        """bind with r (None in the first round), then this party's additive g(0), g(2), g(3)"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        out = np.zeros((3, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_toggle_round(self.ctx.h, self.h, eq.h, rr.ctypes.data if rr is not None else None, party, out.ctypes.data))
        return mont_limbs_to_int(out)

    def final_claims(self):
        fl, pa, pb = (np.zeros(4, dtype=np.uint64) for _ in range(3))
        self.ctx.check(self._l.cozk_toggle_final_claims(self.ctx.h, self.h, fl.ctypes.data, pa.ctypes.data, pb.ctypes.data))
        f, a, b = (mont_limbs_to_int(x.reshape(1, 4))[0] for x in (fl, pa, pb))
        return f, ((a, b) if self.mode == L.MODE_REP3 else a)

    def download(self):
        nf, npn = _sz(), _sz()
        self.ctx.check(self._l.cozk_toggle_download(self.ctx.h, self.h, None, None, None, ctypes.byref(nf), ctypes.byref(npn)))
        fl = np.zeros((nf.value, 4), dtype=np.uint64)
        pa = np.zeros((npn.value, 4), dtype=np.uint64)
        pb = np.zeros((npn.value, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_toggle_download(self.ctx.h, self.h, fl.ctypes.data, pa.ctypes.data, pb.ctypes.data, None, None))
        a = mont_limbs_to_int(pa)
        fps = list(zip(a, mont_limbs_to_int(pb))) if self.mode == L.MODE_REP3 else a
        return mont_limbs_to_int(fl), fps

    def free(self):
        if getattr(self, "h", None):
            self._l.cozk_toggle_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PrimaryInstr(ctypes.Structure):
    """cozk_primary_instr: one row of the instruction table -- a collation form (L.G_*) over indices into the E polynomials"""
    _fields_ = [("form", ctypes.c_int), ("n_mems", ctypes.c_int), ("mems", ctypes.c_int * L.PRIMARY_MAX_MEMS), ("bits", ctypes.c_int)]

    @classmethod
    def of(cls, form, mems, bits=0):
        mems = list(mems)
        row = cls(form=form, n_mems=len(mems), bits=bits)
        for t, m in enumerate(mems[:L.PRIMARY_MAX_MEMS]):
            row.mems[t] = m
        return row


class PrimarySumcheck:
    """Lasso's primary sumcheck of the instruction lookups on the device (`cozk_primary`): one party's state and the three steps
    of a round.  The exchange between the levels and the protocol around the rounds are the caller's"""

    def __init__(self, ctx, h, mode, n_instr, n_mem):
        self._l = _decl()
        self.ctx, self.h, self.mode, self.n_instr, self.n_mem = ctx, h, mode, n_instr, n_mem

    @classmethod
    def create(cls, ctx, mode, party, instrs, flags, E, outputs, eq):
        """`instrs` = PrimaryInstr rows, `flags` = one Vec per row (0/1 U8 columns, or FR vectors that are already bound), `E` =
        the Rep3DensePolynomials the rows index, `outputs` = lookup_outputs, `eq` = an FR Vec; all of `mode` and one length.
        Everything is copied: the arguments stay untouched and need not outlive the object"""
        l = _decl()
        rows = (PrimaryInstr * max(len(instrs), 1))(*instrs)
        fl = (_vp * max(len(flags), 1))(*[None if v is None else v.h for v in flags])
        Ep = (_vp * max(len(E), 1))(*[None if v is None else v.h for v in E])
        h = _vp()
        ctx.check(l.cozk_primary_create(ctx.h, mode, party, rows, len(instrs), fl, Ep, len(E), outputs.h, eq.h, ctypes.byref(h)))
        return cls(ctx, h, mode, len(instrs), len(E))

    def degree(self):
        return self._l.cozk_primary_degree(self.h)

    def __len__(self):
        return self._l.cozk_primary_len(self.h)

    def round_begin(self, r=None):
        """bind with r (None in the first round), the linear pass and the item list -> (n_items, n_levels)"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        n_items, n_levels = _sz(), _i()
        self.ctx.check(self._l.cozk_primary_round_begin(self.ctx.h, self.h, rr.ctypes.data if rr is not None else None, ctypes.byref(n_items),
                                                        ctypes.byref(n_levels)))
        return n_items.value, n_levels.value

    def level(self, level, key_self=None, key_prev=None, counter=0):
        """the local half of multiplication level `level` -> (send, recv, n_elems): device addresses (None: no buffer) of this
        party's n_elems new additive shares and of where the previous party's must land before the next call"""
        send, recv, n = _vp(), _vp(), _sz()
        self.ctx.check(self._l.cozk_primary_level(self.ctx.h, self.h, level, L.prf_key(key_self), L.prf_key(key_prev), counter, ctypes.byref(send),
                                                  ctypes.byref(recv), ctypes.byref(n)))
        return send.value, recv.value, n.value

    def level_elems(self, level):
        """what `level` will report as n_elems in the current round (0: the level holds nothing)"""
        return L.lib().cozk_primary_level_elems(self.h, level)

    def round_finish(self):
        """this party's additive evaluations at X = 0, 2, 3, .., degree"""
        d = self.degree()
        out = np.zeros((d, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_primary_round_finish(self.ctx.h, self.h, out.ctypes.data))
        return mont_limbs_to_int(out)

    def final_evals(self, r):
        """bind with the last challenge -> (E(r) per memory, flag(r) per instruction, lookup_outputs(r), eq(r)); E and the outputs as
        ints (plain) or (a, b) tuples (Rep3)"""
        rr = fr_to_mont_limbs([r])[0]
        Ee, Fe = np.zeros((2 * self.n_mem, 4), dtype=np.uint64), np.zeros((self.n_instr, 4), dtype=np.uint64)
        oe, qe = np.zeros((2, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_primary_final_evals(self.ctx.h, self.h, rr.ctypes.data, Ee.ctypes.data, Fe.ctypes.data, oe.ctypes.data,
                                                        qe.ctypes.data))
        ev, o = mont_limbs_to_int(Ee), mont_limbs_to_int(oe)
        if self.mode == L.MODE_REP3:
            return [(ev[2 * m], ev[2 * m + 1]) for m in range(self.n_mem)], mont_limbs_to_int(Fe), (o[0], o[1]), mont_limbs_to_int(qe)[0]
        return [ev[2 * m] for m in range(self.n_mem)], mont_limbs_to_int(Fe), o[0], mont_limbs_to_int(qe)[0]

    def free(self):
        if getattr(self, "h", None):
            self._l.cozk_primary_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PRIMARY_GROUP_SYMBOLS = ["cozk_primary_group_create", "cozk_primary_group_level", "cozk_primary_group_round_finish", "cozk_primary_group_len",
                         "cozk_primary_group_level_buffer", "cozk_primary_group_free"]
PRIMARY_GROUP_MAX = 15
# the king level exchange and the public exchange plan (beside the lists above, whose lengths tests pin)
PRIMARY_KING_SYMBOLS = ["cozk_primary_group_create_king", "cozk_primary_group_level_king", "cozk_primary_group_staging_bytes",
                        "cozk_primary_level_elems", "cozk_primary_plan"]
PRIMARY_MAX_LEVELS = 4


def primary_plan(ctx, instrs, flags, log_n):
    """the public exchange plan (`cozk_primary_plan`): from the instruction table and the U8 flag columns alone, the n_elems every
    level of every round will exchange -> (rows[round][level - 1], total)"""
    l = L.lib()
    rows = (PrimaryInstr * max(len(instrs), 1))(*instrs)
    fl = (_vp * max(len(flags), 1))(*[None if v is None else v.h for v in flags])
    out = np.zeros((max(log_n, 1), PRIMARY_MAX_LEVELS), dtype=np.uint64)
    total = ctypes.c_uint64()
    ctx.check(l.cozk_primary_plan(ctx.h, rows, len(instrs), fl, log_n, out.ctypes.data, ctypes.byref(total)))
    return [[int(x) for x in row] for row in out[:log_n]], int(total.value)


class PrimaryGroup:
    """k = 2t + 1 PLAIN `PrimarySumcheck` members of one table, one set of flags and one state -- the senders of a Shamir prover --
    driven on the stream of the driver `ctx` (`cozk_primary_group_*`, csrc/primary_group.inc): one multiplication level with its
    degree reduction in two launches, one grouped round_finish.  `keys[m]` = member m's t PRF keys (32 bytes each).  The members may
    belong to other contexts on the same device; the group refers to them and they must outlive it."""

    def __init__(self, ctx, members, keys):
        """keys = None: a group without PRF keys (`cozk_primary_group_create_king`): king levels only"""
        self._l = L.lib()
        self.ctx = ctx
        self.members = list(members)
        self.k = len(self.members)
        arr = (_vp * max(1, self.k))(*[None if m is None else m.h for m in self.members])
        h = _vp()
        if keys is None:
            ctx.check(self._l.cozk_primary_group_create_king(ctx.h, arr, self.k, ctypes.byref(h)))
        else:
            blob = b"".join(bytes(k) for ks in keys for k in ks)
            ctx.check(self._l.cozk_primary_group_create(ctx.h, arr, self.k, blob, ctypes.byref(h)))
        self.h = h

    def level_king(self, level, r_t, r_2t, r_offset=0):
        """the king form of `level` on a preprocessed double-random pair: r_t[q] / r_2t[m] = member q's degree-t and member m's
        degree-2t half (FR Vecs on the driver's device, None allowed only to provoke the refusal); pair element r_offset + pos serves
        position pos once -> n_elems"""
        n = _sz()
        rt = (_vp * max(1, len(r_t)))(*[None if v is None else v.h for v in r_t])
        r2t = (_vp * max(1, len(r_2t)))(*[None if v is None else v.h for v in r_2t])
        self.ctx.check(self._l.cozk_primary_group_level_king(self.h, level, rt, r2t, r_offset, ctypes.byref(n)))
        return n.value

    def staging_bytes(self):
        """the staging block's current size in bytes"""
        return self._l.cozk_primary_group_staging_bytes(self.h)

    def __len__(self):
        return self._l.cozk_primary_group_len(self.h)

    def level(self, level, counter=0):
        """multiplication level `level` of the current round for all members: every member's slot values re-dealt and combined into
        every member's level buffer -> n_elems per (sender, receiver) pair (0: nothing launched, the counter stays)"""
        n = _sz()
        self.ctx.check(self._l.cozk_primary_group_level(self.h, level, counter, ctypes.byref(n)))
        return n.value

    def round_finish_raw(self, degree):
        out = np.zeros((self.k, degree, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_primary_group_round_finish(self.h, out.ctypes.data))
        return out

    def round_finish(self):
        """every member's evaluations at X = 0, 2, 3, .., degree: row m is member m's own round_finish"""
        d = self.members[0].degree()
        v = mont_limbs_to_int(self.round_finish_raw(d).reshape(-1, 4))
        return [v[d * m:d * (m + 1)] for m in range(self.k)]

    def level_buffer(self, member, level):
        """(device address or None, n_elems) of a member's level buffer"""
        buf, n = _vp(), _sz()
        self.ctx.check(self._l.cozk_primary_group_level_buffer(self.h, member, level, ctypes.byref(buf), ctypes.byref(n)))
        return buf.value, n.value

    def free(self):
        if getattr(self, "h", None):
            self._l.cozk_primary_group_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ToggleGroup:
    """ONE PLAIN toggle layer with k fingerprint planes over one copy of the public flags, driven on the stream of the driver `ctx`
    (`cozk_toggle_group_*`): the senders of a Shamir prover.  `flag_vecs` = one U8 Vec of N entries per pair of circuits,
    `fp_vecs` = k FR Vecs of 2 x pairs x N entries, which may belong to other contexts on the same device.  Without
    take_ownership the group only refers to the fingerprint Vecs: they are only read and must outlive it."""

    def __init__(self, ctx, flag_vecs, fp_vecs, take_ownership=False):
        self._l = L.lib()
        self.ctx = ctx
        self._flag_vecs, self._fp_vecs = list(flag_vecs), list(fp_vecs)
        self.k = len(self._fp_vecs)
        fl = (_vp * max(len(self._flag_vecs), 1))(*[None if v is None else v.h for v in self._flag_vecs])
        fp = (_vp * max(self.k, 1))(*[None if v is None else v.h for v in self._fp_vecs])
        h = _vp()
        ctx.check(self._l.cozk_toggle_group_create(ctx.h, fl, len(self._flag_vecs), fp, self.k, 1 if take_ownership else 0, ctypes.byref(h)))
        self.h = h

    def layer_outputs(self, owners=None):
        """every member's dense interleaved layer flag ? fingerprint : 1 in one launch -> k FR Vecs, member m's a vector of owners[m]
        (default: the driver)"""
        owners = list(owners) if owners is not None else [self.ctx] * self.k
        out = (_vp * max(self.k, 1))()
        self.ctx.check(self._l.cozk_toggle_group_layer_outputs(self.h, (_vp * max(self.k, 1))(*[c.h for c in owners]), out))
        return [Vec(owners[m], _vp(out[m]), L.SCALAR_FR) for m in range(self.k)]

    def round(self, eq, r=None):
        """bind planes, flags and eq with r (None in the first round), then every member's g(0), g(2), g(3) -> k lists of 3"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        out = np.zeros((3 * self.k, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_toggle_group_round(self.h, eq.h, rr.ctypes.data if rr is not None else None, out.ctypes.data))
        v = mont_limbs_to_int(out)
        return [v[3 * m:3 * m + 3] for m in range(self.k)]

    def bind(self, r):
        rr = fr_to_mont_limbs([r])[0]
        self.ctx.check(self._l.cozk_toggle_group_bind(self.h, rr.ctypes.data))

    def final_claims(self, k_final=None):
        """(the bound flag, the bound fingerprints of members 0..k_final - 1) of a fully bound group"""
        k_final = self.k if k_final is None else k_final
        fl, fp = np.zeros(4, dtype=np.uint64), np.zeros((max(k_final, 1), 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_toggle_group_final_claims(self.h, fl.ctypes.data, fp.ctypes.data, k_final))
        return mont_limbs_to_int(fl.reshape(1, 4))[0], mont_limbs_to_int(fp)[:max(k_final, 0)]

    def free(self):
        if getattr(self, "h", None):
            self._l.cozk_toggle_group_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sparse_stats(ctx):
    st = SparseStats()
    ctx.check(L.lib().cozk_sparse_get_stats(ctx.h, ctypes.byref(st)))
    return st


def sparse_reset_stats(ctx):
    ctx.check(L.lib().cozk_sparse_reset_stats(ctx.h))


class SparseLayer:
    """Rep3SparseInterleavedPolynomial on the device as stored pairs (`cozk_sparse_layer`): a sorted list of pair indices and the
    pairs' (L, R) values; a missing pair is the party's trivial share of one in both entries.  Build one with `from_toggle`,
    `from_lists` or `from_output`."""

    def __init__(self, ctx, h, mode):
        self._l = L.lib()
        self.ctx, self.h, self.mode = ctx, h, mode

    @classmethod
    def from_toggle(cls, ctx, toggle, party=0):
        """layer_output of an unbound ToggleLayer: the pairs with a set flag"""
        h = _vp()
        ctx.check(L.lib().cozk_toggle_sparse_output(ctx.h, toggle.h, party, ctypes.byref(h)))
        return cls(ctx, h, toggle.mode)

    @classmethod
    def from_lists(cls, ctx, n, idx, pairs):
        """`idx` = strictly increasing pair indices, `pairs` = one (L, R) per index, ints (plain) or (a, b) tuples (Rep3)"""
        rep3 = bool(pairs) and isinstance(pairs[0][0], tuple)
        return cls.from_vecs(ctx, L.MODE_REP3 if rep3 else L.MODE_PLAIN, n, *cls._vecs(ctx, idx, pairs, rep3))

    @staticmethod
    def _vecs(ctx, idx, pairs, rep3):
        flat = [v for pr in pairs for v in pr]
        iv = Vec.from_ints(ctx, list(idx), kind=L.SCALAR_U32)
        if rep3:
            return iv, Vec.from_ints(ctx, [v[0] for v in flat]), Vec.from_ints(ctx, [v[1] for v in flat])
        return iv, Vec.from_ints(ctx, flat), None

    @classmethod
    def from_vecs(cls, ctx, mode, n, idx, a, b=None, take_ownership=False):
        h = _vp()
        ctx.check(L.lib().cozk_sparse_layer_create(ctx.h, mode, n, idx.h, a.h, b.h if b is not None else None, 1 if take_ownership else 0,
                                                   ctypes.byref(h)))
        return cls(ctx, h, mode)

    def __len__(self):
        return self._l.cozk_sparse_layer_len(self.h)

    @property
    def count(self):
        return self._l.cozk_sparse_layer_count(self.h)

    @property
    def nbytes(self):
        return self._l.cozk_sparse_layer_bytes(self.h)

    def next_count(self):
        """stored pairs after a bind = stored pairs of the output layer"""
        n = _sz()
        self.ctx.check(self._l.cozk_sparse_layer_next_count(self.ctx.h, self.h, ctypes.byref(n)))
        return n.value

    def output_local(self, masked=False, key_self=None, key_prev=None, counter=0):
        """the compact vector of 2 * next_count() additive products (+ the zero-sharing masks at counter + position)"""
        h = _vp()
        self.ctx.check(self._l.cozk_sparse_layer_output_local(self.ctx.h, self.h, 1 if masked else 0, L.prf_key(key_self), L.prf_key(key_prev), counter,
                                                              ctypes.byref(h)))
        return Vec(self.ctx, h, L.SCALAR_FR)

    def from_output(self, va, vb=None, take_ownership=False):
        """the next layer: the products of output_local (a) and, for Rep3, what the ring reshare gave (b)"""
        h = _vp()
        self.ctx.check(self._l.cozk_sparse_layer_from_output(self.ctx.h, self.h, va.h, vb.h if vb is not None else None, 1 if take_ownership else 0,
                                                             ctypes.byref(h)))
        return SparseLayer(self.ctx, h, self.mode)

    def bind(self, r):
        rr = fr_to_mont_limbs([r])[0]
        self.ctx.check(self._l.cozk_sparse_layer_bind(self.ctx.h, self.h, rr.ctypes.data))

    def round(self, eq, r=None, party=0):
        """bind layer and eq with r (None in the first round), then this party's additive g(0), g(2), g(3)"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        out = np.zeros((3, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_sparse_layer_round(self.ctx.h, self.h, eq.h, rr.ctypes.data if rr is not None else None, party, out.ctypes.data))
        return mont_limbs_to_int(out)

    def to_dense(self, party=0):
        from .poly import Rep3DenseInterleavedPolynomial
        h = _vp()
        self.ctx.check(self._l.cozk_sparse_layer_to_dense(self.ctx.h, self.h, party, ctypes.byref(h)))
        return Rep3DenseInterleavedPolynomial(self.ctx, h, self.mode)

    def download(self):
        """(idx, pairs): the pair indices and one (L, R) per index"""
        cnt = self.count
        idx = np.zeros(max(cnt, 1), dtype=np.uint32)
        a = np.zeros((max(2 * cnt, 1), 4), dtype=np.uint64)
        b = np.zeros((max(2 * cnt, 1), 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_sparse_layer_download(self.ctx.h, self.h, idx.ctypes.data, a.ctypes.data, b.ctypes.data))
        va = mont_limbs_to_int(a)[:2 * cnt]
        vals = list(zip(va, mont_limbs_to_int(b)[:2 * cnt])) if self.mode == L.MODE_REP3 else va
        return [int(i) for i in idx[:cnt]], [(vals[2 * i], vals[2 * i + 1]) for i in range(cnt)]

    def free(self):
        if getattr(self, "h", None):
            self._l.cozk_sparse_layer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
