"""Host-side handles over the C ABI (include/cozk.h): context, device vectors, SRS bases, MSM.

Mirrors the reference's MSM seam: `VariableBaseMSM::{msm_field_elements, batch_msm}` behind
`PST13::{commit, batch_commit, open}` (co-jolt/src/poly/commitment/pst13.rs:282-331,428-474).
Field elements cross this layer as Python ints (canonical) or numpy uint64[n,4] Montgomery limbs.
"""
import ctypes

import numpy as np

from . import _lib as L

FR_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FQ_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_MONT = 1 << 256
_MASK64 = (1 << 64) - 1

_KIND_DTYPE = {L.SCALAR_U8: np.uint8, L.SCALAR_U16: np.uint16, L.SCALAR_U32: np.uint32,
               L.SCALAR_U64: np.uint64, L.SCALAR_I64: np.int64}


def fr_to_mont_limbs(values, mod=FR_MOD):
    """canonical ints -> uint64[n,4] Montgomery limbs (arkworks in-memory layout)"""
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (int(v) % mod) * _MONT % mod
        out[i, 0] = m & _MASK64
        out[i, 1] = (m >> 64) & _MASK64
        out[i, 2] = (m >> 128) & _MASK64
        out[i, 3] = (m >> 192) & _MASK64
    return out


_RINV = {FR_MOD: pow(_MONT, -1, FR_MOD), FQ_MOD: pow(_MONT, -1, FQ_MOD)}


def mont_limbs_to_int(limbs, mod=FR_MOD):
    """uint64[...,4] Montgomery limbs -> list of canonical ints"""
    arr = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    rinv = _RINV[mod]
    res = []
    for row in arr:
        m = int(row[0]) | (int(row[1]) << 64) | (int(row[2]) << 128) | (int(row[3]) << 192)
        res.append(m * rinv % mod)
    return res


def point_to_abi(pt):
    """affine (x, y) canonical ints or None -> (uint64[8], infinity flag)"""
    if pt is None:
        return np.zeros(8, dtype=np.uint64), 1
    xy = np.concatenate([fr_to_mont_limbs([pt[0]], FQ_MOD)[0], fr_to_mont_limbs([pt[1]], FQ_MOD)[0]])
    return xy, 0


def point_from_abi(xy, inf):
    if inf:
        return None
    x = mont_limbs_to_int(xy[:4], FQ_MOD)[0]
    y = mont_limbs_to_int(xy[4:], FQ_MOD)[0]
    return (x, y)


def wire_g1_encode(pt):
    """ark-serialize uncompressed G1Affine bytes of an affine point (cozk_wire_g1_encode; host only)"""
    xy, inf = point_to_abi(pt)
    out = (ctypes.c_uint8 * 64)()
    rc = L.lib().cozk_wire_g1_encode(xy.ctypes.data, inf, out)
    if rc != L.OK:
        raise L.CozkError(rc, "wire_g1_encode")
    return bytes(out)


def wire_g1_decode(b):
    """inverse, with arkworks' Validate::Yes checks (raises CozkError for bytes arkworks would reject)"""
    buf = (ctypes.c_uint8 * 64)(*bytes(b))
    xy = np.zeros(8, dtype=np.uint64)
    inf = ctypes.c_int()
    rc = L.lib().cozk_wire_g1_decode(buf, xy.ctypes.data, ctypes.byref(inf))
    if rc != L.OK:
        raise L.CozkError(rc, "wire_g1_decode: invalid point encoding")
    return point_from_abi(xy, inf.value)


class Context:
    """One per (party, GPU).  Not thread-safe (single-owner, like an IoContext fork)."""

    def __init__(self, device=0):
        self._l = L.lib()
        h = ctypes.c_void_p()
        rc = self._l.cozk_ctx_create(device, ctypes.byref(h))
        if rc != L.OK:
            if rc == L.ERR_NO_DEVICE:
                raise L.CozkError(rc, "no HIP device visible: the cozk engine has no CPU fallback")
            raise L.CozkError(rc, "cozk_ctx_create failed")
        self.h = h
        self.device = device

    def check(self, rc):
        if rc != L.OK:
            msg = self._l.cozk_last_error(self.h)
            raise L.CozkError(rc, msg.decode() if msg else "?")

    def synchronize(self):
        self.check(self._l.cozk_ctx_synchronize(self.h))

    def set_resident_rounds(self, enable):
        """True / False: force the resident round kernel of cozk_layer_prove_rounds on / off; None: the automatic
        default (on only while this is the one live context on its device in the process)"""
        self.check(self._l.cozk_ctx_set_resident_rounds(self.h, -1 if enable is None else (1 if enable else 0)))

    # ---- native Rep3 ring over RCCL (cozk_ring_*): one party per GPU / process
    @staticmethod
    def ring_unique_id():
        """128 opaque bytes for cozk_ring_init; ONE participant draws them, the host hands them to the others"""
        buf = (ctypes.c_uint8 * 128)()
        rc = L.lib().cozk_ring_unique_id(buf)
        if rc != L.OK:
            raise L.CozkError(rc, "cozk_ring_unique_id failed (librccl unavailable?)")
        return bytes(buf)

    def ring_init(self, ring_id, rank, nranks=3):
        self.check(self._l.cozk_ring_init(self.h, bytes(ring_id), rank, nranks))

    def ring_destroy(self):
        self.check(self._l.cozk_ring_destroy(self.h))

    def ring_info(self):
        r, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        self.check(self._l.cozk_ring_info(self.h, ctypes.byref(r), ctypes.byref(n), ctypes.byref(b)))
        return r.value, n.value, b.value

    def reshare(self, send):
        """send `send` to the next party, return what the previous party sent (cozk_reshare)"""
        recv = Vec.alloc(self, len(send), L.SCALAR_FR)
        self.check(self._l.cozk_reshare(self.h, send.h, recv.h))
        return recv

    def rep3_mul_vec(self, xa, xb, ya, yb, key_self, key_prev, counter=0):
        """rep3::arithmetic::mul_vec, whole (local product + mask + ring exchange) -> (c.a, c.b) vectors"""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self.check(self._l.cozk_rep3_mul_vec(self.h, xa.h, xb.h, ya.h, yb.h, L.prf_key(key_self), L.prf_key(key_prev), counter,
                                             ctypes.byref(a), ctypes.byref(b)))
        return Vec(self, a, L.SCALAR_FR), Vec(self, b, L.SCALAR_FR)

    def all_to_all(self, send, recv_lens=None):
        """every rank to every rank on the context's ring (cozk_ring_all_to_all): send[r] goes to rank r (None: nothing),
        the returned list holds what rank r sent here.  recv_lens[r] = the length expected from rank r (None: nothing);
        by default the pattern of `send` mirrored"""
        if recv_lens is None:
            recv_lens = [None if v is None else len(v) for v in send]
        recv = [None if n is None else Vec.alloc(self, n, L.SCALAR_FR) for n in recv_lens]
        ptrs = lambda vs: (ctypes.c_void_p * max(len(vs), 1))(*[None if v is None else v.h for v in vs])
        self.check(self._l.cozk_ring_all_to_all(self.h, ptrs(send), ptrs(recv)))
        return recv

    def shamir_mul_vec(self, a, b, keys, degree, counter=0):
        """this party's share of a x b as a degree-`degree` sharing again, one party per process over the context's ring
        (cozk_shamir_mul_vec): party = ring rank, parties = ring size; b and keys may be None on a party > 2 * degree"""
        h = ctypes.c_void_p()
        self.check(self._l.cozk_shamir_mul_vec(self.h, a.h, None if b is None else b.h, None if keys is None else _shamir_keys(keys),
                                               degree, counter, ctypes.byref(h)))
        return Vec(self, h, L.SCALAR_FR)

    def shamir_rand_vec(self, n, keys, degree, counter=0):
        """this party's halves of ranks - degree double-random pairs of n elements, one party per process over the context's
        ring (cozk_shamir_rand_vec): keys = its 3 * degree + 1 private PRF keys; returns the list of (r_t, r_2t)"""
        nr = ctypes.c_int(0)  # stays 0 without a ring: the call below then says so
        self._l.cozk_ring_info(self.h, None, ctypes.byref(nr), None)
        rt, r2t = (ctypes.c_void_p * 32)(), (ctypes.c_void_p * 32)()
        self.check(self._l.cozk_shamir_rand_vec(self.h, n, _shamir_keys(keys), degree, counter, rt, r2t))
        return [(Vec(self, ctypes.c_void_p(rt[k]), L.SCALAR_FR), Vec(self, ctypes.c_void_p(r2t[k]), L.SCALAR_FR)) for k in range(nr.value - degree)]

    def shamir_mul_king_vec(self, a, b, r_t, r_2t, degree, king=0):
        """this party's share of a x b as a degree-`degree` sharing again with a king and one double-random pair
        (cozk_shamir_mul_king_vec), one party per process over the context's ring; a, b and r_2t may be None on a party
        > 2 * degree.  The pair must not be used again"""
        h = ctypes.c_void_p()
        opt = lambda v: None if v is None else v.h
        self.check(self._l.cozk_shamir_mul_king_vec(self.h, opt(a), opt(b), opt(r_t), opt(r_2t), degree, king, ctypes.byref(h)))
        return Vec(self, h, L.SCALAR_FR)

    def close(self):
        if self.h:
            self._l.cozk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- profiling of the dominant kernel
    def prof_enable(self, on=True):
        self.check(self._l.cozk_prof_enable(self.h, 1 if on else 0))

    def prof_read(self):
        n = ctypes.c_uint64()
        ms = ctypes.c_double()
        adds = ctypes.c_uint64()
        nbytes = ctypes.c_uint64()
        self.check(self._l.cozk_prof_read(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(adds), ctypes.byref(nbytes)))
        return n.value, ms.value, adds.value, nbytes.value

    def bench_montmul(self, lanes, iters, variant=0):
        ms = ctypes.c_double()
        self.check(self._l.cozk_bench_montmul(self.h, lanes, iters, variant, ctypes.byref(ms)))
        return ms.value

    # ---- host G1 helpers
    def g1_sum(self, points):
        k = len(points)
        xy = np.zeros((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.int32)
        for i, p in enumerate(points):
            xy[i], inf[i] = point_to_abi(p)
        out = np.zeros(8, dtype=np.uint64)
        oi = ctypes.c_int()
        self.check(self._l.cozk_g1_sum(self.h, xy.ctypes.data, inf.ctypes.data, k, out.ctypes.data, ctypes.byref(oi)))
        return point_from_abi(out, oi.value)

    def g1_mul(self, point, scalar):
        xy, inf = point_to_abi(point)
        s = fr_to_mont_limbs([scalar])[0]
        out = np.zeros(8, dtype=np.uint64)
        oi = ctypes.c_int()
        self.check(self._l.cozk_g1_mul(self.h, xy.ctypes.data, inf, s.ctypes.data, out.ctypes.data, ctypes.byref(oi)))
        return point_from_abi(out, oi.value)


class Vec:
    """Device-resident scalar vector (`cozk_vec`)."""

    def __init__(self, ctx, handle, kind):
        self.ctx = ctx
        self.h = handle
        self.kind = kind

    @classmethod
    def alloc(cls, ctx, n, kind=L.SCALAR_FR):
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_vec_alloc(ctx.h, n, kind, ctypes.byref(h)))
        return cls(ctx, h, kind)

    @classmethod
    def from_ints(cls, ctx, values, kind=L.SCALAR_FR):
        """values: canonical ints (FR) or small integers (other kinds)"""
        if kind == L.SCALAR_FR:
            arr = fr_to_mont_limbs(values)
        else:
            arr = np.asarray(values, dtype=_KIND_DTYPE[kind])
        return cls.from_numpy(ctx, arr, kind)

    @classmethod
    def from_numpy(cls, ctx, arr, kind=L.SCALAR_FR):
        arr = np.ascontiguousarray(arr)
        n = arr.shape[0]
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_vec_upload(ctx.h, arr.ctypes.data if n else None, n, kind, ctypes.byref(h)))
        return cls(ctx, h, kind)

    @classmethod
    def random(cls, ctx, n, seed, kind=L.SCALAR_FR, max_bits=0):
        v = cls.alloc(ctx, n, kind)
        ctx.check(ctx._l.cozk_vec_fill_random(ctx.h, v.h, seed, max_bits))
        return v

    def __len__(self):
        return self.ctx._l.cozk_vec_len(self.h)

    def device_ptr(self):
        return self.ctx._l.cozk_vec_device_ptr(self.h)

    def to_numpy(self):
        n = len(self)
        if self.kind == L.SCALAR_FR:
            out = np.empty((n, 4), dtype=np.uint64)
        else:
            out = np.empty(n, dtype=_KIND_DTYPE[self.kind])
        self.ctx.check(self.ctx._l.cozk_vec_download(self.ctx.h, self.h, out.ctypes.data if n else None))
        return out

    def to_ints(self):
        a = self.to_numpy()
        if self.kind == L.SCALAR_FR:
            return mont_limbs_to_int(a)
        return [int(x) for x in a]

    def narrow(self, kind):
        """this FR vector as a U32 / U64 vector of the same values (cozk_vec_narrow: what msm_field_elements' dispatch on the scalars'
        bit length amounts to); raises CozkError if a value does not fit"""
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_vec_narrow(self.ctx.h, self.h, kind, ctypes.byref(h)))
        return Vec(self.ctx, h, kind)

    def rep3_share(self, key0, key1, party, counter=0):
        """Rep3 shares (a, b) of this secret vector for `party` (cozk_rep3_share_vec); key0 / key1 = 32-byte PRF keys"""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_rep3_share_vec(self.ctx.h, self.h, L.prf_key(key0), L.prf_key(key1), counter, party,
                                                       ctypes.byref(a), ctypes.byref(b)))
        return Vec(self.ctx, a, L.SCALAR_FR), Vec(self.ctx, b, L.SCALAR_FR)

    def rep3_scatter(self, key0, key1, party, party_ctx, counter=0):
        """the witness scatter device to device (cozk_rep3_scatter): this (dealer-side) secret vector's shares for `party`,
        as vectors owned by `party_ctx` (same or another GPU)"""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_rep3_scatter(self.ctx.h, self.h, L.prf_key(key0), L.prf_key(key1), counter, party_ctx.h, party,
                                                     ctypes.byref(a), ctypes.byref(b)))
        return Vec(party_ctx, a, L.SCALAR_FR), Vec(party_ctx, b, L.SCALAR_FR)

    @classmethod
    def prf(cls, ctx, n, key, counter=0):
        """out[i] = PRF(key, counter + i): the keyed ChaCha12 stream every share / mask is drawn from"""
        v = cls.alloc(ctx, n, L.SCALAR_FR)
        ctx.check(ctx._l.cozk_vec_fill_prf(ctx.h, v.h, L.prf_key(key), counter))
        return v

    def binop(self, op, other, base_field=False):
        out = Vec.alloc(self.ctx, len(self), L.SCALAR_FR)
        self.ctx.check(self.ctx._l.cozk_vec_binop(self.ctx.h, op, 1 if base_field else 0, self.h, other.h, out.h))
        return out

    def scale(self, s):
        """v[i] *= s in place (cozk_vec_scale): share x public; s = r - 1 negates"""
        sm = fr_to_mont_limbs([s])[0]
        self.ctx.check(self.ctx._l.cozk_vec_scale(self.ctx.h, self.h, sm.ctypes.data))
        return self

    def add_scalar(self, s):
        """v[i] += s in place (cozk_vec_add_scalar): share + public"""
        sm = fr_to_mont_limbs([s])[0]
        self.ctx.check(self.ctx._l.cozk_vec_add_scalar(self.ctx.h, self.h, sm.ctypes.data))
        return self

    # ---- Shamir sharing (mpc-types/src/protocols/shamir.rs): party p's share vector evaluates at x = p + 1
    def shamir_share(self, keys, degree, num_parties, counter=0):
        """the num_parties Shamir share vectors of this secret vector (cozk_shamir_share_vec); keys = `degree` 32-byte PRF
        keys, coefficient c of element i is PRF(keys[c - 1], counter + i)"""
        out = (ctypes.c_void_p * max(num_parties, 1))()
        self.ctx.check(self.ctx._l.cozk_shamir_share_vec(self.ctx.h, self.h, _shamir_keys(keys), degree, num_parties, counter, out))
        return [Vec(self.ctx, ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(num_parties)]

    def shamir_scatter(self, keys, degree, party_ctxs, counter=0):
        """shamir_share whose vector p is owned by party_ctxs[p] (same or another GPU): cozk_shamir_scatter"""
        n = len(party_ctxs)
        out = (ctypes.c_void_p * max(n, 1))()
        ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
        self.ctx.check(self.ctx._l.cozk_shamir_scatter(self.ctx.h, self.h, _shamir_keys(keys), degree, n, counter, ctxs, out))
        return [Vec(party_ctxs[p], ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(n)]

    def shamir_mul_deal(self, other, keys, degree, num_parties, counter=0):
        """a dealer's step of the multiplication with degree reduction (cozk_shamir_mul_deal): the num_parties share vectors
        of a fresh degree-`degree` sharing of self[i] * other[i], in one launch; keys = this party's `degree` private keys"""
        out = (ctypes.c_void_p * max(num_parties, 1))()
        self.ctx.check(self.ctx._l.cozk_shamir_mul_deal(self.ctx.h, self.h, other.h, _shamir_keys(keys), degree, num_parties, counter, out))
        return [Vec(self.ctx, ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(num_parties)]

    def shamir_mul_deal_pairs(self, keys, degree, num_parties, counter=0):
        """shamir_mul_deal of one interleaved GKR layer (cozk_shamir_mul_deal_pairs): the num_parties share vectors of a fresh
        degree-`degree` sharing of self[2 j] * self[2 j + 1], in one launch; the length must be even"""
        out = (ctypes.c_void_p * max(num_parties, 1))()
        self.ctx.check(self.ctx._l.cozk_shamir_mul_deal_pairs(self.ctx.h, self.h, _shamir_keys(keys), degree, num_parties, counter, out))
        return [Vec(self.ctx, ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(num_parties)]

    def shamir_mul_mask(self, other, r_2t):
        """self[i] * other[i] + r_2t[i] in one launch (cozk_shamir_mul_mask): what a party 0..2 * degree sends to the king"""
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_shamir_mul_mask(self.ctx.h, self.h, other.h, r_2t.h, ctypes.byref(h)))
        return Vec(self.ctx, h, L.SCALAR_FR)

    def shamir_mul_mask_pairs(self, r_2t, r_offset=0):
        """self[2 j] * self[2 j + 1] + r_2t[r_offset + j] in one launch (cozk_shamir_mul_mask_pairs): what a party 0..2 * degree
        sends to the king for one interleaved GKR layer; the half of the pair is addressed by an element offset"""
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_shamir_mul_mask_pairs(self.ctx.h, self.h, r_2t.h, r_offset, ctypes.byref(h)))
        return Vec(self.ctx, h, L.SCALAR_FR)

    def free(self):
        if self.h:
            self.ctx._l.cozk_vec_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _shamir_keys(keys):
    return b"".join(L.prf_key(k) for k in keys)


def _points(points):
    return np.ascontiguousarray(np.asarray(list(points), dtype=np.uint32))


def shamir_eval(ctx, coeffs, num_parties):
    """evaluate_poly at x = 1..=num_parties with the caller's coefficient vectors, coeffs[0] = the secret vector
    (cozk_shamir_eval_vec) -> num_parties share vectors"""
    k = len(coeffs)
    arr = (ctypes.c_void_p * max(k, 1))(*[v.h for v in coeffs])
    out = (ctypes.c_void_p * max(num_parties, 1))()
    ctx.check(ctx._l.cozk_shamir_eval_vec(ctx.h, arr, k - 1, num_parties, out))
    return [Vec(ctx, ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(num_parties)]


def shamir_lagrange(points):
    """lagrange_from_coeff (cozk_shamir_lagrange; host only, no context) -> canonical ints"""
    pts = _points(points)
    out = np.zeros((max(len(pts), 1), 4), dtype=np.uint64)
    rc = L.lib().cozk_shamir_lagrange(pts.ctypes.data if len(pts) else None, len(pts), out.ctypes.data)
    if rc != L.OK:
        raise L.CozkError(rc, "shamir_lagrange: 1..32 distinct points in 1..32")
    return mont_limbs_to_int(out[:len(pts)])


def shamir_combine(shares, points, degree):
    """combine_field_elements (cozk_shamir_combine_vec): opens the first degree + 1 of the share vectors at `points`"""
    ctx = shares[0].ctx
    pts = _points(points)
    arr = (ctypes.c_void_p * len(shares))(*[v.h for v in shares])
    h = ctypes.c_void_p()
    ctx.check(ctx._l.cozk_shamir_combine_vec(ctx.h, arr, pts.ctypes.data, len(shares), degree, ctypes.byref(h)))
    return Vec(ctx, h, L.SCALAR_FR)


def shamir_mul(party_ctxs, a_shares, b_shares, keys_per_party, degree, counter=0):
    """share x share -> a degree-`degree` sharing of the product, all parties in this process (cozk_shamir_mul_inproc):
    party p owns party_ctxs[p], a_shares[p], b_shares[p] and its `degree` keys keys_per_party[p]; for p > 2 * degree the
    three may be None.  Returns one vector per party, owned by that party's context"""
    n = len(party_ctxs)
    arr = lambda hs: (ctypes.c_void_p * max(n, 1))(*hs)
    ctxs = arr([c.h for c in party_ctxs])
    a = arr([None if v is None else v.h for v in a_shares])
    b = arr([None if v is None else v.h for v in b_shares])
    blocks, keys = _key_blocks(n, keys_per_party)
    out = (ctypes.c_void_p * max(n, 1))()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_mul_inproc(ctxs, a, b, keys, degree, n, counter, out))
    return [Vec(party_ctxs[p], ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(n)]


def _key_blocks(n, keys_per_party):
    """per-party key blocks for the in-process drivers: (the buffers, to be kept alive; the pointer table)"""
    blocks = [None if k is None else ctypes.create_string_buffer(_shamir_keys(k), max(32 * len(k), 1)) for k in keys_per_party]
    return blocks, (ctypes.c_void_p * max(n, 1))(*[None if k is None else ctypes.addressof(k) for k in blocks])


def shamir_mul_pairs(party_ctxs, layers, keys_per_party, degree, counter=0):
    """one tree level of a grand product, all parties in this process (cozk_shamir_mul_pairs_inproc): layers[p] = party p's share
    vector of an interleaved layer (even length 2m); returns per party its share vector of the m products layer[2 j] * layer[2 j + 1],
    a degree-`degree` sharing again.  layers[p] and keys_per_party[p] may be None for p > 2 * degree"""
    n = len(party_ctxs)
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    blocks, keys = _key_blocks(n, keys_per_party)
    out = (ctypes.c_void_p * max(n, 1))()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_mul_pairs_inproc(ctxs, _handles(n, layers), keys, degree, n, counter, out))
    return [Vec(party_ctxs[p], ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(n)]


class ShamirGpResult(ctypes.Structure):
    """cozk_shamir_gp_result"""
    _fields_ = [("verified", ctypes.c_int), ("n_layers", ctypes.c_int), ("proof_len", ctypes.c_uint64), ("n_opened", ctypes.c_uint64),
                ("t_construct_ms", ctypes.c_double), ("t_prove_ms", ctypes.c_double)]


class ShamirGpStats(ctypes.Structure):
    """cozk_shamir_gp_stats: how the rounds ran -- calls of cozk_layer_group_round / _final against per-sender cozk_layer_round
    and per-opener final claims"""
    _fields_ = [("group_rounds", ctypes.c_uint64), ("single_rounds", ctypes.c_uint64), ("group_finals", ctypes.c_uint64),
                ("single_finals", ctypes.c_uint64)]


class ShamirGpToggleStats(ctypes.Structure):
    """cozk_shamir_gp_toggle_stats: how the toggle layer's rounds ran -- calls of cozk_toggle_group_round against per-sender
    cozk_toggle_round"""
    _fields_ = [("toggle_group_rounds", ctypes.c_uint64), ("toggle_single_rounds", ctypes.c_uint64)]


SHAMIR_MAX_PARTIES = 32  # COZK_SHAMIR_MAX_PARTIES


class ShamirHarnessHandle(L.HarnessHandle):
    """What the in-process Shamir prover harnesses share (csrc/host/shamir_harness.hpp): the read-back of what went over the star --
    `PREFIX_msgs`, `_finals`, their `_len`, `_get_stats` -- and the device list of a config.  A subclass sets PREFIX, CONFIG, RESULT."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        cls.EXTRA = {cls.PREFIX + "_msgs_len": (sz, [vp]), cls.PREFIX + "_msgs": (i, [vp, vp, sz]), cls.PREFIX + "_finals_len": (sz, [vp]),
                     cls.PREFIX + "_finals": (i, [vp, vp, sz]), cls.PREFIX + "_get_stats": (i, [vp, ctypes.POINTER(ShamirGpStats)])}

    @staticmethod
    def _devices(devices):
        """one device per party (an int: all on it), padded with device 0 to the config's array"""
        devs = [devices] * SHAMIR_MAX_PARTIES if isinstance(devices, int) else list(devices) + [0] * (SHAMIR_MAX_PARTIES - len(devices))
        return (ctypes.c_int * SHAMIR_MAX_PARTIES)(*devs[:SHAMIR_MAX_PARTIES])

    def _fe_list(self, what):
        n = self._f("_" + what + "_len")(self.h)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        rc = self._f("_" + what)(self.h, out.ctypes.data, n)
        if rc != L.OK:
            raise L.CozkError(rc, what)
        return mont_limbs_to_int(out[:n])

    def _rows(self, what, k):
        v = self._fe_list(what)
        return [v[i:i + k] for i in range(0, len(v), k)]

    def msgs(self):
        """the masked messages of the degree-2t openings, [m][p <= 2t]"""
        return self._rows("msgs", 2 * self.cfg.degree + 1)

    def finals(self):
        """the shares of the degree-t openings, [value][p <= t], in the order opened"""
        return self._rows("finals", self.cfg.degree + 1)

    def stats(self):
        st = ShamirGpStats()
        rc = self._f("_get_stats")(self.h, ctypes.byref(st))
        if rc != L.OK:
            raise L.CozkError(rc, "get_stats")
        return st


class ShamirGpProof:
    """what shamir_gp_prove returns: .proof_bytes, the final .claim and point .r (canonical ints), .result (ShamirGpResult), and
    what went over the star -- .msgs[m][p], sender p's masked message of opening m, and .finals[layer, top first][p] = (L, R),
    opener p's final-claim shares"""

    def __init__(self, l, h, degree):
        res = ShamirGpResult()
        def ok(rc):
            if rc != L.OK:
                raise L.CozkError(rc, "shamir_gp accessor")

        ok(l.cozk_shamir_gp_get_result(h, ctypes.byref(res)))
        self.result = res
        self._stats = ShamirGpStats()
        ok(l.cozk_shamir_gp_get_stats(h, ctypes.byref(self._stats)))
        buf = (ctypes.c_uint8 * max(int(res.proof_len), 1))()
        ok(l.cozk_shamir_gp_proof_bytes(h, buf, int(res.proof_len)))
        self.proof_bytes = bytes(buf)[:int(res.proof_len)]
        nr = l.cozk_shamir_gp_point_len(h)
        claim, r = np.zeros(4, dtype=np.uint64), np.zeros((max(nr, 1), 4), dtype=np.uint64)
        ok(l.cozk_shamir_gp_final(h, claim.ctypes.data, r.ctypes.data))
        self.claim, self.r = mont_limbs_to_int(claim)[0], mont_limbs_to_int(r[:nr])

        def table(length, get):
            k = length(h)
            raw = np.zeros((max(k, 1), 4), dtype=np.uint64)
            ok(get(h, raw.ctypes.data, k))
            return mont_limbs_to_int(raw[:k])

        s = 2 * degree + 1
        flat = table(l.cozk_shamir_gp_msgs_len, l.cozk_shamir_gp_msgs)
        self.msgs = [flat[i:i + s] for i in range(0, len(flat), s)]
        flat = table(l.cozk_shamir_gp_finals_len, l.cozk_shamir_gp_finals)
        pairs = [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]
        self.finals = [pairs[i:i + degree + 1] for i in range(0, len(pairs), degree + 1)]
        # a toggled proof: the toggle layer's (flag, fingerprint) claims; None for a dense proof
        self._toggle_stats = ShamirGpToggleStats()
        ok(l.cozk_shamir_gp_get_toggle_stats(h, ctypes.byref(self._toggle_stats)))
        fl, fp = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        self.toggle_claims = None
        if l.cozk_shamir_gp_toggle_claims(h, fl.ctypes.data, fp.ctypes.data) == L.OK:
            self.toggle_claims = (mont_limbs_to_int(fl.reshape(1, 4))[0], mont_limbs_to_int(fp.reshape(1, 4))[0])


    @property
    def stats(self):
        """ShamirGpStats of the proof (cozk_shamir_gp_get_stats)"""
        return self._stats


    @property
    def toggle_stats(self):
        """ShamirGpToggleStats of the proof (cozk_shamir_gp_get_toggle_stats); all zero for a dense proof"""
        return self._toggle_stats


def shamir_gp_prove(party_ctxs, leaves, batch_size, mul_keys, rand_keys, degree, mul_counter=0, rand_counter=0, label=b"cozk", verify=True):
    """the dense batched grand product proved by len(party_ctxs) Shamir parties in this process (cozk_shamir_gp_prove_inproc):
    leaves[p] = party p's share vector of the interleaved leaves (not modified), mul_keys[p] = its `degree` keys of the tree's
    multiplications, rand_keys[p] = its 3 * degree + 1 keys of the opening masks.  The proof is the plain prover's, byte for byte.
    (rand_keys, rand_counter) and (mul_keys, mul_counter) ranges must never be used again.  Returns a ShamirGpProof"""
    n = len(party_ctxs)
    l = party_ctxs[0]._l
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    mb, mk = _key_blocks(n, mul_keys)
    rb, rk = _key_blocks(n, rand_keys)
    h = ctypes.c_void_p()
    party_ctxs[0].check(l.cozk_shamir_gp_prove_inproc(ctxs, _handles(n, leaves), batch_size, mk, rk, degree, n, mul_counter, rand_counter,
                                                      bytes(label), 1 if verify else 0, ctypes.byref(h)))
    try:
        return ShamirGpProof(l, h, degree)
    finally:
        l.cozk_shamir_gp_free(h)


def _handles(n, vs):
    return (ctypes.c_void_p * max(n, 1))(*[None if v is None else v.h for v in vs])


def shamir_rand_deal(ctx, n, keys, degree, num_parties, counter=0):
    """one party's dealing of the double-random preprocessing (cozk_shamir_rand_deal): a PRF secret vector of n elements dealt
    with degree `degree` and with 2 * degree; keys = 3 * degree + 1 PRF keys.  Returns (out_t, out_2t), num_parties vectors each"""
    ot, o2 = (ctypes.c_void_p * max(num_parties, 1))(), (ctypes.c_void_p * max(num_parties, 1))()
    ctx.check(ctx._l.cozk_shamir_rand_deal(ctx.h, n, _shamir_keys(keys), degree, num_parties, counter, ot, o2))
    wrap = lambda t: [Vec(ctx, ctypes.c_void_p(t[p]), L.SCALAR_FR) for p in range(num_parties)]
    return wrap(ot), wrap(o2)


def shamir_rand_extract(ctx, recv, count):
    """out[k] = sum_j (j + 1)^k recv[j], k < count (cozk_shamir_rand_extract): the Vandermonde step on the vectors one party
    received; privacy needs count <= parties - degree"""
    out = (ctypes.c_void_p * max(count, 1))()
    ctx.check(ctx._l.cozk_shamir_rand_extract(ctx.h, _handles(len(recv), recv), len(recv), count, out))
    return [Vec(ctx, ctypes.c_void_p(out[k]), L.SCALAR_FR) for k in range(count)]


def shamir_rand(party_ctxs, keys_per_party, n, degree, counter=0):
    """the double-random preprocessing with all parties in this process (cozk_shamir_rand_inproc): keys_per_party[p] = party p's
    3 * degree + 1 keys.  Returns per party the list of its parties - degree pairs (r_t, r_2t), owned by that party's context"""
    np_ = len(party_ctxs)
    cnt = np_ - degree
    ctxs = (ctypes.c_void_p * max(np_, 1))(*[c.h for c in party_ctxs])
    blocks, keys = _key_blocks(np_, keys_per_party)
    rt, r2t = (ctypes.c_void_p * max(np_ * cnt, 1))(), (ctypes.c_void_p * max(np_ * cnt, 1))()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_rand_inproc(ctxs, keys, n, degree, np_, counter, rt, r2t))
    vec = lambda t, q, k: Vec(party_ctxs[q], ctypes.c_void_p(t[q * cnt + k]), L.SCALAR_FR)
    return [[(vec(rt, q, k), vec(r2t, q, k)) for k in range(cnt)] for q in range(np_)]


def shamir_mul_king(party_ctxs, a_shares, b_shares, r_t, r_2t, degree, king=0):
    """share x share -> a degree-`degree` sharing of the product with a king and ONE double-random pair, all parties in this
    process (cozk_shamir_mul_king_inproc): r_t[p], r_2t[p] = party p's halves of the pair; a_shares[p], b_shares[p], r_2t[p]
    may be None for p > 2 * degree.  The pair must not be used again.  Returns one vector per party"""
    n = len(party_ctxs)
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    out = (ctypes.c_void_p * max(n, 1))()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_mul_king_inproc(ctxs, _handles(n, a_shares), _handles(n, b_shares), _handles(n, r_t),
                                                                    _handles(n, r_2t), degree, n, king, out))
    return [Vec(party_ctxs[p], ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(n)]


def shamir_king_finish(ctx, masked, degree, r_t, r_offset=0, want_z=False):
    """the king's open and len(r_t) parties' unmask in one launch (cozk_shamir_king_finish): z = the degree-2t opening of the
    2 * degree + 1 masked vectors, out[q][i] = z[i] - r_t[q][r_offset + i].  Returns the list out, or (out, z) with want_z"""
    count = len(r_t)
    out = (ctypes.c_void_p * max(count, 1))()
    z = ctypes.c_void_p()
    ctx.check(ctx._l.cozk_shamir_king_finish(ctx.h, _handles(len(masked), masked), degree, _handles(count, r_t), r_offset, count, out,
                                             ctypes.byref(z) if want_z else None))
    vecs = [Vec(ctx, ctypes.c_void_p(out[q]), L.SCALAR_FR) for q in range(count)]
    return (vecs, Vec(ctx, z, L.SCALAR_FR)) if want_z else vecs


def shamir_mul_king_pairs(party_ctxs, layers, r_t, r_2t, degree, r_offset=0, king=0):
    """one tree level of a grand product with a king, all parties in this process (cozk_shamir_mul_king_pairs_inproc): layers[p] =
    party p's share vector of an interleaved layer (even length 2m); product j consumes element r_offset + j of the pair
    (r_t[p], r_2t[p]).  layers[p] and r_2t[p] may be None for p > 2 * degree.  No element of a pair may be used twice"""
    n = len(party_ctxs)
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    out = (ctypes.c_void_p * max(n, 1))()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_mul_king_pairs_inproc(ctxs, _handles(n, layers), _handles(n, r_t), _handles(n, r_2t), r_offset,
                                                                          degree, n, king, out))
    return [Vec(party_ctxs[p], ctypes.c_void_p(out[p]), L.SCALAR_FR) for p in range(n)]


class ShamirGpPrepResult(ctypes.Structure):
    """cozk_shamir_gp_prep_result"""
    _fields_ = [("n_openings", ctypes.c_uint64), ("pair_elems", ctypes.c_uint64), ("pairs_held", ctypes.c_int), ("used", ctypes.c_int),
                ("t_offline_ms", ctypes.c_double)]


class ShamirGpPrep:
    """the preprocessing of ONE king grand product (cozk_shamir_gp_prep_inproc), made before the leaves exist; .result is a
    ShamirGpPrepResult.  close() it before its party contexts"""

    def __init__(self, party_ctxs, h, degree):
        self.party_ctxs, self.h, self.degree = list(party_ctxs), h, degree

    @property
    def result(self):
        res = ShamirGpPrepResult()
        rc = self.party_ctxs[0]._l.cozk_shamir_gp_prep_get_result(self.h, ctypes.byref(res))
        if rc != L.OK:
            raise L.CozkError(rc, "shamir_gp_prep accessor")
        return res

    def close(self):
        if getattr(self, "h", None):
            self.party_ctxs[0]._l.cozk_shamir_gp_prep_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shamir_gp_prep(party_ctxs, rand_keys, n_leaves, batch_size, degree, rand_counter=0):
    """everything a king grand product of n_leaves interleaved leaves in batch_size circuits needs before the leaves exist
    (cozk_shamir_gp_prep_inproc): the opening masks and the double-random pairs of the tree.  rand_keys[p] = party p's
    3 * degree + 1 keys; (rand_keys, rand_counter .. + M + n_leaves / 2) must never be used again.  Returns a ShamirGpPrep"""
    n = len(party_ctxs)
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    rb, rk = _key_blocks(n, rand_keys)
    h = ctypes.c_void_p()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_gp_prep_inproc(ctxs, rk, n_leaves, batch_size, degree, n, rand_counter, ctypes.byref(h)))
    return ShamirGpPrep(party_ctxs, h, degree)


def shamir_gp_prove_king(party_ctxs, leaves, batch_size, prep, king=0, label=b"cozk", verify=True):
    """shamir_gp_prove with the king construct, consuming the ShamirGpPrep `prep` (cozk_shamir_gp_prove_king_inproc): no fresh
    randomness online.  The proof is the plain prover's, byte for byte; a prep serves one proof.  Returns a ShamirGpProof"""
    n = len(party_ctxs)
    l = party_ctxs[0]._l
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    h = ctypes.c_void_p()
    party_ctxs[0].check(l.cozk_shamir_gp_prove_king_inproc(ctxs, _handles(n, leaves), batch_size, prep.h, king, bytes(label), 1 if verify else 0,
                                                           ctypes.byref(h)))
    try:
        return ShamirGpProof(l, h, prep.degree)
    finally:
        l.cozk_shamir_gp_free(h)


def shamir_tgp_prove(party_ctxs, flags, fingerprints, mul_keys, rand_keys, degree, mul_counter=0, rand_counter=0, label=b"cozk", verify=True):
    """the toggled batched grand product proved by len(party_ctxs) Shamir parties in this process (cozk_shamir_tgp_prove_inproc):
    flags = one public 0/1 U8 Vec of N entries per pair of circuits, vectors of party_ctxs[0]; fingerprints[p] = party p's share
    vector of the 2 * len(flags) * N fingerprints (not modified; may be None for p > 2 * degree); keys and counters as for
    shamir_gp_prove.  The proof is the plain toggled prover's, byte for byte.  Returns a ShamirGpProof with .toggle_claims"""
    n = len(party_ctxs)
    l = party_ctxs[0]._l
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    mb, mk = _key_blocks(n, mul_keys)
    rb, rk = _key_blocks(n, rand_keys)
    h = ctypes.c_void_p()
    party_ctxs[0].check(l.cozk_shamir_tgp_prove_inproc(ctxs, _handles(len(flags), flags), len(flags), _handles(n, fingerprints), mk, rk, degree, n,
                                                       mul_counter, rand_counter, bytes(label), 1 if verify else 0, ctypes.byref(h)))
    try:
        return ShamirGpProof(l, h, degree)
    finally:
        l.cozk_shamir_gp_free(h)


def shamir_tgp_prep(party_ctxs, rand_keys, n_pairs, n_per, degree, rand_counter=0):
    """shamir_gp_prep for a toggled grand product of n_pairs flag columns of n_per entries (cozk_shamir_tgp_prep_inproc): the masks
    of the dense tree and of the toggle layer's rounds, the construct pairs behind them.  Serves shamir_tgp_prove_king only"""
    n = len(party_ctxs)
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    rb, rk = _key_blocks(n, rand_keys)
    h = ctypes.c_void_p()
    party_ctxs[0].check(party_ctxs[0]._l.cozk_shamir_tgp_prep_inproc(ctxs, rk, n_pairs, n_per, degree, n, rand_counter, ctypes.byref(h)))
    return ShamirGpPrep(party_ctxs, h, degree)


def shamir_tgp_prove_king(party_ctxs, flags, fingerprints, prep, king=0, label=b"cozk", verify=True):
    """shamir_tgp_prove with the king construct, consuming the toggled ShamirGpPrep `prep` (cozk_shamir_tgp_prove_king_inproc)"""
    n = len(party_ctxs)
    l = party_ctxs[0]._l
    ctxs = (ctypes.c_void_p * max(n, 1))(*[c.h for c in party_ctxs])
    h = ctypes.c_void_p()
    party_ctxs[0].check(l.cozk_shamir_tgp_prove_king_inproc(ctxs, _handles(len(flags), flags), len(flags), _handles(n, fingerprints), prep.h, king,
                                                            bytes(label), 1 if verify else 0, ctypes.byref(h)))
    try:
        return ShamirGpProof(l, h, prep.degree)
    finally:
        l.cozk_shamir_gp_free(h)


def shamir_combine_points(ctx, points_g1, points, degree):
    """combine_curve_point (cozk_shamir_combine_points): opens the parties' commitments; points_g1 = affine points or None"""
    k = len(points_g1)
    xy = np.zeros((max(k, 1), 8), dtype=np.uint64)
    inf = np.zeros(max(k, 1), dtype=np.int32)
    for i, p in enumerate(points_g1):
        xy[i], inf[i] = point_to_abi(p)
    pts = _points(points)
    out = np.zeros(8, dtype=np.uint64)
    oi = ctypes.c_int()
    ctx.check(ctx._l.cozk_shamir_combine_points(ctx.h, xy.ctypes.data, inf.ctypes.data, pts.ctypes.data, k, degree, out.ctypes.data,
                                                ctypes.byref(oi)))
    return point_from_abi(out, oi.value)


class Bases:
    """Device-resident SRS slice (`ck.powers_of_g[i]`), optionally with the 16-window table."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    @classmethod
    def upload(cls, ctx, points, precompute=True):
        n = len(points)
        xy = np.zeros((n, 8), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        for i, p in enumerate(points):
            xy[i], inf[i] = point_to_abi(p)
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_bases_upload(ctx.h, xy.ctypes.data, inf.ctypes.data, n, 1 if precompute else 0,
                                           ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_scalars(cls, ctx, scalars_vec, g=(1, 2), precompute=True):
        """bases[i] = scalars[i] * g, computed on the GPU (`MultilinearPC::setup`)"""
        gxy, _ = point_to_abi(g)
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_bases_from_scalars(ctx.h, scalars_vec.h, gxy.ctypes.data, 1 if precompute else 0,
                                                 ctypes.byref(h)))
        return cls(ctx, h)

    def pair_sums(self, precompute=True):
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._l.cozk_bases_pair_sums(self.ctx.h, self.h, 1 if precompute else 0, ctypes.byref(h)))
        return Bases(self.ctx, h)

    def __len__(self):
        return self.ctx._l.cozk_bases_len(self.h)

    def download(self, offset=0, n=None):
        if n is None:
            n = len(self) - offset
        xy = np.zeros((n, 8), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        self.ctx.check(self.ctx._l.cozk_bases_download(self.ctx.h, self.h, offset, n, xy.ctypes.data, inf.ctypes.data))
        return [point_from_abi(xy[i], inf[i]) for i in range(n)]

    # ---- VariableBaseMSM
    def msm(self, scalars, offset=0):
        """scalars: Vec (device resident) -> affine point or None"""
        out = np.zeros(8, dtype=np.uint64)
        oi = ctypes.c_int()
        self.ctx.check(self.ctx._l.cozk_msm_vec(self.ctx.h, self.h, offset, scalars.h, out.ctypes.data, ctypes.byref(oi)))
        return point_from_abi(out, oi.value)

    def msm_host(self, arr, kind=L.SCALAR_FR, offset=0):
        """host scalars (numpy) -> affine point; PCIe-inclusive form of the seam"""
        arr = np.ascontiguousarray(arr)
        n = arr.shape[0]
        out = np.zeros(8, dtype=np.uint64)
        oi = ctypes.c_int()
        self.ctx.check(self.ctx._l.cozk_msm(self.ctx.h, self.h, offset, arr.ctypes.data if n else None, kind, n,
                                            out.ctypes.data, ctypes.byref(oi)))
        return point_from_abi(out, oi.value)

    def batch_msm_raw(self, vecs, offset=0):
        """k device vectors -> (uint64[k,8], int32[k]) without int conversion (bench path)"""
        k = len(vecs)
        arr = (ctypes.c_void_p * k)(*[v.h for v in vecs])
        out = np.zeros((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.int32)
        self.ctx.check(self.ctx._l.cozk_batch_msm_vec(self.ctx.h, self.h, offset, arr, k, out.ctypes.data,
                                                      inf.ctypes.data))
        return out, inf

    def batch_msm(self, vecs, offset=0):
        out, inf = self.batch_msm_raw(vecs, offset)
        return [point_from_abi(out[i], inf[i]) for i in range(len(vecs))]

    def free(self):
        if self.h:
            self.ctx._l.cozk_bases_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
