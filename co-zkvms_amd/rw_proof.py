"""The read-write memory proof over the consistent witness of `rw_memory_witness` (the dealer's side of Jolt's ReadWriteMemoryProof):
the leaves of its grand-product circuits from the compact columns (`rw_memory_leaves`, `rw_memory_init_final_leaves`) and the proof
itself as an in-process harness (`RwProof`), with the timestamp range check of `ts_proof` chained behind the memory check under one
transcript and one opening accumulator."""
import ctypes

from . import _lib as L
from .engine import fr_to_mont_limbs

RW_PROOF_SYMBOLS = ["cozk_rw_memory_leaves", "cozk_rw_memory_init_final_leaves", "cozk_rw_proof_create", "cozk_rw_proof_error", "cozk_rw_proof_destroy",
                    "cozk_rw_proof_prove", "cozk_rw_proof_proof_bytes"]
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_rw_memory_leaves.restype = _i
    l.cozk_rw_memory_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz]
    l.cozk_rw_memory_init_final_leaves.restype = _i
    l.cozk_rw_memory_init_final_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]
    return l


def _handles(vecs):
    return (_vp * max(1, len(vecs)))(*[None if v is None else v.h for v in vecs])


def rw_memory_leaves(ctx, addr, v_read, t_read, v_written, gamma, tau, out, offset=0):
    """The 2 n_slots read / write circuits of the memory check into the FR Vec `out` from `offset`, circuit-major (include/cozk.h has the
    layout): addr[s] a U8 or U32 Vec, v_read[s] / t_read[s] U32 Vecs, v_written a list with a U32 Vec or None per slot (None: the slot
    only reads; v_written=None: no slot writes), all of one length n; gamma and tau canonical ints.  Asynchronous on the context's
    stream.  An inconsistent argument raises CozkError."""
    l = _decl()
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    vw = None if v_written is None else _handles(v_written)
    ctx.check(l.cozk_rw_memory_leaves(ctx.h, _handles(addr), _handles(v_read), _handles(t_read), vw, len(addr), g.ctypes.data, t.ctypes.data, out.h, offset))


def rw_memory_init_final_leaves(ctx, v_init, v_final, t_final, gamma, tau, out, offset=0):
    """out[offset + a] = h(a, v_init[a], 0), out[offset + MEM + a] = h(a, v_final[a], t_final[a]) from three U32 Vecs of MEM entries;
    the conventions of `rw_memory_leaves`."""
    l = _decl()
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    ctx.check(l.cozk_rw_memory_init_final_leaves(ctx.h, v_init.h, v_final.h, t_final.h, g.ctypes.data, t.ctypes.data, out.h, offset))


class RwProofConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("device", ctypes.c_int), ("log_n", ctypes.c_int), ("log_mem", ctypes.c_int), ("n_slots", ctypes.c_int),
                ("seed", ctypes.c_uint64), ("precompute", ctypes.c_int), ("with_ts", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int)]


class RwProofResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_commit_ms", ctypes.c_double),
                ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_ts_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double),
                ("proof_len", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32)]


class RwProof(L.HarnessHandle):
    """The read-write memory proof as an in-process harness (`cozk_rw_proof_*`, csrc/host/rw_memory_proof.hpp): a Jolt-shaped trace from
    `seed` over the first n_slots of rs1, rs2, rd, ram, the witness walks on the device, then prove() = commit of the compact columns,
    the two grand products of the memory check, two openings from compact columns, with with_ts the timestamp range check under the same
    transcript (t_read committed once), one reduce_and_prove, and the plain verifier.  PLAIN only.  tamper: 1 bumps a v_read (the
    multiset check rejects), 2 sends a wrong claim (the leaf check rejects), 3 bumps a final counter of the range check ("timestamp:
    multiset equality"); leaves_fused=False makes the leaves by the composition of fingerprint_leaves (the same proof bytes)."""
    PREFIX, CONFIG, RESULT = "cozk_rw_proof", RwProofConfig, RwProofResult

    def __init__(self, log_n=10, log_mem=10, n_slots=4, seed=1, device=0, precompute=True, with_ts=True, leaves_fused=True, tamper=0, mode="plain"):
        cfg = RwProofConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.device, cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.seed = device, log_n, log_mem, n_slots, seed
        cfg.precompute, cfg.with_ts, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), (1 if with_ts else 0), (1 if leaves_fused else 0), tamper
        self._open(cfg)
