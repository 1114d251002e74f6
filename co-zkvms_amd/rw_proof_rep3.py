"""The read-write memory check by three Rep3 parties (Rep3ReadWriteMemoryProver, co-jolt/src/jolt/vm/read_write_memory/worker.rs:
196-344): the leaves of its grand-product circuits from public compact address and timestamp columns and value polynomials, plain or
Rep3 shares (`rw_memory_shared_leaves`, `rw_memory_shared_init_final_leaves`), and the proof itself as a three-party in-process harness
over the consistent witness of `RwProof` (`RwProofRep3`), whose bytes are the plain proof's."""
import ctypes

from . import _lib as L
from .engine import fr_to_mont_limbs

RW_PROOF_REP3_SYMBOLS = ["cozk_rw_memory_shared_leaves", "cozk_rw_memory_shared_init_final_leaves", "cozk_rw_proof_rep3_create", "cozk_rw_proof_rep3_error",
                         "cozk_rw_proof_rep3_destroy", "cozk_rw_proof_rep3_prove", "cozk_rw_proof_rep3_proof_bytes"]
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_rw_memory_shared_leaves.restype = _i
    l.cozk_rw_memory_shared_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _i, _i, _vp, _vp, _sz]
    l.cozk_rw_memory_shared_init_final_leaves.restype = _i
    l.cozk_rw_memory_shared_init_final_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz]
    return l


def _handles(items):
    return (_vp * max(1, len(items)))(*[None if v is None else v.h for v in items])


def _mode(mode):
    return L.MODE_PLAIN if mode == "plain" else L.MODE_REP3 if mode == "rep3" else mode


def rw_memory_shared_leaves(ctx, addr, v_read, t_read, v_written, gamma, tau, mode, party_id, out_a, out_b=None, offset=0):
    """The 2 n_slots read / write circuits of the memory check, circuit-major from `offset` (include/cozk.h has the layout), with the
    values as polynomials: addr[s] a U8 or U32 Vec, t_read[s] a U32 Vec, all of one length n; v_read[s] a polynomial of at least n
    entries, plain or Rep3; v_written a list with a polynomial or None per slot (None: the slot only reads; v_written=None: no slot
    writes); gamma and tau canonical ints; mode "plain" (out_a takes the leaves) or "rep3" (out_a, out_b take the two components of
    party_id's shares; a plain polynomial is a public one).  Asynchronous on the context's stream.  An inconsistent argument raises
    CozkError."""
    l = _decl()
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    vw = None if v_written is None else _handles(v_written)
    ctx.check(l.cozk_rw_memory_shared_leaves(ctx.h, _handles(addr), _handles(v_read), _handles(t_read), vw, len(addr), g.ctypes.data, t.ctypes.data, _mode(mode),
                                             party_id, out_a.h, None if out_b is None else out_b.h, offset))


def rw_memory_shared_init_final_leaves(ctx, v_init, v_final, t_final, gamma, tau, mode, party_id, out_a, out_b=None, offset=0):
    """out[offset + a] = h(a, v_init[a], 0) and out[offset + MEM + a] = h(a, v_final[a], t_final[a]) from the U32 Vec t_final of MEM
    entries and two polynomials of at least MEM entries, plain or Rep3; the conventions of `rw_memory_shared_leaves`."""
    l = _decl()
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    ctx.check(l.cozk_rw_memory_shared_init_final_leaves(ctx.h, v_init.h, v_final.h, t_final.h, g.ctypes.data, t.ctypes.data, _mode(mode), party_id, out_a.h,
                                                        None if out_b is None else out_b.h, offset))


class RwProofRep3Config(ctypes.Structure):
    _fields_ = [("devices", ctypes.c_int * 3), ("log_n", ctypes.c_int), ("log_mem", ctypes.c_int), ("n_slots", ctypes.c_int), ("seed", ctypes.c_uint64),
                ("precompute", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int)]


class RwProofRep3Result(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_share_ms", ctypes.c_double),
                ("t_commit_ms", ctypes.c_double), ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double),
                ("ring_bytes", ctypes.c_uint64), ("proof_len", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32)]


class RwProofRep3(L.HarnessHandle):
    """The read-write memory proof by three Rep3 parties as an in-process harness (`cozk_rw_proof_rep3_*`,
    csrc/host/rw_memory_proof_rep3.hpp): the instance of `RwProof(seed, with_ts=False)`, its secret columns v_read, v_written and
    v_final shared at create, then prove() = commit, the leaves in REP3, the two grand products, two openings that join public compact
    columns with shared polynomials, one reduce_and_prove, and `RwProof`'s verifier.  The proof bytes are `RwProof`'s.  tamper: 1 bumps a
    v_read before the sharing (the multiset check rejects), 2 makes party 0 send a wrong claim share (the leaf check rejects);
    leaves_fused=False makes the leaves by the composition of fingerprint_leaves (the same proof bytes)."""
    PREFIX, CONFIG, RESULT = "cozk_rw_proof_rep3", RwProofRep3Config, RwProofRep3Result

    def __init__(self, log_n=10, log_mem=10, n_slots=4, seed=1, devices=(0, 0, 0), precompute=True, leaves_fused=True, tamper=0):
        cfg = RwProofRep3Config()
        cfg.devices = (ctypes.c_int * 3)(*devices)
        cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.seed = log_n, log_mem, n_slots, seed
        cfg.precompute, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), int(leaves_fused), tamper
        self._open(cfg)
