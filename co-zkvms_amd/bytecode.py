"""The bytecode memory check on the device (Rep3BytecodeProver, co-jolt/src/jolt/vm/bytecode/worker.rs:43-142): a consistent witness
over the six public table columns (`bytecode_witness`: the gathers v_read / v_imm and the counters t_read / t_final) and the leaves of
its four grand-product circuits from seven compact public columns plus the one field column imm (`bytecode_leaves`,
`bytecode_init_final_leaves`), in PLAIN and REP3, and the proof itself as an in-process harness (`BytecodeProof`)."""
import ctypes

from . import _lib as L
from .engine import Vec, fr_to_mont_limbs

BYTECODE_SYMBOLS = ["cozk_bytecode_witness", "cozk_bytecode_leaves", "cozk_bytecode_init_final_leaves", "cozk_bytecode_proof_create",
                    "cozk_bytecode_proof_error", "cozk_bytecode_proof_destroy", "cozk_bytecode_proof_prove", "cozk_bytecode_proof_proof_bytes"]
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_bytecode_witness.restype = _i
    l.cozk_bytecode_witness.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
    l.cozk_bytecode_leaves.restype = _i
    l.cozk_bytecode_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz]
    l.cozk_bytecode_init_final_leaves.restype = _i
    l.cozk_bytecode_init_final_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz]
    return l


def _handles(vecs):
    return (_vp * max(1, len(vecs)))(*[None if v is None else v.h for v in vecs])


def _mode(mode):
    return L.MODE_PLAIN if mode == "plain" else L.MODE_REP3 if mode == "rep3" else mode


def bytecode_witness(ctx, a, table):
    """a: a U32 Vec of n rows read, one per step; table: the six columns of B rows (address U32 or U64, bitflags U64, rd, rs1, rs2 U8,
    imm I64).  Returns (v_read, v_imm, t_read, t_final): v_read a list of five Vecs, v_read[k][j] = table[k][a[j]] in the column's own
    kind; v_imm an FR Vec, from_i64(table[5][a[j]]); t_read a U32 Vec, the number of earlier steps at the same row; t_final a U32 Vec of
    B entries, the number of steps at each row.  a[j] >= B or an inconsistent argument raises CozkError (COZK_ERR_INVALID_ARG) and
    returns nothing."""
    l = _decl()
    if len(table) != 6:
        raise ValueError("bytecode_witness: six table columns")
    v_read, v_imm, t_read, t_final = (_vp * 5)(), _vp(), _vp(), _vp()
    ctx.check(l.cozk_bytecode_witness(ctx.h, a.h, _handles(table), v_read, ctypes.byref(v_imm), ctypes.byref(t_read), ctypes.byref(t_final)))
    return ([Vec(ctx, _vp(v_read[k]), table[k].kind) for k in range(5)], Vec(ctx, v_imm, L.SCALAR_FR), Vec(ctx, t_read, L.SCALAR_U32),
            Vec(ctx, t_final, L.SCALAR_U32))


def bytecode_leaves(ctx, a, v, t_read, imm, gamma, tau, mode, party_id, out_a, out_b=None, offset=0):
    """The read circuit at out[offset + j] and the write circuit at out[offset + n + j] in one launch (include/cozk.h has the formula):
    a, v[0..4], t_read compact Vecs (U8 / U16 / U32 / U64, mixed freely) of one length n; imm a polynomial of at least n entries, plain
    or Rep3; gamma and tau canonical ints; mode "plain" or "rep3" (out_b required).  Asynchronous on the context's stream.  An
    inconsistent argument raises CozkError."""
    l = _decl()
    if len(v) != 5:
        raise ValueError("bytecode_leaves: five value columns")
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    ctx.check(l.cozk_bytecode_leaves(ctx.h, a.h, _handles(v), t_read.h, imm.h, g.ctypes.data, t.ctypes.data, _mode(mode), party_id, out_a.h,
                                     None if out_b is None else out_b.h, offset))


def bytecode_init_final_leaves(ctx, table, t_final, gamma, tau, mode, party_id, out_a, out_b=None, offset=0):
    """The init circuit at out[offset + i] and the final circuit at out[offset + B + i] in one launch from the six table columns
    (table[5], imm, may be an I64 Vec) and t_final, all of B entries; the row number is never stored.  The conventions of
    `bytecode_leaves`; in "rep3" mode the leaves are the trivial shares of a public value."""
    l = _decl()
    if len(table) != 6:
        raise ValueError("bytecode_init_final_leaves: six table columns")
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    ctx.check(l.cozk_bytecode_init_final_leaves(ctx.h, _handles(table), t_final.h, g.ctypes.data, t.ctypes.data, _mode(mode), party_id, out_a.h,
                                                None if out_b is None else out_b.h, offset))


class BytecodeProofConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("device", ctypes.c_int), ("log_n", ctypes.c_int), ("log_b", ctypes.c_int), ("seed", ctypes.c_uint64),
                ("precompute", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int)]


class BytecodeProofResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_commit_ms", ctypes.c_double),
                ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double), ("proof_len", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32)]


class BytecodeProof(L.HarnessHandle):
    """The bytecode proof as an in-process harness (`cozk_bytecode_proof_*`, csrc/host/bytecode_proof.hpp): a seeded table of 2^log_b rows
    and a trace of 2^log_n steps, `bytecode_witness` on the device, then prove() = commit of the nine columns, the two grand products,
    ONE opening that joins the seven compact columns with v_imm, t_final opened alone, one reduce_and_prove, and the plain verifier, which
    runs the multiset check.  PLAIN only.  tamper: 1 bumps v_rd[N / 2] ("multiset equality"), 2 sends a wrong claim ("leaf claim"), 3
    bumps t_final[a[N / 2]] ("multiset equality"); leaves_fused=False makes the leaves by the composition (the same proof bytes)."""
    PREFIX, CONFIG, RESULT = "cozk_bytecode_proof", BytecodeProofConfig, BytecodeProofResult

    def __init__(self, log_n=10, log_b=10, seed=1, device=0, precompute=True, leaves_fused=True, tamper=0, mode="plain"):
        cfg = BytecodeProofConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.device, cfg.log_n, cfg.log_b, cfg.seed = device, log_n, log_b, seed
        cfg.precompute, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), (1 if leaves_fused else 0), tamper
        self._open(cfg)
