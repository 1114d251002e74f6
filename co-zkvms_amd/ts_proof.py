"""The device calls of the timestamp range-check proof (TimestampValidityProof::prove, read_write_memory/worker.rs:78-105): openings of
compact public columns without an Fr copy of them (`compact_batch_evaluate_at_chi`, `compact_linear_combination`) and the leaves of
the proof's 6 n_slots + 1 grand-product circuits in one launch (`timestamp_range_leaves`), from the t_read columns of
`rw_memory_witness` and the counter families of `timestamp_range_witness`."""
import ctypes

import numpy as np

from . import _lib as L
from .engine import Vec, fr_to_mont_limbs, mont_limbs_to_int

TS_PROOF_SYMBOLS = ["cozk_compact_batch_evaluate_at_chi", "cozk_compact_linear_combination", "cozk_timestamp_range_leaves", "cozk_ts_proof_create",
                    "cozk_ts_proof_error", "cozk_ts_proof_destroy", "cozk_ts_proof_prove", "cozk_ts_proof_proof_bytes"]
COMPACT_MAX_COLS = 24
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_compact_batch_evaluate_at_chi.restype = _i
    l.cozk_compact_batch_evaluate_at_chi.argtypes = [_vp, _vp, _sz, _vp, _vp]
    l.cozk_compact_linear_combination.restype = _i
    l.cozk_compact_linear_combination.argtypes = [_vp, _vp, _vp, _sz, _vp]
    l.cozk_timestamp_range_leaves.restype = _i
    l.cozk_timestamp_range_leaves.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz]
    return l


def _handles(vecs):
    return (_vp * max(1, len(vecs)))(*[v.h for v in vecs])


def compact_batch_evaluate_at_chi(ctx, cols, chi, raw=False):
    """cols: 1 to 24 U8 / U16 / U32 / U64 Vecs of one length n; chi: an FR Vec of at least n entries.  Returns sum_i chi[i] cols[c][i]
    per column as canonical ints (raw: the uint64[k, 4] Montgomery limbs), bit for bit Rep3DensePolynomial.batch_evaluate_at_chi on
    PLAIN polynomials of the same values.  A wrong kind, unequal lengths, a column count out of range or a short chi raises CozkError."""
    l = _decl()
    k = len(cols)
    out = np.zeros((max(1, k), 4), dtype=np.uint64)
    ctx.check(l.cozk_compact_batch_evaluate_at_chi(ctx.h, _handles(cols), k, chi.h, out.ctypes.data))
    return out[:k] if raw else mont_limbs_to_int(out[:k])


def compact_linear_combination(ctx, cols, coeffs):
    """A new FR Vec out[i] = sum_c coeffs[c] cols[c][i] (coeffs: canonical ints), bit for bit Rep3DensePolynomial.linear_combination
    on PLAIN polynomials of the same values; the kinds and limits of `compact_batch_evaluate_at_chi`."""
    l = _decl()
    cf = fr_to_mont_limbs(list(coeffs)) if len(coeffs) else np.zeros((1, 4), dtype=np.uint64)
    h = _vp()
    ctx.check(l.cozk_compact_linear_combination(ctx.h, _handles(cols), cf.ctypes.data, len(cols), ctypes.byref(h)))
    return Vec(ctx, h, L.SCALAR_FR)


def timestamp_range_leaves(ctx, t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, gamma, tau, out, offset=0):
    """The leaves of the range check's 6 n_slots + 1 circuits into the FR Vec `out` from `offset`, circuit-major (include/cozk.h has the
    layout); every column a U32 Vec of n entries (the witness with M == n), gamma and tau canonical ints.  t_read[s][j] > j or an
    inconsistent argument raises CozkError (COZK_ERR_INVALID_ARG)."""
    l = _decl()
    g, t = fr_to_mont_limbs([gamma]), fr_to_mont_limbs([tau])
    ctx.check(l.cozk_timestamp_range_leaves(ctx.h, _handles(t_read), _handles(rc_rt), _handles(rc_gmr), _handles(fc_rt), _handles(fc_gmr), len(t_read),
                                            g.ctypes.data, t.ctypes.data, out.h, offset))


class TsProofConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("device", ctypes.c_int), ("log_n", ctypes.c_int), ("log_mem", ctypes.c_int), ("n_slots", ctypes.c_int),
                ("seed", ctypes.c_uint64), ("precompute", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int)]


class TsProofResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_commit_ms", ctypes.c_double),
                ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double), ("proof_len", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32)]


class TsProof(L.HarnessHandle):
    """The timestamp range-check proof as an in-process harness (`cozk_ts_proof_*`, csrc/host/ts_range_proof.hpp): a Jolt-shaped trace
    from `seed`, both witness walks on the device, then prove() = commit of the 5 n_slots compact columns, one batched grand product
    over the 6 n_slots + 1 circuits, one claim exchange, one reduce_and_prove, and the plain verifier.  PLAIN only.  tamper: 1 bumps a
    final counter (the multiset check rejects), 2 sends a wrong claim (the leaf check rejects); leaves_fused=False makes the leaves by
    the composition of fingerprint_leaves (the same proof bytes)."""
    PREFIX, CONFIG, RESULT = "cozk_ts_proof", TsProofConfig, TsProofResult

    def __init__(self, log_n=10, log_mem=10, n_slots=4, seed=1, device=0, precompute=True, leaves_fused=True, tamper=0, mode="plain"):
        cfg = TsProofConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.device, cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.seed = device, log_n, log_mem, n_slots, seed
        cfg.precompute, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), (1 if leaves_fused else 0), tamper
        self._open(cfg)
