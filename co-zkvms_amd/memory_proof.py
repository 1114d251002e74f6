"""The output check of the read-write memory proof on the device (`OutputCheck`, cozk_output_check_*: the windowed sumcheck over the
compact v_final) and the whole ReadWriteMemoryProof in the reference's order as an in-process harness (`MemoryProof`,
cozk_memory_proof_*: memory check, output check, timestamp range check under one transcript and one opening accumulator)."""
import ctypes

import numpy as np

from . import _lib as L
from .engine import fr_to_mont_limbs, mont_limbs_to_int

MEMORY_PROOF_SYMBOLS = ["cozk_output_check_create", "cozk_output_check_round", "cozk_output_check_final", "cozk_output_check_len", "cozk_output_check_free",
                        "cozk_memory_proof_create", "cozk_memory_proof_error", "cozk_memory_proof_destroy", "cozk_memory_proof_prove",
                        "cozk_memory_proof_proof_bytes"]
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_output_check_create.restype = _i
    l.cozk_output_check_create.argtypes = [_vp, _vp, _vp, _sz, _vp, ctypes.POINTER(_vp)]
    l.cozk_output_check_shared_create.restype = _i
    l.cozk_output_check_shared_create.argtypes = [_vp, _vp, _vp, _sz, _vp, _i, ctypes.POINTER(_vp)]
    l.cozk_output_check_round.restype = _i
    l.cozk_output_check_round.argtypes = [_vp, _vp, _vp]
    l.cozk_output_check_final.restype = _i
    l.cozk_output_check_final.argtypes = [_vp, _vp, _vp]
    l.cozk_output_check_len.restype = _sz
    l.cozk_output_check_len.argtypes = [_vp]
    l.cozk_output_check_free.restype = _i
    l.cozk_output_check_free.argtypes = [_vp]
    return l


class OutputCheck:
    """sum_x eq(r_eq, x) io_range(x) (v_final(x) - v_io(x)) = 0, degree 3, HighToLow, from the compact columns: v_final a U32 Vec of 2^m
    words, v_io a U32 Vec of the io window's words only, io_start the window's first word, r_eq m canonical ints.  round(None) is round
    0, round(r) binds the previous variable and gives the next round, final(r) the last bind; v_final and v_io are only read and must
    outlive the handle (it keeps them alive).  A refused argument raises CozkError with the call's text."""

    def __init__(self, ctx, v_final, v_io, io_start, r_eq, party=None):
        self.ctx, self._l, self.h = ctx, _decl(), None
        self._keep = (v_final, v_io)
        rr = None if r_eq is None else fr_to_mont_limbs(list(r_eq)) if len(r_eq) else np.zeros((1, 4), dtype=np.uint64)
        h = _vp()
        args = (ctx.h, None if v_final is None else v_final.h, None if v_io is None else v_io.h, io_start, None if rr is None else rr.ctypes.data)
        if party is None:
            ctx.check(self._l.cozk_output_check_create(*args, ctypes.byref(h)))
        else:
            ctx.check(self._l.cozk_output_check_shared_create(*args, party, ctypes.byref(h)))
        self.h = h

    @classmethod
    def shared(cls, ctx, v_final, v_io, io_start, r_eq, party=0):
        """The same check on a v_final that is a `Rep3DensePolynomial` of 2^m unbound entries, plain or a Rep3 party's share
        (cozk_output_check_shared_create); party 0..2 for Rep3, 0 for plain.  Every round value of a Rep3 party is its additive share
        (a + b) / 2 of the dense rounds on linear_combination([v_final, v_io], [1, -1], mode, party), and final(r)[2] the additive share of
        (v_final - v_io)(r); the three parties' values sum to the plain ones."""
        return cls(ctx, v_final, v_io, io_start, r_eq, party=party)

    def __len__(self):
        return self._l.cozk_output_check_len(self.h)

    def round(self, r=None):
        """-> the round polynomial at X = 0, 2, 3 (canonical ints)"""
        rr = fr_to_mont_limbs([r]) if r is not None else None
        out = np.zeros((3, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_output_check_round(self.h, rr.ctypes.data if rr is not None else None, out.ctypes.data))
        return mont_limbs_to_int(out)

    def final(self, r):
        """-> (eq(r), io_range(r), (v_final - v_io)(r))"""
        rr = fr_to_mont_limbs([r]) if r is not None else None
        out = np.zeros((3, 4), dtype=np.uint64)
        self.ctx.check(self._l.cozk_output_check_final(self.h, rr.ctypes.data if rr is not None else None, out.ctypes.data))
        return tuple(mont_limbs_to_int(out))

    def free(self):
        if self.h:
            self._l.cozk_output_check_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MemoryProofConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("device", ctypes.c_int), ("log_n", ctypes.c_int), ("log_mem", ctypes.c_int), ("n_slots", ctypes.c_int),
                ("seed", ctypes.c_uint64), ("precompute", ctypes.c_int), ("with_ts", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int),
                ("io_start", ctypes.c_uint64), ("io_len", ctypes.c_uint64), ("windowed", ctypes.c_int)]


class MemoryProofResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_commit_ms", ctypes.c_double),
                ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_out_ms", ctypes.c_double), ("t_ts_ms", ctypes.c_double),
                ("t_open_ms", ctypes.c_double), ("proof_len", ctypes.c_uint64), ("prefix_len", ctypes.c_uint64), ("out_peak_bytes", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32)]


class MemoryProof(L.HarnessHandle):
    """The whole ReadWriteMemoryProof as an in-process harness (`cozk_memory_proof_*`, csrc/host/memory_proof.hpp): `RwProof`'s trace,
    witness and steps, with the output check between the memory check and the timestamp range check: v_io is v_final over the io
    window [io_start, io_start + io_len) words.  windowed=True runs the output check's rounds by `OutputCheck`'s calls, windowed=False
    by the dense composition on Fr copies (the same proof bytes).  proof[:prefix_len] is `RwProof`'s prefix at the same config.
    tamper: 1-3 are `RwProof`'s, 4 adds 1 to v_io[io_len // 2] ("output check: final claim")."""
    PREFIX, CONFIG, RESULT = "cozk_memory_proof", MemoryProofConfig, MemoryProofResult

    def __init__(self, log_n=10, log_mem=10, n_slots=4, seed=1, device=0, precompute=True, with_ts=True, leaves_fused=True, tamper=0, io_start=64, io_len=1,
                 windowed=True, mode="plain"):
        cfg = MemoryProofConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.device, cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.seed = device, log_n, log_mem, n_slots, seed
        cfg.precompute, cfg.with_ts, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), (1 if with_ts else 0), (1 if leaves_fused else 0), tamper
        cfg.io_start, cfg.io_len, cfg.windowed = io_start, io_len, int(windowed)
        self._open(cfg)
