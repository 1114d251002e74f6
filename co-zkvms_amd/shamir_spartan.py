"""co-noir-spartan proved by n Shamir parties (`cozk_shamir_spartan_*`, csrc/host/shamir_spartan.hpp) and the Spartan groups its
sumcheck rounds run as (`cozk_spartan_group_*`, csrc/spartan_group.inc): one round of k members against ONE public polynomial in one
launch and one fetch.  The proof is the plain prover's, byte for byte (SpartanHarness(mode="plain"), oracle/pyspartan.py)."""
import ctypes

import numpy as np

from . import _lib as L
from .engine import SHAMIR_MAX_PARTIES as MAX_PARTIES, ShamirHarnessHandle, fr_to_mont_limbs, mont_limbs_to_int

FIRST, SECOND = L.SPARTAN_GROUP_FIRST, L.SPARTAN_GROUP_SECOND


class SpartanGroup:
    """k members of P PLAIN polynomials each (FIRST: (za, zb, zc) against eq, 4 evaluations; SECOND: (z) against lin = alpha A + beta B +
    gamma C, 3 evaluations), driven on the stream of the driver `ctx`.  The members may belong to other contexts on the same device; the
    group refers to them and they must outlive it.  It copies `pub` at create and owns that copy."""

    def __init__(self, ctx, kind, members, pub):
        self.ctx = ctx
        self.kind = kind
        self.P, self.E = (3, 4) if kind == FIRST else (1, 3)
        self.members = [tuple(m) if isinstance(m, (tuple, list)) else (m,) for m in members]
        planes = [p for m in self.members for p in m]
        arr = (ctypes.c_void_p * max(1, len(planes)))(*[p.h for p in planes])
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_spartan_group_create(ctx.h, kind, arr, len(self.members), pub.h, ctypes.byref(h)))
        self.h = h

    def __len__(self):
        return self.ctx._l.cozk_spartan_group_len(self.h)

    def round_raw(self, r):
        """Montgomery limbs (k, E, 4) of one round; r: limbs of the previous challenge or None in the first round"""
        out = np.zeros((len(self.members), self.E, 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_spartan_group_round(self.h, r.ctypes.data if r is not None else None, out.ctypes.data))
        return out

    def round(self, r):
        """bind every plane and the public polynomial with r (None in the first round), then each member's E evaluations"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        v = mont_limbs_to_int(self.round_raw(rr))
        return [v[self.E * m:self.E * (m + 1)] for m in range(len(self.members))]

    def final_raw(self, r, k_final):
        out = np.zeros((self.P * k_final + 1, 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_spartan_group_final(self.h, r.ctypes.data if r is not None else None, k_final, out.ctypes.data))
        return out

    def final(self, r, k_final):
        """the last bind with r (None: none) -> ([the P final values of member m for m < k_final], the public polynomial's)"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        v = mont_limbs_to_int(self.final_raw(rr, k_final))
        return [v[self.P * m:self.P * (m + 1)] for m in range(k_final)], v[-1]

    def pub_raw(self):
        out = np.zeros((len(self), 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_spartan_group_pub_download(self.h, out.ctypes.data))
        return out

    def free(self):
        if self.h:
            self.ctx._l.cozk_spartan_group_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ShamirSpartanConfig(ctypes.Structure):
    _fields_ = [("log_n", ctypes.c_int), ("precompute", ctypes.c_int), ("degree", ctypes.c_int), ("num_parties", ctypes.c_int),
                ("devices", ctypes.c_int * MAX_PARTIES), ("seed", ctypes.c_uint64), ("share_counter", ctypes.c_uint64),
                ("rand_counter", ctypes.c_uint64)]


class ShamirSpartanResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("grouped", ctypes.c_int), ("proof_len", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32),
                ("n_opened", ctypes.c_uint64), ("wall_ms", ctypes.c_double), ("t_zero_round_ms", ctypes.c_double), ("t_commit_ms", ctypes.c_double),
                ("t_masks_ms", ctypes.c_double), ("t_sumcheck1_ms", ctypes.c_double), ("t_matrix_build_ms", ctypes.c_double),
                ("t_sumcheck2_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double)]


SHAMIR_SPARTAN_SYMBOLS = ["cozk_shamir_spartan_create", "cozk_shamir_spartan_error", "cozk_shamir_spartan_destroy", "cozk_shamir_spartan_prove",
                          "cozk_shamir_spartan_proof_bytes", "cozk_shamir_spartan_msgs_len", "cozk_shamir_spartan_msgs",
                          "cozk_shamir_spartan_finals_len", "cozk_shamir_spartan_finals", "cozk_shamir_spartan_get_stats"]


class ShamirSpartanHarness(ShamirHarnessHandle):
    """n Shamir parties of degree t prove the co-noir-spartan instance of (seed, log_n); one device per party (an int: all on it).
    msgs(): the masked first-sumcheck messages [m][p <= 2t], m = 4 round + evaluation index.  finals(): [value][p <= t]: za, zb,
    zc(rx); round by round the second sumcheck's g(0..2); z's final value; z(ry)"""
    PREFIX, CONFIG, RESULT = "cozk_shamir_spartan", ShamirSpartanConfig, ShamirSpartanResult

    def __init__(self, log_n=10, parties=3, degree=1, devices=0, seed=1, precompute=True, share_counter=0, rand_counter=0):
        cfg = ShamirSpartanConfig()
        cfg.log_n = log_n
        cfg.precompute = 1 if precompute else 0
        cfg.degree = degree
        cfg.num_parties = parties
        cfg.devices = self._devices(devices)
        cfg.seed = seed
        cfg.share_counter = share_counter
        cfg.rand_counter = rand_counter
        self._open(cfg)
