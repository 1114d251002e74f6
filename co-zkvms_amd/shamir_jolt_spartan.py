"""co-jolt's Spartan worker proved by n Shamir parties (`cozk_shamir_jolt_spartan_*`, csrc/host/shamir_jolt_spartan.hpp) and the groups
its outer and shift sumchecks run as (`cozk_outer_group_*`, `cozk_shift_group_*`, csrc/outer_group.inc): one round of k members in one
launch and one fetch.  The proof is the plain prover's, byte for byte (OuterHarness(mode="plain", full=True), oracle/pyspartan_outer.py)."""
import ctypes

import numpy as np

from .engine import SHAMIR_MAX_PARTIES as MAX_PARTIES, ShamirHarnessHandle, fr_to_mont_limbs, mont_limbs_to_int


class OuterGroup:
    """k PLAIN `SpartanOuter` members of one system, one tau and one state, driven on the stream of the driver `ctx`.  The members may
    belong to other contexts on the same device; the group refers to them and they must outlive it."""

    def __init__(self, ctx, members):
        self.ctx = ctx
        self.members = list(members)
        arr = (ctypes.c_void_p * max(1, len(self.members)))(*[m.h for m in self.members])
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_outer_group_create(ctx.h, arr, len(self.members), ctypes.byref(h)))
        self.h = h

    def __len__(self):
        return self.ctx._l.cozk_outer_group_len(self.h)

    def round_raw(self, r, claims):
        """Montgomery limbs (k, 4, 4) of one round; r: limbs of the previous challenge or None in the first round; claims: limbs (k, 4)"""
        out = np.zeros((len(self.members), 4, 4), dtype=np.uint64)
        claims = np.ascontiguousarray(claims, dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_outer_group_round(self.h, r.ctypes.data if r is not None else None, claims.ctypes.data, out.ctypes.data))
        return out

    def round(self, r, claims):
        """bind every member with r (None in the first round), then each member's four coefficients from its hint claims[m]"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        v = mont_limbs_to_int(self.round_raw(rr, fr_to_mont_limbs(list(claims))).reshape(-1, 4))
        return [v[4 * m:4 * (m + 1)] for m in range(len(self.members))]

    def final_raw(self, r, k_final):
        out = np.zeros((max(1, k_final), 3, 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_outer_group_final(self.h, r.ctypes.data, k_final, out.ctypes.data))
        return out[:k_final]

    def final(self, r, k_final):
        """the last bind with r -> [Az(r), Bz(r), Cz(r)] of members 0 .. k_final - 1"""
        v = mont_limbs_to_int(self.final_raw(fr_to_mont_limbs([r])[0], k_final).reshape(-1, 4))
        return [v[3 * m:3 * (m + 1)] for m in range(k_final)]

    def free(self):
        if self.h:
            self.ctx._l.cozk_outer_group_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ShiftGroup:
    """k members of ONE PLAIN polynomial each against ONE public polynomial, HighToLow, evaluations at 0 and 2.  The group refers to the
    members; it copies `pub` at create and owns that copy."""

    def __init__(self, ctx, members, pub):
        self.ctx = ctx
        self.members = list(members)
        arr = (ctypes.c_void_p * max(1, len(self.members)))(*[p.h for p in self.members])
        h = ctypes.c_void_p()
        ctx.check(ctx._l.cozk_shift_group_create(ctx.h, arr, len(self.members), pub.h, ctypes.byref(h)))
        self.h = h

    def __len__(self):
        return self.ctx._l.cozk_shift_group_len(self.h)

    def round_raw(self, r):
        out = np.zeros((len(self.members), 2, 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_shift_group_round(self.h, r.ctypes.data if r is not None else None, out.ctypes.data))
        return out

    def round(self, r):
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        v = mont_limbs_to_int(self.round_raw(rr).reshape(-1, 4))
        return [v[2 * m:2 * (m + 1)] for m in range(len(self.members))]

    def final_raw(self, r, k_final):
        out = np.zeros((k_final + 1, 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_shift_group_final(self.h, r.ctypes.data if r is not None else None, k_final, out.ctypes.data))
        return out

    def final(self, r, k_final):
        """the last bind with r (None: none) -> ([member m's final value for m < k_final], the public polynomial's)"""
        rr = fr_to_mont_limbs([r])[0] if r is not None else None
        v = mont_limbs_to_int(self.final_raw(rr, k_final))
        return v[:k_final], v[-1]

    def pub_raw(self):
        out = np.zeros((len(self), 4), dtype=np.uint64)
        self.ctx.check(self.ctx._l.cozk_shift_group_pub_download(self.h, out.ctypes.data))
        return out

    def free(self):
        if self.h:
            self.ctx._l.cozk_shift_group_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ShamirJoltSpartanConfig(ctypes.Structure):
    _fields_ = [("log_steps", ctypes.c_int), ("system", ctypes.c_int), ("degree", ctypes.c_int), ("num_parties", ctypes.c_int),
                ("devices", ctypes.c_int * MAX_PARTIES), ("seed", ctypes.c_uint64), ("share_counter", ctypes.c_uint64),
                ("rand_counter", ctypes.c_uint64)]


class ShamirJoltSpartanResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("grouped", ctypes.c_int), ("proof_len", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32),
                ("n_opened", ctypes.c_uint64), ("wall_ms", ctypes.c_double), ("t_build_ms", ctypes.c_double), ("t_masks_ms", ctypes.c_double),
                ("t_outer_ms", ctypes.c_double), ("t_inner_ms", ctypes.c_double), ("t_shift_ms", ctypes.c_double),
                ("t_openings_ms", ctypes.c_double)]


OUTER_GROUP_SYMBOLS = ["cozk_outer_group_create", "cozk_outer_group_round", "cozk_outer_group_final", "cozk_outer_group_len",
                       "cozk_outer_group_free"]
SHIFT_GROUP_SYMBOLS = ["cozk_shift_group_create", "cozk_shift_group_round", "cozk_shift_group_final", "cozk_shift_group_len",
                       "cozk_shift_group_pub_download", "cozk_shift_group_free"]
SHAMIR_JOLT_SPARTAN_SYMBOLS = ["cozk_shamir_jolt_spartan_create", "cozk_shamir_jolt_spartan_error", "cozk_shamir_jolt_spartan_destroy",
                               "cozk_shamir_jolt_spartan_prove", "cozk_shamir_jolt_spartan_proof_bytes", "cozk_shamir_jolt_spartan_msgs_len",
                               "cozk_shamir_jolt_spartan_msgs", "cozk_shamir_jolt_spartan_finals_len", "cozk_shamir_jolt_spartan_finals",
                               "cozk_shamir_jolt_spartan_get_stats"]


class ShamirJoltSpartanHarness(ShamirHarnessHandle):
    """n Shamir parties of degree t prove the whole Spartan worker on the outer harness's instance of (seed, log_steps, system); one
    device per party (an int: all on it).  msgs(): the masked outer messages [m][p <= 2t], m = 4 round + coefficient.  finals():
    [value][p <= t] in proof order: Az, Bz, Cz(r); the inner rounds' coefficients; shift_claim; the shift rounds' coefficients; the
    witness evaluations; the shift-witness evaluations"""
    PREFIX, CONFIG, RESULT = "cozk_shamir_jolt_spartan", ShamirJoltSpartanConfig, ShamirJoltSpartanResult

    def __init__(self, log_steps=4, system="jolt", parties=3, degree=1, devices=0, seed=1, share_counter=0, rand_counter=0):
        cfg = ShamirJoltSpartanConfig()
        cfg.log_steps = log_steps
        cfg.system = system if isinstance(system, int) else (1 if system == "jolt" else 0)
        cfg.degree = degree
        cfg.num_parties = parties
        cfg.devices = self._devices(devices)
        cfg.seed = seed
        cfg.share_counter = share_counter
        cfg.rand_counter = rand_counter
        self._open(cfg)
