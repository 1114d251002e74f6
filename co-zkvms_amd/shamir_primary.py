"""Lasso's primary sumcheck of the instruction lookups proved by n Shamir parties (`cozk_shamir_primary_*`,
csrc/host/shamir_primary.hpp) on the lookups harness's instance of (seed, log_n, n_pairs = n_mem, mix).  Between the multiplication levels
of the collation programs the 2t + 1 senders reduce the degree (`cozk_primary_group_*`, lookups.PrimaryGroup).  The proof is the plain
prover's, byte for byte (LookupsHarness(mode="plain", primary=True) up to proof_len, oracle/pyprimary.py)."""
import ctypes

import numpy as np

from . import _lib as L
from .engine import ShamirGpStats, mont_limbs_to_int
from .lookups import PrimaryGroup, PRIMARY_GROUP_SYMBOLS  # noqa: F401  (the group the prover's levels run as)

MAX_PARTIES = 32


class ShamirPrimaryConfig(ctypes.Structure):
    _fields_ = [("log_n", ctypes.c_int), ("n_mem", ctypes.c_int), ("mix", ctypes.c_int), ("degree", ctypes.c_int), ("num_parties", ctypes.c_int),
                ("devices", ctypes.c_int * MAX_PARTIES), ("seed", ctypes.c_uint64), ("share_counter", ctypes.c_uint64),
                ("mul_counter", ctypes.c_uint64), ("rand_counter", ctypes.c_uint64), ("tamper_final", ctypes.c_int)]


class ShamirPrimaryResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("grouped", ctypes.c_int), ("degree", ctypes.c_int), ("proof_len", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32), ("n_opened", ctypes.c_uint64), ("n_exchanges", ctypes.c_uint64),
                ("n_exchanged", ctypes.c_uint64), ("wall_ms", ctypes.c_double), ("t_build_ms", ctypes.c_double), ("t_masks_ms", ctypes.c_double),
                ("t_rounds_ms", ctypes.c_double), ("t_finals_ms", ctypes.c_double)]


_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SHAMIR_PRIMARY_SYMBOLS = ["cozk_shamir_primary_create", "cozk_shamir_primary_error", "cozk_shamir_primary_destroy", "cozk_shamir_primary_prove",
                          "cozk_shamir_primary_proof_bytes", "cozk_shamir_primary_msgs_len", "cozk_shamir_primary_msgs",
                          "cozk_shamir_primary_finals_len", "cozk_shamir_primary_finals", "cozk_shamir_primary_get_stats"]


class ShamirPrimary(L.HarnessHandle):
    """n Shamir parties of degree t prove the primary sumcheck; one device per party (an int: all on it).  mix = "uniform" | "sha2"
    (or 0 | 1).  tamper_final = k > 0 (tests): element k - 1 of `finals` is corrupted before it is opened"""
    PREFIX, CONFIG, RESULT = "cozk_shamir_primary", ShamirPrimaryConfig, ShamirPrimaryResult
    EXTRA = {"cozk_shamir_primary_msgs_len": (_sz, [_vp]), "cozk_shamir_primary_msgs": (_i, [_vp, _vp, _sz]),
             "cozk_shamir_primary_finals_len": (_sz, [_vp]), "cozk_shamir_primary_finals": (_i, [_vp, _vp, _sz]),
             "cozk_shamir_primary_get_stats": (_i, [_vp, ctypes.POINTER(ShamirGpStats)])}

    def __init__(self, log_n=6, n_mem=54, mix="uniform", parties=3, degree=1, devices=0, seed=1, share_counter=0, mul_counter=0, rand_counter=0,
                 tamper_final=0):
        cfg = ShamirPrimaryConfig()
        cfg.log_n = log_n
        cfg.n_mem = n_mem
        cfg.mix = mix if isinstance(mix, int) else (1 if mix == "sha2" else 0)
        cfg.degree = degree
        cfg.num_parties = parties
        devs = [devices] * MAX_PARTIES if isinstance(devices, int) else list(devices) + [0] * (MAX_PARTIES - len(devices))
        cfg.devices = (ctypes.c_int * MAX_PARTIES)(*devs[:MAX_PARTIES])
        cfg.seed = seed
        cfg.share_counter = share_counter
        cfg.mul_counter = mul_counter
        cfg.rand_counter = rand_counter
        cfg.tamper_final = tamper_final
        self._open(cfg)

    def _fe_list(self, what):
        n = self._f("_" + what + "_len")(self.h)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        rc = self._f("_" + what)(self.h, out.ctypes.data, n)
        if rc != L.OK:
            raise L.CozkError(rc, what)
        return mont_limbs_to_int(out[:n])

    def msgs(self):
        """the masked round messages [D round + k][p <= 2t]"""
        k = 2 * self.cfg.degree + 1
        v = self._fe_list("msgs")
        return [v[i:i + k] for i in range(0, len(v), k)]

    def finals(self):
        """[value][p <= t]: E_0(r) .. E_{n_mem - 1}(r), lookup_outputs(r)"""
        k = self.cfg.degree + 1
        v = self._fe_list("finals")
        return [v[i:i + k] for i in range(0, len(v), k)]

    def stats(self):
        st = ShamirGpStats()
        rc = self._f("_get_stats")(self.h, ctypes.byref(st))
        if rc != L.OK:
            raise L.CozkError(rc, "get_stats")
        return st
