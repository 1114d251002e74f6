"""Lasso's primary sumcheck of the instruction lookups proved by n Shamir parties (`cozk_shamir_primary_*`,
csrc/host/shamir_primary.hpp) on the lookups harness's instance of (seed, log_n, n_pairs = n_mem, mix).  Between the multiplication levels
of the collation programs the 2t + 1 senders reduce the degree (`cozk_primary_group_*`, lookups.PrimaryGroup).  The proof is the plain
prover's, byte for byte (LookupsHarness(mode="plain", primary=True) up to proof_len, oracle/pyprimary.py)."""
import ctypes

from ._lib import CozkError
from .engine import SHAMIR_MAX_PARTIES as MAX_PARTIES, ShamirHarnessHandle
from .lookups import PrimaryGroup, PRIMARY_GROUP_SYMBOLS, PRIMARY_KING_SYMBOLS, primary_plan  # noqa: F401  (the group the prover's levels run as)


class ShamirPrimaryConfig(ctypes.Structure):
    _fields_ = [("log_n", ctypes.c_int), ("n_mem", ctypes.c_int), ("mix", ctypes.c_int), ("degree", ctypes.c_int), ("num_parties", ctypes.c_int),
                ("devices", ctypes.c_int * MAX_PARTIES), ("seed", ctypes.c_uint64), ("share_counter", ctypes.c_uint64),
                ("mul_counter", ctypes.c_uint64), ("rand_counter", ctypes.c_uint64), ("tamper_final", ctypes.c_int)]


class ShamirPrimaryResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("grouped", ctypes.c_int), ("degree", ctypes.c_int), ("proof_len", ctypes.c_uint64),
                ("proof_digest", ctypes.c_uint8 * 32), ("n_opened", ctypes.c_uint64), ("n_exchanges", ctypes.c_uint64),
                ("n_exchanged", ctypes.c_uint64), ("wall_ms", ctypes.c_double), ("t_build_ms", ctypes.c_double), ("t_masks_ms", ctypes.c_double),
                ("t_rounds_ms", ctypes.c_double), ("t_finals_ms", ctypes.c_double)]


SHAMIR_PRIMARY_SYMBOLS = ["cozk_shamir_primary_create", "cozk_shamir_primary_error", "cozk_shamir_primary_destroy", "cozk_shamir_primary_prove",
                          "cozk_shamir_primary_proof_bytes", "cozk_shamir_primary_msgs_len", "cozk_shamir_primary_msgs",
                          "cozk_shamir_primary_finals_len", "cozk_shamir_primary_finals", "cozk_shamir_primary_get_stats"]


class ShamirPrimaryPrepResult(ctypes.Structure):
    """cozk_shamir_primary_prep_result"""
    _fields_ = [("n_openings", ctypes.c_uint64), ("pair_elems", ctypes.c_uint64), ("n_exchanges", ctypes.c_uint64), ("used", ctypes.c_int),
                ("t_offline_ms", ctypes.c_double)]


# the king construct's entry points (beside SHAMIR_PRIMARY_SYMBOLS, whose length tests pin)
SHAMIR_PRIMARY_KING_SYMBOLS = ["cozk_shamir_primary_prep", "cozk_shamir_primary_prep_get_result", "cozk_shamir_primary_prove_king"]


class ShamirPrimary(ShamirHarnessHandle):
    """n Shamir parties of degree t prove the primary sumcheck; one device per party (an int: all on it).  mix = "uniform" | "sha2"
    (or 0 | 1).  tamper_final = k > 0 (tests): element k - 1 of `finals` is corrupted before it is opened.  msgs(): the masked round
    messages [D round + k][p <= 2t].  finals(): [value][p <= t]: E_0(r) .. E_{n_mem - 1}(r), lookup_outputs(r)"""
    PREFIX, CONFIG, RESULT = "cozk_shamir_primary", ShamirPrimaryConfig, ShamirPrimaryResult

    def __init__(self, log_n=6, n_mem=54, mix="uniform", parties=3, degree=1, devices=0, seed=1, share_counter=0, mul_counter=0, rand_counter=0,
                 tamper_final=0):
        cfg = ShamirPrimaryConfig()
        cfg.log_n = log_n
        cfg.n_mem = n_mem
        cfg.mix = mix if isinstance(mix, int) else (1 if mix == "sha2" else 0)
        cfg.degree = degree
        cfg.num_parties = parties
        cfg.devices = self._devices(devices)
        cfg.seed = seed
        cfg.share_counter = share_counter
        cfg.mul_counter = mul_counter
        cfg.rand_counter = rand_counter
        cfg.tamper_final = tamper_final
        self._open(cfg)

    @classmethod
    def _decl(cls):
        l = super()._decl()
        vp, i = ctypes.c_void_p, ctypes.c_int
        for name, args in (("cozk_shamir_primary_prep", [vp, ctypes.POINTER(ShamirPrimaryPrepResult)]),
                           ("cozk_shamir_primary_prep_get_result", [vp, ctypes.POINTER(ShamirPrimaryPrepResult)]),
                           ("cozk_shamir_primary_prove_king", [vp, i, i, ctypes.POINTER(ShamirPrimaryResult)])):
            fn = getattr(l, name)
            fn.restype = i
            fn.argtypes = args
        return l

    def _king_call(self, name, *args):
        res = args[-1]
        rc = getattr(self._l, name)(self.h, *args[:-1], ctypes.byref(res))
        if rc != 0:
            raise CozkError(rc, self.last_error() or "?")
        return res

    def prep(self):
        """the preprocessing of ONE king prove (`cozk_shamir_primary_prep`): the exchange plan from the public flags, the opening masks
        and the exchanges' double-random pair -> ShamirPrimaryPrepResult.  Once per handle"""
        return self._king_call("cozk_shamir_primary_prep", ShamirPrimaryPrepResult())

    def prep_result(self):
        return self._king_call("cozk_shamir_primary_prep_get_result", ShamirPrimaryPrepResult())

    def prove_king(self, king=0, verify=True):
        """prove with the king level exchange on the prep's pair (`cozk_shamir_primary_prove_king`); consumes the prep.  The proof is
        prove()'s, byte for byte"""
        return self._king_call("cozk_shamir_primary_prove_king", king, 1 if verify else 0, ShamirPrimaryResult())
