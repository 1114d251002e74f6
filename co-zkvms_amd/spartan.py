"""co-noir-spartan harness over the C ABI (`cozk_spartan_*`): BASELINE config 4 restated -- the
worker side of SpartanProverWorker::prove (co-noir-spartan/co-spartan/src/worker.rs:119-300) on a satisfied
synthetic R1CS, coordinator + verifier on the calling thread."""
import ctypes

from . import _lib as L


class SpartanConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("log_n", ctypes.c_int), ("precompute", ctypes.c_int), ("devices", ctypes.c_int * 3),
                ("seed", ctypes.c_uint64), ("lookup_round", ctypes.c_int), ("log_pub_workers", ctypes.c_int)]


class SpartanResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_zero_round_ms", ctypes.c_double),
                ("t_commit_ms", ctypes.c_double), ("t_sumcheck1_ms", ctypes.c_double), ("t_matrix_build_ms", ctypes.c_double),
                ("t_sumcheck2_ms", ctypes.c_double), ("t_open_ms", ctypes.c_double), ("t_worker_ms", ctypes.c_double),
                ("bytes_star_up", ctypes.c_uint64), ("bytes_star_down", ctypes.c_uint64), ("star_messages", ctypes.c_uint64),
                ("proof_len", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32), ("t_lookup_ms", ctypes.c_double),
                ("pub_workers", ctypes.c_int), ("pub_star_messages", ctypes.c_uint64), ("pub_bytes_up", ctypes.c_uint64),
                ("pub_bytes_down", ctypes.c_uint64)]


SPARTAN_SYMBOLS = ["cozk_spartan_create", "cozk_spartan_error", "cozk_spartan_destroy", "cozk_spartan_prove", "cozk_spartan_proof_bytes"]


class SpartanHarness(L.HarnessHandle):
    PREFIX, CONFIG, RESULT = "cozk_spartan", SpartanConfig, SpartanResult

    def __init__(self, mode="plain", log_n=10, precompute=True, devices=(0, 0, 0), seed=1, lookup_round=False, log_pub_workers=0):
        cfg = SpartanConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.log_n = log_n
        cfg.precompute = 1 if precompute else 0
        cfg.devices = (ctypes.c_int * 3)(*devices)
        cfg.seed = seed
        cfg.lookup_round = 1 if lookup_round else 0
        cfg.log_pub_workers = log_pub_workers
        self._open(cfg)
