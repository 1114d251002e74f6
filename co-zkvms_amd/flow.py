"""The ONE chained co-jolt worker flow over the C ABI (`cozk_flow_*`): commit-all -> bytecode -> instruction lookups -> read-write
memory -> Spartan -> one reduce_and_prove (co-jolt/src/jolt/vm/jolt/worker.rs:175-266)."""
import ctypes

from . import _lib as L


class FlowConfig(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("log_n", ctypes.c_int), ("log_m", ctypes.c_int), ("log_b", ctypes.c_int), ("log_mem", ctypes.c_int),
                ("n_mem", ctypes.c_int), ("n_subtables", ctypes.c_int), ("devices", ctypes.c_int * 3), ("seed", ctypes.c_uint64),
                ("precompute", ctypes.c_int), ("small_witness", ctypes.c_int), ("lookups_witness", ctypes.c_int), ("lookups_tamper", ctypes.c_int)]


class FlowResult(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int)] + [(k, ctypes.c_double) for k in (
        "wall_ms", "t_commit_ms", "t_bytecode_ms", "t_primary_ms", "t_lookups_gp_ms", "t_rw_ms", "t_spartan_ms", "t_open_ms", "t_worker_ms",
        "t_spartan_build_ms")] + [(k, ctypes.c_uint64) for k in (
            "bytes_star_up", "bytes_star_down", "bytes_ring", "star_messages", "n_polys", "n_openings", "proof_len")] + [("proof_digest", ctypes.c_uint8 * 32)]


FLOW_SYMBOLS = ["cozk_flow_create", "cozk_flow_error", "cozk_flow_destroy", "cozk_flow_num_polys", "cozk_flow_ctx", "cozk_flow_prove", "cozk_flow_proof_bytes"]
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


class FlowHarness(L.HarnessHandle):
    PREFIX, CONFIG, RESULT = "cozk_flow", FlowConfig, FlowResult
    EXTRA = {"cozk_flow_num_polys": (_sz, [_vp]), "cozk_flow_ctx": (_vp, [_vp, _i])}

    def __init__(self, mode="plain", log_n=4, log_m=3, log_b=3, log_mem=3, n_mem=6, n_subtables=3, devices=(0, 0, 0), seed=1, precompute=1, small_witness=0,
                 lookups_witness=0, lookups_tamper=0):
        """lookups_witness=1 (needs log_m == 16): read_cts / E / final_cts of the instruction lookups are a consistent instance made
        on the device (cozk_lasso_witness) and the verifier runs the multiset-equality check of their hashes; lookups_tamper=k > 0
        (tests) bumps final_cts[0][k - 1] so that only that check can reject"""
        cfg = FlowConfig()
        cfg.mode = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
        cfg.log_n, cfg.log_m, cfg.log_b, cfg.log_mem = log_n, log_m, log_b, log_mem
        cfg.n_mem, cfg.n_subtables = n_mem, n_subtables
        cfg.devices = (ctypes.c_int * 3)(*devices)
        cfg.seed = seed
        cfg.precompute = precompute
        cfg.small_witness = small_witness
        cfg.lookups_witness, cfg.lookups_tamper = lookups_witness, lookups_tamper
        self._open(cfg)

    def num_polys(self):
        return int(self._l.cozk_flow_num_polys(self.h))

    def ctx_handle(self, party=0):
        return self._l.cozk_flow_ctx(self.h, party)
