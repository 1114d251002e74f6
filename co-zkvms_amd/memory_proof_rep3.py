"""The memory check and the output check of ReadWriteMemoryProof by three Rep3 parties as an in-process harness (`MemoryProofRep3`,
cozk_memory_proof_rep3_*): `RwProofRep3`'s sharing and steps, then the output check on each party's share of v_final, by
`OutputCheck.shared`'s device calls or by the dense composition in Rep3.  The proof bytes are `MemoryProof`'s at with_ts=False."""
import ctypes

from . import _lib as L

# the shared output check's create is declared by memory_proof.py (OutputCheck.shared) and listed here, with the harness that drives it
MEMORY_PROOF_REP3_SYMBOLS = ["cozk_output_check_shared_create", "cozk_memory_proof_rep3_create", "cozk_memory_proof_rep3_error", "cozk_memory_proof_rep3_destroy",
                             "cozk_memory_proof_rep3_prove", "cozk_memory_proof_rep3_proof_bytes"]


class MemoryProofRep3Config(ctypes.Structure):
    _fields_ = [("devices", ctypes.c_int * 3), ("log_n", ctypes.c_int), ("log_mem", ctypes.c_int), ("n_slots", ctypes.c_int), ("seed", ctypes.c_uint64),
                ("precompute", ctypes.c_int), ("leaves_fused", ctypes.c_int), ("tamper", ctypes.c_int), ("io_start", ctypes.c_uint64), ("io_len", ctypes.c_uint64),
                ("windowed", ctypes.c_int)]


class MemoryProofRep3Result(ctypes.Structure):
    _fields_ = [("verified", ctypes.c_int), ("wall_ms", ctypes.c_double), ("t_witness_ms", ctypes.c_double), ("t_share_ms", ctypes.c_double),
                ("t_commit_ms", ctypes.c_double), ("t_leaves_ms", ctypes.c_double), ("t_gp_ms", ctypes.c_double), ("t_out_ms", ctypes.c_double),
                ("t_open_ms", ctypes.c_double), ("ring_bytes", ctypes.c_uint64), ("proof_len", ctypes.c_uint64), ("prefix_len", ctypes.c_uint64),
                ("out_peak_bytes", ctypes.c_uint64), ("proof_digest", ctypes.c_uint8 * 32)]


class MemoryProofRep3(L.HarnessHandle):
    """`RwProofRep3` with the output check behind the memory check (`cozk_memory_proof_rep3_*`, csrc/host/memory_proof_rep3.hpp): the
    instance and the io window of `MemoryProof(seed, with_ts=False)`; prove() = the memory check by three Rep3 parties, r_eq, log_mem
    rounds on each party's share of v_final (windowed=True: `OutputCheck.shared`'s calls, windowed=False: the dense composition in Rep3,
    the same proof bytes), one opening of the shared v_final, one reduce_and_prove, and `MemoryProof`'s verifier.  The proof bytes are
    `MemoryProof`'s; proof[:prefix_len] is `RwProofRep3`'s prefix.  tamper: 1 and 2 are `RwProofRep3`'s, 4 adds 1 to v_io[io_len // 2]
    ("output check: final claim")."""
    PREFIX, CONFIG, RESULT = "cozk_memory_proof_rep3", MemoryProofRep3Config, MemoryProofRep3Result

    def __init__(self, log_n=10, log_mem=10, n_slots=4, seed=1, devices=(0, 0, 0), precompute=True, leaves_fused=True, tamper=0, io_start=64, io_len=1,
                 windowed=True):
        cfg = MemoryProofRep3Config()
        cfg.devices = (ctypes.c_int * 3)(*devices)
        cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.seed = log_n, log_mem, n_slots, seed
        cfg.precompute, cfg.leaves_fused, cfg.tamper = (1 if precompute else 0), int(leaves_fused), tamper
        cfg.io_start, cfg.io_len, cfg.windowed = io_start, io_len, int(windowed)
        self._open(cfg)
