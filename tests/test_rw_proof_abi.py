"""CPU test of the surface of the read-write memory proof: the python binding's symbols are declared in include/cozk.h and exported by
the library, the config and result structs have the header's fields in the header's order, the package exports the calls, and the
compact opening takes the proof's column counts (no GPU needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rw_proof_symbols_declared_and_exported(cozk):
    RP = importlib.import_module("co-zkvms_amd.rw_proof")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert RP.RW_PROOF_SYMBOLS == ["cozk_rw_memory_leaves", "cozk_rw_memory_init_final_leaves", "cozk_rw_proof_create", "cozk_rw_proof_error",
                                   "cozk_rw_proof_destroy", "cozk_rw_proof_prove", "cozk_rw_proof_proof_bytes"]
    assert cozk.RwProof is RP.RwProof and RP.RwProof.PREFIX == "cozk_rw_proof"
    for struct, name in ((RP.RwProofConfig, "cozk_rw_proof_config"), (RP.RwProofResult, "cozk_rw_proof_result")):  # the fields, in the header's order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    assert [f[0] for f in RP.RwProofConfig._fields_] == ["mode", "device", "log_n", "log_mem", "n_slots", "seed", "precompute", "with_ts", "leaves_fused", "tamper"]
    assert cozk.RW_PROOF_SYMBOLS == RP.RW_PROOF_SYMBOLS
    assert cozk.rw_memory_leaves is RP.rw_memory_leaves and cozk.rw_memory_init_final_leaves is RP.rw_memory_init_final_leaves
    assert cozk.RwProofConfig is RP.RwProofConfig and cozk.RwProofResult is RP.RwProofResult
    for n in RP.RW_PROOF_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    define = lambda name: re.search(r"#define %s (\w+)" % name, header).group(1)
    # the opening at r_rw carries 3 n_slots + 2 columns at 4 slots, the range check's 5 n_slots
    assert int(define("COZK_COMPACT_MAX_COLS")) >= 3 * 4 + 2
