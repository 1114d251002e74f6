"""CPU test of the surface of the timestamp range-check proof's device calls: the python binding's symbols are declared in
include/cozk.h and exported by the library, the package exports the three calls, and the constants agree with the header (no GPU
needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ts_proof_symbols_declared_and_exported(cozk):
    TP = importlib.import_module("co-zkvms_amd.ts_proof")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert TP.TS_PROOF_SYMBOLS == ["cozk_compact_batch_evaluate_at_chi", "cozk_compact_linear_combination", "cozk_timestamp_range_leaves",
                                   "cozk_ts_proof_create", "cozk_ts_proof_error", "cozk_ts_proof_destroy", "cozk_ts_proof_prove", "cozk_ts_proof_proof_bytes"]
    assert cozk.TsProof is TP.TsProof and TP.TsProof.PREFIX == "cozk_ts_proof"
    for struct, name in ((TP.TsProofConfig, "cozk_ts_proof_config"), (TP.TsProofResult, "cozk_ts_proof_result")):  # the fields, in the header's order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    assert cozk.TS_PROOF_SYMBOLS == TP.TS_PROOF_SYMBOLS
    assert cozk.compact_batch_evaluate_at_chi is TP.compact_batch_evaluate_at_chi
    assert cozk.compact_linear_combination is TP.compact_linear_combination
    assert cozk.timestamp_range_leaves is TP.timestamp_range_leaves
    for n in TP.TS_PROOF_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    assert TP.COMPACT_MAX_COLS == int(re.search(r"#define COZK_COMPACT_MAX_COLS (\d+)", header).group(1))
    assert TP.COMPACT_MAX_COLS >= 24  # the proof opens 5 columns per slot, 20 with Jolt's 4 slots
    assert TP.COMPACT_MAX_COLS >= 5 * 4
