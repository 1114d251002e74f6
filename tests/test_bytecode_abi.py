"""CPU test of the surface of the bytecode memory check: the python binding's symbols are declared in include/cozk.h and exported by the
library, the device calls' parameter lists are the header's, the proof harness's config and result structs have the header's fields in
the header's order, and the package exports the calls and the harness (no GPU needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bytecode_symbols_declared_and_exported(cozk):
    BC = importlib.import_module("co-zkvms_amd.bytecode")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    calls = ["cozk_bytecode_witness", "cozk_bytecode_leaves", "cozk_bytecode_init_final_leaves"]
    assert BC.BYTECODE_SYMBOLS == calls + ["cozk_bytecode_proof_create", "cozk_bytecode_proof_error", "cozk_bytecode_proof_destroy",
                                           "cozk_bytecode_proof_prove", "cozk_bytecode_proof_proof_bytes"]
    assert cozk.BYTECODE_SYMBOLS == BC.BYTECODE_SYMBOLS and cozk.bytecode is BC
    assert cozk.bytecode_witness is BC.bytecode_witness and cozk.bytecode_leaves is BC.bytecode_leaves
    assert cozk.bytecode_init_final_leaves is BC.bytecode_init_final_leaves
    assert cozk.BytecodeProof is BC.BytecodeProof and BC.BytecodeProof.PREFIX == "cozk_bytecode_proof"
    assert cozk.BytecodeProofConfig is BC.BytecodeProofConfig and cozk.BytecodeProofResult is BC.BytecodeProofResult
    for n in BC.BYTECODE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    BC._decl()
    for n in calls:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % n, header)
        assert len(decl.group(1).split(",")) == len(getattr(lib, n).argtypes), n  # one ctypes argument per declared parameter
    params = lambda n: [p.split()[-1].strip("*") for p in re.search(r"\bint %s\s*\(([^;]*)\);" % n, header).group(1).split(",")]
    assert params("cozk_bytecode_witness") == ["ctx", "a", "table", "v_read", "v_imm", "t_read", "t_final"]
    assert params("cozk_bytecode_leaves") == ["ctx", "a", "v", "t_read", "imm", "gamma[4]", "tau[4]", "mode", "party_id", "out_a", "out_b", "offset"]
    assert params("cozk_bytecode_init_final_leaves") == ["ctx", "table", "t_final", "gamma[4]", "tau[4]", "mode", "party_id", "out_a", "out_b", "offset"]
    for struct, name in ((BC.BytecodeProofConfig, "cozk_bytecode_proof_config"), (BC.BytecodeProofResult, "cozk_bytecode_proof_result")):  # the header's order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    assert [f[0] for f in BC.BytecodeProofConfig._fields_] == ["mode", "device", "log_n", "log_b", "seed", "precompute", "leaves_fused", "tamper"]
