"""CPU test of the surface of the output check and the whole read-write memory proof: the python binding's symbols are declared in
include/cozk.h and exported by the library, the config and result structs have the header's fields in the header's order, the package
exports the calls, and every bad config is refused with its text before any context exists (no GPU needed)."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


def test_memory_proof_symbols_declared_and_exported(cozk):
    MP = importlib.import_module("co-zkvms_amd.memory_proof")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert MP.MEMORY_PROOF_SYMBOLS == ["cozk_output_check_create", "cozk_output_check_round", "cozk_output_check_final", "cozk_output_check_len",
                                       "cozk_output_check_free", "cozk_memory_proof_create", "cozk_memory_proof_error", "cozk_memory_proof_destroy",
                                       "cozk_memory_proof_prove", "cozk_memory_proof_proof_bytes"]
    assert cozk.MemoryProof is MP.MemoryProof and MP.MemoryProof.PREFIX == "cozk_memory_proof" and cozk.OutputCheck is MP.OutputCheck
    for struct, name in ((MP.MemoryProofConfig, "cozk_memory_proof_config"), (MP.MemoryProofResult, "cozk_memory_proof_result")):  # the fields, in the header's order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    RP = importlib.import_module("co-zkvms_amd.rw_proof")
    assert [f[0] for f in MP.MemoryProofConfig._fields_] == [f[0] for f in RP.RwProofConfig._fields_] + ["io_start", "io_len", "windowed"]
    assert [f[0] for f in MP.MemoryProofResult._fields_] == ["verified", "wall_ms", "t_witness_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_out_ms", "t_ts_ms",
                                                             "t_open_ms", "proof_len", "prefix_len", "out_peak_bytes", "proof_digest"]
    assert cozk.MEMORY_PROOF_SYMBOLS == MP.MEMORY_PROOF_SYMBOLS
    assert cozk.MemoryProofConfig is MP.MemoryProofConfig and cozk.MemoryProofResult is MP.MemoryProofResult
    for n in MP.MEMORY_PROOF_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n


BAD_CONFIGS = [(dict(mode="rep3"), "mode is COZK_MODE_PLAIN"), (dict(log_n=0), "log_n in 1..22"), (dict(log_n=23), "log_n in 1..22"),
               (dict(n_slots=0), "n_slots in 1..4"), (dict(n_slots=5), "n_slots in 1..4"), (dict(log_mem=4), "log_mem in 5..24"),
               (dict(log_mem=25), "log_mem in 5..24"), (dict(tamper=5), "tamper in 0..4"), (dict(tamper=-1), "tamper in 0..4"),
               (dict(tamper=3, with_ts=False), "3 only with with_ts"), (dict(io_len=0), "io_len is at least 1 word"),
               (dict(io_start=60, io_len=5), "io_start + io_len > MEM"), (dict(io_start=65, io_len=1), "io_start + io_len > MEM"),
               (dict(io_start=2 ** 64 - 1, io_len=2), "io_start + io_len > MEM"), (dict(windowed=2), "windowed is 0 or 1"), (dict(windowed=-1), "windowed is 0 or 1")]


@pytest.mark.parametrize("kw,text", BAD_CONFIGS)
def test_bad_configs_are_refused_before_any_context_exists(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.MemoryProof(**dict(dict(log_n=4, log_mem=6, io_start=3, io_len=5), **kw))
    assert e.value.code == INVALID_ARG and "memory_proof: " in str(e.value) and text in str(e.value), str(e.value)
