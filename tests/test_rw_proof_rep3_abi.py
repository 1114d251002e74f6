"""CPU test of the surface of the Rep3 read-write memory proof: the python binding's symbols are declared in include/cozk.h and exported
by the library, the config and result structs have the header's fields in the header's order, the package exports the calls, and an
out-of-range config is refused with its text before any context exists (no GPU needed)."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


def test_rw_proof_rep3_symbols_declared_and_exported(cozk):
    R3 = importlib.import_module("co-zkvms_amd.rw_proof_rep3")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert R3.RW_PROOF_REP3_SYMBOLS == ["cozk_rw_memory_shared_leaves", "cozk_rw_memory_shared_init_final_leaves", "cozk_rw_proof_rep3_create",
                                        "cozk_rw_proof_rep3_error", "cozk_rw_proof_rep3_destroy", "cozk_rw_proof_rep3_prove", "cozk_rw_proof_rep3_proof_bytes"]
    assert cozk.RwProofRep3 is R3.RwProofRep3 and R3.RwProofRep3.PREFIX == "cozk_rw_proof_rep3"
    for struct, name in ((R3.RwProofRep3Config, "cozk_rw_proof_rep3_config"), (R3.RwProofRep3Result, "cozk_rw_proof_rep3_result")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    assert [f[0] for f in R3.RwProofRep3Config._fields_] == ["devices", "log_n", "log_mem", "n_slots", "seed", "precompute", "leaves_fused", "tamper"]
    assert [f[0] for f in R3.RwProofRep3Result._fields_] == ["verified", "wall_ms", "t_witness_ms", "t_share_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_open_ms",
                                                             "ring_bytes", "proof_len", "proof_digest"]
    assert cozk.RW_PROOF_REP3_SYMBOLS == R3.RW_PROOF_REP3_SYMBOLS
    assert cozk.rw_memory_shared_leaves is R3.rw_memory_shared_leaves and cozk.rw_memory_shared_init_final_leaves is R3.rw_memory_shared_init_final_leaves
    assert cozk.RwProofRep3Config is R3.RwProofRep3Config and cozk.RwProofRep3Result is R3.RwProofRep3Result
    for n in R3.RW_PROOF_REP3_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n


@pytest.mark.parametrize("kw,text", [(dict(log_n=0), "rw_proof_rep3: log_n in 1..22"), (dict(log_n=23), "rw_proof_rep3: log_n in 1..22"),
                                     (dict(log_mem=4), "rw_proof_rep3: log_mem in 5..24"), (dict(log_mem=25), "rw_proof_rep3: log_mem in 5..24"),
                                     (dict(n_slots=0), "rw_proof_rep3: n_slots in 1..4"), (dict(n_slots=5), "rw_proof_rep3: n_slots in 1..4"),
                                     (dict(leaves_fused=2), "leaves_fused are 0 or 1"), (dict(tamper=3), "rw_proof_rep3: tamper in 0..2"),
                                     (dict(tamper=-1), "rw_proof_rep3: tamper in 0..2")])
def test_out_of_range_configs_are_refused_before_any_context_exists(cozk, kw, text):
    """these refusals need no device: on a machine without one they come with their own text, not with the context's"""
    with pytest.raises(cozk.CozkError) as e:
        cozk.RwProofRep3(**dict(dict(log_n=4, log_mem=6), **kw))
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
