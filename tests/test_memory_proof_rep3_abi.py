"""CPU test of the surface of the three-party memory proof and of the shared output check: the python binding's symbols are declared in
include/cozk.h and exported by the library, the config and result structs have the header's fields in the header's order, the package
exports the calls, a null config or handle is refused, and an out-of-range config is refused with its text before any context exists
(no GPU needed)."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OK = -1, 0


def test_memory_proof_rep3_symbols_declared_and_exported(cozk):
    M3 = importlib.import_module("co-zkvms_amd.memory_proof_rep3")
    MPm = importlib.import_module("co-zkvms_amd.memory_proof")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert M3.MEMORY_PROOF_REP3_SYMBOLS == ["cozk_output_check_shared_create", "cozk_memory_proof_rep3_create", "cozk_memory_proof_rep3_error",
                                            "cozk_memory_proof_rep3_destroy", "cozk_memory_proof_rep3_prove", "cozk_memory_proof_rep3_proof_bytes"]
    assert cozk.MemoryProofRep3 is M3.MemoryProofRep3 and M3.MemoryProofRep3.PREFIX == "cozk_memory_proof_rep3"
    for struct, name in ((M3.MemoryProofRep3Config, "cozk_memory_proof_rep3_config"), (M3.MemoryProofRep3Result, "cozk_memory_proof_rep3_result")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [f for decl in re.findall(r"(?:int|double|uint64_t|uint8_t)\s+([^;]+);", body) for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert fields == [f[0] for f in struct._fields_], name
    assert [f[0] for f in M3.MemoryProofRep3Config._fields_] == ["devices", "log_n", "log_mem", "n_slots", "seed", "precompute", "leaves_fused", "tamper", "io_start",
                                                                 "io_len", "windowed"]
    assert [f[0] for f in M3.MemoryProofRep3Result._fields_] == ["verified", "wall_ms", "t_witness_ms", "t_share_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_out_ms",
                                                                 "t_open_ms", "ring_bytes", "proof_len", "prefix_len", "out_peak_bytes", "proof_digest"]
    assert cozk.MEMORY_PROOF_REP3_SYMBOLS == M3.MEMORY_PROOF_REP3_SYMBOLS
    assert cozk.MemoryProofRep3Config is M3.MemoryProofRep3Config and cozk.MemoryProofRep3Result is M3.MemoryProofRep3Result
    assert callable(cozk.OutputCheck.shared) and cozk.OutputCheck is MPm.OutputCheck
    for n in M3.MEMORY_PROOF_REP3_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n


def test_a_null_config_or_handle_is_refused(cozk):
    M3 = importlib.import_module("co-zkvms_amd.memory_proof_rep3")
    l = M3.MemoryProofRep3._decl()
    h = ctypes.c_void_p()
    cfg, res = M3.MemoryProofRep3Config(), M3.MemoryProofRep3Result()
    assert l.cozk_memory_proof_rep3_create(None, ctypes.byref(h)) == INVALID_ARG and not h
    assert l.cozk_memory_proof_rep3_create(ctypes.byref(cfg), None) == INVALID_ARG
    assert l.cozk_memory_proof_rep3_prove(None, 1, ctypes.byref(res)) == INVALID_ARG
    buf = (ctypes.c_uint8 * 8)()
    assert l.cozk_memory_proof_rep3_proof_bytes(None, buf, 8) == INVALID_ARG
    assert l.cozk_memory_proof_rep3_error(None) == b"null harness"
    assert l.cozk_memory_proof_rep3_destroy(None) == OK
    # a harness whose create was refused: prove with it, or with a null result, is refused too
    cfg.log_n, cfg.log_mem, cfg.n_slots, cfg.io_len = 0, 6, 4, 1
    assert l.cozk_memory_proof_rep3_create(ctypes.byref(cfg), ctypes.byref(h)) == INVALID_ARG and h
    assert b"memory_proof_rep3: log_n in 1..22" in l.cozk_memory_proof_rep3_error(h)
    assert l.cozk_memory_proof_rep3_prove(h, 1, ctypes.byref(res)) == INVALID_ARG
    assert l.cozk_memory_proof_rep3_prove(h, 1, None) == INVALID_ARG
    assert l.cozk_memory_proof_rep3_destroy(h) == OK
    # the shared output check's create: a null context or out
    oc = ctypes.c_void_p()
    MPm = importlib.import_module("co-zkvms_amd.memory_proof")
    assert MPm._decl().cozk_output_check_shared_create(None, None, None, 0, None, 0, ctypes.byref(oc)) == INVALID_ARG and not oc


@pytest.mark.parametrize("kw,text", [(dict(log_n=0), "memory_proof_rep3: log_n in 1..22"), (dict(log_n=23), "memory_proof_rep3: log_n in 1..22"),
                                     (dict(log_mem=4), "memory_proof_rep3: log_mem in 5..24"), (dict(log_mem=25), "memory_proof_rep3: log_mem in 5..24"),
                                     (dict(n_slots=0), "memory_proof_rep3: n_slots in 1..4"), (dict(n_slots=5), "memory_proof_rep3: n_slots in 1..4"),
                                     (dict(leaves_fused=2), "leaves_fused are 0 or 1"), (dict(tamper=3), "3 only with with_ts"),
                                     (dict(tamper=5), "memory_proof_rep3: tamper in 0..4"), (dict(tamper=-1), "memory_proof_rep3: tamper in 0..4"),
                                     (dict(io_len=0), "memory_proof_rep3: io_len is at least 1 word"),
                                     (dict(io_start=60, io_len=5), "memory_proof_rep3: io_start + io_len > MEM"),
                                     (dict(windowed=2), "memory_proof_rep3: windowed is 0 or 1")])
def test_out_of_range_configs_are_refused_before_any_context_exists(cozk, kw, text):
    """these refusals need no device: on a machine without one they come with their own text, not with the context's"""
    with pytest.raises(cozk.CozkError) as e:
        cozk.MemoryProofRep3(**dict(dict(log_n=4, log_mem=6, io_start=3, io_len=5), **kw))
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
