"""The chained co-jolt flow with a CONSISTENT instruction-lookup witness (cozk_flow_config.lookups_witness; csrc/host/flow_harness.hpp):
read_cts / E / final_cts come from cozk_lasso_witness over the committed query chunks, and the harness verifier runs the
multiset-equality check of the lookups' memory-checking hashes (lasso/memory_checking/worker.rs:40-127) that the seeded counters
could not pass.  oracle/pyflow.py does not reach log_n = 16 in Python integers, so there is no byte comparison here: the new
kernels are compared exactly in test_gpu_lasso_witness.py and the rest of the proof runs code that is byte-checked elsewhere."""
import importlib

import pytest

pytestmark = pytest.mark.gpu

SHAPE = dict(log_n=16, log_m=16, log_b=8, log_mem=8, n_mem=6, n_subtables=3, seed=2026)
MULTISET = "lookups: multiset equality of the memory-checking hashes"


@pytest.fixture(scope="module")
def FL():
    return importlib.import_module("co-zkvms_amd.flow")


def test_consistent_lookups_verify_plain_equals_rep3_and_repeat(cozk, FL):
    digs = {}
    for mode in ("plain", "rep3"):
        h = FL.FlowHarness(mode=mode, lookups_witness=1, **SHAPE)
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        assert bytes(h.prove(verify=False).proof_digest) == bytes(r.proof_digest)
        digs[mode] = bytes(r.proof_digest)
        h.close()
    assert digs["plain"] == digs["rep3"]


def test_a_bumped_final_counter_fails_only_the_multiset_check(cozk, FL):
    h = FL.FlowHarness(mode="plain", lookups_witness=1, lookups_tamper=1, **SHAPE)
    r = h.prove(verify=True)
    assert r.verified == 0
    assert MULTISET in h.last_error()
    h.close()


def test_seeded_lookups_at_the_same_shape_still_verify(cozk, FL):
    h = FL.FlowHarness(mode="plain", lookups_witness=0, **SHAPE)
    r = h.prove(verify=True)
    assert r.verified == 1, h.last_error()
    h.close()


def test_consistent_lookups_need_the_16_bit_table(cozk, FL):
    with pytest.raises(cozk.CozkError) as e:
        FL.FlowHarness(mode="plain", lookups_witness=1, **dict(SHAPE, log_m=12))
    assert e.value.code == -1 and "lookups_witness needs log_m == 16" in str(e.value)
