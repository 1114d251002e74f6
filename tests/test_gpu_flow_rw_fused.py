"""GPU: the chained flow's phase 4a with its leaves made by the two fused shared calls (COZK_RW_FUSED=1, csrc/host/flow_harness.hpp:
cozk_rw_memory_shared_leaves and cozk_rw_memory_shared_init_final_leaves over the flow's compact address and timestamp columns and its
value polynomials, the shared v_init among them) gives, byte for byte, the proof of the ten cozk_fingerprint_leaves launches, in plain
and rep3 mode -- the REP3 path of the kernels under a real caller, the public part entering the shares through add_public."""
import importlib

import pytest

pytestmark = pytest.mark.gpu
CONFIGS = [dict(log_n=3, log_m=3, log_b=2, log_mem=3, n_mem=6, n_subtables=3, seed=5),
           dict(log_n=5, log_m=3, log_b=4, log_mem=4, n_mem=9, n_subtables=4, seed=7)]  # the two of test_gpu_flow_bytecode_fused.py


def _prove(h, monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("COZK_RW_FUSED", raising=False)
    else:
        monkeypatch.setenv("COZK_RW_FUSED", switch)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    return bytes(res.proof_digest), h.proof_bytes(res)  # the bytes of this prove: the handle keeps only its last proof


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "2p%d-2p%d" % (c["log_n"], c["log_mem"]))
def test_flow_digest_is_the_same_with_the_switch_on_and_off(cozk, monkeypatch, mode, cfg):
    FL = importlib.import_module("co-zkvms_amd.flow")
    assert "cozk_rw_memory_shared_leaves" in cozk.RW_PROOF_REP3_SYMBOLS  # the switch names calls this library has
    h = FL.FlowHarness(mode=mode, **cfg)
    unset = _prove(h, monkeypatch, None)
    off = _prove(h, monkeypatch, "0")
    on = _prove(h, monkeypatch, "1")
    assert unset == off == on
    h.close()
