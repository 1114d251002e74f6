"""GPU: the chained flow's phase 2 with its leaves made by the two fused calls (COZK_BYTECODE_FUSED=1, csrc/host/flow_harness.hpp:
cozk_bytecode_leaves and cozk_bytecode_init_final_leaves over the flow's compact columns and its V_IMM polynomial) gives, byte for
byte, the proof of the four cozk_fingerprint_leaves launches, in plain and rep3 mode -- the REP3 path of the kernels under a real
caller, the public part entering the shares through add_public."""
import importlib

import pytest

pytestmark = pytest.mark.gpu
CONFIGS = [dict(log_n=3, log_m=3, log_b=2, log_mem=3, n_mem=6, n_subtables=3, seed=5),
           dict(log_n=5, log_m=3, log_b=4, log_mem=4, n_mem=9, n_subtables=4, seed=7)]  # two of test_gpu_flow.py's


def _prove(h, monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("COZK_BYTECODE_FUSED", raising=False)
    else:
        monkeypatch.setenv("COZK_BYTECODE_FUSED", switch)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    return res


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "2p%d-2p%d" % (c["log_n"], c["log_b"]))
def test_flow_digest_is_the_same_with_the_switch_on_and_off(cozk, monkeypatch, mode, cfg):
    FL = importlib.import_module("co-zkvms_amd.flow")
    assert "cozk_bytecode_leaves" in cozk.BYTECODE_SYMBOLS  # the switch names calls this library has
    h = FL.FlowHarness(mode=mode, **cfg)
    unset = _prove(h, monkeypatch, None)
    off = _prove(h, monkeypatch, "0")
    on = _prove(h, monkeypatch, "1")
    assert bytes(unset.proof_digest) == bytes(off.proof_digest) == bytes(on.proof_digest)
    assert h.proof_bytes(on) == h.proof_bytes(off)
    h.close()
