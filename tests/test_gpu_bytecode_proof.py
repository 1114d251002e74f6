"""GPU tests of the bytecode proof harness (cozk_bytecode_proof_*, csrc/host/bytecode_proof.hpp): the proof bytes equal
tests/bytecode_ref.py's prove at small sizes with the table shorter and longer than the trace; either leaves path verifies and gives one
digest at 2^10 and 2^16 steps; each tamper is rejected with its reason; two proves of one handle give the same bytes; bad configs are
refused."""
import functools
import hashlib
import importlib

import pytest

import bytecode_ref as B

pytestmark = pytest.mark.gpu
INVALID_ARG = -1


@pytest.fixture(scope="module")
def BC():
    return importlib.import_module("co-zkvms_amd.bytecode")


@functools.lru_cache(maxsize=None)
def _ref(log_n, log_b, seed):
    cfg = dict(log_n=log_n, log_b=log_b, seed=seed)
    p = B.prove(cfg)
    assert B.verify(p, cfg)[0]
    return p["proof_bytes"]


@pytest.mark.parametrize("log_n,log_b", [(1, 1), (3, 5), (6, 3), (6, 5)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composition"])
def test_proof_bytes_equal_the_python_restatement(cozk, BC, log_n, log_b, fused):
    h = BC.BytecodeProof(log_n=log_n, log_b=log_b, seed=3, leaves_fused=fused)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert hashlib.sha256(got).hexdigest() == bytes(res.proof_digest).hex() and int(res.proof_len) == len(got)
    assert got == _ref(log_n, log_b, 3)
    h.close()


@pytest.mark.parametrize("log_n,log_b", [(10, 10), (16, 14)])
def test_either_leaves_path_verifies_with_one_digest(cozk, BC, log_n, log_b):
    digs = []
    for fused in (True, False):
        h = BC.BytecodeProof(log_n=log_n, log_b=log_b, seed=2026, leaves_fused=fused)
        res = h.prove(verify=True)
        assert res.verified == 1, h.last_error()
        digs.append(bytes(res.proof_digest))
        h.close()
    assert digs[0] == digs[1]


@pytest.mark.parametrize("log_n", [6, 16])
@pytest.mark.parametrize("tamper,reason", [(1, B.REASON_MULTISET), (2, B.REASON_LEAF), (3, B.REASON_MULTISET)])
def test_tampers_are_rejected_with_their_reasons(cozk, BC, log_n, tamper, reason):
    h = BC.BytecodeProof(log_n=log_n, log_b=log_n - 2, seed=9, tamper=tamper)
    res = h.prove(verify=True)
    assert res.verified == 0 and h.last_error().startswith("verification failed: " + reason + ":"), h.last_error()
    if log_n == 6:  # the restatement rejects for the same reason, and its bytes are the harness's
        cfg = dict(log_n=log_n, log_b=log_n - 2, seed=9, tamper=tamper)
        p = B.prove(cfg)
        assert B.verify(p, cfg)[1] == reason and p["proof_bytes"] == h.proof_bytes(res)
    h.close()


def test_two_proves_of_one_handle_give_equal_bytes(cozk, BC):
    h = BC.BytecodeProof(log_n=8, log_b=9, seed=5)
    r1 = h.prove(verify=True)
    b1 = h.proof_bytes(r1)
    r2 = h.prove(verify=False)
    assert r1.verified == 1 and r2.verified == -1 and h.proof_bytes(r2) == b1 and bytes(r1.proof_digest) == bytes(r2.proof_digest)
    h.close()


@pytest.mark.parametrize("kw,text", [(dict(mode="rep3"), "mode is COZK_MODE_PLAIN"), (dict(log_n=0), "log_n in 1..22"), (dict(log_n=23), "log_n in 1..22"),
                                     (dict(log_b=0), "log_b in 1..22"), (dict(log_b=23), "log_b in 1..22"), (dict(tamper=4), "tamper in 0..3")])
def test_bad_configs_are_refused(cozk, BC, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        BC.BytecodeProof(**dict(dict(log_n=4, log_b=4), **kw))
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
