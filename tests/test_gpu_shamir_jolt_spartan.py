"""GPU tests of co-jolt's Spartan worker proved by n Shamir parties (cozk_shamir_jolt_spartan_*): the proof is the plain prover's,
byte for byte (oracle/pyspartan_outer.py run_full, OuterHarness(mode="plain", full=True)); msgs and finals are those of the big-int
restatement tests/shamir_jolt_spartan_ref.py; the grouped rounds (cozk_outer_group_*, cozk_shift_group_*) and the per-sender rounds
(COZK_SHAMIR_GP_GROUP=0) give the same bytes."""
import hashlib
import importlib

import pytest

import pyspartan_outer as SO
import shamir_jolt_spartan_ref as JS

pytestmark = pytest.mark.gpu
SWITCH = "COZK_SHAMIR_GP_GROUP"
INVALID = -1
SEED = 5
SHAPES = [("toy", 2), ("toy", 4), ("jolt", 0), ("jolt", 1), ("jolt", 3)]


def _bits(system):
    return 7 if system == "jolt" else 3


@pytest.fixture(scope="module")
def plain_proofs():
    return {s: SO.run_full(dict(mode="plain", log_steps=s[1], seed=SEED, system=s[0])) for s in SHAPES}


def _prove(cozk, system, log_steps, seed, n, t, devices=0, **kw):
    h = cozk.ShamirJoltSpartanHarness(log_steps=log_steps, system=system, parties=n, degree=t, devices=devices, seed=seed, **kw)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    return h, res


def _grouped_stats(system, log_steps):
    return (log_steps + _bits(system) + log_steps, 0, 2 if log_steps else 1, 0)


def _single_stats(system, log_steps, t):
    return (0, (2 * t + 1) * (log_steps + _bits(system)) + (t + 1) * log_steps, 0, (2 if log_steps else 1) * (t + 1))


def _stats(h):
    st = h.stats()
    return (st.group_rounds, st.single_rounds, st.group_finals, st.single_finals)


@pytest.mark.parametrize("n,t", [(3, 1), (5, 2), (8, 2)])
@pytest.mark.parametrize("system,log_steps", SHAPES)
def test_proof_is_the_plain_provers(cozk, plain_proofs, monkeypatch, system, log_steps, n, t):
    monkeypatch.delenv(SWITCH, raising=False)
    h, res = _prove(cozk, system, log_steps, SEED, n, t)
    want = plain_proofs[(system, log_steps)]
    assert want["verified"]
    assert h.proof_bytes(res) == want["proof_bytes"]
    assert bytes(res.proof_digest).hex() == want["digest"]
    assert res.grouped == 1 and res.n_opened == 4 * (log_steps + _bits(system))
    assert _stats(h) == _grouped_stats(system, log_steps)
    h.close()


@pytest.mark.parametrize("system,log_steps,n,t,sc,rc", [("jolt", 3, 5, 2, 7, 11), ("toy", 2, 3, 1, 0, 0)])
def test_msgs_and_finals_are_the_restatements(cozk, monkeypatch, system, log_steps, n, t, sc, rc):
    monkeypatch.delenv(SWITCH, raising=False)
    ref = JS.prove(system, log_steps, SEED, n, t, share_counter=sc, rand_counter=rc)
    h, res = _prove(cozk, system, log_steps, SEED, n, t, share_counter=sc, rand_counter=rc)
    assert h.proof_bytes(res) == ref["proof_bytes"]
    assert h.msgs() == ref["msgs"]
    assert h.finals() == ref["finals"]
    assert len(h.msgs()) == JS.num_openings(system, log_steps) and len(h.finals()) == JS.finals_len(system, log_steps)
    h.close()


@pytest.mark.parametrize("system,log_steps,n,t", [("jolt", 6, 5, 2), ("toy", 10, 3, 1)])
def test_grouped_and_per_sender_rounds_give_the_same_bytes(cozk, monkeypatch, system, log_steps, n, t):
    h = cozk.ShamirJoltSpartanHarness(log_steps=log_steps, system=system, parties=n, degree=t, seed=9)
    monkeypatch.delenv(SWITCH, raising=False)
    res_g = h.prove(verify=True)
    got_g = (h.proof_bytes(res_g), h.msgs(), h.finals())
    assert res_g.verified == 1 and res_g.grouped == 1, h.last_error()
    assert _stats(h) == _grouped_stats(system, log_steps)
    monkeypatch.setenv(SWITCH, "0")
    res_s = h.prove(verify=True)
    got_s = (h.proof_bytes(res_s), h.msgs(), h.finals())
    assert res_s.verified == 1 and res_s.grouped == 0, h.last_error()
    assert _stats(h) == _single_stats(system, log_steps, t)
    assert got_g == got_s
    monkeypatch.setenv(SWITCH, "1")
    res_b = h.prove(verify=True)  # and back
    assert res_b.grouped == 1 and h.proof_bytes(res_b) == got_g[0] and h.msgs() == got_g[1] and h.finals() == got_g[2]
    h.close()


def test_past_one_workgroup_at_2p10_jolt(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    OU = importlib.import_module("co-zkvms_amd.outer")
    log_steps, seed = 10, 21
    plain = OU.OuterHarness(mode="plain", log_steps=log_steps, seed=seed, system="jolt", full=True)
    pres = plain.prove(verify=True)
    assert pres.verified == 1
    want = bytes(pres.proof_digest)
    plain.close()
    h, res = _prove(cozk, "jolt", log_steps, seed, 8, 2)
    assert bytes(res.proof_digest) == want and res.grouped == 1
    again = h.prove(verify=True)
    assert again.verified == 1 and bytes(again.proof_digest) == want
    assert hashlib.sha256(h.proof_bytes(again)).digest() == want
    h.close()


def test_seven_senders(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    system, log_steps, n, t = "jolt", 4, 7, 3
    want = SO.run_full(dict(mode="plain", log_steps=log_steps, seed=SEED, system=system))
    h, res = _prove(cozk, system, log_steps, SEED, n, t)
    assert h.proof_bytes(res) == want["proof_bytes"] and res.grouped == 1
    assert _stats(h) == _grouped_stats(system, log_steps)
    assert all(len(m) == 7 for m in h.msgs()) and all(len(f) == 4 for f in h.finals())
    h.close()


@pytest.mark.parametrize("kw,text", [
    (dict(parties=3, degree=0), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(parties=17, degree=8), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(parties=4, degree=2), "2 * degree + 1 <= num_parties"),
    (dict(parties=33, degree=1), "num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(parties=3, degree=1, log_steps=-1), "log_steps out of range (0..24)"),
    (dict(parties=3, degree=1, log_steps=25), "log_steps out of range (0..24)"),
    (dict(parties=3, degree=1, system=2), "system is 0 (toy) or 1"),
])
def test_refused_configurations(cozk, kw, text):
    args = dict(log_steps=3, seed=1)
    args.update(kw)
    with pytest.raises(cozk.CozkError) as e:
        cozk.ShamirJoltSpartanHarness(**args)
    assert e.value.code == INVALID and "shamir_jolt_spartan: " in str(e.value) and text in str(e.value)


def test_senders_on_two_gpus_take_the_per_sender_path(cozk, plain_proofs, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    monkeypatch.delenv(SWITCH, raising=False)
    system, log_steps, n, t = "jolt", 3, 5, 2
    h, res = _prove(cozk, system, log_steps, SEED, n, t, devices=[p % 2 for p in range(n)])
    assert h.proof_bytes(res) == plain_proofs[(system, log_steps)]["proof_bytes"] and res.grouped == 0
    assert _stats(h) == _single_stats(system, log_steps, t)
    h.close()
