"""GPU tests of co-noir-spartan proved by n Shamir parties (cozk_shamir_spartan_*): the proof is the plain prover's, byte for byte
(oracle/pyspartan.py, SpartanHarness(mode="plain")); msgs and finals are those of the big-int restatement tests/shamir_spartan_ref.py;
the grouped rounds (cozk_spartan_group_*) and the per-poly rounds (COZK_SHAMIR_GP_GROUP=0) give the same bytes."""
import hashlib

import pytest

import pyspartan as SP
import shamir_spartan_ref as SS

pytestmark = pytest.mark.gpu
SWITCH = "COZK_SHAMIR_GP_GROUP"
INVALID = -1


@pytest.fixture(scope="module")
def plain_proofs():
    return {(log_n, seed): SP.run({"log_n": log_n, "seed": seed}) for log_n, seed in ((3, 5), (6, 7))}


def _prove(cozk, log_n, seed, n, t, devices=0, **kw):
    h = cozk.ShamirSpartanHarness(log_n=log_n, parties=n, degree=t, devices=devices, seed=seed, **kw)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    return h, res


@pytest.mark.parametrize("n,t", [(3, 1), (5, 2), (8, 2)])
@pytest.mark.parametrize("log_n,seed", [(3, 5), (6, 7)])
def test_proof_is_the_plain_provers(cozk, plain_proofs, monkeypatch, log_n, seed, n, t):
    monkeypatch.delenv(SWITCH, raising=False)
    h, res = _prove(cozk, log_n, seed, n, t)
    want = plain_proofs[(log_n, seed)]
    assert want["verified"]
    assert h.proof_bytes(res) == want["proof_bytes"]
    assert bytes(res.proof_digest).hex() == want["digest"]
    assert res.grouped == 1 and res.n_opened == 4 * log_n
    st = h.stats()
    assert (st.group_rounds, st.single_rounds, st.group_finals, st.single_finals) == (2 * log_n, 0, 2, 0)
    h.close()


def test_msgs_and_finals_are_the_restatements(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    log_n, seed, n, t = 3, 5, 5, 2
    ref = SS.prove(log_n, seed, n, t, share_counter=7, rand_counter=11)
    h, res = _prove(cozk, log_n, seed, n, t, share_counter=7, rand_counter=11)
    assert h.proof_bytes(res) == ref["proof_bytes"]
    assert h.msgs() == ref["msgs"]
    assert h.finals() == ref["finals"]
    assert len(h.msgs()) == 4 * log_n and len(h.finals()) == 3 * log_n + 5
    h.close()


def test_multi_workgroup_rounds_at_2p13(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    log_n, seed = 13, 21
    plain = cozk.SpartanHarness(mode="plain", log_n=log_n, seed=seed)
    pres = plain.prove(verify=True)
    assert pres.verified == 1
    want = bytes(pres.proof_digest)
    plain.close()
    h, res = _prove(cozk, log_n, seed, 8, 2)
    assert bytes(res.proof_digest) == want and res.grouped == 1
    again = h.prove(verify=True)
    assert again.verified == 1 and bytes(again.proof_digest) == want
    assert hashlib.sha256(h.proof_bytes(again)).digest() == want
    h.close()


@pytest.mark.parametrize("log_n,seed,n,t", [(6, 7, 5, 2), (12, 9, 3, 1)])
def test_grouped_and_per_poly_rounds_give_the_same_bytes(cozk, monkeypatch, log_n, seed, n, t):
    h = cozk.ShamirSpartanHarness(log_n=log_n, parties=n, degree=t, seed=seed)
    monkeypatch.delenv(SWITCH, raising=False)
    res_g = h.prove(verify=True)
    got_g = (h.proof_bytes(res_g), h.msgs(), h.finals())
    st = h.stats()
    assert res_g.verified == 1 and res_g.grouped == 1
    assert (st.group_rounds, st.single_rounds, st.group_finals, st.single_finals) == (2 * log_n, 0, 2, 0)
    monkeypatch.setenv(SWITCH, "0")
    res_s = h.prove(verify=True)
    got_s = (h.proof_bytes(res_s), h.msgs(), h.finals())
    st = h.stats()
    assert res_s.verified == 1 and res_s.grouped == 0
    assert (st.group_rounds, st.single_rounds, st.group_finals, st.single_finals) == (0, (2 * t + 1) * log_n + (t + 1) * log_n, 0, 2 * (t + 1))
    assert got_g == got_s
    monkeypatch.setenv(SWITCH, "1")
    res_b = h.prove(verify=True)  # and back
    assert res_b.grouped == 1 and h.proof_bytes(res_b) == got_g[0]
    h.close()


@pytest.mark.parametrize("kw,text", [
    (dict(parties=3, degree=0), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(parties=17, degree=8), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(parties=4, degree=2), "2 * degree + 1 <= num_parties"),
    (dict(parties=33, degree=1), "num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(parties=3, degree=1, log_n=0), "log_n out of range"),
    (dict(parties=3, degree=1, log_n=25), "log_n out of range"),
])
def test_refused_configurations(cozk, kw, text):
    args = dict(log_n=3, seed=1)
    args.update(kw)
    with pytest.raises(cozk.CozkError) as e:
        cozk.ShamirSpartanHarness(**args)
    assert e.value.code == INVALID and "shamir_spartan: " in str(e.value) and text in str(e.value)


def test_senders_on_two_gpus_take_the_per_poly_path(cozk, plain_proofs, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    monkeypatch.delenv(SWITCH, raising=False)
    log_n, seed, n, t = 6, 7, 5, 2
    h, res = _prove(cozk, log_n, seed, n, t, devices=[p % 2 for p in range(n)])
    assert h.proof_bytes(res) == plain_proofs[(log_n, seed)]["proof_bytes"] and res.grouped == 0
    st = h.stats()
    assert (st.group_rounds, st.single_rounds) == (0, (2 * t + 1) * log_n + (t + 1) * log_n)
    h.close()
