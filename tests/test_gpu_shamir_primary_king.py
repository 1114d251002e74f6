"""GPU tests of the KING construct of the Shamir primary prover (cozk_shamir_primary_prep, cozk_shamir_primary_prove_king): the proof is
the plain prover's, byte for byte (LookupsHarness(mode="plain", primary=True) up to proof_len) and cozk_shamir_primary_prove's of a twin
handle; the finals are the twin's bytes (evaluations of the dealt columns: the construct does not enter), the round messages open to the
twin's; the grouped exchanges (cozk_primary_group_level_king) and the per-sender composition (COZK_SHAMIR_GP_GROUP=0) give the same
bytes; the prep is single-use."""
import importlib

import pytest

import pylookups as PL
import pyref as O
import shamir_primary_king_ref as KR
import shamir_ref as S

pytestmark = pytest.mark.gpu
SWITCH = "COZK_SHAMIR_GP_GROUP"
INVALID = -1
SEED = 6
N_MEM = 54  # as the lookups tests use
PARTIES = [(3, 1), (8, 2), (10, 4)]
SHAPES = [(5, "uniform"), (5, "sha2"), (10, "uniform"), (10, "sha2")]
MIX = {"uniform": 0, "sha2": 1}
COUNTERS = dict(share_counter=7, mul_counter=13, rand_counter=11)


@pytest.fixture(scope="module")
def LK():
    return importlib.import_module("co-zkvms_amd.lookups")


@pytest.fixture(scope="module")
def plain_proofs(LK):
    """the plain lookups harness with the primary phase, once per shape: its proof starts with the primary sumcheck's part"""
    out = {}
    for log_n, mix in SHAPES:
        h = LK.LookupsHarness(mode="plain", log_n=log_n, n_pairs=N_MEM, density_pct=10, seed=SEED, primary=True, mix=mix)
        res = h.prove(verify=True)
        assert res.verified == 1, h.last_error()
        out[(log_n, mix)] = h.proof_bytes(res)
        h.close()
    return out


@pytest.fixture(scope="module")
def plans():
    """the plan restated in Python, once per shape: (X, total)"""
    out = {}
    for log_n, mix in SHAPES:
        n = 1 << log_n
        instrs = PL.instr_table(N_MEM)
        which = [PL.mix_instr(MIX[mix], v) for v in O.synthetic_small(SEED + 1234567, n, 8)]
        rows, total = KR.plan(instrs, [[1 if which[x] == i else 0 for x in range(n)] for i in range(len(instrs))], log_n)
        out[(log_n, mix)] = (len(KR.exchanges(rows)), total)
    return out


def _handle(cozk, log_n, mix, n, t, **kw):
    args = dict(COUNTERS)
    args.update(kw)
    return cozk.ShamirPrimary(log_n=log_n, n_mem=N_MEM, mix=mix, parties=n, degree=t, seed=SEED, **args)


def _stats(h):
    st = h.stats()
    return (st.group_rounds, st.single_rounds, st.group_finals, st.single_finals)


def _opened(msgs, t):
    lam = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    return [S.reconstruct(m, lam) for m in msgs]


@pytest.mark.parametrize("n,t", PARTIES)
@pytest.mark.parametrize("log_n,mix", SHAPES)
def test_king_prove_is_the_plain_and_the_resharing_provers(cozk, plain_proofs, plans, monkeypatch, log_n, mix, n, t):
    X, total = plans[(log_n, mix)]
    twin = _handle(cozk, log_n, mix, n, t)
    want = {}
    for leg in ("1", "0"):  # the resharing prover of the twin handle, grouped and per sender
        monkeypatch.setenv(SWITCH, leg)
        res = twin.prove(verify=True)
        assert res.verified == 1, twin.last_error()
        want[leg] = dict(proof=twin.proof_bytes(res), finals=twin.finals(), opened=_opened(twin.msgs(), t), msgs=twin.msgs(), stats=_stats(twin),
                         nx=(res.n_exchanges, res.n_exchanged))
    twin.close()
    assert want["1"]["proof"] == want["0"]["proof"] == plain_proofs[(log_n, mix)][:len(want["1"]["proof"])]
    assert want["1"]["nx"] == (X, total)
    kings = sorted({0, 2 * t, n - 1})  # the first and the last sender, and (n > 2t + 1) a party above 2t
    assert len(kings) == (3 if n > 2 * t + 1 else 2)
    got = {}
    for king in kings:
        for leg in ("1", "0"):
            monkeypatch.setenv(SWITCH, leg)
            h = _handle(cozk, log_n, mix, n, t)
            pre = h.prep()
            assert (pre.n_openings, pre.pair_elems, pre.n_exchanges, pre.used) == (8 * log_n, total, X, 0) and pre.t_offline_ms > 0
            res = h.prove_king(king=king, verify=True)
            assert res.verified == 1, h.last_error()
            assert h.prep_result().used == 1
            assert res.grouped == int(leg) and res.degree == 8 and res.n_opened == 8 * log_n
            assert (res.n_exchanges, res.n_exchanged) == (X, total) and res.n_exchanged == pre.pair_elems
            proof = h.proof_bytes(res)
            assert proof == want[leg]["proof"] and len(plain_proofs[(log_n, mix)]) > res.proof_len == len(proof)
            assert h.finals() == want[leg]["finals"]
            msgs = h.msgs()
            assert _opened(msgs, t) == want[leg]["opened"] and msgs != want[leg]["msgs"]  # other sharings of the same messages
            assert _stats(h) == want[leg]["stats"]
            assert _stats(h) == ((X + log_n, 0, 0, 0) if leg == "1" else (0, want["0"]["stats"][1], 0, 0)) and _stats(h)[1] % (2 * t + 1) == 0
            got[(king, leg)] = (proof, msgs, h.finals())
            h.close()
    # the king only relays, and the group is the composition: the same bytes whoever is king and either way
    assert all(v == got[(0, "1")] for v in got.values())


def test_a_tampered_opener_share_is_rejected(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    good = _handle(cozk, 5, "uniform", 8, 2)
    good.prep()
    res = good.prove_king(king=3)
    want = good.proof_bytes(res)
    good.close()
    for k in (1, 3 * 7 + 2, (N_MEM + 1) * 3):  # E_0 at opener 0, E_7 at opener 1, lookup_outputs at opener 2
        h = _handle(cozk, 5, "uniform", 8, 2, tamper_final=k)
        h.prep()
        bad = h.prove_king(king=3, verify=True)
        assert bad.verified == 0 and "verification failed" in h.last_error()
        assert h.proof_bytes(bad) != want
        h.close()


def test_prep_misuse_is_refused_before_any_launch(cozk, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    h = _handle(cozk, 5, "uniform", 5, 2)

    def refused(text, fn):
        with pytest.raises(cozk.CozkError) as e:
            fn()
        assert e.value.code == INVALID and text in str(e.value), str(e.value)

    assert h.prep_result().used == 0 and h.prep_result().pair_elems == 0
    refused("shamir_primary_prove_king: no preprocessing", lambda: h.prove_king(king=0))
    assert _stats(h) == (0, 0, 0, 0)  # nothing ran
    pre = h.prep()
    refused("shamir_primary_prep: the harness has been preprocessed", h.prep)
    for king in (-1, 5, 32):
        refused("shamir_primary_prove_king: 0 <= king < num_parties", lambda: h.prove_king(king=king))
    assert h.prep_result().used == 0  # a refused call consumes nothing
    res = h.prove_king(king=4)
    assert res.verified == 1 and res.n_exchanged == pre.pair_elems
    proof = h.proof_bytes(res)
    refused("shamir_primary_prove_king: the preprocessing has been used (a pair must never be used twice)", lambda: h.prove_king(king=4))
    assert h.prep_result().used == 1
    again = h.prove(verify=True)  # the resharing prover of the same handle still runs, and gives the same proof
    assert again.verified == 1 and h.proof_bytes(again) == proof
    h.close()


def test_senders_on_two_gpus_take_the_per_sender_path(cozk, plain_proofs, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    monkeypatch.delenv(SWITCH, raising=False)
    log_n, mix, n, t = 5, "uniform", 8, 2
    for king in (0, 1, n - 1):  # a king beside sender 0, one on the other device, a party above 2t
        h = _handle(cozk, log_n, mix, n, t, devices=[p % 2 for p in range(n)])
        h.prep()
        res = h.prove_king(king=king)
        assert res.verified == 1 and res.grouped == 0, h.last_error()
        assert h.proof_bytes(res) == plain_proofs[(log_n, mix)][:res.proof_len]
        assert _stats(h)[0] == 0 and _stats(h)[1] > 0
        h.close()
