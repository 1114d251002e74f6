"""CPU tests of the protocol claim behind cozk_shamir_jolt_spartan_*: co-jolt's Spartan worker run by n Shamir parties on their
shares (tests/shamir_jolt_spartan_ref.py) gives the plain prover's proof, byte for byte (oracle/pyspartan_outer.py run_full)."""
import pytest

import pyref as O
import pyspartan_outer as SO
import shamir_jolt_spartan_ref as JS
import shamir_ref as S

R = S.R
SHAPES = [("toy", 2), ("toy", 4), ("jolt", 0), ("jolt", 1), ("jolt", 3)]
PARTIES = [(3, 1), (5, 2), (8, 2)]
SEED = 5
CASES = [(system, log_steps, n, t) for system, log_steps in SHAPES for n, t in PARTIES]


@pytest.fixture(scope="module")
def plain():
    out = {}
    for system, log_steps in SHAPES:
        out[(system, log_steps)] = SO.run_full(dict(mode="plain", log_steps=log_steps, seed=SEED, system=system))
        assert out[(system, log_steps)]["verified"]
    return out


@pytest.fixture(scope="module")
def runs():
    return {c: JS.prove(c[0], c[1], SEED, c[2], c[3], share_counter=7, rand_counter=11) for c in CASES}


def _plain_cubics(proof):
    """the plain prover's four coefficients per outer round, from the compressed polynomials and the running claim"""
    tr = O.Transcript(b"cozk-spartan")
    tr.challenge_vector(len(proof["outer"]["round_polys"]))
    claim, out = 0, []
    for comp in proof["outer"]["round_polys"]:
        poly = [comp[0], (claim - 2 * comp[0] - sum(comp[1:])) % R] + list(comp[1:])
        tr.append_scalars(comp)
        claim = O.unipoly_eval(poly, tr.challenge_scalar())
        out.append(poly)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-n%d-t%d" % c)
def test_shamir_proof_is_the_plain_proof(runs, plain, case):
    ref = plain[case[:2]]
    assert runs[case]["proof_bytes"] == ref["proof_bytes"]
    assert runs[case]["digest"] == ref["digest"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-n%d-t%d" % c)
def test_openings_and_finals_shape(runs, case):
    system, log_steps, n, t = case
    out = runs[case]
    M = JS.num_openings(system, log_steps)
    assert M == len(out["msgs"]) == len(out["locals"]) == 4 * len(out["proof"]["outer"]["round_polys"])
    assert all(len(m) == 2 * t + 1 for m in out["msgs"])
    assert len(out["finals"]) == JS.finals_len(system, log_steps) and all(len(f) == t + 1 for f in out["finals"])
    assert len(out["zero"]) == 2 * t + 1 and all(len(z) == M for z in out["zero"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-n%d-t%d" % c)
def test_locals_are_degree_2t_sharings_of_the_plain_coefficients(runs, plain, case):
    system, log_steps, n, t = case
    out = runs[case]
    cubics = _plain_cubics(plain[case[:2]]["proof"])
    lam2 = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    lam1 = S.lagrange_from_coeff(list(range(1, t + 2)))
    checked = 0
    for m, loc in enumerate(out["locals"]):
        want = cubics[m // 4][m % 4]
        assert S.reconstruct(loc, lam2) == want
        assert S.reconstruct([out["zero"][p][m] for p in range(2 * t + 1)], lam2) == 0
        assert S.reconstruct(out["msgs"][m], lam2) == want and out["msgs"][m] != loc
        if m == 0:  # the first round's t(0) is 0 at every party: the constant sharing of the plain prover's 0
            assert loc == [0] * (2 * t + 1) and want == 0
        elif want != 0:  # a coefficient that carries t(0) or t(inf), sums of products of two shares, with Az Bz != 0
            assert S.reconstruct(loc[:t + 1], lam1) != want
            checked += 1
    # the single step of (jolt, 0) has Az Bz = 0 in its first round (the plain cubic is 0 there); at every other shape only m = 0 is 0
    if (system, log_steps) != ("jolt", 0):
        assert checked == len(out["locals"]) - 1
    assert checked >= len(out["locals"]) - 7


@pytest.mark.parametrize("case", [("jolt", 1, 5, 2), ("toy", 2, 3, 1)])
def test_2t_senders_do_not_open_the_outer_messages(runs, plain, case):
    system, log_steps, n, t = case
    out = runs[case]
    cubics = _plain_cubics(plain[case[:2]]["proof"])
    lam_short = S.lagrange_from_coeff(list(range(1, 2 * t + 1)))
    for m in (1, 2, 3, 5, 11):
        for src in ("msgs", "locals"):
            assert S.reconstruct(out[src][m][:2 * t], lam_short) != cubics[m // 4][m % 4]
    short = JS.prove(system, log_steps, SEED, n, t, share_counter=7, rand_counter=11, first_senders=2 * t)
    assert short["outer_polys"][0] != cubics[0]
    assert short["proof_bytes"] != out["proof_bytes"]


def test_counters_change_shares_not_the_proof(runs):
    case = ("jolt", 1, 3, 1)
    base = runs[case]
    shares = JS.prove(*case[:2], SEED, *case[2:], share_counter=1000, rand_counter=11)
    masks = JS.prove(*case[:2], SEED, *case[2:], share_counter=7, rand_counter=2000)
    for other in (shares, masks):
        assert other["proof_bytes"] == base["proof_bytes"]
        assert other["msgs"] != base["msgs"]
    assert shares["finals"] != base["finals"] and shares["locals"] != base["locals"]
    assert masks["finals"] == base["finals"] and masks["locals"] == base["locals"] and masks["zero"] != base["zero"]


def test_dense_cz_is_not_the_product_of_the_shares():
    """why the restatement evaluates Cz from its own linear combination: on shares Cz_p != Az_p Bz_p, in the clear Cz = Az Bz"""
    uniform, cross, padded, clear, is_public = JS.instance("toy", SEED, 1)
    cols = JS.party_columns(clear, is_public, SEED, 3, 1, 0)
    az, bz, cz = JS.dense_azbzcz(uniform, cross, padded, clear, 2)
    assert (az, bz, cz) == tuple(SO.dense_azbzcz(uniform, cross, clear, padded, 2))
    pa, pb, pc = JS.dense_azbzcz(uniform, cross, padded, cols[0], 2)
    assert pc[0] != pa[0] * pb[0] % R and cz[0] == az[0] * bz[0] % R
    lam = S.lagrange_from_coeff([1, 2])
    per = [JS.dense_azbzcz(uniform, cross, padded, cols[p], 2) for p in range(2)]
    for q, clear_q in enumerate((az, bz, cz)):
        assert [S.reconstruct([per[p][q][i] for p in range(2)], lam) for i in range(2 * padded)] == clear_q
