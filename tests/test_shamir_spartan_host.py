"""CPU tests of the protocol claim behind cozk_shamir_spartan_*: co-noir-spartan run by n Shamir parties on their shares
(tests/shamir_spartan_ref.py) gives the plain prover's proof, byte for byte (oracle/pyspartan.py)."""
import pytest

import pyspartan as SP
import shamir_ref as S
import shamir_spartan_ref as SS

R = S.R
CASES = [(3, 5, 3, 1), (3, 5, 5, 2), (1, 9, 7, 3)]  # (log_n, seed, n, t)


@pytest.fixture(scope="module")
def runs():
    return {c: SS.prove(c[0], c[1], c[2], c[3], share_counter=7, rand_counter=11) for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_shamir_proof_is_the_plain_proof(runs, case):
    log_n, seed, n, t = case
    plain = SP.run({"log_n": log_n, "seed": seed})
    assert plain["verified"]
    assert runs[case]["proof_bytes"] == plain["proof_bytes"]
    assert runs[case]["digest"] == plain["digest"]


@pytest.mark.parametrize("case", CASES)
def test_openings_and_finals_shape(runs, case):
    log_n, seed, n, t = case
    out = runs[case]
    assert SS.num_openings(log_n) == 4 * log_n == len(out["msgs"]) == len(out["locals"])
    assert all(len(m) == 2 * t + 1 for m in out["msgs"])
    assert len(out["finals"]) == 3 + 3 * log_n + 2 and all(len(f) == t + 1 for f in out["finals"])
    assert all(len(z) == 4 * log_n for z in out["zero"]) and len(out["zero"]) == 2 * t + 1


@pytest.mark.parametrize("case", CASES)
def test_masks_are_sharings_of_zero_and_hide_the_local_values(runs, case):
    log_n, seed, n, t = case
    out = runs[case]
    lam = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    for m in range(4 * log_n):
        assert S.reconstruct([out["zero"][p][m] for p in range(2 * t + 1)], lam) == 0
        assert out["msgs"][m] != out["locals"][m]
        assert S.reconstruct(out["msgs"][m], lam) == S.reconstruct(out["locals"][m], lam) == out["sc1"][m // 4][m % 4]


def test_2t_senders_do_not_open_the_first_sumcheck(runs):
    log_n, seed, n, t = case = (3, 5, 5, 2)
    out = runs[case]
    lam_short = S.lagrange_from_coeff(list(range(1, 2 * t + 1)))
    for m in (0, 1, 5, 11):
        for src in ("msgs", "locals"):
            assert S.reconstruct(out[src][m][:2 * t], lam_short) != out["sc1"][m // 4][m % 4]
    short = SS.prove(log_n, seed, n, t, share_counter=7, rand_counter=11, first_senders=2 * t)
    assert short["proof_bytes"] != out["proof_bytes"]


def test_counters_change_shares_not_the_proof(runs):
    case = (3, 5, 3, 1)
    other = SS.prove(*case, share_counter=1000, rand_counter=2000)
    assert other["proof_bytes"] == runs[case]["proof_bytes"]
    assert other["msgs"] != runs[case]["msgs"] and other["finals"] != runs[case]["finals"]
