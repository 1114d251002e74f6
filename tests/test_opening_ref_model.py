"""tests/opening_ref.py (big-int sums over raw Montgomery residues, the PST fold, the Boolean-point indicator) against
oracle/pyref.py's own functions at small sizes: the two expectation routes of the opening round -- the share arithmetic of
O.opening_compute_quadratic term by term, and one dot product over the stored residues -- agree in both share modes, at odd
lengths and with r - 1, 0 and 1 at the ends of each half.  No GPU."""
import pytest

import opening_ref as F
import pyref as O
import reduction_ref as X

R = O.R
EDGES = [R - 1, 0, 1]


def _opening(rng, half, mode):
    """canonical (poly, eq) of length 2 * half with the edge values at the first and last index of each half"""
    n = 2 * half
    a, b, eq = ([rng.field() for _ in range(n)] for _ in range(3))
    for j, i in enumerate((0, half - 1, half, n - 1)):
        a[i], b[i], eq[i] = EDGES[j % 3], EDGES[(j + 1) % 3], EDGES[(j + 2) % 3]
    return (list(zip(a, b)) if mode == "rep3" else a), eq


@pytest.mark.parametrize("half", [1, 2, 3, 257, 1000])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_open_quadratic_routes_agree_with_the_oracle(mode, half):
    rng = O.SplitMix64(7 * half + (mode == "plain"))
    poly, eq = _opening(rng, half, mode)
    want = F.open_quadratic_pyref(poly, eq)
    # the oracle's own round function: one live opening with coefficient 1; its polynomial goes through (0, e0) and (2, e2)
    claim = rng.field()
    uni = O.opening_compute_quadratic([{"poly": poly, "eq": eq, "point_len": 5, "claim": None}], [1], 5, claim)
    assert (O.unipoly_eval(uni, 0), O.unipoly_eval(uni, 2)) == want
    assert O.unipoly_eval(uni, 1) == (claim - want[0]) % R
    if mode == "rep3":
        a, b = F.residues([s[0] for s in poly]), F.residues([s[1] for s in poly])
    else:
        a, b = F.residues(poly), None
    assert F.open_quadratic_raw(a, b, F.residues(eq)) == want


def test_open_quadratic_raw_takes_any_stored_word():
    """the raw route reads the integers as stored: it does not need them reduced (a device vector's are), and a plain polynomial
    is NOT the Rep3 one with b = 0 (no TWO_INV)"""
    rng = O.SplitMix64(3)
    a, eq = [rng.field() for _ in range(10)], [rng.field() for _ in range(10)]
    base = F.open_quadratic_raw(a, None, eq)
    assert F.open_quadratic_raw([x + R for x in a], None, eq) == base
    assert F.open_quadratic_raw(a, [0] * 10, eq) == tuple(v * O.TWO_INV % R for v in base)
    assert F.open_quadratic_raw(a, None, eq) == F.open_quadratic_pyref(F.values(a), F.values(eq))


def test_residues_round_trip_and_match_the_stored_layout():
    rng = O.SplitMix64(4)
    vals = EDGES + [rng.field() for _ in range(20)]
    assert F.values(F.residues(vals)) == vals
    assert F.residues([1]) == [O.R_MONT_ONE]
    assert X.from_raw(X.to_raw(F.residues(vals))) == [O.to_mont(v, R) for v in vals]


@pytest.mark.parametrize("p", [0, 1, R - 1, None])
def test_pst_fold_is_the_loop_body_of_pst_open(p):
    """O.pst_open keeps neither q nor r': its proofs are the MSMs of q over the setup's powers and its value is the last r'"""
    nv = 3
    rng = O.SplitMix64(11)
    ck = O.pst_setup(nv, rng)
    evals = [R - 1] + [rng.field() for _ in range((1 << nv) - 2)] + [R - 1]
    point = [rng.field() if p is None else p] + [rng.field() for _ in range(nv - 1)]
    proofs, value = O.pst_open(ck, evals, point)
    r = evals
    for i, pi in enumerate(point):
        q, r = F.pst_fold(r, pi)
        assert len(q) == len(r) == 1 << (nv - i - 1)
        assert O.msm_naive(ck["powers_of_g"][i], [q[x >> 1] for x in range(1 << (nv - i))]) == proofs[i]
    assert r == [value] == [O.pst_evaluate_le(evals, point)]


def test_boolean_point_gives_the_indicator_of_its_big_endian_index():
    for bits in ([], [1], [0, 1], [1, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0, 1]):
        assert O.eq_evals(bits) == F.indicator(1 << len(bits), F.big_endian_index(bits))
    assert F.big_endian_index([1, 0, 0]) == 4
