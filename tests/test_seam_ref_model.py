"""tests/seam_ref.py (periodic tables: P terms with multiplicities instead of a walk over the table) against the brute-force
oracles of oracle/pyref.py and oracle/pylogup.py run over the expanded tables: every round of a whole sumcheck, the binds in
both orders, plain values and Rep3 shares, lengths below, at and above a multiple of the period (and odd on the way down).
No GPU."""
import pytest

import pylogup as G
import pyref as O
import seam_ref as S

R = O.R
LENGTHS = [300, 1000, 1024]
PERIODS = [7, 49]


def _pattern(rng, P, mode):
    if mode == "rep3":
        return [(rng.field(), rng.field()) for _ in range(P)]
    return [rng.field() for _ in range(P)]


@pytest.mark.parametrize("order", [O.LOW_TO_HIGH, O.HIGH_TO_LOW])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("n", LENGTHS + [2, 3, 49, 98])
def test_bind_both_orders_down_to_one_element(n, P, mode, order):
    rng = O.SplitMix64(n * 5 + P + order)
    table = (_pattern(rng, P, mode), n)
    full = S.expand(table)
    assert len(full) == n and full[:P] == table[0][:n]
    while len(full) > 1:
        r = rng.field()
        table, full = S.bind(table, r, order), O.dense_bind(full, r, order)
        assert table[1] == len(full) and S.expand(table) == full


def test_class_counts_add_up():
    for half in (0, 1, 6, 7, 8, 150, 512):
        for P in PERIODS:
            counts = [S.class_count(half, P, c) for c in range(P)]
            assert counts == [sum(1 for b in range(half) if b % P == c) for c in range(P)]


@pytest.mark.parametrize("mode", ["rep3", "plain"])
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("n", LENGTHS)
def test_prod_round_evals_all_rounds(n, P, mode):
    """m = 3 with the shared factor in the middle, degree 3 and degree 2 of the same tables"""
    rng = O.SplitMix64(n + P)
    tables = [(_pattern(rng, P, "plain"), n), (_pattern(rng, P, mode), n), (_pattern(rng, P, "plain"), n)]
    full = [S.expand(t) for t in tables]
    while len(full[0]) > 1:
        for degree in (3, 2):
            assert S.prod_round_evals(tables, degree) == O.prod_round_evals(full, degree)
        r = rng.field()
        tables = [S.bind(t, r, O.HIGH_TO_LOW) for t in tables]
        full = [O.dense_bind(f, r, O.HIGH_TO_LOW) for f in full]
    assert [S.expand(t) for t in tables] == full


@pytest.mark.parametrize("mode", ["rep3", "plain"])
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("n", LENGTHS)
def test_spartan_rounds_all_rounds(n, P, mode):
    rng = O.SplitMix64(2 * n + P)
    first = [(_pattern(rng, P, mode), n) for _ in range(3)] + [(_pattern(rng, P, "plain"), n)]
    second = [(_pattern(rng, P, mode), n)] + [(_pattern(rng, P, "plain"), n) for _ in range(3)]
    coef = [rng.field(), 0, R - 1]
    f_full, s_full = [S.expand(t) for t in first], [S.expand(t) for t in second]
    while len(f_full[0]) > 1:
        assert S.spartan_first_round_evals(*first) == O.spartan_first_round_evals(*f_full)
        assert S.spartan_second_round_evals(*second, coef) == O.spartan_second_round_evals(*s_full, coef)
        r = rng.field()
        first, second = ([S.bind(t, r, O.LOW_TO_HIGH) for t in ts] for ts in (first, second))
        f_full, s_full = ([O.dense_bind(f, r, O.LOW_TO_HIGH) for f in fs] for fs in (f_full, s_full))
    assert [S.expand(t) for t in first] == f_full and [S.expand(t) for t in second] == s_full


@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("n", LENGTHS)
def test_prodlist_round_all_rounds(n, P):
    """degree 4 with a repeated factor, a one-factor product and the coefficients 0, 1, r - 1"""
    rng = O.SplitMix64(3 * n + P)
    tables = [(_pattern(rng, P, "plain"), n) for _ in range(3)]
    products = [(1, [0, 1, 2, 0]), (R - 1, [1, 1]), (0, [2]), (rng.field(), [2])]
    full = [S.expand(t) for t in tables]
    while len(full[0]) > 1:
        assert S.prodlist_round(tables, products, 4) == G.prove_round(full, products, 4)
        r = rng.field()
        tables = [S.bind(t, r, O.LOW_TO_HIGH) for t in tables]
        full = G.fix_variables(full, r)
    assert [S.expand(t) for t in tables] == full


@pytest.mark.parametrize("mode", ["rep3", "plain"])
@pytest.mark.parametrize("P,ncols", [(7, 4), (49, 8), (49, 7), (7, 1)])
def test_sparse_row_sums(P, ncols, mode):
    """rows that are empty, shorter and longer than the period lcm(P, ncols), starting anywhere in it"""
    rng = O.SplitMix64(P + ncols)
    values = _pattern(rng, P, "plain")
    z = _pattern(rng, ncols, mode)
    row_ptr = [0, 0, 1, 66, 66, 131, 131 + 5 * P * ncols + 3, 131 + 5 * P * ncols + 3, 4000]
    entries = [(r, e % ncols, values[e % P]) for r, (e0, e1) in enumerate(zip(row_ptr, row_ptr[1:])) for e in range(e0, e1)]
    assert S.sparse_row_sums(values, z, row_ptr) == O.sparse_matvec(entries, z, len(row_ptr) - 1)


def test_tiled_dot_matches_the_walk():
    rng = O.SplitMix64(8)
    a, b = _pattern(rng, 49, "plain"), _pattern(rng, 49, "plain")
    for n in (1, 48, 49, 50, 300):
        assert S.tiled_dot(n, a, b) == sum(a[i % 49] * b[i % 49] for i in range(n))
        assert S.tiled_dot(n, a) == sum(a[i % 49] for i in range(n))
