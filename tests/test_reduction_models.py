"""CPU tier of the directed reduction tests: the bit-level models of fr_mul_small_add (co-zkvms_amd/csrc/shamir.hip) and of
fr_wide_reduce (co-zkvms_amd/csrc/poly.hip.hpp) against plain big-int arithmetic on the directed operand sets of
tests/reduction_ref.py.  What passes here is what justifies feeding those sets to the device (test_gpu_shamir.py,
test_gpu_shamir_dn.py, test_gpu_prims.py): they do sit on the bounds the kernels' comments argue."""
import pytest

import prims_harness as H
import reduction_ref as X

R = X.R
# what the directed set amounts to (the generator is deterministic): its size, and how many of its cases take q = Q - 1
SMALL_CASES = 5377
SMALL_CASES_LOW_ESTIMATE = 2112


def test_small_multiplier_model_on_the_directed_set():
    """the quotient estimate is Q - 1 or Q (shamir.hip, the comment over fr_mul_small_add) and both happen for every p and Q >= 1"""
    cases = X.small_mul_add_cases()
    low, high = set(), set()
    n_low = 0
    for p, Q, a, c in cases:
        got, q, quot = X.small_mul_add_model(a, p, c)
        assert got == (a * p + c) % R, (p, Q, hex(a), hex(c))
        assert quot in (Q - 1, Q) and q in (quot - 1, quot), (p, Q, quot, q)
        (low if q == quot - 1 else high).add((p, quot))
        n_low += q == quot - 1
    print("small_mul_add_cases: %d cases, %d with q = floor(t / r) - 1" % (len(cases), n_low))
    assert (len(cases), n_low) == (SMALL_CASES, SMALL_CASES_LOW_ESTIMATE)
    want = {(p, Q) for p in range(1, X.SMALL_P_MAX + 1) for Q in range(1, p + 1)}
    assert want <= low and want <= high
    sub = X.small_mul_add_cases(X.small_boundary_deltas)  # the subset of the deeper chains keeps both paths for every (p, Q)
    paths = set()
    for p, _, a, c in sub:
        _, q, quot = X.small_mul_add_model(a, p, c)
        paths.add((p, quot, q == quot))
    assert all((p, Q, True) in paths and (p, Q, False) in paths for p, Q in want)


def test_small_multiplier_model_refuses_a_short_divisor():
    """D without its + 1 overestimates: t - q r goes negative on the directed set, which is what the device test then sees"""
    d, shift = X.SMALL_D - 1, X.SMALL_SHIFT
    assert any(((a * p + c) >> shift) // d > (a * p + c) // R for p, Q, a, c in X.small_mul_add_cases())


def test_wide_reduce_model_at_the_term_counts_of_the_bound():
    """fr_wide_reduce gives N a b / R mod r from one term up to the last N it takes, and even the columns alone (the plainer
    bound, never below) allow the 2^29 terms the comment over FrWide promises, for every canonical pair"""
    e = H.edges(R)
    n_t2 = n_short = 0
    for a in e:
        for b in e:
            nmax, ncol = X.wide_n_max(a, b), X.wide_n_columns(a, b)
            assert ncol >= nmax >= 1 << 29, (hex(a), hex(b), nmax)
            n_short += nmax < ncol
            for n in X.WIDE_N + (nmax,):
                cols = X.wide_columns(a, b, n)
                assert X.wide_value(cols) == n * a * b
                assert X.wide_reduce_model(cols) == n * a * b * X.RINV % R, (hex(a), hex(b), n)
                n_t2 += X.wide_value(cols) >> 512 != 0
    assert n_t2 > 0
    assert 28 * (R - 1) ** 2 >= 1 << 512 > 27 * (R - 1) ** 2  # where the third word starts
    # any operands at all, 2^29 terms: column 7 holds 8 products, and a carry below 2^64 still fits on top of it
    assert (1 << 29) * 8 * ((1 << 32) - 1) ** 2 + (1 << 64) <= X.WIDE_COLUMN_BOUND
    print("wide_n_max is below wide_n_columns for %d of %d pairs" % (n_short, len(e) ** 2))
    assert n_short > 0


def test_wide_reduce_needs_the_carry_inside_the_column_bound():
    """columns below 2^96 are not enough: with the last N the columns alone allow, a column plus the carry into it reaches 2^96
    for some operands, and the chain's 64-bit carry (poly.hip.hpp, fr_wide_reduce) would drop a bit.  wide_n_max is exact"""
    e = H.edges(R)
    pair = next((a, b) for a in e for b in e if X.wide_n_max(a, b) < X.wide_n_columns(a, b))
    with pytest.raises(AssertionError):
        X.wide_reduce_model(X.wide_columns(*pair, X.wide_n_columns(*pair)))
    for a in e:
        for b in e:
            if a and b:
                with pytest.raises(AssertionError):
                    X.wide_reduce_model(X.wide_columns(a, b, X.wide_n_max(a, b) + 1))


def test_wide_reduce_model_on_words_at_multiples_of_r():
    for t0 in (0,) + X.WIDE_WORDS:
        for t1 in (0,) + X.WIDE_WORDS:
            cols = X.wide_columns_of_words(t0, t1)
            assert X.wide_value(cols) == t0 + (t1 << 256)
            assert X.wide_reduce_model(cols) == (t0 + (t1 << 256)) * X.RINV % R
