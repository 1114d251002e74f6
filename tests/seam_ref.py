"""Exact references at lengths that plain big-int loops cannot reach in seconds: PERIODIC tables.

A table is (pattern, length): element i is pattern[i % P] with P = len(pattern); an entry is an int (plain value) or an
(a, b) tuple (Rep3 share).  Every table of one call has the same P and the same length.

A sumcheck round pairs elements -- LowToHigh (2b, 2b + 1), HighToLow (b, b + half), half = length // 2 -- and the pair at
index b depends only on c = b % P: LowToHigh reads pattern[2c % P] and pattern[(2c + 1) % P] (and, 2 being invertible mod an
odd P, the P classes are P different pairs), HighToLow reads pattern[c] and pattern[(c + half) % P].  So
  * a round's sums are the P terms of one period, each times the number of b < half in its class, and
  * the bound table is periodic again with the same P (length half),
and a whole sumcheck -- every round message, the final values -- is followed at any length at a cost of P terms per round.
The term of one class is the brute-force oracle's own formula run on the two-element table [lo, hi]; what this module adds
is the counting, which tests/test_seam_ref_model.py checks against the oracles run over the expanded tables.

P = 49 is coprime to every grid stride of the kernels (a power of two times 3), so a lane walks through the whole pattern.
Plain Python and numpy, no GPU."""
import numpy as np

import prims_harness as H
import pylogup as G
import pyref as O
import reduction_ref as X

R = O.R
LOW_TO_HIGH, HIGH_TO_LOW = O.LOW_TO_HIGH, O.HIGH_TO_LOW
PERIOD = 49


def expand(table):
    pattern, length = table
    return [pattern[i % len(pattern)] for i in range(length)]


def pair(table, c, order):
    """(lo, hi) of every pair index b with b % P == c"""
    pattern, length = table
    P = len(pattern)
    if order == LOW_TO_HIGH:
        return pattern[2 * c % P], pattern[(2 * c + 1) % P]
    return pattern[c % P], pattern[(c + length // 2) % P]


def class_count(half, P, c):
    """how many b in [0, half) have b % P == c"""
    return half // P + (c < half % P)


def bind(table, r, order):
    """dense_bind of the whole table: (pattern of the bound table, length // 2)"""
    pattern, length = table
    out = []
    for c in range(len(pattern)):
        lo, hi = pair(table, c, order)
        out.append(O.sh_add(lo, O.sh_mul_public(O.sh_sub(hi, lo), r)))
    return out, length // 2


def _scaled(v, k):
    return O.sh_mul_public(v, k % R)


def _round(tables, order, term):
    """sum over the classes of count * term([[lo, hi] of every table]); term returns a list of ints or shares"""
    P, length = len(tables[0][0]), tables[0][1]
    assert all(len(p) == P and n == length for p, n in tables)
    half = length // 2
    total = None
    for c in range(min(P, half)):
        t = [_scaled(v, class_count(half, P, c)) for v in term([list(pair(tb, c, order)) for tb in tables])]
        total = t if total is None else [O.sh_add(x, y) for x, y in zip(total, t)]
    return total


def prod_round_evals(tables, degree):
    """O.prod_round_evals (HighToLow) of the expanded tables"""
    return _round(tables, HIGH_TO_LOW, lambda two: O.prod_round_evals(two, degree))


def spartan_first_round_evals(za, zb, zc, pub):
    """O.spartan_first_round_evals (LowToHigh) of the expanded tables"""
    return _round([za, zb, zc, pub], LOW_TO_HIGH, lambda two: O.spartan_first_round_evals(*two))


def spartan_second_round_evals(z, pa, pb, pc, coef):
    """O.spartan_second_round_evals (LowToHigh) of the expanded tables"""
    return _round([z, pa, pb, pc], LOW_TO_HIGH, lambda two: O.spartan_second_round_evals(*two, coef))


def prodlist_round(tables, products, degree):
    """pylogup.prove_round (LowToHigh) of the expanded tables"""
    return _round(tables, LOW_TO_HIGH, lambda two: G.prove_round(two, products, degree))


def sparse_row_sums(values, z, row_ptr):
    """rows of a CSR matrix whose entry e has value values[e % P] and column e % len(z): [sum_{e in row} z[col e] * value e],
    O.sparse_matvec's rows.  The terms repeat with period L = lcm(P, len(z)); prefix sums over one period give every row."""
    P, nc = len(values), len(z)
    L = P * nc // np.gcd(P, nc).item()
    prefix = [O.sh_zero(z[0])]
    for t in range(L):
        prefix.append(O.sh_add(prefix[-1], O.sh_mul_public(z[t % nc], values[t % P])))

    def upto(e):  # the sum over entries 0 .. e - 1
        return O.sh_add(_scaled(prefix[L], e // L), prefix[e % L])

    return [O.sh_sub(upto(e1), upto(e0)) for e0, e1 in zip(row_ptr, row_ptr[1:])]


# ------------------------------------------------------------------------------------------------ periodic vectors on the device
def tiled(ctx, cozk, pattern, n):
    """a device FR vector of n elements whose RAW words repeat `pattern` (Vec.from_numpy: no Montgomery conversion, the device
    multiplies exactly these residues)"""
    return cozk.Vec.from_numpy(ctx, np.resize(X.to_raw(pattern), (n, 4)))


def tiled_dot(n, *patterns):
    """sum_{i < n} prod_k patterns[k][i mod period] for patterns of one period, the sum of products in big ints"""
    period = len(patterns[0])
    total = 0
    for j in range(period):
        term = (n // period) + (j < n % period)
        for p in patterns:
            term *= p[j]
        total += term
    return total


def wide_pattern(seed):
    """r - 1, a primitive-harness edge, a random residue, ... : 16 triples and one more r - 1"""
    rng = O.SplitMix64(seed)
    pat = [v for e in H.edges(R) for v in (R - 1, e, rng.field())] + [R - 1]
    assert len(pat) == PERIOD
    return pat


def wide_inputs(fill, mode, seed, eval_sum):
    """(a, b, public) patterns: all r - 1, or mixed.  Where the kernel multiplies a + b (eval_sum) the all-(r - 1) run keeps b
    at zero so that the factor itself is r - 1"""
    one = [R - 1] * PERIOD
    if fill == "all_r_minus_1":
        return one, ([0] * PERIOD if eval_sum else one) if mode == "rep3" else None, one
    a, b, pub = wide_pattern(seed), wide_pattern(seed + 1)[::-1], wide_pattern(seed + 2)
    pub = pub[5:] + pub[:5]  # r - 1 meets r - 1, an edge and a random value
    return a, b if mode == "rep3" else None, pub


def wide_poly(cozk, ctx, a, b, n):
    return cozk.Rep3DensePolynomial.from_vec_shares(ctx, tiled(ctx, cozk, a, n), tiled(ctx, cozk, b, n) if b is not None else None)


def tiled_values(ctx, cozk, pattern, n):
    """a device FR vector of n elements whose VALUES repeat the canonical `pattern` (its Montgomery words, tiled)"""
    return tiled(ctx, cozk, [v * X.MONT % R for v in pattern], n)


def tiled_poly(ctx, cozk, table):
    """the table as a device polynomial: Rep3 if its entries are shares"""
    pattern, n = table
    if isinstance(pattern[0], tuple):
        return cozk.Rep3DensePolynomial.from_vec_shares(ctx, tiled_values(ctx, cozk, [s[0] for s in pattern], n),
                                                        tiled_values(ctx, cozk, [s[1] for s in pattern], n))
    return cozk.Rep3DensePolynomial.from_vec_shares(ctx, tiled_values(ctx, cozk, pattern, n))
