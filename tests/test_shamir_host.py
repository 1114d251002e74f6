"""CPU tier of the Shamir seam: cozk_shamir_lagrange (pure host, no context) against the big-int restatement
(tests/shamir_ref.py of mpc-types/src/protocols/shamir.rs), its argument checks, and the restatement's own identities."""
import ctypes
import itertools

import numpy as np
import pytest

import pyref as O
import shamir_ref as S

R = O.R
EDGE_SECRETS = [0, 1, R - 1, R - 2]


def _secrets(seed, n):
    return EDGE_SECRETS + O.synthetic_fr(seed, n - len(EDGE_SECRETS))


@pytest.mark.parametrize("points", [list(range(1, 3)), list(range(1, 8)), list(range(1, 33)), [8, 1, 5, 3, 2],
                                    [10, 4, 7, 1, 9, 2, 6], [32], [31, 32]], ids=lambda p: "-".join(map(str, p))[:24])
def test_lagrange_matches_restatement(cozk, points):
    lam = cozk.shamir_lagrange(points)
    assert lam == S.lagrange_from_coeff(points)
    assert sum(lam) % R == 1  # the constant polynomial 1 opens to 1


@pytest.mark.parametrize("parties,degree", [(3, 1), (10, 6), (8, 2), (32, 15)])
def test_lagrange_opens_restated_shares(cozk, parties, degree):
    v = _secrets(900 + parties, 16)
    sh = S.share_vec(v, S.keys_for(17 + degree, degree), degree, parties, counter=5)
    for pts in ([p + 1 for p in range(degree + 1)], [parties - p for p in range(degree + 1)]):
        lam = cozk.shamir_lagrange(pts)
        assert [S.reconstruct([sh[p - 1][i] for p in pts], lam) for i in range(len(v))] == v


def _raw_lagrange(cozk, pts):
    arr = np.asarray(pts, dtype=np.uint32)
    out = np.zeros((max(len(pts), 1), 4), dtype=np.uint64)
    return cozk._lib.lib().cozk_shamir_lagrange(arr.ctypes.data if len(pts) else None, len(pts), out.ctypes.data)


@pytest.mark.parametrize("pts", [[], [0, 1], [1, 2, 1], [1, 33], list(range(1, 34))], ids=["empty", "zero", "repeat", "above-max", "k-above-max"])
def test_lagrange_rejects_bad_points(cozk, pts):
    assert _raw_lagrange(cozk, pts) == -1  # COZK_ERR_INVALID_ARG
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_lagrange(pts)
    assert e.value.code == -1


def test_lagrange_rejects_null_pointers(cozk):
    l = cozk._lib.lib()
    pts = np.asarray([1, 2], dtype=np.uint32)
    out = np.zeros((2, 4), dtype=np.uint64)
    assert l.cozk_shamir_lagrange(None, 2, out.ctypes.data) == -1
    assert l.cozk_shamir_lagrange(pts.ctypes.data, 2, None) == -1


@pytest.mark.parametrize("parties,degree", [(3, 1), (10, 6), (8, 2)])
def test_restatement_any_subset_reconstructs(parties, degree):
    """shamir.rs test_shamir: the first degree + 1 shares and other subsets of that size open the secret, in any order"""
    n = 257
    v = _secrets(4000 + parties, n)
    sh = S.share_vec(v, S.keys_for(31 + parties, degree), degree, parties, counter=(1 << 33) + 7)
    subsets = list(itertools.islice(itertools.combinations(range(1, parties + 1), degree + 1), 0, None, 7))[:6]
    subsets.append(tuple(reversed(range(parties - degree, parties + 1))))
    for pts in subsets:
        assert S.combine_vec([sh[p - 1] for p in pts], list(pts), degree) == v
    # more shares than needed: the first degree + 1 are used, as in combine_field_elements
    allp = list(range(1, parties + 1))
    assert S.combine_vec(sh, allp, degree) == v


@pytest.mark.parametrize("parties,degree", [(8, 2), (3, 1)])
def test_restatement_product_needs_twice_the_degree(parties, degree):
    """share x share is a sharing of degree 2 * degree (ops.rs:93-118): it opens from 2 * degree + 1 shares and does NOT
    from degree + 1 -- a sharing whose random coefficients were all zero would pass the second check too"""
    n = 64
    a, b = _secrets(1, n), list(reversed(_secrets(2, n)))
    sa = S.share_vec(a, S.keys_for(41, degree), degree, parties, counter=3)
    sb = S.share_vec(b, S.keys_for(42, degree), degree, parties, counter=3)
    prod = [[x * y % R for x, y in zip(sa[p], sb[p])] for p in range(parties)]
    want = [x * y % R for x, y in zip(a, b)]
    pts = list(range(parties, parties - 2 * degree - 1, -1))
    assert S.combine_vec([prod[p - 1] for p in pts], pts, 2 * degree) == want
    low = S.combine_vec([prod[p - 1] for p in pts[:degree + 1]], pts[:degree + 1], degree)
    assert sum(x != y for x, y in zip(low, want)) >= n // 2


def test_restatement_evaluate_poly_is_horner():
    poly = [5, R - 1, 7, R - 2]
    for x in (1, 2, 32):
        assert S.evaluate_poly(poly, x) == sum(c * pow(x, k, R) for k, c in enumerate(poly)) % R
    assert S.share(poly, 3) == [S.evaluate_poly(poly, x) for x in (1, 2, 3)]
