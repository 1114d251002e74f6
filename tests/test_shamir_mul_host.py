"""CPU tier of the Shamir multiplication with degree reduction: the big-int restatement (tests/shamir_mul_ref.py) proves
itself -- its output is a degree-t sharing of a b that can be multiplied again -- and the new entry points exist and refuse
bad arguments on the host, with no device."""
import ctypes

import pytest

import pyref as O
import shamir_mul_ref as M
import shamir_ref as S

R = O.R
SHAPES = [(3, 1), (5, 2), (8, 2), (7, 3)]
N = 8


def _secrets(seed):
    return [0, 1, R - 1] + O.synthetic_fr(seed, N - 3)


def _scattered(parties, degree):
    """degree + 1 parties (1-based points), from the high end and not contiguous where the party count allows it"""
    pts = [parties - 2 * i for i in range(degree + 1)]
    return pts if pts[-1] >= 1 else list(range(parties, parties - degree - 1, -1))


def _open(shares, pts, degree):
    return S.combine_vec([shares[p - 1] for p in pts], pts, degree)


def _deal(seed, parties, degree, counter):
    v = _secrets(seed)
    return v, S.share_vec(v, S.keys_for(seed, degree), degree, parties, counter=counter)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d-t%d" % s)
def product(request):
    parties, degree = request.param
    a, sa = _deal(11, parties, degree, 0)
    b, sb = _deal(12, parties, degree, N)
    keys = M.party_keys(3, parties, degree)
    return parties, degree, a, b, sa, sb, keys, M.mul(sa, sb, keys, degree, counter=2 * N)


def test_restatement_opens_to_the_product_from_t_plus_1(product):
    parties, degree, a, b, _, _, _, c = product
    want = [x * y % R for x, y in zip(a, b)]
    assert _open(c, _scattered(parties, degree), degree) == want
    assert _open(c, list(range(1, degree + 2)), degree) == want


def test_restatement_result_is_a_degree_t_sharing(product):
    """t + 1 result shares interpolate to every other party's share: evaluate the polynomial through them at x = q + 1 with
    the Lagrange basis shifted to that point"""
    parties, degree, _, _, _, _, _, c = product
    pts = _scattered(parties, degree)
    for q in range(1, parties + 1):
        lam = []
        for i in pts:
            num, den = 1, 1
            for j in pts:
                if j != i:
                    num = num * (j - q) % R
                    den = den * (j - i) % R
            lam.append(num * pow(den, -1, R) % R)
        assert [S.reconstruct([c[p - 1][i] for p in pts], lam) for i in range(N)] == c[q - 1], "party %d" % q


def test_restatement_products_chain(product):
    parties, degree, a, b, _, _, keys, c = product
    z, sz = _deal(13, parties, degree, 3 * N)
    d = M.mul(c, sz, keys, degree, counter=4 * N)
    assert _open(d, _scattered(parties, degree), degree) == [x * y * w % R for x, y, w in zip(a, b, z)]


def test_restatement_ignores_parties_above_2t(product):
    parties, degree, _, _, sa, sb, keys, c = product
    k = M.dealers(degree)
    junk = O.synthetic_fr(99, N)
    ga = sa[:k] + [junk] * (parties - k)
    gb = sb[:k] + [None] * (parties - k)
    gk = keys[:k] + [None] * (parties - k)
    assert M.mul(ga, gb, gk, degree, counter=2 * N) == c


def test_restatement_finish_is_the_degree_2t_combine(product):
    parties, degree, _, _, sa, sb, keys, c = product
    k = M.dealers(degree)
    h = [M.mul_deal(sa[p], sb[p], keys[p], degree, parties, counter=2 * N) for p in range(k)]
    lam = S.lagrange_from_coeff(list(range(1, k + 1)))
    for q in range(parties):
        assert [sum(l * h[p][q][i] for p, l in enumerate(lam)) % R for i in range(N)] == c[q]


# ------------------------------------------------------------------------------------------------ the ABI, without a device
def test_wrappers_exist(cozk):
    assert callable(cozk.shamir_mul)
    for name in ("shamir_mul_deal",):
        assert callable(getattr(cozk.Vec, name))
    for name in ("all_to_all", "shamir_mul_vec"):
        assert callable(getattr(cozk.Context, name))
    for sym in ("cozk_shamir_mul_deal", "cozk_shamir_mul_inproc", "cozk_shamir_mul_vec", "cozk_ring_all_to_all"):
        assert sym in cozk._lib.SIGNATURES and hasattr(cozk._lib.lib(), sym)


def test_null_arguments_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    SENT = 0x5A5A
    keys = b"\x01" * 64
    out = (ctypes.c_void_p * 8)(*([SENT] * 8))
    assert l.cozk_shamir_mul_deal(None, None, None, keys, 2, 5, 0, out) == -1  # COZK_ERR_INVALID_ARG
    assert [out[i] for i in range(8)] == [None] * 5 + [SENT] * 3
    out = (ctypes.c_void_p * 40)(*([SENT] * 40))
    assert l.cozk_shamir_mul_deal(None, None, None, keys, 2, 33, 0, out) == -1
    assert all(out[i] == SENT for i in range(40))  # the length of out[] is unknown: untouched
    assert l.cozk_shamir_mul_deal(None, None, None, keys, 2, 5, 0, None) == -1
    out = (ctypes.c_void_p * 8)(*([SENT] * 8))
    assert l.cozk_shamir_mul_inproc(None, None, None, None, 2, 5, 0, out) == -1
    assert [out[i] for i in range(8)] == [None] * 5 + [SENT] * 3
    assert l.cozk_shamir_mul_inproc(None, None, None, None, 2, 5, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_mul_vec(None, None, None, keys, 1, 0, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_mul_vec(None, None, None, keys, 1, 0, None) == -1
    assert l.cozk_ring_all_to_all(None, None, None) == -1
