"""CPU tier of the Shamir multiplication with a king and double-random pairs: the big-int restatement (tests/shamir_dn_ref.py)
proves itself -- both halves of every pair are sharings of their stated degree of one value, the product is a degree-t sharing
of a b that multiplies again and opens to what the resharing multiplication (tests/shamir_mul_ref.py) opens to -- and the new
entry points exist and refuse bad arguments on the host, with no device."""
import ctypes

import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_mul_ref as M
import shamir_ref as S

R = O.R
SHAPES = [(3, 1), (5, 2), (8, 2), (7, 3), (15, 7)]
N = 8


def _secrets(seed):
    return [0, 1, R - 1] + O.synthetic_fr(seed, N - 3)


def _scattered(parties, k):
    """k parties (1-based points), from the high end and not contiguous where the party count allows it"""
    pts = [parties - 2 * i for i in range(k)]
    return pts if pts[-1] >= 1 else list(range(parties, parties - k, -1))


def _open(shares, pts, degree):
    return S.combine_vec([shares[p - 1] for p in pts], pts, degree)


def _interpolates_to_every_party(shares, pts):
    """the polynomial through the shares at `pts` passes through every other party's share (Lagrange basis shifted to q)"""
    for q in range(1, len(shares) + 1):
        lam = []
        for i in pts:
            num, den = 1, 1
            for j in pts:
                if j != i:
                    num = num * (j - q) % R
                    den = den * (j - i) % R
            lam.append(num * pow(den, -1, R) % R)
        assert [S.reconstruct([shares[p - 1][i] for p in pts], lam) for i in range(N)] == shares[q - 1], "party %d" % q


def _deal(seed, parties, degree, counter):
    v = _secrets(seed)
    return v, S.share_vec(v, S.keys_for(seed, degree), degree, parties, counter=counter)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d-t%d" % s)
def world(request):
    parties, degree = request.param
    keys = D.party_keys(5, parties, degree)
    pairs = D.rand(keys, degree, N, counter=3 * N)
    a, sa = _deal(11, parties, degree, 0)
    b, sb = _deal(12, parties, degree, N)
    half = lambda k, h: [pairs[q][k][h] for q in range(parties)]
    return dict(parties=parties, degree=degree, keys=keys, pairs=pairs, a=a, b=b, sa=sa, sb=sb, half=half)


def test_restatement_yields_n_minus_t_pairs_of_one_value(world):
    parties, degree, half = world["parties"], world["degree"], world["half"]
    assert all(len(p) == parties - degree for p in world["pairs"])
    for k in range(parties - degree):
        want = D.pair_value(world["keys"], k, N, counter=3 * N)
        assert _open(half(k, 0), _scattered(parties, degree + 1), degree) == want, "pair %d, degree t" % k
        assert _open(half(k, 1), _scattered(parties, 2 * degree + 1), 2 * degree) == want, "pair %d, degree 2t" % k
    assert len({tuple(D.pair_value(world["keys"], k, N, counter=3 * N)) for k in range(parties - degree)}) == parties - degree


def test_restatement_halves_are_sharings_of_their_stated_degree(world):
    parties, degree, half = world["parties"], world["degree"], world["half"]
    for k in range(parties - degree):
        _interpolates_to_every_party(half(k, 0), _scattered(parties, degree + 1))
        _interpolates_to_every_party(half(k, 1), _scattered(parties, 2 * degree + 1))
    # and of no lower one: the second half does not open with degree 2t - 1
    want = D.pair_value(world["keys"], 0, N, counter=3 * N)
    low = _open(half(0, 1), _scattered(parties, 2 * degree + 1), 2 * degree - 1)
    assert sum(x != y for x, y in zip(low, want)) >= N // 2


def _kings(parties, degree):
    return sorted({0, 2 * degree} | ({parties - 1} if parties - 1 > 2 * degree else set()))


def test_restatement_mul_king_opens_to_the_product(world):
    parties, degree, half = world["parties"], world["degree"], world["half"]
    want = [x * y % R for x, y in zip(world["a"], world["b"])]
    got = None
    for king in _kings(parties, degree):
        c = D.mul_king(world["sa"], world["sb"], half(0, 0), half(0, 1), degree, king=king)
        assert _open(c, _scattered(parties, degree + 1), degree) == want, "king %d" % king
        assert got is None or c == got  # the king changes who computes, not what
        got = c
    _interpolates_to_every_party(got, _scattered(parties, degree + 1))
    pts = list(range(parties, parties - degree - 1, -1))
    low = _open(got, pts, degree - 1)
    assert sum(x != y for x, y in zip(low, want)) >= N // 2


def test_restatement_products_chain_and_agree_with_the_resharing(world):
    parties, degree, half = world["parties"], world["degree"], world["half"]
    z, sz = _deal(13, parties, degree, 2 * N)
    c = D.mul_king(world["sa"], world["sb"], half(0, 0), half(0, 1), degree)
    d = D.mul_king(c, sz, half(1, 0), half(1, 1), degree, king=2 * degree)
    pts = _scattered(parties, degree + 1)
    assert _open(d, pts, degree) == [x * y * w % R for x, y, w in zip(world["a"], world["b"], z)]
    grr = M.mul(world["sa"], world["sb"], M.party_keys(3, parties, degree), degree, counter=4 * N)
    assert _open(c, pts, degree) == _open(grr, pts, degree)


def test_restatement_ignores_factors_above_2t(world):
    parties, degree, half = world["parties"], world["degree"], world["half"]
    k = D.senders(degree)
    c = D.mul_king(world["sa"], world["sb"], half(0, 0), half(0, 1), degree)
    junk = O.synthetic_fr(99, N)
    for rest in ([junk] * (parties - k), [None] * (parties - k)):
        assert D.mul_king(world["sa"][:k] + rest, world["sb"][:k] + rest, half(0, 0), half(0, 1)[:k] + rest, degree) == c


def test_restatement_extract_is_the_vandermonde_matrix():
    rec = [O.synthetic_fr(70 + j, 3) for j in range(5)]
    out = D.extract(rec, 4)
    assert out[0] == [sum(v[i] for v in rec) % R for i in range(3)]
    assert out[3] == [sum((j + 1) ** 3 * v[i] for j, v in enumerate(rec)) % R for i in range(3)]
    assert D.mul_mask([2, R - 1], [3, R - 1], [R - 6, 5]) == [0, 6]


# ------------------------------------------------------------------------------------------------ the ABI, without a device
SYMBOLS = ("cozk_shamir_rand_deal", "cozk_shamir_rand_extract", "cozk_shamir_rand_inproc", "cozk_shamir_rand_vec", "cozk_shamir_mul_mask",
           "cozk_shamir_mul_king_inproc", "cozk_shamir_mul_king_vec")


def test_wrappers_exist(cozk):
    for name in ("shamir_rand_deal", "shamir_rand_extract", "shamir_rand", "shamir_mul_king"):
        assert callable(getattr(cozk, name))
    assert callable(cozk.Vec.shamir_mul_mask)
    for name in ("shamir_rand_vec", "shamir_mul_king_vec"):
        assert callable(getattr(cozk.Context, name))
    for sym in SYMBOLS:
        assert sym in cozk._lib.SIGNATURES and hasattr(cozk._lib.lib(), sym)


SENT = 0x5A5A


def _table(k=40):
    return (ctypes.c_void_p * k)(*([SENT] * k))


def _cleared(t, k):
    return all(t[i] is None for i in range(k)) and all(t[i] == SENT for i in range(k, len(t)))


def test_null_and_out_of_range_arguments_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    keys = b"\x01" * (32 * 22)
    # rand_deal: two tables of num_parties
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_deal(None, 8, keys, 2, 5, 0, x, y) == -1  # COZK_ERR_INVALID_ARG
    assert _cleared(x, 5) and _cleared(y, 5)
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_deal(None, 8, keys, 2, 33, 0, x, y) == -1
    assert _cleared(x, 0) and _cleared(y, 0)  # the length of the tables is unknown: untouched
    y = _table()
    assert l.cozk_shamir_rand_deal(None, 8, keys, 2, 5, 0, None, y) == -1 and _cleared(y, 5)
    assert l.cozk_shamir_rand_deal(None, 8, keys, 2, 5, 0, None, None) == -1
    # rand_extract: count handles
    x = _table()
    assert l.cozk_shamir_rand_extract(None, None, 5, 3, x) == -1 and _cleared(x, 3)
    x = _table()
    assert l.cozk_shamir_rand_extract(None, None, 5, 33, x) == -1 and _cleared(x, 0)
    x = _table()
    assert l.cozk_shamir_rand_extract(None, None, 5, 0, x) == -1 and _cleared(x, 0)
    assert l.cozk_shamir_rand_extract(None, None, 5, 3, None) == -1
    # rand_inproc: n (n - t) handles per table
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_inproc(None, None, 8, 2, 5, 0, x, y) == -1
    assert _cleared(x, 15) and _cleared(y, 15)
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_inproc(None, None, 8, 2, 33, 0, x, y) == -1
    assert _cleared(x, 0) and _cleared(y, 0)
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_inproc(None, None, 8, 0, 5, 0, x, y) == -1  # degree 0: n - t pairs is not what the caller sized
    assert _cleared(x, 0) and _cleared(y, 0)
    x = _table()
    assert l.cozk_shamir_rand_inproc(None, None, 8, 2, 5, 0, x, None) == -1 and _cleared(x, 15)
    # rand_vec: ranks - degree handles, unknown without a ring
    x, y = _table(), _table()
    assert l.cozk_shamir_rand_vec(None, 8, keys, 1, 0, x, y) == -1
    assert _cleared(x, 0) and _cleared(y, 0)
    assert l.cozk_shamir_rand_vec(None, 8, keys, 1, 0, None, None) == -1
    # the online step
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_mul_mask(None, None, None, None, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_mul_mask(None, None, None, None, None) == -1
    x = _table()
    assert l.cozk_shamir_mul_king_inproc(None, None, None, None, None, 2, 5, 0, x) == -1 and _cleared(x, 5)
    x = _table()
    assert l.cozk_shamir_mul_king_inproc(None, None, None, None, None, 2, 5, 5, x) == -1 and _cleared(x, 5)  # king = n
    x = _table()
    assert l.cozk_shamir_mul_king_inproc(None, None, None, None, None, 1, 33, 0, x) == -1 and _cleared(x, 0)
    assert l.cozk_shamir_mul_king_inproc(None, None, None, None, None, 2, 5, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_mul_king_vec(None, None, None, None, None, 1, 0, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_mul_king_vec(None, None, None, None, None, 1, 0, None) == -1
