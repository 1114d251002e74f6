"""GPU tests of the Spartan groups (cozk_spartan_group_create / _round / _final / _free): one round of a co-noir-spartan sumcheck for
several members against ONE public polynomial.  The yardstick is the per-poly path -- cozk_spartan_first_round / cozk_spartan_second_round
and cozk_poly_bind(.., LOW_TO_HIGH), which test_gpu_poly.py holds to the oracle -- on polynomials with the same data.  Bar: bit-exact, raw
Montgomery limbs through the C ABI (ctypes).  No test provokes a device fault: every bad argument is refused on the host before any launch."""
import ctypes

import numpy as np
import pytest

import pyref as O
import pyspartan as SP

pytestmark = pytest.mark.gpu
INVALID = -1  # COZK_ERR_INVALID_ARG
SENT = 0x5A5A
FIRST, SECOND = 1, 2
R = O.R


@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


def _fr(cozk, x):
    return np.ascontiguousarray(cozk.fr_to_mont_limbs([x])[0])


def _poly(cozk, c, length, seed, mode=None):
    return cozk.Rep3DensePolynomial.random(c, length, seed, mode=cozk.MODE_PLAIN if mode is None else mode)


def _raw(p):
    n = len(p)
    a = np.zeros((n, 4), dtype=np.uint64)
    b = np.zeros((n, 4), dtype=np.uint64)
    p.ctx.check(p.ctx._l.cozk_poly_download(p.ctx.h, p.h, a.ctypes.data, b.ctypes.data))
    return a


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert len(x) == len(y) and np.array_equal(_raw(x), _raw(y))


class Side:
    """k members and the public polynomial(s), twice from the same seeds: `grp` for the group, `one` for the per-poly calls.
    FIRST: member = (za, zb, zc), public = eq.  SECOND: member = (z), public columns a, b, c with coefficients coef; the group's public
    polynomial is their linear combination, `lin` its twin bound by cozk_poly_bind."""

    def __init__(self, cozk, pcs, kind, k, length, seed):
        self.cozk, self.kind, self.k, self.P, self.E = cozk, kind, k, 3 if kind == FIRST else 1, 4 if kind == FIRST else 3
        mk = lambda: [tuple(_poly(cozk, pcs[m % len(pcs)], length, seed + 10 * m + j) for j in range(self.P)) for m in range(k)]
        self.grp, self.one = mk(), mk()
        d = pcs[0]
        self.d = d
        if kind == FIRST:
            self.pub_g = _poly(cozk, d, length, seed + 5000)
            self.pub_s = [_poly(cozk, m[0].ctx, length, seed + 5000) for m in self.one]
        else:
            rng = O.SplitMix64(seed + 77)
            self.coef = [rng.field() for _ in range(3)]
            self.cf = np.ascontiguousarray(cozk.fr_to_mont_limbs(self.coef))
            cols = lambda c: [_poly(cozk, c, length, seed + 6000 + j) for j in range(3)]
            self.pub_g = cozk.Rep3DensePolynomial.linear_combination(cols(d), self.coef, out_mode=cozk.MODE_PLAIN)
            self.lin = cozk.Rep3DensePolynomial.linear_combination(cols(d), self.coef, out_mode=cozk.MODE_PLAIN)
            self.pub_s = [cols(m[0].ctx) for m in self.one]
        self.g = cozk.SpartanGroup(d, kind, self.grp, self.pub_g)

    def planes(self, which):
        return [p for m in which for p in m]

    def single_round(self, m, r):
        """the composition: bind with r (None in the first round), then the per-poly round call"""
        c = self.one[m][0].ctx
        l = c._l
        pubs = [self.pub_s[m]] if self.kind == FIRST else self.pub_s[m]
        if r is not None:
            for p in list(self.one[m]) + pubs:
                c.check(l.cozk_poly_bind(c.h, p.h, r.ctypes.data, 0))
        if self.kind == FIRST:
            out = np.zeros((4, 4), dtype=np.uint64)
            za, zb, zc = self.one[m]
            c.check(l.cozk_spartan_first_round(c.h, za.h, zb.h, zc.h, pubs[0].h, out.ctypes.data))
            return out
        oa, ob = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
        c.check(l.cozk_spartan_second_round(c.h, self.one[m][0].h, pubs[0].h, pubs[1].h, pubs[2].h, self.cf.ctypes.data, oa.ctypes.data, ob.ctypes.data))
        return oa

    def single_final(self, m, r):
        c = self.one[m][0].ctx
        pubs = [self.pub_s[m]] if self.kind == FIRST else self.pub_s[m]
        for p in list(self.one[m]) + pubs:
            c.check(c._l.cozk_poly_bind(c.h, p.h, r.ctypes.data, 0))
        return np.concatenate([_raw(p) for p in self.one[m]])

    def pub_twin(self, r):
        """the public polynomial as cozk_poly_bind leaves it: FIRST member 0's eq (already bound by its round), SECOND the twin"""
        if self.kind == FIRST:
            return _raw(self.pub_s[0])
        if r is not None:
            self.d.check(self.d._l.cozk_poly_bind(self.d.h, self.lin.h, r.ctypes.data, 0))
        return _raw(self.lin)

    def check_round(self, r):
        got = self.g.round_raw(r)
        for m in range(self.k):
            assert np.array_equal(got[m], self.single_round(m, r)), "member %d" % m
        _same(self.planes(self.grp), self.planes(self.one))
        assert np.array_equal(self.g.pub_raw(), self.pub_twin(r))

    def check_final(self, r, k_final):
        got = self.g.final_raw(r, k_final)
        for m in range(k_final):
            assert np.array_equal(got[self.P * m:self.P * (m + 1)], self.single_final(m, r)), "member %d" % m
        _same(self.planes(self.grp[:k_final]), self.planes(self.one[:k_final]))
        assert all(len(p) == 1 for p in self.planes(self.grp[:k_final]))
        for m in range(k_final, self.k):  # left untouched
            assert all(len(p) == 2 for p in self.grp[m])
            self.single_final(m, r)
        pub = self.pub_twin(r) if self.kind == SECOND or k_final else None
        if pub is None:  # FIRST with k_final == 0: member 0's eq was bound by single_final above
            pub = _raw(self.pub_s[0])
        assert len(self.g) == 1 and np.array_equal(self.g.pub_raw(), pub) and np.array_equal(got[-1:], pub)
        if self.kind == SECOND:  # the bound lin is alpha a + beta b + gamma c of the bound columns: the same field element
            a, b, c = [self.cozk.mont_limbs_to_int(_raw(p))[0] for p in self.pub_s[0]]
            assert self.cozk.mont_limbs_to_int(pub)[0] == (self.coef[0] * a + self.coef[1] * b + self.coef[2] * c) % R


def _run_both(cozk, pcs, kind, k, length, k_final=None):
    s = Side(cozk, pcs, kind, k, length, seed=1000 * length + 10 * k + kind)
    rng = O.SplitMix64(length + 3 * k + kind)
    r = None
    for _ in range(length.bit_length() - 1):
        s.check_round(r)
        r = _fr(cozk, rng.field())
    s.check_final(r, k if k_final is None else k_final)
    s.g.free()
    _same(s.planes(s.grp[:k if k_final is None else k_final]), s.planes(s.one[:k if k_final is None else k_final]))  # the members outlive the group


# 2: no binding round; 4, 64: one workgroup per member; 2048: the single-launch bound; 4096: the first multi-workgroup size (the sums
# as they stand, one fused bind), then the hand-over to the single launch; 8192: two multi-workgroup fused binds before the hand-over
LENGTHS = [2, 4, 64, 2048, 4096, 8192]


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("kind", [FIRST, SECOND])
def test_group_rounds_equal_per_poly_rounds(cozk, party_ctxs, kind, k, length):
    _run_both(cozk, party_ctxs, kind, k, length)


@pytest.mark.parametrize("kind", [FIRST, SECOND])
def test_31_members(cozk, party_ctxs, kind):
    _run_both(cozk, party_ctxs, kind, 31, 16)


@pytest.mark.parametrize("kind", [FIRST, SECOND])
def test_final_of_the_first_members_only(cozk, party_ctxs, kind):
    _run_both(cozk, party_ctxs, kind, 5, 8, k_final=3)
    _run_both(cozk, party_ctxs, kind, 3, 4, k_final=0)


def test_sum_grid_cap_gives_the_same_sums(cozk, party_ctxs, monkeypatch):
    monkeypatch.setenv("COZK_SUM_GRID_MAX", "2")  # lanes add many terms each; the per-poly calls do not read the cap
    _run_both(cozk, party_ctxs, FIRST, 3, 8192)
    _run_both(cozk, party_ctxs, SECOND, 3, 8192)


@pytest.mark.parametrize("kind", [FIRST, SECOND])
def test_against_big_ints(cozk, party_ctxs, kind):
    k, length, P = 3, 8, 3 if kind == FIRST else 1
    rng = O.SplitMix64(99 + kind)
    vals = [[[rng.field() for _ in range(length)] for _ in range(P)] for _ in range(k)]
    coef = [rng.field() for _ in range(3)]
    cols = [[rng.field() for _ in range(length)] for _ in range(3)]
    pub = cols[0] if kind == FIRST else [sum(c * col[i] for c, col in zip(coef, cols)) % R for i in range(length)]
    d = party_ctxs[0]
    members = [tuple(cozk.Rep3DensePolynomial.new(party_ctxs[m], v) for v in vals[m]) for m in range(k)]
    g = cozk.SpartanGroup(d, kind, members, cozk.Rep3DensePolynomial.new(d, pub))
    r = None
    for _ in range(3):
        if r is not None:
            vals = [[SP.fix_low(v, r) for v in m] for m in vals]
            cols = [SP.fix_low(c, r) for c in cols]
            pub = SP.fix_low(pub, r)
        if kind == FIRST:
            want = [O.spartan_first_round_evals(m[0], m[1], m[2], pub) for m in vals]
        else:
            want = [O.spartan_second_round_evals(m[0], cols[0], cols[1], cols[2], coef) for m in vals]
        assert g.round(r) == want
        assert [[p.coeffs() for p in m] for m in members] == vals
        r = rng.field()
    finals, pub_final = g.final(r, k)
    assert finals == [[SP.fix_low(v, r)[0] for v in m] for m in vals] and pub_final == SP.fix_low(pub, r)[0]
    g.free()


# ------------------------------------------------------------------------------------------------ refusals
def _expect_invalid(cozk, driver, rc, *texts):
    assert rc == INVALID
    msg = cozk._lib.lib().cozk_last_error(driver.h).decode()
    assert msg and all(t in msg for t in texts), msg


def _arr(polys):
    return (ctypes.c_void_p * 120)(*([x.h.value if x is not None else None for x in polys] + [None] * (120 - len(polys))))


def test_refusals_leave_members_and_public_polynomial_untouched(cozk, party_ctxs):
    l = cozk._lib.lib()
    pcs = party_ctxs
    d = pcs[0]
    rng = O.SplitMix64(12)
    s = Side(cozk, pcs, FIRST, 3, 16, seed=7)
    planes, pub = s.planes(s.grp), s.pub_g
    before = [_raw(p) for p in planes + [pub]]
    rep3 = _poly(cozk, d, 16, 8, mode=cozk.MODE_REP3)
    short, twelve, single = _poly(cozk, d, 8, 9), [_poly(cozk, d, 12, 10 + j) for j in range(4)], [_poly(cozk, d, 1, 20 + j) for j in range(4)]
    many = [_poly(cozk, d, 16, 100 + j) for j in range(99)]

    def create(driver, kind, pl, k, p, text, out=True):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_spartan_group_create(driver.h if driver else None, kind, _arr(pl) if pl is not None else None, k, p.h if p is not None else None,
                                         ctypes.byref(h) if out else None)
        if driver:
            _expect_invalid(cozk, driver, rc, "spartan_group_create: ", text)
        assert rc == INVALID and (not out or h.value is None)

    create(None, FIRST, planes, 3, pub, "null argument")  # no driver: nowhere to leave the text
    create(d, FIRST, None, 3, pub, "null argument")
    create(d, FIRST, planes, 3, None, "null argument")
    create(d, FIRST, planes, 3, pub, "null argument", out=False)
    create(d, 0, planes, 3, pub, "unknown kind")
    create(d, FIRST, planes, 0, pub, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, FIRST, planes, -1, pub, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, FIRST, many, 33, pub, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, FIRST, planes[:4] + [None] + planes[5:], 3, pub, "null member plane")
    create(d, FIRST, planes[:4] + [rep3] + planes[5:], 3, pub, "every member plane must be PLAIN")
    create(d, FIRST, planes, 3, rep3, "the public polynomial must be PLAIN")
    create(d, FIRST, planes[:4] + [short] + planes[5:], 3, pub, "must have one length")
    create(d, FIRST, planes, 3, short, "must have one length")
    create(d, FIRST, twelve[:3], 1, twelve[3], "the length must be a power of two >= 2")
    create(d, FIRST, single[:3], 1, single[3], "the length must be a power of two >= 2")
    create(d, FIRST, planes[:8] + [planes[1]], 3, pub, "duplicate plane")
    create(d, SECOND, planes[:2] + [planes[0]], 3, pub, "duplicate plane")
    create(d, SECOND, [planes[0], pub], 2, pub, "a member plane is the public polynomial")
    assert all(np.array_equal(x, _raw(p)) for x, p in zip(before, planes + [pub]))

    g = s.g
    r = _fr(cozk, rng.field())
    out = np.zeros((3 * 4 + 4, 4), dtype=np.uint64)
    pub_before = g.pub_raw()
    assert l.cozk_spartan_group_round(None, None, out.ctypes.data) == INVALID
    assert l.cozk_spartan_group_final(None, None, 0, out.ctypes.data) == INVALID
    _expect_invalid(cozk, d, l.cozk_spartan_group_round(g.h, None, None), "spartan_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_spartan_group_final(g.h, r.ctypes.data, 3, None), "spartan_group_final: null argument")
    for k_final in (-1, 4):
        _expect_invalid(cozk, d, l.cozk_spartan_group_final(g.h, r.ctypes.data, k_final, out.ctypes.data), "spartan_group_final: 0 <= k_final <= k")
    for rr in (None, r):  # 16 elements do not end at one, with a bind or without
        _expect_invalid(cozk, d, l.cozk_spartan_group_final(g.h, rr.ctypes.data if rr is not None else None, 3, out.ctypes.data),
                        "spartan_group_final: the bind must leave one element")
    # a member that was driven on its own has another length: refused
    c1 = planes[3].ctx
    twin = _poly(cozk, c1, 16, 7 + 10 * 1 + 0)
    c1.check(l.cozk_poly_bind(c1.h, planes[3].h, r.ctypes.data, 0))
    _expect_invalid(cozk, d, l.cozk_spartan_group_round(g.h, None, out.ctypes.data), "spartan_group_round: every member plane must have the group's current length")
    assert (out == 0).all() and np.array_equal(pub_before, g.pub_raw()) and len(g) == 16
    assert all(np.array_equal(x, _raw(p)) for i, (x, p) in enumerate(zip(before, planes)) if i != 3)
    g.free()

    # ... and the members still work: every round to the end by a new group, against the per-poly calls
    s.grp[1] = (twin,) + s.grp[1][1:]
    s.g = cozk.SpartanGroup(d, FIRST, s.grp, pub)
    r = None
    for _ in range(4):
        s.check_round(r)
        r = _fr(cozk, rng.field())
    # a binding round on members that the bind leaves fully bound (2 elements), then on fully bound members
    live = [_raw(p) for p in s.planes(s.grp)] + [s.g.pub_raw()]
    _expect_invalid(cozk, d, l.cozk_spartan_group_round(s.g.h, r.ctypes.data, out.ctypes.data), "spartan_group_round: a binding round on members that the bind leaves fully bound")
    assert all(np.array_equal(x, y) for x, y in zip(live, [_raw(p) for p in s.planes(s.grp)] + [s.g.pub_raw()]))
    s.check_final(r, 3)
    for rr in (None, r):
        _expect_invalid(cozk, d, l.cozk_spartan_group_round(s.g.h, rr.ctypes.data if rr is not None else None, out.ctypes.data),
                        "spartan_group_round: the members are fully bound")
    _expect_invalid(cozk, d, l.cozk_spartan_group_final(s.g.h, r.ctypes.data, 3, out.ctypes.data), "spartan_group_final: the bind must leave one element")
    assert (out == 0).all()
    _same(s.planes(s.grp), s.planes(s.one))
    d.check(l.cozk_spartan_group_final(s.g.h, None, 3, out.ctypes.data))  # without a bind: the final values again
    assert np.array_equal(out[:9], np.concatenate([_raw(p) for p in s.planes(s.grp)]))
    s.g.free()
    assert l.cozk_spartan_group_free(None) == 0


def test_member_on_another_device_is_refused(cozk, party_ctxs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    l = cozk._lib.lib()
    d = party_ctxs[0]
    other = cozk.Context(1)
    here, there, pub, pub_there = _poly(cozk, d, 8, 1), _poly(cozk, other, 8, 2), _poly(cozk, d, 8, 3), _poly(cozk, other, 8, 3)
    for pl, p, text in (([here, there], pub, "every member must live on the driver's device"), ([here], pub_there, "the public polynomial must live on the driver's device")):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_spartan_group_create(d.h, SECOND, _arr(pl), len(pl), p.h, ctypes.byref(h))
        _expect_invalid(cozk, d, rc, "spartan_group_create: ", text)
        assert h.value is None
    g = cozk.SpartanGroup(d, SECOND, [here], pub)  # the member here still serves
    g.free()
    del there, pub_there
    other.close()
