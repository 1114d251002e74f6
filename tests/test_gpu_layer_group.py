"""GPU tests of the layer groups (cozk_layer_group_create / _round / _final / _free): one sumcheck round of several layers that share
the public eq polynomial, the challenge and the claim.  The yardstick is the per-layer path -- cozk_layer_round, cozk_layer_bind and
cozk_layer_final_claims, which test_gpu_poly.py holds to the oracle -- on clones of the same layers.  Bar: bit-exact, raw Montgomery
limbs through the C ABI (ctypes).  No test provokes a device fault: every bad argument is refused on the host before any launch."""
import ctypes

import numpy as np
import pytest

import pyref as O

pytestmark = pytest.mark.gpu
INVALID = -1  # COZK_ERR_INVALID_ARG
SENT = 0x5A5A


@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


def _nv(length):
    """rounds of a layer's sumcheck (test_gpu_poly.py)"""
    return max(0, ((length + 1) // 2 - 1).bit_length())


def _fr(cozk, x):
    return np.ascontiguousarray(cozk.fr_to_mont_limbs([x])[0])


def _members(cozk, pcs, mode, k, length, seed):
    """k seeded layers with different data, member m on context m mod 8"""
    P = cozk.Rep3DenseInterleavedPolynomial
    out = []
    for m in range(k):
        c = pcs[m % len(pcs)]
        a = cozk.Vec.random(c, length, seed + 2 * m)
        b = cozk.Vec.random(c, length, seed + 2 * m + 1) if mode == "rep3" else None
        out.append(P.from_vecs(c, a, b))
    return out


def _raw(layer):
    """(len, a limbs, b limbs) of a layer as it stands"""
    n = len(layer)
    a = np.zeros((n, 4), dtype=np.uint64)
    b = np.zeros((n, 4), dtype=np.uint64)
    layer.ctx.check(layer.ctx._l.cozk_layer_download(layer.ctx.h, layer.h, a.ctypes.data, b.ctypes.data))
    return n, a, b


def _same(xs, ys):
    for x, y in zip(xs, ys):
        nx, ax, bx = _raw(x)
        ny, ay, by = _raw(y)
        assert nx == ny and np.array_equal(ax, ay) and np.array_equal(bx, by)


def _single_round(member, eq, r, claim):
    out = np.zeros((4, 4), dtype=np.uint64)
    c = member.ctx
    c.check(c._l.cozk_layer_round(c.h, member.h, eq.h, r.ctypes.data if r is not None else None, claim.ctypes.data, out.ctypes.data))
    return out


def _group_round(l, g, eq, r, claim, k):
    out = np.full((4 * k, 4), 0xA5, dtype=np.uint64)
    rc = l.cozk_layer_group_round(g.h, eq.h, r.ctypes.data if r is not None else None, claim.ctypes.data, out.ctypes.data)
    return rc, out


def _single_final(member, r):
    c = member.ctx
    if r is not None:
        c.check(c._l.cozk_layer_bind(c.h, member.h, r.ctypes.data))
    out = np.zeros((4, 4), dtype=np.uint64)
    c.check(c._l.cozk_layer_final_claims(c.h, member.h, out.ctypes.data))
    return out


def _group_final(l, g, eq, r, k_final):
    out = np.full((4 * max(k_final, 1), 4), 0xA5, dtype=np.uint64)
    rc = l.cozk_layer_group_final(g.h, eq.h, r.ctypes.data if r is not None else None, k_final, out.ctypes.data)
    return rc, out


def _run_both(cozk, pcs, mode, k, length, nv=None, final=True):
    """every round to the end, by the group on the layers and by the per-layer calls on their clones (each with an eq of its own on
    its own context); compares every coefficient of every member, the bound layers after every round, the eq lengths and the final
    claims"""
    l = cozk._lib.lib()
    nv = _nv(length) if nv is None else nv
    rng = O.SplitMix64(1000 * length + 10 * k + (mode == "rep3"))
    w = [rng.field() for _ in range(nv)]
    grp = _members(cozk, pcs, mode, k, length, seed=length + k)
    one = [x.clone() for x in grp]
    eq_g = cozk.SplitEqPolynomial(pcs[0], w)
    eq_s = [cozk.SplitEqPolynomial(x.ctx, w) for x in one]
    g = cozk.LayerGroup(pcs[0], grp)
    r = None
    for _ in range(nv):
        claim = _fr(cozk, rng.field())
        rc, got = _group_round(l, g, eq_g, r, claim, k)
        pcs[0].check(rc)
        for m in range(k):
            want = _single_round(one[m], eq_s[m], r, claim)
            assert np.array_equal(got[4 * m:4 * m + 4], want), "member %d" % m
            assert eq_s[m].lens() == eq_g.lens()
        _same(grp, one)
        r = _fr(cozk, rng.field())
    if final:
        rc, got = _group_final(l, g, eq_g, r, k)
        pcs[0].check(rc)
        for m in range(k):
            assert np.array_equal(got[4 * m:4 * m + 4], _single_final(one[m], r)), "member %d" % m
        assert all(len(x) == 2 for x in grp)
        _same(grp, one)
        if r is not None:  # the group's final binds the eq too (cozk_layer_prove_rounds behind its last round)
            eq_s[0].bind(rng.field())
            assert eq_g.lens() == eq_s[0].lens()
    g.free()
    _same(grp, one)  # the members outlive the group


# 2: no round, final without a bind; 4: one chunk; 12, 1000: ragged tails; 2048: the last small length; 2052, 4096: the first round through
# the large path, then the hand-over to the small kernel; 16384: 4096 chunks -- the 9 x 29 kernels, then the saturated ones, then the small one
LENGTHS = [2, 4, 12, 1000, 2048, 2052, 4096, 16384]


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("k", [1, 3, 5, 15])
@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_group_rounds_equal_per_layer_rounds(cozk, party_ctxs, mode, k, length):
    _run_both(cozk, party_ctxs, mode, k, length)


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_group_of_32_members(cozk, party_ctxs, mode):
    _run_both(cozk, party_ctxs, mode, 32, 8)


@pytest.mark.parametrize("length", [12, 1000])
@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_group_rounds_with_a_short_eq(cozk, party_ctxs, mode, length):
    """an eq polynomial of one variable less than the layer has: more chunks than eq pairs (nch > limit), the sums stop at the
    shorter side as the per-layer kernels' do; the layer is not down to two elements at the end, so no final"""
    _run_both(cozk, party_ctxs, mode, 3, length, nv=_nv(length) - 1, final=False)


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_group_rounds_on_one_workgroup_per_member(cozk, party_ctxs, mode, monkeypatch):
    """COZK_SUM_GRID_MAX=1: every large launch is one workgroup, so member m's three rows of the shared partials start at
    3 m gx with gx = 1, and the one finishing kernel reads 3 k rows of one partial"""
    monkeypatch.setenv("COZK_SUM_GRID_MAX", "1")
    _run_both(cozk, party_ctxs, mode, 5, 16384)


@pytest.mark.parametrize("length", [16, 16384])
@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_group_and_per_layer_calls_interleave(cozk, party_ctxs, mode, length):
    """round 0 by the group, round 1 by cozk_layer_round on each member and cozk_spliteq_bind on the group's eq, round 2 by the group
    again: the same results as the per-layer calls all the way (at 16384 all three rounds are large-path rounds)"""
    l = cozk._lib.lib()
    pcs, k = party_ctxs, 3
    rng = O.SplitMix64(77 + length)
    w = [rng.field() for _ in range(_nv(length))]
    grp = _members(cozk, pcs, mode, k, length, seed=5)
    one = [x.clone() for x in grp]
    eq_g = cozk.SplitEqPolynomial(pcs[0], w)
    eq_s = [cozk.SplitEqPolynomial(x.ctx, w) for x in one]
    eq_mid = [cozk.SplitEqPolynomial(x.ctx, w) for x in grp]  # what round 1 binds beside the members of the group
    g = cozk.LayerGroup(pcs[0], grp)
    claims = [_fr(cozk, rng.field()) for _ in range(3)]
    rs = [None] + [_fr(cozk, rng.field()) for _ in range(2)]
    want = [[_single_round(one[m], eq_s[m], rs[j], claims[j]) for m in range(k)] for j in range(3)]
    rc, got = _group_round(l, g, eq_g, rs[0], claims[0], k)
    pcs[0].check(rc)
    assert all(np.array_equal(got[4 * m:4 * m + 4], want[0][m]) for m in range(k))
    for m in range(k):
        assert np.array_equal(_single_round(grp[m], eq_mid[m], rs[1], claims[1]), want[1][m])
    pcs[0].check(l.cozk_spliteq_bind(pcs[0].h, eq_g.h, rs[1].ctypes.data))
    rc, got = _group_round(l, g, eq_g, rs[2], claims[2], k)
    pcs[0].check(rc)
    assert all(np.array_equal(got[4 * m:4 * m + 4], want[2][m]) for m in range(k))
    assert eq_g.lens() == eq_s[0].lens()
    _same(grp, one)


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_final_leaves_members_from_k_final_untouched(cozk, party_ctxs, mode):
    l = cozk._lib.lib()
    pcs, k = party_ctxs, 5
    rng = O.SplitMix64(9)
    grp = _members(cozk, pcs, mode, k, 4, seed=3)
    one = [x.clone() for x in grp]
    before = [_raw(x) for x in grp]
    g = cozk.LayerGroup(pcs[0], grp)
    eq = cozk.SplitEqPolynomial(pcs[0], [rng.field()])
    r = _fr(cozk, rng.field())
    rc, got = _group_final(l, g, eq, None, 0)  # nobody, no bind: nothing happens
    pcs[0].check(rc)
    assert (got == np.uint64(0xA5)).all() and eq.lens() == (2, 1)
    rc, got = _group_final(l, g, eq, r, 2)
    pcs[0].check(rc)
    for m in range(2):
        assert np.array_equal(got[4 * m:4 * m + 4], _single_final(one[m], r))
    _same(grp[:2], one[:2])
    for m in range(2, k):  # their length and their bytes
        n, a, b = _raw(grp[m])
        assert n == 4 and np.array_equal(a, before[m][1]) and np.array_equal(b, before[m][2])
    assert eq.lens() == (1, 1)  # bound with the members


def test_python_layer_group(cozk, party_ctxs):
    """poly.LayerGroup in canonical integers against Rep3DenseInterleavedPolynomial.round / bind / final_claims"""
    pcs = party_ctxs
    for mode in ("plain", "rep3"):
        rng = O.SplitMix64(31)
        w = [rng.field() for _ in range(2)]
        grp = _members(cozk, pcs, mode, 3, 8, seed=40)
        one = [x.clone() for x in grp]
        eq_g, eq_s = cozk.SplitEqPolynomial(pcs[0], w), [cozk.SplitEqPolynomial(x.ctx, w) for x in one]
        g = cozk.LayerGroup(pcs[0], grp)
        r = None
        for _ in range(2):
            claim = rng.field()
            assert g.round(eq_g, r, claim) == [one[m].round(eq_s[m], r, claim) for m in range(3)]
            r = rng.field()
        for x in one:
            x.bind(r)
        assert g.final(eq_g, r, 3) == [x.final_claims() for x in one]
        g.free()


# ------------------------------------------------------------------------------------------------ refusals
def _expect_invalid(cozk, driver, rc, text):
    assert rc == INVALID
    msg = cozk._lib.lib().cozk_last_error(driver.h).decode()
    assert text in msg, msg


def _arr(layers):
    return (ctypes.c_void_p * 40)(*([x.h.value if x is not None else None for x in layers] + [None] * (40 - len(layers))))


def test_refusals_leave_no_handle_and_working_members(cozk, party_ctxs):
    l = cozk._lib.lib()
    pcs = party_ctxs
    d = pcs[0]
    rng = O.SplitMix64(12)
    plain = _members(cozk, pcs, "plain", 4, 16, seed=7)
    one = [x.clone() for x in plain]
    rep3 = _members(cozk, pcs, "rep3", 1, 16, seed=8)
    short = _members(cozk, pcs, "plain", 1, 8, seed=9)
    many = plain + [plain[0].clone() for _ in range(29)]

    def create(driver, layers, k, text, out=True):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_layer_group_create(driver.h if driver else None, _arr(layers) if layers is not None else None, k, ctypes.byref(h) if out else None)
        if driver:
            _expect_invalid(cozk, driver, rc, "layer_group_create: " + text)
        assert rc == INVALID and (not out or h.value is None)

    create(None, plain, 4, "null argument")  # no driver: nowhere to leave the text
    create(d, None, 4, "null argument")
    create(d, plain, 4, "null argument", out=False)
    create(d, plain, 0, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, plain, -1, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, many, 33, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, [plain[0], None, plain[2]], 3, "null member")
    create(d, [plain[0], rep3[0]], 2, "the members must have one mode")
    create(d, [plain[0], short[0]], 2, "the members must have one length >= 2")
    create(d, [plain[0], plain[1], plain[0]], 3, "duplicate member")

    w = [rng.field() for _ in range(3)]
    eq, eq_other = cozk.SplitEqPolynomial(d, w), cozk.SplitEqPolynomial(pcs[1], w)
    g = cozk.LayerGroup(d, plain)
    claim, r = _fr(cozk, rng.field()), _fr(cozk, rng.field())
    out = np.zeros((16, 4), dtype=np.uint64)
    assert l.cozk_layer_group_round(None, eq.h, None, claim.ctypes.data, out.ctypes.data) == INVALID
    assert l.cozk_layer_group_final(None, eq.h, None, 0, out.ctypes.data) == INVALID
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, None, None, claim.ctypes.data, out.ctypes.data), "layer_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, eq.h, None, None, out.ctypes.data), "layer_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, eq.h, None, claim.ctypes.data, None), "layer_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, eq_other.h, None, claim.ctypes.data, out.ctypes.data),
                    "layer_group_round: the eq polynomial must be the driver's")
    _expect_invalid(cozk, d, l.cozk_layer_group_final(g.h, None, None, 0, out.ctypes.data), "layer_group_final: null argument")
    _expect_invalid(cozk, d, l.cozk_layer_group_final(g.h, eq.h, None, 0, None), "layer_group_final: null argument")
    _expect_invalid(cozk, d, l.cozk_layer_group_final(g.h, eq_other.h, None, 0, out.ctypes.data), "layer_group_final: the eq polynomial must be the driver's")
    for k_final in (-1, 5):
        _expect_invalid(cozk, d, l.cozk_layer_group_final(g.h, eq.h, None, k_final, out.ctypes.data), "layer_group_final: 0 <= k_final <= k")
    # 16 elements are not down to their claims, with a bind or without
    for rr in (None, r):
        _expect_invalid(cozk, d, l.cozk_layer_group_final(g.h, eq.h, rr.ctypes.data if rr is not None else None, 4, out.ctypes.data),
                        "layer_group_final: the members must be fully bound (len == 2) after the bind")
    assert (out == 0).all() and eq.lens() == (4, 2)
    _same(plain, one)  # nothing ran

    # a member that was driven on its own has another length: refused until the others have caught up
    eq1 = cozk.SplitEqPolynomial(plain[1].ctx, w)
    _single_round(plain[1], eq1, None, claim)
    _single_round(plain[1], eq1, r, claim)
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, eq.h, None, claim.ctypes.data, out.ctypes.data), "layer_group_round: the members must have one length")
    for m in (0, 2, 3):
        e = cozk.SplitEqPolynomial(plain[m].ctx, w)
        _single_round(plain[m], e, None, claim)
        _single_round(plain[m], e, r, claim)
    d.check(l.cozk_spliteq_bind(d.h, eq.h, r.ctypes.data))

    # ... and then the members still work: the rest of the rounds by the group, against the per-layer calls on the clones
    eq_s = [cozk.SplitEqPolynomial(x.ctx, w) for x in one]
    for m in range(4):
        _single_round(one[m], eq_s[m], None, claim)
        _single_round(one[m], eq_s[m], r, claim)
    _same(plain, one)
    r2 = _fr(cozk, rng.field())
    rc, got = _group_round(l, g, eq, r2, claim, 4)
    d.check(rc)
    for m in range(4):
        assert np.array_equal(got[4 * m:4 * m + 4], _single_round(one[m], eq_s[m], r2, claim))
    r3 = _fr(cozk, rng.field())
    rc, got = _group_final(l, g, eq, r3, 4)
    d.check(rc)
    for m in range(4):
        assert np.array_equal(got[4 * m:4 * m + 4], _single_final(one[m], r3))
    _same(plain, one)

    # fully bound: the members are down to their two claims, and so is the eq
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g.h, eq.h, r.ctypes.data, claim.ctypes.data, out.ctypes.data),
                    "layer_group_round: the members are already fully bound")
    assert eq.lens() == (1, 1)
    g4 = cozk.LayerGroup(d, _members(cozk, pcs, "plain", 2, 4, seed=10))
    _expect_invalid(cozk, d, l.cozk_layer_group_round(g4.h, eq.h, r.ctypes.data, claim.ctypes.data, out.ctypes.data),
                    "layer_group_round: eq polynomial already fully bound")
    _expect_invalid(cozk, d, l.cozk_layer_group_final(g4.h, eq.h, r.ctypes.data, 2, out.ctypes.data), "layer_group_final: eq polynomial already fully bound")
    assert [len(x) for x in g4.layers] == [4, 4]
    g.free()
    _same(plain, one)
    assert l.cozk_layer_group_free(None) == 0


def test_member_on_another_device_is_refused(cozk, party_ctxs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    l = cozk._lib.lib()
    other = cozk.Context(1)
    here = _members(cozk, party_ctxs, "plain", 1, 8, seed=1)
    there = _members(cozk, [other], "plain", 1, 8, seed=2)
    h = ctypes.c_void_p(SENT)
    rc = l.cozk_layer_group_create(party_ctxs[0].h, _arr(here + there), 2, ctypes.byref(h))
    _expect_invalid(cozk, party_ctxs[0], rc, "layer_group_create: every member must live on the driver's device")
    assert h.value is None
    g = cozk.LayerGroup(party_ctxs[0], here)  # the member here still serves
    g.free()
    del there
    other.close()
