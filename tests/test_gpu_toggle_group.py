"""GPU tests of the toggle groups (cozk_toggle_group_create / _layer_outputs / _round / _bind / _final_claims / _free): ONE PLAIN
toggle layer with k fingerprint planes over one copy of the public flags.  The yardstick is k separate PLAIN toggle layers driven
by cozk_toggle_round, cozk_toggle_bind, cozk_toggle_layer_output and cozk_toggle_final_claims, which test_gpu_lookups.py holds to
the oracle, and at the sizes where Python is quick oracle/pysparse.py itself.  Bar: bit-exact, raw Montgomery limbs through the C ABI
(ctypes).  No test provokes a device fault: every bad argument is refused on the host before any launch."""
import ctypes
import importlib

import numpy as np
import pytest

import pyref as O
import pysparse as SP
from test_gpu_shamir import EDGE_MONT
from test_gpu_shamir_gp import SENT, _expect_invalid, party_ctxs  # noqa: F401

pytestmark = pytest.mark.gpu
R = O.R
PY_MAX = 2048  # fingerprints per member x members up to which the big-int oracle runs too


def _lk():
    return importlib.import_module("co-zkvms_amd.lookups")


def _fr(cozk, x):
    return np.ascontiguousarray(cozk.fr_to_mont_limbs([x])[0])


def _instance(cozk, pcs, n_pairs, n, density, k, seed):
    """flag indices per pair, their U8 Vecs on the driver pcs[0], and k fingerprint planes (ints, and Vecs with member m on context
    m mod 8) that start with the field's corner values"""
    rng = O.SplitMix64(seed)
    idx = [sorted(i for i in range(n) if rng.next() % 100 < density) for _ in range(n_pairs)]
    fl = [cozk.Vec.from_ints(pcs[0], [1 if i in set(s) else 0 for i in range(n)], kind=cozk.SCALAR_U8) for s in idx]
    total = 2 * n_pairs * n
    edge = [0, 1, R - 1, R - 2] + EDGE_MONT
    ints = [(edge + O.synthetic_fr(seed + 1 + m, total))[:total] for m in range(k)]
    fps = [cozk.Vec.from_ints(pcs[m % len(pcs)], ints[m]) for m in range(k)]
    return idx, fl, ints, fps


def _group_round(l, g, eq, r, k):
    out = np.full((3 * k, 4), 0xA5, dtype=np.uint64)
    rc = l.cozk_toggle_group_round(g.h, eq.h, r.ctypes.data if r is not None else None, out.ctypes.data)
    return rc, out


def _single_round(t, eq, r):
    out = np.zeros((3, 4), dtype=np.uint64)
    t.ctx.check(t._l.cozk_toggle_round(t.ctx.h, t.h, eq.h, r.ctypes.data if r is not None else None, 0, out.ctypes.data))
    return out


def _layer_raw(layer):
    n = len(layer)
    a, b = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    layer.ctx.check(layer.ctx._l.cozk_layer_download(layer.ctx.h, layer.h, a.ctypes.data, b.ctypes.data))
    return a


def _run(cozk, pcs, n_pairs, n, density, k):
    """outputs, every round until the group is fully bound, the last bind and the final claims: the group against k PLAIN toggle
    layers, each with an eq of its own on its own context"""
    lk, l = _lk(), cozk._lib.lib()
    idx, fl, ints, fps = _instance(cozk, pcs, n_pairs, n, density, k, seed=1000 * n + 10 * k + n_pairs)
    before = [v.to_numpy().copy() for v in fps]
    group = lk.ToggleGroup(pcs[0], fl, fps)
    singles = [lk.ToggleLayer.from_vecs(v.ctx, fl, v) for v in fps]
    use_py = 2 * n_pairs * n * k <= PY_MAX
    py = [SP.ToggleLayer(idx, [row[b * n:(b + 1) * n] for b in range(2 * n_pairs)], 0, 1) for row in ints] if use_py else []
    # layer outputs: one launch for all members, each an FR vector of its owner
    outs = group.layer_outputs([v.ctx for v in fps])
    for m in range(k):
        assert outs[m].ctx is fps[m].ctx and len(outs[m]) == 2 * n_pairs * n
        assert np.array_equal(outs[m].to_numpy(), _layer_raw(singles[m].layer_output())), "member %d" % m
    nv = (2 * n_pairs - 1).bit_length() + n.bit_length() - 1
    rng = O.SplitMix64(77 * n + k)
    w = [rng.field() for _ in range(nv)]
    eq_g = cozk.SplitEqPolynomial(pcs[0], w)
    eq_s = [cozk.SplitEqPolynomial(t.ctx, w) for t in singles]
    eq_py = [O.SplitEq(w) for _ in py]
    r, r_int, seen = None, None, set()
    for j in range(nv):
        if j:
            for t, e in zip(py, eq_py):
                t.bind(r_int)
                e.bind(r_int)
        rc, got = _group_round(l, group, eq_g, r, k)
        pcs[0].check(rc)
        seen.add(eq_g.lens()[0] != 1)  # nested (E1 x E2) or flat (E2 alone)
        for m in range(k):
            assert np.array_equal(got[3 * m:3 * m + 3], _single_round(singles[m], eq_s[m], r)), "round %d member %d" % (j, m)
            assert eq_s[m].lens() == eq_g.lens()
        if use_py:
            gi = cozk.mont_limbs_to_int(got)
            for m in range(k):
                ev = py[m].compute_cubic_evals(eq_py[m], 0)
                assert gi[3 * m:3 * m + 3] == [ev[0] % R, ev[2] % R, ev[3] % R], "round %d member %d" % (j, m)
        r_int = rng.field()
        r = _fr(cozk, r_int)
    if nv >= 2:
        assert seen == {True, False}  # both eq layouts
    # a binding round would leave nothing to sum: refused, and nothing moves
    rc, _ = _group_round(l, group, eq_g, r, k)
    _expect_invalid(cozk, pcs[0], rc, "toggle_group_round: the bind leaves the group fully bound")
    group.bind(r_int)
    for t in singles:
        t.bind(r_int)
    for k_final in sorted({k, (k + 1) // 2, 0}):
        flag, fpc = group.final_claims(k_final)
        assert len(fpc) == k_final
        for m in range(k_final):
            assert (flag, fpc[m]) == singles[m].final_claims(), "member %d" % m
    if use_py:
        for t in py:
            t.bind(r_int)
        flag, fpc = group.final_claims()
        assert [(flag, x) for x in fpc] == [(t.final_claims()[0] % R, t.final_claims()[1] % R) for t in py]
    # fully bound: no round, no bind
    rc, _ = _group_round(l, group, eq_g, None, k)
    _expect_invalid(cozk, pcs[0], rc, "toggle_group_round: the group is fully bound")
    _expect_invalid(cozk, pcs[0], l.cozk_toggle_group_bind(group.h, r.ctypes.data), "toggle_group_bind: the group is fully bound")
    group.free()
    for m in range(k):  # the inputs are only read, and outlive the group
        assert np.array_equal(fps[m].to_numpy(), before[m])
    for s, v in zip(idx, fl):
        assert v.to_ints() == [1 if i in set(s) else 0 for i in range(n)]


# (n_pairs, N, density %, k): coalesces at the first bind; batch 6 padded to 8; -; no active pair; the queue flushes on every step; a
# flush that leaves a remainder in the queue, and every member chunk; the largest group
SHAPES = [(1, 2, 50, 1), (3, 8, 60, 3), (2, 64, 15, 5), (5, 4, 0, 3), (1, 512, 100, 3), (2, 2048, 70, 15), (1, 256, 30, 32)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "p%d-N%d-d%d-k%d" % s)
def test_group_equals_separate_toggle_layers(cozk, party_ctxs, shape):
    _run(cozk, party_ctxs, *shape)


def test_group_with_many_pairs_per_lane(cozk, party_ctxs, monkeypatch):
    monkeypatch.setenv("COZK_SUM_GRID_MAX", "1")
    _run(cozk, party_ctxs, 2, 2048, 70, 5)


def test_take_ownership_adopts_the_planes(cozk, party_ctxs):
    lk = _lk()
    idx, fl, ints, fps = _instance(cozk, party_ctxs, 1, 8, 50, 3, seed=5)
    keep = [cozk.Vec.from_ints(v.ctx, x) for v, x in zip(fps, ints)]
    want = lk.ToggleGroup(party_ctxs[0], fl, keep).layer_outputs()
    group = lk.ToggleGroup(party_ctxs[0], fl, fps, take_ownership=True)
    assert all(len(v) == 0 for v in fps)  # adopted
    got = group.layer_outputs()
    for a, b in zip(got, want):
        assert np.array_equal(a.to_numpy(), b.to_numpy())
    group.free()


def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l, lk = cozk._lib.lib(), _lk()
    p0, p1 = party_ctxs[0], party_ctxs[1]
    mk = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    arr = lambda vs: (ctypes.c_void_p * 40)(*([x.h.value if x is not None else None for x in vs] + [None] * (40 - len(vs))))
    F = [mk(p0, [1, 0, 1, 1], cozk.SCALAR_U8)]                      # one pair, N = 4
    good = [mk(party_ctxs[m], list(range(1, 9))) for m in range(3)]  # 2 circuits x 4

    def create(driver, flags, n_pairs, fps, k, text):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_toggle_group_create(driver.h if driver else None, arr(flags) if flags is not None else None, n_pairs, arr(fps) if fps is not None else None, k,
                                        0, ctypes.byref(h))
        if driver:
            _expect_invalid(cozk, driver, rc, "toggle_group_create: " + text)
        assert rc == -1 and h.value is None

    create(None, F, 1, good, 3, "")
    create(p0, None, 1, good, 3, "null argument")
    create(p0, F, 1, None, 3, "null argument")
    create(p0, F, 0, good, 3, "null argument")
    create(p0, F, 1, good, 0, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(p0, F, 1, good * 11, 33, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(p0, F, 1, [good[0], None, good[2]], 3, "null fingerprint vector")
    create(p0, F, 1, [good[0], mk(p1, list(range(8)), cozk.SCALAR_U32), good[2]], 3, "the fingerprints must be FR vectors")
    create(p0, F, 1, [good[0], mk(p1, list(range(1, 5))), good[2]], 3, "the fingerprint vectors must have one length")
    create(p0, F, 1, [good[0], good[0], good[2]], 3, "duplicate fingerprint vector")
    create(p0, F, 1, [mk(p0, list(range(1, 8)))], 1, "fingerprints.len() must be 2 * n_pairs * N")
    create(p0, [mk(p0, [1, 0, 1], cozk.SCALAR_U8)], 1, [mk(p0, list(range(1, 7)))], 1, "fingerprints per circuit must be a power of two >= 2")
    create(p0, [mk(p0, [1], cozk.SCALAR_U8)], 1, [mk(p0, [1, 2])], 1, "fingerprints per circuit must be a power of two >= 2")
    create(p0, [None], 1, good, 3, "every flag column is a U8 vector of N entries")
    create(p0, [mk(p0, [1, 0, 1, 1], cozk.SCALAR_U32)], 1, good, 3, "every flag column is a U8 vector of N entries")
    create(p0, [mk(p0, [1, 0], cozk.SCALAR_U8)], 1, good, 3, "every flag column is a U8 vector of N entries")
    assert l.cozk_toggle_group_create(p0.h, arr(F), 1, arr(good), 3, 0, None) == -1

    g = lk.ToggleGroup(p0, F, good)
    eq0, eq1 = cozk.SplitEqPolynomial(p0, [3, 5, 7]), cozk.SplitEqPolynomial(p1, [3, 5, 7])
    out = np.zeros((9, 4), dtype=np.uint64)
    fl4, fp12 = np.zeros(4, dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    r = _fr(cozk, 11)
    o = (ctypes.c_void_p * 40)(*([SENT] * 40))
    _expect_invalid(cozk, p0, l.cozk_toggle_group_layer_outputs(g.h, None, o), "toggle_group_layer_outputs: null argument")
    assert all(o[m] is None for m in range(3)) and o[3] == SENT
    o = (ctypes.c_void_p * 40)(*([SENT] * 40))
    _expect_invalid(cozk, p0, l.cozk_toggle_group_layer_outputs(g.h, (ctypes.c_void_p * 3)(p0.h, None, p0.h), o), "toggle_group_layer_outputs: null owner")
    assert all(o[m] is None for m in range(3))
    assert l.cozk_toggle_group_layer_outputs(g.h, (ctypes.c_void_p * 3)(p0.h, p0.h, p0.h), None) == -1
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, None, None, out.ctypes.data), "toggle_group_round: null argument")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq0.h, None, None), "toggle_group_round: null argument")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq1.h, None, out.ctypes.data), "toggle_group_round: the eq polynomial must be the driver's")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_bind(g.h, None), "toggle_group_bind: null argument")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_final_claims(g.h, fl4.ctypes.data, fp12.ctypes.data, 3), "toggle_group_final_claims: the group is not fully bound")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_final_claims(g.h, fl4.ctypes.data, fp12.ctypes.data, 4), "toggle_group_final_claims: 0 <= k_final <= k")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_final_claims(g.h, fl4.ctypes.data, fp12.ctypes.data, -1), "toggle_group_final_claims: 0 <= k_final <= k")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_final_claims(g.h, None, fp12.ctypes.data, 3), "toggle_group_final_claims: null argument")
    # nothing ran: the group still proves from the start, and equals a fresh one
    first = g.round(eq0)
    fresh = lk.ToggleGroup(p0, F, good)  # the twin: it sees no refused call
    eq_f = cozk.SplitEqPolynomial(p0, [3, 5, 7])
    assert first == fresh.round(eq_f)
    # a fully bound eq polynomial: refused before the group or that eq polynomial binds -- the next round equals the twin's
    eq_b = cozk.SplitEqPolynomial(p0, [3])
    eq_b.bind(5)
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq_b.h, r.ctypes.data, out.ctypes.data), "toggle_group_round: eq polynomial already fully bound")
    assert eq_b.lens() == (1, 1) and eq0.lens() == eq_f.lens()
    assert g.round(eq0, 11) == fresh.round(eq_f, 11)
    _expect_invalid(cozk, p0, l.cozk_toggle_group_layer_outputs(g.h, (ctypes.c_void_p * 3)(p0.h, p0.h, p0.h), o), "toggle_group_layer_outputs: needs an unbound group")
    assert g.round(eq0, 13) == fresh.round(eq_f, 13)
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq0.h, r.ctypes.data, out.ctypes.data), "toggle_group_round: the bind leaves the group fully bound")
    assert eq0.lens() == eq_f.lens()
    g.bind(17)
    fresh.bind(17)
    claims = g.final_claims(3)
    assert claims == fresh.final_claims(3)
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq0.h, r.ctypes.data, out.ctypes.data), "toggle_group_round: the group is fully bound")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_round(g.h, eq0.h, None, out.ctypes.data), "toggle_group_round: the group is fully bound")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_bind(g.h, r.ctypes.data), "toggle_group_bind: the group is fully bound")
    _expect_invalid(cozk, p0, l.cozk_toggle_group_final_claims(g.h, fl4.ctypes.data, fp12.ctypes.data, 4), "toggle_group_final_claims: 0 <= k_final <= k")
    assert len(g.final_claims(3)[1]) == 3
    assert g.final_claims(3) == claims and eq0.lens() == eq_f.lens()  # the refused calls on the fully bound group changed nothing
    assert [v.to_ints() for v in good] == [list(range(1, 9))] * 3


def test_fingerprints_on_another_device_are_refused(cozk, party_ctxs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = cozk.Context(1)
    try:
        F = [cozk.Vec.from_ints(party_ctxs[0], [1, 0, 1, 1], kind=cozk.SCALAR_U8)]
        fps = [cozk.Vec.from_ints(party_ctxs[0], list(range(1, 9))), cozk.Vec.from_ints(other, list(range(1, 9)))]
        with pytest.raises(cozk.CozkError) as e:
            _lk().ToggleGroup(party_ctxs[0], F, fps)
        assert e.value.code == -1 and "every fingerprint vector must live on the driver's device" in str(e.value)
    finally:
        other.close()
