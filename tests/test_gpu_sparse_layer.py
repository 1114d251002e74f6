"""GPU parity of the sparse pair layers (cozk_sparse_layer_*, csrc/sparse_layer.inc) with the oracle's LITERAL restatement of
Rep3SparseInterleavedPolynomial (oracle/pysparse.py: SparseLayer, sparse_layer_output, toggled_construct).  The object is forced sparse
whatever its density (the storage rule belongs to the prover): 0 % (nothing stored), 100 % (every pair stored), batches that are no
power of two, and a layer that spans several workgroups and scan tiles.

The dense formulation pads a ragged tail with zeros where a sparse layer reads a missing pair as ones, so a sparse layer runs the
rounds whose length is a multiple of 4 -- every round down to the coalesce point, and every round of a power-of-two batch; the bind
after the last such round is still compared with the oracle."""
import copy
import functools
import importlib

import pytest

import pyref as O
import pysparse as S
from sparse_tiles_ref import opened as _opened, sumcheck as _sumcheck  # the round driver, shared with test_gpu_sparse_tiles.py

pytestmark = pytest.mark.gpu
R = O.R
SHAPES = [(4, 16, 30, 3), (6, 8, 60, 1), (10, 4, 50, 1), (2, 2, 100, 3), (4, 8, 0, 1), (8, 256, 10, 3), (6, 4096, 10, 1)]
REP3_SHAPES = [s for s in SHAPES if s[3] == 3]
KEYS = [bytes([17 * (p + 1) + i for i in range(32)]) for p in range(3)]  # KEYS[p]: shared by party p and party p + 1


def _instance(batch, n, density, seed, nparties):
    """as tests/test_gpu_lookups.py builds its instances"""
    rng = O.SplitMix64(seed)
    cols = [[1 if rng.next() % 100 < density else 0 for _ in range(n)] for _ in range(batch // 2)]
    vals = [[rng.field() for _ in range(n)] for _ in range(batch)]
    if nparties == 1:
        fps = [vals]
    else:
        sh = [[O.rep3_share(v, rng) for v in row] for row in vals]
        fps = [[[s[p] for s in row] for row in sh] for p in range(3)]
    return cols, vals, fps


@functools.lru_cache(maxsize=None)
def _case(batch, n, density, nparties):
    """the instance and the oracle's tree, computed once per shape and never changed (the tests work on deep copies)"""
    cols, vals, fps = _instance(batch, n, density, 100 + batch + n, nparties)
    flag_indices = [[i for i, f in enumerate(c) if f] for c in cols]
    toggles, sparse = S.toggled_construct(flag_indices, fps)
    return cols, fps, sparse


def _lk():
    return importlib.import_module("co-zkvms_amd.lookups")


def _stored_pairs(cols, batch, n):
    return [b * (n // 2) + i // 2 for b in range(batch) for i in range(0, n, 2) if cols[b // 2][i] | cols[b // 2][i + 1]]


@pytest.mark.parametrize("batch,n,density,nparties", SHAPES)
def test_toggle_output_scattered_equals_the_dense_toggle_output(cozk, ctx, batch, n, density, nparties):
    LK = _lk()
    cols, fps, sparse = _case(batch, n, density, nparties)
    want_idx = _stored_pairs(cols, batch, n)
    for p in range(nparties):
        tg = LK.ToggleLayer(ctx, cols, fps[p])
        sp = LK.SparseLayer.from_toggle(ctx, tg, party=p)
        assert len(sp) == batch * n
        assert sp.count == len(want_idx)
        assert sp.nbytes == len(want_idx) * (64 * (2 if nparties == 3 else 1) + 4)
        idx, pairs = sp.download()
        assert idx == want_idx
        dense, ref = sp.to_dense(party=p), tg.layer_output(party=p)
        got = dense.coeffs()
        assert got == ref.coeffs()
        assert got == sparse[0][p].coalesce()
        assert pairs == [(got[2 * j], got[2 * j + 1]) for j in idx]
        for o in (dense, ref, sp, tg):
            o.free()


@pytest.mark.parametrize("batch,n,density,nparties", SHAPES)
def test_layer0_rounds_and_binds_match_the_sparse_oracle_per_party(cozk, ctx, batch, n, density, nparties):
    LK = _lk()
    cols, fps, sparse = _case(batch, n, density, nparties)
    tgs = [LK.ToggleLayer(ctx, cols, fps[p]) for p in range(nparties)]
    devs = [LK.SparseLayer.from_toggle(ctx, tgs[p], party=p) for p in range(nparties)]
    forms = _sumcheck(cozk, ctx, devs, [copy.deepcopy(sparse[0][p]) for p in range(nparties)], 5, exact=True)
    assert "nested" in forms
    if batch & (batch - 1) == 0 and batch * n >= 16:  # a power-of-two batch runs to the last round: the flat table once E1 is bound
        assert forms == {"flat", "nested"}
    for o in devs + tgs:
        o.free()


def _climb(ctx, LK, sp, nparties, masked):
    """one level up the tree for every party: output_local, the ring reshare of the compact vectors (Rep3), from_output"""
    counter = 1000
    vas = [sp[p].output_local(masked=masked, key_self=KEYS[p], key_prev=KEYS[(p + 2) % 3], counter=counter) for p in range(nparties)]
    G = sp[0].next_count()
    assert all(len(v) == 2 * G for v in vas)
    if nparties == 1:
        return [sp[0].from_output(vas[0])], vas
    host = [v.to_numpy() for v in vas]
    vbs = [cozk_vec_from(ctx, host[(p + 2) % 3]) for p in range(3)]  # c.b = the previous party's c.a
    return [sp[p].from_output(vas[p], vbs[p]) for p in range(3)], vas


def cozk_vec_from(ctx, limbs):
    E = importlib.import_module("co-zkvms_amd.engine")
    return E.Vec.from_numpy(ctx, limbs)


@pytest.mark.parametrize("batch,n,density,nparties", SHAPES)
def test_plain_higher_layers_match_the_sparse_oracle(cozk, ctx, batch, n, density, nparties):
    LK = _lk()
    cols, fps, sparse = _case(batch, n, density, 1)
    tg = LK.ToggleLayer(ctx, cols, fps[0])
    layers = [[LK.SparseLayer.from_toggle(ctx, tg, party=0)]]
    for li in range(1, min(3, len(sparse))):  # layers 1 and 2, where the tree has them
        nxt, _ = _climb(ctx, LK, layers[-1], 1, masked=False)
        assert nxt[0].count == layers[-1][0].next_count() and len(nxt[0]) == len(layers[-1][0]) // 2
        dense = nxt[0].to_dense(party=0)
        assert dense.coeffs() == sparse[li][0].coalesce()
        dense.free()
        layers.append(nxt)
    for li in range(1, len(layers)):
        _sumcheck(cozk, ctx, layers[li], [copy.deepcopy(sparse[li][0])], 40 + li, exact=True)
    for o in [l[0] for l in layers] + [tg]:
        o.free()


@pytest.mark.parametrize("batch,n,density,nparties", REP3_SHAPES)
def test_rep3_higher_layers_open_to_the_oracle_and_the_masks_cancel(cozk, ctx, batch, n, density, nparties):
    LK = _lk()
    cols, fps, sparse = _case(batch, n, density, 3)
    tgs = [LK.ToggleLayer(ctx, cols, fps[p]) for p in range(3)]
    layers = [[LK.SparseLayer.from_toggle(ctx, tgs[p], party=p) for p in range(3)]]
    for li in range(1, min(3, len(sparse))):
        plain = [s.output_local(masked=False).to_ints() for s in layers[-1]]
        nxt, vas = _climb(ctx, LK, layers[-1], 3, masked=True)
        masked = [v.to_ints() for v in vas]
        if masked[0]:
            assert all(masked[p] != plain[p] for p in range(3))  # the masks are on ...
        assert [sum(c) % R for c in zip(*masked)] == [sum(c) % R for c in zip(*plain)]  # ... and cancel
        dense = [nxt[p].to_dense(party=p) for p in range(3)]
        assert _opened([d.coeffs() for d in dense]) == _opened([sparse[li][p].coalesce() for p in range(3)])
        for d in dense:
            d.free()
        layers.append(nxt)
    for li in range(1, len(layers)):
        _sumcheck(cozk, ctx, layers[li], [copy.deepcopy(sparse[li][p]) for p in range(3)], 60 + li, exact=False)
    for o in [s for l in layers for s in l] + tgs:
        o.free()


def test_create_from_explicit_lists_round_trips_through_download(cozk, ctx):
    LK = _lk()
    rng = O.SplitMix64(9)
    idx = [0, 1, 4, 7]
    plain = [(rng.field(), rng.field()) for _ in idx]
    sp = LK.SparseLayer.from_lists(ctx, 16, idx, plain)
    assert (len(sp), sp.count, sp.nbytes, sp.next_count()) == (16, 4, 4 * 68, 3)
    assert sp.download() == (idx, plain)
    want = [1] * 16
    for j, (l, r) in zip(idx, plain):
        want[2 * j], want[2 * j + 1] = l, r
    dense = sp.to_dense()
    assert dense.coeffs() == want
    dense.free()
    sp.free()
    shares = [((rng.field(), rng.field()), (rng.field(), rng.field())) for _ in idx]
    sp = LK.SparseLayer.from_lists(ctx, 16, idx, shares)
    assert (sp.count, sp.nbytes) == (4, 4 * 132)
    assert sp.download() == (idx, shares)
    dense = sp.to_dense(party=1)
    got = dense.coeffs()
    assert [got[2 * j] for j in idx] == [s[0] for s in shares] and got[4] == (0, 1)
    dense.free()
    sp.free()
    empty = LK.SparseLayer.from_lists(ctx, 8, [], [])
    assert (empty.count, empty.nbytes, empty.next_count()) == (0, 0, 0) and empty.download() == ([], [])
    dense = empty.to_dense()
    assert dense.coeffs() == [1] * 8
    dense.free()
    empty.free()


def test_refusals_leave_out_null_and_the_object_usable(cozk, ctx):
    LK = _lk()
    E = importlib.import_module("co-zkvms_amd.engine")
    LB = importlib.import_module("co-zkvms_amd._lib")
    rng = O.SplitMix64(3)
    idx = [0, 2, 3]
    pairs = [(rng.field(), rng.field()) for _ in idx]
    flat = [v for pr in pairs for v in pr]
    iv, av = E.Vec.from_ints(ctx, idx, kind=LB.SCALAR_U32), E.Vec.from_ints(ctx, flat)

    def refused(fn, *a, **k):
        with pytest.raises(cozk.CozkError) as ei:
            fn(*a, **k)
        assert ei.value.code == -1 and len(str(ei.value)) > len("cozk error -1: ")

    mk = LK.SparseLayer.from_vecs
    refused(mk, ctx, LB.MODE_PLAIN, 8, E.Vec.from_ints(ctx, idx, kind=LB.SCALAR_U64), av)          # idx not U32
    refused(mk, ctx, LB.MODE_PLAIN, 8, E.Vec.from_ints(ctx, [0, 3, 2], kind=LB.SCALAR_U32), av)    # not increasing
    refused(mk, ctx, LB.MODE_PLAIN, 8, E.Vec.from_ints(ctx, [0, 2, 2], kind=LB.SCALAR_U32), av)    # not strictly
    refused(mk, ctx, LB.MODE_PLAIN, 8, E.Vec.from_ints(ctx, [0, 2, 4], kind=LB.SCALAR_U32), av)    # index >= n / 2
    refused(mk, ctx, LB.MODE_PLAIN, 8, iv, E.Vec.from_ints(ctx, flat[:5]))                         # wrong length
    refused(mk, ctx, LB.MODE_PLAIN, 8, iv, E.Vec.from_ints(ctx, [1] * 6, kind=LB.SCALAR_U64))      # wrong kind
    refused(mk, ctx, LB.MODE_REP3, 8, iv, av)                                                      # Rep3 without b
    refused(mk, ctx, LB.MODE_REP3, 8, iv, av, E.Vec.from_ints(ctx, flat[:4]))                      # b of the wrong length
    refused(mk, ctx, LB.MODE_PLAIN, 7, iv, av)                                                     # n odd
    refused(mk, ctx, LB.MODE_PLAIN, 0, E.Vec.from_ints(ctx, [], kind=LB.SCALAR_U32), E.Vec.alloc(ctx, 0))  # n below 2
    refused(mk, ctx, 7, 8, iv, av)                                                                 # no such mode
    l = LB.lib()
    import ctypes
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_create(ctx.h, LB.MODE_PLAIN, 8, iv.h, None, None, 0, ctypes.byref(h)) == -1 and h.value is None  # null values
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_create(ctx.h, LB.MODE_PLAIN, 7, iv.h, av.h, None, 0, ctypes.byref(h)) == -1 and h.value is None

    sp = mk(ctx, LB.MODE_PLAIN, 8, iv, av)
    w = [rng.field(), rng.field()]
    eq = cozk.SplitEqPolynomial(ctx, w)
    other = cozk.Context(0)
    try:
        foreign = cozk.SplitEqPolynomial(other, w)
        refused(sp.round, foreign)                      # an eq of another context
        foreign.free()
    finally:
        other.close()
    first = sp.round(eq)
    eq.bind(rng.field())
    eq.bind(rng.field())
    refused(sp.round, eq)                               # a fully bound eq
    refused(sp.round, cozk.SplitEqPolynomial(ctx, w), party=5)
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_to_dense(ctx.h, sp.h, 9, ctypes.byref(h)) == -1 and h.value is None
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_from_output(ctx.h, sp.h, av.h, None, 0, ctypes.byref(h)) == -1 and h.value is None  # 6 values for 2 groups
    r = rng.field()
    sp.bind(r)                                          # 8 -> 4
    assert (len(sp), sp.count) == (4, 2)
    sp.bind(r)                                          # 4 -> 2: one pair
    assert (len(sp), sp.count) == (2, 1)
    stored = sp.download()
    refused(sp.bind, r)                                 # fewer than one pair
    refused(sp.round, cozk.SplitEqPolynomial(ctx, w), r)
    refused(sp.output_local)                            # a length that is no multiple of 4
    assert (len(sp), sp.count) == (2, 1)
    assert sp.download() == stored                      # the refused bind and round moved no value
    dense = sp.to_dense()
    assert len(dense.coeffs()) == 2
    dense.free()
    sp.free()
    # the object is usable after a refusal: the same round again gives the same values
    sp = mk(ctx, LB.MODE_PLAIN, 8, iv, av)
    refused(sp.round, cozk.SplitEqPolynomial(ctx, w), party=5)
    assert sp.round(cozk.SplitEqPolynomial(ctx, w)) == first
    sp.free()


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_round_refusals_leave_layer_eq_and_party_untouched(cozk, ctx, mode):
    """every refusal of cozk_sparse_layer_round comes before the layer's bind, the eq polynomial's bind and the adoption of the party:
    a subject and a twin that sees no refused call, 16 dense entries (8 pairs, 4 stored) over an eq polynomial of three variables.
    Refused before the first round and after every round, each time with (length, count, stored pairs) and the eq tables unmoved:
      * a binding round over an eq polynomial with ONE variable left -- the bind would leave no round to run (a check behind
        the binds would move the layer and that eq polynomial and refuse afterwards);
      * a fully bound eq polynomial, asked as party 1: a Rep3 layer from explicit lists has no party yet and must not take this one
        (a layer that did would refuse the rounds of party 2 from then on);
      * a party out of range; at 4 entries, a binding round (the length would be no multiple of 4).
    Every round of the subject then equals the twin's, and so do the layers at the end."""
    LK = _lk()
    rng = O.SplitMix64(41 + (mode == "rep3"))
    n, idx, party = 16, [0, 2, 3, 6], (2 if mode == "rep3" else 0)
    val = (lambda: (rng.field(), rng.field())) if mode == "rep3" else rng.field
    pairs = [(val(), val()) for _ in idx]
    sp, twin = (LK.SparseLayer.from_lists(ctx, n, idx, pairs) for _ in range(2))
    w = [rng.field() for _ in range(3)]
    eq, eq_twin = cozk.SplitEqPolynomial(ctx, w), cozk.SplitEqPolynomial(ctx, w)
    one_left = cozk.SplitEqPolynomial(ctx, w[:1])
    bound = cozk.SplitEqPolynomial(ctx, w[:1])
    bound.bind(rng.field())
    spare = cozk.SplitEqPolynomial(ctx, w)  # never bound: three variables at every point
    assert one_left.lens() == (2, 1) and bound.lens() == (1, 1)

    def refused(text, *a, **k):
        with pytest.raises(cozk.CozkError) as ei:
            sp.round(*a, **k)
        assert ei.value.code == -1 and text in str(ei.value), str(ei.value)

    def state():
        return (len(sp), sp.count, sp.download(), eq.lens(), eq.download(), one_left.lens(), one_left.download(), bound.lens(), spare.lens())

    r = None
    for rnd in range(4):  # before round `rnd`: 16, 16, 8, 4 entries
        before = state()
        assert before[0] == (16, 16, 8, 4)[rnd]
        if rnd < 3:
            refused("sparse_layer_round: the bind would leave no round to run", one_left, rng.field(), party=party)
        refused("sparse_layer_round: eq polynomial already fully bound", bound, party=1)
        refused("sparse_layer_round: eq polynomial already fully bound", bound, rng.field(), party=1)
        refused("sparse_layer_round: the party must be 0..2", eq, None, party=5)
        assert sp._l.cozk_sparse_layer_round(ctx.h, sp.h, eq.h, None, party, None) == -1  # a NULL output
        if rnd == 3:
            refused("sparse_layer_round: the dense length must be a multiple of 4", spare, r, party=party)
        assert state() == before
        if rnd == 3:
            break
        assert sp.round(eq, r, party=party) == twin.round(eq_twin, r, party=party), rnd
        r = rng.field()
    assert (len(sp), sp.count, sp.download()) == (len(twin), twin.count, twin.download())
    assert (eq.lens(), eq.download()) == (eq_twin.lens(), eq_twin.download())
    sp.bind(r)
    twin.bind(r)
    assert (len(sp), sp.download()) == (2, twin.download())
    for x in (sp, twin, eq, eq_twin, one_left, bound, spare):
        x.free()
