"""The plain prover's grouped split-eq layer kernels, k_layer_cubic9<1, 2> and k_layer_bind_cubic9<1, 2> (csrc/poly.hip: layer9_terms /
layer9_walk / layer9_group_flush with NESTED == 2), against oracle/pyref.py at the smallest sizes at which layer_variant picks them:
a plain layer of >= 1024 chunks under an E1 table of >= 512 pairs.  Their path is their own -- one contiguous chunk range per
workgroup (`per` rounded up to 256), per-lane group sums keyed by x2 = c >> e1_shift, a flush on every change of group and one after
the loop, K3 at the end -- and every other test that reaches it runs layers a power of two long.

Shapes (cozk_spliteq_new: E1 = 2^(nv - nv / 2) entries, E2 = 2^(nv / 2)):
  A  nv = 19, E1 = 1024, E2 = 512, a group = 512 chunks: the sums alone.
       2^19 + 790: 131 270 chunks; the last chunk holds 2 elements, the last wave 6 chunks (the direct path), and of the 257 groups
                   the last has 198 chunks;
       2^19 + 2:   group 256 is one half-full chunk;
       2^20:       every wave staged, every group full.
  B  nv = 21, E1 = 2048 before the bind and 1024 after it, E2 = 1024: bind + sums.  2^21 + 790 elements bind to 262 243 output chunks,
     the last of them fed by one input chunk of 2 elements.
COZK_SUM_GRID_MAX (read on every call) pins the grid of 2^19 + 790 to 1 (513 walk iterations per lane: the lazy sums fold four
times), 3 (per = 43 776 chunks = 85.5 groups: workgroups 1 and 2 start in the middle of a group), 200 (per = 768 = 1.5 groups;
workgroups 171..199 have an empty range and must still write zero partials) and 512 (one group per workgroup, the upper half idle).
A pin only bites below the default grid, which comes from an occupancy query and is not asserted.  The pins are what sees a lane cross
from one group into the next at shape A: with the reset of the group sums on a change of group taken out, the default grid and
the pin to 512 (at most one group per lane) still pass and the pins to 1, 3 and 200 fail.

Every comparison is equality of field elements as integers.  The downloaded layers and the oracle's results are kept per
(length, seed) for the module, so all grid cases of a shape share one oracle evaluation."""
import importlib

import numpy as np
import pytest

import pyref as O

pytestmark = pytest.mark.gpu
GRID = "COZK_SUM_GRID_MAX"
RAGGED = (1 << 19) + 790
LENGTHS_A = [RAGGED, (1 << 19) + 2, 1 << 20]
LENGTH_B = (1 << 21) + 790
SEED = 61  # shape A and B layers, member 0 of the group; the other members and the Rep3 layer take seeds of their own


def _lib():
    return importlib.import_module("co-zkvms_amd._lib")


@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def _nv(length):
    """rounds of a layer's sumcheck (test_gpu_poly.py): the oracle's chunk_size and the kernel's E1_half then describe the same groups"""
    return ((length + 1) // 2 - 1).bit_length()


def _layer(cozk, ctx, length, mode, seed):
    a = cozk.Vec.random(ctx, length, seed)
    b = cozk.Vec.random(ctx, length, seed + 1) if mode == "rep3" else None
    return cozk.Rep3DenseInterleavedPolynomial.from_vecs(ctx, a, b, take_ownership=True)


def _raw(layer):
    n = len(layer)
    a = np.empty((n, 4), dtype=np.uint64)
    b = np.empty((n, 4), dtype=np.uint64)
    layer.ctx.check(layer.ctx._l.cozk_layer_download(layer.ctx.h, layer.h, a.ctypes.data, b.ctypes.data))
    return a if layer.mode == _lib().MODE_PLAIN else np.concatenate([a, b])


def _pin(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv(GRID, raising=False)
    else:
        monkeypatch.setenv(GRID, str(grid))


class _Case:
    """one seeded layer as downloaded, its challenges and claims, and the oracle's bound layers and round messages on it, each
    computed once and never modified"""

    def __init__(self, cozk, ctx, length, seed, mode):
        rng = O.SplitMix64(length * 11 + seed)
        self.length, self.seed, self.mode = length, seed, mode
        self.w = [rng.field() for _ in range(_nv(length))]
        self.rs = [rng.field() for _ in range(2)]
        self.claims = [rng.field() for _ in range(3)]
        lay = _layer(cozk, ctx, length, mode, seed)
        self._layers = [lay.coeffs()]
        lay.free()
        self._msgs = {}

    def eq(self, binds):
        e = O.SplitEq(self.w)
        for r in self.rs[:binds]:
            e.bind(r)
        return e

    def layer(self, binds):
        while len(self._layers) <= binds:
            self._layers.append(O.interleaved_bind(self._layers[-1], self.rs[len(self._layers) - 1]))
        return self._layers[binds]

    def message(self, binds):
        """the round message after `binds` binds, against claims[binds]"""
        if binds not in self._msgs:
            self._msgs[binds] = O.interleaved_compute_cubic(self.layer(binds), self.eq(binds), self.claims[binds])
        return self._msgs[binds]


_CASES = {}


def _case(cozk, ctx, length, seed, mode="plain"):
    if (length, seed) not in _CASES:
        _CASES[(length, seed)] = _Case(cozk, ctx, length, seed, mode)
    c = _CASES[(length, seed)]
    assert c.mode == mode
    return c


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _selected(layer, eq, mode="plain"):
    """what layer_variant (csrc/poly.hip) decides on, as the ABI shows it -- mirrors LAYER_GROUPED_MIN_E1H = 512 and
    LAYER_F9_MIN_CHUNKS = 1024: with a plain layer these pick NESTED = 2, and a change of either threshold fails here instead of
    sending the test through another kernel.  For the fused round call it after the round: the variant is chosen for the bound
    layer under the bound tables."""
    L = _lib()
    assert layer.mode == (L.MODE_PLAIN if mode == "plain" else L.MODE_REP3)
    assert eq.lens()[0] // 2 >= 512  # LAYER_GROUPED_MIN_E1H
    assert len(layer) // 4 >= 1024  # LAYER_F9_MIN_CHUNKS


# ---------------------------------------------------------------- 1: the sums alone
@pytest.mark.parametrize("length,grid", [(n, None) for n in LENGTHS_A] + [(RAGGED, g) for g in (1, 3, 200, 512)])
def test_compute_cubic_equals_the_oracle(cozk, ctx, monkeypatch, length, grid):
    c = _case(cozk, ctx, length, SEED)
    lay, eq = _layer(cozk, ctx, length, "plain", SEED), cozk.SplitEqPolynomial(ctx, c.w)
    assert eq.lens() == (1024, 512) and len(lay) == length
    _selected(lay, eq)
    _pin(monkeypatch, grid)
    assert lay.compute_cubic(eq, c.claims[0]) == c.message(0)
    lay.free()
    eq.free()


# ---------------------------------------------------------------- 2, 3: bind + sums
def _first_fused_round(cozk, ctx, c, check_layer):
    """round(eq, r0, claim) as the first call on a fresh shape B layer, against the oracle"""
    lay, eq = _layer(cozk, ctx, c.length, "plain", c.seed), cozk.SplitEqPolynomial(ctx, c.w)
    assert eq.lens() == (2048, 1024)
    got = lay.round(eq, c.rs[0], c.claims[1])
    ref_eq = c.eq(1)
    assert eq.lens() == (ref_eq.E1_len, ref_eq.E2_len) == (1024, 1024)
    assert len(lay) == 2 * ((c.length + 3) // 4)
    _selected(lay, eq)
    assert got == c.message(1)
    if check_layer:
        assert lay.coeffs() == c.layer(1)
    return lay, eq


@pytest.mark.parametrize("grid", [None, 1, 3, 200])
def test_first_fused_round_equals_the_oracle(cozk, ctx, monkeypatch, grid):
    c = _case(cozk, ctx, LENGTH_B, SEED)
    _pin(monkeypatch, grid)
    lay, eq = _first_fused_round(cozk, ctx, c, True)
    lay.free()
    eq.free()


def test_fused_round_after_the_variant_drops_to_1(cozk, ctx, monkeypatch):
    """the next round of shape B: E1 is down to 512 entries (256 pairs), so k_layer_bind_cubic9<1, 1> takes over on a layer that the
    grouped kernel wrote"""
    c = _case(cozk, ctx, LENGTH_B, SEED)
    _pin(monkeypatch, None)
    lay, eq = _first_fused_round(cozk, ctx, c, False)
    got = lay.round(eq, c.rs[1], c.claims[2])
    ref_eq = c.eq(2)
    assert eq.lens() == (ref_eq.E1_len, ref_eq.E2_len) == (512, 1024)
    assert eq.lens()[0] // 2 < 512 and len(lay) // 4 >= 1024  # below LAYER_GROUPED_MIN_E1H, still above LAYER_F9_MIN_CHUNKS
    assert got == c.message(2)
    assert lay.coeffs() == c.layer(2)
    lay.free()
    eq.free()


# ---------------------------------------------------------------- 4: worst-case operands
def test_all_r_minus_1_at_one_workgroup_equals_the_oracle(cozk, ctx, monkeypatch):
    """every element R - 1 under a random w, 513 chunks per lane: the group sums, the flushes and K3 stay inside the bounds that
    tests/test_fr9_model.py proves"""
    rng = O.SplitMix64(4)
    w = [rng.field() for _ in range(_nv(RAGGED))]
    claim = rng.field()
    limbs = np.tile(cozk.fr_to_mont_limbs([O.R - 1]), (RAGGED, 1))
    lay = cozk.Rep3DenseInterleavedPolynomial.from_vecs(ctx, cozk.Vec.from_numpy(ctx, limbs), take_ownership=True)
    eq = cozk.SplitEqPolynomial(ctx, w)
    _selected(lay, eq)
    _pin(monkeypatch, 1)
    assert lay.compute_cubic(eq, claim) == O.interleaved_compute_cubic([O.R - 1] * RAGGED, O.SplitEq(w), claim)
    lay.free()
    eq.free()


# ---------------------------------------------------------------- 6: the whole chain
def test_prove_rounds_equals_separate_calls(cozk, ctx, monkeypatch):
    """one proof through NESTED = 2 (round 0), 1, 0, the Montgomery kernels, the resident kernel and the host tail"""
    c = _case(cozk, ctx, RAGGED, SEED)
    nv = _nv(RAGGED)
    assert nv == 19
    rng = O.SplitMix64(6)
    rs = [rng.field() for _ in range(nv)]
    claims = [rng.field() for _ in range(nv)]
    _pin(monkeypatch, None)
    sep, eq_s = _layer(cozk, ctx, RAGGED, "plain", SEED), cozk.SplitEqPolynomial(ctx, c.w)
    _selected(sep, eq_s)
    expected, claim = [], c.claims[0]
    for j in range(nv):
        expected.append(sep.compute_cubic(eq_s, claim))
        sep.bind(rs[j])
        eq_s.bind(rs[j])
        claim = claims[j]
    assert expected[0] == c.message(0)
    one, eq_o = _layer(cozk, ctx, RAGGED, "plain", SEED), cozk.SplitEqPolynomial(ctx, c.w)
    seen = []

    def exchange(rnd, cf):
        seen.append(cf)
        return rs[rnd], claims[rnd]

    ctx.set_resident_rounds(True)
    try:
        got_r, final = one.prove_rounds(eq_o, c.claims[0], nv, exchange)
    finally:
        ctx.set_resident_rounds(None)
    assert seen == expected
    assert got_r == rs
    assert final == sep.final_claims()
    assert one.coeffs() == sep.coeffs()
    for x in (sep, one, eq_s, eq_o):
        x.free()


# ---------------------------------------------------------------- 7: Rep3 stays ungrouped
def test_rep3_compute_cubic_equals_the_oracle(cozk, ctx, monkeypatch):
    """the same length and tables under a Rep3 layer: only the mode keeps layer_variant at NESTED = 1 (k_layer_cubic9<2, 1>)"""
    c = _case(cozk, ctx, RAGGED, SEED + 100, "rep3")
    lay, eq = _layer(cozk, ctx, RAGGED, "rep3", SEED + 100), cozk.SplitEqPolynomial(ctx, c.w)
    _selected(lay, eq, "rep3")
    _pin(monkeypatch, None)
    assert lay.compute_cubic(eq, c.claims[0]) == c.message(0)
    lay.free()
    eq.free()


# ---------------------------------------------------------------- 5: layer group (last: its contexts then exist for this test alone)
@pytest.mark.parametrize("grid", [None, 3])
def test_layer_group_rows_equal_each_member_alone(cozk, ctx, party_ctxs, monkeypatch, grid):
    """three plain members with different data, one launch each on the driver's stream into the rows of one reservation: round 0
    (k_layer_cubic9<1, 2>) and the fused round 1 (E1 is then 512 entries: k_layer_bind_cubic9<1, 1>) against the members' own calls
    at the default grid"""
    c = _case(cozk, ctx, RAGGED, SEED)
    pcs = party_ctxs
    grp = [_layer(cozk, pcs[m], RAGGED, "plain", SEED + 10 * m) for m in range(3)]
    one = [x.clone() for x in grp]
    eq_g = cozk.SplitEqPolynomial(pcs[0], c.w)
    eq_s = [cozk.SplitEqPolynomial(x.ctx, c.w) for x in one]
    g = cozk.LayerGroup(pcs[0], grp)
    try:  # a failing assertion must not leave a layer behind its context, which the module's teardown closes
        _selected(grp[0], eq_g)
        _pin(monkeypatch, None)
        want0 = [one[m].compute_cubic(eq_s[m], c.claims[0]) for m in range(3)]
        want1 = [one[m].round(eq_s[m], c.rs[0], c.claims[1]) for m in range(3)]
        assert want0[0] == c.message(0)
        assert len({tuple(x) for x in want0}) == 3
        _pin(monkeypatch, grid)
        assert g.round(eq_g, None, c.claims[0]) == want0
        assert g.round(eq_g, c.rs[0], c.claims[1]) == want1
        assert eq_g.lens() == eq_s[0].lens()
        for m in range(3):
            assert np.array_equal(_raw(grp[m]), _raw(one[m])), m
    finally:
        g.free()
        for x in grp + one + eq_s + [eq_g]:
            x.free()
