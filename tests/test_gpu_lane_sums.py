"""The lazy 9 x 29 round sums at thousands of terms per lane.  The round-sum kernels (k_layer_cubic9, k_layer_bind_cubic9,
k_toggle_cubic9, k_outer_round_act9) add every term of a lane into unreduced accumulators that are folded once per FR9_FOLD_PERIOD
terms (csrc/fr9.hip.hpp); at the default grids a lane sees a few hundred terms at most.  COZK_SUM_GRID_MAX=1 runs those launches on
ONE workgroup (256 lanes), so each lane adds len / 4 / 256 chunk terms, and every result must equal the default grid's bit for bit.

Variant -> terms per lane at the pinned grid (plain layers group the E1 pairs (NESTED = 2) while E1 has >= 512 pairs, Rep3 never does):
  * Rep3 layer 2^22: compute_cubic NESTED = 1, 4096; fused bind + sums NESTED = 1, 2048;
  * plain layer 2^25: rounds 0-2 NESTED = 2, 32768 / 16384 / 8192 chunk terms into the group sums and 4096 flushes into each sum;
    round 3 (E1 down to 256 pairs) NESTED = 1, 4096 (the plain sums carry lambda^3 and end with the smaller K3, so fewer terms
    would not break the unfolded kernels);
  * toggle layer 2^20 pairs: round 0 (u8 flags) 4096 heavy terms at 100 % density (~1024 at 25 %), rounds 1, 2 (bound flags)
    2048 and 1024;
  * whole proofs: OuterHarness(log_steps=18) (>= 2^20 pairs in round 0), LookupsHarness(log_n=14, n_pairs=54, 100 %), a GP proof
    of 2^21 leaves, and the committed golden pipelines."""
import importlib
import json
import os

import numpy as np
import pytest

import pyref as O
import pysparse as S

pytestmark = pytest.mark.gpu
GRID = "COZK_SUM_GRID_MAX"


def _lib():
    return importlib.import_module("co-zkvms_amd._lib")


def _raw(layer):
    """the layer's storage as raw Montgomery limbs (no host conversion)"""
    n = len(layer)
    a = np.empty((n, 4), dtype=np.uint64)
    b = np.empty((n, 4), dtype=np.uint64)
    layer.ctx.check(layer.ctx._l.cozk_layer_download(layer.ctx.h, layer.h, a.ctypes.data, b.ctypes.data))
    return a if layer.mode == _lib().MODE_PLAIN else np.concatenate([a, b])


def _pinned(monkeypatch, fn):
    monkeypatch.setenv(GRID, "1")
    try:
        return fn()
    finally:
        monkeypatch.delenv(GRID)


def _layer(cozk, ctx, log_len, mode, seed):
    a = cozk.Vec.random(ctx, 1 << log_len, seed)
    b = cozk.Vec.random(ctx, 1 << log_len, seed + 1) if mode == "rep3" else None
    return cozk.Rep3DenseInterleavedPolynomial.from_vecs(ctx, a, b, take_ownership=True)


@pytest.mark.parametrize("mode,log_len,rounds", [("rep3", 22, 2), ("plain", 25, 4)])
def test_layer_rounds_at_one_workgroup_equal_the_default_grid(cozk, ctx, monkeypatch, mode, log_len, rounds):
    monkeypatch.delenv(GRID, raising=False)
    rng = O.SplitMix64(log_len)
    w = [rng.field() for _ in range(log_len - 1)]
    rs = [rng.field() for _ in range(rounds)]
    claim = rng.field()
    ref, pin = _layer(cozk, ctx, log_len, mode, 900), _layer(cozk, ctx, log_len, mode, 900)
    eq_ref, eq_pin = cozk.SplitEqPolynomial(ctx, w), cozk.SplitEqPolynomial(ctx, w)
    # compute_cubic alone (layer_cubic_sums) on the unbound layer
    want = ref.compute_cubic(eq_ref, claim)
    assert _pinned(monkeypatch, lambda: pin.compute_cubic(eq_pin, claim)) == want
    for j in range(rounds):  # the fused round: bind (k_layer_bind_cubic9 from round 1 on) + sums
        r = rs[j - 1] if j else None
        want = ref.round(eq_ref, r, claim)
        got = _pinned(monkeypatch, lambda: pin.round(eq_pin, r, claim))
        assert got == want, (mode, j)
        if j:  # the bound layer
            assert np.array_equal(_raw(pin), _raw(ref)), (mode, j)
        claim = O.unipoly_eval(want, rs[j]) if j + 1 < rounds else claim
    for x in (ref, pin, eq_ref, eq_pin):
        x.free()


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_layer_rounds_at_one_workgroup_equal_the_oracle(cozk, ctx, monkeypatch, mode):
    """2^18 elements (256 chunk terms per lane at the pinned grid): round 0 and 1 against O.interleaved_compute_cubic"""
    log_len = 18
    rng = O.SplitMix64(77)
    w = [rng.field() for _ in range(log_len - 1)]
    r0, claim = rng.field(), rng.field()
    lay = _layer(cozk, ctx, log_len, mode, 31)
    coeffs = lay.coeffs()
    eq_dev, eq = cozk.SplitEqPolynomial(ctx, w), O.SplitEq(w)
    got = _pinned(monkeypatch, lambda: lay.round(eq_dev, None, claim))
    assert got == O.interleaved_compute_cubic(coeffs, eq, claim)
    claim = O.unipoly_eval(got, r0)
    got = _pinned(monkeypatch, lambda: lay.round(eq_dev, r0, claim))
    coeffs = O.interleaved_bind(coeffs, r0)
    eq.bind(r0)
    assert got == O.interleaved_compute_cubic(coeffs, eq, claim)
    assert lay.coeffs() == coeffs
    lay.free()
    eq_dev.free()


def _toggle(cozk, ctx, mode, npairs_cols, n, density, seed):
    L = _lib()
    LK = importlib.import_module("co-zkvms_amd.lookups")
    rnd = np.random.default_rng(seed)
    flags = [cozk.Vec.from_numpy(ctx, (rnd.integers(0, 100, n) < density).astype(np.uint8), kind=L.SCALAR_U8)
             for _ in range(npairs_cols)]
    fa = cozk.Vec.random(ctx, 2 * npairs_cols * n, seed)
    fb = cozk.Vec.random(ctx, 2 * npairs_cols * n, seed + 1) if mode == "rep3" else None
    return LK.ToggleLayer.from_vecs(ctx, flags, fa, fb)


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("density", [100, 25])
def test_toggle_rounds_at_one_workgroup_equal_the_default_grid(cozk, ctx, monkeypatch, mode, density):
    monkeypatch.delenv(GRID, raising=False)
    n = 1 << 19  # 2 pair columns x 2^19 = 2^20 pairs in round 0
    nv = (4 * n).bit_length() - 1
    rng = O.SplitMix64(density)
    w = [rng.field() for _ in range(nv)]
    rs = [rng.field() for _ in range(3)]
    ref, pin = _toggle(cozk, ctx, mode, 2, n, density, 5), _toggle(cozk, ctx, mode, 2, n, density, 5)
    eq_ref, eq_pin = cozk.SplitEqPolynomial(ctx, w), cozk.SplitEqPolynomial(ctx, w)
    for j in range(3):
        r = rs[j - 1] if j else None
        want = ref.round(eq_ref, r, party=1)
        assert _pinned(monkeypatch, lambda: pin.round(eq_pin, r, party=1)) == want, (mode, density, j)
    for x in (ref, pin, eq_ref, eq_pin):
        x.free()


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_toggle_rounds_at_one_workgroup_equal_the_sparse_oracle(cozk, ctx, monkeypatch, mode):
    """2^13 pairs (the smallest nested layer of k_toggle_cubic9) at one workgroup: rounds 0-2 against oracle/pysparse.py"""
    LK = importlib.import_module("co-zkvms_amd.lookups")
    n, batch, density = 1 << 12, 4, 60
    rng = O.SplitMix64(404)
    cols = [[1 if rng.next() % 100 < density else 0 for _ in range(n)] for _ in range(batch // 2)]
    vals = [[rng.field() for _ in range(n)] for _ in range(batch)]
    if mode == "plain":
        fps, party, nparties = vals, 0, 1
    else:
        sh = [[O.rep3_share(v, rng) for v in row] for row in vals]
        fps, party, nparties = [[s[1] for s in row] for row in sh], 1, 3
    ref = S.ToggleLayer([[i for i, f in enumerate(c) if f] for c in cols], fps, party, nparties)
    dev = LK.ToggleLayer(ctx, cols, fps)
    nv = (batch * n).bit_length() - 1
    w = [rng.field() for _ in range(nv)]
    rs = [rng.field() for _ in range(3)]
    eq_ref, eq_dev = O.SplitEq(w), cozk.SplitEqPolynomial(ctx, w)
    claim = rng.field()
    for j in range(3):
        ev = ref.compute_cubic_evals(eq_ref, claim)
        got = _pinned(monkeypatch, lambda: dev.round(eq_dev, rs[j - 1] if j else None, party=party))
        assert got == [ev[0], ev[2], ev[3]], (mode, j)
        ref.bind(rs[j])
        eq_ref.bind(rs[j])
    dev.free()
    eq_dev.free()


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_toggle_montgomery_rounds_at_one_workgroup_equal_the_sparse_oracle(cozk, ctx, monkeypatch, mode):
    """2^10 pairs (below TOGGLE_F9_MIN_PAIRS: k_toggle_cubic, the Montgomery kernel) at one workgroup, 60 % flags: every wave looks
    four times in round 0 and carries what is left of its queue (64 < queue < 128) from one look to the next.  All 11 rounds -- u8 and
    bound flags, nested and flat eq tables, the coalesced rounds -- against oracle/pysparse.py"""
    LK = importlib.import_module("co-zkvms_amd.lookups")
    n, batch, density = 1 << 9, 4, 60
    rng = O.SplitMix64(405)
    cols = [[1 if rng.next() % 100 < density else 0 for _ in range(n)] for _ in range(batch // 2)]
    vals = [[rng.field() for _ in range(n)] for _ in range(batch)]
    if mode == "plain":
        fps, party, nparties = vals, 0, 1
    else:
        sh = [[O.rep3_share(v, rng) for v in row] for row in vals]
        fps, party, nparties = [[s[1] for s in row] for row in sh], 1, 3
    ref = S.ToggleLayer([[i for i, f in enumerate(c) if f] for c in cols], fps, party, nparties)
    dev = LK.ToggleLayer(ctx, cols, fps)
    nv = (batch * n).bit_length() - 1
    assert nv == 11
    w = [rng.field() for _ in range(nv)]
    rs = [rng.field() for _ in range(nv)]
    eq_ref, eq_dev = O.SplitEq(w), cozk.SplitEqPolynomial(ctx, w)
    claim = rng.field()
    for j in range(nv):
        ev = ref.compute_cubic_evals(eq_ref, claim)
        got = _pinned(monkeypatch, lambda: dev.round(eq_dev, rs[j - 1] if j else None, party=party))
        assert got == [ev[0], ev[2], ev[3]], (mode, j)
        ref.bind(rs[j])
        eq_ref.bind(rs[j])
    dev.free()
    eq_dev.free()


def _digests(monkeypatch, make, pinned):
    if pinned:
        monkeypatch.setenv(GRID, "1")
    else:
        monkeypatch.delenv(GRID, raising=False)
    try:
        h = make()
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        d = (bytes(r.proof_digest), r.proof_len)
        h.close()
        return d
    finally:
        monkeypatch.delenv(GRID, raising=False)


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_outer_proof_at_one_workgroup(cozk, monkeypatch, mode):
    OU = importlib.import_module("co-zkvms_amd.outer")
    make = lambda: OU.OuterHarness(mode=mode, log_steps=18, seed=3)
    assert _digests(monkeypatch, make, True) == _digests(monkeypatch, make, False)


def test_lookups_proof_at_one_workgroup(cozk, monkeypatch):
    LK = importlib.import_module("co-zkvms_amd.lookups")
    make = lambda: LK.LookupsHarness(mode="plain", log_n=14, n_pairs=54, density_pct=100, seed=9)
    assert _digests(monkeypatch, make, True) == _digests(monkeypatch, make, False)


def test_gp_proof_of_2_21_leaves_at_one_workgroup(cozk, monkeypatch):
    make = lambda: cozk.Harness(mode="plain", log_n=12, n_fr=2, n_u16=1, n_u32=1, n_flags=1, n_small=0, gp_batch=2,
                                gp_log_leaves=20, seed=21)
    assert _digests(monkeypatch, make, True) == _digests(monkeypatch, make, False)


def test_golden_pipelines_at_one_workgroup(cozk, monkeypatch):
    """tests/golden/round2_pipelines.json reproduced with every round-sum launch on one workgroup"""
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "round2_pipelines.json")))
    LK = importlib.import_module("co-zkvms_amd.lookups")
    OU = importlib.import_module("co-zkvms_amd.outer")
    monkeypatch.setenv(GRID, "1")
    for row in G["lookups"]:
        cfg = dict(row["cfg"])
        h = LK.LookupsHarness(mode=cfg.pop("mode"), primary=bool(cfg.pop("primary", 0)), **cfg)
        r = h.prove(verify=True)
        assert r.verified == 1 and bytes(r.proof_digest).hex() == row["digest"] and r.proof_len == row["proof_len"], row["cfg"]
        h.close()
    for row in G["spartan"]:
        cfg = dict(row["cfg"])
        for mode in ("plain", "rep3"):
            h = cozk.SpartanHarness(mode=mode, log_n=cfg["log_n"], seed=cfg["seed"], lookup_round=bool(cfg.get("lookup_round", 0)))
            r = h.prove(verify=True)
            assert r.verified == 1 and bytes(r.proof_digest).hex() == row["digest"], (row["cfg"], mode)
            h.close()
    for row in G["outer"]:
        cfg = dict(row["cfg"])
        h = OU.OuterHarness(mode=cfg["mode"], log_steps=cfg["log_steps"], seed=cfg["seed"])
        r = h.prove(verify=True)
        assert r.verified == 1 and bytes(r.proof_digest).hex() == row["digest"], row["cfg"]
        h.close()
