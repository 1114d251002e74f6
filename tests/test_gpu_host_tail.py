"""GPU tier: the host tail of cozk_layer_prove_rounds (the last rounds of a layer on the host, csrc/host/layer_tail.hpp) against the
same call with the tail switched off (COZK_HOST_TAIL_MAX=0, read on every call), and the resident kernel's watchdog with and without
the tail."""
import time

import pytest

import pyref as O

pytestmark = pytest.mark.gpu


def _shares(rng, n, mode):
    if mode == "rep3":
        return [(rng.field(), rng.field()) for _ in range(n)]
    return [rng.field() for _ in range(n)]


def _inputs(length, mode, seed):
    rng = O.SplitMix64(seed)
    coeffs = _shares(rng, length, mode)
    nv = max(0, ((length + 1) // 2 - 1).bit_length())
    return dict(coeffs=coeffs, nv=nv, w=[rng.field() for _ in range(nv)], claim0=rng.field(), rs=[rng.field() for _ in range(nv)],
                claims=[rng.field() for _ in range(nv)])


def _prove(cozk, ctx, inp, resident, stall=None):
    """one prove_rounds call -> everything the call and the ABI let a caller see afterwards"""
    layer = cozk.Rep3DenseInterleavedPolynomial.new(ctx, inp["coeffs"])
    eq = cozk.SplitEqPolynomial(ctx, inp["w"])
    seen = []

    def exchange(rnd, cf):
        seen.append(cf)
        if rnd == stall:
            time.sleep(1.6)
        return inp["rs"][rnd], inp["claims"][rnd]

    ctx.set_resident_rounds(resident)
    try:
        got_r, finals = layer.prove_rounds(eq, inp["claim0"], inp["nv"], exchange)
    finally:
        ctx.set_resident_rounds(None)
    return dict(seen=seen, r=got_r, finals=finals, coeffs=layer.coeffs(), lens=eq.lens(), eq=eq.download())


def _separate(cozk, ctx, inp):
    """the same rounds as compute_cubic / bind / final_claims called one by one"""
    sep = cozk.Rep3DenseInterleavedPolynomial.new(ctx, inp["coeffs"])
    eq = cozk.SplitEqPolynomial(ctx, inp["w"])
    seen, c = [], inp["claim0"]
    for j in range(inp["nv"]):
        seen.append(sep.compute_cubic(eq, c))
        sep.bind(inp["rs"][j])
        eq.bind(inp["rs"][j])
        c = inp["claims"][j]
    return dict(seen=seen, r=inp["rs"], finals=sep.final_claims(), coeffs=sep.coeffs(), lens=eq.lens(), eq=eq.download())


# 6: entirely on the host.  130: with the threshold at 128 the resident kernel hands over after one round, with per-round launches
# the host takes 130 -> 66 pending.  2048: the longest layer the resident kernel takes and the cap of the threshold.  4104 (ragged:
# 4104 -> 2052 -> 1026): launched rounds, then the resident kernel, then the host.
@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
@pytest.mark.parametrize("length", [6, 130, 2048, 4104])
def test_host_tail_equals_device_tail(cozk, ctx, monkeypatch, length, mode, resident):
    inp = _inputs(length, mode, length * 11 + (mode == "plain"))
    monkeypatch.setenv("COZK_HOST_TAIL_MAX", "0")
    want = _prove(cozk, ctx, inp, resident)
    assert want["r"] == inp["rs"] and len(want["seen"]) == inp["nv"] and len(want["coeffs"]) == 2
    for tail_max in (8, 128, 2048):
        monkeypatch.setenv("COZK_HOST_TAIL_MAX", str(tail_max))
        got = _prove(cozk, ctx, inp, resident)
        for key in ("seen", "r", "finals", "coeffs", "lens", "eq"):
            assert got[key] == want[key], "COZK_HOST_TAIL_MAX=%d: %s differs from the run without a host tail" % (tail_max, key)


def test_resident_watchdog_without_host_tail(cozk, ctx, monkeypatch):
    """the stall in the middle of the resident tail and in its last round, as in test_gpu_poly's watchdog test, with the host tail
    off: every remaining round stays on the device, so the mid-tail stall of the resident kernel stays covered"""
    monkeypatch.setenv("COZK_RESIDENT_TIMEOUT_S", "1")
    monkeypatch.setenv("COZK_HOST_TAIL_MAX", "0")
    inp = _inputs(512, "rep3", 4242)
    want = _separate(cozk, ctx, inp)
    for stall in (3, inp["nv"] - 1):
        got = _prove(cozk, ctx, inp, True, stall=stall)
        for key in ("seen", "r", "finals", "coeffs", "lens"):
            assert got[key] == want[key], "stall in round %d: %s" % (stall, key)


def test_resident_watchdog_then_launched_hand_over(cozk, ctx, monkeypatch):
    """default thresholds, 2048 elements, the callback of resident round 1 outlasts the watchdog: the kernel leaves, the call goes on
    with one launch per round from the state it left, and hands the layer to the host at the threshold of launched rounds"""
    monkeypatch.setenv("COZK_RESIDENT_TIMEOUT_S", "1")
    monkeypatch.delenv("COZK_HOST_TAIL_MAX", raising=False)
    inp = _inputs(2048, "rep3", 777)
    want = _separate(cozk, ctx, inp)
    got = _prove(cozk, ctx, inp, True, stall=1)
    for key in ("seen", "r", "finals", "coeffs", "lens", "eq"):
        assert got[key] == want[key], key
