"""GPU tests of cozk_timestamp_range_leaves (csrc/ts_range_witness.hip): every leaf equal, byte for byte, to the composition of
cozk_fingerprint_leaves calls it replaces, and to tests/ts_proof_ref.py.  Lengths around a wave, a workgroup and a witness tile;
1, 4 and 8 slots; t_read all zero and t_read[j] = j; t_read made on the device by cozk_rw_memory_witness; a non-zero offset with
guard entries on both sides; gamma 0, 1, r - 1 and random; the refusals."""
import importlib

import numpy as np
import pytest

import pyref as O
import rw_witness_ref as W
import ts_proof_ref as P
import ts_range_ref as TR

pytestmark = pytest.mark.gpu
R = O.R
INVALID_ARG = -1
GUARD = 0x5EED


@pytest.fixture(scope="module")
def TP():
    return importlib.import_module("co-zkvms_amd.ts_proof")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("co-zkvms_amd.lasso").LASSO_TILE


def _u32(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint32), cozk.SCALAR_U32)


def _composition(cozk, ctx, d, ns, n, g, tau, out, offset):
    """the 6 ns + 1 circuits from cozk_fingerprint_leaves, one call per circuit, with a materialised iota column"""
    t_read, rc_rt, rc_gmr, fc_rt, fc_gmr = d
    g1, g2 = (1 + g) % R, g * g % R
    iota = _u32(cozk, ctx, np.arange(n))
    leaf = lambda c, cols, coeffs, const: cozk.fingerprint_leaves(ctx, cols, coeffs, [], [], const % R, "plain", 0, out, offset=offset + c * n, n=n)
    for s in range(ns):
        leaf(4 * s, [t_read[s], rc_rt[s]], [g1, g2], -tau)
        leaf(4 * s + 1, [t_read[s], rc_rt[s]], [g1, g2], g2 - tau)
        leaf(4 * s + 2, [iota, t_read[s], rc_gmr[s]], [g1, (-g1) % R, g2], -tau)
        leaf(4 * s + 3, [iota, t_read[s], rc_gmr[s]], [g1, (-g1) % R, g2], g2 - tau)
        leaf(4 * ns + 1 + 2 * s, [iota, fc_rt[s]], [g1, g2], -tau)
        leaf(4 * ns + 2 + 2 * s, [iota, fc_gmr[s]], [g1, g2], -tau)
    leaf(4 * ns, [iota], [g1], -tau)


def _check(cozk, ctx, TP, t_read, g, tau, d_t_read=None, ref=True, offset=0, tail=0):
    ns, n = len(t_read), len(t_read[0])
    fams = TR.ts_range(t_read, n)
    d = [d_t_read or [_u32(cozk, ctx, c) for c in t_read]] + [[_u32(cozk, ctx, c) for c in fam] for fam in fams]
    total = (6 * ns + 1) * n
    guard = cozk.fr_to_mont_limbs([GUARD])[0]
    fused = cozk.Vec.from_numpy(ctx, np.tile(guard, (offset + total + tail, 1)))
    comp = cozk.Vec.from_numpy(ctx, np.tile(guard, (offset + total + tail, 1)))
    TP.timestamp_range_leaves(ctx, *d, g, tau, fused, offset)
    _composition(cozk, ctx, d, ns, n, g, tau, comp, offset)
    got = fused.to_numpy()
    assert got.tobytes() == comp.to_numpy().tobytes()
    assert np.array_equal(got[:offset], np.tile(guard, (offset, 1))) and np.array_equal(got[offset + total:], np.tile(guard, (tail, 1)))
    if ref:
        want = [x for c in P.range_leaves(t_read, *fams, g, tau) for x in c]
        assert cozk.mont_limbs_to_int(got[offset:offset + total]) == want
    return fams


def _t_read(seed, ns, n):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 1 << 62, size=n) % (np.arange(n) + 1)).tolist() for _ in range(ns)]


@pytest.mark.parametrize("n", [1, 64, 65, 257, 4097])
@pytest.mark.parametrize("ns", [1, 4, 8])
def test_leaves_equal_the_composition_and_the_reference(cozk, ctx, TP, n, ns):
    sm = O.SplitMix64(600 + n + ns)
    _check(cozk, ctx, TP, _t_read(601 + n, ns, n), sm.field(), sm.field(), ref=n <= 257 or ns == 1)


def test_one_step_past_a_witness_tile_with_an_offset_and_guards(cozk, ctx, TP, T):
    sm = O.SplitMix64(610)
    _check(cozk, ctx, TP, _t_read(611, 2, T + 1), sm.field(), sm.field(), ref=False, offset=37, tail=5)


@pytest.mark.parametrize("g", [0, 1, R - 1, None], ids=["zero", "one", "minus_one", "random"])
def test_gamma_at_its_edges_and_t_read_at_its_extremes(cozk, ctx, TP, g):
    n = 300
    sm = O.SplitMix64(620)
    tau = sm.field()
    g = sm.field() if g is None else g
    _check(cozk, ctx, TP, [[0] * n, list(range(n)), _t_read(621, 1, n)[0]], g, tau, offset=3, tail=2)


def test_t_read_made_on_the_device(cozk, ctx, TP):
    n, MEM = 300, 500
    rng = np.random.default_rng(630)
    u32 = lambda k: rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32).tolist()
    addr = [rng.integers(0, 32, size=n).tolist() for _ in range(3)] + [rng.integers(0, MEM, size=n).tolist()]
    vw, iw, vi = [None, None, u32(n), u32(n)], [None, None, None, (rng.integers(0, 100, size=n) < 30).astype(np.uint8).tolist()], u32(MEM)
    up = lambda cols, dt, kind: [None if c is None else cozk.Vec.from_numpy(ctx, np.asarray(c, dtype=dt), kind) for c in cols]
    out = cozk.rw_memory_witness(ctx, up(addr, np.uint32, cozk.SCALAR_U32), up(vw, np.uint32, cozk.SCALAR_U32), up(iw, np.uint8, cozk.SCALAR_U8), _u32(cozk, ctx, vi))
    t_read = W.replay(addr, vw, iw, vi)[1]
    sm = O.SplitMix64(631)
    g, tau = sm.field(), sm.field()
    fams = _check(cozk, ctx, TP, t_read, g, tau, d_t_read=out[1])
    assert P.multiset_holds(P.multiset_hashes(P.range_leaves(t_read, *fams, g, tau)), 4)


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_a_good_call_after_them(cozk, ctx, TP):
    n, ns = 200, 4
    t_read = [[j * 3 // 4 for j in range(n)] for _ in range(ns)]
    fams = TR.ts_range(t_read, n)
    up = lambda fam: [_u32(cozk, ctx, c) for c in fam]
    d = [up(t_read)] + [up(f) for f in fams]
    out = cozk.Vec.alloc(ctx, (6 * ns + 1) * n)
    late = [list(c) for c in t_read]
    late[3][90] = 91  # t_read[s][j] = j + 1 ...
    late[1][90] = 91  # ... the smallest (step, slot) is named
    late[0][120] = 1 << 31
    _refused(cozk, "timestamp_range_leaves: step 90, slot 1: t_read is greater than the step", lambda: TP.timestamp_range_leaves(ctx, up(late), *d[1:], 5, 7, out))
    u8 = cozk.Vec.from_numpy(ctx, np.zeros(n, dtype=np.uint8), cozk.SCALAR_U8)
    _refused(cozk, "every column is a U32 vector", lambda: TP.timestamp_range_leaves(ctx, d[0], d[1], d[2][:3] + [u8], d[3], d[4], 5, 7, out))
    _refused(cozk, "every column has n entries", lambda: TP.timestamp_range_leaves(ctx, d[0], d[1], d[2], d[3][:3] + [_u32(cozk, ctx, fams[2][3][:-1])], d[4], 5, 7, out))
    _refused(cozk, "1 <= n_slots <= 8", lambda: TP.timestamp_range_leaves(ctx, *[f[:1] * 9 for f in d], 5, 7, out))
    _refused(cozk, "room for (6 n_slots + 1) n entries from offset", lambda: TP.timestamp_range_leaves(ctx, *d, 5, 7, out, 1))
    _refused(cozk, "room for (6 n_slots + 1) n entries from offset", lambda: TP.timestamp_range_leaves(ctx, *d, 5, 7, d[1][0]))
    _check(cozk, ctx, TP, t_read, 5, 7)  # the context works on after a refusal
