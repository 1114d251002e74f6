"""GPU tests of cozk_rw_memory_leaves and cozk_rw_memory_init_final_leaves (csrc/rw_memory_leaves.hip): every leaf equal, byte for byte,
to the composition of cozk_fingerprint_leaves calls with an iota column (the calls of flow_harness.hpp's phase 4 with compact columns)
AND to the big-int values of tests/rw_proof_ref.py.  Lengths 1, 2, 63, 257, 4097 and one step past a workgroup of 256 (the kernel has
no grid stride: a workgroup covers 256 steps of one slot); MEM 32 and 4097; 1, 4 and 8 slots; U8 and U32 address columns mixed; v_written
NULL for all, some and no slots; a non-zero offset with guard entries on both sides; columns all 0xFFFFFFFF with gamma and tau in
{0, 1, r - 1} and a random pair; each refusal with its text and the context working afterwards."""
import importlib

import numpy as np
import pytest

import pyref as O
import rw_proof_ref as P

pytestmark = pytest.mark.gpu
R = O.R
INVALID_ARG = -1
GUARD = 0x5EED
TOP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def RP():
    return importlib.import_module("co-zkvms_amd.rw_proof")


def _u32(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint32), cozk.SCALAR_U32)


def _u8(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint8), cozk.SCALAR_U8)


def _guarded(cozk, ctx, n):
    return cozk.Vec.from_numpy(ctx, np.tile(cozk.fr_to_mont_limbs([GUARD])[0], (n, 1)))


def _columns(seed, ns, n, written, u8, top=False):
    """addr (below 256 where the slot's column is U8), v_read, t_read, v_written (None where `written[s]` is false)"""
    rng = np.random.default_rng(seed)
    col = lambda hi: ([min(TOP, hi - 1)] * n if top else rng.integers(0, hi, size=n, dtype=np.uint64).tolist())
    addr = [col(256 if u8[s] else 1 << 32) for s in range(ns)]
    return addr, [col(1 << 32) for _ in range(ns)], [col(1 << 32) for _ in range(ns)], [col(1 << 32) if written[s] else None for s in range(ns)]


def _check_rw(cozk, ctx, RP, cols, u8, g, tau, offset=0, tail=0):
    addr, v_read, t_read, v_written = cols
    ns, n = len(addr), len(addr[0])
    d_addr = [(_u8 if u8[s] else _u32)(cozk, ctx, addr[s]) for s in range(ns)]
    d_vr, d_tr = [_u32(cozk, ctx, c) for c in v_read], [_u32(cozk, ctx, c) for c in t_read]
    d_vw = [None if c is None else _u32(cozk, ctx, c) for c in v_written]
    total = 2 * ns * n
    fused, comp = _guarded(cozk, ctx, offset + total + tail), _guarded(cozk, ctx, offset + total + tail)
    RP.rw_memory_leaves(ctx, d_addr, d_vr, d_tr, None if all(c is None for c in d_vw) else d_vw, g, tau, fused, offset)
    iota = _u32(cozk, ctx, np.arange(n))
    g2 = g * g % R
    for s in range(ns):  # the calls of flow_harness.hpp:634-635
        w = d_vw[s] if d_vw[s] is not None else d_vr[s]
        cozk.fingerprint_leaves(ctx, [d_vr[s], d_tr[s], d_addr[s]], [g, g2, 1], [], [], -tau % R, "plain", 0, comp, offset=offset + 2 * s * n, n=n)
        cozk.fingerprint_leaves(ctx, [w, iota, d_addr[s]], [g, g2, 1], [], [], -tau % R, "plain", 0, comp, offset=offset + (2 * s + 1) * n, n=n)
    got = fused.to_numpy()
    assert got.tobytes() == comp.to_numpy().tobytes()
    guard = cozk.fr_to_mont_limbs([GUARD])[0]
    assert np.array_equal(got[:offset], np.tile(guard, (offset, 1))) and np.array_equal(got[offset + total:], np.tile(guard, (tail, 1)))
    want = [x for c in P.rw_leaves(addr, v_read, t_read, v_written, g, tau) for x in c]
    assert cozk.mont_limbs_to_int(got[offset:offset + total]) == want


def _check_if(cozk, ctx, RP, MEM, seed, g, tau, top=False, offset=0, tail=0):
    rng = np.random.default_rng(seed)
    col = lambda: [TOP] * MEM if top else rng.integers(0, 1 << 32, size=MEM, dtype=np.uint64).tolist()
    v_init, v_final, t_final = col(), col(), col()
    d = [_u32(cozk, ctx, c) for c in (v_init, v_final, t_final)]
    fused, comp = _guarded(cozk, ctx, offset + 2 * MEM + tail), _guarded(cozk, ctx, offset + 2 * MEM + tail)
    RP.rw_memory_init_final_leaves(ctx, *d, g, tau, fused, offset)
    iota = _u32(cozk, ctx, np.arange(MEM))
    cozk.fingerprint_leaves(ctx, [d[0], iota], [g, 1], [], [], -tau % R, "plain", 0, comp, offset=offset, n=MEM)  # flow_harness.hpp:637-638
    cozk.fingerprint_leaves(ctx, [d[1], d[2], iota], [g, g * g % R, 1], [], [], -tau % R, "plain", 0, comp, offset=offset + MEM, n=MEM)
    got = fused.to_numpy()
    assert got.tobytes() == comp.to_numpy().tobytes()
    guard = cozk.fr_to_mont_limbs([GUARD])[0]
    assert np.array_equal(got[:offset], np.tile(guard, (offset, 1))) and np.array_equal(got[offset + 2 * MEM:], np.tile(guard, (tail, 1)))
    want = [x for c in P.if_leaves(v_init, v_final, t_final, g, tau) for x in c]
    assert cozk.mont_limbs_to_int(got[offset:offset + 2 * MEM]) == want


def _written(ns, which):
    return {"all": [True] * ns, "none": [False] * ns, "some": [s % 2 == 1 for s in range(ns)]}[which]


@pytest.mark.parametrize("n", [1, 2, 63, 257, 4097])
@pytest.mark.parametrize("ns", [1, 4, 8])
def test_leaves_equal_the_composition_and_the_big_int_values(cozk, ctx, RP, n, ns):
    sm = O.SplitMix64(700 + n + ns)
    u8 = [s % 2 == 0 for s in range(ns)]  # U8 and U32 address columns mixed
    _check_rw(cozk, ctx, RP, _columns(701 + n, ns, n, _written(ns, "some"), u8), u8, sm.field(), sm.field())


@pytest.mark.parametrize("which", ["all", "none"])
def test_v_written_for_all_slots_and_for_none_past_a_workgroup_with_an_offset(cozk, ctx, RP, which):
    sm = O.SplitMix64(710)
    u8 = [False, True, True, False]
    _check_rw(cozk, ctx, RP, _columns(711, 4, 256 + 1, _written(4, which), u8), u8, sm.field(), sm.field(), offset=37, tail=5)


@pytest.mark.parametrize("g", [0, 1, R - 1, None], ids=["g_zero", "g_one", "g_minus_one", "g_random"])
@pytest.mark.parametrize("tau", [0, 1, R - 1, None], ids=["tau_zero", "tau_one", "tau_minus_one", "tau_random"])
def test_columns_all_ones_with_gamma_and_tau_at_their_edges(cozk, ctx, RP, g, tau):
    sm = O.SplitMix64(730)
    g = sm.field() if g is None else g
    tau = sm.field() if tau is None else tau
    u8 = [True, False, False]
    _check_rw(cozk, ctx, RP, _columns(731, 3, 70, [False, True, True], u8, top=True), u8, g, tau)
    _check_if(cozk, ctx, RP, 70, 732, g, tau, top=True)


@pytest.mark.parametrize("MEM", [32, 4097])
def test_init_final_leaves(cozk, ctx, RP, MEM):
    sm = O.SplitMix64(740 + MEM)
    _check_if(cozk, ctx, RP, MEM, 741 + MEM, sm.field(), sm.field(), offset=11, tail=3)


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_good_calls_after_them(cozk, ctx, RP):
    n, ns, MEM = 200, 4, 64
    u8 = [True, True, True, False]
    cols = _columns(750, ns, n, [False, False, True, True], u8)
    addr, v_read, t_read, v_written = cols
    d_addr = [(_u8 if u8[s] else _u32)(cozk, ctx, addr[s]) for s in range(ns)]
    d_vr, d_tr = [_u32(cozk, ctx, c) for c in v_read], [_u32(cozk, ctx, c) for c in t_read]
    d_vw = [None if c is None else _u32(cozk, ctx, c) for c in v_written]
    out = cozk.Vec.alloc(ctx, 2 * ns * n)
    short = _u32(cozk, ctx, v_read[0][:-1])
    u16 = cozk.Vec.from_numpy(ctx, np.zeros(n, dtype=np.uint16), cozk.SCALAR_U16)
    u8v = _u8(cozk, ctx, [0] * n)
    call = lambda a=d_addr, vr=d_vr, tr=d_tr, vw=d_vw, o=out, off=0: RP.rw_memory_leaves(ctx, a, vr, tr, vw, 5, 7, o, off)
    _refused(cozk, "rw_memory_leaves: addr[s] is a U8 or U32 vector", lambda: call(a=d_addr[:3] + [u16]))
    _refused(cozk, "rw_memory_leaves: v_read[s], t_read[s] and v_written[s] are U32 vectors", lambda: call(vr=d_vr[:3] + [u8v]))
    _refused(cozk, "rw_memory_leaves: v_read[s], t_read[s] and v_written[s] are U32 vectors", lambda: call(vw=d_vw[:3] + [u8v]))
    _refused(cozk, "rw_memory_leaves: every column has n entries", lambda: call(tr=d_tr[:3] + [short]))
    over = cozk.rw_memory.RW_MEMORY_MAX_SLOTS + 1
    _refused(cozk, "rw_memory_leaves: 1 <= n_slots <= %d" % cozk.rw_memory.RW_MEMORY_MAX_SLOTS, lambda: call(a=d_addr[:1] * over, vr=d_vr[:1] * over, tr=d_tr[:1] * over, vw=None))
    _refused(cozk, "rw_memory_leaves: out is an FR vector with room for 2 n_slots n entries from offset", lambda: call(off=1))
    _refused(cozk, "rw_memory_leaves: out is an FR vector with room for 2 n_slots n entries from offset", lambda: call(o=d_vr[0]))
    d3 = [_u32(cozk, ctx, [1] * MEM) for _ in range(3)]
    out2 = cozk.Vec.alloc(ctx, 2 * MEM)
    _refused(cozk, "rw_memory_init_final_leaves: v_init, v_final and t_final are U32 vectors", lambda: RP.rw_memory_init_final_leaves(ctx, d3[0], _u8(cozk, ctx, [0] * MEM), d3[2], 5, 7, out2))
    _refused(cozk, "rw_memory_init_final_leaves: every column has MEM entries", lambda: RP.rw_memory_init_final_leaves(ctx, d3[0], d3[1], _u32(cozk, ctx, [1] * (MEM - 1)), 5, 7, out2))
    _refused(cozk, "rw_memory_init_final_leaves: out is an FR vector with room for 2 MEM entries from offset", lambda: RP.rw_memory_init_final_leaves(ctx, *d3, 5, 7, out2, 1))
    _refused(cozk, "rw_memory_init_final_leaves: out is an FR vector with room for 2 MEM entries from offset", lambda: RP.rw_memory_init_final_leaves(ctx, *d3, 5, 7, d3[0]))
    _check_rw(cozk, ctx, RP, cols, u8, 5, 7)  # the context works on after a refusal
    _check_if(cozk, ctx, RP, MEM, 751, 5, 7)
