"""GPU tests of cozk_rw_memory_shared_leaves and cozk_rw_memory_shared_init_final_leaves (csrc/rw_memory_leaves.hip): every leaf equal,
byte for byte, to the composition of cozk_fingerprint_leaves calls with an iota column in the same mode for the same party (the ten
launches of rw_memory_leaves_composed with polynomial terms) AND to the big-int values of tests/rw_shared_ref.py.  PLAIN, and REP3 for
parties 0, 1 and 2; lengths 1, 2, 63, 257, 4097 (the kernels have no grid stride: a workgroup covers 256 steps of one slot); 1, 4 and 8
slots with U8 and U32 address columns mixed; MEM 32 and 4097; v_written NULL for all, some and no slots; a REP3 call whose v_init is a
public polynomial and one where every value is; polynomials longer than n; a non-zero offset with guard entries on both sides of out_a
and out_b; share components in {0, r - 1} with columns all 0xFFFFFFFF and gamma, tau in {0, 1, r - 1} and a random pair; each refusal
with its text and the context working afterwards."""
import importlib

import numpy as np
import pytest

import pyref as O
import rw_shared_ref as S

pytestmark = pytest.mark.gpu
R = O.R
INVALID_ARG = -1
GUARD = 0x5EED
TOP = 0xFFFFFFFF
MODES = [("plain", 0), ("rep3", 0), ("rep3", 1), ("rep3", 2)]
MODE_IDS = ["plain", "rep3_p0", "rep3_p1", "rep3_p2"]


@pytest.fixture(scope="module")
def R3():
    return importlib.import_module("co-zkvms_amd.rw_proof_rep3")


def _u32(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint32), cozk.SCALAR_U32)


def _u8(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint8), cozk.SCALAR_U8)


def _guarded(cozk, ctx, n):
    return cozk.Vec.from_numpy(ctx, np.tile(cozk.fr_to_mont_limbs([GUARD])[0], (n, 1)))


def _public(seed, n, top=False):
    rng = np.random.default_rng(seed)
    return [TOP] * n if top else rng.integers(0, 1 << 32, size=n, dtype=np.uint64).tolist()


def _field(seed, n):
    sm = O.SplitMix64(seed)
    return [sm.field() for _ in range(n)]


def _value(seed, n, shared):
    """a value column of n entries: field elements (a PLAIN polynomial) or pairs of them (Rep3 share components)"""
    return list(zip(_field(seed, n), _field(seed + 1, n))) if shared else _field(seed, n)


EDGE = [(0, R - 1), (R - 1, 0), (R - 1, R - 1), (0, 0)]


def _edge_value(n, shared):
    return [EDGE[j % 4] for j in range(n)] if shared else [(0, R - 1)[j % 2] for j in range(n)]


def _columns(seed, ns, n, u8, top=False):
    """addr (below 256 where the slot's column is U8) and t_read per slot; top: every entry the largest its kind holds"""
    addr = [[a % 256 for a in _public(seed + s, n, top)] if u8[s] else _public(seed + s, n, top) for s in range(ns)]
    return addr, [_public(seed + 50 + s, n, top) for s in range(ns)]


def _outs(cozk, ctx, size, rep3):
    return [_guarded(cozk, ctx, size) for _ in range(2 if rep3 else 1)]


def _compare(cozk, fused, comp, want, offset, total, tail):
    guard = cozk.fr_to_mont_limbs([GUARD])[0]
    for x, y, w in zip(fused, comp, want):
        got = x.to_numpy()
        assert got.tobytes() == y.to_numpy().tobytes()
        assert np.array_equal(got[:offset], np.tile(guard, (offset, 1))) and np.array_equal(got[offset + total:], np.tile(guard, (tail, 1)))
        assert cozk.mont_limbs_to_int(got[offset:offset + total]) == w


def _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, g, tau, mode, party, offset=0, tail=0):
    """v_read[s], v_written[s] (None: the slot only reads): value columns of at least n entries, as rw_shared_ref takes them"""
    ns, n = len(addr), len(addr[0])
    d_addr = [(_u8 if u8[s] else _u32)(cozk, ctx, addr[s]) for s in range(ns)]
    d_tr = [_u32(cozk, ctx, c) for c in t_read]
    p_vr = [cozk.Rep3DensePolynomial.new(ctx, c) for c in v_read]
    p_vw = [None if c is None else cozk.Rep3DensePolynomial.new(ctx, c) for c in v_written]
    rep3 = mode == "rep3"
    total = 2 * ns * n
    fused, comp = _outs(cozk, ctx, offset + total + tail, rep3), _outs(cozk, ctx, offset + total + tail, rep3)
    R3.rw_memory_shared_leaves(ctx, d_addr, p_vr, d_tr, None if all(p is None for p in p_vw) else p_vw, g, tau, mode, party, *fused, offset=offset)
    iota = _u32(cozk, ctx, np.arange(n))
    g2 = g * g % R
    for s in range(ns):  # rw_memory_leaves_composed: the value a polynomial term, the address and the times compact columns
        w = p_vw[s] if p_vw[s] is not None else p_vr[s]
        cozk.fingerprint_leaves(ctx, [d_tr[s], d_addr[s]], [g2, 1], [p_vr[s]], [g], -tau % R, mode, party, *comp, offset=offset + 2 * s * n, n=n)
        cozk.fingerprint_leaves(ctx, [iota, d_addr[s]], [g2, 1], [w], [g], -tau % R, mode, party, *comp, offset=offset + (2 * s + 1) * n, n=n)
    want = S.rw_shared_leaves(addr, v_read, t_read, v_written, g, tau, mode, party)
    _compare(cozk, fused, comp, want, offset, total, tail)


def _check_if(cozk, ctx, R3, v_init, v_final, t_final, g, tau, mode, party, offset=0, tail=0):
    MEM = len(t_final)
    d_tf = _u32(cozk, ctx, t_final)
    p_vi, p_vf = cozk.Rep3DensePolynomial.new(ctx, v_init), cozk.Rep3DensePolynomial.new(ctx, v_final)
    rep3 = mode == "rep3"
    fused, comp = _outs(cozk, ctx, offset + 2 * MEM + tail, rep3), _outs(cozk, ctx, offset + 2 * MEM + tail, rep3)
    R3.rw_memory_shared_init_final_leaves(ctx, p_vi, p_vf, d_tf, g, tau, mode, party, *fused, offset=offset)
    iota = _u32(cozk, ctx, np.arange(MEM))
    cozk.fingerprint_leaves(ctx, [iota], [1], [p_vi], [g], -tau % R, mode, party, *comp, offset=offset, n=MEM)
    cozk.fingerprint_leaves(ctx, [d_tf, iota], [g * g % R, 1], [p_vf], [g], -tau % R, mode, party, *comp, offset=offset + MEM, n=MEM)
    want = S.if_shared_leaves(v_init, v_final, t_final, g, tau, mode, party)
    _compare(cozk, fused, comp, want, offset, 2 * MEM, tail)


def _written(ns, which):
    return {"all": [True] * ns, "none": [False] * ns, "some": [s % 2 == 1 for s in range(ns)]}[which]


def _values(seed, ns, n, written, shared):
    return [_value(seed + 2 * s, n, shared) for s in range(ns)], [_value(seed + 100 + 2 * s, n, shared) if written[s] else None for s in range(ns)]


@pytest.mark.parametrize("n", [1, 2, 63, 257, 4097])
@pytest.mark.parametrize("ns", [1, 4, 8])
def test_leaves_equal_the_composition_and_the_big_int_values(cozk, ctx, R3, n, ns):
    sm = O.SplitMix64(800 + n + ns)
    g, tau = sm.field(), sm.field()
    u8 = [s % 2 == 0 for s in range(ns)]  # U8 and U32 address columns mixed
    addr, t_read = _columns(801 + n, ns, n, u8)
    for mode, party in MODES:
        v_read, v_written = _values(810 + 10 * party, ns, n, _written(ns, "some"), mode == "rep3")
        _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, g, tau, mode, party)


@pytest.mark.parametrize("which", ["all", "none"])
@pytest.mark.parametrize("mode,party", MODES, ids=MODE_IDS)
def test_v_written_for_all_slots_and_for_none_past_a_workgroup_with_an_offset(cozk, ctx, R3, which, mode, party):
    """guard entries on both sides of out_a and out_b; the polynomials are longer than n"""
    sm = O.SplitMix64(820)
    n, u8 = 256 + 1, [False, True, True, False]
    addr, t_read = _columns(821, 4, n, u8)
    v_read, v_written = _values(822 + party, 4, n + 3, _written(4, which), mode == "rep3")
    _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, sm.field(), sm.field(), mode, party, offset=37, tail=5)


@pytest.mark.parametrize("MEM", [32, 4097])
@pytest.mark.parametrize("mode,party", MODES, ids=MODE_IDS)
def test_init_final_leaves(cozk, ctx, R3, MEM, mode, party):
    sm = O.SplitMix64(830 + MEM)
    shared = mode == "rep3"
    _check_if(cozk, ctx, R3, _value(831 + party, MEM + 1, shared), _value(841 + party, MEM, shared), _public(851 + MEM, MEM), sm.field(), sm.field(), mode, party,
              offset=11, tail=3)


@pytest.mark.parametrize("party", [0, 1, 2])
def test_rep3_calls_with_public_polynomials(cozk, ctx, R3, party):
    """a public polynomial joins the public part: v_init public beside a shared v_final (the harness's call), then every value public,
    then public and shared value columns mixed over the slots"""
    sm = O.SplitMix64(860 + party)
    g, tau = sm.field(), sm.field()
    MEM, n, ns = 300, 257, 4
    t_final = _public(861, MEM)
    _check_if(cozk, ctx, R3, _value(862, MEM, False), _value(863 + party, MEM, True), t_final, g, tau, "rep3", party, offset=3, tail=2)
    _check_if(cozk, ctx, R3, _value(862, MEM, False), _value(866, MEM, False), t_final, g, tau, "rep3", party)
    u8 = [True, True, True, False]
    addr, t_read = _columns(870, ns, n, u8)
    written = [False, False, True, True]
    v_read, v_written = _values(871, ns, n, written, False)
    _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, g, tau, "rep3", party)
    sh_read, sh_written = _values(880 + party, ns, n, written, True)
    mixed_read = [sh_read[0], v_read[1], sh_read[2], v_read[3]]
    mixed_written = [None, None, v_written[2], sh_written[3]]
    _check_rw(cozk, ctx, R3, addr, t_read, u8, mixed_read, mixed_written, g, tau, "rep3", party, offset=5, tail=1)


@pytest.mark.parametrize("g", [0, 1, R - 1, None], ids=["g_zero", "g_one", "g_minus_one", "g_random"])
@pytest.mark.parametrize("tau", [0, 1, R - 1, None], ids=["tau_zero", "tau_one", "tau_minus_one", "tau_random"])
def test_edge_shares_and_saturated_columns_with_gamma_and_tau_at_their_edges(cozk, ctx, R3, g, tau):
    sm = O.SplitMix64(890)
    g = sm.field() if g is None else g
    tau = sm.field() if tau is None else tau
    n, u8 = 70, [True, False, False]
    addr, t_read = _columns(891, 3, n, u8, top=True)
    for mode, party in MODES:
        shared = mode == "rep3"
        v_read = [_edge_value(n, shared) for _ in range(3)]
        v_written = [None, _edge_value(n, shared)[::-1], _edge_value(n, shared)]
        _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, g, tau, mode, party)
        _check_if(cozk, ctx, R3, _edge_value(n, shared), _edge_value(n, shared)[::-1], [TOP] * n, g, tau, mode, party)


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_good_calls_after_them(cozk, ctx, R3):
    n, ns, MEM = 200, 4, 64
    u8 = [True, True, True, False]
    addr, t_read = _columns(900, ns, n, u8)
    written = [False, False, True, True]
    v_read, v_written = _values(901, ns, n, written, False)
    sh_read, sh_written = _values(911, ns, n, written, True)
    d_addr = [(_u8 if u8[s] else _u32)(cozk, ctx, addr[s]) for s in range(ns)]
    d_tr = [_u32(cozk, ctx, c) for c in t_read]
    poly = lambda c: None if c is None else cozk.Rep3DensePolynomial.new(ctx, c)
    p_vr, p_vw, s_vr, s_vw = [poly(c) for c in v_read], [poly(c) for c in v_written], [poly(c) for c in sh_read], [poly(c) for c in sh_written]
    short_poly = poly(v_read[0][:-1])
    out, out_b = cozk.Vec.alloc(ctx, 2 * ns * n), cozk.Vec.alloc(ctx, 2 * ns * n)
    short_out = cozk.Vec.alloc(ctx, 2 * ns * n - 1)
    short = _u32(cozk, ctx, t_read[0][:-1])
    u16 = cozk.Vec.from_numpy(ctx, np.zeros(n, dtype=np.uint16), cozk.SCALAR_U16)
    u8v = _u8(cozk, ctx, [0] * n)
    W = "rw_memory_shared_leaves: "
    call = lambda a=d_addr, vr=p_vr, tr=d_tr, vw=p_vw, mode="plain", party=0, oa=out, ob=None, off=0: R3.rw_memory_shared_leaves(ctx, a, vr, tr, vw, 5, 7, mode, party, oa, ob, off)
    _refused(cozk, W + "addr[s] is a U8 or U32 vector", lambda: call(a=d_addr[:3] + [u16]))
    _refused(cozk, W + "addr[s] is a U8 or U32 vector", lambda: call(a=d_addr[:3] + [out_b]))
    _refused(cozk, W + "t_read[s] is a U32 vector", lambda: call(tr=d_tr[:3] + [u8v]))
    _refused(cozk, W + "every column has n entries", lambda: call(tr=d_tr[:3] + [short]))
    _refused(cozk, W + "every column has n entries", lambda: call(a=d_addr[:3] + [short]))
    _refused(cozk, W + "a value polynomial is shorter than n", lambda: call(vr=[short_poly] + p_vr[1:]))
    _refused(cozk, W + "a value polynomial is shorter than n", lambda: call(vw=p_vw[:3] + [short_poly]))
    _refused(cozk, W + "a shared value polynomial needs mode COZK_MODE_REP3", lambda: call(vr=s_vr))
    _refused(cozk, W + "a shared value polynomial needs mode COZK_MODE_REP3", lambda: call(vw=s_vw))
    _refused(cozk, W + "mode is COZK_MODE_PLAIN or COZK_MODE_REP3", lambda: call(mode=7))
    _refused(cozk, W + "0 <= party_id < 3", lambda: call(party=3))
    _refused(cozk, W + "0 <= party_id < 3", lambda: call(party=-1))
    _refused(cozk, W + "REP3 needs out_b", lambda: call(mode="rep3", vr=s_vr, vw=s_vw))
    _refused(cozk, W + "REP3 needs out_b", lambda: call(mode="rep3", vr=s_vr, vw=s_vw, ob=out))  # aliased
    _refused(cozk, W + "REP3 needs out_b", lambda: call(mode="rep3", vr=s_vr, vw=s_vw, ob=short_out))
    _refused(cozk, W + "REP3 needs out_b", lambda: call(mode="rep3", vr=s_vr, vw=s_vw, ob=d_tr[0]))
    _refused(cozk, W + "out_b is NULL for PLAIN", lambda: call(ob=out_b))
    _refused(cozk, W + "out_a is an FR vector with room for 2 n_slots n entries from offset", lambda: call(off=1))
    _refused(cozk, W + "out_a is an FR vector with room for 2 n_slots n entries from offset", lambda: call(oa=short_out))
    _refused(cozk, W + "out_a is an FR vector with room for 2 n_slots n entries from offset", lambda: call(oa=d_tr[0]))
    over = cozk.rw_memory.RW_MEMORY_MAX_SLOTS + 1
    _refused(cozk, W + "1 <= n_slots <= %d" % cozk.rw_memory.RW_MEMORY_MAX_SLOTS, lambda: call(a=d_addr[:1] * over, vr=p_vr[:1] * over, tr=d_tr[:1] * over, vw=None))
    t_final = _public(920, MEM)
    v_init, v_final, sh_final = _value(921, MEM, False), _value(922, MEM, False), _value(923, MEM, True)
    d_tf, p_vi, p_vf, s_vf = _u32(cozk, ctx, t_final), poly(v_init), poly(v_final), poly(sh_final)
    out2, out2_b = cozk.Vec.alloc(ctx, 2 * MEM), cozk.Vec.alloc(ctx, 2 * MEM)
    F = "rw_memory_shared_init_final_leaves: "
    inf = lambda vi=p_vi, vf=p_vf, tf=d_tf, mode="plain", party=0, oa=out2, ob=None, off=0: R3.rw_memory_shared_init_final_leaves(ctx, vi, vf, tf, 5, 7, mode, party, oa, ob, off)
    _refused(cozk, F + "t_final is a U32 vector", lambda: inf(tf=_u8(cozk, ctx, [0] * MEM)))
    _refused(cozk, F + "a value polynomial is shorter than MEM", lambda: inf(vi=poly(v_init[:-1])))
    _refused(cozk, F + "a value polynomial is shorter than MEM", lambda: inf(vf=poly(v_final[:-1])))
    _refused(cozk, F + "a shared value polynomial needs mode COZK_MODE_REP3", lambda: inf(vf=s_vf))
    _refused(cozk, F + "mode is COZK_MODE_PLAIN or COZK_MODE_REP3", lambda: inf(mode=7))
    _refused(cozk, F + "0 <= party_id < 3", lambda: inf(party=3))
    _refused(cozk, F + "REP3 needs out_b", lambda: inf(mode="rep3", vf=s_vf))
    _refused(cozk, F + "REP3 needs out_b", lambda: inf(mode="rep3", vf=s_vf, ob=out2))
    _refused(cozk, F + "out_b is NULL for PLAIN", lambda: inf(ob=out2_b))
    _refused(cozk, F + "out_a is an FR vector with room for 2 MEM entries from offset", lambda: inf(off=1))
    _refused(cozk, F + "out_a is an FR vector with room for 2 MEM entries from offset", lambda: inf(oa=d_tf))
    # the context works on after a refusal
    _check_rw(cozk, ctx, R3, addr, t_read, u8, v_read, v_written, 5, 7, "plain", 0)
    _check_rw(cozk, ctx, R3, addr, t_read, u8, sh_read, sh_written, 5, 7, "rep3", 1)
    _check_if(cozk, ctx, R3, v_init, sh_final, t_final, 5, 7, "rep3", 0)
