"""GPU tests of cozk_bytecode_leaves and cozk_bytecode_init_final_leaves (csrc/bytecode_leaves.hip): every leaf equal, byte for byte, to
the composition of cozk_fingerprint_leaves calls with an iota column (the four launches of flow_harness.hpp's phase 2) AND to the
big-int values of tests/bytecode_ref.py.  Lengths 1, 2, 63, 257, 4097 (the kernels have no grid stride: a workgroup covers 256 entries);
tables of 32 and 4097 rows; the column kinds mixed and all U64; every column at 2^64 - 1 with the imm word at r - 1 and gamma, tau in
{0, 1, r - 1} and a random pair; an I64 imm column with negatives (big-int only: the composition takes no I64 column) and the same
column as U64 (the composition too); a non-zero offset with guard entries on both sides; REP3 for parties 0, 1 and 2 with a shared and
with a public imm; each refusal with its text and the context working afterwards."""
import importlib

import numpy as np
import pytest

import bytecode_ref as B
import pyref as O

pytestmark = pytest.mark.gpu
R = O.R
INVALID_ARG = -1
GUARD = 0x5EED
M64 = (1 << 64) - 1
BITS = {1: 8, 2: 16, 3: 32, 4: 64}  # COZK_SCALAR_U8 .. U64
DTYPE = {1: np.uint8, 2: np.uint16, 3: np.uint32, 4: np.uint64}
MIXED = (3, 4, 4, 1, 2, 1, 3)       # a U32, address and bitflags U64, rd U8, rs1 U16, rs2 U8, t_read U32
WIDE = (4,) * 7


@pytest.fixture(scope="module")
def BC():
    return importlib.import_module("co-zkvms_amd.bytecode")


def _vec(cozk, ctx, col, kind):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=DTYPE[kind]), kind)


def _guarded(cozk, ctx, n):
    return cozk.Vec.from_numpy(ctx, np.tile(cozk.fr_to_mont_limbs([GUARD])[0], (n, 1)))


def _columns(seed, n, kinds, top=False):
    rng = np.random.default_rng(seed)
    return [[(1 << BITS[k]) - 1] * n if top else rng.integers(0, 1 << BITS[k], size=n, dtype=np.uint64, endpoint=False).tolist() for k in kinds]


def _field_column(seed, n):
    sm = O.SplitMix64(seed)
    return [sm.field() for _ in range(n)]


def _expect_shares(pub, sh, party):
    """add_public on the imm shares: party 0's a and party 1's b carry the public part"""
    a = [(x[0] + (p if party == 0 else 0)) % R for x, p in zip(sh, pub)]
    b = [(x[1] + (p if party == 1 else 0)) % R for x, p in zip(sh, pub)]
    return a, b


def _check_guards(cozk, got, offset, total, tail):
    guard = cozk.fr_to_mont_limbs([GUARD])[0]
    assert np.array_equal(got[:offset], np.tile(guard, (offset, 1))) and np.array_equal(got[offset + total:], np.tile(guard, (tail, 1)))


def _check_rw(cozk, ctx, BC, cols, kinds, imm, g, tau, mode="plain", party=0, public_imm=False, offset=0, tail=0):
    """imm: field elements (plain), or (a, b) shares with mode rep3; public_imm: a plain polynomial in a rep3 call"""
    n = len(cols[0])
    d = [_vec(cozk, ctx, c, k) for c, k in zip(cols, kinds)]
    poly = cozk.Rep3DensePolynomial.new(ctx, imm)
    rep3 = mode == "rep3"
    size = offset + 2 * n + tail
    outs = [[_guarded(cozk, ctx, size) for _ in range(2 if rep3 else 1)] for _ in range(2)]
    fused, comp = outs
    BC.bytecode_leaves(ctx, d[0], d[1:6], d[6], poly, g, tau, mode, party, *fused, offset=offset)
    p = B._powers(g)
    for c, const in ((0, -tau % R), (1, (p[7] - tau) % R)):  # flow_bytecode_worker's two read / write launches
        cozk.fingerprint_leaves(ctx, d, p[1:8], [poly], [1], const, mode, party, *comp, offset=offset + c * n, n=n)
    got = [v.to_numpy() for v in fused]
    for x, y in zip(got, comp):
        assert x.tobytes() == y.to_numpy().tobytes()
        _check_guards(cozk, x, offset, 2 * n, tail)
    zeros = [0] * n
    pub = B.read_write_leaves(cols[0], cols[1:6], cols[6], zeros if rep3 and not public_imm else imm, g, tau)
    pub = pub[0] + pub[1]
    if not rep3:
        want = [pub]
    else:
        sh = [(0, 0)] * (2 * n) if public_imm else list(imm) * 2
        want = _expect_shares(pub, sh, party)
    for x, w in zip(got, want):
        assert cozk.mont_limbs_to_int(x[offset:offset + 2 * n]) == list(w)


def _check_if(cozk, ctx, BC, table, kinds, t_final, t_kind, g, tau, mode="plain", party=0, offset=0, tail=0, compose=True):
    """kinds[5] == cozk.SCALAR_I64: table[5] is signed and only the big-int values are compared"""
    Bn = len(table[0])
    up = lambda col, k: cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.int64), k) if k == cozk.SCALAR_I64 else _vec(cozk, ctx, col, k)
    d = [up(c, k) for c, k in zip(table, kinds)]
    d_tf = _vec(cozk, ctx, t_final, t_kind)
    rep3 = mode == "rep3"
    size = offset + 2 * Bn + tail
    fused, comp = [[_guarded(cozk, ctx, size) for _ in range(2 if rep3 else 1)] for _ in range(2)]
    BC.bytecode_init_final_leaves(ctx, d, d_tf, g, tau, mode, party, *fused, offset=offset)
    got = [v.to_numpy() for v in fused]
    for x in got:
        _check_guards(cozk, x, offset, 2 * Bn, tail)
    if compose:
        iota = _vec(cozk, ctx, np.arange(Bn), 3)
        p = B._powers(g)
        init = [iota] + d[:5] + [d[5]]
        cozk.fingerprint_leaves(ctx, init, p[1:7] + [1], [], [], -tau % R, mode, party, *comp, offset=offset, n=Bn)
        cozk.fingerprint_leaves(ctx, init + [d_tf], p[1:7] + [1, p[7]], [], [], -tau % R, mode, party, *comp, offset=offset + Bn, n=Bn)
        for x, y in zip(got, comp):
            assert x.tobytes() == y.to_numpy().tobytes()
    pub = B.init_final_leaves(table, t_final, g, tau)
    pub = pub[0] + pub[1]
    want = [pub] if not rep3 else _expect_shares(pub, [(0, 0)] * (2 * Bn), party)
    for x, w in zip(got, want):
        assert cozk.mont_limbs_to_int(x[offset:offset + 2 * Bn]) == list(w)


@pytest.mark.parametrize("n", [1, 2, 63, 257, 4097])
@pytest.mark.parametrize("kinds", [MIXED, WIDE], ids=["mixed", "all_u64"])
def test_read_write_leaves_equal_the_composition_and_the_big_int_values(cozk, ctx, BC, n, kinds):
    sm = O.SplitMix64(600 + n)
    _check_rw(cozk, ctx, BC, _columns(601 + n, n, kinds), kinds, _field_column(602 + n, n), sm.field(), sm.field())


@pytest.mark.parametrize("Bn", [32, 4097])
@pytest.mark.parametrize("kinds", [MIXED, WIDE], ids=["mixed", "all_u64"])
def test_init_final_leaves_equal_the_composition_and_the_big_int_values(cozk, ctx, BC, Bn, kinds):
    sm = O.SplitMix64(610 + Bn)
    cols = _columns(611 + Bn, Bn, kinds)
    _check_if(cozk, ctx, BC, cols[:6], kinds[:6], cols[6], kinds[6], sm.field(), sm.field(), offset=11, tail=3)


@pytest.mark.parametrize("g", [0, 1, R - 1, None], ids=["g_zero", "g_one", "g_minus_one", "g_random"])
@pytest.mark.parametrize("tau", [0, 1, R - 1, None], ids=["tau_zero", "tau_one", "tau_minus_one", "tau_random"])
def test_every_column_saturated_with_gamma_and_tau_at_their_edges(cozk, ctx, BC, g, tau):
    sm = O.SplitMix64(630)
    g = sm.field() if g is None else g
    tau = sm.field() if tau is None else tau
    cols = _columns(631, 70, WIDE, top=True)
    _check_rw(cozk, ctx, BC, cols, WIDE, [R - 1] * 70, g, tau)
    _check_if(cozk, ctx, BC, cols[:6], WIDE[:6], cols[6], 4, g, tau)


def test_signed_imm_column_against_big_int_and_as_u64_against_the_composition(cozk, ctx, BC):
    sm = O.SplitMix64(640)
    g, tau = sm.field(), sm.field()
    _, table = B.bytecode_instance(641, 8, 300)  # -2^63 and 2^63 - 1 in rows 1 and 2, about half of the rest negative
    assert sum(v < 0 for v in table[5]) > 100 and sum(v > 0 for v in table[5]) > 100
    t_final = _columns(642, 300, (3,))[0]
    kinds = (4, 4, 1, 1, 1, cozk.SCALAR_I64)
    _check_if(cozk, ctx, BC, table, kinds, t_final, 3, g, tau, compose=False)
    unsigned = table[:5] + [[v & M64 for v in table[5]]]  # the same bits read as U64: another value, which the composition takes too
    _check_if(cozk, ctx, BC, unsigned, (4, 4, 1, 1, 1, 4), t_final, 3, g, tau)


def test_offset_with_guard_entries_past_a_workgroup(cozk, ctx, BC):
    sm = O.SplitMix64(650)
    _check_rw(cozk, ctx, BC, _columns(651, 257, MIXED), MIXED, _field_column(652, 257), sm.field(), sm.field(), offset=37, tail=5)


@pytest.mark.parametrize("party", [0, 1, 2])
def test_rep3_parties_against_fingerprint_leaves_in_rep3(cozk, ctx, BC, party):
    sm = O.SplitMix64(660 + party)
    g, tau = sm.field(), sm.field()
    n = 257
    cols = _columns(661, n, MIXED)
    shares = list(zip(_field_column(662 + party, n), _field_column(665 + party, n)))
    _check_rw(cozk, ctx, BC, cols, MIXED, shares, g, tau, mode="rep3", party=party, offset=3, tail=2)
    _check_rw(cozk, ctx, BC, cols, MIXED, _field_column(668, n), g, tau, mode="rep3", party=party, public_imm=True)
    _check_if(cozk, ctx, BC, cols[:6], MIXED[:6], cols[6], MIXED[6], g, tau, mode="rep3", party=party, offset=3, tail=2)


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_good_calls_after_them(cozk, ctx, BC):
    n = 200
    cols = _columns(670, n, MIXED)
    imm = _field_column(671, n)
    d = [_vec(cozk, ctx, c, k) for c, k in zip(cols, MIXED)]
    poly = cozk.Rep3DensePolynomial.new(ctx, imm)
    shared = cozk.Rep3DensePolynomial.new(ctx, list(zip(imm, imm)))
    short_poly = cozk.Rep3DensePolynomial.new(ctx, imm[:-1])
    out, out_b = cozk.Vec.alloc(ctx, 2 * n), cozk.Vec.alloc(ctx, 2 * n)
    short = _vec(cozk, ctx, cols[6][:-1], 3)
    i64 = cozk.Vec.from_numpy(ctx, np.zeros(n, dtype=np.int64), cozk.SCALAR_I64)
    rw = lambda a=d[0], v=d[1:6], t=d[6], p=poly, mode="plain", party=0, oa=out, ob=None, off=0: BC.bytecode_leaves(ctx, a, v, t, p, 5, 7, mode, party, oa, ob, off)
    _refused(cozk, "bytecode_leaves: a, v[0..4] and t_read are U8 / U16 / U32 / U64 vectors", lambda: rw(a=i64))
    _refused(cozk, "bytecode_leaves: a, v[0..4] and t_read are U8 / U16 / U32 / U64 vectors", lambda: rw(v=d[1:5] + [out]))
    _refused(cozk, "bytecode_leaves: every column has n entries", lambda: rw(t=short))
    _refused(cozk, "bytecode_leaves: imm is shorter than n", lambda: rw(p=short_poly))
    _refused(cozk, "bytecode_leaves: a shared imm needs mode COZK_MODE_REP3", lambda: rw(p=shared))
    _refused(cozk, "bytecode_leaves: mode is COZK_MODE_PLAIN or COZK_MODE_REP3", lambda: rw(mode=7))
    _refused(cozk, "bytecode_leaves: 0 <= party_id < 3", lambda: rw(party=3))
    _refused(cozk, "bytecode_leaves: out_a is an FR vector with room for two circuits from offset", lambda: rw(off=1))
    _refused(cozk, "bytecode_leaves: out_a is an FR vector with room for two circuits from offset", lambda: rw(oa=d[0]))
    _refused(cozk, "bytecode_leaves: REP3 needs out_b", lambda: rw(mode="rep3", p=shared))
    _refused(cozk, "bytecode_leaves: REP3 needs out_b", lambda: rw(mode="rep3", p=shared, ob=short))
    _refused(cozk, "bytecode_leaves: out_b is NULL for PLAIN", lambda: rw(ob=out_b))
    inf = lambda tb=d[:6], tf=d[6], mode="plain", party=0, oa=out, ob=None, off=0: BC.bytecode_init_final_leaves(ctx, tb, tf, 5, 7, mode, party, oa, ob, off)
    _refused(cozk, "bytecode_init_final_leaves: table[0..4] and t_final are U8 / U16 / U32 / U64 vectors", lambda: inf(tb=[i64] + d[1:6]))
    _refused(cozk, "bytecode_init_final_leaves: table[0..4] and t_final are U8 / U16 / U32 / U64 vectors", lambda: inf(tf=i64))
    _refused(cozk, "bytecode_init_final_leaves: table[5] is a U8 / U16 / U32 / U64 / I64 vector", lambda: inf(tb=d[:5] + [out_b]))
    _refused(cozk, "bytecode_init_final_leaves: every column has B entries", lambda: inf(tf=short))
    _refused(cozk, "bytecode_init_final_leaves: out_a is an FR vector with room for two circuits from offset", lambda: inf(off=1))
    _refused(cozk, "bytecode_init_final_leaves: REP3 needs out_b", lambda: inf(mode="rep3"))
    _refused(cozk, "bytecode_init_final_leaves: out_b is NULL for PLAIN", lambda: inf(ob=out_b))
    _refused(cozk, "bytecode_init_final_leaves: 0 <= party_id < 3", lambda: inf(party=-1))
    _check_rw(cozk, ctx, BC, cols, MIXED, imm, 5, 7)  # the context works on after a refusal
    _check_if(cozk, ctx, BC, cols[:6], MIXED[:6], cols[6], MIXED[6], 5, 7)
