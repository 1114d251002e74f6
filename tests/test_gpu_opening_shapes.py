"""The kernels behind the opening proof and the table builders at the shapes their small tests cannot show: eq tables past one
entry per thread of k_eq_build and through both starting buffers of k_eq_expand, the split-eq tables themselves after every bind
(cozk_spliteq_download), the opening round in both share modes, by value and through the pointer table, with mixed lengths and a
strided grid, the leaf fingerprints on their staged path and at the limits of the by-value one, the PST fold past one workgroup,
and every refusal.  Bit-exact.

Small cases are compared with oracle/pyref.py (pyspartan_outer.py for eq_plus_one); the long openings use device-generated
vectors and one big-int sum over their raw residues, tests/opening_ref.py (checked against the oracle on the CPU by
tests/test_opening_ref_model.py).

The launch constants of csrc/poly.hip and csrc/spartan_inner.inc that the shapes are chosen by -- a change there says which test
to resize:"""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import opening_ref as F
import pyref as O
import pyspartan_outer as S
import reduction_ref as X

pytestmark = pytest.mark.gpu
R = O.R

PT = 256                   # threads per workgroup (grid_for: one element per thread)
BATCH_GRID_MAX = 512       # workgroups of k_open_quadratic / k_open_quadratic_args at most: above, lanes stride
EQ_BUILD_THREADS = 1024    # k_eq_build is ONE workgroup of this many threads
EQ_BUILD_MAX_NV = 13       # eq_evals_device: nv <= 13 -> k_eq_build, above -> k_eq_expand launches
EQ_BUILD_SLOTS = 8         # fe e[8]: entries a k_eq_build thread can hold
OPEN_BY_VALUE_MAX = 16     # cozk_open_quadratic_evals: k <= 16 -> k_open_quadratic_args, above -> k_open_quadratic
LEAF_BY_VALUE_COLS = 16    # cozk_fingerprint_leaves: ks <= 16 && kp <= 8 -> k_fingerprint_leaves_args, else k_fingerprint_leaves
LEAF_BY_VALUE_POLYS = 8
LEAF_MAX = 32              # ks, kp <= 32
ERR_INVALID_ARG = -1       # COZK_ERR_INVALID_ARG (include/cozk.h)

EDGES = [R - 1, 0, 1]
SMALL_HALVES = [1, 257, 512, 513, 3 * PT + 5]  # one pair; two workgroups with a one-lane tail, two full ones, three and four ragged
BIG_HALF = (1 << 17) + (1 << 9) + 3            # 131587 > 512 x 256 = 131072 lanes: 515 lanes of the capped grid take two terms
assert BATCH_GRID_MAX * PT < BIG_HALF < 2 * BATCH_GRID_MAX * PT
assert all(h == 1 or h > PT for h in SMALL_HALVES)
RAGGED = 3 * PT + 5                            # 773 elements: three full workgroups and five lanes of a fourth


def _refused(call, *args):
    with pytest.raises(Exception) as e:
        call(*args)
    assert getattr(e.value, "code", None) == ERR_INVALID_ARG, e.value


# ------------------------------------------------------------------------------------------------ k_eq_build, k_eq_expand
EQ_NVS = [9, 10, 11, 12, 13, 14, 15, 16]
# the last level of nv reads 2^(nv - 1) entries: exactly one per thread at 11, two at 12, four at 13 (of the eight a thread can hold)
assert 1 << (11 - 1) == EQ_BUILD_THREADS
assert (1 << (EQ_BUILD_MAX_NV - 1)) // EQ_BUILD_THREADS == 4 <= EQ_BUILD_SLOTS
assert max(n for n in EQ_NVS if n <= EQ_BUILD_MAX_NV) == EQ_BUILD_MAX_NV and EQ_BUILD_MAX_NV + 1 in EQ_NVS and EQ_BUILD_MAX_NV + 2 in EQ_NVS


@pytest.mark.parametrize("nv", EQ_NVS)
def test_eq_evals_random_point(cozk, ctx, nv):
    """eq_evals_device: `if (nv <= 13)` takes k_eq_build, else the k_eq_expand launches, whose first buffer is `out` for even nv
    and `tmp` for odd nv.  A k_eq_build that drops a thread's second entry (e[cnt] with cnt stuck at 0) leaves the upper half of
    every level from nv = 12 wrong; an odd-nv result left in `tmp` gives the table of nv - 1 variables (or nothing) in `out`."""
    rng = O.SplitMix64(100 + nv)
    r = [rng.field() for _ in range(nv)]
    assert cozk.eq_evals(ctx, r).to_ints() == O.eq_evals(r)


@pytest.mark.parametrize("nv", EQ_NVS)
def test_eq_evals_edge_coordinates(cozk, ctx, nv):
    """the same dispatch with 0, 1 and r - 1 among the coordinates, first and last included: a coordinate 0 or 1 zeroes half of
    every later level, r - 1 makes `e - e * rj` wrap"""
    rng = O.SplitMix64(200 + nv)
    r = [rng.field() for _ in range(nv)]
    r[0], r[1], r[nv // 2], r[-2], r[-1] = R - 1, 0, 1, 0, R - 1
    r[3] = 1
    assert cozk.eq_evals(ctx, r).to_ints() == O.eq_evals(r)


@pytest.mark.parametrize("nv", [EQ_BUILD_MAX_NV, EQ_BUILD_MAX_NV + 2])
def test_eq_evals_boolean_point_is_an_indicator(cozk, ctx, nv):
    """the largest k_eq_build table and the odd k_eq_expand one at a Boolean point: the table is 1 at the point's big-endian index
    (r[0] is the most significant bit) and 0 elsewhere -- a bit order reversed, or (2i, 2i + 1) swapped, moves the one"""
    bits = [(0x5A3C96 >> j) & 1 for j in range(nv)]
    assert 0 < sum(bits) < nv and bits != bits[::-1]
    assert cozk.eq_evals(ctx, bits).to_ints() == F.indicator(1 << nv, F.big_endian_index(bits))


# ------------------------------------------------------------------------------------------------ k_eq_plus_one
@pytest.mark.parametrize("l", [10, 13])
def test_eq_plus_one_evals_past_two_workgroups(cozk, ctx, l):
    """grid_for(2^l) = 4 and 32 workgroups, one y per thread, against pyspartan_outer.eq_plus_one_evals: a random point; the
    Boolean x = 2^(l-1) - 1, whose successor 2^(l-1) has k = l - 1 trailing zeros and NO high part (m = 0: the loop over r_high
    must not run, r[l - 1 - k] = r[0] is the cleared bit); x = 2^l - 1, which has no successor: the all-zero table"""
    P = importlib.import_module("co-zkvms_amd.poly")
    n = 1 << l
    assert n // PT > 2
    rng = O.SplitMix64(300 + l)
    r = [rng.field() for _ in range(l)]
    assert P.eq_plus_one_evals(ctx, r).to_ints() == S.eq_plus_one_evals(r)[1]
    x = [0] + [1] * (l - 1)
    assert F.big_endian_index(x) + 1 == n // 2
    tab = P.eq_plus_one_evals(ctx, x).to_ints()
    assert tab == F.indicator(n, n // 2) == S.eq_plus_one_evals(x)[1]
    tab = P.eq_plus_one_evals(ctx, [1] * l).to_ints()
    assert tab == [0] * n == S.eq_plus_one_evals([1] * l)[1]


# ------------------------------------------------------------------------------------------------ k_fold_pairs, k_scale_by_first
SPLITEQ_NVS = [0, 1, 2, 3, 22, 27, 29]
# nv = 22: both halves 2^11 -- folds of 4, 2, 1 workgroups, k_scale_by_first over 8; nv = 27: E2 = 2^13 by k_eq_build at its limit,
# E1 = 2^14 by k_eq_expand from `out`; nv = 29: E2 = 2^14, E1 = 2^15 from `tmp`
assert (1 << (22 // 2)) // PT == 8 and (1 << (22 - 22 // 2)) // 2 // PT == 4
assert 27 // 2 == EQ_BUILD_MAX_NV and 27 - 27 // 2 == EQ_BUILD_MAX_NV + 1
assert 29 // 2 == EQ_BUILD_MAX_NV + 1 and 29 - 29 // 2 == EQ_BUILD_MAX_NV + 2


def _spliteq_equal(dev, ref):
    assert dev.lens() == (ref.E1_len, ref.E2_len)
    e1, e2 = dev.download()
    assert e1 == ref.E1[:ref.E1_len]
    assert e2 == ref.E2[:ref.E2_len]


@pytest.mark.parametrize("nv", SPLITEQ_NVS)
def test_spliteq_tables_after_construction_and_every_bind(cozk, ctx, nv):
    """cozk_spliteq_new builds E2 = evals(w[..m]) and E1 = evals(w[m..]); spliteq_advance folds E1 down to one value, then E2:
    `if (s.fold_n == 1)` is the one bind that also launches k_scale_by_first over all of E2.  Both tables are read back after
    construction and after EVERY bind: a k_scale_by_first that stops after its first workgroup leaves E2[256..] unscaled at the
    collapse, a k_fold_pairs with the wrong block stride breaks the first fold of more than one workgroup.  Challenges 0, 1 and
    r - 1 sit in an E1 fold, in the first E2 fold and in the last bind.  A bind of the fully bound object is refused and changes
    nothing."""
    rng = O.SplitMix64(400 + nv)
    w = [rng.field() for _ in range(nv)]
    dev, ref = cozk.SplitEqPolynomial(ctx, w), O.SplitEq(w)
    assert dev.get_num_vars() == nv
    _spliteq_equal(dev, ref)
    ch = [rng.field() for _ in range(nv)]
    n1 = nv - nv // 2  # binds of E1
    for i, e in zip((1, n1, nv - 1) if nv >= 22 else range(nv), EDGES):
        ch[i] = e
    if nv >= 3:
        assert sorted(ch.count(e) > 0 for e in EDGES) == [True] * 3
    for r in ch:
        dev.bind(r)
        ref.bind(r)
        _spliteq_equal(dev, ref)
    assert dev.lens() == (1, 1)
    _refused(dev.bind, rng.field())
    _spliteq_equal(dev, ref)
    dev.free()


def test_spliteq_download_refuses_a_foreign_context(cozk, ctx):
    """cozk_spliteq_download: `e->ctx == ctx`; either pointer may be null"""
    rng = O.SplitMix64(450)
    w = [rng.field() for _ in range(5)]
    dev, ref = cozk.SplitEqPolynomial(ctx, w), O.SplitEq(w)
    other = cozk.Context(0)
    try:
        _refused(dev.download, other)
    finally:
        other.close()
    e2 = np.zeros((ref.E2_len, 4), dtype=np.uint64)
    ctx.check(ctx._l.cozk_spliteq_download(ctx.h, dev.h, None, e2.ctypes.data))
    assert cozk.mont_limbs_to_int(e2) == ref.E2
    assert ctx._l.cozk_spliteq_download(ctx.h, None, None, e2.ctypes.data) == ERR_INVALID_ARG
    _spliteq_equal(dev, ref)
    dev.free()


# ------------------------------------------------------------------------------------------------ k_open_quadratic_args, k_open_quadratic
def _edge_rows(arr, half, shift):
    """r - 1, 0, 1 (Montgomery form) at the first and last index of each half"""
    for j, i in enumerate((0, half - 1, half, 2 * half - 1)):
        arr[i] = X.to_raw(F.residues([EDGES[(j + shift) % 3]]))[0]
    return arr


class _Opening:
    """one opening of length 2 * half: device-random raw words with the edge values written in, the device polynomials made of
    exactly those words, and the expected (eval_0, eval_2) from the big-int sum over them"""

    def __init__(self, cozk, ctx, half, mode, seed, zero=False):
        n = 2 * half
        words = [_edge_rows(cozk.Vec.random(ctx, n, seed=seed + 7 * c).to_numpy(), half, c) for c in range(3)]
        if zero:
            words[0][:] = 0
            words[1][:] = 0
        a, b, eq = words if mode == "rep3" else (words[0], None, words[2])
        vec = lambda x: cozk.Vec.from_numpy(ctx, x)
        self.poly = cozk.Rep3DensePolynomial.from_vec_shares(ctx, vec(a), vec(b) if b is not None else None)
        self.eq = cozk.Rep3DensePolynomial.from_vec_shares(ctx, vec(eq))
        ia, ib, ie = X.from_raw(a), X.from_raw(b) if b is not None else None, X.from_raw(eq)
        self.want = F.open_quadratic_raw(ia, ib, ie)
        if half <= 2048:  # the oracle's share arithmetic on the canonical values, where a walk is cheap
            va, ve = F.values(ia), F.values(ie)
            assert self.want == F.open_quadratic_pyref(list(zip(va, F.values(ib))) if ib is not None else va, ve)


def _halves(k, big_at=None):
    hs = [SMALL_HALVES[i % len(SMALL_HALVES)] for i in range(k)]
    if big_at is not None:
        hs[big_at] = BIG_HALF
    return hs


OPEN_CASES = [(1, 0), (OPEN_BY_VALUE_MAX, None), (OPEN_BY_VALUE_MAX + 1, 5), (40, None)]


@pytest.mark.parametrize("k,big_at", OPEN_CASES, ids=["k%d" % c[0] for c in OPEN_CASES])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_open_quadratic_mixed_lengths_both_kernels(cozk, ctx, mode, k, big_at):
    """cozk_open_quadratic_evals: `if (k <= 16)` passes the operands by value to k_open_quadratic_args<NC>, else uploads the pointer
    table for k_open_quadratic<NC>; NC = 1 plain, 2 Rep3 (eval = TWO_INV (a + b) . eq).  One call mixes half = 1, 257, 512, 513 and
    773; the grid is sized by the longest (not the first in the list), so the workgroups of a shorter opening past its end must
    store zeros into their own rows partial[(2 y + e) * gridDim.x + x] -- a row index built from the wrong block coordinate, or a
    stale partial, shows in a neighbour.  k = 1 and k = 17 hold half = 131587 > 512 x 256 lanes: lanes 0..514 take two terms."""
    assert (k <= OPEN_BY_VALUE_MAX) == (k in (1, 16)) and (big_at is None or k in (1, OPEN_BY_VALUE_MAX + 1))
    hs = _halves(k, big_at)
    assert k == 1 or max(hs) != hs[0]
    ops = [_Opening(cozk, ctx, h, mode, seed=1000 * k + 31 * i + (mode == "plain")) for i, h in enumerate(hs)]
    got = cozk.open_quadratic_evals([o.poly for o in ops], [o.eq for o in ops])
    assert got == [o.want for o in ops]


@pytest.mark.parametrize("k", [3, OPEN_BY_VALUE_MAX + 2])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_open_quadratic_zero_polynomial_between_neighbours(cozk, ctx, mode, k):
    """an all-zero polynomial in the middle of the list: its two rows come back exactly (0, 0) beside non-zero neighbours, in both
    kernels (k = 3 by value, k = 18 through the pointer table)"""
    hs = _halves(k)
    z = k // 2
    hs[z] = RAGGED
    ops = [_Opening(cozk, ctx, h, mode, seed=77 * k + i, zero=(i == z)) for i, h in enumerate(hs)]
    got = cozk.open_quadratic_evals([o.poly for o in ops], [o.eq for o in ops])
    assert got == [o.want for o in ops]
    assert got[z] == (0, 0) and all(g != (0, 0) for i, g in enumerate(got) if i != z)


def test_open_quadratic_refusals_leave_the_context_usable(cozk, ctx):
    """k = 0, a null polynomial or eq, a Rep3 eq, lengths that differ, mixed share modes: COZK_ERR_INVALID_ARG each, and the next
    valid call on the same context gives the right sums"""
    l = ctx._l
    vp = ctypes.c_void_p
    a = _Opening(cozk, ctx, 257, "rep3", seed=1)
    b = _Opening(cozk, ctx, 5, "rep3", seed=2)
    p = _Opening(cozk, ctx, 257, "plain", seed=3)
    out = np.zeros((4, 4), dtype=np.uint64)

    def call(polys, eqs, k=2):
        return l.cozk_open_quadratic_evals(ctx.h, (vp * 2)(*polys), (vp * 2)(*eqs), k, out.ctypes.data)

    bad = [
        call([a.poly.h, b.poly.h], [a.eq.h, b.eq.h], k=0),
        call([a.poly.h, None], [a.eq.h, b.eq.h]),
        call([a.poly.h, b.poly.h], [a.eq.h, None]),
        call([a.poly.h, b.poly.h], [a.eq.h, b.poly.h]),   # a Rep3 eq
        call([a.poly.h, b.poly.h], [a.eq.h, a.eq.h]),     # len(eq) != len(poly)
        call([a.poly.h, p.poly.h], [a.eq.h, p.eq.h]),     # Rep3 and plain polynomials in one call
        call([p.poly.h, a.poly.h], [p.eq.h, a.eq.h]),
    ]
    for rc in bad:
        assert rc == ERR_INVALID_ARG
        assert cozk.open_quadratic_evals([a.poly, b.poly], [a.eq, b.eq]) == [a.want, b.want]
    assert cozk.open_quadratic_evals([p.poly], [p.eq]) == [p.want]


# ------------------------------------------------------------------------------------------------ k_fingerprint_leaves, k_fingerprint_leaves_args
LEAF_N, LEAF_OFFSET, LEAF_TAIL = RAGGED, 37, 19
LEAF_SHAPES = [(16, 8), (17, 1), (1, 9), (32, 32), (0, 3), (5, 0)]
assert LEAF_SHAPES[0] == (LEAF_BY_VALUE_COLS, LEAF_BY_VALUE_POLYS) and LEAF_SHAPES[1][0] == LEAF_BY_VALUE_COLS + 1
assert LEAF_SHAPES[2][1] == LEAF_BY_VALUE_POLYS + 1 and LEAF_SHAPES[3] == (LEAF_MAX, LEAF_MAX)
_BITS = {"U64": 64, "U8": 8, "U16": 16, "U32": 32}
_KIND_ORDER = ["U64", "U8", "U16", "U32"]  # the single column of the (1, 9) shape is a U64 one


def _staged(ks, kp):
    return not (ks <= LEAF_BY_VALUE_COLS and kp <= LEAF_BY_VALUE_POLYS)


@functools.lru_cache(maxsize=None)
def _leaf_case(ks, kp):
    """the data of one shape, shared by the four provers: compact columns of all four kinds (some longer than n) with their extreme
    values, polynomials alternately SHARED (a secret and its three additive parts) and public, coefficients with r - 1, 0 and 1"""
    rng = O.SplitMix64(5000 + 40 * ks + kp)
    n = LEAF_N
    kinds = [_KIND_ORDER[k % 4] for k in range(ks)]
    cols = []
    for k, kind in enumerate(kinds):
        col = [rng.next() & ((1 << _BITS[kind]) - 1) for _ in range(n + (3 if k % 3 == 1 else 0))]
        top = (1 << _BITS[kind]) - 1
        col[0], col[1], col[n - 1] = top, 0, top
        if kind == "U64":  # the high word x.l[1]: all ones, exactly one, exactly zero under a full low word
            col[2], col[3], col[n - 2] = 1 << 32, (1 << 32) - 1, 1 << 63
        cols.append(col)
    polys = []
    for j in range(kp):
        v = [rng.field() for _ in range(n + (2 if j % 4 == 3 else 0))]
        v[0], v[1], v[n - 1] = R - 1, 0, R - 1
        if j % 2 == 0:
            t0, t1 = [rng.field() for _ in v], [rng.field() for _ in v]
            polys.append(("shared", v, [t0, t1, [(x - y - z) % R for x, y, z in zip(v, t0, t1)]]))
        else:
            polys.append(("public", v, None))
    cc = ([R - 1, 0, 1] + [rng.field() for _ in range(ks)])[:ks]
    pc = ([1, R - 1, 0] + [rng.field() for _ in range(kp)])[:kp]
    return dict(kinds=kinds, cols=cols, polys=polys, cc=cc, pc=pc, constant=rng.field())


def _party_polys(case, party):
    """the polynomial lists of one prover: the plain prover holds the secrets, party p the Rep3 share (t_p, t_{p-1})"""
    out = []
    for kind, v, t in case["polys"]:
        out.append(list(zip(t[party], t[(party + 2) % 3])) if kind == "shared" and party is not None else v)
    return out


def _run_leaves(cozk, ctx, case, party):
    """-> the n leaves of `party` ((a, b) pairs, plain values for party None), written at LEAF_OFFSET into a longer output whose
    other elements must keep their values"""
    rng = O.SplitMix64(9)
    total = LEAF_OFFSET + LEAF_N + LEAF_TAIL
    fill = [[rng.field() for _ in range(total)] for _ in range(2)]
    mode = "plain" if party is None else "rep3"
    out_a = cozk.Vec.from_ints(ctx, fill[0])
    out_b = cozk.Vec.from_ints(ctx, fill[1]) if mode == "rep3" else None
    cols = [cozk.Vec.from_ints(ctx, c, kind=getattr(cozk, "SCALAR_" + k)) for c, k in zip(case["cols"], case["kinds"])]
    polys = [cozk.Rep3DensePolynomial.new(ctx, p) for p in _party_polys(case, party)]
    cozk.fingerprint_leaves(ctx, cols, case["cc"], polys, case["pc"], case["constant"], mode, party or 0, out_a, out_b, offset=LEAF_OFFSET, n=LEAF_N)
    got = []
    for o, f in zip((out_a, out_b), fill):
        if o is None:
            continue
        v = o.to_ints()
        assert v[:LEAF_OFFSET] == f[:LEAF_OFFSET] and v[LEAF_OFFSET + LEAF_N:] == f[LEAF_OFFSET + LEAF_N:]
        got.append(v[LEAF_OFFSET:LEAF_OFFSET + LEAF_N])
    return got[0] if party is None else list(zip(*got))


def _leaves_ref(case, party):
    # O.fingerprint_leaves stops at the shortest list: the device is told n
    return O.fingerprint_leaves([c[:LEAF_N] for c in case["cols"]], case["cc"], [p[:LEAF_N] for p in _party_polys(case, party)], case["pc"],
                                case["constant"], party)


@pytest.mark.parametrize("party", [None, 0, 1, 2])
@pytest.mark.parametrize("ks,kp", LEAF_SHAPES, ids=["%dx%d" % s for s in LEAF_SHAPES])
def test_fingerprint_leaves_by_value_limits_and_staged_path(cozk, ctx, ks, kp, party):
    """cozk_fingerprint_leaves: `if (ks <= 16 && kp <= 8)` fills FingerprintArgs for k_fingerprint_leaves_args<NC>, else stages
    dcols | dcs | dds | da | db in one scratch block (32-byte and 16-byte aligned by hand) for k_fingerprint_leaves<NC>: (16, 8) is
    the last by-value shape, (17, 1) and (1, 9) the first staged ones on either limit, (32, 32) the largest (dds / da overlapping
    there would turn the last coefficients into pointers), (0, 3) and (5, 0) the empty lists.  n = 773 at offset 37 of a longer
    output; U64 columns hold 2^64 - 1, 2^32, 2^32 - 1 and 2^63 (a high word ignored changes those leaves only); public polynomials
    enter party 0's a and party 1's b, and for party 2 both of their pointers are null."""
    assert _staged(ks, kp) == ((ks, kp) in [(17, 1), (1, 9), (32, 32)])
    case = _leaf_case(ks, kp)
    assert _run_leaves(cozk, ctx, case, party) == _leaves_ref(case, party)


def test_fingerprint_leaves_largest_shape_parties_open_to_the_plain_prover(cozk, ctx):
    """(32, 32), staged, Rep3: a_0 + a_1 + a_2 of every leaf is the plain prover's leaf -- the public part (columns, public
    polynomials, constant) is added exactly once"""
    case = _leaf_case(LEAF_MAX, LEAF_MAX)
    parts = [_run_leaves(cozk, ctx, case, p) for p in range(3)]
    assert [(x[0] + y[0] + z[0]) % R for x, y, z in zip(*parts)] == _leaves_ref(case, None)
    for p in range(3):  # Rep3: party p's b is party p - 1's a
        assert [s[1] for s in parts[p]] == [s[0] for s in parts[(p + 2) % 3]]


def test_fingerprint_leaves_refusals_leave_the_context_usable(cozk, ctx):
    """ks = 33, kp = 33, an FR vector as a column, a column or polynomial shorter than n, offset + n past the output, a shared
    polynomial with a plain output, a Rep3 output without out_b: COZK_ERR_INVALID_ARG each, nothing written, and the valid call
    that follows is right"""
    rng = O.SplitMix64(600)
    n = 40
    col_ref = [rng.next() & 0xFFFF for _ in range(n)]
    shared_ref = [(rng.field(), rng.field()) for _ in range(n)]
    pub_ref = [rng.field() for _ in range(n)]
    col = cozk.Vec.from_ints(ctx, col_ref, kind=cozk.SCALAR_U16)
    short_col = cozk.Vec.from_ints(ctx, col_ref[:n - 1], kind=cozk.SCALAR_U16)
    fr_col = cozk.Vec.from_ints(ctx, pub_ref)
    shared, pub = cozk.Rep3DensePolynomial.new(ctx, shared_ref), cozk.Rep3DensePolynomial.new(ctx, pub_ref)
    short_poly = cozk.Rep3DensePolynomial.new(ctx, pub_ref[:n - 1])
    fill = [rng.field() for _ in range(n + 2)]
    out_a, out_b = cozk.Vec.from_ints(ctx, fill), cozk.Vec.from_ints(ctx, fill)
    c, d, cst = rng.field(), rng.field(), rng.field()
    fl = lambda *a, **kw: cozk.fingerprint_leaves(ctx, *a, **kw)
    bad = [
        lambda: fl([col] * (LEAF_MAX + 1), [c] * (LEAF_MAX + 1), [pub], [d], cst, "rep3", 0, out_a, out_b, offset=1, n=n),
        lambda: fl([col], [c], [pub] * (LEAF_MAX + 1), [d] * (LEAF_MAX + 1), cst, "rep3", 0, out_a, out_b, offset=1, n=n),
        lambda: fl([fr_col], [c], [pub], [d], cst, "rep3", 0, out_a, out_b, offset=1, n=n),
        lambda: fl([short_col], [c], [pub], [d], cst, "rep3", 0, out_a, out_b, offset=1, n=n),
        lambda: fl([col], [c], [short_poly], [d], cst, "rep3", 0, out_a, out_b, offset=1, n=n),
        lambda: fl([col], [c], [pub], [d], cst, "rep3", 0, out_a, out_b, offset=3, n=n),
        lambda: fl([col], [c], [shared], [d], cst, "plain", 0, out_a, None, offset=1, n=n),
        lambda: fl([col], [c], [shared], [d], cst, "rep3", 0, out_a, None, offset=1, n=n),
    ]
    for call in bad:
        _refused(call)
        assert out_a.to_ints() == fill and out_b.to_ints() == fill
    fl([col], [c], [shared, pub], [d, c], cst, "rep3", 1, out_a, out_b, offset=1, n=n)
    want = O.fingerprint_leaves([col_ref], [c], [shared_ref, pub_ref], [d, c], cst, 1)
    assert list(zip(out_a.to_ints()[1:n + 1], out_b.to_ints()[1:n + 1])) == want


# ------------------------------------------------------------------------------------------------ k_pst_fold
PST_HALVES = [1, 257, 513, RAGGED]
PST_POINTS = {"zero": 0, "one": 1, "r_minus_1": R - 1, "random": None}


@pytest.mark.parametrize("point", list(PST_POINTS))
@pytest.mark.parametrize("h", PST_HALVES)
def test_pst_fold_past_one_workgroup_into_longer_outputs(cozk, ctx, h, point):
    """grid_for(h) = 1, 2, 3 and 4 workgroups (a one-lane tail, a ragged one): q[b] = r[2b + 1] - r[2b] and
    r'[b] = r[2b] + p q[b] with r - 1 at both ends of r, the fold point 0, 1, r - 1 and random; q and r' are LONGER than h and
    their tails keep their values (`if (i >= half) return`)"""
    rng = O.SplitMix64(700 + h)
    p = PST_POINTS[point] if PST_POINTS[point] is not None else rng.field()
    r = [rng.field() for _ in range(2 * h)]
    r[0] = r[-1] = R - 1
    fq, fr = [rng.field() for _ in range(h + 5)], [rng.field() for _ in range(h + 9)]
    q, rn = cozk.Vec.from_ints(ctx, fq), cozk.Vec.from_ints(ctx, fr)
    cozk.pst_fold(ctx, cozk.Vec.from_ints(ctx, r), p, q, rn)
    want_q, want_r = F.pst_fold(r, p)
    assert q.to_ints() == want_q + fq[h:]
    assert rn.to_ints() == want_r + fr[h:]


def test_pst_fold_refusals_leave_the_outputs_untouched(cozk, ctx):
    """cozk_pst_fold: an odd or empty r, outputs shorter than r->n / 2, and r, q or r_next that is not an FR vector -- the check
    `q->kind == COZK_SCALAR_FR && r_next->kind == COZK_SCALAR_FR` is what keeps a U8 vector of h BYTES from receiving h field
    elements.  COZK_ERR_INVALID_ARG each; the FR outputs keep their values and the next valid fold is right."""
    rng = O.SplitMix64(800)
    h = 257
    r_ref = [rng.field() for _ in range(2 * h)]
    fill = [rng.field() for _ in range(h)]
    r = cozk.Vec.from_ints(ctx, r_ref)
    q, rn = cozk.Vec.from_ints(ctx, fill), cozk.Vec.from_ints(ctx, fill)
    p = rng.field()
    bytes_h = cozk.Vec.from_ints(ctx, [7] * h, kind=cozk.SCALAR_U8)
    words_h = cozk.Vec.from_ints(ctx, [7] * h, kind=cozk.SCALAR_U64)
    bytes_2h = cozk.Vec.from_ints(ctx, [7] * (2 * h), kind=cozk.SCALAR_U8)
    bad = [
        (cozk.Vec.from_ints(ctx, r_ref[:2 * h - 1]), q, rn),
        (cozk.Vec.alloc(ctx, 0), q, rn),
        (r, cozk.Vec.from_ints(ctx, fill[:h - 1]), rn),
        (r, q, cozk.Vec.from_ints(ctx, fill[:h - 1])),
        (bytes_2h, q, rn),
        (r, bytes_h, rn),
        (r, q, bytes_h),
        (r, words_h, rn),
        (r, q, words_h),
    ]
    for rv, qv, nv in bad:
        _refused(cozk.pst_fold, ctx, rv, p, qv, nv)
        assert q.to_ints() == fill and rn.to_ints() == fill
        assert bytes_h.to_ints() == [7] * h and words_h.to_ints() == [7] * h
    cozk.pst_fold(ctx, r, p, q, rn)
    assert (q.to_ints(), rn.to_ints()) == F.pst_fold(r_ref, p)


# ------------------------------------------------------------------------------------------------ the same omission elsewhere
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_mul_vec_local_refuses_narrow_vectors(cozk, ctx, mode):
    """cozk_rep3_mul_vec_local compared element counts only: a U8 vector of n entries as any share component would be read as n
    field elements.  Every position is refused, and the valid call that follows is O.rep3_local_mul"""
    rng = O.SplitMix64(900)
    n = 300
    xs, ys = [(rng.field(), rng.field()) for _ in range(n)], [(rng.field(), rng.field()) for _ in range(n)]
    V = cozk.Vec
    xa, xb, ya, yb = (V.from_ints(ctx, [s[c] for s in v]) for v in (xs, ys) for c in (0, 1))
    narrow = V.from_ints(ctx, [3] * n, kind=cozk.SCALAR_U8)
    good = [xa, xb, ya, yb] if mode == "rep3" else [xa, None, ya, None]
    for i, v in enumerate(good):
        if v is not None:
            _refused(cozk.rep3_mul_vec_local, ctx, *(good[:i] + [narrow] + good[i + 1:]))
    got = cozk.rep3_mul_vec_local(ctx, *good).to_ints()
    if mode == "rep3":
        assert got == [O.rep3_local_mul(x, y) for x, y in zip(xs, ys)]
    else:
        assert got == [x[0] * y[0] % R for x, y in zip(xs, ys)]
