"""The kernels behind co-noir-spartan's worker and co-jolt's Spartan inner / shift sumchecks at the shapes one workgroup of random
values cannot show: several workgroups (the partial[e * gridDim.x + block] rows that k_finish_sums adds up), a grid-stride loop that
gives a lane two terms, the long-row queue of the sparse matrix-vector product, every degree and limit of the product list, the wide
accumulator of the batched dot product past its third word, and the refusals.  Bit-exact, both share modes where the kernel has both.

Small random cases are compared with the brute-force oracles (oracle/pyref.py, oracle/pylogup.py); the large ones use periodic
tables, whose exact sums tests/seam_ref.py computes from one period (checked against the same oracles on the CPU by
tests/test_seam_ref_model.py).

The launch constants of csrc/poly.hip and csrc/logup.inc that the shapes are chosen by -- a change there says which test to resize:"""
import ctypes
import importlib

import numpy as np
import pytest

import pylogup as G
import pyref as O
import reduction_ref as X
import seam_ref as S

pytestmark = pytest.mark.gpu
R = O.R

PT = 256                # threads per workgroup
BATCH_GRID_MAX = 512    # k_prod_round, k_spartan_first, k_spartan_second
ROUND_GRID_MAX = 1024   # k_prodlist_round
EVAL_GRID_MAX = 192     # k_poly_batch_dot_public
SPMV_LONG = 64          # a row with more entries goes to the queue
SPMV_CHUNK = 2048       # entries per queued work item
G_ITEMS = 4096          # workgroups of k_sparse_matvec3_items at most
G_ROWS = 1024           # workgroups of k_sparse_matvec3_rows at most
PL_MAX_POLYS, PL_MAX_TERMS, PL_MAX_FACTORS = 48, 32, 4
ERR_INVALID_ARG = -1    # COZK_ERR_INVALID_ARG (include/cozk.h)

SMALL_HALVES = [257, 512, 513, 3 * 256 + 5]  # two workgroups with a one-lane tail, two full ones, three and four ragged
BIG_HALF = (1 << 17) + (1 << 9) + 3          # 131587 > 512 x 256 = 131072 lanes: 515 lanes of the capped grid take two terms
assert BATCH_GRID_MAX * PT < BIG_HALF < 2 * BATCH_GRID_MAX * PT


def _rand(rng, n, mode):
    return [(rng.field(), rng.field()) for _ in range(n)] if mode == "rep3" else [rng.field() for _ in range(n)]


def _pattern(rng, mode):
    """one period of a table: random, with r - 1, 0 and 1 among the entries"""
    pat = _rand(rng, S.PERIOD, mode)
    edge = [R - 1, 0, 1]
    for k, e in enumerate(edge):
        pat[5 * k] = (e, edge[(k + 1) % 3]) if mode == "rep3" else e
    return pat


def _new(cozk, ctx, coeffs):
    return cozk.Rep3DensePolynomial.new(ctx, coeffs)


def _second(cozk, mode, polys, coef):
    got = cozk.spartan_second_round(*polys, coef)
    return [g[0] for g in got] if mode == "plain" else got


def _follow_periodic(cozk, ctx, tables, order, device_round, ref_round, rng, rounds=3):
    """round 0 of the periodic tables, then `rounds - 1` more after binding on the device; the bound polynomials' first, middle and
    last coefficients at the end"""
    polys = [S.tiled_poly(ctx, cozk, t) for t in tables]
    for _ in range(rounds):
        assert device_round(polys) == ref_round(tables)
        r = rng.field()
        for p in polys:
            p.bind(r, order)
        tables = [S.bind(t, r, order) for t in tables]
    for p, (pattern, n) in zip(polys, tables):
        assert len(p) == n
        for i in (0, n // 2, n - 1):
            assert p.get_bound_coeff(i) == pattern[i % len(pattern)]


# ------------------------------------------------------------------------------------------------ k_prod_round
# (mode, m, degree, index of the shared factor): degree = m for m = 1..4, degree < m, the shared factor first, in the middle, last
PROD_CASES = [("plain", m, d, None) for m, d in [(1, 1), (2, 2), (3, 3), (4, 4), (3, 2)]] + \
             [("rep3", m, d, s) for m, d, s in [(1, 1, 0), (2, 2, 0), (2, 2, 1), (3, 3, 0), (3, 3, 1), (3, 3, 2), (4, 4, 0), (4, 4, 2), (4, 4, 3),
                                               (3, 2, 1)]]
PROD_IDS = ["%s-m%d-d%d-s%s" % c for c in PROD_CASES]


@pytest.mark.parametrize("half", SMALL_HALVES)
@pytest.mark.parametrize("mode,m,degree,shared_at", PROD_CASES, ids=PROD_IDS)
def test_prod_round_several_workgroups_all_rounds(cozk, ctx, mode, m, degree, shared_at, half):
    """2 to 4 workgroups (one lane, none, or five lanes past a full one), then every round down to one element -- odd lengths on the
    way drop their last element as dense_bind does -- against O.prod_round_evals"""
    rng = O.SplitMix64(1000 * half + 10 * m + degree + (shared_at or 0))
    ref = [_rand(rng, 2 * half, "rep3" if j == shared_at else "plain") for j in range(m)]
    polys = [_new(cozk, ctx, c) for c in ref]
    while len(ref[0]) >= 2:
        assert cozk.prod_sumcheck_evals(polys, degree) == O.prod_round_evals(ref, degree)
        r = rng.field()
        for p in polys:
            p.bind(r, cozk.HIGH_TO_LOW)
        ref = [O.dense_bind(c, r, O.HIGH_TO_LOW) for c in ref]
    assert [p.coeffs() for p in polys] == ref


@pytest.mark.parametrize("mode,m,degree,shared_at", PROD_CASES, ids=PROD_IDS)
def test_prod_round_two_terms_per_lane(cozk, ctx, mode, m, degree, shared_at):
    """cap: BATCH_GRID_MAX = 512 workgroups x 256 lanes = 131072 lanes; half = 2^17 + 2^9 + 3 = 131587 gives lanes 0..514 two terms
    and fills all 512 partials of every row.  Rounds 1 and 2 (half = 65793, 32896: 258 and 129 workgroups, ragged) follow the
    device's own HighToLow binds of an odd length."""
    rng = O.SplitMix64(77 + 10 * m + degree + (shared_at or 0))
    tables = [(_pattern(rng, "rep3" if j == shared_at else "plain"), 2 * BIG_HALF) for j in range(m)]
    _follow_periodic(cozk, ctx, tables, cozk.HIGH_TO_LOW, lambda ps: cozk.prod_sumcheck_evals(ps, degree),
                     lambda ts: S.prod_round_evals(ts, degree), rng)


# ------------------------------------------------------------------------------------------------ k_spartan_first / k_spartan_second
@pytest.mark.parametrize("half", SMALL_HALVES)
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_spartan_first_several_workgroups_all_rounds(cozk, ctx, mode, half):
    """the eight partial rows (four of A x B x pub, four of C x pub) over 2 to 4 workgroups, every round down to length 2"""
    rng = O.SplitMix64(31 * half + (mode == "plain"))
    ref = [_rand(rng, 2 * half, mode) for _ in range(3)] + [_rand(rng, 2 * half, "plain")]
    polys = [_new(cozk, ctx, c) for c in ref]
    while len(ref[0]) >= 2:
        assert cozk.spartan_first_round(*polys) == O.spartan_first_round_evals(*ref)
        r = rng.field()
        for p in polys:
            p.bind(r, cozk.LOW_TO_HIGH)
        ref = [O.dense_bind(c, r, O.LOW_TO_HIGH) for c in ref]
    assert [p.coeffs() for p in polys] == ref


def _coef(kind, rng):
    return {"random": [rng.field() for _ in range(3)], "one_zero": [rng.field(), 0, rng.field()], "all_r_minus_1": [R - 1] * 3}[kind]


@pytest.mark.parametrize("coef", ["random", "one_zero", "all_r_minus_1"])
@pytest.mark.parametrize("half", SMALL_HALVES)
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_spartan_second_several_workgroups_all_rounds(cozk, ctx, mode, half, coef):
    """the 3 (plain) or 6 (Rep3: component k in rows 3k .. 3k + 2) partial rows over 2 to 4 workgroups, every round down to length 2"""
    rng = O.SplitMix64(37 * half + (mode == "plain") + len(coef))
    cf = _coef(coef, rng)
    ref = [_rand(rng, 2 * half, mode)] + [_rand(rng, 2 * half, "plain") for _ in range(3)]
    polys = [_new(cozk, ctx, c) for c in ref]
    while len(ref[0]) >= 2:
        assert _second(cozk, mode, polys, cf) == O.spartan_second_round_evals(*ref, cf)
        r = rng.field()
        for p in polys:
            p.bind(r, cozk.LOW_TO_HIGH)
        ref = [O.dense_bind(c, r, O.LOW_TO_HIGH) for c in ref]
    assert [p.coeffs() for p in polys] == ref


@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_spartan_first_two_terms_per_lane(cozk, ctx, mode):
    """cap: BATCH_GRID_MAX = 512 x 256 = 131072 lanes; half = 131587 gives lanes 0..514 two terms in each of the eight accumulators.
    Rounds 1 and 2 run on the device's LowToHigh binds (length 131587, odd, then 65793)."""
    rng = O.SplitMix64(501 + (mode == "plain"))
    tables = [(_pattern(rng, mode), 2 * BIG_HALF) for _ in range(3)] + [(_pattern(rng, "plain"), 2 * BIG_HALF)]
    _follow_periodic(cozk, ctx, tables, cozk.LOW_TO_HIGH, lambda ps: cozk.spartan_first_round(*ps), lambda ts: S.spartan_first_round_evals(*ts), rng)


@pytest.mark.parametrize("coef", ["random", "one_zero", "all_r_minus_1"])
@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_spartan_second_two_terms_per_lane(cozk, ctx, mode, coef):
    """cap: BATCH_GRID_MAX = 512 x 256 = 131072 lanes; half = 131587 gives lanes 0..514 two terms; then two rounds on the device's
    binds"""
    rng = O.SplitMix64(601 + (mode == "plain") + len(coef))
    cf = _coef(coef, rng)
    tables = [(_pattern(rng, mode), 2 * BIG_HALF)] + [(_pattern(rng, "plain"), 2 * BIG_HALF) for _ in range(3)]
    _follow_periodic(cozk, ctx, tables, cozk.LOW_TO_HIGH, lambda ps: _second(cozk, mode, ps, cf), lambda ts: S.spartan_second_round_evals(*ts, cf), rng)


# ------------------------------------------------------------------------------------------------ k_prodlist_round
def _LG():
    return importlib.import_module("co-zkvms_amd.logup")


def _prodlist_all_rounds(cozk, ctx, polys_ref, products, rng):
    """every round message and the final values of a product list against pylogup.prove_round / fix_variables"""
    pl = _LG().ProdList(ctx, [cozk.Vec.from_ints(ctx, p) for p in polys_ref], products)
    degree = max(len(f) for _, f in products)
    assert pl.degree == degree
    ref, r = polys_ref, None
    for _ in range(len(polys_ref[0]).bit_length() - 1):
        if r is not None:
            ref = G.fix_variables(ref, r)
        assert pl.round(r) == G.prove_round(ref, products, degree)
        r = rng.field()
    assert pl.final(r) == [p[0] for p in G.fix_variables(ref, r)]
    pl.free()


PRODLIST_SHAPES = {
    "degree1": lambda c: [(c, [0]), (R - 1, [1]), (0, [2]), (1, [1])],
    "degree2": lambda c: [(1, [0, 0]), (c, [0, 1]), (R - 1, [2]), (0, [1, 2])],
    "degree4": lambda c: [(1, [0, 0, 0, 0]), (c, [0, 1, 2, 3]), (R - 1, [1, 1]), (0, [3]), (c, [2, 3, 3])],
}


@pytest.mark.parametrize("nv", [1, 10, 11])
@pytest.mark.parametrize("shape", list(PRODLIST_SHAPES))
def test_prodlist_degrees_1_2_4_repeated_factors_and_edge_coefficients(cozk, ctx, shape, nv):
    """max_multiplicands 1, 2 and 4 (2, 3 and 5 evaluations per round), a polynomial twice and four times in one product, the
    coefficients 0, 1 and r - 1; 2 and 4 workgroups in the first round (half = 512, 1024), and one variable (n = 2: one round, then
    final)"""
    rng = O.SplitMix64(nv * 7 + len(shape))
    products = PRODLIST_SHAPES[shape](rng.field())
    _prodlist_all_rounds(cozk, ctx, [_rand(rng, 1 << nv, "plain") for _ in range(4)], products, rng)


def test_prodlist_at_its_limits_48_polynomials_32_products(cozk, ctx):
    """exactly PL_MAX_POLYS = 48 polynomials and PL_MAX_TERMS = 32 products of 1 to PL_MAX_FACTORS = 4 factors that reach every
    polynomial, index 47 included"""
    rng = O.SplitMix64(4832)
    counts = [1 + q % PL_MAX_FACTORS for q in range(PL_MAX_TERMS)]  # 80 factor slots, dealt round the 48 polynomials in turn
    firsts = [sum(counts[:q]) for q in range(PL_MAX_TERMS)]
    products = [([0, 1, R - 1, rng.field()][q % 4], [(firsts[q] + j) % PL_MAX_POLYS for j in range(counts[q])]) for q in range(PL_MAX_TERMS)]
    assert {j for _, f in products for j in f} == set(range(PL_MAX_POLYS))
    _prodlist_all_rounds(cozk, ctx, [_rand(rng, 64, "plain") for _ in range(PL_MAX_POLYS)], products, rng)


def test_prodlist_two_terms_per_lane_all_20_rounds(cozk, ctx):
    """cap: ROUND_GRID_MAX = 1024 workgroups x 256 lanes = 262144 lanes; 2^20 elements are half = 2^19 pairs, two terms in every lane
    of round 0 (round 1 fills the capped grid exactly, the later ones shrink it).  All 20 rounds and the final values follow the
    device's own fix_variables."""
    n = 1 << 20
    assert n // 2 == 2 * ROUND_GRID_MAX * PT
    rng = O.SplitMix64(2020)
    tables = [(_pattern(rng, "plain"), n) for _ in range(3)]
    products = [(1, [0, 1, 2]), (R - 1, [0, 0]), (rng.field(), [2]), (0, [1])]
    pl = _LG().ProdList(ctx, [S.tiled_values(ctx, cozk, p, n) for p, _ in tables], products)
    r = None
    for _ in range(20):
        if r is not None:
            tables = [S.bind(t, r, O.LOW_TO_HIGH) for t in tables]
        assert pl.round(r) == S.prodlist_round(tables, products, 3)
        r = rng.field()
    tables = [S.bind(t, r, O.LOW_TO_HIGH) for t in tables]
    assert [n1 for _, n1 in tables] == [1, 1, 1]
    assert pl.final(r) == [p[0] for p, _ in tables]
    pl.free()


def test_prodlist_refusals_leave_the_context_usable(cozk, ctx):
    """every refusal of cozk_prodlist_create / _round / _final is COZK_ERR_INVALID_ARG, and a good call follows each"""
    LG = _LG()
    rng = O.SplitMix64(99)
    ref = [_rand(rng, 4, "plain") for _ in range(2)]
    vecs = [cozk.Vec.from_ints(ctx, p) for p in ref]
    good = [(rng.field(), [0, 1]), (1, [1])]

    def refused(polys, products):
        with pytest.raises(cozk.CozkError) as e:
            LG.ProdList(ctx, polys, products)
        assert e.value.code == ERR_INVALID_ARG
        pl = LG.ProdList(ctx, vecs, good)  # the context still works
        assert pl.round() == G.prove_round(ref, good, 2)
        pl.free()

    refused([vecs[0]] * (PL_MAX_POLYS + 1), good)
    refused(vecs, [(1, [0])] * (PL_MAX_TERMS + 1))
    refused(vecs, [(1, [0, 1, 0, 1, 0])])
    refused(vecs, [(1, [0]), (1, [])])
    refused(vecs, [(1, [0, -1])])
    refused(vecs, [(1, [0, len(vecs)])])
    refused([cozk.Vec.from_ints(ctx, [1, 2, 3, 4, 5, 6])] * 2, good)
    refused([vecs[0], cozk.Vec.from_ints(ctx, [1, 2])], good)
    refused([vecs[0], cozk.Vec.from_ints(ctx, list(range(8)))], good)

    def refused_call(call):
        with pytest.raises(cozk.CozkError) as e:
            call()
        assert e.value.code == ERR_INVALID_ARG
        return str(e.value)

    # final with two variables left, then the same object goes through its rounds
    pl = LG.ProdList(ctx, vecs, good)
    refused_call(lambda: pl.final(rng.field()))
    assert pl.round() == G.prove_round(ref, good, 2)
    r = rng.field()
    ref1 = G.fix_variables(ref, r)
    assert pl.round(r) == G.prove_round(ref1, good, 2)
    r = rng.field()
    finals = [p[0] for p in G.fix_variables(ref1, r)]
    # one variable left: its randomness belongs to final; a round with it is refused and leaves the list to the final below
    assert "prodlist_round: nothing left to sum after this fix" in refused_call(lambda: pl.round(r))
    assert pl.final(r) == finals
    # fully fixed: no round with a challenge, none without, no second final; the context goes on
    assert "prodlist_round: fully fixed" in refused_call(lambda: pl.round(rng.field()))
    assert "prodlist_round: no variable left" in refused_call(lambda: pl.round())
    assert "prodlist_final: one variable must be left" in refused_call(lambda: pl.final(rng.field()))
    pl.free()
    pl = LG.ProdList(ctx, vecs, good)
    assert pl.round() == G.prove_round(ref, good, 2)
    pl.free()


# ------------------------------------------------------------------------------------------------ k_sparse_matvec3 and its long-row queue
def _u32(cozk, ctx, arr):
    return cozk.Vec.from_numpy(ctx, np.asarray(arr, dtype=np.uint32), cozk.SCALAR_U32)


def _check_csr(row_ptr, col, ncols):
    """the preconditions of cozk_sparse_matvec3 (not checked on the device): every column in range, row_ptr monotone from 0 to nnz"""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    assert row_ptr[0] == 0 and row_ptr[-1] == len(col) and np.all(np.diff(row_ptr) >= 0)
    assert len(col) == 0 or (col.min() >= 0 and col.max() < ncols)
    assert len(col) < 1 << 32


@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_sparse_matvec_short_and_long_rows_in_one_matrix(cozk, ctx, mode):
    """rows of 0, 1, SPMV_LONG = 64 (the last one-lane row) and 65 (the first queued row) entries, of SPMV_CHUNK - 1 = 2047, 2048
    (one full item), 2049 (a one-entry second item) and 4097 (three items) entries; a long row first, a long row last, empty rows
    between; random values and columns"""
    counts = [65, 0, 1, 64, 0, 0, 2047, 2048, 2049, 0, 4097, 3, 0, 65]
    assert counts[0] == SPMV_LONG + 1 == counts[-1] and {0, 1, SPMV_LONG, SPMV_CHUNK - 1, SPMV_CHUNK, SPMV_CHUNK + 1, 2 * SPMV_CHUNK + 1} <= set(counts)
    rng = O.SplitMix64(640 + (mode == "plain"))
    ncols = 37
    z = _rand(rng, ncols, mode)
    row_ptr = [0]
    for k in counts:
        row_ptr.append(row_ptr[-1] + k)
    nnz = row_ptr[-1]
    col = [rng.next() % ncols for _ in range(nnz)]
    vals = [[rng.field() for _ in range(nnz)], [rng.field() % 7 for _ in range(nnz)], [rng.field() for _ in range(nnz)]]
    _check_csr(row_ptr, col, ncols)
    rows = [r for r, k in enumerate(counts) for _ in range(k)]
    out = cozk.sparse_matvec3(_u32(cozk, ctx, row_ptr), _u32(cozk, ctx, col), *[cozk.Vec.from_ints(ctx, v) for v in vals], _new(cozk, ctx, z))
    for o, v in zip(out, vals):
        assert o.coeffs() == O.sparse_matvec(list(zip(rows, col, v)), z, len(counts))


def _sparse_periodic(cozk, ctx, mode, row_ptr, seed):
    """a matrix with col[e] = e % ncols and periodic values against S.sparse_row_sums, the three outputs one by one"""
    rng = O.SplitMix64(seed + (mode == "plain"))
    ncols = 8
    z = _rand(rng, ncols, mode)
    nnz = int(row_ptr[-1])
    col = (np.arange(nnz, dtype=np.int64) % ncols).astype(np.uint32)
    _check_csr(row_ptr, col, ncols)
    pats = [_pattern(rng, "plain") for _ in range(3)]
    out = cozk.sparse_matvec3(_u32(cozk, ctx, row_ptr), _u32(cozk, ctx, col), *[S.tiled_values(ctx, cozk, p, nnz) for p in pats], _new(cozk, ctx, z))
    ptr = [int(x) for x in row_ptr]
    for o, p in zip(out, pats):
        assert o.coeffs() == S.sparse_row_sums(p, z, ptr)


@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_sparse_matvec_more_long_rows_and_items_than_workgroups(cozk, ctx, mode):
    """caps: g_rows = 1024 workgroups of k_sparse_matvec3_rows and g_items = 4096 of k_sparse_matvec3_items; 4100 rows of
    SPMV_LONG + 1 = 65 entries are 4100 long rows (workgroups 0..3 take five rows, the others four) and 4100 one-chunk items (workgroups
    0..3 take two).  The host's queue bound is max_rows = nnz / 64 + 1 = 4165 for these 4100: the closest a matrix comes to it."""
    nrows, per = 4100, SPMV_LONG + 1
    assert nrows > G_ITEMS > G_ROWS and nrows <= nrows * per // SPMV_LONG + 1
    _sparse_periodic(cozk, ctx, mode, np.arange(nrows + 1, dtype=np.int64) * per, 4100)


@pytest.mark.parametrize("mode", ["rep3", "plain"])
def test_sparse_matvec_one_row_of_more_items_than_lanes(cozk, ctx, mode):
    """cap: the PT = 256 lanes of the one workgroup that k_sparse_matvec3_rows gives a long row; 256 x SPMV_CHUNK + 1 = 524289 entries
    are 257 items, so lane 0 adds two partial sums (the last item holds a single entry)"""
    nnz = PT * SPMV_CHUNK + 1
    assert (nnz + SPMV_CHUNK - 1) // SPMV_CHUNK == PT + 1
    _sparse_periodic(cozk, ctx, mode, np.array([0, nnz], dtype=np.int64), 257)


# ------------------------------------------------------------------------------------------------ k_poly_batch_dot_public
def _batch_dot_periodic(cozk, ctx, n, fill, nq):
    """two Rep3 polynomials and a plain one times nq public vectors, all periodic raw residues (hence RINV^2, as in test_gpu_poly.py)"""
    P = importlib.import_module("co-zkvms_amd.poly")
    ins = [S.wide_inputs(fill, "rep3", 31, False), S.wide_inputs(fill, "rep3", 41, False), S.wide_inputs(fill, "plain", 51, False)]
    pubs = [ins[0][2], ins[1][2][7:] + ins[1][2][:7]][:nq]
    polys = [S.wide_poly(cozk, ctx, a, b, n) for a, b, _ in ins]
    got = P.batch_dot_public(polys, [S.tiled(ctx, cozk, p, n) for p in pubs])
    dot = lambda v, pub: S.tiled_dot(n, v, pub) * X.RINV * X.RINV % R
    assert got == [[(dot(a, pub), dot(b, pub) if b is not None else 0) for pub in pubs] for a, b, _ in ins]
    if fill == "all_r_minus_1":
        assert S.tiled_dot(n, ins[0][0], pubs[0]) == n * (R - 1) ** 2  # the closed form


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("fill", ["all_r_minus_1", "mixed"])
def test_batch_dot_public_many_worst_case_terms_per_lane(cozk, ctx, fill, nq):
    """cap: EVAL_GRID_MAX = 192 workgroups x 256 lanes = 49152 lanes; 2^21 elements are 42 or 43 terms per lane, past the 28 worst-case
    terms from which the third word of a FrWide is non-zero (poly.hip.hpp), in up to four accumulators per lane (a and b times two
    public vectors); the plain polynomial's row keeps its b slots at zero"""
    n = 1 << 21
    assert n // (EVAL_GRID_MAX * PT) == 42 and n % (EVAL_GRID_MAX * PT) != 0
    _batch_dot_periodic(cozk, ctx, n, fill, nq)


@pytest.mark.parametrize("nq", [1, 2])
def test_batch_dot_public_first_stride(cozk, ctx, nq):
    """cap: EVAL_GRID_MAX x 256 = 49152 lanes; n = 49153 gives lane 0 of workgroup 0 its second term and no other lane one"""
    _batch_dot_periodic(cozk, ctx, EVAL_GRID_MAX * PT + 1, "mixed", nq)


def test_batch_dot_public_130_polynomials_520_result_rows(cozk, ctx):
    """k = 130 polynomials (Rep3 and plain alternating) x 2 public vectors at n = 300, no multiple of the block: a pointer table of
    260 entries, 130 rows of workgroups and 520 partial rows for k_finish_sums"""
    P = importlib.import_module("co-zkvms_amd.poly")
    rng = O.SplitMix64(130)
    n, k = 300, 130
    cols = [_rand(rng, n, "rep3" if i % 2 == 0 else "plain") for i in range(k)]
    pubs = [_rand(rng, n, "plain") for _ in range(2)]
    got = P.batch_dot_public([_new(cozk, ctx, c) for c in cols], [cozk.Vec.from_ints(ctx, p) for p in pubs])
    assert len(got) == k
    for c, g in zip(cols, got):
        if isinstance(c[0], tuple):
            want = [(sum(x[0] * w for x, w in zip(c, p)) % R, sum(x[1] * w for x, w in zip(c, p)) % R) for p in pubs]
        else:
            want = [(sum(x * w for x, w in zip(c, p)) % R, 0) for p in pubs]
        assert g == want


# ------------------------------------------------------------------------------------------------ k_logup_h, k_boost_degree, k_vec_gather
@pytest.mark.parametrize("with_m", [True, False])
def test_logup_h_zero_denominator_gives_zero(cozk, ctx, with_m):
    """values (-x) mod r at the first, a middle and the last index make phi = 0 there; ark_ff::batch_inversion leaves a zero in
    place, so h = 0 there (Fr::inv(0) = 0), with multiplicities and without; 777 elements: three full workgroups and a ragged one"""
    rng = O.SplitMix64(777 + with_m)
    n = 777
    x = rng.field()
    vals = [rng.field() for _ in range(n)]
    zeros = (0, 300, n - 1)
    for i in zeros:
        vals[i] = (-x) % R
    m = [1 + rng.next() % 5 for _ in range(n)] if with_m else None
    phi, h = _LG().logup_h(ctx, cozk.Vec.from_ints(ctx, vals), cozk.Vec.from_ints(ctx, m) if with_m else None, x)
    want_phi = [(x + t) % R for t in vals]
    assert [i for i, p in enumerate(want_phi) if p == 0] == list(zeros)
    inv = [pow(p, -1, R) if p else 0 for p in want_phi]
    assert phi.to_ints() == want_phi
    assert h.to_ints() == ([mv * iv % R for mv, iv in zip(m, inv)] if with_m else inv)


def test_boost_degree_one_element_and_unchanged_dimension(cozk, ctx):
    LG = _LG()
    rng = O.SplitMix64(12)
    v = rng.field()
    one = cozk.Vec.from_ints(ctx, [v])
    assert LG.boost_degree(ctx, one, 0).to_ints() == [v] == G.boost_degree([v], 0)
    assert LG.boost_degree(ctx, one, 4).to_ints() == G.boost_degree([v], 4)
    g = [rng.field() for _ in range(512)]
    gv = cozk.Vec.from_ints(ctx, g)
    assert LG.boost_degree(ctx, gv, 9).to_ints() == g
    assert LG.boost_degree(ctx, gv, 11).to_ints() == G.boost_degree(g, 11)


def test_gather_index_equal_to_the_source_length_gives_zero(cozk, ctx):
    """k_vec_gather defines every index >= len(src) as "no entry": 0, like the 0xffffffff marker and the padding"""
    rng = O.SplitMix64(13)
    src = [rng.field() for _ in range(300)]
    idx = [0, len(src), len(src) - 1, 0xFFFFFFFF, len(src), 7]
    got = _LG().gather(ctx, idx, cozk.Vec.from_ints(ctx, src), 8).to_ints()
    assert got == [src[0], 0, src[-1], 0, 0, src[7], 0, 0]


# ------------------------------------------------------------------------------------------------ null first entries
def test_null_first_polynomial_is_refused_not_dereferenced(cozk, ctx):
    """cozk_prodlist_create, cozk_poly_batch_dot_public, cozk_prod_sumcheck_evals and cozk_open_quadratic_evals with polys[0] = NULL
    return COZK_ERR_INVALID_ARG, and the context serves the same call with its polynomial in place"""
    LG = _LG()
    l = LG._decl()
    rng = O.SplitMix64(5)
    n = 8
    a, e = _rand(rng, n, "rep3"), _rand(rng, n, "plain")
    pa, pe = _new(cozk, ctx, a), _new(cozk, ctx, e)
    va, ve = cozk.Vec.from_ints(ctx, [s[0] for s in a]), cozk.Vec.from_ints(ctx, e)
    out = np.zeros((16, 4), dtype=np.uint64)
    vp = ctypes.c_void_p

    assert l.cozk_prod_sumcheck_evals(ctx.h, (vp * 2)(None, pe.h), 2, 2, out.ctypes.data) == ERR_INVALID_ARG
    assert cozk.prod_sumcheck_evals([pa, pe], 2) == O.prod_round_evals([a, e], 2)

    assert l.cozk_open_quadratic_evals(ctx.h, (vp * 2)(None, pa.h), (vp * 2)(pe.h, pe.h), 2, out.ctypes.data) == ERR_INVALID_ARG
    assert len(cozk.open_quadratic_evals([pa, pa], [pe, pe])) == 2

    assert l.cozk_poly_batch_dot_public(ctx.h, (vp * 2)(None, pa.h), 2, (vp * 1)(ve.h), 1, out.ctypes.data) == ERR_INVALID_ARG
    P = importlib.import_module("co-zkvms_amd.poly")
    assert P.batch_dot_public([pa], [ve]) == [[O.dense_dot_product_with_public(a, e)]]

    coefs = cozk.fr_to_mont_limbs([1])
    h = vp()
    rc = l.cozk_prodlist_create(ctx.h, (vp * 2)(None, va.h), 2, coefs.ctypes.data, (ctypes.c_int * 1)(2), (ctypes.c_int * 2)(0, 1), 1, ctypes.byref(h))
    assert rc == ERR_INVALID_ARG and not h
    pl = LG.ProdList(ctx, [va, ve], [(1, [0, 1])])
    assert pl.round() == G.prove_round([[s[0] for s in a], e], [(1, [0, 1])], 2)
    pl.free()
