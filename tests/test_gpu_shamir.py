"""GPU parity of the Shamir seam (cozk_shamir_*, cozk_vec_add_scalar) against the big-int restatement of
mpc-types/src/protocols/shamir.rs (tests/shamir_ref.py).  Bar: bit-exact; calls go through the C ABI (ctypes).
No test provokes a device fault: every bad argument is rejected on the host before any launch."""
import ctypes

import numpy as np
import pytest

import prims_harness as H
import pyref as O
import reduction_ref as X
import shamir_ref as S

pytestmark = pytest.mark.gpu

R = O.R
RINV = pow(1 << 256, -1, R)
# the issue's edge operands, and the canonical values whose MONTGOMERY residues (what the Horner chain multiplies) are
# r - 1, r - 2, 1 and 2^253 - 1
EDGE = [0, 1, 2, R - 1, R - 2, O.R_MONT_ONE, (1 << 253) + 12345, (1 << 253) - 1]
EDGE_MONT = [(R - 1) * RINV % R, (R - 2) * RINV % R, RINV, ((1 << 253) - 1) * RINV % R]


def _secrets(seed, n):
    e = [0, 1, R - 1, R - 2] + EDGE_MONT
    return (e + O.synthetic_fr(seed, max(n - len(e), 0)))[:n]


def _ints(vecs):
    return [v.to_ints() for v in vecs]


# ------------------------------------------------------------------------------------------------ (a) share
@pytest.mark.parametrize("counter", [0, (1 << 33) + 7])
@pytest.mark.parametrize("parties,degree,n", [(p, d, n) for p, d in ((3, 1), (10, 6), (8, 2)) for n in (0, 1, 257, 1000)] +
                         [(32, 15, 257), (32, 1, 257)])
def test_share_vec_matches_restatement(cozk, ctx, parties, degree, n, counter):
    v = _secrets(100 + parties + n, n)
    keys = S.keys_for(7 * parties + degree, degree)
    got = cozk.Vec.from_ints(ctx, v).shamir_share(keys, degree, parties, counter=counter)
    assert len(got) == parties and all(len(g) == n for g in got)
    assert _ints(got) == S.share_vec(v, keys, degree, parties, counter=counter)  # every party's vector


# ------------------------------------------------------------------------------------------------ (b) combine
@pytest.mark.parametrize("parties,degree", [(3, 1), (10, 6), (8, 2), (32, 15)])
def test_combine_vec_opens_the_secret(cozk, ctx, parties, degree):
    n = 300
    v = _secrets(200 + parties, n)
    sh = cozk.Vec.from_ints(ctx, v).shamir_share(S.keys_for(3 + degree, degree), degree, parties, counter=11)
    first = list(range(1, degree + 2))
    assert cozk.shamir_combine([sh[p - 1] for p in first], first, degree).to_ints() == v
    scattered = [parties - 2 * i if parties - 2 * i > 0 else 2 * i - parties + 1 for i in range(degree + 1)]
    scattered = sorted(set(scattered), key=scattered.index)
    if len(scattered) < degree + 1:
        scattered = list(range(parties, parties - degree - 1, -1))
    assert cozk.shamir_combine([sh[p - 1] for p in scattered], scattered, degree).to_ints() == v
    # k > degree + 1 shares: the first degree + 1 are used (combine_field_elements); garbage behind them must not matter
    allp = list(range(parties, 0, -1))
    vecs = [sh[p - 1] for p in allp]
    if parties > degree + 1:
        vecs[-1] = cozk.Vec.random(ctx, n, seed=5)
    assert cozk.shamir_combine(vecs, allp, degree).to_ints() == v
    assert cozk.shamir_combine([cozk.Vec.from_ints(ctx, [])] * 2, [1, 2], 1).to_ints() == []


# ------------------------------------------------------------------------------------------------ (c) edge operands
@pytest.mark.parametrize("degree", [1, 2, 7, 8, 15])
def test_eval_edge_operands_every_position_every_party(cozk, ctx, degree):
    """drives the edge operands through the small-multiplier reduction (fr_mul_small_add) at every p <= 32, in every
    coefficient position, through the templated (1..7) and the looped (8..15) kernel variant"""
    edge = EDGE + EDGE_MONT
    m = len(edge)
    rng = O.SplitMix64(77 + degree)
    cols = [[] for _ in range(degree + 1)]
    for pos in range(degree + 1):  # block 1: `e` at `pos`, r - 1 everywhere else; block 2: `e` at pos, random elsewhere
        for e in edge:
            for c in range(degree + 1):
                cols[c].append(e if c == pos else R - 1)
        for e in edge:
            for c in range(degree + 1):
                cols[c].append(e if c == pos else rng.field())
    for e in edge:  # the same operand in every position
        for c in range(degree + 1):
            cols[c].append(e)
    for k in range(m):  # rotations of the edge set across the positions
        for c in range(degree + 1):
            cols[c].append(edge[(k + c) % m])
    got = cozk.shamir_eval(ctx, [cozk.Vec.from_ints(ctx, c) for c in cols], 32)
    want = S.eval_vec(cols, 32)
    for p in range(32):
        assert got[p].to_ints() == want[p], "party %d" % p
    raw = np.concatenate([g.to_numpy() for g in got])  # canonical limbs: below r as 256-bit integers
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


# ------------------------------------------------------------------------------------------------ (c') the quotient estimate
# Horner with a plain evaluation point is linear, so raw Montgomery residues go in (Vec.from_numpy) and the expectation is
# S.eval_vec of the residues themselves; the raw words that come out are compared as they are, so every output is canonical.
def _assert_canonical(raw):
    """raw limbs (k x 4 u64) are below r as 256-bit integers"""
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


def _eval_raw(cozk, ctx, cols, parties=32):
    """cozk_shamir_eval_vec on residue columns cols[c][lane] -> (got, want)[party][lane], raw"""
    out = cozk.shamir_eval(ctx, [cozk.Vec.from_numpy(ctx, X.to_raw(c)) for c in cols], parties)
    raw = [g.to_numpy() for g in out]
    _assert_canonical(np.concatenate(raw))
    return [X.from_raw(r) for r in raw], S.eval_vec(cols, parties)


def test_eval_small_multiplier_at_the_quotient_estimate_bound(cozk, ctx):
    """bound: q = T / D is floor(t / r) or one less, one subtraction finishes (shamir.hip:14-20): t = a p + c on every multiple of
    r a p <= 32 reaches, either side of it and of the delta where the estimate switches; the lane's own party p sits on it"""
    cases = X.small_mul_add_cases()
    got, want = _eval_raw(cozk, ctx, [[c for _, _, _, c in cases], [a for _, _, a, _ in cases]])
    for party in range(32):
        assert got[party] == want[party], "party %d" % party
    for lane, (p, _, a, c) in enumerate(cases):  # what the directed lanes are for
        assert got[p - 1][lane] == (a * p + c) % R


@pytest.mark.parametrize("degree", [2, 7, 8, 15])
def test_eval_quotient_estimate_bound_first_and_last_horner_step(cozk, ctx, degree):
    """bound: as above (shamir.hip:14-20), in the unrolled (2, 7) and the rolled (8, 15) kernel: (a, c) as the two leading
    coefficients (the first Horner step, whatever follows) and as coef_1 and the secret under zero coefficients (the last)"""
    cases = X.small_mul_add_cases(X.small_boundary_deltas)
    m = len(cases)
    cols = [[0] * (2 * m) for _ in range(degree + 1)]
    for lane, (_, _, a, c) in enumerate(cases):
        cols[degree][lane], cols[degree - 1][lane] = a, c
        cols[1][m + lane], cols[0][m + lane] = a, c
    got, want = _eval_raw(cozk, ctx, cols)
    for party in range(32):
        assert got[party] == want[party], "party %d" % party
    for lane, (p, _, a, c) in enumerate(cases):
        assert got[p - 1][m + lane] == (a * p + c) % R


def test_eval_limb_carry_operands(cozk, ctx):
    """bound: the 8 multiply-adds' carries m < 2^38 (shamir.hip:26): every pair of the primitive harness' edge residues, among
    them low limbs all ones (which EDGE lacks), as (a, c) at degree 1 for all 32 multipliers"""
    e = H.edges(R)
    got, want = _eval_raw(cozk, ctx, [[c for _ in e for c in e], [a for a in e for _ in e]])
    for party in range(32):
        assert got[party] == want[party], "party %d" % party


def test_combine_31_shares_of_r_minus_1(cozk, ctx):
    """bound: the wide accumulator's words T0 + T1 R + T2 R^2 (poly.hip.hpp:84-90) in k_shamir_combine: 31 terms lambda_j s_j with
    every share the residue r - 1, at degree 30, more than one block and a ragged tail"""
    n, pts = 300, list(range(1, 32))
    share = X.to_raw([R - 1] * n)
    got = cozk.shamir_combine([cozk.Vec.from_numpy(ctx, share) for _ in pts], pts, 30).to_numpy()
    lam = S.lagrange_from_coeff(pts)
    assert X.from_raw(got) == [sum(l * (R - 1) for l in lam) % R] * n  # lambda_j R * s_j / R: the residue of the sum
    rev = list(range(32, 1, -1))  # the same shares at other points: other coefficients
    got = cozk.shamir_combine([cozk.Vec.from_numpy(ctx, share) for _ in rev], rev, 30).to_numpy()
    assert X.from_raw(got) == [sum(l * (R - 1) for l in S.lagrange_from_coeff(rev)) % R] * n


# ------------------------------------------------------------------------------------------------ (d) local operators
def test_local_operators_then_combine(cozk, ctx):
    parties, degree, n = 8, 2, 200
    a, b = _secrets(1, n), list(reversed(_secrets(2, n)))
    sa = cozk.Vec.from_ints(ctx, a).shamir_share(S.keys_for(1, degree), degree, parties)
    sb = cozk.Vec.from_ints(ctx, b).shamir_share(S.keys_for(2, degree), degree, parties, counter=n)
    pts = [7, 2, 5]
    pub, k = R - 3, (1 << 200) + 9
    for op, f in ((cozk.OP_ADD, lambda x, y: (x + y) % R), (cozk.OP_SUB, lambda x, y: (x - y) % R)):
        out = [sa[p - 1].binop(op, sb[p - 1]) for p in pts]
        assert cozk.shamir_combine(out, pts, degree).to_ints() == [f(x, y) for x, y in zip(a, b)]
    out = [sa[p - 1].binop(cozk.OP_ADD, sb[p - 1]).add_scalar(pub).scale(k) for p in pts]  # (a + b + pub) * k
    assert cozk.shamir_combine(out, pts, degree).to_ints() == [(x + y + pub) * k % R for x, y in zip(a, b)]
    neg = [sa[p - 1].binop(cozk.OP_ADD, cozk.Vec.from_ints(ctx, [0] * n)).scale(R - 1) for p in pts]
    assert cozk.shamir_combine(neg, pts, degree).to_ints() == [(-x) % R for x in a]
    e = cozk.Vec.from_ints(ctx, EDGE + EDGE_MONT)
    for s in EDGE:
        assert cozk.Vec.from_ints(ctx, EDGE + EDGE_MONT).add_scalar(s).to_ints() == [(x + s) % R for x in EDGE + EDGE_MONT]
    assert e.add_scalar(0).to_ints() == EDGE + EDGE_MONT


@pytest.mark.parametrize("parties,degree,pts", [(8, 2, [6, 1, 8, 3, 4]), (32, 15, [32 - i for i in range(31)])])
def test_share_times_share_opens_with_twice_the_degree(cozk, ctx, parties, degree, pts):
    n = 128
    a, b = _secrets(11, n), list(reversed(_secrets(12, n)))
    sa = cozk.Vec.from_ints(ctx, a).shamir_share(S.keys_for(21, degree), degree, parties)
    sb = cozk.Vec.from_ints(ctx, b).shamir_share(S.keys_for(22, degree), degree, parties)
    prod = [sa[p - 1].binop(cozk.OP_MUL, sb[p - 1]) for p in pts]
    want = [x * y % R for x, y in zip(a, b)]
    assert cozk.shamir_combine(prod, pts, 2 * degree).to_ints() == want
    low = cozk.shamir_combine(prod, pts, degree).to_ints()  # degree + 1 shares do not open a product
    assert sum(x != y for x, y in zip(low, want)) >= n // 2


# ------------------------------------------------------------------------------------------------ (e) commitments
@pytest.mark.parametrize("parties,degree", [(3, 1), (8, 2)])
def test_commitments_of_shares_open_to_the_commitment_of_the_secret(cozk, ctx, parties, degree):
    """test_shamir_field_to_point (shamir.rs:493-519) at vector scale: MSM is linear, so Lagrange on the parties' MSMs opens
    the MSM of the secret vector"""
    n = 256
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, n, seed=606))
    V = cozk.Vec.random(ctx, n, seed=707)
    sh = V.shamir_share(S.keys_for(9, degree), degree, parties, counter=1)
    commits = [B.msm(s) for s in sh]
    want = B.msm(V)
    assert want is not None
    for pts in (list(range(1, degree + 2)), list(range(parties, parties - degree - 1, -1)), list(range(parties, 0, -1))):
        assert cozk.shamir_combine_points(ctx, [commits[p - 1] for p in pts], pts, degree) == want
    # the big-int route for one subset
    pts = list(range(1, degree + 2))
    lam = S.lagrange_from_coeff(pts)
    acc = None
    for p, l in zip(pts, lam):
        acc = O.g1_add(acc, O.g1_mul(commits[p - 1], l))
    assert acc == want
    # an infinity share point is accepted: the all-zero polynomial's shares commit to the identity
    zero = cozk.Vec.from_ints(ctx, [0] * n)
    zs = cozk.shamir_eval(ctx, [zero] * (degree + 1), parties)
    zc = [B.msm(s) for s in zs]
    assert zc[0] is None
    assert cozk.shamir_combine_points(ctx, zc[:degree + 1], pts, degree) is None
    mixed = [None] + [commits[p - 1] for p in pts[1:]]
    acc = None
    for pt, l in zip(mixed, lam):
        acc = O.g1_add(acc, O.g1_mul(pt, l))
    assert cozk.shamir_combine_points(ctx, mixed, pts, degree) == acc


# ------------------------------------------------------------------------------------------------ (f) scatter
def test_scatter_onto_other_contexts(cozk, ctx):
    parties, degree, n = 8, 2, 1000
    v = _secrets(808, n)
    V = cozk.Vec.from_ints(ctx, v)
    keys = S.keys_for(61, degree)
    want = S.share_vec(v, keys, degree, parties, counter=4)
    pcs = [cozk.Context(0) for _ in range(2)]
    party_ctxs = [pcs[p % 2] for p in range(parties)]
    got = V.shamir_scatter(keys, degree, party_ctxs, counter=4)
    for p in range(parties):
        assert got[p].ctx is party_ctxs[p]
        assert got[p].to_ints() == want[p]
        assert got[p].binop(cozk.OP_ADD, got[p]).to_ints() == [2 * x % R for x in want[p]]  # the party computes on it at once
    assert _ints(V.shamir_share(keys, degree, parties, counter=4)) == want
    for g in got:
        g.free()
    for c in pcs:
        c.close()


def test_scatter_orders_against_the_party_stream(cozk, ctx):
    """as test_rep3_scatter_orders_against_the_party_stream: a block the party freed a moment ago may still be read by kernels
    queued on the party's stream; the dealer's stream must not overwrite it early"""
    n = 1 << 20
    party_ctx = cozk.Context(0)
    X = cozk.Vec.random(party_ctx, n, seed=4242)
    acc = X.binop(cozk.OP_ADD, X)
    for _ in range(8):
        nxt = acc.binop(cozk.OP_ADD, X)
        acc.free()
        acc = nxt
    X.free()
    V = cozk.Vec.random(ctx, n, seed=77)
    keys = S.keys_for(63, 1)
    got = V.shamir_scatter(keys, 1, [party_ctx] * 3)
    want = cozk.Vec.random(party_ctx, n, seed=4242).to_ints()
    res = acc.to_ints()
    assert res[:64] == [10 * x % R for x in want[:64]] and res[-64:] == [10 * x % R for x in want[-64:]]
    exp = V.shamir_share(keys, 1, 3)
    for g, e in zip(got, exp):
        assert g.to_ints()[:32] == e.to_ints()[:32] and g.to_ints()[-32:] == e.to_ints()[-32:]
    party_ctx.close()


def test_scatter_peer_copy_two_gpus(cozk, ctx):
    """the hipMemcpyPeer leg of cozk_shamir_scatter (dealer on GPU 0, odd parties on GPU 1)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    n = 1 << 16
    V = cozk.Vec.random(ctx, n, seed=31)
    keys = S.keys_for(71, 2)
    other = cozk.Context(1)
    party_ctxs = [other if p % 2 else ctx for p in range(8)]
    got = V.shamir_scatter(keys, 2, party_ctxs, counter=7)
    exp = V.shamir_share(keys, 2, 8, counter=7)
    for p in range(8):
        assert got[p].ctx is party_ctxs[p] and got[p].to_ints() == exp[p].to_ints()
    for g in got:
        g.free()
    other.close()


# ------------------------------------------------------------------------------------------------ (g) production size
def test_share_multiply_combine_2p22(cozk, ctx):
    parties, degree, n = 8, 2, 1 << 22
    A, B = cozk.Vec.random(ctx, n, seed=1001), cozk.Vec.random(ctx, n, seed=1002)
    ka, kb = S.keys_for(81, degree), S.keys_for(82, degree)
    ctr = (1 << 40) + 3
    sa = A.shamir_share(ka, degree, parties, counter=ctr)
    sb = B.shamir_share(kb, degree, parties, counter=ctr)
    pts = [8, 3, 5, 1, 6]
    prod = [sa[p - 1].binop(cozk.OP_MUL, sb[p - 1]) for p in pts]
    got = cozk.shamir_combine(prod, pts, 2 * degree).to_numpy()
    want = A.binop(cozk.OP_MUL, B).to_numpy()
    assert np.array_equal(got, want)  # raw Montgomery limbs: canonical outputs are unique
    idx = list(range(0, n, n // 1024))[:1023] + [n - 1]
    a_np = A.to_numpy()
    secrets = cozk.mont_limbs_to_int(a_np[idx])
    coefs = [[O.prf_fr(k, ctr + i) for i in idx] for k in ka]
    for p in range(parties):
        sp = cozk.mont_limbs_to_int(sa[p].to_numpy()[idx])
        assert sp == [S.evaluate_poly([secrets[j]] + [c[j] for c in coefs], p + 1) for j in range(len(idx))], "party %d" % p


# ------------------------------------------------------------------------------------------------ (h) argument checks
def _expect_invalid(cozk, ctx, rc, text):
    assert rc == -1  # COZK_ERR_INVALID_ARG
    msg = cozk._lib.lib().cozk_last_error(ctx.h).decode()
    assert text in msg, msg


def test_argument_checks_leave_no_handle(cozk, ctx):
    l = cozk._lib.lib()
    V = cozk.Vec.from_ints(ctx, [1, 2, 3])
    U = cozk.Vec.from_ints(ctx, [1, 2, 3], kind=cozk.SCALAR_U32)
    W = cozk.Vec.from_ints(ctx, [1, 2])
    keys = b"".join(S.keys_for(1, 15))
    SENT = 0x5A5A
    def outs():
        return (ctypes.c_void_p * 40)(*([SENT] * 40))
    untouched_or_null = lambda o, k: all(o[i] in (None, SENT) for i in range(40)) and all(o[i] is None for i in range(k))
    # share / scatter / eval: degree and party ranges
    ctxs = (ctypes.c_void_p * 40)(*([ctx.h.value] * 40))
    vecs = (ctypes.c_void_p * 40)(*([V.h.value] * 40))
    for deg, np_, text in ((0, 3, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE"), (16, 32, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE"),
                           (2, 2, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES"), (1, 33, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES"),
                           (-1, 3, "1 <= degree")):
        o = outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_share_vec(ctx.h, V.h, keys, deg, np_, 0, o), "shamir_share_vec: " + text)
        assert untouched_or_null(o, np_ if 1 <= np_ <= 32 else 0)
        o = outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_scatter(ctx.h, V.h, keys, deg, np_, 0, ctxs, o), "shamir_scatter: " + text)
        assert untouched_or_null(o, np_ if 1 <= np_ <= 32 else 0)
        if 0 <= deg <= 16:
            o = outs()
            _expect_invalid(cozk, ctx, l.cozk_shamir_eval_vec(ctx.h, vecs, deg, np_, o), "shamir_eval_vec: " + text)
            assert untouched_or_null(o, np_ if 1 <= np_ <= 32 else 0)
    o = outs()
    _expect_invalid(cozk, ctx, l.cozk_shamir_share_vec(ctx.h, U.h, keys, 1, 3, 0, o), "must be an FR vector")
    assert untouched_or_null(o, 3)
    _expect_invalid(cozk, ctx, l.cozk_shamir_share_vec(ctx.h, None, keys, 1, 3, 0, outs()), "null argument")
    _expect_invalid(cozk, ctx, l.cozk_shamir_share_vec(ctx.h, V.h, None, 1, 3, 0, outs()), "null argument")
    _expect_invalid(cozk, ctx, l.cozk_shamir_share_vec(ctx.h, V.h, keys, 1, 3, 0, None), "null output")
    _expect_invalid(cozk, ctx, l.cozk_shamir_scatter(ctx.h, V.h, keys, 1, 3, 0, None, outs()), "null argument")
    nullctx = (ctypes.c_void_p * 3)(ctx.h.value, None, ctx.h.value)
    o = outs()
    _expect_invalid(cozk, ctx, l.cozk_shamir_scatter(ctx.h, V.h, keys, 1, 3, 0, nullctx, o), "null party context")
    assert untouched_or_null(o, 3)
    mixed = (ctypes.c_void_p * 3)(V.h.value, W.h.value, V.h.value)
    o = outs()
    _expect_invalid(cozk, ctx, l.cozk_shamir_eval_vec(ctx.h, mixed, 2, 3, o), "equal length")
    assert untouched_or_null(o, 3)
    mixed = (ctypes.c_void_p * 3)(V.h.value, U.h.value, V.h.value)
    _expect_invalid(cozk, ctx, l.cozk_shamir_eval_vec(ctx.h, mixed, 2, 3, outs()), "FR coefficient vectors")
    mixed = (ctypes.c_void_p * 3)(V.h.value, None, V.h.value)
    _expect_invalid(cozk, ctx, l.cozk_shamir_eval_vec(ctx.h, mixed, 2, 3, outs()), "FR coefficient vectors")

    # combines
    def pts(*p):
        return np.asarray(p, dtype=np.uint32)
    def combine(vs, p, k, deg):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_combine_vec(ctx.h, vs, p.ctypes.data if p is not None else None, k, deg, ctypes.byref(h))
        assert h.value is None
        return rc
    three = (ctypes.c_void_p * 3)(V.h.value, V.h.value, V.h.value)
    _expect_invalid(cozk, ctx, combine(three, pts(1, 2, 3), 3, 3), "0 <= degree < k")
    _expect_invalid(cozk, ctx, combine(three, pts(1, 2, 3), 3, -1), "0 <= degree < k")
    _expect_invalid(cozk, ctx, combine(three, pts(1, 2, 3), 0, 0), "1 <= k <= COZK_SHAMIR_MAX_PARTIES")
    _expect_invalid(cozk, ctx, combine(vecs, pts(*range(1, 34)), 33, 1), "1 <= k <= COZK_SHAMIR_MAX_PARTIES")
    _expect_invalid(cozk, ctx, combine(three, pts(1, 0, 3), 3, 1), "points must lie in 1..COZK_SHAMIR_MAX_PARTIES")
    _expect_invalid(cozk, ctx, combine(three, pts(1, 33, 3), 3, 1), "points must lie in 1..COZK_SHAMIR_MAX_PARTIES")
    _expect_invalid(cozk, ctx, combine(three, pts(1, 2, 1), 3, 1), "points must be distinct")
    _expect_invalid(cozk, ctx, combine(three, None, 3, 1), "null points")
    _expect_invalid(cozk, ctx, combine((ctypes.c_void_p * 3)(V.h.value, V.h.value, W.h.value), pts(1, 2, 3), 3, 1), "equal length")
    _expect_invalid(cozk, ctx, combine((ctypes.c_void_p * 3)(V.h.value, U.h.value, V.h.value), pts(1, 2, 3), 3, 1), "k FR share vectors")
    _expect_invalid(cozk, ctx, combine((ctypes.c_void_p * 3)(V.h.value, None, V.h.value), pts(1, 2, 3), 3, 1), "k FR share vectors")
    _expect_invalid(cozk, ctx, combine(None, pts(1, 2, 3), 3, 1), "null argument")
    _expect_invalid(cozk, ctx, l.cozk_shamir_combine_vec(ctx.h, three, pts(1, 2, 3).ctypes.data, 3, 1, None), "null output")

    xy = np.zeros((3, 8), dtype=np.uint64)
    inf = np.ones(3, dtype=np.int32)
    out = np.zeros(8, dtype=np.uint64)
    oi = ctypes.c_int()
    def cpoints(p, k, deg, xy_=xy, out_=out, oi_=ctypes.byref(oi)):
        return l.cozk_shamir_combine_points(ctx.h, xy_.ctypes.data if xy_ is not None else None, inf.ctypes.data,
                                            p.ctypes.data if p is not None else None, k, deg, out_.ctypes.data if out_ is not None else None, oi_)
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 3), 3, 3), "shamir_combine_points: 0 <= degree < k")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 3), 0, 0), "shamir_combine_points: 1 <= k")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 2), 3, 1), "points must be distinct")
    _expect_invalid(cozk, ctx, cpoints(pts(0, 2, 3), 3, 1), "points must lie in")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 40), 3, 1), "points must lie in")
    _expect_invalid(cozk, ctx, cpoints(None, 3, 1), "null points")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 3), 3, 1, xy_=None), "null argument")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 3), 3, 1, out_=None), "null argument")
    _expect_invalid(cozk, ctx, cpoints(pts(1, 2, 3), 3, 1, oi_=None), "null argument")
    assert cpoints(pts(1, 2, 3), 3, 1) == 0 and oi.value == 1  # three infinity shares open to infinity

    s = cozk.fr_to_mont_limbs([5])[0]
    _expect_invalid(cozk, ctx, l.cozk_vec_add_scalar(ctx.h, U.h, s.ctypes.data), "vec_add_scalar: bad argument")
    _expect_invalid(cozk, ctx, l.cozk_vec_add_scalar(ctx.h, V.h, None), "vec_add_scalar: bad argument")
    _expect_invalid(cozk, ctx, l.cozk_vec_add_scalar(ctx.h, None, s.ctypes.data), "vec_add_scalar: bad argument")
    assert V.to_ints() == [1, 2, 3]  # nothing ran
