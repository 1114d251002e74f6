"""GPU tests of the Shamir multiplication with a king and preprocessed double-random pairs (cozk_shamir_rand_{deal, extract,
inproc, vec}, cozk_shamir_mul_mask, cozk_shamir_mul_king_{inproc, vec}) against the big-int restatement tests/shamir_dn_ref.py.
Bar: bit-exact; calls go through the C ABI (ctypes).  No test provokes a device fault: every bad argument is rejected on the host
before any launch."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 - a torch host maps its own librccl first; libcozk then reuses that copy (one RCCL per process)

import pyref as O
import reduction_ref as X
import shamir_dn_ref as D
import shamir_mul_ref as M
import shamir_ref as S
from test_gpu_shamir import EDGE, EDGE_MONT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
NMAX = 1000
SHAPES = [(3, 1), (5, 2), (8, 2), (15, 7), (32, 7)]
LENGTHS = [0, 1, 257, 1000]


def _secrets(seed, n):
    e = [0, 1, R - 1, R - 2] + EDGE_MONT
    return (O.synthetic_fr(seed, max(n - len(e), 1)) + e)[:n]


def _ints(vecs):
    return [v.to_ints() for v in vecs]


def _assert_canonical(raw):
    """raw limbs (k x 4 u64) are below r as 256-bit integers"""
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


# ------------------------------------------------------------------------------------------------ (a) deal parity
def _deal_keys(degree):
    return S.keys_for(40 + degree, D.num_keys(degree))


@functools.lru_cache(maxsize=None)
def _streams(degree, counter):
    """the dealer's 3t + 1 PRF vectors at the longest length, computed once: a shorter deal uses their prefixes"""
    return [O.prf_fr_vec(k, counter, NMAX) for k in _deal_keys(degree)]


@pytest.mark.parametrize("counter", [0, (1 << 33) + 7])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("parties,degree", SHAPES)
def test_rand_deal_matches_eval_of_the_prf_streams(cozk, ctx, parties, degree, n, counter):
    got_t, got_2t = cozk.shamir_rand_deal(ctx, n, _deal_keys(degree), degree, parties, counter=counter)
    assert len(got_t) == len(got_2t) == parties and all(len(g) == n for g in got_t + got_2t)
    st = [s[:n] for s in _streams(degree, counter)]
    assert _ints(got_t) == S.eval_vec(st[:degree + 1], parties)
    assert _ints(got_2t) == S.eval_vec([st[0]] + st[degree + 1:], parties)
    # both open to the secret stream nobody stored, on the device
    lo = cozk.shamir_combine(got_t[:degree + 1], list(range(1, degree + 2)), degree)
    hi = cozk.shamir_combine(got_2t[:2 * degree + 1], list(range(1, 2 * degree + 2)), 2 * degree)
    assert np.array_equal(lo.to_numpy(), hi.to_numpy()) and lo.to_ints() == st[0]
    if n == 257 and counter == 0:
        u, w = D.rand_deal(_deal_keys(degree), degree, parties, n, counter=counter)
        assert _ints(got_t) == u and _ints(got_2t) == w


# ------------------------------------------------------------------------------------------------ (b) extract parity
@functools.lru_cache(maxsize=None)
def _inputs():
    return [O.synthetic_fr(5000 + j, NMAX - 3) + [0, 1, R - 1] for j in range(32)]


@functools.lru_cache(maxsize=None)
def _extract_want(parties, count):
    """at the longest length; an element's outputs depend on that element alone, so a shorter extraction is a prefix"""
    return D.extract(_inputs()[:parties], count)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("parties,count", [(p, p - t) for p, t in SHAPES] + [(32, 1), (32, 31)])
def test_rand_extract_matches_restatement(cozk, ctx, parties, count, n):
    recv = [cozk.Vec.from_ints(ctx, v[NMAX - n:]) for v in _inputs()[:parties]]  # the tail: 0, 1, r - 1 at every length
    got = cozk.shamir_rand_extract(ctx, recv, count)
    assert len(got) == count and all(len(g) == n for g in got)
    assert _ints(got) == [w[NMAX - n:] for w in _extract_want(parties, count)]


# ------------------------------------------------------------------------------------------------ (c) extract, edge operands
@pytest.mark.parametrize("case", ["rotated", "all_r_minus_1"])
def test_rand_extract_edge_operands(cozk, ctx, case):
    """31 outputs from 32 inputs: every tile, powers up to 32^30, the accumulators driven by the values next to 0, r and 2^253"""
    edge = EDGE + EDGE_MONT
    assert len(edge) == 12
    ins = [edge[j % 12:] + edge[:j % 12] for j in range(32)] if case == "rotated" else [[R - 1] * 12] * 32
    got = cozk.shamir_rand_extract(ctx, [cozk.Vec.from_ints(ctx, v) for v in ins], 31)
    assert _ints(got) == D.extract(ins, 31)
    _assert_canonical(np.concatenate([g.to_numpy() for g in got]))


def test_rand_extract_first_power_step_at_the_quotient_estimate_bound(cozk, ctx):
    """bound: q = T / D is floor(t / r) or one less (shamir.hip:14-20) in k_shamir_extract's power step w (j + 1): input j alone is
    ceil(Q r / (j + 1)) or floor(Q r / (j + 1)), so the first step lands less than j + 1 above or below Q r.  The extraction is
    linear: raw residues go in and the restatement runs on them"""
    lanes = [(j, w) for j in range(32) for Q in range(1, j + 1) for w in (-(-Q * R // (j + 1)), Q * R // (j + 1))]
    assert len(lanes) == 2 * sum(range(32)) and all(0 < w < R for _, w in lanes)
    assert all(abs(w * (j + 1) - (w * (j + 1) + R // 2) // R * R) < j + 1 for j, w in lanes)
    ins = [[w if j == k else 0 for j, w in lanes] for k in range(32)]
    got = cozk.shamir_rand_extract(ctx, [cozk.Vec.from_numpy(ctx, X.to_raw(v)) for v in ins], 31)
    raw = [g.to_numpy() for g in got]
    _assert_canonical(np.concatenate(raw))
    assert [X.from_raw(r) for r in raw] == D.extract(ins, 31)


# ------------------------------------------------------------------------------------------------ (d) extract vs composition
def test_rand_extract_equals_scale_and_add(cozk, ctx):
    parties, degree, n = 8, 2, 1000
    recv = [cozk.Vec.random(ctx, n, seed=600 + j) for j in range(parties)]
    got = cozk.shamir_rand_extract(ctx, recv, parties - degree)
    for k in range(parties - degree):
        acc = None
        for j in range(parties):
            term = cozk.Vec.from_numpy(ctx, recv[j].to_numpy()).scale(pow(j + 1, k, R))
            acc = term if acc is None else acc.binop(cozk.OP_ADD, term)
        assert np.array_equal(got[k].to_numpy(), acc.to_numpy()), "output %d" % k  # raw Montgomery limbs


# ------------------------------------------------------------------------------------------------ (e) mask
def test_mul_mask_edge_operands(cozk, ctx):
    edge = EDGE + EDGE_MONT
    a = [x for x in edge for _ in edge for _ in edge]
    b = [y for _ in edge for y in edge for _ in edge]
    c = [z for _ in edge for _ in edge for z in edge]
    assert len(a) == 12 ** 3
    got = cozk.Vec.from_ints(ctx, a).shamir_mul_mask(cozk.Vec.from_ints(ctx, b), cozk.Vec.from_ints(ctx, c))
    assert got.to_ints() == [(x * y + z) % R for x, y, z in zip(a, b, c)] == D.mul_mask(a, b, c)
    _assert_canonical(got.to_numpy())


def test_mul_mask_equals_mul_then_add(cozk, ctx):
    n = 1000
    A, B, C = (cozk.Vec.random(ctx, n, seed=s) for s in (61, 62, 63))
    fused = A.shamir_mul_mask(B, C)
    composed = A.binop(cozk.OP_MUL, B).binop(cozk.OP_ADD, C)
    assert np.array_equal(fused.to_numpy(), composed.to_numpy())
    E = cozk.Vec.alloc(ctx, 0)
    assert len(E.shamir_mul_mask(E, E)) == 0


# ------------------------------------------------------------------------------------------------ (f) in-process
@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


RAND_COUNTER = (1 << 40) + 5


@functools.lru_cache(maxsize=None)
def _rand_want(parties, degree):
    """the restatement's pairs at 257 elements; element i depends on counter + i alone, so one element is the prefix"""
    keys = D.party_keys(7, parties, degree)
    return keys, D.rand(keys, degree, 257, counter=RAND_COUNTER)


def _high_end(parties, k):
    return list(range(parties, parties - k, -1))


@pytest.mark.parametrize("king_at", ["0", "2t", "n-1"])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (7, 3)])
def test_rand_and_mul_king_inproc(cozk, ctx, party_ctxs, parties, degree, n, king_at):
    king = {"0": 0, "2t": 2 * degree, "n-1": parties - 1}[king_at]
    pcs = party_ctxs[:parties]
    keys, want_pairs = _rand_want(parties, degree)
    pairs = cozk.shamir_rand(pcs, keys, n, degree, counter=RAND_COUNTER)
    assert len(pairs) == parties and all(len(p) == parties - degree for p in pairs)
    pair_ints = [[(x.to_ints(), y.to_ints()) for x, y in pairs[q]] for q in range(parties)]
    for q in range(parties):
        for k in range(parties - degree):
            assert pairs[q][k][0].ctx is pcs[q] and pairs[q][k][1].ctx is pcs[q]
            assert pair_ints[q][k] == (want_pairs[q][k][0][:n], want_pairs[q][k][1][:n]), "party %d pair %d" % (q, k)
    half = lambda k, h: [pairs[q][k][h] for q in range(parties)]
    half_ints = lambda k, h: [pair_ints[q][k][h] for q in range(parties)]

    a, b, c = _secrets(61, n), list(reversed(_secrets(62, n))), _secrets(63, n)
    deal = lambda v, seed, ctr: cozk.Vec.from_ints(ctx, v).shamir_scatter(S.keys_for(seed, degree), degree, pcs, counter=ctr)
    sa, sb, sc = deal(a, 71, 0), deal(b, 72, n), deal(c, 73, 2 * n)
    got = cozk.shamir_mul_king(pcs, sa, sb, half(0, 0), half(0, 1), degree, king=king)
    got_ints = _ints(got)  # (the downloads also drain every party's stream before another context reads the vectors below)
    for q in range(parties):
        assert got[q].ctx is pcs[q] and len(got[q]) == n
    assert got_ints == D.mul_king(_ints(sa), _ints(sb), half_ints(0, 0), half_ints(0, 1), degree, king=king)  # every party's output
    ab = [x * y % R for x, y in zip(a, b)]
    pts = _high_end(parties, degree + 1)
    opened = cozk.shamir_combine([got[p - 1] for p in pts], pts, degree).to_ints()
    assert opened == ab
    # the resharing multiplication opens to the same value
    grr = cozk.shamir_mul(pcs, sa, sb, M.party_keys(7, parties, degree), degree, counter=3 * n)
    _ints(grr)
    assert cozk.shamir_combine([grr[p - 1] for p in pts], pts, degree).to_ints() == opened
    # negative control: t parties' worth of degree does not open it
    low = cozk.shamir_combine([got[p - 1] for p in pts], pts, degree - 1).to_ints()
    assert sum(x != y for x, y in zip(low, ab)) >= (n + 1) // 2
    # the product is a degree-t sharing: it multiplies again, with pair 1
    again = cozk.shamir_mul_king(pcs, got, sc, half(1, 0), half(1, 1), degree, king=king)
    again_ints = _ints(again)
    assert again_ints == D.mul_king(got_ints, _ints(sc), half_ints(1, 0), half_ints(1, 1), degree, king=king)
    assert cozk.shamir_combine([again[p - 1] for p in pts], pts, degree).to_ints() == [x * y % R for x, y in zip(ab, c)]
    # parties above 2t that are not the king send nothing: garbage or no factors and second halves there change no output
    k = D.senders(degree)
    rest = [p for p in range(k, parties) if p != king]
    if rest:
        junk = {p: cozk.Vec.random(pcs[p], n + 3, seed=p) for p in rest}
        for fill in (lambda p: junk[p], lambda p: None):
            sub = lambda vs: [fill(p) if p in rest else vs[p] for p in range(parties)]
            same = cozk.shamir_mul_king(pcs, sub(sa), sub(sb), half(0, 0), sub(half(0, 1)), degree, king=king)
            assert _ints(same) == got_ints


@pytest.mark.parametrize("king_at", ["0", "n-1"])
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (8, 2)])
def test_mul_king_inproc_equals_the_pairs_call_at_offset_zero(cozk, party_ctxs, parties, degree, n, king_at):
    """cozk_shamir_mul_king_inproc(a, b, ..) and cozk_shamir_mul_king_pairs_inproc(v, .., r_offset = 0) with v[2j] = a[j],
    v[2j + 1] = b[j] run one king driver and finish with one k_shamir_king_finish launch: equal raw words for every party, and the
    restatement's.  Both are element-wise in the parties' vectors, which therefore need not be sharings: where the length allows,
    the factors begin with all 144 pairs of the edge operands, the second factor's rotated by the party.  n - 1 is above 2t at (8, 2)"""
    king = 0 if king_at == "0" else parties - 1
    pcs, k = party_ctxs[:parties], D.senders(degree)
    edge = EDGE + EDGE_MONT
    ex, ey = [x for x in edge for _ in edge], [y for _ in edge for y in edge]
    lead = lambda blk, p: (blk[p:] + blk[:p]) if n >= len(blk) else []
    a = [(lead(ex, 0) + O.synthetic_fr(310 + p, n))[:n] for p in range(k)]
    b = [(lead(ey, p) + O.synthetic_fr(320 + p, n))[:n] for p in range(k)]
    v = [[z for xy in zip(a[p], b[p]) for z in xy] for p in range(k)]
    rt = [([0, R - 1][q % 2:] + O.synthetic_fr(330 + q, n))[:n] for q in range(parties)]
    r2t = [([R - 1, 0][p % 2:] + O.synthetic_fr(340 + p, n))[:n] for p in range(k)]
    up = lambda vs: [cozk.Vec.from_ints(pcs[p], x) for p, x in enumerate(vs)] + [None] * (parties - len(vs))  # nothing above 2t
    A, B, V, RT, R2T = up(a), up(b), up(v), up(rt), up(r2t)
    plain = cozk.shamir_mul_king(pcs, A, B, RT, R2T, degree, king=king)
    pairs = cozk.shamir_mul_king_pairs(pcs, V, RT, R2T, degree, r_offset=0, king=king)
    want = D.mul_king(a + [None] * (parties - k), b + [None] * (parties - k), rt, r2t + [None] * (parties - k), degree, king=king)
    for q in range(parties):
        assert plain[q].ctx is pcs[q] and pairs[q].ctx is pcs[q] and len(plain[q]) == len(pairs[q]) == n
        raw = plain[q].to_numpy()
        assert np.array_equal(raw, pairs[q].to_numpy()), "party %d" % q  # raw Montgomery limbs
        _assert_canonical(raw)
    assert _ints(plain) == want and _ints(pairs) == want
    assert _ints(A[:k]) == a and _ints(B[:k]) == b and _ints(V[:k]) == v and _ints(RT) == rt and _ints(R2T[:k]) == r2t  # only read


def test_rand_and_mul_king_inproc_empty(cozk, ctx, party_ctxs):
    pcs = party_ctxs[:5]
    pairs = cozk.shamir_rand(pcs, D.party_keys(1, 5, 2), 0, 2)
    assert [len(p) for p in pairs] == [3] * 5 and all(len(x) == 0 and len(y) == 0 for p in pairs for x, y in p)
    empty = [cozk.Vec.alloc(c, 0) for c in pcs]
    got = cozk.shamir_mul_king(pcs, empty, empty, [p[0][0] for p in pairs], [p[0][1] for p in pairs], 2, king=4)
    assert [len(g) for g in got] == [0] * 5 and all(g.to_ints() == [] for g in got)
    ot, o2 = cozk.shamir_rand_deal(ctx, 0, S.keys_for(1, 7), 2, 5)
    assert [len(g) for g in ot + o2] == [0] * 10


# ------------------------------------------------------------------------------------------------ (g) refusals
def _expect_invalid(cozk, ctx, rc, text):
    """`text` = "entry point: part of the message": the message names the entry point first"""
    assert rc == -1  # COZK_ERR_INVALID_ARG
    msg = cozk._lib.lib().cozk_last_error(ctx.h).decode()
    who, _, part = text.rpartition(": ")
    assert msg.startswith(who) and part in msg, msg


def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l = cozk._lib.lib()
    V = cozk.Vec.from_ints(ctx, [1, 2, 3])
    W = cozk.Vec.from_ints(ctx, [1, 2])
    U = cozk.Vec.from_ints(ctx, [1, 2, 3], kind=cozk.SCALAR_U32)
    keys = b"".join(S.keys_for(1, 25))
    SENT = 0x5A5A

    def outs():
        return (ctypes.c_void_p * 40)(*([SENT] * 40))

    def cleared(o, k):
        return all(o[i] is None for i in range(k)) and all(o[i] == SENT for i in range(k, 40))

    arr = lambda hs: (ctypes.c_void_p * 40)(*(list(hs) + [None] * (40 - len(hs))))
    hv = lambda vs: arr([v.h.value if v else None for v in vs])

    def deal(ks, deg, parties, text, k=None):
        x, y = outs(), outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_rand_deal(ctx.h, 3, ks, deg, parties, 0, x, y), "shamir_rand_deal: " + text)
        assert cleared(x, parties if k is None else k) and cleared(y, parties if k is None else k)

    deal(keys, 8, 32, "2 * degree <= COZK_SHAMIR_MAX_DEGREE")  # 2t = 16 > 15: the degree-2t sharing could not be dealt
    deal(keys, 0, 3, "1 <= degree")
    deal(keys, 2, 4, "2 * degree + 1 <= num_parties")
    deal(keys, 1, 2, "2 * degree + 1 <= num_parties")
    deal(None, 1, 3, "null argument")
    deal(keys, 1, 33, "num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)  # the tables' length is unknown: untouched
    x = outs()
    _expect_invalid(cozk, ctx, l.cozk_shamir_rand_deal(ctx.h, 3, keys, 1, 3, 0, x, None), "null output")
    assert cleared(x, 3)

    def extract(vs, parties, count, text, k=None):
        o = outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_rand_extract(ctx.h, hv(vs), parties, count, o), "shamir_rand_extract: " + text)
        assert cleared(o, count if k is None else k)

    extract([V, V, V], 3, 3, "1 <= count <= num_parties - 1")  # count = n
    extract([V, V, V], 3, 0, "1 <= count <= num_parties - 1", k=0)
    extract([V] * 32, 32, 32, "1 <= count <= num_parties - 1")
    extract([V, W, V], 3, 2, "the vectors must have one length")
    extract([V, U, V], 3, 2, "num_parties FR vectors")
    extract([V, None, V], 3, 2, "num_parties FR vectors")
    extract([V], 1, 1, "2 <= num_parties")
    extract([V] * 33, 33, 2, "num_parties <= COZK_SHAMIR_MAX_PARTIES")
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_rand_extract(ctx, [V, V, V], 3)
    assert e.value.code == -1

    h = ctypes.c_void_p(SENT)
    for a, b, c, text in ((V, W, V, "one length"), (V, V, W, "one length"), (V, U, V, "must be FR vectors"), (V, None, V, "null argument")):
        h.value = SENT
        rc = l.cozk_shamir_mul_mask(ctx.h, a.h, b.h if b else None, c.h, ctypes.byref(h))
        _expect_invalid(cozk, ctx, rc, "shamir_mul_mask: " + text)
        assert h.value is None
    with pytest.raises(cozk.CozkError) as e:
        V.shamir_mul_mask(V, W)
    assert e.value.code == -1

    # in process: the text is left with party 0
    p0 = party_ctxs[0]
    mk = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    good = [mk(c, [1, 2, 3]) for c in party_ctxs[:5]]
    short = mk(party_ctxs[1], [1, 2])
    stray = mk(party_ctxs[0], [1, 2, 3])  # the right length, the wrong party's context
    all_ctxs = lambda parties: arr([c.h.value for c in party_ctxs[:parties]] + [party_ctxs[0].h.value] * max(parties - 8, 0))

    def king_inproc(parties, deg, king, a, b, rt, r2t, text, ctxs=None, k=None):
        o = outs()
        rc = l.cozk_shamir_mul_king_inproc(all_ctxs(parties) if ctxs is None else ctxs, hv(a), hv(b), hv(rt), hv(r2t), deg, parties, king, o)
        _expect_invalid(cozk, p0, rc, "shamir_mul_king_inproc: " + text)
        assert cleared(o, parties if k is None else k)

    g3 = good[:3]
    swap = lambda vs, i, v: vs[:i] + [v] + vs[i + 1:]
    king_inproc(3, 1, 3, g3, g3, g3, g3, "0 <= king < num_parties")  # king = n
    king_inproc(3, 1, -1, g3, g3, g3, g3, "0 <= king < num_parties")
    king_inproc(3, 1, 0, g3, swap(g3, 1, short), g3, g3, "must have one length")
    king_inproc(3, 1, 0, g3, g3, swap(g3, 1, short), g3, "must have one length")
    king_inproc(3, 1, 0, g3, g3, g3, swap(g3, 1, stray), "must be a vector of its party's context")  # a pair vector of the wrong context
    king_inproc(3, 1, 0, g3, g3, swap(g3, 2, stray), g3, "must be a vector of its party's context")
    king_inproc(3, 1, 0, swap(g3, 1, stray), g3, g3, g3, "must be a vector of its party's context")
    king_inproc(3, 1, 0, g3, swap(g3, 2, None), g3, g3, "null a factor of parties 0..2 * degree")
    king_inproc(3, 1, 0, g3, g3, swap(g3, 2, None), g3, "null the first half of the pair")
    king_inproc(3, 1, 0, g3, g3, g3, swap(g3, 0, mk(party_ctxs[0], [1, 2, 3], cozk.SCALAR_U32)), "must be an FR vector")
    king_inproc(3, 1, 0, g3, g3, g3, g3, "null party context", ctxs=arr([party_ctxs[0].h.value, None, party_ctxs[2].h.value]))
    king_inproc(4, 2, 0, good[:4], good[:4], good[:4], good[:4], "2 * degree + 1 <= num_parties")
    king_inproc(32, 8, 0, g3, g3, g3, g3, "2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    king_inproc(33, 1, 0, g3, g3, g3, g3, "num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_mul_king(party_ctxs[:3], g3, g3, g3, swap(g3, 1, stray), 1)
    assert e.value.code == -1

    kb = ctypes.create_string_buffer(keys, len(keys))
    kp = lambda parties: arr([ctypes.addressof(kb)] * parties)

    def rand_inproc(parties, deg, key_ptrs, text, ctxs=None, k=None):
        x, y = (ctypes.c_void_p * 1100)(*([SENT] * 1100)), (ctypes.c_void_p * 1100)(*([SENT] * 1100))
        rc = l.cozk_shamir_rand_inproc(all_ctxs(parties) if ctxs is None else ctxs, key_ptrs, 3, deg, parties, 0, x, y)
        _expect_invalid(cozk, p0, rc, "shamir_rand_inproc: " + text)
        k = parties * (parties - deg) if k is None else k
        for t in (x, y):
            assert all(t[i] is None for i in range(k)) and all(t[i] == SENT for i in range(k, 1100))

    rand_inproc(32, 8, kp(32), "2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    rand_inproc(4, 2, kp(4), "2 * degree + 1 <= num_parties")
    rand_inproc(3, 1, arr([ctypes.addressof(kb), None, ctypes.addressof(kb)]), "every party needs its key block")
    rand_inproc(3, 1, kp(3), "null party context", ctxs=arr([party_ctxs[0].h.value, None, party_ctxs[2].h.value]))
    rand_inproc(33, 1, kp(33), "num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_rand(party_ctxs[:4], D.party_keys(1, 4, 2), 3, 2)
    assert e.value.code == -1

    # one party per process: refused without a ring, nothing touched
    x, y = outs(), outs()
    _expect_invalid(cozk, ctx, l.cozk_shamir_rand_vec(ctx.h, 3, keys, 1, 0, x, y), "cozk_ring_init has not been called")
    assert cleared(x, 0) and cleared(y, 0)
    h.value = SENT
    _expect_invalid(cozk, ctx, l.cozk_shamir_mul_king_vec(ctx.h, V.h, V.h, V.h, V.h, 1, 0, ctypes.byref(h)), "cozk_ring_init has not been called")
    assert h.value is None
    with pytest.raises(cozk.CozkError) as e:
        ctx.shamir_rand_vec(3, S.keys_for(1, 4), 1)
    assert "cozk_ring_init has not been called" in str(e.value)
    assert V.to_ints() == [1, 2, 3] and _ints(good) == [[1, 2, 3]] * 5  # nothing ran


def test_vec_entry_points_on_a_single_rank_ring(cozk):
    """one rank cannot hold 2t + 1 parties: both one-party-per-process calls refuse on the host, with the ring up"""
    c = cozk.Context(0)
    try:
        c.ring_init(cozk.Context.ring_unique_id(), 0, 1)
        V = cozk.Vec.from_ints(c, [1, 2, 3])
        with pytest.raises(cozk.CozkError) as err:
            c.shamir_rand_vec(3, S.keys_for(1, 4), 1)
        assert err.value.code == -1 and "shamir_rand_vec" in str(err.value) and "num_parties" in str(err.value)
        with pytest.raises(cozk.CozkError) as err:
            c.shamir_mul_king_vec(V, V, V, V, 1)
        assert err.value.code == -1 and "shamir_mul_king_vec" in str(err.value) and "num_parties" in str(err.value)
        c.ring_destroy()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (h) one party per process
def test_rand_vec_and_mul_king_vec_three_processes_one_gpu_each(cozk, tmp_path):
    if torch.cuda.device_count() < 3:
        pytest.skip("needs 3 GPUs: RCCL refuses two ranks of one communicator on the same device")
    parties, degree, n, king = 3, 1, 257, 1
    a, b = _secrets(81, n), list(reversed(_secrets(82, n)))
    sa = S.share_vec(a, S.keys_for(83, degree), degree, parties)
    sb = S.share_vec(b, S.keys_for(84, degree), degree, parties, counter=n)
    keys = D.party_keys(9, parties, degree)
    script = os.path.join(ROOT, "tools", "shamir_dn_party.py")
    procs = []
    try:
        ring_id = None
        for rank in range(parties):  # three FRESH interpreters; rank 0 draws the ring id and prints it before it joins
            job = tmp_path / ("party%d.json" % rank)
            job.write_text(json.dumps({"a": [hex(x) for x in sa[rank]], "b": [hex(x) for x in sb[rank]], "keys": [k.hex() for k in keys[rank]],
                                       "degree": degree, "counter": 2 * n, "king": king, "out": str(tmp_path / ("out%d.json" % rank))}))
            cmd = [sys.executable, script, "--rank", str(rank), "--ranks", str(parties), "--job", str(job)]
            if rank:
                cmd += ["--ring-id", ring_id]
            p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=open(tmp_path / ("err%d.txt" % rank), "w"), text=True)
            procs.append(p)
            if rank == 0:
                for line in p.stdout:  # ends with the pipe if the child dies first
                    if line.startswith("ring-id "):
                        ring_id = line.split()[1]
                        break
                assert ring_id and len(ring_id) == 256, (tmp_path / "err0.txt").read_text()[-2000:]
        for rank, p in enumerate(procs):
            out, _ = p.communicate(timeout=300)
            assert p.returncode == 0, out[-2000:] + (tmp_path / ("err%d.txt" % rank)).read_text()[-2000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = [json.loads((tmp_path / ("out%d.json" % r)).read_text()) for r in range(parties)]
    unhex = lambda xs: [int(x, 16) for x in xs]
    want = D.rand(keys, degree, n, counter=2 * n)
    got_pairs = [[(unhex(x), unhex(y)) for x, y in r["pairs"]] for r in res]
    assert got_pairs == [[(x, y) for x, y in want[q]] for q in range(parties)]
    got = [unhex(r["c"]) for r in res]
    assert got == D.mul_king(sa, sb, [want[q][0][0] for q in range(parties)], [want[q][0][1] for q in range(parties)], degree, king=king)
    assert S.combine_vec(got[1:], [2, 3], degree) == [x * y % R for x, y in zip(a, b)]


# ------------------------------------------------------------------------------------------------ (h) two devices
def test_rand_and_mul_king_inproc_peer_copy_two_gpus(cozk, ctx):
    """the hipMemcpyPeer legs of cozk_shamir_rand_inproc and cozk_shamir_mul_king_inproc: odd parties on GPU 1, the king on
    either device"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    parties, degree, n = 5, 2, 257
    other = [cozk.Context(1) for _ in range(2)]
    mine = [cozk.Context(0) for _ in range(3)]
    pcs = [other[p // 2] if p % 2 else mine[p // 2] for p in range(parties)]
    keys = D.party_keys(11, parties, degree)
    pairs = cozk.shamir_rand(pcs, keys, n, degree, counter=5)
    want = D.rand(keys, degree, n, counter=5)
    for q in range(parties):
        assert [(x.to_ints(), y.to_ints()) for x, y in pairs[q]] == [(x, y) for x, y in want[q]]
    a, b = _secrets(91, n), list(reversed(_secrets(92, n)))
    sa = cozk.Vec.from_ints(ctx, a).shamir_scatter(S.keys_for(93, degree), degree, pcs)
    sb = cozk.Vec.from_ints(ctx, b).shamir_scatter(S.keys_for(94, degree), degree, pcs, counter=n)
    sa_i, sb_i = _ints(sa), _ints(sb)
    for k, king in enumerate((0, 1)):
        got = cozk.shamir_mul_king(pcs, sa, sb, [pairs[q][k][0] for q in range(parties)], [pairs[q][k][1] for q in range(parties)], degree, king=king)
        assert _ints(got) == D.mul_king(sa_i, sb_i, [want[q][k][0] for q in range(parties)], [want[q][k][1] for q in range(parties)], degree, king=king)
        for q in range(parties):
            assert got[q].ctx is pcs[q]
        for v in got:
            v.free()
    for v in sa + sb + [h for p in pairs for xy in p for h in xy]:
        v.free()
    for c in other + mine:
        c.close()
