"""GPU tests of the king grand product (cozk_shamir_mul_mask_pairs, cozk_shamir_king_finish, cozk_shamir_mul_king_pairs_inproc,
cozk_shamir_gp_prep_inproc, cozk_shamir_gp_prove_king_inproc) against the big-int restatement tests/shamir_gp_king_ref.py, the
composed entry points and the plain oracle.  Bar: bit-exact; calls go through the C ABI (ctypes).  No test provokes a device fault:
every bad argument is rejected on the host before any launch."""
import ctypes

import numpy as np
import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_king_ref as K
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S
from test_gpu_shamir import EDGE, EDGE_MONT
from test_gpu_shamir_gp import GP_SHAPES, MUL_CTR, RAND_CTR, SENT, _cleared, _expect_invalid, _high_end, _ints, _layer, _oracle_proof, _outs, party_ctxs  # noqa: F401

pytestmark = pytest.mark.gpu
R = O.R


def _canonical(raw):
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


# ------------------------------------------------------------------------------------------------ (a) the mask kernel
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("m", [0, 1, 257, 1000])
def test_mask_pairs_matches_the_mask_of_the_halves(cozk, ctx, m, off):
    v = _layer(700 + m, m)
    r2t = O.synthetic_fr(701 + off, m + off + 2)  # a half of a pair longer than off + m
    V, P = cozk.Vec.from_ints(ctx, v), cozk.Vec.from_ints(ctx, r2t)
    got = V.shamir_mul_mask_pairs(P, off)
    assert len(got) == m
    assert got.to_ints() == K.mul_mask_pairs(v, r2t, off) == D.mul_mask(v[0::2], v[1::2], r2t[off:off + m])
    halves = cozk.Vec.from_ints(ctx, v[0::2]).shamir_mul_mask(cozk.Vec.from_ints(ctx, v[1::2]), cozk.Vec.from_ints(ctx, r2t[off:off + m]))
    assert np.array_equal(got.to_numpy(), halves.to_numpy())  # raw Montgomery limbs
    assert V.to_ints() == v and P.to_ints() == r2t  # only read


def test_mask_pairs_edge_operands(cozk, ctx):
    """all 144 pairs of the edge operands of test_gpu_shamir.py through the Montgomery product and the addition of the mask"""
    edge = EDGE + EDGE_MONT
    v = [z for x in edge for y in edge for z in (x, y)]
    assert len(v) == 288
    V = cozk.Vec.from_ints(ctx, v)
    for r in (0, R - 1):
        got = V.shamir_mul_mask_pairs(cozk.Vec.from_ints(ctx, [5] + [r] * 144), 1)
        assert got.to_ints() == [(x * y + r) % R for x in edge for y in edge]
        _canonical(got.to_numpy())


# ------------------------------------------------------------------------------------------------ (b) the finish kernel
@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("length", [1, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (8, 2), (15, 7), (32, 15)])
def test_king_finish_matches_combine_and_subtract(cozk, ctx, parties, degree, length, off):
    k = 2 * degree + 1
    masked = [([0, R - 1][j % 2:j % 2 + 1] + O.synthetic_fr(800 + j, length))[:length] for j in range(k)]
    rts = [[R - 1, 0][q % 2:q % 2 + 1] * (off + 1) + O.synthetic_fr(900 + q, length) for q in range(parties)]  # longer than off + length
    mv = [cozk.Vec.from_ints(ctx, x) for x in masked]
    rv = [cozk.Vec.from_ints(ctx, x) for x in rts]
    pts = list(range(1, k + 1))
    z_want = cozk.shamir_combine(mv, pts, 2 * degree)
    z_ref, out_ref = K.king_finish(masked, degree, rts, off)
    assert z_want.to_ints() == z_ref
    want = [z_want.binop(cozk.OP_SUB, cozk.Vec.from_ints(ctx, x[off:off + length])).to_numpy() for x in rts]
    for count in (1, parties):
        got, z = cozk.shamir_king_finish(ctx, mv, degree, rv[:count], off, want_z=True)
        bare = cozk.shamir_king_finish(ctx, mv, degree, rv[:count], off)  # no output for z
        assert len(got) == len(bare) == count and all(len(g) == length and g.ctx is ctx for g in got)
        assert np.array_equal(z.to_numpy(), z_want.to_numpy())
        for q in range(count):
            assert np.array_equal(got[q].to_numpy(), want[q]) and np.array_equal(bare[q].to_numpy(), want[q]), "party %d" % q
            assert got[q].to_ints() == out_ref[q]
        _canonical(np.concatenate([g.to_numpy() for g in got] + [z.to_numpy()]))
    assert _ints(mv) == masked and _ints(rv) == rts  # only read


# ------------------------------------------------------------------------------------------------ (c) one tree level, in process
def _pair0(cozk, pcs, degree, n_elems, seed):
    """pair 0 of one preprocessing call on the device, and its integers (tests/test_gpu_shamir_dn.py holds the call to its restatement)"""
    pairs = cozk.shamir_rand(pcs, D.party_keys(seed, len(pcs), degree), n_elems, degree, counter=11)
    rt, r2t = [p[0][0] for p in pairs], [p[0][1] for p in pairs]
    return rt, r2t, _ints(rt), _ints(r2t)


@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (7, 3)])
def test_mul_king_pairs_inproc(cozk, ctx, party_ctxs, parties, degree, m):
    pcs = party_ctxs[:parties]
    v = _layer(61, m)
    sv = cozk.Vec.from_ints(ctx, v).shamir_scatter(S.keys_for(71, degree), degree, pcs, counter=5)
    sv_ints = _ints(sv)
    rt, r2t, rt_ints, r2t_ints = _pair0(cozk, pcs, degree, m + 5, 9)
    prod = G.pair_products(v)
    pts = _high_end(parties, degree + 1)
    k = G.senders(degree)
    for off, king in ((0, 0), (3, parties - 1)):  # the king is a sender once, and the highest party once (above 2t where parties > 2t + 1)
        got = cozk.shamir_mul_king_pairs(pcs, sv, rt, r2t, degree, r_offset=off, king=king)
        got_ints = _ints(got)
        for q in range(parties):
            assert got[q].ctx is pcs[q] and len(got[q]) == m
        assert got_ints == K.mul_king_pairs(sv_ints, rt_ints, r2t_ints, degree, offset=off, king=king)  # every party's output
        assert cozk.shamir_combine([got[p - 1] for p in pts], pts, degree).to_ints() == prod
        if parties > k:  # parties above 2t send nothing: garbage or no layer and second half there change no output
            junk = [cozk.Vec.random(pcs[p], 2 * m + 3, seed=p) for p in range(k, parties)]
            for rest in (junk, [None] * (parties - k)):
                same = cozk.shamir_mul_king_pairs(pcs, sv[:k] + rest, rt, r2t[:k] + rest, degree, r_offset=off, king=king)
                assert _ints(same) == got_ints
    assert _ints(sv) == sv_ints and _ints(rt) == rt_ints and _ints(r2t) == r2t_ints  # only read


def test_mul_king_pairs_inproc_empty(cozk, party_ctxs):
    pcs = party_ctxs[:5]
    empty = lambda: [cozk.Vec.alloc(c, 0) for c in pcs]
    got = cozk.shamir_mul_king_pairs(pcs, empty(), empty(), empty(), 2, king=4)
    assert [len(g) for g in got] == [0] * 5 and all(g.to_ints() == [] for g in got)


# ------------------------------------------------------------------------------------------------ (d) the prover
KINGS = [0, 1, 2, 0, 7, 3]


@pytest.mark.parametrize("shape,king", list(zip(GP_SHAPES, KINGS)), ids=lambda x: str(x))
def test_shamir_gp_prove_king(cozk, ctx, party_ctxs, shape, king):
    parties, degree, batch, per = shape
    pcs = party_ctxs[:parties]
    plain = G.leaves(21, batch, per)
    n_leaves = len(plain)
    leaves = cozk.Vec.from_ints(ctx, plain).shamir_scatter(S.keys_for(22, degree), degree, pcs, counter=9)
    shares = _ints(leaves)
    rk = D.party_keys(4, parties, degree)
    prep = cozk.shamir_gp_prep(pcs, rk, n_leaves, batch, degree, rand_counter=RAND_CTR)
    pr = prep.result
    held = K.pairs_needed(n_leaves, batch)
    assert held == {2: 0, 4: 1}.get(per, 2)  # (3, 1, 1, 2) has no level, (3, 1, 1, 4) uses pair 0 only
    assert (pr.n_openings, pr.pair_elems, pr.pairs_held, pr.used) == (G.num_openings(n_leaves, batch), n_leaves // 2 if held else 0, held, 0)
    assert pr.t_offline_ms > 0
    got = cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=king)
    want_bytes, want_claim, want_r = _oracle_proof(plain, batch)
    assert got.proof_bytes == want_bytes  # the plain prover's proof, byte for byte
    grr = cozk.shamir_gp_prove(pcs, leaves, batch, M.party_keys(3, parties, degree), rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    assert got.proof_bytes == grr.proof_bytes  # and the resharing prover's
    res = got.result
    assert res.verified == 1 and res.proof_len == len(want_bytes)
    assert (got.claim, got.r) == (want_claim, want_r)
    ref = K.prove(shares, batch, K.prep(rk, degree, n_leaves, batch, rand_counter=RAND_CTR), degree, king=king)
    assert res.n_layers == len(ref["layers"]) and res.n_opened == len(ref["msgs"]) == pr.n_openings
    assert got.msgs == ref["msgs"]  # the masks, their order, the counters and every level's slice of its pair
    assert got.finals == ref["finals"]
    assert res.t_construct_ms >= 0 and res.t_prove_ms > 0
    assert (prep.result.used, prep.result.pairs_held) == (1, 0)
    assert _ints(leaves) == shares  # the leaves are only read
    # the same prep a second time is refused on the host, and nothing runs
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=king)
    assert e.value.code == -1 and "shamir_gp_prove_king_inproc: the preprocessing has been used" in str(e.value)
    assert _ints(leaves) == shares
    prep.close()
    # a fresh prep from the same keys and counter: identical bytes and messages; the verifier is optional
    fresh = cozk.shamir_gp_prep(pcs, rk, n_leaves, batch, degree, rand_counter=RAND_CTR)
    again = cozk.shamir_gp_prove_king(pcs, leaves, batch, fresh, king=king, verify=False)
    assert again.proof_bytes == got.proof_bytes and again.msgs == got.msgs and again.finals == got.finals and again.result.verified == -1
    fresh.close()


# ------------------------------------------------------------------------------------------------ (e) per-round launches
def test_shamir_gp_prove_king_large_layers(cozk, ctx, party_ctxs):
    """layers above 2048 elements: the per-round launches and the mask kernel over several workgroups.  The n-party big-int
    restatement is too slow at this size: the plain oracle's proof is the yardstick"""
    parties, degree, batch, per = 8, 2, 2, 1 << 11
    plain = O.synthetic_fr(33, batch * per)
    leaves = cozk.Vec.from_ints(ctx, plain).shamir_scatter(S.keys_for(34, degree), degree, party_ctxs, counter=1)
    prep = cozk.shamir_gp_prep(party_ctxs, D.party_keys(6, parties, degree), len(plain), batch, degree, rand_counter=RAND_CTR)
    assert (prep.result.pair_elems, prep.result.pairs_held) == (batch * per // 2, 2)
    got = cozk.shamir_gp_prove_king(party_ctxs, leaves, batch, prep, king=5)
    want_bytes, want_claim, want_r = _oracle_proof(plain, batch)
    assert got.proof_bytes == want_bytes
    assert got.result.verified == 1 and (got.claim, got.r) == (want_claim, want_r)
    prep.close()


# ------------------------------------------------------------------------------------------------ (f) refusals
def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l = cozk._lib.lib()
    mkv = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    arr = lambda hs: (ctypes.c_void_p * 40)(*(list(hs) + [None] * (40 - len(hs))))
    hs = lambda vs: arr([x.h.value if x else None for x in vs])
    V, W, U = mkv(ctx, [1, 2, 3, 4]), mkv(ctx, [1, 2, 3]), mkv(ctx, [1, 2, 3, 4], cozk.SCALAR_U32)
    P2, P3 = mkv(ctx, [7, 8]), mkv(ctx, [7, 8, 9])

    def mask(v, r, off, text):
        h = ctypes.c_void_p(SENT)
        _expect_invalid(cozk, ctx, l.cozk_shamir_mul_mask_pairs(ctx.h, v.h if v else None, r.h if r else None, off, ctypes.byref(h)), "shamir_mul_mask_pairs: " + text)
        assert h.value is None

    mask(None, P2, 0, "null argument")
    mask(V, None, 0, "null argument")
    mask(W, P2, 0, "the layer must have an even length")
    mask(U, P2, 0, "the layer must be an FR vector")
    mask(V, U, 0, "the mask must be an FR vector")
    mask(V, P2, 1, "r_offset + len(v) / 2 <= len(r_2t)")
    mask(V, P3, 2, "r_offset + len(v) / 2 <= len(r_2t)")
    mask(V, P3, (1 << 64) - 1, "r_offset + len(v) / 2 <= len(r_2t)")
    _expect_invalid(cozk, ctx, l.cozk_shamir_mul_mask_pairs(ctx.h, V.h, P2.h, 0, None), "null output")
    with pytest.raises(cozk.CozkError) as e:
        V.shamir_mul_mask_pairs(P2, 1)
    assert e.value.code == -1

    def finish(masked, deg, rts, off, count, text, k=None, z=True):
        o, zh = _outs(), ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_king_finish(ctx.h, hs(masked) if masked is not None else None, deg, hs(rts) if rts is not None else None, off, count, o,
                                       ctypes.byref(zh) if z else None)
        _expect_invalid(cozk, ctx, rc, "shamir_king_finish: " + text)
        assert _cleared(o, count if k is None else k) and (zh.value is None or not z)

    three = [V, V, V]
    finish(None, 1, [V], 0, 1, "null argument")
    finish(three, 1, None, 0, 1, "null argument")
    finish(three, 0, [V], 0, 1, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    finish(three, 16, [V], 0, 1, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    finish(three, 1, [V], 0, 0, "1 <= count <= COZK_SHAMIR_MAX_PARTIES", k=0)
    finish(three, 1, [V], 0, 33, "1 <= count <= COZK_SHAMIR_MAX_PARTIES", k=0)  # out[] untouched: its length is unknown
    finish([V, None, V], 1, [V], 0, 1, "2 * degree + 1 masked FR vectors")
    finish([V, U, V], 1, [V], 0, 1, "2 * degree + 1 masked FR vectors")
    finish([V, W, V], 1, [V], 0, 1, "the masked vectors must have one length")
    finish(three, 1, [V, None], 0, 2, "count FR first halves of the pair")
    finish(three, 1, [U], 0, 1, "count FR first halves of the pair")
    finish(three, 1, [V, W], 0, 2, "r_offset + len(masked) <= len(r_t)", z=False)
    finish(three, 1, [V], 1, 1, "r_offset + len(masked) <= len(r_t)")
    _expect_invalid(cozk, ctx, l.cozk_shamir_king_finish(ctx.h, hs(three), 1, hs([V]), 0, 1, None, None), "null output")

    # in process: the text is left with party 0
    p0 = party_ctxs[0]
    three_ctxs = arr([c.h.value for c in party_ctxs[:3]])
    good = [mkv(c, [1, 2, 3, 4]) for c in party_ctxs[:3]]
    half = [mkv(c, [5, 6, 7]) for c in party_ctxs[:3]]

    def level(parties, deg, v, rt, r2t, off, king, text, ctxs=None, k=None):
        o = _outs()
        rc = l.cozk_shamir_mul_king_pairs_inproc(three_ctxs if ctxs is None else ctxs, hs(v), hs(rt), hs(r2t), off, deg, parties, king, o)
        _expect_invalid(cozk, p0, rc, "shamir_mul_king_pairs_inproc: " + text)
        assert _cleared(o, parties if k is None else k)

    level(3, 1, good, half, half, 2, 0, "r_offset + len(v) / 2 <= len of the halves of the pair")
    level(3, 1, good, half, half, 0, 3, "0 <= king < num_parties")
    level(3, 1, good, half, half, 0, -1, "0 <= king < num_parties")
    level(3, 1, [good[0], mkv(party_ctxs[1], [1, 2, 3]), good[2]], half, half, 0, 0, "the layer must have an even length")
    level(3, 1, [good[0], mkv(party_ctxs[1], [1, 2]), good[2]], half, half, 0, 0, "the layers must have one length")
    level(3, 1, [good[0], good[1], mkv(party_ctxs[2], [1, 2, 3, 4], cozk.SCALAR_U32)], half, half, 0, 0, "the layer must be an FR vector")
    level(3, 1, [good[0], None, good[2]], half, half, 0, 0, "parties 0..2 * degree need their layer")
    level(3, 1, [good[0], good[0], good[2]], half, half, 0, 0, "party p's layer must be a vector of party_ctxs[p]")
    level(3, 1, good, [half[0], None, half[2]], half, 0, 0, "null first half of the pair")
    level(3, 1, good, half, [half[0], None, half[2]], 0, 0, "parties 0..2 * degree need the second half of the pair")
    level(3, 1, good, [half[0], mkv(party_ctxs[1], [5, 6]), half[2]], half, 0, 0, "the halves of the pair must have one length")
    level(3, 1, good, half, [half[0], half[1], mkv(party_ctxs[2], [5, 6])], 0, 0, "the halves of the pair must have one length")
    level(3, 1, good, [half[0], half[1], mkv(party_ctxs[2], [5, 6, 7], cozk.SCALAR_U32)], half, 0, 0, "the halves of the pair must be FR vectors")
    level(3, 1, good, [half[0], half[0], half[2]], half, 0, 0, "party p's halves of the pair must be vectors of party_ctxs[p]")
    level(3, 1, good, half, [half[0], half[0], half[2]], 0, 0, "party p's halves of the pair must be vectors of party_ctxs[p]")
    level(3, 1, good, half, half, 0, 0, "null party context", ctxs=arr([party_ctxs[0].h.value, None, party_ctxs[2].h.value]))
    level(3, 0, good, half, half, 0, 0, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    level(17, 8, good * 6, half * 6, half * 6, 0, 0, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    level(4, 2, good, half, half, 0, 0, "2 * degree + 1 <= num_parties")
    level(33, 1, good, half, half, 0, 0, "2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)  # out[] untouched: its length is unknown
    _expect_invalid(cozk, p0, l.cozk_shamir_mul_king_pairs_inproc(three_ctxs, hs(good), hs(half), hs(half), 0, 1, 3, 0, None), "null output")
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_mul_king_pairs(party_ctxs[:3], good, half, half, 1, r_offset=2)
    assert e.value.code == -1

    # the preprocessing: the handle stays NULL
    rk = ctypes.create_string_buffer(b"\x02" * (32 * 22), 32 * 22)
    rp = [ctypes.addressof(rk)] * 3

    def prep(parties, deg, n_leaves, batch, rkeys, text, ctxs=None):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_gp_prep_inproc(three_ctxs if ctxs is None else ctxs, arr(rkeys) if rkeys is not None else None, n_leaves, batch, deg, parties, 0,
                                          ctypes.byref(h))
        _expect_invalid(cozk, p0, rc, "shamir_gp_prep_inproc: " + text)
        assert h.value is None

    prep(3, 1, 4, 3, rp, "leaves.len() % batch_size != 0")
    prep(3, 1, 4, 0, rp, "leaves.len() % batch_size != 0")
    prep(3, 1, 0, 1, rp, "leaves.len() % batch_size != 0")
    prep(3, 1, 4, 4, rp, "leaves per circuit must be a power of two >= 2")
    prep(3, 1, 6, 1, rp, "leaves per circuit must be a power of two >= 2")
    prep(3, 1, 4, 1, [rp[0], rp[1], None], "every party needs its mask key block")
    prep(3, 1, 4, 1, None, "null argument")
    prep(3, 1, 4, 1, rp, "null party context", ctxs=arr([party_ctxs[0].h.value, party_ctxs[1].h.value, None]))
    prep(3, 0, 4, 1, rp, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    prep(17, 8, 4, 1, rp * 6, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    prep(4, 2, 4, 1, rp, "2 * degree + 1 <= num_parties")
    assert l.cozk_shamir_gp_prep_inproc(three_ctxs, arr(rp), 4, 1, 1, 3, 0, None) == -1

    # the prover: everything before any launch, the handle stays NULL, the prep stays unused
    pcs = party_ctxs[:3]
    keys = D.party_keys(8, 3, 1)
    pre = cozk.shamir_gp_prep(pcs, keys, 4, 1, 1)

    def gp(leaves, batch, king, text, ctxs=None, label=b"cozk", prep_h=pre.h):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_gp_prove_king_inproc(three_ctxs if ctxs is None else ctxs, hs(leaves) if leaves is not None else None, batch, prep_h, king, label, 1,
                                                ctypes.byref(h))
        _expect_invalid(cozk, p0, rc, "shamir_gp_prove_king_inproc: " + text)
        assert h.value is None and pre.result.used == 0

    gp(good, 1, 0, "null argument", prep_h=None)
    gp(good, 1, 0, "null argument", label=None)
    gp(None, 1, 0, "null argument")
    gp(good, 1, 3, "0 <= king < num_parties")
    gp(good, 1, -1, "0 <= king < num_parties")
    gp(good, 1, 0, "null party context", ctxs=arr([party_ctxs[0].h.value, party_ctxs[1].h.value, None]))
    gp(good, 1, 0, "the preprocessing was made for other party contexts", ctxs=arr([party_ctxs[0].h.value, party_ctxs[1].h.value, party_ctxs[3].h.value]))
    gp([good[0], None, good[2]], 1, 0, "parties 0..2 * degree need their leaves")
    gp([good[0], mkv(party_ctxs[1], [1, 2]), good[2]], 1, 0, "the leaves must have one length")
    gp([good[0], good[1], mkv(party_ctxs[2], [1, 2, 3, 4], cozk.SCALAR_U32)], 1, 0, "the leaves must be FR vectors")
    gp([good[0], good[0], good[2]], 1, 0, "party p's leaves must be a vector of party_ctxs[p]")
    gp(good, 3, 0, "leaves.len() % batch_size != 0")
    gp(good, 0, 0, "leaves.len() % batch_size != 0")
    gp(good, 4, 0, "leaves per circuit must be a power of two >= 2")
    gp(good, 2, 0, "the preprocessing was made for another (n_leaves, batch_size)")
    gp([mkv(c, [1, 2, 3, 4, 5, 6, 7, 8]) for c in pcs], 1, 0, "the preprocessing was made for another (n_leaves, batch_size)")
    assert l.cozk_shamir_gp_prove_king_inproc(three_ctxs, hs(good), 1, pre.h, 0, b"cozk", 1, None) == -1
    assert _ints(good) == [[1, 2, 3, 4]] * 3 and pre.result.used == 0  # nothing ran
    assert cozk.shamir_gp_prove_king(pcs, good, 1, pre).result.verified == 1  # and the prep still serves its one proof
    h = ctypes.c_void_p(SENT)
    _expect_invalid(cozk, p0, l.cozk_shamir_gp_prove_king_inproc(three_ctxs, hs(good), 1, pre.h, 0, b"cozk", 1, ctypes.byref(h)),
                    "shamir_gp_prove_king_inproc: the preprocessing has been used")
    assert h.value is None
    pre.close()
