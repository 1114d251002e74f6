"""GPU tests of the Shamir grand product prover (cozk_shamir_mul_deal_pairs, cozk_shamir_mul_pairs_inproc,
cozk_shamir_gp_prove_inproc) against the big-int restatement tests/shamir_gp_ref.py and the plain oracle.  Bar: bit-exact; calls go
through the C ABI (ctypes).  No test provokes a device fault: every bad argument is rejected on the host before any launch."""
import ctypes
import functools

import numpy as np
import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S
from test_gpu_shamir import EDGE, EDGE_MONT

pytestmark = pytest.mark.gpu
R = O.R
MMAX = 1000


def _layer(seed, m):
    """an interleaved layer of m pairs with the field's corner values among its first elements"""
    e = [0, 1, R - 1, R - 2] + EDGE_MONT
    return (e + O.synthetic_fr(seed, max(2 * m - len(e), 1)))[:2 * m]


def _ints(vecs):
    return [v.to_ints() for v in vecs]


@functools.lru_cache(maxsize=None)
def _coefs(degree, counter):
    """the dealer's PRF coefficient vectors at the longest length, computed once: a shorter deal uses their prefixes"""
    return S.prf_coeffs(S.keys_for(40 + degree, degree), degree, counter, MMAX)


def _poly(cozk):
    import importlib
    return importlib.import_module("co-zkvms_amd.poly")


# ------------------------------------------------------------------------------------------------ (a) deal parity
@pytest.mark.parametrize("counter", [0, (1 << 33) + 7])
@pytest.mark.parametrize("m", [0, 1, 257, 1000])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (15, 7), (17, 8), (32, 15)])
def test_mul_deal_pairs_matches_share_of_the_pair_products(cozk, ctx, parties, degree, m, counter):
    v = _layer(500 + parties, m)
    keys = S.keys_for(40 + degree, degree)
    V = cozk.Vec.from_ints(ctx, v)
    got = V.shamir_mul_deal_pairs(keys, degree, parties, counter=counter)
    assert len(got) == parties and all(len(g) == m for g in got)
    prod = G.pair_products(v)
    want = S.eval_vec([prod] + [c[:m] for c in _coefs(degree, counter)], parties)  # = S.share_vec(prod, keys, ...)
    assert _ints(got) == want  # every party's vector
    if m == 257 and counter == 0:
        assert want == S.share_vec(prod, keys, degree, parties, counter=counter) == G.mul_deal_pairs(v, keys, degree, parties, counter=counter)
    # raw Montgomery limbs (canonical outputs are unique) against the two composed forms
    halves = cozk.Vec.from_ints(ctx, v[0::2]).shamir_mul_deal(cozk.Vec.from_ints(ctx, v[1::2]), keys, degree, parties, counter=counter)
    for g, h in zip(got, halves):
        assert np.array_equal(g.to_numpy(), h.to_numpy())
    if m:  # (a layer holds at least one pair)
        layer = _poly(cozk).Rep3DenseInterleavedPolynomial.from_vecs(ctx, V)
        composed = layer.layer_output_local().shamir_share(keys, degree, parties, counter=counter)
        for g, c in zip(got, composed):
            assert np.array_equal(g.to_numpy(), c.to_numpy())
    assert V.to_ints() == v  # the layer is only read


# ------------------------------------------------------------------------------------------------ (b) edge operands
@pytest.mark.parametrize("degree", [1, 7, 8, 15])
def test_mul_deal_pairs_edge_operands_through_the_product(cozk, ctx, degree):
    """all pairs of the edge operands of test_gpu_shamir.py (EDGE + EDGE_MONT: 12 values, 144 pairs), interleaved, through the
    Montgomery product in front of the Horner chains, at 32 parties, through the templated (1, 7) and the rolled (8, 15) variant"""
    edge = EDGE + EDGE_MONT
    v = [z for x in edge for y in edge for z in (x, y)]
    assert len(v) == 2 * len(edge) ** 2 == 288  # every operand against every operand
    keys = S.keys_for(40 + degree, degree)
    got = cozk.Vec.from_ints(ctx, v).shamir_mul_deal_pairs(keys, degree, 32, counter=0)
    prod = G.pair_products(v)
    assert prod == [x * y % R for x in edge for y in edge]
    want = S.eval_vec([prod] + [c[:144] for c in _coefs(degree, 0)], 32)
    for p in range(32):
        assert got[p].to_ints() == want[p], "party %d" % p
    raw = np.concatenate([g.to_numpy() for g in got])  # canonical limbs: below r as 256-bit integers
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


# ------------------------------------------------------------------------------------------------ (c) refusals
def _expect_invalid(cozk, ctx, rc, text):
    assert rc == -1  # COZK_ERR_INVALID_ARG
    msg = cozk._lib.lib().cozk_last_error(ctx.h).decode()
    assert text in msg, msg


SENT = 0x5A5A


def _outs():
    return (ctypes.c_void_p * 40)(*([SENT] * 40))


def _cleared(o, k):
    return all(o[i] is None for i in range(k)) and all(o[i] == SENT for i in range(k, 40))


@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l = cozk._lib.lib()
    V = cozk.Vec.from_ints(ctx, [1, 2, 3, 4])
    W = cozk.Vec.from_ints(ctx, [1, 2, 3])
    U = cozk.Vec.from_ints(ctx, [1, 2, 3, 4], kind=cozk.SCALAR_U32)
    keys = b"".join(S.keys_for(1, 15))

    def deal(v, ks, deg, parties, text, k=None):
        o = _outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_mul_deal_pairs(ctx.h, v.h if v else None, ks, deg, parties, 0, o), "shamir_mul_deal_pairs: " + text)
        assert _cleared(o, parties if k is None else k)

    deal(W, keys, 1, 3, "the layer must have an even length")
    deal(U, keys, 1, 3, "the layer must be an FR vector")
    deal(V, keys, 6, 10, "2 * degree + 1 <= num_parties")
    deal(V, keys, 1, 2, "2 * degree + 1 <= num_parties")
    deal(V, None, 1, 3, "null argument")
    deal(None, keys, 1, 3, "null argument")
    deal(V, keys, 0, 3, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    deal(V, keys, 16, 32, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    deal(V, keys, 1, 33, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)  # out[] untouched: its length is unknown
    _expect_invalid(cozk, ctx, l.cozk_shamir_mul_deal_pairs(ctx.h, V.h, keys, 1, 3, 0, None), "null output")
    for bad, deg, parties in ((W, 1, 3), (U, 1, 3), (V, 6, 10)):
        with pytest.raises(cozk.CozkError) as e:
            bad.shamir_mul_deal_pairs(S.keys_for(1, deg), deg, parties)
        assert e.value.code == -1

    # in process: the same rules for every dealer; the text is left with party 0
    p0 = party_ctxs[0]
    mk = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    arr = lambda hs: (ctypes.c_void_p * 40)(*(list(hs) + [None] * (40 - len(hs))))
    kb = ctypes.create_string_buffer(keys, len(keys))
    all_ctxs = arr([c.h.value for c in party_ctxs[:3]])

    def inproc(parties, deg, v, key_ptrs, text, ctxs=None, k=None):
        o = _outs()
        rc = l.cozk_shamir_mul_pairs_inproc(all_ctxs if ctxs is None else ctxs, arr([x.h.value if x else None for x in v]), arr(key_ptrs), deg, parties, 0, o)
        _expect_invalid(cozk, p0, rc, "shamir_mul_pairs_inproc: " + text)
        assert _cleared(o, parties if k is None else k)

    good = [mk(c, [1, 2, 3, 4]) for c in party_ctxs[:3]]
    kp = [ctypes.addressof(kb)] * 3
    inproc(3, 1, [good[0], mk(party_ctxs[1], [1, 2, 3]), good[2]], kp, "the layer must have an even length")
    inproc(3, 1, [good[0], mk(party_ctxs[1], [1, 2]), good[2]], kp, "the layers must have one length")
    inproc(3, 1, [good[0], good[1], mk(party_ctxs[2], [1, 2, 3, 4], cozk.SCALAR_U32)], kp, "the layer must be an FR vector")
    inproc(3, 1, good, [kp[0], None, kp[2]], "parties 0..2 * degree need their key block")
    inproc(3, 1, [good[0], None, good[2]], kp, "parties 0..2 * degree need their layer")
    inproc(3, 1, [good[0], good[0], good[2]], kp, "party p's layer must be a vector of party_ctxs[p]")
    inproc(3, 1, good, kp, "null party context", ctxs=arr([party_ctxs[0].h.value, None, party_ctxs[2].h.value]))
    inproc(10, 6, good * 4, kp * 4, "2 * degree + 1 <= num_parties")
    inproc(33, 1, good, kp, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)
    with pytest.raises(cozk.CozkError) as e:
        cozk.shamir_mul_pairs(party_ctxs[:3], [good[0], mk(party_ctxs[1], [1, 2, 3]), good[2]], M.party_keys(1, 3, 1), 1)
    assert e.value.code == -1

    # the prover: everything before any launch, the handle stays NULL, the text is left with party 0
    rk = ctypes.create_string_buffer(b"\x02" * (32 * 22), 32 * 22)
    rp = [ctypes.addressof(rk)] * 3

    def gp(parties, deg, batch, leaves, mkeys, rkeys, text, ctxs=None, label=b"cozk"):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_gp_prove_inproc(all_ctxs if ctxs is None else ctxs, arr([x.h.value if x else None for x in leaves]), batch, arr(mkeys), arr(rkeys),
                                           deg, parties, 0, 0, label, 1, ctypes.byref(h))
        _expect_invalid(cozk, p0, rc, "shamir_gp_prove_inproc: " + text)
        assert h.value is None

    gp(3, 1, 3, good, kp, rp, "leaves.len() % batch_size != 0")
    gp(3, 1, 0, good, kp, rp, "leaves.len() % batch_size != 0")
    gp(3, 1, 4, good, kp, rp, "leaves per circuit must be a power of two >= 2")
    six = [mk(c, [1, 2, 3, 4, 5, 6]) for c in party_ctxs[:3]]
    gp(3, 1, 1, six, kp, rp, "leaves per circuit must be a power of two >= 2")
    gp(3, 1, 1, [good[0], mk(party_ctxs[1], [1, 2]), good[2]], kp, rp, "the leaves must have one length")
    gp(3, 1, 1, [good[0], good[1], mk(party_ctxs[2], [1, 2, 3, 4], cozk.SCALAR_U32)], kp, rp, "the leaves must be FR vectors")
    gp(3, 1, 1, [good[0], good[0], good[2]], kp, rp, "party p's leaves must be a vector of party_ctxs[p]")
    gp(3, 1, 1, [good[0], None, good[2]], kp, rp, "parties 0..2 * degree need their leaves and their key block")
    gp(3, 1, 1, good, [kp[0], None, kp[2]], rp, "parties 0..2 * degree need their leaves and their key block")
    gp(3, 1, 1, good, kp, [rp[0], rp[1], None], "every party needs its mask key block")
    gp(3, 1, 1, good, kp, rp, "null party context", ctxs=arr([party_ctxs[0].h.value, party_ctxs[1].h.value, None]))
    gp(3, 1, 1, good, kp, rp, "null argument", label=None)
    gp(3, 0, 1, good, kp, rp, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    gp(4, 2, 1, good, kp, rp, "2 * degree + 1 <= num_parties")
    gp(17, 8, 1, good * 6, kp * 6, rp * 6, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    assert l.cozk_shamir_gp_prove_inproc(all_ctxs, arr([x.h.value for x in good]), 1, arr(kp), arr(rp), 1, 3, 0, 0, b"cozk", 1, None) == -1
    assert V.to_ints() == [1, 2, 3, 4] and _ints(good) == [[1, 2, 3, 4]] * 3  # nothing ran


# ------------------------------------------------------------------------------------------------ (d) one tree level, in process
def _high_end(parties, k):
    return list(range(parties, parties - k, -1))


@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (7, 3)])
def test_mul_pairs_inproc(cozk, ctx, party_ctxs, parties, degree, m):
    pcs = party_ctxs[:parties]
    v = _layer(61, m)
    sv = cozk.Vec.from_ints(ctx, v).shamir_scatter(S.keys_for(71, degree), degree, pcs, counter=5)
    keys = M.party_keys(7, parties, degree)
    got = cozk.shamir_mul_pairs(pcs, sv, keys, degree, counter=3 * m)
    got_ints = _ints(got)  # (the downloads also drain every party's stream before another context reads the vectors below)
    for q in range(parties):
        assert got[q].ctx is pcs[q] and len(got[q]) == m
    sv_ints = _ints(sv)
    assert got_ints == M.mul([s[0::2] for s in sv_ints], [s[1::2] for s in sv_ints], keys, degree, counter=3 * m)  # every party's output
    assert got_ints == G.mul_pairs(sv_ints, keys, degree, counter=3 * m)
    prod = G.pair_products(v)
    pts = _high_end(parties, degree + 1)
    assert cozk.shamir_combine([got[p - 1] for p in pts], pts, degree).to_ints() == prod
    # parties above 2t deal nothing: garbage or no vectors and keys there change no output
    k = G.senders(degree)
    if parties > k:
        junk = [cozk.Vec.random(pcs[p], 2 * m + 3, seed=p) for p in range(k, parties)]
        for rest in (junk, [None] * (parties - k)):
            same = cozk.shamir_mul_pairs(pcs, sv[:k] + rest, keys[:k] + [None] * (parties - k), degree, counter=3 * m)
            assert _ints(same) == got_ints
    assert _ints(sv) == sv_ints  # the layer is only read


def test_mul_pairs_inproc_empty(cozk, party_ctxs):
    pcs = party_ctxs[:5]
    empty = [cozk.Vec.alloc(c, 0) for c in pcs]
    got = cozk.shamir_mul_pairs(pcs, empty, M.party_keys(1, 5, 2), 2)
    assert [len(g) for g in got] == [0] * 5 and all(g.to_ints() == [] for g in got)


# ------------------------------------------------------------------------------------------------ (e) the prover
MUL_CTR, RAND_CTR = (1 << 33) + 5, (1 << 32) + 77
GP_SHAPES = [(3, 1, 1, 2), (3, 1, 1, 4), (3, 1, 2, 16), (5, 2, 4, 8), (8, 2, 2, 16), (7, 3, 2, 8)]


def _oracle_proof(plain, batch):
    proof, r = O.gp_prove(O.gp_construct([plain], batch, None), O.Transcript())
    claim, r2 = O.gp_verify(proof, batch, O.Transcript())
    assert r2 == r
    return G.ser_proof(proof), claim, r


@pytest.mark.parametrize("parties,degree,batch,per", GP_SHAPES, ids=lambda x: str(x))
def test_shamir_gp_prove(cozk, ctx, party_ctxs, parties, degree, batch, per):
    pcs = party_ctxs[:parties]
    plain = G.leaves(21, batch, per)
    leaves = cozk.Vec.from_ints(ctx, plain).shamir_scatter(S.keys_for(22, degree), degree, pcs, counter=9)
    shares = _ints(leaves)
    mk, rk = M.party_keys(3, parties, degree), D.party_keys(4, parties, degree)
    got = cozk.shamir_gp_prove(pcs, leaves, batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    want_bytes, want_claim, want_r = _oracle_proof(plain, batch)
    assert got.proof_bytes == want_bytes  # the plain prover's proof, byte for byte
    res = got.result
    assert res.verified == 1 and res.proof_len == len(want_bytes)
    assert (got.claim, got.r) == (want_claim, want_r)
    ref = G.prove(shares, batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    assert ref["proof"] == O.gp_prove(O.gp_construct([plain], batch, None), O.Transcript())[0]
    assert res.n_layers == len(ref["layers"]) and res.n_opened == len(ref["msgs"]) == G.num_openings(len(plain), batch)
    assert got.msgs == ref["msgs"]  # the masks, their order and both counters
    assert got.finals == ref["finals"]
    assert res.t_construct_ms >= 0 and res.t_prove_ms > 0
    assert _ints(leaves) == shares  # the leaves are only read
    again = cozk.shamir_gp_prove(pcs, leaves, batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    assert again.proof_bytes == got.proof_bytes and again.msgs == got.msgs and again.finals == got.finals
    # parties above 2t send nothing: no leaves and no multiplication keys there change nothing; and the verifier is optional
    k = G.senders(degree)
    if parties > k:
        rest = [None] * (parties - k)
        same = cozk.shamir_gp_prove(pcs, leaves[:k] + rest, batch, mk[:k] + rest, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR, verify=False)
        assert same.proof_bytes == got.proof_bytes and same.msgs == got.msgs and same.result.verified == -1


# ------------------------------------------------------------------------------------------------ (f) per-round launches
def test_shamir_gp_prove_large_layers(cozk, ctx, party_ctxs):
    """layers above 2048 elements: the per-round launches run, not only the single-launch small path.  The
    n-party big-int restatement is too slow at this size: the plain oracle's proof is the yardstick"""
    parties, degree, batch, per = 8, 2, 2, 1 << 11
    plain = O.synthetic_fr(33, batch * per)
    leaves = cozk.Vec.from_ints(ctx, plain).shamir_scatter(S.keys_for(34, degree), degree, party_ctxs, counter=1)
    got = cozk.shamir_gp_prove(party_ctxs, leaves, batch, M.party_keys(5, parties, degree), D.party_keys(6, parties, degree), degree,
                               mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    want_bytes, want_claim, want_r = _oracle_proof(plain, batch)
    assert got.proof_bytes == want_bytes
    assert got.result.verified == 1 and (got.claim, got.r) == (want_claim, want_r)
