"""CPU tier of the king grand product: the big-int restatement (tests/shamir_gp_king_ref.py) proves itself -- with the king construct
and preprocessed pairs n Shamir parties still produce the plain prover's proof, under the resharing prover's zero masks; every level
opens to the plain layer; the masked sum opens to a b + the pair's value; the slices of pair 1 are disjoint and end where stated --
and the new entry points exist and refuse bad arguments on the host, with no device."""
import ctypes

import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_king_ref as K
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S

R = O.R
# (parties, degree, batch, interleaved leaves per circuit, king): the shapes of tests/test_gpu_shamir_gp_king.py
SHAPES = [(3, 1, 1, 2, 0), (3, 1, 1, 4, 1), (3, 1, 2, 16, 2), (5, 2, 4, 8, 0), (8, 2, 2, 16, 7), (7, 3, 2, 8, 3)]
MUL_CTR, RAND_CTR = (1 << 33) + 5, (1 << 32) + 77


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d-t%d-b%d-per%d-king%d" % s)
def world(request):
    parties, degree, batch, per, king = request.param
    plain = G.leaves(21, batch, per)
    shares = S.share_vec(plain, S.keys_for(22, degree), degree, parties, counter=9)
    rk = D.party_keys(4, parties, degree)
    pre = K.prep(rk, degree, len(plain), batch, rand_counter=RAND_CTR)
    res = K.prove(shares, batch, pre, degree, king=king)
    return dict(parties=parties, degree=degree, batch=batch, per=per, king=king, plain=plain, shares=shares, rk=rk, pre=pre, res=res)


def test_king_proof_is_the_plain_and_the_resharing_provers_proof(world):
    res, batch, degree = world["res"], world["batch"], world["degree"]
    want, want_r = O.gp_prove(O.gp_construct([world["plain"]], batch, None), O.Transcript())
    assert res["proof"] == want and res["r"] == want_r
    assert O.gp_verify(res["proof"], batch, O.Transcript()) == (res["claim"], res["r"])
    grr = G.prove(world["shares"], batch, M.party_keys(3, world["parties"], degree), world["rk"], degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    assert res["proof"] == grr["proof"] and (res["claim"], res["r"]) == (grr["claim"], grr["r"])
    assert G.ser_proof(res["proof"]) == G.ser_proof(want)
    assert len(res["msgs"]) == len(grr["msgs"]) == world["pre"]["M"]
    # the same masks over other sharings of the same tree: message minus local value is the mask in both provers
    unmask = lambda r: [[(x - y) % R for x, y in zip(msg, loc)] for msg, loc in zip(r["msgs"], r["locals"])]
    assert unmask(res) == unmask(grr)


def test_zero_masks_are_the_resharing_provers(world):
    pre, degree = world["pre"], world["degree"]
    assert pre["M"] == G.num_openings(len(world["plain"]), world["batch"])
    assert pre["zero"] == G.zero_masks(world["rk"], degree, pre["M"], RAND_CTR)
    k = G.senders(degree)
    lam = S.lagrange_from_coeff(list(range(1, k + 1)))
    assert all(S.reconstruct([pre["zero"][p][m] for p in range(k)], lam) == 0 for m in range(pre["M"]))


def test_every_level_opens_to_the_plain_layer(world):
    parties, degree = world["parties"], world["degree"]
    plain_layers = O.gp_construct([world["plain"]], world["batch"], None)
    pts = list(range(parties, parties - degree - 1, -1))  # the t + 1 highest parties
    layers = world["res"]["layers"]
    assert len(layers) == len(plain_layers) == G.num_layers(len(world["plain"]), world["batch"])
    for mine, theirs in zip(layers, plain_layers):
        assert S.combine_vec([mine[p - 1] for p in pts], pts, degree) == theirs[0]
    # the king changes who computes, not what
    other = K.construct(world["shares"], world["batch"], world["pre"], degree, king=(world["king"] + 1) % parties)
    assert other == layers


def test_masked_sum_opens_to_the_product_plus_the_pair_value(world):
    degree, pre, layers = world["degree"], world["pre"], world["res"]["layers"]
    n_leaves, batch = len(world["plain"]), world["batch"]
    plain_layers = O.gp_construct([world["plain"]], batch, None)
    k = G.senders(degree)
    half = n_leaves // 2
    for i, (pair, off, m) in enumerate(K.level_slices(n_leaves, batch)):
        masked = [K.mul_mask_pairs(layers[i][p], pre["pairs"][p][pair][1], off) for p in range(k)]
        z, outs = K.king_finish(masked, degree, [q[pair][0] for q in pre["pairs"]], off)
        value = D.pair_value(world["rk"], pair, half, counter=RAND_CTR + pre["M"])[off:off + m]
        assert z == [(ab + r) % R for ab, r in zip(G.pair_products(plain_layers[i][0]), value)]
        assert outs == layers[i + 1]


def test_pair_slices_are_disjoint_and_end_where_stated(world):
    n_leaves, batch = len(world["plain"]), world["batch"]
    slices = K.level_slices(n_leaves, batch)
    assert len(slices) == G.num_layers(n_leaves, batch) - 1
    assert K.pairs_needed(n_leaves, batch) == len({s[0] for s in slices}) == len(world["pre"]["pairs"][0])
    if slices:
        assert slices[0] == (0, 0, n_leaves // 2)  # pair 0 serves level 0 whole
    end = 0
    for i, (pair, off, m) in enumerate(slices[1:], start=1):
        assert pair == 1 and off == end == n_leaves // 2 - n_leaves // 2 ** i  # the sum of the output lengths of levels 1..i - 1
        assert m == n_leaves // 2 ** (i + 1)
        end = off + m
    if len(slices) > 1:
        assert end == n_leaves // 2 - 2 * batch


def test_shapes_without_a_level_and_with_one():
    assert K.level_slices(2, 1) == [] and K.pairs_needed(2, 1) == 0
    assert K.level_slices(4, 1) == [(0, 0, 2)] and K.pairs_needed(4, 1) == 1
    assert K.level_slices(32, 2) == [(0, 0, 16), (1, 0, 8), (1, 8, 4)] and K.pairs_needed(32, 2) == 2
    assert K.mul_mask_pairs([2, 3, R - 1, R - 1], [9, 9, 5, 7], 2) == [11, 8]


# ------------------------------------------------------------------------------------------------ the ABI, without a device
SYMBOLS = ("cozk_shamir_mul_mask_pairs", "cozk_shamir_king_finish", "cozk_shamir_mul_king_pairs_inproc", "cozk_shamir_gp_prep_inproc",
           "cozk_shamir_gp_prep_free", "cozk_shamir_gp_prep_get_result", "cozk_shamir_gp_prove_king_inproc")


def test_wrappers_exist(cozk):
    for name in ("shamir_king_finish", "shamir_mul_king_pairs", "shamir_gp_prep", "shamir_gp_prove_king"):
        assert callable(getattr(cozk, name))
    assert callable(cozk.Vec.shamir_mul_mask_pairs) and callable(cozk.ShamirGpPrep.close)
    for sym in SYMBOLS:
        assert sym in cozk._lib.SIGNATURES and hasattr(cozk._lib.lib(), sym)
    assert [f[0] for f in cozk.ShamirGpPrepResult._fields_] == ["n_openings", "pair_elems", "pairs_held", "used", "t_offline_ms"]
    assert ctypes.sizeof(cozk.ShamirGpResult) == 40  # the existing result struct has not grown


SENT = 0x5A5A


def _table(k=40):
    return (ctypes.c_void_p * k)(*([SENT] * k))


def _cleared(t, k):
    return all(t[i] is None for i in range(k)) and all(t[i] == SENT for i in range(k, len(t)))


def test_null_and_out_of_range_arguments_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_mul_mask_pairs(None, None, None, 0, ctypes.byref(h)) == -1 and h.value is None  # COZK_ERR_INVALID_ARG
    assert l.cozk_shamir_mul_mask_pairs(None, None, None, 0, None) == -1
    x, z = _table(), ctypes.c_void_p(SENT)
    assert l.cozk_shamir_king_finish(None, None, 2, None, 0, 8, x, ctypes.byref(z)) == -1 and _cleared(x, 8) and z.value is None
    x = _table()
    assert l.cozk_shamir_king_finish(None, None, 2, None, 0, 33, x, None) == -1 and _cleared(x, 0)  # the table's length is unknown: untouched
    assert l.cozk_shamir_king_finish(None, None, 2, None, 0, 8, None, None) == -1
    x = _table()
    assert l.cozk_shamir_mul_king_pairs_inproc(None, None, None, None, 0, 2, 5, 0, x) == -1 and _cleared(x, 5)
    x = _table()
    assert l.cozk_shamir_mul_king_pairs_inproc(None, None, None, None, 0, 1, 33, 0, x) == -1 and _cleared(x, 0)
    assert l.cozk_shamir_mul_king_pairs_inproc(None, None, None, None, 0, 2, 5, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_gp_prep_inproc(None, None, 8, 1, 1, 3, 0, ctypes.byref(h)) == -1 and h.value is None
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_gp_prep_inproc(None, None, 8, 1, 8, 17, 0, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_gp_prep_inproc(None, None, 8, 1, 1, 3, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_gp_prove_king_inproc(None, None, 1, None, 0, b"cozk", 1, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_gp_prove_king_inproc(None, None, 1, None, 0, b"cozk", 1, None) == -1
    res = cozk.ShamirGpPrepResult()
    assert l.cozk_shamir_gp_prep_get_result(None, ctypes.byref(res)) == -1
    assert l.cozk_shamir_gp_prep_free(None) == 0
