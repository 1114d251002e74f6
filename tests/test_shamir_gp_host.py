"""CPU tier of the Shamir grand product prover: the big-int restatement (tests/shamir_gp_ref.py) proves itself -- n Shamir parties
produce the plain prover's proof of the same leaves, the plain verifier accepts it, every opening of degree 2t is masked and
needs all 2t + 1 messages -- and the new entry points exist and refuse bad arguments on the host, with no device."""
import ctypes

import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S

R = O.R
# (parties, degree, batch, interleaved leaves per circuit)
SHAPES = [(3, 1, 1, 4), (3, 1, 2, 16), (5, 2, 4, 8), (8, 2, 2, 16), (7, 3, 1, 2), (5, 2, 3, 8)]
MUL_CTR, RAND_CTR = (1 << 33) + 5, 77


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d-t%d-b%d-per%d" % s)
def world(request):
    parties, degree, batch, per = request.param
    plain = G.leaves(21, batch, per)
    shares = S.share_vec(plain, S.keys_for(22, degree), degree, parties, counter=9)
    res = G.prove(shares, batch, M.party_keys(3, parties, degree), D.party_keys(4, parties, degree), degree, mul_counter=MUL_CTR,
                  rand_counter=RAND_CTR)
    want, want_r = O.gp_prove(O.gp_construct([plain], batch, None), O.Transcript())
    return dict(parties=parties, degree=degree, batch=batch, per=per, plain=plain, shares=shares, res=res, want=want, want_r=want_r)


def _opened_scalars(proof):
    """what the openings of degree 2t must give, in their order: the outputs, then per layer and round the four coefficients (the
    linear one, which the proof leaves out, from g(0) + g(1) = the running claim, as the verifier derives it)"""
    out = list(proof["outputs"])
    tr = O.Transcript()
    tr.append_scalars(proof["outputs"])
    padded = list(proof["outputs"])
    while len(padded) & (len(padded) - 1):
        padded.append(0)
    r = tr.challenge_vector(len(padded).bit_length() - 1)
    claim = sum(e * v for e, v in zip(O.eq_evals(r), padded)) % R
    for lp in proof["layers"]:
        for comp in lp["round_polys"]:
            poly = [comp[0], (claim - 2 * comp[0] - sum(comp[1:])) % R] + list(comp[1:])
            out += poly
            tr.append_scalars(comp)
            claim = O.unipoly_eval(poly, tr.challenge_scalar())
        tr.append_scalar(lp["left"])
        tr.append_scalar(lp["right"])
        claim = (lp["left"] + tr.challenge_scalar() * (lp["right"] - lp["left"])) % R
    return out


def test_restatement_gives_the_plain_provers_proof(world):
    res = world["res"]
    assert res["proof"] == world["want"]
    assert res["r"] == world["want_r"]
    assert O.gp_verify(res["proof"], world["batch"], O.Transcript()) == (res["claim"], res["r"])
    assert G.ser_proof(res["proof"]) == G.ser_proof(world["want"])


def test_restatement_construction_opens_to_the_plain_layers(world):
    parties, degree = world["parties"], world["degree"]
    plain_layers = O.gp_construct([world["plain"]], world["batch"], None)
    pts = list(range(parties, parties - degree - 1, -1))  # the t + 1 highest parties: they dealt nothing when n > 2t + 1
    assert len(world["res"]["layers"]) == len(plain_layers)
    for mine, theirs in zip(world["res"]["layers"], plain_layers):
        assert S.combine_vec([mine[p - 1] for p in pts], pts, degree) == theirs[0]


def test_restatement_openings_are_masked_and_need_every_sender(world):
    degree, res = world["degree"], world["res"]
    k = G.senders(degree)
    scalars = _opened_scalars(res["proof"])
    rounds = sum(len(lp["round_polys"]) for lp in res["proof"]["layers"])
    assert len(res["msgs"]) == len(res["locals"]) == len(scalars) == world["batch"] + 4 * rounds  # M
    assert len(res["msgs"]) == G.num_openings(len(world["plain"]), world["batch"])
    lam = S.lagrange_from_coeff(list(range(1, k + 1)))
    low = S.lagrange_from_coeff(list(range(1, k)))
    for m, (msg, loc, want) in enumerate(zip(res["msgs"], res["locals"], scalars)):
        assert len(msg) == k
        assert all(x != y for x, y in zip(msg, loc)), "opening %d is sent unmasked" % m
        assert S.reconstruct(msg, lam) == want, "opening %d" % m
        assert S.reconstruct(loc, lam) == want  # the mask shares zero
        assert S.reconstruct(msg[:k - 1], low) != want, "opening %d opens from 2t messages" % m


def test_restatement_final_claims_open_with_degree_t(world):
    degree, res = world["degree"], world["res"]
    lam = S.lagrange_from_coeff(list(range(1, degree + 2)))
    assert len(res["finals"]) == len(res["proof"]["layers"])
    for fin, lp in zip(res["finals"], res["proof"]["layers"]):
        assert len(fin) == degree + 1
        assert S.reconstruct([f[0] for f in fin], lam) == lp["left"]
        assert S.reconstruct([f[1] for f in fin], lam) == lp["right"]


def test_restatement_counters_and_label_matter(world):
    parties, degree, batch = world["parties"], world["degree"], world["batch"]
    mk, rk = M.party_keys(3, parties, degree), D.party_keys(4, parties, degree)
    base = world["res"]
    other = G.prove(world["shares"], batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR + 1)
    assert other["proof"] == base["proof"] and other["msgs"] != base["msgs"]  # other masks, the same proof
    if len(base["layers"]) > 1:
        other = G.prove(world["shares"], batch, mk, rk, degree, mul_counter=MUL_CTR + 1, rand_counter=RAND_CTR)
        assert other["proof"] == base["proof"] and other["layers"][1] != base["layers"][1]  # other sharings of the same tree
    other = G.prove(world["shares"], batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR, label=b"other")
    assert other["proof"]["outputs"] == base["proof"]["outputs"] and other["r"] != base["r"]


def test_restatement_pair_deal_is_the_deal_of_the_halves():
    v = O.synthetic_fr(31, 10)
    keys = S.keys_for(32, 2)
    assert G.mul_deal_pairs(v, keys, 2, 5, counter=3) == S.share_vec(G.pair_products(v), keys, 2, 5, counter=3)
    assert G.pair_products([2, 3, R - 1, R - 1]) == [6, 1]
    assert G.rounds_per_layer(24, 3) == [2, 3, 4] and G.num_openings(24, 3) == 3 + 4 * 9 and G.num_openings(2, 1) == 1


# ------------------------------------------------------------------------------------------------ the ABI, without a device
SYMBOLS = ("cozk_shamir_mul_deal_pairs", "cozk_shamir_mul_pairs_inproc", "cozk_shamir_gp_prove_inproc", "cozk_shamir_gp_free",
           "cozk_shamir_gp_get_result", "cozk_shamir_gp_proof_bytes", "cozk_shamir_gp_point_len", "cozk_shamir_gp_final",
           "cozk_shamir_gp_msgs_len", "cozk_shamir_gp_msgs", "cozk_shamir_gp_finals_len", "cozk_shamir_gp_finals")


def test_wrappers_exist(cozk):
    for name in ("shamir_mul_pairs", "shamir_gp_prove"):
        assert callable(getattr(cozk, name))
    assert callable(cozk.Vec.shamir_mul_deal_pairs)
    for sym in SYMBOLS:
        assert sym in cozk._lib.SIGNATURES and hasattr(cozk._lib.lib(), sym)
    assert [f[0] for f in cozk.ShamirGpResult._fields_] == ["verified", "n_layers", "proof_len", "n_opened", "t_construct_ms", "t_prove_ms"]


SENT = 0x5A5A


def _table(k=40):
    return (ctypes.c_void_p * k)(*([SENT] * k))


def _cleared(t, k):
    return all(t[i] is None for i in range(k)) and all(t[i] == SENT for i in range(k, len(t)))


def test_null_and_out_of_range_arguments_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    keys = b"\x01" * (32 * 22)
    x = _table()
    assert l.cozk_shamir_mul_deal_pairs(None, None, keys, 2, 5, 0, x) == -1 and _cleared(x, 5)  # COZK_ERR_INVALID_ARG
    x = _table()
    assert l.cozk_shamir_mul_deal_pairs(None, None, keys, 2, 33, 0, x) == -1 and _cleared(x, 0)  # the table's length is unknown: untouched
    assert l.cozk_shamir_mul_deal_pairs(None, None, keys, 2, 5, 0, None) == -1
    x = _table()
    assert l.cozk_shamir_mul_pairs_inproc(None, None, None, 2, 5, 0, x) == -1 and _cleared(x, 5)
    x = _table()
    assert l.cozk_shamir_mul_pairs_inproc(None, None, None, 2, 4, 0, x) == -1 and _cleared(x, 4)  # 2t + 1 > n
    x = _table()
    assert l.cozk_shamir_mul_pairs_inproc(None, None, None, 1, 33, 0, x) == -1 and _cleared(x, 0)
    assert l.cozk_shamir_mul_pairs_inproc(None, None, None, 2, 5, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_gp_prove_inproc(None, None, 1, None, None, 1, 3, 0, 0, b"cozk", 1, ctypes.byref(h)) == -1 and h.value is None
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_gp_prove_inproc(None, None, 1, None, None, 8, 17, 0, 0, b"cozk", 1, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_gp_prove_inproc(None, None, 1, None, None, 1, 3, 0, 0, b"cozk", 1, None) == -1
    # the accessors of no handle
    res = cozk.ShamirGpResult()
    buf = (ctypes.c_uint64 * 8)()
    assert l.cozk_shamir_gp_get_result(None, ctypes.byref(res)) == -1
    assert l.cozk_shamir_gp_proof_bytes(None, buf, 64) == -1
    assert l.cozk_shamir_gp_final(None, buf, buf) == -1
    assert l.cozk_shamir_gp_msgs(None, buf, 2) == -1 and l.cozk_shamir_gp_finals(None, buf, 2) == -1
    assert l.cozk_shamir_gp_point_len(None) == 0 and l.cozk_shamir_gp_msgs_len(None) == 0 and l.cozk_shamir_gp_finals_len(None) == 0
    assert l.cozk_shamir_gp_free(None) == 0
