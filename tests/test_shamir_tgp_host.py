"""CPU tier of the toggled Shamir grand product: the big-int restatement (tests/shamir_tgp_ref.py) proves itself -- n Shamir parties
produce the plain toggled prover's proof of the clear witness, the plain verifier accepts it, the final claims are the leaf
polynomials at the final point, every opening needs its 2t + 1 masked messages while the toggle layer's unmasked messages are of
degree t, M is the dense tree's count plus 4 per toggle round, and the king construct gives the same bytes -- and the new entry
points exist and refuse bad arguments on the host, with no device."""
import ctypes

import pytest

import pyref as O
import pysparse as SP
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S
import shamir_tgp_ref as T

R = O.R
# (n_pairs, N, density %, t, n)
SHAPES = [(1, 2, 50, 1, 3), (3, 8, 60, 2, 5), (2, 64, 15, 1, 4), (1, 16, 40, 7, 15), (2, 8, 0, 1, 3), (1, 4, 100, 1, 3)]
MUL_CTR, RAND_CTR = (1 << 33) + 5, (1 << 32) + 77


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "p%d-N%d-d%d-t%d-n%d" % s)
def world(request):
    n_pairs, n, density, degree, parties = request.param
    flags, vals = T.instance(7, n_pairs, n, density)
    flat = [v for row in vals for v in row]
    shares = S.share_vec(flat, S.keys_for(22, degree), degree, parties, counter=9)
    mk, rk = M.party_keys(3, parties, degree), D.party_keys(4, parties, degree)
    res = T.prove(flags, shares, n, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    toggles, sparse = SP.toggled_construct(flags, [vals])
    want, want_r = SP.toggled_prove(toggles, sparse, O.Transcript())
    return dict(n_pairs=n_pairs, n=n, degree=degree, parties=parties, flags=flags, vals=vals, shares=shares, mk=mk, rk=rk, res=res, want=want,
                want_r=want_r)


def test_restatement_gives_the_plain_toggled_provers_proof(world):
    res = world["res"]
    assert res["proof"] == world["want"] and res["r"] == world["want_r"]
    assert G.ser_proof(res["proof"]) == G.ser_proof(world["want"])
    assert SP.toggled_verify(res["proof"], O.Transcript()) == (res["flag"], res["fingerprint"], res["r"])
    assert (res["flag"], res["fingerprint"]) == SP.toggled_leaf_mles(world["flags"], world["vals"], res["r"])


def test_level_zero_opens_to_the_plain_toggle_output(world):
    degree, parties, n = world["degree"], world["parties"], world["n"]
    flat = [v for row in world["vals"] for v in row]
    pts = list(range(parties, parties - degree - 1, -1))  # the t + 1 highest parties
    level0 = world["res"]["layers"][0]
    assert S.combine_vec([level0[p - 1] for p in pts], pts, degree) == [x % R for x in T.toggle_output(world["flags"], flat, n)]


def test_every_opening_needs_its_masked_messages_and_the_toggle_messages_are_of_degree_t(world):
    res, degree = world["res"], world["degree"]
    k2 = G.senders(degree)
    lam2t = S.lagrange_from_coeff(list(range(1, k2 + 1)))
    lamt = S.lagrange_from_coeff(list(range(1, degree + 2)))
    assert all(len(m) == k2 for m in res["msgs"])
    opened = [S.reconstruct(m, lam2t) for m in res["msgs"]]
    batch = 2 * world["n_pairs"]
    assert opened[:batch] == res["proof"]["outputs"]
    # the unmasked values open to the same scalars; the masks are sharings of zero that differ from zero somewhere
    assert [S.reconstruct(l, lam2t) for l in res["locals"]] == opened
    assert any(m != l for m, l in zip(res["msgs"], res["locals"]))
    # the toggle layer's openings are the last 4 (nv + d): unmasked they are degree-t sharings of the plain prover's coefficients
    rounds = T.toggle_rounds(world["n_pairs"], world["n"])
    assert len(res["toggle_locals"]) == rounds == len(res["proof"]["layers"][-1]["round_polys"])
    tail = opened[len(opened) - 4 * rounds:]
    for j, co in enumerate(res["toggle_locals"]):
        for c in range(4):
            assert S.reconstruct(co[c][:degree + 1], lamt) == S.reconstruct(co[c], lam2t) == tail[4 * j + c]
    # the finals: the public flag and the degree-t fingerprint shares
    last = res["finals"][-1]
    assert len(last) == degree + 1 and all(f[0] == res["flag"] for f in last)
    assert S.reconstruct([f[1] for f in last], lamt) == res["fingerprint"]


def test_opening_count_matches_the_formula(world):
    n_pairs, n = world["n_pairs"], world["n"]
    batch = 2 * n_pairs
    nv, d = (batch - 1).bit_length(), n.bit_length() - 1
    M_ = G.num_openings(batch * n, batch) + 4 * (nv + d)
    assert T.num_openings(n_pairs, n) == M_ == len(world["res"]["msgs"])
    assert T.toggle_rounds(n_pairs, n) == nv + d == len(world["res"]["r"])


def test_king_construct_gives_the_same_proof_bytes(world):
    degree, parties, n = world["degree"], world["parties"], world["n"]
    pre = T.prep(world["rk"], degree, world["n_pairs"], n, rand_counter=RAND_CTR)
    assert pre["M"] == T.num_openings(world["n_pairs"], n) and pre["toggled"]
    assert pre["zero"] == G.zero_masks(world["rk"], degree, pre["M"], RAND_CTR)  # the resharing prover's masks
    for king in (0, parties - 1):
        res = T.prove_king(world["flags"], world["shares"], n, pre, degree, king=king)
        assert G.ser_proof(res["proof"]) == G.ser_proof(world["want"])
        assert (res["claim"], res["r"], res["flag"], res["fingerprint"]) == tuple(world["res"][k] for k in ("claim", "r", "flag", "fingerprint"))
        assert res["layers"][0][:G.senders(degree)] == world["res"]["layers"][0][:G.senders(degree)]
    with pytest.raises(AssertionError):  # a dense prep does not serve the toggled prover
        T.prove_king(world["flags"], world["shares"], n, dict(pre, toggled=False), degree)


# ------------------------------------------------------------------------------------------------ the ABI, without a device
SYMBOLS = ("cozk_shamir_tgp_prove_inproc", "cozk_shamir_tgp_prep_inproc", "cozk_shamir_tgp_prove_king_inproc", "cozk_shamir_gp_toggle_claims",
           "cozk_shamir_gp_get_toggle_stats")
SENT = 0x5A5A


def test_wrappers_exist(cozk):
    for name in ("shamir_tgp_prove", "shamir_tgp_prep", "shamir_tgp_prove_king"):
        assert callable(getattr(cozk, name))
    for sym in SYMBOLS:
        assert sym in cozk._lib.SIGNATURES and hasattr(cozk._lib.lib(), sym)
    assert [f[0] for f in cozk.ShamirGpToggleStats._fields_] == ["toggle_group_rounds", "toggle_single_rounds"]
    assert ctypes.sizeof(cozk.ShamirGpResult) == 40 and ctypes.sizeof(cozk.ShamirGpStats) == 32  # the existing structs have not grown


def test_null_and_out_of_range_arguments_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_tgp_prove_inproc(None, None, 1, None, None, None, 1, 3, 0, 0, b"cozk", 1, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_tgp_prove_inproc(None, None, 1, None, None, None, 1, 3, 0, 0, b"cozk", 1, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_tgp_prep_inproc(None, None, 1, 8, 1, 3, 0, ctypes.byref(h)) == -1 and h.value is None
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_tgp_prep_inproc(None, None, 1, 6, 1, 3, 0, ctypes.byref(h)) == -1 and h.value is None  # N not a power of two
    assert l.cozk_shamir_tgp_prep_inproc(None, None, 1, 8, 1, 3, 0, None) == -1
    h = ctypes.c_void_p(SENT)
    assert l.cozk_shamir_tgp_prove_king_inproc(None, None, 1, None, None, 0, b"cozk", 1, ctypes.byref(h)) == -1 and h.value is None
    assert l.cozk_shamir_tgp_prove_king_inproc(None, None, 1, None, None, 0, b"cozk", 1, None) == -1
    fl, fp = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    assert l.cozk_shamir_gp_toggle_claims(None, fl, fp) == -1
    assert l.cozk_shamir_gp_get_toggle_stats(None, ctypes.byref(cozk.ShamirGpToggleStats())) == -1
