"""GPU tests of the Shamir grand product provers on layer groups (cozk_layer_group_round / _final behind
cozk_shamir_gp_prove_inproc and cozk_shamir_gp_prove_king_inproc): every shape runs grouped and again with COZK_SHAMIR_GP_GROUP=0,
which selects the per-sender loop.  Proof bytes, messages and final-claim shares are equal between the two, equal to the big-int
restatements (tests/shamir_gp_ref.py, tests/shamir_gp_king_ref.py) at the small shapes and to the plain oracle's proof at all of
them; cozk_shamir_gp_get_stats counts the calls made, so a silent fall-back cannot hide."""
import functools

import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_king_ref as K
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S
from test_gpu_shamir_gp import MUL_CTR, RAND_CTR, _ints, _oracle_proof, party_ctxs  # noqa: F401

pytestmark = pytest.mark.gpu
SWITCH = "COZK_SHAMIR_GP_GROUP"
# (parties, degree, batch, leaves per circuit): a layer without rounds; ...; layers above 2048 elements
SMALL = [(3, 1, 1, 2), (3, 1, 2, 16), (5, 2, 4, 8), (7, 3, 2, 8)]
LARGE = (8, 2, 2, 1 << 11)
KING = {3: 1, 5: 2, 7: 3, 8: 5}


@functools.lru_cache(maxsize=None)
def _plain(shape):
    parties, degree, batch, per = shape
    return tuple(O.synthetic_fr(33, batch * per) if shape == LARGE else G.leaves(21, batch, per))


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    return _oracle_proof(list(_plain(shape)), shape[2])


def _keys(shape):
    parties, degree = shape[:2]
    return M.party_keys(3, parties, degree), D.party_keys(4, parties, degree)


def _leaves(cozk, ctx, pcs, shape):
    return cozk.Vec.from_ints(ctx, list(_plain(shape))).shamir_scatter(S.keys_for(22, shape[1]), shape[1], pcs, counter=9)


def _prove(cozk, pcs, leaves, shape, king):
    parties, degree, batch, per = shape
    mk, rk = _keys(shape)
    if not king:
        return cozk.shamir_gp_prove(pcs, leaves, batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    prep = cozk.shamir_gp_prep(pcs, rk, batch * per, batch, degree, rand_counter=RAND_CTR)
    try:
        return cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=KING[parties])
    finally:
        prep.close()


def _both_ways(cozk, ctx, party_ctxs, shape, king, monkeypatch):
    parties, degree, batch, per = shape
    pcs = party_ctxs[:parties]
    leaves = _leaves(cozk, ctx, pcs, shape)
    monkeypatch.delenv(SWITCH, raising=False)
    grouped = _prove(cozk, pcs, leaves, shape, king)
    monkeypatch.setenv(SWITCH, "0")
    single = _prove(cozk, pcs, leaves, shape, king)
    monkeypatch.setenv(SWITCH, "1")  # anything but 0 leaves the groups on
    again = _prove(cozk, pcs, leaves, shape, king)
    monkeypatch.delenv(SWITCH)
    want_bytes, want_claim, want_r = _oracle(shape)
    for got in (grouped, single, again):
        assert got.proof_bytes == want_bytes  # the plain prover's proof, byte for byte
        assert got.result.verified == 1 and (got.claim, got.r) == (want_claim, want_r)
    assert grouped.msgs == single.msgs == again.msgs and grouped.finals == single.finals == again.finals
    layers = grouped.result.n_layers
    rounds = (grouped.result.n_opened - batch) // 4
    assert layers == per.bit_length() - 1 and rounds == sum(range((batch - 1).bit_length(), (batch - 1).bit_length() + layers))
    for got in (grouped, again):
        s = got.stats
        assert (s.group_rounds, s.group_finals, s.single_rounds, s.single_finals) == (rounds, layers, 0, 0)
    s = single.stats
    assert (s.group_rounds, s.group_finals, s.single_rounds, s.single_finals) == (0, 0, (2 * degree + 1) * rounds, (degree + 1) * layers)
    return grouped, _ints(leaves)


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_shamir_gp_grouped_equals_ungrouped(cozk, ctx, party_ctxs, shape, monkeypatch):
    parties, degree, batch, per = shape
    got, shares = _both_ways(cozk, ctx, party_ctxs, shape, False, monkeypatch)
    mk, rk = _keys(shape)
    ref = G.prove(shares, batch, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    assert got.msgs == ref["msgs"] and got.finals == ref["finals"]


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_shamir_gp_king_grouped_equals_ungrouped(cozk, ctx, party_ctxs, shape, monkeypatch):
    parties, degree, batch, per = shape
    got, shares = _both_ways(cozk, ctx, party_ctxs, shape, True, monkeypatch)
    ref = K.prove(shares, batch, K.prep(_keys(shape)[1], degree, batch * per, batch, rand_counter=RAND_CTR), degree, king=KING[parties])
    assert got.msgs == ref["msgs"] and got.finals == ref["finals"]


@pytest.mark.parametrize("king", [False, True], ids=["reshare", "king"])
def test_shamir_gp_grouped_large_layers(cozk, ctx, party_ctxs, king, monkeypatch):
    """layers above 2048 elements: the members' large launches back to back on one reservation, then the hand-over to the one-launch
    kernel.  The n-party big-int restatement is too slow at this size: the plain oracle's proof and the ungrouped run are the yardsticks"""
    _both_ways(cozk, ctx, party_ctxs, LARGE, king, monkeypatch)
