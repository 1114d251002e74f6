"""Two blind spots of the PRF-fed kernels, against the big-int restatements (oracle/pyref.py, tests/shamir_*_ref.py); bit-exact:
  * counter + i crossing 2^32 INSIDE one vector: chacha12_block (csrc/prf.hip.hpp) splits the 64-bit counter into two state
    words, and every other test keeps a whole vector on one side of a carry between them;
  * every instantiation of the dealing kernel k_shamir_share<DEG, Src> (csrc/shamir.hip): DEG = 1..7 unrolled and the rolled
    variant at each degree 8..15 it serves, for all five sources."""
import functools

import pytest

import pyref as O
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S

pytestmark = pytest.mark.gpu

R = O.R
WRAP_COUNTER = (1 << 32) - 128  # elements 0..127 below the carry, 128..256 above
WRAP_N = 257


def _ints(vecs):
    return [v.to_ints() for v in vecs]


# ------------------------------------------------------------------------------------------------ counters across 2^32
def test_counter_crosses_2p32_in_the_stream_and_the_rep3_consumers(cozk, ctx):
    """bound: the counter's low word wraps and its high word takes the carry (prf.hip.hpp, chacha12_block's words 12 and 13)
    at element 128 of each vector: the PRF fill, the Rep3 dealing, the masked layer output and the masked local product"""
    n, ctr = WRAP_N, WRAP_COUNTER
    k0, k1 = O.harness_prf_key(61, 0), O.harness_prf_key(62, 0)
    s0, s1 = O.prf_fr_vec(k0, ctr, n), O.prf_fr_vec(k1, ctr, n)
    assert s0[128:] != O.prf_fr_vec(k0, 0, n - 128)  # the high word counts: a stream that drops the carry differs
    assert cozk.Vec.prf(ctx, n, k0, counter=ctr).to_ints() == s0
    v = O.synthetic_fr(4141, n)
    V = cozk.Vec.from_ints(ctx, v)
    exp = O.rep3_share_vec(v, k0, k1, counter=ctr)
    for p in range(3):
        a, b = V.rep3_share(k0, k1, p, counter=ctr)
        assert (a.to_ints(), b.to_ints()) == ([x[0] for x in exp[p]], [x[1] for x in exp[p]]), "party %d" % p
    # masked layer output: n outputs from 2 n interleaved coefficients, mask_j = PRF(key_self, ctr + j) - PRF(key_prev, ctr + j)
    coeffs = O.synthetic_fr(4242, 2 * n)
    layer = cozk.Rep3DenseInterleavedPolynomial.new(ctx, coeffs)
    got = layer.layer_output_local(masked=True, key_self=k0, key_prev=k1, counter=ctr).to_ints()
    plain = O.interleaved_layer_output_local(coeffs)
    assert len(plain) == n and got == [(x + a - b) % R for x, a, b in zip(plain, s0, s1)]
    # the local half of rep3 mul_vec with its zero-sharing mask
    rng = O.SplitMix64(4343)
    xs, ys = [(rng.field(), rng.field()) for _ in range(n)], [(rng.field(), rng.field()) for _ in range(n)]
    vec = lambda sh, c: cozk.Vec.from_ints(ctx, [s[c] for s in sh])
    got = cozk.rep3_mul_vec_local(ctx, vec(xs, 0), vec(xs, 1), vec(ys, 0), vec(ys, 1), key_self=k0, key_prev=k1, counter=ctr).to_ints()
    assert got == [(O.rep3_local_mul(x, y) + a - b) % R for x, y, a, b in zip(xs, ys, s0, s1)]


def test_counter_crosses_2p32_in_the_shamir_dealing_sources(cozk, ctx):
    """bound: as above (prf.hip.hpp, chacha12_block's words 12 and 13) through shamir_prf_fr (shamir.hip:55-73), the copy of the
    stream the dealing kernel inlines: share, mul-deal, pair-deal and both degrees of rand-deal"""
    n, ctr, degree, parties = WRAP_N, WRAP_COUNTER, 2, 5
    keys = S.keys_for(71, degree)
    v, w = O.synthetic_fr(4444, n), O.synthetic_fr(4545, n)
    V, W = cozk.Vec.from_ints(ctx, v), cozk.Vec.from_ints(ctx, w)
    assert _ints(V.shamir_share(keys, degree, parties, counter=ctr)) == S.share_vec(v, keys, degree, parties, counter=ctr)
    assert _ints(V.shamir_mul_deal(W, keys, degree, parties, counter=ctr)) == M.mul_deal(v, w, keys, degree, parties, counter=ctr)
    layer = [x for pair in zip(v, w) for x in pair]
    got = cozk.Vec.from_ints(ctx, layer).shamir_mul_deal_pairs(keys, degree, parties, counter=ctr)
    assert _ints(got) == G.mul_deal_pairs(layer, keys, degree, parties, counter=ctr)
    rkeys = S.keys_for(72, D.num_keys(degree))
    got_t, got_2t = cozk.shamir_rand_deal(ctx, n, rkeys, degree, parties, counter=ctr)
    want_t, want_2t = D.rand_deal(rkeys, degree, parties, n, counter=ctr)
    assert _ints(got_t) == want_t and _ints(got_2t) == want_2t


# ------------------------------------------------------------------------------------------------ every degree, every source
SWEEP_N = 65
SWEEP_COUNTER = 9
SWEEP_SEED = 73


@functools.lru_cache(maxsize=None)
def _streams():
    """the 22 PRF streams every degree's keys are a prefix of (S.keys_for(seed, d) = the first d keys), computed once"""
    return [O.prf_fr_vec(k, SWEEP_COUNTER, SWEEP_N) for k in S.keys_for(SWEEP_SEED, D.num_keys(7))]


@functools.lru_cache(maxsize=None)
def _factors():
    return O.synthetic_fr(4646, SWEEP_N - 4) + [0, 1, R - 1, R - 2], [R - 1, 2] + O.synthetic_fr(4747, SWEEP_N - 2)


@pytest.mark.parametrize("degree", range(1, 16))
def test_every_degree_of_every_dealing_source(cozk, ctx, degree):
    """k_shamir_share<DEG, Src> (shamir.hip:116-150): DEG = 3, 4, 5 and the rolled variant at 9..14 were never launched; here
    every degree 1..15 for share, eval, mul-deal and pair-deal, and 1..7 (2 t <= 15) for rand-deal, at 65 elements and
    2 degree + 1 parties"""
    n, parties, ctr = SWEEP_N, min(2 * degree + 1, 32), SWEEP_COUNTER
    st = _streams()
    keys = S.keys_for(SWEEP_SEED, degree)
    a, b = _factors()
    A, B = cozk.Vec.from_ints(ctx, a), cozk.Vec.from_ints(ctx, b)
    assert _ints(A.shamir_share(keys, degree, parties, counter=ctr)) == S.eval_vec([a] + st[:degree], parties)
    got = cozk.shamir_eval(ctx, [A] + [cozk.Vec.from_ints(ctx, c) for c in st[:degree]], parties)
    assert _ints(got) == S.eval_vec([a] + st[:degree], parties)
    prod = [x * y % R for x, y in zip(a, b)]
    assert _ints(A.shamir_mul_deal(B, keys, degree, parties, counter=ctr)) == S.eval_vec([prod] + st[:degree], parties)
    layer = [x for pair in zip(a, b) for x in pair]
    got = cozk.Vec.from_ints(ctx, layer).shamir_mul_deal_pairs(keys, degree, parties, counter=ctr)
    assert _ints(got) == S.eval_vec([prod] + st[:degree], parties)
    if 2 * degree <= 15:
        got_t, got_2t = cozk.shamir_rand_deal(ctx, n, S.keys_for(SWEEP_SEED, D.num_keys(degree)), degree, parties, counter=ctr)
        assert _ints(got_t) == S.eval_vec(st[:degree + 1], parties)
        assert _ints(got_2t) == S.eval_vec([st[0]] + st[degree + 1:3 * degree + 1], parties)
