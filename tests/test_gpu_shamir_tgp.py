"""GPU tests of the toggled Shamir grand product (cozk_shamir_tgp_prove_inproc, cozk_shamir_tgp_prep_inproc,
cozk_shamir_tgp_prove_king_inproc, cozk_shamir_gp_toggle_claims, cozk_shamir_gp_get_toggle_stats) against the big-int restatement
tests/shamir_tgp_ref.py and, through it, the plain toggled oracle (oracle/pysparse.py).  Every shape runs with the toggle layer as ONE
toggle group and again with COZK_SHAMIR_GP_GROUP=0, a PLAIN toggle layer per sender; the stats count the calls made, so a silent
fall-back cannot hide.  Bar: bit-exact.  No test provokes a device fault: every bad argument is refused on the host before any launch."""
import ctypes
import functools

import pytest

import pyref as O
import pysparse as SP
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_mul_ref as M
import shamir_ref as S
import shamir_tgp_ref as T
from test_gpu_shamir_gp import MUL_CTR, RAND_CTR, SENT, _expect_invalid, _ints, party_ctxs  # noqa: F401

pytestmark = pytest.mark.gpu
R = O.R
SWITCH = "COZK_SHAMIR_GP_GROUP"
# (n_pairs, N, density %, t, n): the first five shapes of tests/test_shamir_tgp_host.py; the king's construct at the first three
SMALL = [(1, 2, 50, 1, 3), (3, 8, 60, 2, 5), (2, 64, 15, 1, 4), (1, 16, 40, 7, 15), (2, 8, 0, 1, 3)]
LARGE = (2, 4096, 10, 2, 8)


@pytest.fixture(scope="module")
def many_ctxs(cozk, party_ctxs):
    """15 parties for the (t, n) = (7, 15) shape: the module's eight contexts and seven more"""
    extra = [cozk.Context(0) for _ in range(7)]
    yield list(party_ctxs) + extra
    for c in extra:
        c.close()


@functools.lru_cache(maxsize=None)
def _world(shape):
    """the clear instance, the keys, and the plain oracle's proof bytes"""
    n_pairs, n, density, degree, parties = shape
    flags, vals = T.instance(7, n_pairs, n, density)
    toggles, sparse = SP.toggled_construct(flags, [vals])
    want, want_r = SP.toggled_prove(toggles, sparse, O.Transcript())
    return dict(flags=flags, vals=vals, flat=[v for row in vals for v in row], mk=M.party_keys(3, parties, degree), rk=D.party_keys(4, parties, degree),
                want=G.ser_proof(want), want_r=want_r)


def _device_inputs(cozk, ctx, pcs, shape):
    n_pairs, n, density, degree, parties = shape
    w = _world(shape)
    fl = [cozk.Vec.from_ints(pcs[0], [1 if i in set(s) else 0 for i in range(n)], kind=cozk.SCALAR_U8) for s in w["flags"]]
    fps = cozk.Vec.from_ints(ctx, w["flat"]).shamir_scatter(S.keys_for(22, degree), degree, pcs, counter=9)
    return fl, fps


def _prove(cozk, pcs, fl, fps, shape, king):
    n_pairs, n, density, degree, parties = shape
    w = _world(shape)
    if king is None:
        return cozk.shamir_tgp_prove(pcs, fl, fps, w["mk"], w["rk"], degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    prep = cozk.shamir_tgp_prep(pcs, w["rk"], n_pairs, n, degree, rand_counter=RAND_CTR)
    try:
        assert prep.result.n_openings == T.num_openings(n_pairs, n)
        got = cozk.shamir_tgp_prove_king(pcs, fl, fps, prep, king=king)
        assert (prep.result.used, prep.result.pairs_held) == (1, 0)
        return got
    finally:
        prep.close()


def _both_ways(cozk, ctx, pcs, shape, king, monkeypatch):
    """grouped, ungrouped, and grouped again with the switch set to something other than 0: identical in everything, the stats aside"""
    n_pairs, n, density, degree, parties = shape
    fl, fps = _device_inputs(cozk, ctx, pcs, shape)
    shares = _ints(fps)
    monkeypatch.delenv(SWITCH, raising=False)
    grouped = _prove(cozk, pcs, fl, fps, shape, king)
    monkeypatch.setenv(SWITCH, "0")
    single = _prove(cozk, pcs, fl, fps, shape, king)
    monkeypatch.setenv(SWITCH, "1")
    again = _prove(cozk, pcs, fl, fps, shape, king)
    monkeypatch.delenv(SWITCH)
    for got in (single, again):
        assert got.proof_bytes == grouped.proof_bytes and (got.claim, got.r) == (grouped.claim, grouped.r)
        assert got.msgs == grouped.msgs and got.finals == grouped.finals and got.toggle_claims == grouped.toggle_claims
        assert got.result.verified == 1
    assert grouped.result.verified == 1
    batch = 2 * n_pairs
    tr = T.toggle_rounds(n_pairs, n)
    layers = n.bit_length() - 1  # dense layers
    rounds = (grouped.result.n_opened - batch) // 4 - tr
    assert grouped.result.n_opened == T.num_openings(n_pairs, n) and grouped.result.n_layers == layers + 1
    assert rounds == sum(range((batch - 1).bit_length(), (batch - 1).bit_length() + layers))
    for got in (grouped, again):
        s, ts = got.stats, got.toggle_stats
        assert (ts.toggle_group_rounds, ts.toggle_single_rounds) == (tr, 0)
        assert (s.group_rounds, s.group_finals, s.single_rounds, s.single_finals) == (rounds, layers, 0, 0)
    s, ts = single.stats, single.toggle_stats
    assert (ts.toggle_group_rounds, ts.toggle_single_rounds) == (0, (2 * degree + 1) * tr)
    assert (s.group_rounds, s.group_finals, s.single_rounds, s.single_finals) == (0, 0, (2 * degree + 1) * rounds, (degree + 1) * layers)
    assert _ints(fps) == shares  # the fingerprints are only read
    assert [v.to_ints() for v in fl] == [[1 if i in set(s) else 0 for i in range(n)] for s in _world(shape)["flags"]]
    return grouped, shares


def _against_ref(got, ref, shape):
    w = _world(shape)
    assert got.proof_bytes == G.ser_proof(ref["proof"]) == w["want"]  # the plain toggled prover's proof, byte for byte
    assert (got.claim, got.r) == (ref["claim"], ref["r"]) and got.r == w["want_r"]
    assert got.msgs == ref["msgs"]  # the masks, their order, the counters
    assert got.finals == ref["finals"]
    assert got.toggle_claims == (ref["flag"], ref["fingerprint"]) == SP.toggled_leaf_mles(w["flags"], w["vals"], got.r)
    assert got.result.proof_len == len(w["want"])


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_shamir_tgp_prove_grouped_and_ungrouped(cozk, ctx, many_ctxs, shape, monkeypatch):
    n_pairs, n, density, degree, parties = shape
    got, shares = _both_ways(cozk, ctx, many_ctxs[:parties], shape, None, monkeypatch)
    w = _world(shape)
    _against_ref(got, T.prove(w["flags"], shares, n, w["mk"], w["rk"], degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR), shape)


@pytest.mark.parametrize("last", [False, True], ids=["king-first", "king-last"])
@pytest.mark.parametrize("shape", SMALL[:3], ids=str)
def test_shamir_tgp_prove_king_grouped_and_ungrouped(cozk, ctx, many_ctxs, shape, last, monkeypatch):
    n_pairs, n, density, degree, parties = shape
    king = parties - 1 if last else 0
    got, shares = _both_ways(cozk, ctx, many_ctxs[:parties], shape, king, monkeypatch)
    w = _world(shape)
    _against_ref(got, T.prove_king(w["flags"], shares, n, T.prep(w["rk"], degree, n_pairs, n, rand_counter=RAND_CTR), degree, king=king), shape)


def test_shamir_tgp_large_grouped_equals_ungrouped(cozk, ctx, party_ctxs, monkeypatch):
    """layers above 2048 elements and a toggle layer of several workgroups and two member chunks.  The n-party big-int restatement is
    too slow at this size: the ungrouped run and the device's own replay of the plain verifier are the yardsticks"""
    n_pairs, n, density, degree, parties = LARGE
    fl = [cozk.Vec.from_ints(party_ctxs[0], [1 if O.SplitMix64(90 + q * n + i).next() % 100 < density else 0 for i in range(n)], kind=cozk.SCALAR_U8)
          for q in range(n_pairs)]
    fps = cozk.Vec.from_ints(ctx, O.synthetic_fr(35, 2 * n_pairs * n)).shamir_scatter(S.keys_for(36, degree), degree, party_ctxs, counter=1)
    mk, rk = M.party_keys(5, parties, degree), D.party_keys(6, parties, degree)
    run = lambda: cozk.shamir_tgp_prove(party_ctxs, fl, fps, mk, rk, degree, mul_counter=MUL_CTR, rand_counter=RAND_CTR)
    monkeypatch.delenv(SWITCH, raising=False)
    grouped = run()
    monkeypatch.setenv(SWITCH, "0")
    single = run()
    monkeypatch.delenv(SWITCH)
    assert grouped.result.verified == 1 and single.result.verified == 1
    assert grouped.proof_bytes == single.proof_bytes and grouped.msgs == single.msgs and grouped.finals == single.finals
    assert (grouped.claim, grouped.r, grouped.toggle_claims) == (single.claim, single.r, single.toggle_claims)
    tr = T.toggle_rounds(n_pairs, n)
    assert (grouped.toggle_stats.toggle_group_rounds, grouped.toggle_stats.toggle_single_rounds) == (tr, 0)
    assert (single.toggle_stats.toggle_group_rounds, single.toggle_stats.toggle_single_rounds) == (0, 5 * tr)
    assert grouped.stats.single_rounds == 0 and single.stats.group_rounds == 0


def test_dense_proof_has_no_toggle_claims(cozk, ctx, party_ctxs):
    pcs = party_ctxs[:3]
    leaves = cozk.Vec.from_ints(ctx, G.leaves(21, 1, 4)).shamir_scatter(S.keys_for(22, 1), 1, pcs, counter=9)
    got = cozk.shamir_gp_prove(pcs, leaves, 1, M.party_keys(3, 3, 1), D.party_keys(4, 3, 1), 1)
    assert got.toggle_claims is None  # cozk_shamir_gp_toggle_claims refuses a dense proof's handle
    assert (got.toggle_stats.toggle_group_rounds, got.toggle_stats.toggle_single_rounds) == (0, 0)


def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l = cozk._lib.lib()
    pcs = party_ctxs[:3]
    p0 = pcs[0]
    mkv = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    arr = lambda hs: (ctypes.c_void_p * 40)(*(list(hs) + [None] * (40 - len(hs))))
    hs = lambda vs: arr([x.h.value if x is not None else None for x in vs])
    three_ctxs = arr([c.h.value for c in pcs])
    F = [mkv(p0, [1, 0, 1, 1], cozk.SCALAR_U8)]          # one pair, N = 4
    good = [mkv(c, list(range(1, 9))) for c in pcs]       # 2 circuits x 4
    kb = ctypes.create_string_buffer(b"\x02" * (32 * 22), 32 * 22)
    kp = [ctypes.addressof(kb)] * 3

    def tgp(parties, deg, flags, n_pairs, fps, mkeys, rkeys, text, ctxs=None, label=b"cozk"):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_tgp_prove_inproc(three_ctxs if ctxs is None else ctxs, hs(flags) if flags is not None else None, n_pairs,
                                            hs(fps) if fps is not None else None, arr(mkeys), arr(rkeys), deg, parties, 0, 0, label, 1, ctypes.byref(h))
        _expect_invalid(cozk, p0, rc, "shamir_tgp_prove_inproc: " + text)
        assert h.value is None

    tgp(3, 1, None, 1, good, kp, kp, "null argument")
    tgp(3, 1, F, 1, None, kp, kp, "null argument")
    tgp(3, 1, F, 1, good, kp, kp, "null argument", label=None)
    tgp(3, 1, F, 0, good, kp, kp, "n_pairs == 0")
    tgp(3, 1, F, 1, [good[0], None, good[2]], kp, kp, "parties 0..2 * degree need their fingerprints and their key block")
    tgp(3, 1, F, 1, good, [kp[0], None, kp[2]], kp, "parties 0..2 * degree need their fingerprints and their key block")
    tgp(3, 1, F, 1, good, kp, [kp[0], kp[1], None], "every party needs its mask key block")
    tgp(3, 1, F, 1, [good[0], mkv(pcs[1], [1, 2]), good[2]], kp, kp, "the fingerprints must have one length")
    tgp(3, 1, F, 1, [good[0], good[1], mkv(pcs[2], list(range(8)), cozk.SCALAR_U32)], kp, kp, "the fingerprints must be FR vectors")
    tgp(3, 1, F, 1, [good[0], good[0], good[2]], kp, kp, "party p's fingerprints must be a vector of party_ctxs[p]")
    tgp(3, 1, F * 3, 3, good, kp, kp, "fingerprints.len() must be 2 * n_pairs * N")
    tgp(3, 1, [mkv(p0, [1, 0, 1], cozk.SCALAR_U8)], 1, [mkv(c, list(range(1, 7))) for c in pcs], kp, kp, "fingerprints per circuit must be a power of two >= 2")
    tgp(3, 1, [mkv(p0, [1, 0], cozk.SCALAR_U8)], 1, good, kp, kp, "every flag column is a U8 vector of N entries")
    tgp(3, 1, [mkv(p0, [1, 0, 1, 1], cozk.SCALAR_U32)], 1, good, kp, kp, "every flag column is a U8 vector of N entries")
    tgp(3, 1, [mkv(pcs[1], [1, 0, 1, 1], cozk.SCALAR_U8)], 1, good, kp, kp, "the flag columns must be vectors of party_ctxs[0]")
    tgp(3, 1, F, 1, good, kp, kp, "null party context", ctxs=arr([pcs[0].h.value, pcs[1].h.value, None]))
    tgp(3, 0, F, 1, good, kp, kp, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")
    tgp(4, 2, F, 1, good, kp, kp, "2 * degree + 1 <= num_parties")
    assert l.cozk_shamir_tgp_prove_inproc(three_ctxs, hs(F), 1, hs(good), arr(kp), arr(kp), 1, 3, 0, 0, b"cozk", 1, None) == -1

    def prep(parties, deg, n_pairs, n_per, rkeys, text):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shamir_tgp_prep_inproc(three_ctxs, arr(rkeys) if rkeys is not None else None, n_pairs, n_per, deg, parties, 0, ctypes.byref(h))
        _expect_invalid(cozk, p0, rc, "shamir_tgp_prep_inproc: " + text)
        assert h.value is None

    prep(3, 1, 0, 4, kp, "n_pairs > 0 and N a power of two >= 2")
    prep(3, 1, 1, 6, kp, "n_pairs > 0 and N a power of two >= 2")
    prep(3, 1, 1, 1, kp, "n_pairs > 0 and N a power of two >= 2")
    prep(3, 1, 1, 4, None, "null argument")
    prep(3, 0, 1, 4, kp, "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE")

    # the two kinds of preprocessing serve their own prover only; a used one serves nothing
    keys = D.party_keys(8, 3, 1)
    dense = cozk.shamir_gp_prep(pcs, keys, 8, 2, 1)
    toggled = cozk.shamir_tgp_prep(pcs, keys, 1, 4, 1)
    assert toggled.result.n_openings == T.num_openings(1, 4) == dense.result.n_openings + 4 * 3

    def king(prep_h, flags, n_pairs, fps, king_id, text, fn="tgp"):
        h = ctypes.c_void_p(SENT)
        if fn == "tgp":
            rc = l.cozk_shamir_tgp_prove_king_inproc(three_ctxs, hs(flags), n_pairs, hs(fps), prep_h, king_id, b"cozk", 1, ctypes.byref(h))
            _expect_invalid(cozk, p0, rc, "shamir_tgp_prove_king_inproc: " + text)
        else:
            rc = l.cozk_shamir_gp_prove_king_inproc(three_ctxs, hs(fps), 2, prep_h, king_id, b"cozk", 1, ctypes.byref(h))
            _expect_invalid(cozk, p0, rc, "shamir_gp_prove_king_inproc: " + text)
        assert h.value is None and (dense.result.used, toggled.result.used) == (0, 0)

    king(dense.h, F, 1, good, 0, "the preprocessing was made for a dense grand product")
    king(toggled.h, F, 1, good, 0, "the preprocessing was made for a toggled grand product", fn="gp")
    king(None, F, 1, good, 0, "null argument")
    king(toggled.h, F, 1, good, 3, "0 <= king < num_parties")
    king(toggled.h, F * 2, 2, [mkv(c, list(range(1, 17))) for c in pcs], 0, "the preprocessing was made for another (n_pairs, N)")
    king(toggled.h, [mkv(p0, [1, 0], cozk.SCALAR_U8)], 1, [mkv(c, [1, 2, 3, 4]) for c in pcs], 0, "the preprocessing was made for another (n_pairs, N)")
    king(toggled.h, [mkv(p0, [1, 0], cozk.SCALAR_U8)], 1, good, 0, "every flag column is a U8 vector of N entries")
    assert _ints(good) == [list(range(1, 9))] * 3  # nothing ran
    assert cozk.shamir_tgp_prove_king(pcs, F, good, toggled).result.verified == 1  # the prep still serves its one proof
    h = ctypes.c_void_p(SENT)
    _expect_invalid(cozk, p0, l.cozk_shamir_tgp_prove_king_inproc(three_ctxs, hs(F), 1, hs(good), toggled.h, 0, b"cozk", 1, ctypes.byref(h)),
                    "shamir_tgp_prove_king_inproc: the preprocessing has been used")
    assert h.value is None
    assert cozk.shamir_gp_prove_king(pcs, good, 2, dense).result.verified == 1
    dense.close()
    toggled.close()


def test_senders_on_two_gpus_take_the_per_sender_path(cozk, ctx, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    shape = SMALL[1]
    n_pairs, n, density, degree, parties = shape
    pcs = [cozk.Context(p % 2) for p in range(parties)]
    try:
        monkeypatch.delenv(SWITCH, raising=False)
        fl, fps = _device_inputs(cozk, ctx, pcs, shape)
        got = _prove(cozk, pcs, fl, fps, shape, None)
        w = _world(shape)
        assert got.proof_bytes == w["want"] and got.result.verified == 1
        tr = T.toggle_rounds(n_pairs, n)
        assert (got.toggle_stats.toggle_group_rounds, got.toggle_stats.toggle_single_rounds) == (0, (2 * degree + 1) * tr)
        assert got.stats.group_rounds == 0
        del fl, fps
    finally:
        for c in pcs:
            c.close()
