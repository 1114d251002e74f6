"""The sparse pair layers (cozk_sparse_layer_*, csrc/sparse_layer.inc) at the borders of their own launch structure, bit-exact
against oracle/pysparse.py (or, at the one size the oracle cannot reach, against the restatement that
tests/test_sparse_tiles_model.py pins to it).

Every structural kernel is a stream compaction over tiles of T = SP_TILE = 2048 list items (8 rows of PT = 256 items, waves of 64):
a count per tile, one workgroup that scans the tile counts, consumers that place each flagged item with ballots, per-wave counts
and a running tile offset, and sp_group, which reads idx[i - 1] and idx[i + 1] and so may find the other half of a group across a
wave, a row or a tile.  tests/sparse_tiles_ref.py builds index lists that put a group on each of those borders; the layers are
made from explicit lists (SparseLayer.from_lists), one per party, with the parties' shares given, so every party's values must
equal the oracle's party bit for bit.

  a. rounds, binds and to_dense in every round: an exact tile, a tile with one item, three tiles
  b. output_local and from_output one level up; the 64-bit mask counter across 2^32
  c. the grid stride of k_sparse_cubic: COZK_SUM_GRID_MAX = 3 (a stride of 768 items, up to six passes per lane) and 1
  d. the toggle route (from_toggle) over four tiles of pairs with placed flags
  e. the scan with more than one tile per lane: 1024 T + 1 items"""
import functools
import importlib

import numpy as np
import pytest

import pyref as O
import pysparse as S
import sparse_tiles_ref as P

pytestmark = pytest.mark.gpu
R = O.R
T = P.T
GRID = "COZK_SUM_GRID_MAX"
KEYS = [bytes([29 * (p + 1) + i for i in range(32)]) for p in range(3)]  # KEYS[p]: shared by party p and party p + 1
MODES = {"plain": 1, "rep3": 3}

# the smallest counts that give an exact tile, a tile with one item, and three tiles
ROUND_CASES = [(pat, cnt) for pat in ("full", "odd_shift") for cnt in (T - 1, T, T + 1)] + [(pat, 2 * T + 1) for pat in ("evens", "odds", "mixed")]
OUTPUT_CASES = [("odd_shift", T + 1), ("mixed", 2 * T + 1)]


def _lk():
    return importlib.import_module("co-zkvms_amd.lookups")


def _engine():
    return importlib.import_module("co-zkvms_amd.engine")


@functools.lru_cache(maxsize=None)
def _case(pattern, cnt, nparties):
    """(idx, per party the pairs): built once per case and never changed"""
    return P.PATTERNS[pattern](cnt), P.share_pairs(cnt, 1000 + cnt + nparties, nparties)


def _layers(ctx, idx, shares):
    LK = _lk()
    return [LK.SparseLayer.from_lists(ctx, P.dense_len(idx), idx, pairs) for pairs in shares]


def _refs(idx, shares):
    return [P.oracle_layer(idx, shares[p], p, len(shares)) for p in range(len(shares))]


def _free(*objs):
    for o in objs:
        o.free()


# ------------------------------------------------------------------------------------------------ a. rounds and binds
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("pattern,cnt", ROUND_CASES)
def test_rounds_binds_and_dense_layers_match_the_oracle_per_party(cozk, ctx, pattern, cnt, mode):
    idx, shares = _case(pattern, cnt, MODES[mode])
    devs = _layers(ctx, idx, shares)
    assert all((len(d), d.count) == (P.dense_len(idx), cnt) for d in devs)
    forms = P.sumcheck(cozk, ctx, devs, _refs(idx, shares), 300 + cnt, exact=True)
    assert forms == {"flat", "nested"}  # a power-of-two length runs to the last round
    _free(*devs)


def test_next_count_is_the_number_of_merged_groups(cozk, ctx):
    for pattern, cnt in ROUND_CASES:
        idx, shares = _case(pattern, cnt, 1)
        sp = _layers(ctx, idx, shares)[0]
        assert sp.next_count() == len(set(j >> 1 for j in idx)), (pattern, cnt)
        sp.free()


# ------------------------------------------------------------------------------------------------ b. one level up
@functools.lru_cache(maxsize=None)
def _mask_stream(p, n):
    """prf(key_self, c) - prf(key_prev, c) of party p at the n counters from COUNTER on"""
    mine, prev = (_prf_stream(k, n) for k in (p, (p + 2) % 3))
    return [(a - b) % R for a, b in zip(mine, prev)]


@functools.lru_cache(maxsize=None)
def _prf_stream(k, n):
    return O.prf_fr_vec(KEYS[k], COUNTER, n)


COUNTER = 2**32 - 7  # the mask counter ctr + 2 * pos crosses 2^32 at the fourth group of the list


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("pattern,cnt", OUTPUT_CASES)
def test_output_local_and_the_next_layer_match_the_oracle(cozk, ctx, pattern, cnt, mode):
    nparties = MODES[mode]
    idx, shares = _case(pattern, cnt, nparties)
    devs, refs = _layers(ctx, idx, shares), _refs(idx, shares)
    n = P.dense_len(idx)
    groups = sorted(set(j >> 1 for j in idx))
    G = len(groups)
    for p in range(nparties):  # a Rep3 layer from lists learns its party here
        d = devs[p].to_dense(party=p)
        assert d.coeffs() == refs[p].coalesce()
        d.free()
    nxt_ref = S.sparse_layer_output(refs)  # zero masks: (local product, the previous party's local product)
    nxt_dense = [r.coalesce() for r in nxt_ref]
    assert all(d.next_count() == G for d in devs)

    plain_vecs = [devs[p].output_local(masked=False) for p in range(nparties)]
    plain = [v.to_ints() for v in plain_vecs]
    for p in range(nparties):
        local = [v[0] if nparties == 3 else v for v in nxt_dense[p]]
        assert plain[p] == [local[e] for q in groups for e in (2 * q, 2 * q + 1)], p  # the oracle's local products, a missing pair = add_one
        assert plain[p] == P.output(idx, shares[p], P.add_one(p, nparties))[1], p

    E = _engine()
    if nparties == 1:
        nxt = [devs[0].from_output(plain_vecs[0])]
        masked_vecs = junk = []
    else:
        # unmasked products, reshared (c.b = the previous party's c.a): the oracle's next layer bit for bit
        host = [v.to_numpy() for v in plain_vecs]
        vbs = [E.Vec.from_numpy(ctx, host[(p + 2) % 3]) for p in range(3)]
        nxt = [devs[p].from_output(plain_vecs[p], vbs[p]) for p in range(3)]
        junk = list(vbs)
        masked_vecs = [devs[p].output_local(masked=True, key_self=KEYS[p], key_prev=KEYS[(p + 2) % 3], counter=COUNTER) for p in range(3)]
        masked = [v.to_ints() for v in masked_vecs]
        assert COUNTER + 2 * G > 2**32 > COUNTER
        for p in range(3):
            assert len(masked[p]) == 2 * G
            assert masked[p] == [(v + m) % R for v, m in zip(plain[p], _mask_stream(p, 2 * G))], p
        assert [sum(c) % R for c in zip(*masked)] == [sum(c) % R for c in zip(*plain)]  # the masks cancel
        host = [v.to_numpy() for v in masked_vecs]
        vbs = [E.Vec.from_numpy(ctx, host[(p + 2) % 3]) for p in range(3)]
        nxt_masked = [devs[p].from_output(masked_vecs[p], vbs[p]) for p in range(3)]
        junk += vbs
        got = []
        for p in range(3):
            assert nxt_masked[p].download()[0] == groups
            d = nxt_masked[p].to_dense(party=p)
            got.append(d.coeffs())
            d.free()
        assert P.opened(got) == P.opened(nxt_dense)  # the masked next layer opens to the oracle's
        _free(*nxt_masked)
    for p in range(nparties):
        assert (len(nxt[p]), nxt[p].count) == (n // 2, G)
        assert nxt[p].download()[0] == groups  # unique(idx >> 1)
        d = nxt[p].to_dense(party=p)
        assert d.coeffs() == nxt_dense[p], p
        d.free()
    _free(*nxt, *plain_vecs, *masked_vecs, *junk, *devs)


# ------------------------------------------------------------------------------------------------ c. the stride of k_sparse_cubic
STRIDE_ROUNDS = 4


def _stride_setup(nparties):
    idx, shares = _case("mixed", 2 * T + 1, nparties)
    n = P.dense_len(idx)
    rng = O.SplitMix64(77)
    w = [rng.field() for _ in range((n // 2 - 1).bit_length())]
    return idx, shares, w, rng.field(), [rng.field() for _ in range(STRIDE_ROUNDS)]


@functools.lru_cache(maxsize=None)
def _stride_oracle(nparties):
    idx, shares, w, claim, rs = _stride_setup(nparties)
    refs, eqs = _refs(idx, shares), [O.SplitEq(w) for _ in range(nparties)]
    out = []
    for k in range(STRIDE_ROUNDS):
        evs = [refs[p].compute_cubic_evals(eqs[p], claim) for p in range(nparties)]
        out.append([[e[0], e[2], e[3]] for e in evs])
        for p in range(nparties):
            refs[p].bind(rs[k])
            eqs[p].bind(rs[k])
    return out


def _stride_device(cozk, ctx, nparties):
    idx, shares, w, _, rs = _stride_setup(nparties)
    devs = _layers(ctx, idx, shares)
    eqs = [cozk.SplitEqPolynomial(ctx, w) for _ in range(nparties)]
    out, r = [], None
    for k in range(STRIDE_ROUNDS):
        out.append([devs[p].round(eqs[p], r, party=p) for p in range(nparties)])
        r = rs[k]
    _free(*devs, *eqs)
    return out


@pytest.mark.parametrize("cap", [3, 1])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_capped_cubic_grid_strides_over_the_whole_list(cozk, ctx, monkeypatch, mode, cap):
    """4097 items are 17 workgroups of PT lanes; capped at 3 the stride is 768 items, which aligns with no tile, and a lane makes
    up to six passes; capped at 1 it makes 17"""
    nparties = MODES[mode]
    monkeypatch.delenv(GRID, raising=False)
    free = _stride_device(cozk, ctx, nparties)
    monkeypatch.setenv(GRID, str(cap))  # read on every call
    capped = _stride_device(cozk, ctx, nparties)
    want = _stride_oracle(nparties)
    for k in range(STRIDE_ROUNDS):
        assert capped[k] == want[k], k
        assert capped[k] == free[k], k


# ------------------------------------------------------------------------------------------------ d. the toggle route
@functools.lru_cache(maxsize=None)
def _toggle_case(batch, n, nparties):
    cols = P.toggle_columns(batch, n)
    rng = O.SplitMix64(batch + n + nparties)
    if nparties == 1:
        fps = [[[rng.field() for _ in range(n)] for _ in range(batch)]]
    else:
        sh = [[O.rep3_share(rng.field(), rng) for _ in range(n)] for _ in range(batch)]
        fps = [[[s[p] for s in row] for row in sh] for p in range(3)]
    _, sparse = S.toggled_construct([[i for i, f in enumerate(c) if f] for c in cols], fps)
    return cols, fps, sparse[0]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("batch,n", [(4, 4096), (8, 2048)])
def test_toggle_route_over_four_tiles_of_pairs(cozk, ctx, batch, n, mode):
    LK = _lk()
    nparties = MODES[mode]
    cols, fps, layer0 = _toggle_case(batch, n, nparties)
    want_idx = P.stored_pairs(cols, batch, n)
    tgs = [LK.ToggleLayer(ctx, cols, fps[p]) for p in range(nparties)]
    devs = [LK.SparseLayer.from_toggle(ctx, tgs[p], party=p) for p in range(nparties)]
    for p in range(nparties):
        assert (len(devs[p]), devs[p].count) == (batch * n, len(want_idx))
        idx, pairs = devs[p].download()
        assert idx == want_idx
        ref = tgs[p].layer_output(party=p)
        dense = ref.coeffs()
        ref.free()
        assert dense == layer0[p].coalesce()
        assert pairs == [(dense[2 * j], dense[2 * j + 1]) for j in idx]
    # round 0 and one bind
    rng = O.SplitMix64(91)
    w = [rng.field() for _ in range((batch * n // 2 - 1).bit_length())]
    claim, r = rng.field(), rng.field()
    for p in range(nparties):
        ref, eq_ref = S.SparseLayer([list(s) for s in layer0[p].coeffs], layer0[p].dense_len, p, nparties), O.SplitEq(w)
        eq = cozk.SplitEqPolynomial(ctx, w)
        ev = ref.compute_cubic_evals(eq_ref, claim)
        assert devs[p].round(eq, party=p) == [ev[0], ev[2], ev[3]], p
        ref.bind(r)
        devs[p].bind(r)
        assert devs[p].download()[0] == sorted(set(j >> 1 for j in want_idx))
        d = devs[p].to_dense(party=p)
        assert d.coeffs() == ref.coalesce(), p
        _free(d, eq)
    _free(*devs, *tgs)


# ------------------------------------------------------------------------------------------------ e. more than one tile per lane
def test_scan_with_two_tiles_per_lane(cozk, ctx):
    """1024 T + 1 items are 1025 tiles (0 .. 1024): k_sparse_scan_blocks runs with per = 2, lane t scans tiles 2t and 2t + 1, lane
    512 scans tile 1024 alone (its single item) and the lanes above it none -- the only branch a production-sized column takes.
    Plain; the values are a periodic tile of 49 raw residues, item i = (pattern[2i mod 49], pattern[(2i + 1) mod 49]), so no list of
    4 M field elements is built.  Counted 1-based the tiles are 1 .. 1025; the sample holds the groups on both sides of the last
    three tile borders, of the first borders inside a lane and between two lanes, the first group and the last."""
    LK, E, LB = _lk(), _engine(), importlib.import_module("co-zkvms_amd._lib")
    cnt = 1024 * T + 1
    idx = np.asarray(P.mixed(cnt, 3), dtype=np.uint32)
    n = P.dense_len([int(idx[-1])])
    rng = O.SplitMix64(49)
    pattern = [0, 1, R - 1] + [rng.field() for _ in range(46)]
    mont = [v * (1 << 256) % R for v in pattern]
    raw = np.frombuffer(b"".join(m.to_bytes(32, "little") for m in mont), dtype="<u8").reshape(49, 4)
    sp = LK.SparseLayer.from_vecs(ctx, LB.MODE_PLAIN, n, E.Vec.from_numpy(ctx, idx, kind=LB.SCALAR_U32),
                                  E.Vec.from_numpy(ctx, np.resize(raw, (2 * cnt, 4))), take_ownership=True)
    assert (len(sp), sp.count) == (n, cnt)

    def pair_at(i):
        return pattern[2 * i % 49], pattern[(2 * i + 1) % 49]

    groups = P.merged(idx)
    want_idx = np.unique(idx >> 1)
    G = len(want_idx)
    assert (groups[0] == want_idx).all()
    assert sp.next_count() == G

    of_item = P.group_of_item(idx)
    borders = [t * T for t in (1, 2, 3, 4, 1022, 1023, 1024)]
    sample = {0, G - 1} | {int(of_item[i]) for b in borders for i in (b - 1, b)}
    assert int(of_item[cnt - 1]) == G - 1
    while len(sample) < 64:
        sample.add(rng.next() % G)
    sample = sorted(sample)
    parts = [P.halves(groups, g, pair_at) for g in sample]
    assert {(a is None, b is None) for a, b in parts} == {(False, False), (False, True), (True, False)}

    out = sp.output_local(masked=False)
    assert len(out) == 2 * G
    got = E.mont_limbs_to_int(out.to_numpy().reshape(G, 8)[sample])
    out.free()
    assert got == [v for a, b in parts for v in P.output_group(a, b, 1)]

    r = rng.field()
    sp.bind(r)
    assert (len(sp), sp.count) == (n // 2, G)
    got_idx, got_val = np.zeros(G, dtype=np.uint32), np.zeros((2 * G, 4), dtype=np.uint64)
    ctx.check(LB.lib().cozk_sparse_layer_download(ctx.h, sp.h, got_idx.ctypes.data, got_val.ctypes.data, None))
    assert (got_idx == want_idx).all()
    got = E.mont_limbs_to_int(got_val.reshape(G, 8)[sample])
    assert got == [v for a, b in parts for v in P.bind_group(a, b, 1, r)]
    sp.free()
