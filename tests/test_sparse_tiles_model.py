"""CPU checks of tests/sparse_tiles_ref.py: every pattern builder places its groups where its table says, and the pair-form
restatement of bind and layer_output equals the literal oracle (oracle/pysparse.py) at small sizes, plain and three parties."""
import numpy as np
import pytest

import pyref as O
import pysparse as S
import sparse_tiles_ref as P

R = O.R
T = P.T
SMALL = 41  # an odd count: the last group of full() is a lone even half


def _strictly_increasing(idx):
    return all(b > a for a, b in zip(idx, idx[1:]))


def _sibling_items(idx):
    """the list positions (i, i + 1) of every pair of siblings"""
    return [(i, i + 1) for i in range(len(idx) - 1) if idx[i] >> 1 == idx[i + 1] >> 1]


def test_the_tile_is_the_kernels():
    assert (P.PT, P.SP_ITEMS, T) == (256, 8, 2048)


@pytest.mark.parametrize("cnt", [1, 2, SMALL, T - 1, T, T + 1, 2 * T + 1])
def test_full_keeps_siblings_inside_every_border(cnt):
    idx = P.full(cnt)
    assert len(idx) == cnt and idx[0] == 0 and _strictly_increasing(idx)
    sib = _sibling_items(idx)
    assert len(sib) == cnt // 2 and all(i % 2 == 0 for i, _ in sib)  # (even, odd): no border of an even size is straddled
    q, head, half, has_sib = P.merged(idx)
    assert len(q) == (cnt + 1) // 2 and not half.any() and has_sib.sum() == cnt // 2


@pytest.mark.parametrize("cnt", [1, 2, SMALL, T - 1, T, T + 1, 2 * T + 1])
def test_odd_shift_straddles_every_border(cnt):
    idx = P.odd_shift(cnt)
    assert len(idx) == cnt and idx[0] == 1 and _strictly_increasing(idx)
    q, head, half, has_sib = P.merged(idx)
    assert (int(half[0]), bool(has_sib[0])) == (1, False)  # item 0 is a lone odd half
    sib = _sibling_items(idx)
    assert len(sib) == (cnt - 1) // 2 and all(i % 2 == 1 for i, _ in sib)  # (odd, even)
    for border in (64, 256, T, 2 * T):  # a wave, a row, a tile, the next tile
        if cnt >= border + 1:
            assert idx[border - 1] >> 1 == idx[border] >> 1
            assert (border - 1, border) in sib


def test_the_single_item_of_a_second_tile():
    idx = P.odd_shift(T + 1)
    assert len(idx) - T == 1  # the second tile holds exactly one item ...
    head = set(P.merged(idx)[1].tolist())
    assert T not in head and T - 1 in head  # ... which is not a head: its group's head closes the first tile
    idx = P.full(T + 1)
    q, head, half, has_sib = P.merged(idx)
    assert int(head[-1]) == T and int(half[-1]) == 0 and not has_sib[-1]  # full: the single item is a head, a lone even half
    idx = P.full(T)
    assert len(idx) == T and T - 1 in [j for _, j in _sibling_items(idx)]  # an exact tile ends on an odd half


@pytest.mark.parametrize("cnt", [1, SMALL, 2 * T + 1])
def test_evens_and_odds_have_no_siblings(cnt):
    for build, want_half in ((P.evens, 0), (P.odds, 1)):
        idx = build(cnt)
        assert len(idx) == cnt and idx[0] == want_half and _strictly_increasing(idx)
        assert _sibling_items(idx) == []
        q, head, half, has_sib = P.merged(idx)
        assert len(q) == cnt and head.tolist() == list(range(cnt))  # every item is a head: next_count == cnt
        assert (half == want_half).all() and not has_sib.any()


def test_splitmix64_array_is_the_oracles_generator():
    for seed in (0, 7, 2**64 - 1):
        rng = O.SplitMix64(seed)
        assert P.splitmix64(seed, 100).tolist() == [rng.next() for _ in range(100)]


@pytest.mark.parametrize("cnt", [SMALL, 2 * T + 1])
def test_mixed_has_every_kind_of_group_and_uneven_tiles(cnt):
    idx = P.mixed(cnt, 7)
    assert len(idx) == cnt and _strictly_increasing(idx)
    rng = O.SplitMix64(7)
    keep = [rng.next() % 3 != 0 for _ in range(idx[-1] + 1)]
    assert idx == [j for j, k in enumerate(keep) if k]  # index j kept iff draw j says so: 2 in 3
    assert P.mixed(cnt, 8) != idx
    q, head, half, has_sib = P.merged(idx)
    kinds = set(zip(half.tolist(), has_sib.tolist()))
    assert kinds == {(0, True), (0, False), (1, False)}  # full groups, lone evens, lone odds
    if cnt > 2 * T:
        per_tile = np.bincount(head // T, minlength=3)  # the third tile is the single last item, a head or not
        assert len(per_tile) == 3 and per_tile[0] != per_tile[1] and 0 < min(per_tile[:2]) < T  # the head count differs from tile to tile
        pos = {(int(i) % 64 == 63, int(i) % 256 == 255, int(i) % T == T - 1) for i, s in zip(head, has_sib) if s}
        assert (True, False, False) in pos  # some group lies across a wave border


def test_merged_is_unique_idx_halved():
    for name, build in P.PATTERNS.items():
        idx = build(SMALL)
        q, head, half, has_sib = P.merged(idx)
        assert q.tolist() == sorted({j >> 1 for j in idx}), name
        assert [idx[i] for i in head] == [min(j for j in idx if j >> 1 == g) for g in q.tolist()]
        assert P.group_of_item(idx).tolist() == [q.tolist().index(j >> 1) for j in idx]
    assert [len(x) for x in P.merged([])] == [0, 0, 0, 0]


def test_dense_len_is_twice_the_power_of_two_above_the_last_index():
    assert [P.dense_len([j]) for j in (1, 2, 3, 4, 2047, 2048, 2049)] == [4, 8, 8, 16, 4096, 8192, 8192]


@pytest.mark.parametrize("nparties", [1, 3])
@pytest.mark.parametrize("pattern", sorted(P.PATTERNS))
def test_two_binds_equal_the_literal_oracle(pattern, nparties):
    idx0 = P.PATTERNS[pattern](SMALL)
    shares = P.share_pairs(SMALL, 11, nparties)
    rng = O.SplitMix64(12)
    rs = [rng.field(), rng.field()]
    for p in range(nparties):
        ref = P.oracle_layer(idx0, shares[p], p, nparties)
        one = S.one_share(p, nparties)
        idx, pairs, n = idx0, shares[p], P.dense_len(idx0)
        assert ref.dense_len == n and ref.coalesce() == P.dense(n, idx, pairs, one)
        for r in rs:
            ref.bind(r)
            want_idx = sorted({j >> 1 for j in idx})
            idx, pairs = P.bind(idx, pairs, one, r)
            n //= 2
            assert idx == want_idx and len(pairs) == len(idx)
            assert ref.dense_len == n and ref.coalesce() == P.dense(n, idx, pairs, one), (p, n)


@pytest.mark.parametrize("nparties", [1, 3])
@pytest.mark.parametrize("pattern", sorted(P.PATTERNS))
def test_local_outputs_equal_the_literal_oracle(pattern, nparties):
    idx = P.PATTERNS[pattern](SMALL)
    shares = P.share_pairs(SMALL, 21, nparties)
    n = P.dense_len(idx)
    nxt = S.sparse_layer_output([P.oracle_layer(idx, shares[p], p, nparties) for p in range(nparties)])  # zero masks
    for p in range(nparties):
        a1 = P.add_one(p, nparties)
        q, flat = P.output(idx, shares[p], a1)
        assert q == sorted({j >> 1 for j in idx}) and len(flat) == 2 * len(q)
        local = [v[0] if nparties == 3 else v for v in nxt[p].coalesce()]  # the a component is the party's own local product
        assert nxt[p].dense_len == n // 2
        assert local == P.dense(n // 2, q, list(zip(flat[0::2], flat[1::2])), a1)
    if nparties == 3:  # the b component is the previous party's a: the ring reshare
        for p in range(3):
            assert [v[1] for v in nxt[p].coalesce()] == [v[0] for v in nxt[(p + 2) % 3].coalesce()]


@pytest.mark.parametrize("batch,n", [(4, 4096), (8, 2048)])
def test_toggle_columns_place_the_flags(batch, n):
    cols = P.toggle_columns(batch, n)
    assert (len(cols), batch * n // 2) == (batch // 2, 4 * T) and all(len(c) == n and set(c) <= {0, 1} for c in cols)
    stored = P.stored_pairs(cols, batch, n)
    at = {j: i for i, j in enumerate(stored)}
    assert T - 1 in at and T in at and at[T] == at[T - 1] + 1  # pairs 2047 | 2048, both stored, on either side of a tile of pairs
    sib = [i for i, _ in _sibling_items(stored) if stored[i] < T]
    assert len(sib) > T // 2 - 8 and all(i % 2 == 1 for i in sib)  # odd_shift-like: every group of tile 0 at items (odd, even)
    assert {(cols[0][2 * j], cols[0][2 * j + 1]) for j in range(n // 2)} == {(0, 0), (1, 1), (1, 0), (0, 1)}  # both, left, right flag
    per_tile = [sum(1 for j in stored if j // T == t) for t in range(4)]
    assert T in per_tile and 0 < per_tile[0] < T
    if batch == 8:  # four independent tiles: one with no flag at all beside one with every flag
        assert per_tile[2:] == [0, T] and 0 < per_tile[1] < T
