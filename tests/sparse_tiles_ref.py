"""Designed index patterns for the sparse pair layers (csrc/sparse_layer.inc), a pair-form restatement of their bind and
layer_output, and the round driver the sparse-layer GPU tests share.  Plain Python and numpy, no GPU.

The device object stores PAIRS: a strictly increasing list idx of pair indices and one (L, R) per index.  Its structural kernels
work on tiles of T = SP_TILE = PT * SP_ITEMS = 256 * 8 list items, rows of PT items and waves of 64; neighbours with equal
idx >> 1 merge into one group.  The builders below put those groups where the kernels' borders are:

  full(cnt)       0 .. cnt-1       every group has both halves; siblings sit at items (even, odd) and never straddle a border
  odd_shift(cnt)  1 .. cnt         item 0 is a lone odd half; after it siblings sit at items (odd, even): a group straddles every
                                   wave border (63|64), every row border (255|256) and every tile border (2047|2048)
  evens(cnt)      0, 2, 4, ..      no siblings; every item is a head with half 0; as many groups as items
  odds(cnt)       1, 3, 5, ..      no siblings; every head has half 1 (the L0 = R0 = one side of sp_quad)
  mixed(cnt, s)   each index kept with probability 2/3 (SplitMix64 of seed s): lone evens, lone odds and full groups in
                  irregular order; the head count differs from tile to tile

The restatement is the kernels' own formulation (stored pairs, a missing pair = (one, one)) in big ints, with numpy for the index
arithmetic only, so that it reaches sizes where the literal oracle (oracle/pysparse.py, single elements and 20 neighbour cases)
is too slow; tests/test_sparse_tiles_model.py pins it to that oracle at small sizes."""
import numpy as np

import pyref as O
import pysparse as S

R = O.R
PT, SP_ITEMS = 256, 8
T = PT * SP_ITEMS  # SP_TILE


# ------------------------------------------------------------------------------------------------ patterns
def full(cnt):
    return list(range(cnt))


def odd_shift(cnt):
    return list(range(1, cnt + 1))


def evens(cnt):
    return list(range(0, 2 * cnt, 2))


def odds(cnt):
    return list(range(1, 2 * cnt, 2))


def splitmix64(seed, n):
    """the first n outputs of pyref.SplitMix64(seed) as a uint64 array: output k hashes seed + k * gamma, so all n at once"""
    z = np.full(n, seed, dtype=np.uint64) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mixed(cnt, seed):
    """the first cnt indices j >= 0 with SplitMix64(seed) output j not a multiple of 3"""
    m = 2 * cnt + 64
    while True:
        kept = np.flatnonzero(splitmix64(seed, m) % np.uint64(3) != 0)
        if len(kept) >= cnt:
            return kept[:cnt].tolist()
        m *= 2


PATTERNS = {"full": full, "odd_shift": odd_shift, "evens": evens, "odds": odds, "mixed": lambda cnt: mixed(cnt, 7)}


# ------------------------------------------------------------------------------------------------ merged groups
def merged(idx):
    """the merged groups of a sorted pair-index list as numpy arrays (q, head, half, has_sib): the group's index idx >> 1, the list
    position of its first item, that item's idx & 1, and whether the next item is the other half"""
    a = np.asarray(idx, dtype=np.int64)
    q = a >> 1
    if len(a) == 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e, e, np.zeros(0, dtype=bool)
    first = np.ones(len(a), dtype=bool)
    first[1:] = q[1:] != q[:-1]
    head = np.flatnonzero(first)
    nxt = np.minimum(head + 1, len(a) - 1)
    has_sib = (head + 1 < len(a)) & (q[nxt] == q[head])
    return q[head], head, a[head] & 1, has_sib


def group_of_item(idx):
    """for every list item the position of its group in merged(idx)"""
    q = np.asarray(idx, dtype=np.int64) >> 1
    first = np.ones(len(q), dtype=bool)
    first[1:] = q[1:] != q[:-1]
    return np.cumsum(first) - 1


def halves(groups, g, pair_at):
    """the two pairs of merged group g, (pair 2q, pair 2q + 1), None where one is not stored; pair_at(i) = the (L, R) of item i"""
    _, head, half, has_sib = groups
    i = int(head[g])
    if half[g]:
        return None, pair_at(i)
    return pair_at(i), (pair_at(i + 1) if has_sib[g] else None)


def _lerp(a, b, r):
    return O.sh_add(a, O.sh_mul_public(O.sh_sub(b, a), r))


def bind_group(p0, p1, one, r):
    """the bound pair (L', R') of one group: L' = L0 + r (L1 - L0), R' likewise, a missing half = (one, one)"""
    (L0, R0), (L1, R1) = p0 or (one, one), p1 or (one, one)
    return _lerp(L0, L1, r), _lerp(R0, R1, r)


def output_group(p0, p1, add_one):
    """the additive local products (p0, p1) of one group in layer_output, a missing pair = the additive trivial one"""
    return tuple(add_one if p is None else O.sh_local_mul(*p) for p in (p0, p1))


def bind(idx, pairs, one, r):
    """-> (unique(idx >> 1), the bound pairs)"""
    groups = merged(idx)
    return groups[0].tolist(), [bind_group(*halves(groups, g, pairs.__getitem__), one, r) for g in range(len(groups[0]))]


def output(idx, pairs, add_one):
    """-> (unique(idx >> 1), the compact vector p0, p1 per group, flat)"""
    groups = merged(idx)
    return groups[0].tolist(), [v for g in range(len(groups[0])) for v in output_group(*halves(groups, g, pairs.__getitem__), add_one)]


def add_one(party, nparties):
    """additive::promote_to_trivial_share(one): the plain prover and party 0 hold 1, the others 0"""
    return 1 if nparties == 1 or party == 0 else 0


def dense(n, idx, pairs, one):
    """the dense interleaved layer of n entries the stored pairs stand for"""
    out = [one] * n
    for j, (l, r) in zip(idx, pairs):
        out[2 * j], out[2 * j + 1] = l, r
    return out


# ------------------------------------------------------------------------------------------------ the literal oracle's view
def dense_len(idx):
    """2 * npairs, npairs the power of two above the last index"""
    return 2 << int(idx[-1]).bit_length()


def oracle_layer(idx, pairs, party, nparties):
    """the stored pairs as ONE segment of oracle/pysparse.py's element lists"""
    seg = [e for j, (l, r) in zip(idx, pairs) for e in ((2 * int(j), l), (2 * int(j) + 1, r))]
    return S.SparseLayer([seg], dense_len(idx), party, nparties)


def share_pairs(cnt, seed, nparties):
    """per party cnt pairs (L, R) of random values: ints for the plain prover, else the three parties' Rep3 shares"""
    rng = O.SplitMix64(seed)
    if nparties == 1:
        return [[(rng.field(), rng.field()) for _ in range(cnt)]]
    sh = [(O.rep3_share(rng.field(), rng), O.rep3_share(rng.field(), rng)) for _ in range(cnt)]
    return [[(l[p], r[p]) for l, r in sh] for p in range(3)]


# ------------------------------------------------------------------------------------------------ placed flags for the toggle route
def stored_pairs(cols, batch, n):
    """the pairs of a toggle layer's output that are not (one, one): one of the pair's two flags is set"""
    return [b * (n // 2) + i // 2 for b in range(batch) for i in range(0, n, 2) if cols[b // 2][i] | cols[b // 2][i + 1]]


def toggle_flags(stored, kinds_from=0):
    """the 0/1 flags of one circuit from `stored` (pair -> bool): a stored pair has both flags, the left or the right one in turn"""
    kinds = ((1, 1), (1, 0), (0, 1))
    out = []
    for i, s in enumerate(stored):
        out += kinds[(i + kinds_from) % 3] if s else (0, 0)
    return out


def toggle_columns(batch, n):
    """one flag column per pair of circuits.  The two circuits of a pair share their flags, and a tile of the flag scan is T pairs.
    (4, 4096): a circuit is a tile, so tiles 0 and 1 carry one column and tiles 2 and 3 the other.  Column 0 leaves out pair 1 alone:
    the list is 0, 2, 3, 4, .., odd_shift-like up to pair 2047 | 2048, both stored, on either side of the first tile border; column
    1 sets every flag.  No tile can be empty beside a full one at this shape, hence
    (8, 2048): a pair of circuits is a tile, four independent tiles.  Tile 0 stores 0, 2 .. 1021, 1023 of each circuit, an even
    count with the groups at items (odd, even) in both circuits and pairs 2047 | 2048 stored; tile 1 a 2-in-3 mix; tile 2 has no flag
    at all; tile 3 every flag."""
    pairs = n // 2
    if (batch, n) == (4, 4096):
        return [toggle_flags([i != 1 for i in range(pairs)]), [1] * n]
    assert (batch, n) == (8, 2048)
    rng = O.SplitMix64(5)
    return [toggle_flags([i not in (1, pairs - 2) for i in range(pairs)]), toggle_flags([rng.next() % 3 != 0 for _ in range(pairs)], 1), [0] * n, [1] * n]


# ------------------------------------------------------------------------------------------------ the shared round driver
def opened(coeffs):
    """the values a Rep3 vector of one party per row opens to: a_0 + a_1 + a_2"""
    return [sum(c[0] for c in col) % R for col in zip(*coeffs)]


def sumcheck(cozk, ctx, devs, refs, seed, exact):
    """every round of a sumcheck over one layer held by len(devs) parties.  exact: per party the round values and the bound layer equal
    the oracle's bit for bit; else the sums over the parties and the opened layers do.  Returns the eq forms the rounds went through."""
    nparties = len(devs)
    n = refs[0].dense_len
    assert len(devs[0]) == n
    nv = max(1, (n // 2 - 1).bit_length())
    rng = O.SplitMix64(seed)
    w = [rng.field() for _ in range(nv)]
    eq_refs = [O.SplitEq(w) for _ in range(nparties)]
    eq_devs = [cozk.SplitEqPolynomial(ctx, w) for _ in range(nparties)]
    claim = rng.field()
    forms = set()

    def check_dense():
        got = [devs[p].to_dense(party=p) for p in range(nparties)]
        want = [refs[p].coalesce() for p in range(nparties)]
        if exact:
            for p in range(nparties):
                assert got[p].coeffs() == want[p], p
        else:
            assert opened([g.coeffs() for g in got]) == opened(want)
        for g in got:
            g.free()

    pending = None
    rounds = 0
    while True:
        n_round = n // 2 if pending is not None else n
        if n_round < 4 or n_round % 4:
            break
        forms.add("flat" if eq_refs[0].E1_len == 1 else "nested")
        evs = [refs[p].compute_cubic_evals(eq_refs[p], claim) for p in range(nparties)]
        gots = [devs[p].round(eq_devs[p], pending, party=p) for p in range(nparties)]
        n = n_round
        if exact:
            for p in range(nparties):
                assert gots[p] == [evs[p][0], evs[p][2], evs[p][3]], (p, rounds)
        else:
            for k, kk in enumerate((0, 2, 3)):
                assert sum(g[k] for g in gots) % R == sum(e[kk] for e in evs) % R, (rounds, kk)
        if pending is not None:
            assert len(devs[0]) == refs[0].dense_len
            check_dense()
        pending = rng.field()
        for p in range(nparties):
            refs[p].bind(pending)
            eq_refs[p].bind(pending)
        rounds += 1
    assert rounds >= 1
    if n >= 4 and n % 4 == 0:  # the bind after the last sparse round
        for p in range(nparties):
            devs[p].bind(pending)
        check_dense()
    for e in eq_devs:
        e.free()
    return forms
