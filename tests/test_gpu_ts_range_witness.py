"""GPU parity of the Lasso counters over an identity table of any length (`cozk_time_counters`) and of the timestamp range-check
witness made of them (`cozk_timestamp_range_witness`, csrc/ts_range_witness.hip) against the sequential loops of
tests/ts_range_ref.py: every output compared for exact equality.  With T = COZK_LASSO_TILE steps per tile, the shapes are the smallest
at which each piece can go wrong: lengths around a wave step, a workgroup, a staged chunk and the tiles, 1 / 3 / 16 columns, tables
around the one-pass / two-pass border of the sort, keys that differ only above bit 16, one segment as long as the column, all
segments of length one, t_read made on the device by cozk_rw_memory_witness, and the refusals."""
import importlib

import numpy as np
import pytest

import pyref as O
import rw_witness_ref as W
import ts_range_ref as TR

pytestmark = pytest.mark.gpu
INVALID_ARG = -1


@pytest.fixture(scope="module")
def TS():
    return importlib.import_module("co-zkvms_amd.ts_range")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("co-zkvms_amd.lasso").LASSO_TILE


def _u32(cozk, ctx, col):
    return cozk.Vec.from_numpy(ctx, np.asarray(col, dtype=np.uint32), cozk.SCALAR_U32)


def _same(name, got, want, length):
    assert len(got) == len(want), name
    for c, (g, w) in enumerate(zip(got, want)):
        g = g.to_numpy()
        assert g.dtype == np.uint32 and g.shape == (length,) and np.array_equal(g, np.asarray(w, dtype=np.uint32)), "%s of column %d differs" % (name, c)


def _check_counters(cozk, ctx, TS, keys, M, want=None):
    want = want or TR.time_counters(keys, M)
    rc, fc = TS.time_counters(ctx, [_u32(cozk, ctx, col) for col in keys], M)
    _same("read_cts", rc, want[0], len(keys[0]))
    _same("final_cts", fc, want[1], M)
    return [v.to_numpy() for v in rc], [v.to_numpy() for v in fc]


NAMES = ("read_cts_read_timestamp", "read_cts_global_minus_read", "final_cts_read_timestamp", "final_cts_global_minus_read")


def _check_witness(cozk, ctx, TS, t_read, M, d_t_read=None):
    want = TR.ts_range(t_read, M)
    got = TS.timestamp_range_witness(ctx, d_t_read or [_u32(cozk, ctx, col) for col in t_read], M)
    for k, name in enumerate(NAMES):
        _same(name, got[k], want[k], len(t_read[0]) if k < 2 else M)
    return got, want


def _lengths(T):
    return [1, 64, 65, 257, 4097, T + 1, 2 * T + 5]


@pytest.mark.parametrize("k", range(7))
def test_time_counters_at_every_length_with_1_3_and_16_columns(cozk, ctx, TS, T, k):
    n, M = _lengths(T)[k], 37
    keys = np.random.default_rng(300 + k).integers(0, M, size=(16, n)).tolist()
    want = TR.time_counters(keys, M)
    for cols in (1, 3, 16):  # the columns are independent: the first `cols` of them give the first `cols` of the results
        _check_counters(cozk, ctx, TS, keys[:cols], M, (want[0][:cols], want[1][:cols]))


@pytest.mark.parametrize("M", [1, 2, 65536, 65537, (1 << 17) + 3])
def test_tables_around_the_one_pass_two_pass_border(cozk, ctx, TS, M):
    n = 300
    keys = np.random.default_rng(310 + M % 7).integers(0, min(M, 32), size=(2, n)).tolist()
    edge = [k for b in (1 << 16, 1 << 17) for k in (b - 2, b - 1, b, b + 1) if k < M] + [M - 1]  # both sides of every 2^16 border, the last entry
    for j in range(0, n, 3):  # each of them several times, interleaved in time with the small keys
        keys[0][j] = edge[(j // 3) % len(edge)]
        keys[1][n - 1 - j] = edge[(j // 6) % len(edge)]
    rc, fc = _check_counters(cozk, ctx, TS, keys, M)
    assert M - 1 in keys[0] and fc[0][M - 1] > 0 and rc[0].max() > 0


def test_keys_that_share_their_low_16_bits_interleaved_in_time(cozk, ctx, TS, T):
    n, M = 2 * T + 9, (5 << 16) + 9  # three tiles, so the second pass orders across tiles too
    rng = np.random.default_rng(320)
    low = rng.integers(0, 3, size=(2, n)) * 1000 + 7
    high = (np.arange(n)[None, :] * 3 + np.arange(2)[:, None] + rng.integers(0, 2, size=(2, n))) % 6  # the high digit changes from step to step
    _check_counters(cozk, ctx, TS, np.minimum(low + (high << 16), M - 1).tolist(), M)


@pytest.mark.parametrize("M,k", [(9, 5), ((1 << 16) + 50, (1 << 16) + 5)], ids=["one_pass", "two_passes"])
def test_one_key_for_every_step(cozk, ctx, TS, T, M, k):
    n = 2 * T + 700
    rc, fc = _check_counters(cozk, ctx, TS, [[k] * n], M)
    assert np.array_equal(rc[0], np.arange(n)) and fc[0][k] == n and fc[0].sum() == n and np.count_nonzero(fc[0]) == 1


def test_every_key_distinct(cozk, ctx, TS):
    n = 65536 + 1000
    M = n + 77
    keys = np.random.default_rng(330).permutation(n).tolist()
    rc, fc = _check_counters(cozk, ctx, TS, [keys], M)
    assert not rc[0].any() and np.all(fc[0][:n] == 1) and not fc[0][n:].any()


def test_sixteen_columns_in_two_batches(cozk, ctx, TS, T):
    """The columns go in batches that keep 6 bytes per (tile, column, digit value) under 256 MiB: with two passes (65536 digit
    values) and 43 tiles that is 15 columns, so the sixteenth goes alone.  This is the one size at which that path runs, so the
    expected counters come from the keys' period, not from the loop: key = ((j + c) mod 1000) * 66 + c repeats every 1000 steps and
    at no other distance, so read_cts[j] = j div 1000; final_cts is the histogram.  Keys lie on both sides of 2^16."""
    n, M = 42 * T + 1, 66 * 1000 + 16
    assert 16 * 6 * 43 * 65536 > (256 << 20) >= 15 * 6 * 43 * 65536
    j = np.arange(n, dtype=np.uint32)
    keys = [((j + c) % 1000) * 66 + c for c in range(16)]
    vecs = [_u32(cozk, ctx, col) for col in keys]
    rc, fc = TS.time_counters(ctx, vecs, M)
    for c in range(16):
        assert np.array_equal(rc[c].to_numpy(), j // 1000), c
        assert np.array_equal(fc[c].to_numpy(), np.bincount(keys[c], minlength=M).astype(np.uint32)), c
    keys[15][5] = M  # a violation in the second batch is named by its column of the call
    vecs[15] = _u32(cozk, ctx, keys[15])
    _refused(cozk, "column 15, step 5:", lambda: TS.time_counters(ctx, vecs, M))


@pytest.mark.parametrize("M", [3, 65536])
def test_time_counters_meet_the_lasso_witness_on_one_key_column(cozk, ctx, TS, T, M):
    """Both routes to a Lasso counter run through one scan of the tile histograms: the same keys as a column of cozk_time_counters and
    as the one dimension of cozk_lasso_witness (one memory used at every step, an identity subtable of M entries) give equal
    read_cts and final_cts.  n = T + 65: two tiles, the last wave step partial; M = 65536 is the largest table both accept and the
    counters' one-pass path."""
    n = T + 65
    keys = np.random.default_rng(335).integers(0, M, size=n, dtype=np.uint32)
    col = _u32(cozk, ctx, keys)
    rc, fc = TS.time_counters(ctx, [col], M)
    l_rc, l_E, l_fc = cozk.lasso_witness(ctx, [col], [_u32(cozk, ctx, np.arange(M))], [None], [0], [0])
    assert np.array_equal(rc[0].to_numpy(), l_rc[0].to_numpy()) and np.array_equal(fc[0].to_numpy(), l_fc[0].to_numpy())
    assert rc[0].to_numpy().shape == (n,) and fc[0].to_numpy().shape == (M,) and int(fc[0].to_numpy().sum()) == n


def _jolt(seed, n, MEM, store_pct=30, n_regs=32):
    """the Jolt-shaped instance of tests/test_gpu_rw_witness.py: rs1, rs2 read; rd writes at every step; ram writes where the store
    flag is set"""
    rng = np.random.default_rng(seed)
    u32 = lambda k: rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32).tolist()
    addr = [rng.integers(0, n_regs, size=n).tolist() for _ in range(3)] + [rng.integers(0, MEM, size=n).tolist()]
    return addr, [None, None, u32(n), u32(n)], [None, None, None, (rng.integers(0, 100, size=n) < store_pct).astype(np.uint8).tolist()], u32(MEM)


def _device_t_read(cozk, ctx, seed, n, MEM):
    """t_read made ON THE DEVICE by cozk_rw_memory_witness (the Vecs, as they are) and the replay's, which it equals"""
    addr, vw, iw, vi = _jolt(seed, n, MEM)
    up = lambda cols, dt, kind: [None if c is None else cozk.Vec.from_numpy(ctx, np.asarray(c, dtype=dt), kind) for c in cols]
    out = cozk.rw_memory_witness(ctx, up(addr, np.uint32, cozk.SCALAR_U32), up(vw, np.uint32, cozk.SCALAR_U32), up(iw, np.uint8, cozk.SCALAR_U8),
                                 _u32(cozk, ctx, vi))
    t_read = W.replay(addr, vw, iw, vi)[1]
    for s in range(4):
        assert np.array_equal(out[1][s].to_numpy(), np.asarray(t_read[s], dtype=np.uint32))
    return out[1], t_read


@pytest.fixture(scope="module")
def three_tiles(cozk, ctx, T):
    """n = 2 T + 300 steps against a table of 2^17 entries: two passes, three tiles"""
    n = 2 * T + 300
    d, h = _device_t_read(cozk, ctx, 340, n, 70000)
    return n, 1 << 17, d, h


def test_witness_of_a_device_made_t_read_in_one_pass(cozk, ctx, TS):
    d, h = _device_t_read(cozk, ctx, 341, 300, 500)
    _check_witness(cozk, ctx, TS, h, 512, d)


def test_witness_of_a_device_made_t_read_in_two_passes_over_three_tiles(cozk, ctx, TS, three_tiles):
    n, M, d, h = three_tiles
    got, want = _check_witness(cozk, ctx, TS, h, M, d)
    assert max(want[0][0]) > 0 and max(want[1][0]) > 0  # both families have repeated keys


@pytest.mark.parametrize("n,M", [(300, 512), (300, 300), (32768 + 77, 1 << 17)], ids=["one_pass", "M_equals_n", "two_passes"])
def test_witness_at_the_extremes_of_t_read(cozk, ctx, TS, n, M):
    zero, own = [0] * n, list(range(n))
    got, want = _check_witness(cozk, ctx, TS, [zero, own], M)
    assert want[0][0] == own and want[1][0] == zero and want[0][1] == zero and want[1][1] == own  # one segment / all segments of one step
    assert want[2][0][0] == n and want[3][1][0] == n and want[3][0][:n] == [1] * n and want[2][1][:n] == [1] * n


def test_outputs_are_the_columns_of_the_memory_checking_leaves(cozk, ctx, TS):
    """end to end through the project's leaf kernel: the call's Vecs, as they are, are the compact columns of cozk_fingerprint_leaves.
    Per (slot, kind), with tuples (key, key, count): init * prod writes == prod reads * final over the downloaded leaves; the four
    products are the reference's; the identity breaks once one final_cts entry is bumped.  h = count g^2 + key (1 + g) - tau, and the
    global-minus-read key is (1 + g) iota - (1 + g) t_read: the key column is never made."""
    n, M = 300, 512
    t_read, h_t_read = _device_t_read(cozk, ctx, 350, n, 500)
    got, want = _check_witness(cozk, ctx, TS, h_t_read, M, t_read)
    rng = O.SplitMix64(351)
    g, tau = rng.field(), rng.field()
    g1, g2 = (1 + g) % O.R, g * g % O.R
    iota_n, iota_M = _u32(cozk, ctx, np.arange(n)), _u32(cozk, ctx, np.arange(M))

    def product(cols, coeffs, const, count):
        out = cozk.Vec.alloc(ctx, count)
        cozk.fingerprint_leaves(ctx, cols, coeffs, [], [], const % O.R, "plain", 0, out, n=count)
        p = 1
        for x in out.to_ints():
            p = p * x % O.R
        return p

    for s in range(4):
        for kind in range(2):  # read timestamp, global minus read
            rc, fc = got[kind][s], got[2 + kind][s]
            key_cols, key_coeffs = ([t_read[s]], [g1]) if kind == 0 else ([iota_n, t_read[s]], [g1, (-g1) % O.R])
            reads = product(key_cols + [rc], key_coeffs + [g2], -tau, n)
            writes = product(key_cols + [rc], key_coeffs + [g2], g2 - tau, n)  # count + 1
            inits = product([iota_M], [g1], -tau, M)
            finals = product([iota_M, fc], [g1, g2], -tau, M)
            assert inits * writes % O.R == reads * finals % O.R, (s, kind)
            keys = h_t_read[s] if kind == 0 else [j - t for j, t in enumerate(h_t_read[s])]
            assert (inits, writes, reads, finals) == TR.hashes(keys, want[kind][s], want[2 + kind][s], g, tau), (s, kind)
            bumped = fc.to_numpy()
            bumped[keys[10]] += 1
            finals = product([iota_M, _u32(cozk, ctx, bumped)], [g1, g2], -tau, M)
            assert inits * writes % O.R != reads * finals % O.R, (s, kind)


def test_the_same_call_twice_gives_the_same_bytes(cozk, ctx, TS, three_tiles):
    n, M, d, h = three_tiles
    runs = []
    for _ in range(2):
        out = TS.timestamp_range_witness(ctx, d, M)
        rc, fc = TS.time_counters(ctx, d[:3], M)
        runs.append([v.to_numpy().tobytes() for group in out for v in group] + [v.to_numpy().tobytes() for v in rc + fc])
    assert len(runs[0]) == 22 and runs[0] == runs[1]
    assert runs[0][16:19] == runs[0][0:3] and runs[0][19:22] == runs[0][8:11]  # the read-timestamp family is time_counters of t_read


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals(cozk, ctx, TS):
    n, M = 200, 16
    keys = np.random.default_rng(360).integers(0, M, size=(3, n)).tolist()
    up = lambda cols: [_u32(cozk, ctx, c) for c in cols]
    bad = [list(c) for c in keys]
    bad[1][150] = M      # a key equal to M ...
    bad[1][77] = M + 5   # ... an earlier one above it ...
    bad[2][3] = 1 << 31  # ... and one in a later column at an earlier step: the smallest (column, step) is named
    _refused(cozk, "column 1, step 77:", lambda: TS.time_counters(ctx, up(bad), M))
    bad[1][77] = keys[1][77]
    _refused(cozk, "column 1, step 150: the key is >= M = 16", lambda: TS.time_counters(ctx, up(bad), M))
    u8 = cozk.Vec.from_numpy(ctx, np.asarray(keys[1], dtype=np.uint8), cozk.SCALAR_U8)
    _refused(cozk, "keys[c] is a U32 vector", lambda: TS.time_counters(ctx, [up(keys)[0], u8], M))
    _refused(cozk, "keys[c] has n entries", lambda: TS.time_counters(ctx, up([keys[0], keys[1][:-1]]), M))
    _refused(cozk, "1 <= n_cols <= 16", lambda: TS.time_counters(ctx, up([keys[0]] * 17), M))
    _refused(cozk, "1 <= n_cols <= 16", lambda: TS.time_counters(ctx, [], M))
    _refused(cozk, "1 <= M < 2^32", lambda: TS.time_counters(ctx, up(keys), 0))

    t_read = [[j * 3 // 4 for j in range(n)] for _ in range(4)]
    late = [list(c) for c in t_read]
    late[3][90] = 91  # t_read[s][j] = j + 1 ...
    late[1][90] = 91  # ... the smallest (step, slot) is named
    late[0][120] = 1 << 31
    _refused(cozk, "step 90, slot 1: t_read is greater than the step", lambda: TS.timestamp_range_witness(ctx, up(late), 256))
    _refused(cozk, "t_read[s] is a U32 vector", lambda: TS.timestamp_range_witness(ctx, [up(t_read)[0], u8], 256))
    _refused(cozk, "t_read[s] has n entries", lambda: TS.timestamp_range_witness(ctx, up([t_read[0], t_read[1][:-1]]), 256))
    _refused(cozk, "1 <= n_slots <= 8", lambda: TS.timestamp_range_witness(ctx, up(t_read[:1] * 9), 256))
    _refused(cozk, "M >= n", lambda: TS.timestamp_range_witness(ctx, up(t_read), n - 1))
    _check_counters(cozk, ctx, TS, keys, M)  # the context works on after a refusal
    _check_witness(cozk, ctx, TS, t_read, n)
