"""GPU parity of the dealer's read-write memory witness (`cozk_rw_memory_witness`, csrc/rw_memory_witness.hip) against the sequential
replay of tests/rw_witness_ref.py: v_read, t_read, v_written, v_final and t_final compared for exact equality.  With T =
COZK_LASSO_TILE operations per tile, the shapes are the smallest at which each piece can go wrong: operation counts around a wave
step, a workgroup and the tiles, 1 / 3 / 4 / 8 slots, memories around the one-pass / two-pass border of the sort, addresses that
differ only above bit 16, one segment as long as the input, slots that alias inside a step, every write pattern, and the refusals.
(n * n_slots >= 2^32 is not reachable without allocating a vector of 2^29 entries, so that refusal is not exercised here.)"""
import importlib

import numpy as np
import pytest

import pyref as O
import rw_witness_ref as W

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
NAMES = ("v_read", "t_read", "v_written", "v_final", "t_final")


@pytest.fixture(scope="module")
def RW():
    return importlib.import_module("co-zkvms_amd.rw_memory")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("co-zkvms_amd.lasso").LASSO_TILE


def _upload(cozk, ctx, addr, v_write, is_write, v_init, addr_kinds=None):
    kinds = addr_kinds or ["U32"] * len(addr)
    dt = {"U8": np.uint8, "U16": np.uint16, "U32": np.uint32}
    a = [cozk.Vec.from_numpy(ctx, np.asarray(c, dtype=dt[k]), getattr(cozk, "SCALAR_" + k)) for c, k in zip(addr, kinds)]
    vw = [None if c is None else cozk.Vec.from_numpy(ctx, np.asarray(c, dtype=np.uint32), cozk.SCALAR_U32) for c in v_write]
    iw = [None if c is None else cozk.Vec.from_numpy(ctx, np.asarray(c, dtype=np.uint8), cozk.SCALAR_U8) for c in is_write]
    return a, vw, iw, cozk.Vec.from_numpy(ctx, np.asarray(v_init, dtype=np.uint32), cozk.SCALAR_U32)


def _device(cozk, ctx, RW, addr, v_write, is_write, v_init, addr_kinds=None):
    out = RW.rw_memory_witness(ctx, *_upload(cozk, ctx, addr, v_write, is_write, v_init, addr_kinds))
    per_slot = [[None if v is None else v.to_numpy() for v in group] for group in out[:3]]
    return per_slot + [out[3].to_numpy(), out[4].to_numpy()]


def _check(cozk, ctx, RW, addr, v_write, is_write, v_init, addr_kinds=None):
    got = _device(cozk, ctx, RW, addr, v_write, is_write, v_init, addr_kinds)
    want = W.replay(addr, v_write, is_write, v_init)
    for name, g, w in zip(NAMES[:3], got, want):
        for s in range(len(addr)):
            if w[s] is None:
                assert g[s] is None, "%s of slot %d should be absent" % (name, s)
            else:
                assert g[s] is not None and g[s].dtype == np.uint32 and np.array_equal(g[s], np.asarray(w[s], dtype=np.uint32)), "%s of slot %d differs" % (name, s)
    for name, g, w in zip(NAMES[3:], got[3:], want[3:]):
        assert g.dtype == np.uint32 and np.array_equal(g, np.asarray(w, dtype=np.uint32)), name + " differs"
    return got


def _jolt(seed, n, MEM, store_pct=30, n_regs=None):
    """rs1, rs2 read; rd writes at every step; ram writes where the store flag is set (numpy's generator: these get long)"""
    rng = np.random.default_rng(seed)
    n_regs = min(MEM, n_regs or MEM)
    u32 = lambda k: rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32).tolist()
    addr = [rng.integers(0, n_regs, size=n).tolist() for _ in range(3)] + [rng.integers(0, MEM, size=n).tolist()]
    return addr, [None, None, u32(n), u32(n)], [None, None, None, (rng.integers(0, 100, size=n) < store_pct).astype(np.uint8).tolist()], u32(MEM)


def _lengths(T):
    return [1, 16, 17, 65, T // 4 + 1, 3 * T // 4 + 5]


@pytest.mark.parametrize("k", range(6))
def test_every_length_around_waves_workgroups_and_tiles(cozk, ctx, RW, T, k):
    _check(cozk, ctx, RW, *_jolt(100 + k, _lengths(T)[k], 37))


def test_three_slots_so_the_operation_count_is_no_multiple_of_four(cozk, ctx, RW):
    addr, vw, iw, vi = _jolt(110, 65, 37)
    _check(cozk, ctx, RW, addr[1:], vw[1:], iw[1:], vi)  # rs2, rd, ram: 195 operations


def test_one_slot_and_eight_slots(cozk, ctx, RW):
    addr, vw, iw, vi = _jolt(111, 300, 23, store_pct=40)
    _check(cozk, ctx, RW, addr[3:], vw[3:], iw[3:], vi)
    _check(cozk, ctx, RW, addr[:1], [None], [None], vi)
    b = _jolt(112, 300, 23, store_pct=70)
    _check(cozk, ctx, RW, addr + b[0], vw + b[1], iw + b[2], vi)


@pytest.mark.parametrize("MEM", [1, 2, 65536, 65537, (1 << 17) + 3])
def test_memory_sizes_around_the_one_pass_two_pass_border(cozk, ctx, RW, MEM):
    addr, vw, iw, vi = _jolt(120 + MEM % 7, 300, MEM, n_regs=min(MEM, 32))
    for j in range(0, 300, 7):  # the last words of the memory, and the words on both sides of every 2^16 border, several times each
        addr[3][j] = (MEM - 1 - (j // 7) % 3) % MEM if j % 2 else min(MEM - 1, 65535 + (j // 14) % 3)
    got = _check(cozk, ctx, RW, addr, vw, iw, vi)
    assert MEM - 1 in addr[3] and got[4][MEM - 1] > 0


def test_addresses_that_share_their_low_16_bits_interleaved_in_time(cozk, ctx, RW, T):
    n, MEM = T // 4 + 1, (5 << 16) + 9  # 4 n operations: more than one tile, so the second pass orders across tiles too
    rng = np.random.default_rng(130)
    low = rng.integers(0, 3, size=(4, n)) * 1000 + 7
    high = (np.arange(n)[None, :] * 3 + np.arange(4)[:, None] + rng.integers(0, 2, size=(4, n))) % 6  # the high digit changes from operation to operation
    addr = np.minimum(low + (high << 16), MEM - 1).tolist()
    _, vw, iw, vi = _jolt(131, n, MEM, store_pct=25)
    _check(cozk, ctx, RW, addr, vw, iw, vi)


def test_one_address_for_every_operation_written_every_1000th_step(cozk, ctx, RW, T):
    n = T // 2 + 700  # 4 n operations in ONE segment: more than two tiles and more than sixteen sweep blocks
    assert 4 * n > 2 * T
    _, vw, _, vi = _jolt(140, n, 9)
    every = [1 if j % 1000 == 999 else 0 for j in range(n)]
    got = _check(cozk, ctx, RW, [[5] * n] * 4, [None, None, vw[2], vw[3]], [None, None, every, [0] * n], vi)
    assert got[0][0][999] == vi[5] and got[0][0][1000] == vw[2][999] and got[4][5] == n - 1
    assert np.array_equal(got[1][0][1:], np.arange(n - 1)) and np.array_equal(got[1][1], np.arange(n))  # rs1 follows step j - 1's ram, rs2 follows rs1


@pytest.mark.parametrize("case", W.aliasing_instances(), ids=[c[0] for c in W.aliasing_instances()])
def test_slots_that_alias_inside_a_step_and_across_steps(cozk, ctx, RW, case):
    _check(cozk, ctx, RW, *case[1:])


def test_no_writing_slot_at_all(cozk, ctx, RW):
    addr, _, _, vi = _jolt(150, 700, 50)
    got = _check(cozk, ctx, RW, addr, [None] * 4, [None] * 4, vi)
    assert np.array_equal(got[3], np.asarray(vi, dtype=np.uint32)) and got[2] == [None] * 4
    for a in range(50):  # t_final is the last touch
        assert got[4][a] == max([j for s in range(4) for j in range(700) if addr[s][j] == a], default=0)


def test_every_slot_writing_at_every_step(cozk, ctx, RW):
    addr, vw, _, vi = _jolt(151, 700, 50)
    _, vw2, _, _ = _jolt(152, 700, 50)
    got = _check(cozk, ctx, RW, addr, [vw2[2], vw2[3], vw[2], vw[3]], [None] * 4, vi)
    assert got[2] == [None] * 4


@pytest.mark.parametrize("pct", [0, 10, 100])
def test_store_flags_at_every_density(cozk, ctx, RW, pct):
    got = _check(cozk, ctx, RW, *_jolt(160 + pct, 1500, 300, store_pct=pct, n_regs=32))
    assert got[2][3] is not None and got[2][:3] == [None] * 3


def test_a_u8_address_column_beside_u32_ones(cozk, ctx, RW):
    addr, vw, iw, vi = _jolt(170, 900, 300, n_regs=256)
    addr[1][:4] = [255, 0, 255, 254]
    _check(cozk, ctx, RW, addr, vw, iw, vi, addr_kinds=["U8", "U8", "U32", "U32"])
    _check(cozk, ctx, RW, addr, vw, iw, vi, addr_kinds=["U32", "U8", "U8", "U32"])


def test_the_same_call_twice_gives_the_same_bytes(cozk, ctx, RW, T):
    args = _jolt(180, T // 4 + 300, (1 << 16) + 500, n_regs=32)
    up = _upload(cozk, ctx, *args)
    runs = []
    for _ in range(2):
        out = RW.rw_memory_witness(ctx, *up)
        runs.append([v.to_numpy().tobytes() for group in out[:3] for v in group if v is not None] + [out[3].to_numpy().tobytes(), out[4].to_numpy().tobytes()])
    assert len(runs[0]) == 11 and runs[0] == runs[1]
    _check(cozk, ctx, RW, *args)


def _refused(cozk, ctx, RW, text, *args, **kw):
    with pytest.raises(cozk.CozkError) as e:
        _device(cozk, ctx, RW, *args, **kw)
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals(cozk, ctx, RW):
    n, MEM = 200, 16
    addr, vw, iw, vi = _jolt(190, n, MEM)
    bad = [list(c) for c in addr]
    bad[3][77] = MEM      # an address equal to MEM ...
    bad[1][77] = MEM + 5  # ... the smallest (step, slot) is named
    bad[0][150] = 1 << 31
    _refused(cozk, ctx, RW, "step 77, slot 1:", bad, vw, iw, vi)
    _refused(cozk, ctx, RW, "is_write[s] given without v_write[s]", addr, [None, None, vw[2], None], iw, vi)
    _refused(cozk, ctx, RW, "addr[s] is a U8 or U32 vector", addr, vw, iw, vi, addr_kinds=["U32", "U16", "U32", "U32"])
    _refused(cozk, ctx, RW, "addr[s] has n entries", [addr[0], addr[1][:-1], addr[2], addr[3]], vw, iw, vi)
    _refused(cozk, ctx, RW, "v_write[s] and is_write[s] have n entries", addr, [None, None, vw[2][:-1], vw[3]], iw, vi)
    _refused(cozk, ctx, RW, "v_write[s] and is_write[s] have n entries", addr, vw, [None, None, None, iw[3] + [1]], vi)
    _refused(cozk, ctx, RW, "1 <= n_slots <= 8", addr * 3, vw * 3, iw * 3, vi)
    a, w, f, i = _upload(cozk, ctx, addr, vw, iw, vi)
    with pytest.raises(cozk.CozkError) as e:  # v_write of a kind other than U32
        RW.rw_memory_witness(ctx, a, [None, None, w[2], f[3]], f, i)
    assert e.value.code == INVALID_ARG and "v_write[s] is a U32 vector" in str(e.value)
    with pytest.raises(cozk.CozkError) as e:
        RW.rw_memory_witness(ctx, a, w, f, f[3])
    assert e.value.code == INVALID_ARG and "v_init is a U32 vector" in str(e.value)
    _check(cozk, ctx, RW, addr, vw, iw, vi)  # the context works on after a refusal


def test_outputs_are_the_columns_of_the_memory_checking_leaves(cozk, ctx, RW):
    """end to end through the project's leaf kernel: the call's Vecs, as they are, are the compact columns of cozk_fingerprint_leaves;
    init * prod writes == prod reads * final over the downloaded leaves, and no longer once one t_final entry is bumped"""
    n, MEM, ns = 300, 500, 4
    addr, vw, iw, vi = _jolt(200, n, MEM, n_regs=32)
    a, w, f, init = _upload(cozk, ctx, addr, vw, iw, vi)
    v_read, t_read, v_written, v_final, t_final = RW.rw_memory_witness(ctx, a, w, f, init)
    rng = O.SplitMix64(201)
    g, tau = rng.field(), rng.field()
    coeffs, const = [1, g, g * g % O.R], (-tau) % O.R
    iota_n = cozk.Vec.from_numpy(ctx, np.arange(n, dtype=np.uint32), cozk.SCALAR_U32)
    iota_mem = cozk.Vec.from_numpy(ctx, np.arange(MEM, dtype=np.uint32), cozk.SCALAR_U32)
    written = [v_read[0], v_read[1], w[2], v_written[3]]  # what each slot leaves behind: read-only, always writing, flagged

    def product(cols, count):
        out = cozk.Vec.alloc(ctx, count)
        cozk.fingerprint_leaves(ctx, cols, coeffs[:len(cols)], [], [], const, "plain", 0, out, n=count)
        p = 1
        for x in out.to_ints():
            p = p * x % O.R
        return p

    reads = writes = 1
    for s in range(ns):
        reads = reads * product([a[s], v_read[s], t_read[s]], n) % O.R
        writes = writes * product([a[s], written[s], iota_n], n) % O.R
    inits = product([iota_mem, init], MEM)  # the init fingerprint carries no time
    finals = product([iota_mem, v_final, t_final], MEM)
    assert inits * writes % O.R == reads * finals % O.R
    want = W.replay(addr, vw, iw, vi)
    assert (inits, writes, reads, finals) == W.hashes(addr, vi, want[0], want[1], W.written(vw, iw, want[0]), want[3], want[4], g, tau)
    bumped = t_final.to_numpy()
    bumped[addr[2][10]] += 1
    finals = product([iota_mem, v_final, cozk.Vec.from_numpy(ctx, bumped, cozk.SCALAR_U32)], MEM)
    assert inits * writes % O.R != reads * finals % O.R
