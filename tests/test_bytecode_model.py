"""CPU tests of tests/bytecode_ref.py: the word model of the exact-sum bytecode leaf kernels (csrc/bytecode_leaves.hip) against big-int
values at the saturating operands, from_i64 at its edges, the shape of the seeded instance at every size the GPU tests use, and the
multiset identity init * writes == reads * final over the instance's witness (and its failure when a counter or a value is bumped),
and the whole proof: verify(prove(cfg)) at (log_n, log_b) = (3, 2) and the three tampers rejected with their reasons."""
import random

import pytest

import bytecode_ref as B
import pyref as O

R = B.R
M64 = (1 << 64) - 1
EDGES = [0, 1, R - 1, None]
SIZES = [(2, 2), (8, 32), (64, 8), (64, 32), (64, 16), (256, 512), (1024, 1024), (65536, 16384), (1, 1), (2, 1), (1, 2), (63, 33), (257, 2), (257, 4097), (4097, 33), (4097, 65537), (32769, 4097)]  # the (N, B) of test_gpu_bytecode_proof.py, then those of test_gpu_bytecode_witness.py


@pytest.mark.parametrize("g", EDGES, ids=["g_zero", "g_one", "g_minus_one", "g_random"])
@pytest.mark.parametrize("tau", EDGES, ids=["tau_zero", "tau_one", "tau_minus_one", "tau_random"])
def test_word_model_equals_the_big_int_leaf_at_the_saturating_operands(g, tau):
    sm = O.SplitMix64(900)
    g = sm.field() if g is None else g
    tau = sm.field() if tau is None else tau
    cols = [M64] * 7
    want = B.read_write_leaves([cols[0]], [[c] for c in cols[1:6]], [cols[6]], [R - 1], g, tau)
    assert B.leaf_word_model(cols, B.mont(R - 1), g, tau) == (B.mont(want[0][0]), B.mont(want[1][0]))
    for imm in (B.I64_MIN, B.I64_MAX, -1, M64):  # the table's imm as I64, and as a U64 column
        table = [[0, M64] for _ in range(5)] + [[0, imm]]
        want = B.init_final_leaves(table, [0, M64], g, tau)
        assert B.init_final_word_model(1, [M64] * 5 + [imm], M64, g, tau) == (B.mont(want[0][1]), B.mont(want[1][1]))


def test_word_model_on_random_operands_of_mixed_widths():
    rng = random.Random(901)
    for _ in range(200):
        g, tau = rng.randrange(R), rng.randrange(R)
        cols = [rng.randrange(1 << rng.choice((8, 16, 32, 64))) for _ in range(7)]
        imm = rng.randrange(R)
        want = B.read_write_leaves([cols[0]], [[c] for c in cols[1:6]], [cols[6]], [imm], g, tau)
        assert B.leaf_word_model(cols, B.mont(imm), g, tau) == (B.mont(want[0][0]), B.mont(want[1][0]))


def test_word_model_of_the_narrow_path():
    """columns without a high half take one multiply-add chain per entry, as the kernels do for U8 / U16 / U32 columns"""
    rng = random.Random(903)
    for _ in range(100):
        g, tau = rng.randrange(R), rng.randrange(R)
        wide = tuple(rng.random() < 0.5 for _ in range(7))
        cols = [rng.randrange(1 << (64 if w else 32)) for w in wide]
        imm = rng.randrange(R)
        want = B.read_write_leaves([cols[0]], [[c] for c in cols[1:6]], [cols[6]], [imm], g, tau)
        assert B.leaf_word_model(cols, B.mont(imm), g, tau, wide) == (B.mont(want[0][0]), B.mont(want[1][0]))
        row = cols[:5] + [rng.choice((-1, 1)) * rng.randrange(1 << 31)]
        p = B._powers(g)
        i = rng.randrange(1 << 32)
        init = (i * p[1] + sum(row[k] * p[2 + k] for k in range(5)) + row[5] - tau) % R
        got = B.init_final_word_model(i, row, cols[6], g, tau, wide[:5] + (False, wide[6]), imm_signed=True)
        assert got == (B.mont(init), B.mont(init + cols[6] * p[7]))


def test_barrett_constant():
    assert B.BC_MU == (1 << 322) // R and B.BC_MU.bit_length() == 69
    assert [(B.BC_MU >> (32 * i)) & B.M32 for i in range(3)] == [0x8E8129EA, 0x291D1898, 0x15]  # BcParams::MU


def test_from_i64():
    assert B.from_i64(0) == 0 and B.from_i64(-1) == R - 1
    assert B.from_i64(B.I64_MIN) == R - (1 << 63) and B.from_i64(B.I64_MAX) == (1 << 63) - 1


@pytest.mark.parametrize("N,Bn", SIZES)
def test_instance_shape(N, Bn):
    a, table = B.bytecode_instance(77, N, Bn)
    assert len(a) == N and all(len(c) == Bn for c in table) and all(0 <= x < Bn for x in a)
    assert all(c[0] == 0 for c in table)  # the no-op row
    assert a[N - N // 8:] == [0] * (N // 8)  # the padding steps sit at row 0
    assert all(table[0][i] == 0x80000000 + 4 * i for i in range(1, Bn)) and all(max(table[k]) < 32 for k in (2, 3, 4))
    if Bn > 2:
        assert table[5][1] == B.I64_MIN and table[5][2] == B.I64_MAX
    if Bn >= 64:  # each sign is one seeded bit: 61 or more rows of one sign have a chance of 2^-60 (13 rows at B = 16 do occur)
        assert any(v < 0 for v in table[5][3:]) and any(v > 0 for v in table[5][3:]) and any(w >> 63 for w in table[1])
    _, _, t_read, t_final = B.witness(a, table)
    if N > Bn:
        assert max(t_final) >= 2 and max(t_read) >= 1  # some row is read at least twice
    if Bn > N:
        assert 0 in t_final  # some row is unvisited
    assert sum(t_final) == N


def test_verify_of_prove_holds_and_the_tampers_are_rejected_with_their_reasons():
    cfg = dict(log_n=3, log_b=2, seed=1)
    proof = B.prove(cfg)
    assert B.verify(proof, cfg) == (True, None, {k: True for k in B.ORDER})
    for tamper, reason in ((1, B.REASON_MULTISET), (2, B.REASON_LEAF), (3, B.REASON_MULTISET)):
        tcfg = dict(cfg, tamper=tamper)
        ok, why, checks = B.verify(B.prove(tcfg), tcfg)
        assert not ok and why == reason, (tamper, why, checks)
        if tamper != 2:
            assert [k for k in B.ORDER if not checks[k]] == [reason]  # only the multiset check can reject


def _hashes(a, table, v_read, v_imm, t_read, t_final, g, tau):
    rw = B.read_write_leaves(a, v_read, t_read, v_imm, g, tau)
    inf = B.init_final_leaves(table, t_final, g, tau)
    return [B.product(c) for c in rw], [B.product(c) for c in inf]


@pytest.mark.parametrize("N,Bn", [(8, 4), (64, 8), (16, 64)])
def test_multiset_identity_holds_over_the_witness_and_breaks_when_it_is_bumped(N, Bn):
    sm = O.SplitMix64(902)
    g, tau = sm.field(), sm.field()
    a, table = B.bytecode_instance(5, N, Bn)
    v_read, v_imm, t_read, t_final = B.witness(a, table)
    assert B.multiset_holds(*_hashes(a, table, v_read, v_imm, t_read, t_final, g, tau))
    bumped = [list(c) for c in v_read]
    bumped[2][N // 2] += 1  # v_rd
    assert not B.multiset_holds(*_hashes(a, table, bumped, v_imm, t_read, t_final, g, tau))
    tf = list(t_final)
    tf[a[N // 2]] += 1
    assert not B.multiset_holds(*_hashes(a, table, v_read, v_imm, t_read, tf, g, tau))
