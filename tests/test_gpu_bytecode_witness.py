"""GPU parity of the bytecode witness (`cozk_bytecode_witness`, csrc/ts_range_witness.hip) against the sequential loop of
tests/bytecode_ref.py: every output compared for exact equality.  Trace lengths 1, 2, 63, 257, 4097 and one step past a counter tile,
tables of 1, 2, 33, 4097 and 65537 rows (one radix pass and two; tables longer and shorter than the trace); every step at one row; the
address column as U32 and as U64; the imm extremes; a[j] >= B refused with the smallest such step named, and a good call after it."""
import importlib

import numpy as np
import pytest

import bytecode_ref as B

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
DTYPES = (np.uint64, np.uint64, np.uint8, np.uint8, np.uint8, np.int64)


@pytest.fixture(scope="module")
def BC():
    return importlib.import_module("co-zkvms_amd.bytecode")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("co-zkvms_amd.lasso").LASSO_TILE


def _kinds(cozk, address_u32=False):
    return (cozk.SCALAR_U32 if address_u32 else cozk.SCALAR_U64, cozk.SCALAR_U64, cozk.SCALAR_U8, cozk.SCALAR_U8, cozk.SCALAR_U8, cozk.SCALAR_I64)


def _upload(cozk, ctx, a, table, address_u32=False):
    dt = (np.uint32 if address_u32 else np.uint64,) + DTYPES[1:]
    d_table = [cozk.Vec.from_numpy(ctx, np.asarray(table[k], dtype=dt[k]), kind) for k, kind in enumerate(_kinds(cozk, address_u32))]
    return cozk.Vec.from_numpy(ctx, np.asarray(a, dtype=np.uint32), cozk.SCALAR_U32), d_table


def _check(cozk, ctx, BC, a, table, address_u32=False):
    d_a, d_table = _upload(cozk, ctx, a, table, address_u32)
    v_read, v_imm, t_read, t_final = BC.bytecode_witness(ctx, d_a, d_table)
    want_v, want_imm, want_tr, want_tf = B.witness(a, table)
    for k in range(5):
        assert v_read[k].kind == d_table[k].kind and len(v_read[k]) == len(a)
        assert v_read[k].to_numpy().tolist() == want_v[k], B.TABLE_NAMES[k]
    assert cozk.mont_limbs_to_int(v_imm.to_numpy()) == want_imm
    assert t_read.kind == cozk.SCALAR_U32 and t_read.to_numpy().tolist() == want_tr
    assert t_final.kind == cozk.SCALAR_U32 and t_final.to_numpy().tolist() == want_tf
    return [v.to_numpy().tobytes() for v in v_read + [v_imm, t_read, t_final]]


@pytest.mark.parametrize("n,Bn", [(1, 1), (2, 1), (1, 2), (63, 33), (257, 2), (257, 4097), (4097, 33), (4097, 65537)])
def test_witness_equals_the_sequential_loop(cozk, ctx, BC, n, Bn):
    a, table = B.bytecode_instance(800 + n + Bn, n, Bn)
    _check(cozk, ctx, BC, a, table)


def test_one_step_past_a_tile_is_deterministic(cozk, ctx, BC, T):
    a, table = B.bytecode_instance(811, T + 1, 4097)
    assert _check(cozk, ctx, BC, a, table) == _check(cozk, ctx, BC, a, table)


def test_every_step_at_one_row_with_a_u32_address_column(cozk, ctx, BC):
    _, table = B.bytecode_instance(812, 8, 33)
    table[0] = [x & 0xFFFFFFFF for x in table[0]]
    _check(cozk, ctx, BC, [2] * 300, table, address_u32=True)   # row 2 holds 2^63 - 1
    _check(cozk, ctx, BC, [1] * 257, table, address_u32=True)   # row 1 holds -2^63
    _check(cozk, ctx, BC, [0] * 63, table, address_u32=False)


def test_imm_extremes(cozk, ctx, BC):
    imm = [0, -1, 1, B.I64_MIN, B.I64_MAX, B.I64_MIN + 1, -(1 << 32), (1 << 32) - 1]
    table = [[7 * i for i in range(8)], [(1 << 64) - 1 - i for i in range(8)], [31] * 8, [0] * 8, list(range(8)), imm]
    _check(cozk, ctx, BC, [i % 8 for i in range(70)], table)


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_a_good_call_after_them(cozk, ctx, BC):
    n, Bn = 300, 33
    a, table = B.bytecode_instance(820, n, Bn)
    bad = list(a)
    bad[150], bad[77], bad[299] = Bn, 1 << 31, Bn + 5
    d_a, d_table = _upload(cozk, ctx, bad, table)
    _refused(cozk, "bytecode_witness: step 77: a[step] is >= B = 33", lambda: BC.bytecode_witness(ctx, d_a, d_table))
    bad[77] = a[77]
    d_a, _ = _upload(cozk, ctx, bad, table)
    _refused(cozk, "bytecode_witness: step 150:", lambda: BC.bytecode_witness(ctx, d_a, d_table))
    good, _ = _upload(cozk, ctx, a, table)
    u8 = cozk.Vec.from_numpy(ctx, np.zeros(Bn, dtype=np.uint8), cozk.SCALAR_U8)
    u64 = cozk.Vec.from_numpy(ctx, np.zeros(Bn, dtype=np.uint64), cozk.SCALAR_U64)
    short = cozk.Vec.from_numpy(ctx, np.zeros(Bn - 1, dtype=np.uint8), cozk.SCALAR_U8)
    swap = lambda k, v: d_table[:k] + [v] + d_table[k + 1:]
    _refused(cozk, "bytecode_witness: a is a U32 vector", lambda: BC.bytecode_witness(ctx, u8, d_table))
    _refused(cozk, "bytecode_witness: table[0] (address) is a U32 or U64 vector", lambda: BC.bytecode_witness(ctx, good, swap(0, u8)))
    _refused(cozk, "bytecode_witness: table[1] (bitflags) is a U64 vector", lambda: BC.bytecode_witness(ctx, good, swap(1, u8)))
    _refused(cozk, "bytecode_witness: table[2..4] (rd, rs1, rs2) are U8 vectors", lambda: BC.bytecode_witness(ctx, good, swap(3, u64)))
    _refused(cozk, "bytecode_witness: table[5] (imm) is an I64 vector", lambda: BC.bytecode_witness(ctx, good, swap(5, u64)))
    _refused(cozk, "bytecode_witness: every table column has B entries", lambda: BC.bytecode_witness(ctx, good, swap(4, short)))
    _refused(cozk, "bytecode_witness: six table columns", lambda: BC.bytecode_witness(ctx, good, swap(2, None)))
    _check(cozk, ctx, BC, a, table)  # the context works on after a refusal
