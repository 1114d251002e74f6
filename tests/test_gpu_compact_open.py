"""GPU tests of the compact-column openings (cozk_compact_batch_evaluate_at_chi, cozk_compact_linear_combination;
csrc/compact_open.inc): exact equality with Python integers and, byte for byte, with the Fr-polynomial calls on PLAIN polynomials of
the same values.  Lengths around a wave, a workgroup and the evaluation grid (a lane carries 16 terms before a second workgroup
starts: 4097 has two workgroups, 2^16 + 3 seventeen, the last one partial); 1, 2, 3, 8, 9, 20 and 24 columns (a workgroup row carries
8: one, two and three rows, full and partial); every kind alone and
all four in one call; all-zero and all-ones columns against chi entries all r - 1; a chi longer than the columns; the refusals.  The
accumulator's bound of 2^32 terms cannot be reached (both calls refuse n >= 2^32): tests/test_ts_proof_model.py holds its model."""
import importlib

import numpy as np
import pytest

import pyref as O

pytestmark = pytest.mark.gpu
R = O.R
INVALID_ARG = -1
LENGTHS = [1, 2, 63, 64, 65, 256, 257, 4097, (1 << 15) + 3, (1 << 16) + 3]
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
NMAX = max(LENGTHS)


@pytest.fixture(scope="module")
def TP():
    return importlib.import_module("co-zkvms_amd.ts_proof")


def _kind(cozk, bits):
    return {8: cozk.SCALAR_U8, 16: cozk.SCALAR_U16, 32: cozk.SCALAR_U32, 64: cozk.SCALAR_U64}[bits]


def _col(cozk, ctx, values, bits):
    return cozk.Vec.from_numpy(ctx, np.asarray(values, dtype=DTYPES[bits]), _kind(cozk, bits))


def _poly(cozk, ctx, values):
    return cozk.Rep3DensePolynomial.new(ctx, [int(v) for v in values])


@pytest.fixture(scope="module")
def data(cozk, ctx):
    """24 random columns of NMAX + 40 entries, kinds cycling U8, U16, U32, U64, and a random chi of the same length: made once; every
    test slices them"""
    rng = np.random.default_rng(500)
    bits = [(8, 16, 32, 64)[c % 4] for c in range(24)]
    cols = [rng.integers(0, 1 << b, size=NMAX + 40, dtype=np.uint64) for b in bits]
    sm = O.SplitMix64(501)
    chi = [sm.field() for _ in range(NMAX + 40)]
    return bits, cols, chi, cozk.Vec.from_ints(ctx, chi)


def _expect_eval(cols, chi, n):
    return [sum(int(c) * int(v) for c, v in zip(chi[:n], col[:n])) % R for col in cols]


@pytest.mark.parametrize("n", LENGTHS)
def test_evaluation_at_every_length_mixed_kinds(cozk, ctx, TP, data, n):
    bits, cols, chi, d_chi = data
    k = 5  # U8, U16, U32, U64, U8: all four kinds in one call; chi is longer than n
    vecs = [_col(cozk, ctx, cols[c][:n], bits[c]) for c in range(k)]
    got = TP.compact_batch_evaluate_at_chi(ctx, vecs, d_chi)
    assert got == _expect_eval(cols[:k], chi, n)
    if n in (65, 4097):  # ... and byte for byte the Fr call
        polys = [_poly(cozk, ctx, cols[c][:n]) for c in range(k)]
        assert got == cozk.Rep3DensePolynomial.batch_evaluate_at_chi(polys, d_chi)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 20, 24])
def test_evaluation_and_combination_at_every_column_count(cozk, ctx, TP, data, k):
    bits, cols, chi, d_chi = data
    n = 4097 + 256 * 3  # more than one workgroup, a partial last one
    vecs = [_col(cozk, ctx, cols[c][:n], bits[c]) for c in range(k)]
    raw = TP.compact_batch_evaluate_at_chi(ctx, vecs, d_chi, raw=True)
    assert cozk.mont_limbs_to_int(raw) == _expect_eval(cols[:k], chi, n)
    assert raw.tobytes() == TP.compact_batch_evaluate_at_chi(ctx, vecs, d_chi, raw=True).tobytes()  # the same call twice
    sm = O.SplitMix64(510 + k)
    coeffs = ([0, 1, R - 1] + [sm.field() for _ in range(k)])[:k] if k >= 3 else [sm.field() for _ in range(k)]
    out = TP.compact_linear_combination(ctx, vecs, coeffs)
    want = [sum(cf * int(cols[c][i]) for c, cf in enumerate(coeffs)) % R for i in range(n)]
    bytes1 = out.to_numpy().tobytes()
    assert len(out) == n and out.to_ints() == want
    assert bytes1 == TP.compact_linear_combination(ctx, vecs, coeffs).to_numpy().tobytes()
    if k in (3, 20):  # byte for byte the Fr calls, below and above the border of k_poly_lincomb's two forms
        polys = [_poly(cozk, ctx, cols[c][:n]) for c in range(k)]
        ref = cozk.Rep3DensePolynomial.linear_combination(polys, coeffs)
        assert ref.copy_share_a().to_numpy().tobytes() == bytes1
        assert cozk.Rep3DensePolynomial.batch_evaluate_at_chi(polys, d_chi) == cozk.mont_limbs_to_int(raw)


@pytest.mark.parametrize("n", LENGTHS)
def test_combination_at_every_length(cozk, ctx, TP, data, n):
    bits, cols, chi, d_chi = data
    k = 4
    vecs = [_col(cozk, ctx, cols[c][:n], bits[c]) for c in range(k)]
    coeffs = [chi[0], R - 1, 1, chi[1]]
    assert TP.compact_linear_combination(ctx, vecs, coeffs).to_ints() == [sum(cf * int(cols[c][i]) for c, cf in enumerate(coeffs)) % R for i in range(n)]


@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_each_kind_alone_with_extreme_values(cozk, ctx, TP, bits):
    n = 1000
    top = (1 << bits) - 1
    worst = cozk.Vec.from_ints(ctx, [R - 1] * n)  # every chi entry r - 1
    sm = O.SplitMix64(520 + bits)
    rnd = [sm.field() for _ in range(3)]
    chi = cozk.Vec.from_ints(ctx, (rnd * n)[:n])
    ones, zeros = _col(cozk, ctx, [top] * n, bits), _col(cozk, ctx, [0] * n, bits)
    ramp = _col(cozk, ctx, [(i * 2654435761) & top for i in range(n)], bits)
    assert TP.compact_batch_evaluate_at_chi(ctx, [ones, zeros, ramp], worst) == [n * (R - 1) * top % R, 0, sum((R - 1) * ((i * 2654435761) & top) for i in range(n)) % R]
    assert TP.compact_batch_evaluate_at_chi(ctx, [ones], chi) == [sum((rnd * n)[:n]) * top % R]
    out = TP.compact_linear_combination(ctx, [ones, zeros, ones], [R - 1, rnd[0], R - 1])
    assert out.to_ints() == [2 * (R - 1) * top % R] * n
    assert TP.compact_linear_combination(ctx, [zeros], [rnd[1]]).to_ints() == [0] * n


def _refused(cozk, text, call):
    with pytest.raises(cozk.CozkError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)


def test_refusals_and_a_good_call_after_them(cozk, ctx, TP, data):
    bits, cols, chi, d_chi = data
    n = 300
    vecs = [_col(cozk, ctx, cols[c][:n], bits[c]) for c in range(3)]
    fr = cozk.Vec.from_ints(ctx, chi[:n])
    i64 = cozk.Vec.from_numpy(ctx, np.arange(n, dtype=np.int64), cozk.SCALAR_I64)
    short = _col(cozk, ctx, cols[1][:n - 1], bits[1])
    short_chi = cozk.Vec.from_ints(ctx, chi[:n - 1])
    for name, call in (("compact_batch_evaluate", lambda v: TP.compact_batch_evaluate_at_chi(ctx, v, d_chi)),
                       ("compact_linear_combination", lambda v: TP.compact_linear_combination(ctx, v, [1] * len(v)))):
        _refused(cozk, name + ": the columns are U8 / U16 / U32 / U64 vectors", lambda: call([vecs[0], fr]))
        _refused(cozk, name + ": the columns are U8 / U16 / U32 / U64 vectors", lambda: call([i64]))
        _refused(cozk, name + ": every column has one length", lambda: call([vecs[0], short]))
        _refused(cozk, name + ": 1 <= k <= 24 columns", lambda: call([vecs[0]] * 25))
        _refused(cozk, name + ": 1 <= k <= 24 columns", lambda: call([]))
    _refused(cozk, "compact_batch_evaluate: chi shorter than the columns", lambda: TP.compact_batch_evaluate_at_chi(ctx, vecs, short_chi))
    _refused(cozk, "compact_batch_evaluate: chi is an FR vector", lambda: TP.compact_batch_evaluate_at_chi(ctx, vecs, vecs[2]))
    assert TP.compact_batch_evaluate_at_chi(ctx, vecs, d_chi) == _expect_eval(cols[:3], chi, n)  # the context works on
    assert TP.compact_linear_combination(ctx, vecs[:1], [3]).to_ints() == [3 * int(v) for v in cols[0][:n]]
