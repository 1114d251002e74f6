"""GPU: the digit forms of the small-scalar MSM columns (COZK_MSM_DIGIT_FORM = plain | offset | auto), the one-launch fold
of heavy buckets and the wide / narrow sort shapes (csrc/msm.hip).  Bar: bit-exact against the big-int oracle.

Bases are s_i * G generated on the device from known scalars, so the expected point of a column v is
(sum_i s_i v_i mod r) * G: one oracle multiplication whatever the length.  The smallest shapes are also checked against
O.msm_naive over the downloaded points."""
import functools
import json
import os
import subprocess
import sys

import pytest

import pyref as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = ("plain", "offset", "auto")
LIMBS = {"U16": 1, "U32": 2, "U64": 4}
SRS_SEED, SRS_N = 515, 1024


@pytest.fixture(scope="module")
def srs(cozk, ctx):
    """1024 bases s_i * G with the window table, and the s_i"""
    s = _srs_scalars(SRS_SEED, SRS_N)
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, SRS_N, seed=SRS_SEED), precompute=True)
    yield B, s
    B.free()


@functools.lru_cache(maxsize=None)
def _srs_scalars(seed, n):
    return O.synthetic_fr(seed, n)


def _expect(s, off, vals):
    return O.g1_mul(O.G1_GEN, sum(a * (b % O.R) for a, b in zip(s[off:off + len(vals)], vals)) % O.R)


def _same_limb(e, limbs):
    return sum(e << (16 * k) for k in range(limbs))


def _column(name, kind, n):
    limbs = LIMBS[kind]
    bits = 16 * limbs
    if name == "uniform":
        return O.synthetic_small(900 + limbs + n, n, bits)
    if name == "zero":
        return [0] * n
    if name == "half":  # 0x8000 in every limb: every offset digit is zero, the result is the correction alone
        return [_same_limb(0x8000, limbs)] * n
    if name == "ones":
        return [(1 << bits) - 1] * n
    if name == "boundary":
        return [_same_limb((32767, 32768, 32769)[i % 3], limbs) for i in range(n)]
    raise ValueError(name)


@pytest.mark.parametrize("name", ["uniform", "zero", "half", "ones", "boundary"])
@pytest.mark.parametrize("n", [1, 2, 63, 700])
@pytest.mark.parametrize("kind", sorted(LIMBS))
def test_every_form_equals_the_oracle(cozk, ctx, srs, monkeypatch, kind, n, name):
    B, s = srs
    vals = _column(name, kind, n)
    v = cozk.Vec.from_ints(ctx, vals, kind=getattr(cozk, "SCALAR_" + kind))
    want = _expect(s, 0, vals)
    if n <= 2:
        assert want == O.msm_naive(B.download()[:n], vals)
    if name == "zero":
        assert want is None
    for form in FORMS:
        monkeypatch.setenv("COZK_MSM_DIGIT_FORM", form)
        assert B.msm(v) == want, form
    if name in ("zero", "half"):
        # the reference total the profile counter reports shows which form `auto` took: an all-zero column places nothing
        # in plain form (n per limb in offset form), a column of 0x8000 limbs nothing in offset form
        monkeypatch.setenv("COZK_MSM_DIGIT_FORM", "auto")
        ctx.prof_enable(True)
        assert B.msm(v) == want
        adds = ctx.prof_read()[2]
        ctx.prof_enable(False)
        assert adds == 0, (name, adds)
    v.free()


def test_unknown_form_is_refused(cozk, ctx, srs, monkeypatch):
    B, _ = srs
    monkeypatch.setenv("COZK_MSM_DIGIT_FORM", "sideways")
    v = cozk.Vec.from_ints(ctx, [1, 2, 3], kind=cozk.SCALAR_U16)
    with pytest.raises(cozk.CozkError):
        B.msm(v)
    v.free()


def _mixed_vecs(cozk, ctx, n, seed):
    kinds = ["FR", "U8", "U16", "U32", "U64", "I64", "U16", "U64"]
    vecs = []
    for p, kind in enumerate(kinds):
        k = getattr(cozk, "SCALAR_" + kind)
        if kind == "I64":
            rng = O.SplitMix64(seed + p)
            vals = [(-1) ** i * (rng.next() >> (1 + i % 40)) for i in range(n)]
            vecs.append(cozk.Vec.from_ints(ctx, vals, kind=k))
        else:
            vecs.append(cozk.Vec.random(ctx, n, seed=seed + p, kind=k, max_bits=1 if kind == "U8" else 0))
    return vecs


@pytest.mark.parametrize("form", FORMS)
def test_mixed_batch_on_two_slices_of_one_srs(cozk, ctx, monkeypatch, form):
    """FR, 0/1 U8, U16, U32, U64 and I64 columns in one batch at a non-zero base offset, on two different (offset, n) slices
    of the same bases: the correction belongs to the slice.  A fresh Bases per form, so the first pass computes the slice
    sums and the second one finds them cached."""
    monkeypatch.setenv("COZK_MSM_DIGIT_FORM", form)
    s = _srs_scalars(SRS_SEED, SRS_N)
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, SRS_N, seed=SRS_SEED), precompute=True)
    cases = [(13, 700, 40), (200, 300, 60)]
    want = {}
    for _pass in range(2):
        for off, n, seed in cases:
            vecs = _mixed_vecs(cozk, ctx, n, seed)
            if (off, n) not in want:
                want[(off, n)] = [_expect(s, off, v.to_ints()) for v in vecs]
            assert B.batch_msm(vecs, offset=off) == want[(off, n)], (off, n, _pass)
            for v in vecs:
                v.free()
    B.free()


def test_table_with_infinity_and_repeated_points_forced_offset(cozk, ctx, monkeypatch):
    n = 200
    rng = O.SplitMix64(66)
    g = [O.g1_mul(O.G1_GEN, rng.field()) for _ in range(5)]
    pts = [None if i % 17 == 3 else g[i % 5] for i in range(n)]
    pts[1] = O.g1_neg(g[0])
    vals = O.synthetic_small(67, n, 16)
    vals[0], vals[1], vals[2] = 0, 32768, 65535
    B = cozk.Bases.upload(ctx, pts, precompute=True)
    v = cozk.Vec.from_ints(ctx, vals, kind=cozk.SCALAR_U16)
    want = O.msm_naive(pts, vals)
    for form in ("offset", "plain", "auto"):
        monkeypatch.setenv("COZK_MSM_DIGIT_FORM", form)
        assert B.msm(v) == want, form
    # a slice whose points sum to infinity: S = g0 - g0
    monkeypatch.setenv("COZK_MSM_DIGIT_FORM", "offset")
    v2 = cozk.Vec.from_ints(ctx, [40000, 7], kind=cozk.SCALAR_U16)
    assert B.msm(v2) == O.msm_naive(pts[:2], [40000, 7])
    v.free()
    v2.free()
    B.free()


@pytest.mark.parametrize("precompute", [True, False])
@pytest.mark.parametrize("n", [9, 600, 40000])
def test_heavy_buckets_fold_in_one_launch(cozk, ctx, monkeypatch, n, precompute):
    """a U8 column of all ones and a plain U16 column of all 65535 (digit -1 plus the carry digit) put n references into one
    bucket each, beside an FR column: at L0 = 8 that is n / 8 level-0 segments.  n = 9: two segments, the first fold level
    finishes everything and the heavy list is empty; n = 600: 75 segments -> 10 partial sums; n = 40 000: 5000 -> 625, so
    k_msm_fold_heavy runs its strided part and its tree.  Without the window table the sort is the old one, the folds the same."""
    monkeypatch.setenv("COZK_MSM_DIGIT_FORM", "plain")
    s = _srs_scalars(77, 40000)[:n]  # the random stream is indexed by position: a prefix is the shorter stream
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, n, seed=77), precompute=precompute)
    ones = cozk.Vec.from_ints(ctx, [1] * n, kind=cozk.SCALAR_U8)
    top = cozk.Vec.from_ints(ctx, [65535] * n, kind=cozk.SCALAR_U16)
    fr = cozk.Vec.random(ctx, n, seed=78)
    total = sum(s) % O.R
    want = [O.g1_mul(O.G1_GEN, total), O.g1_mul(O.G1_GEN, 65535 * total), _expect(s, 0, fr.to_ints())]
    assert B.batch_msm([ones, top, fr]) == want
    for v in (ones, top, fr):
        v.free()
    B.free()


MANY_N = 100000


@pytest.fixture(scope="module")
def srs_many(cozk, ctx):
    s = _srs_scalars(88, MANY_N)
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, MANY_N, seed=88), precompute=True)
    yield B, s
    B.free()


def test_thousands_of_slightly_heavy_buckets(cozk, ctx, srs_many):
    """16 uniform U8 columns of 100 000 scalars: 255 buckets of ~390 references per column.  The set holds 1.6 M references,
    so L0 = 8 and a bucket has ~49 level-0 segments; the plan sizes the fold levels for digits spread over all 2^15 buckets
    (4 references per bucket: one level), after which each of the 16 x 255 = 4080 buckets still holds 7 partial sums and
    goes through the heavy list: several buckets per workgroup of k_msm_fold_heavy, three tree steps each."""
    B, s = srs_many
    vecs = [cozk.Vec.random(ctx, MANY_N, seed=500 + p, kind=cozk.SCALAR_U8) for p in range(16)]
    want = [_expect(s, 0, v.to_ints()) for v in vecs]
    assert B.batch_msm(vecs) == want
    for v in vecs:
        v.free()


def test_two_planned_fold_levels_then_the_heavy_launch(cozk, ctx, srs_many):
    """a uniform FR column of 100 000 scalars (49 references per bucket, 7 segments at L0 = 8: the plan allows
    ceil(1.25 x 49 / 8) + 1 = 9 and queues two fold levels) beside an all-ones U8 column (100 000 references in one bucket:
    12 500 segments -> 1563 -> 196 partial sums for the heavy launch, read from the second ping-pong buffer) and a uniform one"""
    B, s = srs_many
    vecs = [cozk.Vec.random(ctx, MANY_N, seed=600), cozk.Vec.from_ints(ctx, [1] * MANY_N, kind=cozk.SCALAR_U8),
            cozk.Vec.random(ctx, MANY_N, seed=601, kind=cozk.SCALAR_U8)]
    want = [_expect(s, 0, v.to_ints()) for v in vecs]
    assert B.batch_msm(vecs) == want
    for v in vecs:
        v.free()


_CHILD = r"""
import importlib, json, sys
sys.path[:0] = [{root!r}, {oracle!r}, {tests!r}]
import test_gpu_msm_digit_forms as T
cozk = importlib.import_module("co-zkvms_amd")
ctx = cozk.Context(0)
print("POINTS " + json.dumps(T.sort_shape_points(cozk, ctx, False)[0]))
ctx.close()
"""
SHAPE_N = 5000  # two sort workgroups per polynomial


def sort_shape_points(cozk, ctx, with_ints=True):
    """a mixed batch in one launch set, then 70 columns (launch sets of 64 + 6)"""
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, SHAPE_N, seed=91), precompute=True)
    one = _mixed_vecs(cozk, ctx, SHAPE_N, 300)
    two = [cozk.Vec.random(ctx, SHAPE_N, seed=400 + p, kind=cozk.SCALAR_U16 if p % 2 else cozk.SCALAR_U32) for p in range(70)]
    out = [B.batch_msm(one), B.batch_msm(two)]
    ints = [[v.to_ints() for v in one], [v.to_ints() for v in two]] if with_ints else None
    for v in one + two:
        v.free()
    B.free()
    return out, ints


def test_wide_and_narrow_sort_shapes(cozk, ctx):
    """The first launch set of a batch is sorted by wide workgroups, the sets that run beside a gather pass by 256-thread
    ones; under COZK_MSM_SERIAL every set is wide.  That knob is read once per process, so the serial leg runs in a child.
    Both legs == the oracle."""
    s = _srs_scalars(91, SHAPE_N)
    got, ints = sort_shape_points(cozk, ctx)
    want = [[_expect(s, 0, vals) for vals in batch] for batch in ints]
    assert got == want
    env = dict(os.environ, COZK_MSM_SERIAL="1")
    code = _CHILD.format(root=ROOT, oracle=os.path.join(ROOT, "oracle"), tests=HERE)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("POINTS ")][-1]
    assert json.loads(line[len("POINTS "):]) == [[None if p is None else list(p) for p in batch] for batch in want]
