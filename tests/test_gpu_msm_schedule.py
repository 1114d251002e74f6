"""GPU: the launch schedule of the batched MSM (csrc/host/msm_schedule.hpp, executed by csrc/msm.hip) -- which sets are sorted wide and how many sort workgroups a
column of each kind gets -- changes no commitment.  Bar: bit-exact against the big-int oracle.

Bases are s_i * G generated on the device from known scalars (as in test_gpu_msm_digit_forms.py), so the expected point of
a column v is (sum_i s_i v_i mod r) * G.  COZK_MSM_SET_REFS_LOG2 cuts small batches into many launch sets; the decisions
the library takes are read from its COZK_TRACE_MSM lines in a child process and compared with the Python restatement of
the two rules in test_msm_schedule_model.py."""
import functools
import json
import os
import re
import subprocess
import sys

import pytest

import pyref as O
import test_msm_schedule_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRS_SEED, SRS_N = 717, 4097
NBITS = {"U8": 8, "U16": 16, "U32": 32, "U64": 64}
# the A/B switches of the schedule, each on and off (they are read at every call)
SWITCHES = [{}, {"COZK_MSM_SHAPE_RULE": "0"}, {"COZK_MSM_SHAPE_RULE": "1"}, {"COZK_MSM_WG_DIGITS_LOG2": "0"},
            {"COZK_MSM_WG_DIGITS_LOG2": "12"}, {"COZK_MSM_WG_DIGITS_LOG2": "16"}, {"COZK_MSM_WG_DIGITS_LOG2": "18"},
            {"COZK_MSM_SHAPE_RULE": "0", "COZK_MSM_WG_DIGITS_LOG2": "0"}]


@functools.lru_cache(maxsize=None)
def _srs_scalars():
    return O.synthetic_fr(SRS_SEED, SRS_N)


@pytest.fixture(scope="module")
def srs(cozk, ctx):
    B = make_bases(cozk, ctx)
    yield B, _srs_scalars()
    B.free()


def make_bases(cozk, ctx):
    return cozk.Bases.from_scalars(ctx, cozk.Vec.random(ctx, SRS_N, seed=SRS_SEED), precompute=True)


def _expect(vals):
    return O.g1_mul(O.G1_GEN, sum(a * (b % O.R) for a, b in zip(_srs_scalars(), vals)) % O.R)


def make_vecs(cozk, ctx, cols, seed):
    """cols: [(kind name, n)] as in the model; FR / U16 / U32 / U64 columns uniform, U8 columns 0/1 flags"""
    return [cozk.Vec.random(ctx, n, seed=seed + p, kind=getattr(cozk, "SCALAR_" + kind), max_bits=1 if kind == "U8" else 0)
            for p, (kind, n) in enumerate(cols)]


CASES = {"many": M.MANY, "flag_first": M.small_large(True), "flag_last": M.small_large(False),
         "tail_blocks": [("FR", 64)] * 200 + [("U8", 64)] * 57}


def case_points(cozk, ctx, B, name, with_ints=False):
    vecs = make_vecs(cozk, ctx, CASES[name], 3000)
    got = B.batch_msm(vecs)
    ints = [v.to_ints() for v in vecs] if with_ints else None
    for v in vecs:
        v.free()
    return got, ints


_CHILD = r"""
import importlib, json, sys
sys.path[:0] = [{root!r}, {oracle!r}, {tests!r}]
import test_gpu_msm_schedule as T
cozk = importlib.import_module("co-zkvms_amd")
ctx = cozk.Context(0)
B = T.make_bases(cozk, ctx)
T.case_points(cozk, ctx, B, {case!r})  # the first pass also computes the slice sums (one-column MSMs of their own)
sys.stderr.write("MARK\n")
sys.stderr.flush()
print("POINTS " + json.dumps(T.case_points(cozk, ctx, B, {case!r})[0]))
B.free()
ctx.close()
"""
_TRACE = re.compile(r"^cozk msm set (\d+): polys (\d+) refs (\d+) shape (wide|narrow) (\d+)x(\d+) kinds((?: \w+:\d+:\d+)*)$")


def run_child(case, **env):
    """-> (points, trace) of the second pass over `case` in a fresh process; trace = [(index, polys, refs, shape, ltpb, wgs cap, kinds)]"""
    code = _CHILD.format(root=ROOT, oracle=os.path.join(ROOT, "oracle"), tests=HERE, case=case)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=dict(os.environ, COZK_TRACE_MSM="1", **env),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    points = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("POINTS ")][-1][len("POINTS "):])
    err = r.stderr.splitlines()
    trace = []
    for ln in err[err.index("MARK") + 1:]:
        m = _TRACE.match(ln)
        if m:
            kinds = [(k, int(c), int(w)) for k, c, w in (t.split(":") for t in m.group(7).split())]
            trace.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)), int(m.group(6)), kinds))
    return points, trace


def as_json(points):
    return [None if p is None else list(p) for p in points]


def model_trace(cols, cap, digits_log2=M.WG_DIGITS_LOG2):
    return [(i, p, m, sh, kinds) for i, (p, m, sh, kinds) in enumerate(M.schedule(cols, cap, digits_log2))]


def test_many_sets_under_every_switch(cozk, ctx, srs, monkeypatch):
    """24 columns at n = 1024 in the bench's mix and order, cut into 19 launch sets: both sort workspaces are reused, the
    cheapest set is rotated to the front.  Every switch of the schedule, the serial batch and the narrow-only shape give
    the oracle's commitments."""
    B, _ = srs
    assert len(M.cut_sets(M.MANY, 1 << 12)) >= 5
    monkeypatch.setenv("COZK_MSM_SET_REFS_LOG2", "12")
    got, ints = case_points(cozk, ctx, B, "many", with_ints=True)
    want = [_expect(v) for v in ints]
    assert got == want
    for sw in SWITCHES:
        with monkeypatch.context() as mp:
            for k, v in sw.items():
                mp.setenv(k, v)
            assert case_points(cozk, ctx, B, "many")[0] == want, sw
    # COZK_MSM_SERIAL and COZK_MSM_LTPB / COZK_MSM_WGS are read once per process: children
    model = model_trace(M.MANY, 1 << 12)
    points, trace = run_child("many", COZK_MSM_SET_REFS_LOG2="12", COZK_MSM_SERIAL="1")
    assert points == as_json(want)
    assert [(t[0], t[1], t[2], t[6]) for t in trace] == [(m[0], m[1], m[2], m[4]) for m in model]
    assert all(t[3] == M.WIDE and t[4] == 1024 for t in trace)  # nothing runs beside any sort of a serial batch
    points, trace = run_child("many", COZK_MSM_SET_REFS_LOG2="12", COZK_MSM_LTPB="256", COZK_MSM_WGS="64")
    assert points == as_json(want)
    assert [(t[0], t[1], t[2], t[3], t[6]) for t in trace] == model
    assert all(t[4] == 256 and t[5] == 64 for t in trace)


def _values(name, kind, n):
    bits = NBITS[kind]
    limbs = max(bits // 16, 1)
    if name == "equal":  # one bucket per window takes everything
        return [sum(3 << (16 * k) for k in range(limbs)) if bits > 8 else 3] * n
    if name == "zero":
        return [0] * n
    if name == "boundary":  # around the sign change of the offset digits; for U8 around the top of its single digit
        if bits == 8:
            return [(127, 128, 255)[i % 3] for i in range(n)]
        return [sum((32767, 32768, 32769)[i % 3] << (16 * k) for k in range(limbs)) for i in range(n)]
    return O.synthetic_small(1200 + bits + n, n, bits)  # uniform


@pytest.mark.parametrize("kind", sorted(NBITS))
def test_workgroup_counts_at_their_edges(cozk, ctx, srs, monkeypatch, kind):
    """Per narrow kind: the lengths around one workgroup per 4096 scalars (the rule of COZK_MSM_WG_DIGITS_LOG2=0), and at 2^12
    digits per workgroup the longest column with one workgroup and the shortest with two; at the default 2^16 every one of
    them is a single workgroup.  All-equal, all-zero, boundary and uniform values, plain and offset form."""
    B, _ = srs
    nwin = M.NWIN[kind]
    one = (1 << 12) // nwin
    assert M.workgroups([(kind, one)], 12)[0][2] == 1 and M.workgroups([(kind, one + 1)], 12)[0][2] == 2
    forms = ("plain", "offset") if kind != "U8" else ("plain",)
    for n in sorted({1, 2, 4095, 4096, 4097, one, one + 1}):
        for name in ("equal", "zero", "boundary", "uniform"):
            vals = _values(name, kind, n)
            want = _expect(vals)
            if n <= 2:
                assert want == O.msm_naive(B.download(0, n), vals)
            if name == "zero":
                assert want is None
            v = cozk.Vec.from_ints(ctx, vals, kind=getattr(cozk, "SCALAR_" + kind))
            for form in forms:
                for log2 in ("16", "12", "0"):
                    monkeypatch.setenv("COZK_MSM_DIGIT_FORM", form)
                    monkeypatch.setenv("COZK_MSM_WG_DIGITS_LOG2", log2)
                    assert B.msm(v) == want, (n, name, form, log2)
            v.free()


@pytest.mark.parametrize("case,cap_log2,digits_log2", [("flag_first", 16, 16), ("flag_last", 16, 16), ("flag_last", 19, 16),
                                                        ("flag_first", 19, 11)])
def test_small_set_beside_a_large_one(cozk, ctx, srs, case, cap_log2, digits_log2):
    """one flag column and eight field-element columns, n = 4096, in both orders.  Cut one column per set (cap 2^16) the
    flag set runs first either way and the first field-element set behind it is sorted wide, the others narrow; cut at 2^19
    the eight field-element columns are one set in front of the flag (wide, then narrow), or the flag shares the first set.
    The trace shows the shapes and the workgroups per kind that the model gives."""
    B, _ = srs
    env = {"COZK_MSM_SET_REFS_LOG2": str(cap_log2)}
    if digits_log2 != M.WG_DIGITS_LOG2:
        env["COZK_MSM_WG_DIGITS_LOG2"] = str(digits_log2)
    points, trace = run_child(case, **env)
    got, ints = case_points(cozk, ctx, B, case, with_ints=True)
    want = [_expect(v) for v in ints]
    assert got == want and points == as_json(want)
    assert [(t[0], t[1], t[2], t[3], t[6]) for t in trace] == model_trace(CASES[case], 1 << cap_log2, digits_log2)
    for t in trace:
        assert (t[4], t[5]) == ((1024, 64) if t[3] == M.WIDE else (256, 64))
    assert M.WIDE in [t[3] for t in trace[1:]] or cap_log2 == 19


def test_two_tail_blocks_on_a_window_table(cozk, ctx, srs):
    """257 columns of 64 scalars: the smallest batch that crosses the 256 bucket groups of one reduction tail on a window table.  The
    first block is four launch sets of 64 columns, the second a single flag column, sorted wide because nothing runs beside it; the
    set index starts again in every block.  Commitments from the big-int oracle, the trace from the model applied block by block."""
    B, _ = srs
    cols = CASES["tail_blocks"]
    assert [len(b) for b in M.blocks(cols)] == [256, 1]
    points, trace = run_child("tail_blocks")
    got, ints = case_points(cozk, ctx, B, "tail_blocks", with_ints=True)
    want = [_expect(v) for v in ints]
    assert got == want and points == as_json(want)
    assert [(t[0], t[1], t[2], t[3], t[6]) for t in trace] == [m for blk in M.blocks(cols) for m in model_trace(blk, None)]
    assert [t[1] for t in trace] == [64, 64, 64, 64, 1] and trace[-1][0] == 0 and trace[-1][3] == M.WIDE
