"""CPU test of the MSM launch schedule (co-zkvms_amd/csrc/host/msm_schedule.hpp): the stand-alone host program
tests/native/msm_schedule_check (built by co-zkvms_amd/build.py, no GPU and no project library) runs msm_schedule() -- the function
msm_batch executes -- on the cases below and prints every launch set: the COZK_TRACE_MSM line, extended by the tail block, the segment
plan, the buffer sizes, the workspace and the eligibility mask.  All of it is compared with the Python restatement in
test_msm_schedule_model.py, at the benchmark's own sizes too.  A refused case prints the refusal; the function raises every refusal
before it returns, so nothing of a refused batch has been launched."""
import os
import subprocess
import sys

import pytest

import test_msm_schedule_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "msm_schedule_check")
TABLE, GROUPS = 16, 1  # windows per handle: with the window table, without


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "co-zkvms_amd", "build.py"), "--msm-schedule-check"], check=True)
    return EXE


def case(cols, nwin=TABLE, n_bases=None, form="auto", shape_rule=True, digits_log2=M.WG_DIGITS_LOG2, cap_log2=0, serial=False, ltpb="-",
         wgs="-", offsets=None):
    """-> (text for the program, the model's arguments)"""
    offsets = offsets or [0] * len(cols)
    n_bases = max([n for _, n in cols] + [1]) if n_bases is None else n_bases
    text = "case %d %d %s %d %d %d %d %s %s %d\n" % (nwin, n_bases, form, shape_rule, digits_log2, cap_log2, serial, ltpb, wgs, len(cols))
    text += "".join("%s %d %d\n" % (kind, off, n) for (kind, n), off in zip(cols, offsets))
    return text, dict(cols=cols, table=nwin == TABLE, cap=(1 << cap_log2) if cap_log2 else None, digits_log2=digits_log2, shape_rule=shape_rule,
                      serial=serial, offset_forms=form != "plain"), form == "offset"


def expected(model_args, force):
    lines = []
    for b, sets in enumerate(M.batch(**model_args)):
        for s in sets:
            wide = s["shape"] == M.WIDE
            lines.append("cozk msm set %d: polys %d refs %d shape %s %dx%d kinds%s | block %d groups %d pipelined %d cols %d G %d nb %d bound %d L0 %d "
                         "maxseg0 %d fold %d part %d exc %d blk %d ws %d elig %x force %d"
                         % (s["index"], s["polys"], s["refs"], s["shape"], 1024 if wide else 256, 64, "".join(" %s:%d:%d" % k for k in s["kinds"]), b,
                            s["groups"], s["pipelined"], s["first"], s["G"], s["nb"], s["bound"], s["L0"], s["maxseg0"], s["fold_levels"], s["part"],
                            s["exc"], s["blk"], s["ws"], s["elig"], force))
    return lines


def run(exe, cases):
    """-> per case the program's lines"""
    out = subprocess.run([exe], input="".join(c[0] for c in cases), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = []
    for ln in out.stdout.splitlines():
        if ln.startswith("CASE "):
            assert int(ln[5:]) == len(got)
            got.append([])
        else:
            got[-1].append(ln)
    assert len(got) == len(cases)
    return got


MIXED_EMPTY = [("FR", 1024), ("U16", 0), ("U16", 1024), ("FR", 0), ("U8", 0), ("U32", 512), ("U64", 0), ("I64", 7)]
ALL_EMPTY = [("FR", 0), ("U16", 0), ("U8", 0)]
SCHEDULED = {
    "many at 2^12": case(M.MANY, cap_log2=12),
    "flag first at 2^16": case(M.small_large(True), cap_log2=16),
    "flag last at 2^16": case(M.small_large(False), cap_log2=16),
    "flag first at 2^19": case(M.small_large(True), cap_log2=19),
    "flag last at 2^19": case(M.small_large(False), cap_log2=19),
    **{"many, 2^%d digits per workgroup" % d: case(M.MANY, cap_log2=12, digits_log2=d) for d in (0, 11, 12, 16)},
    **{"flag first, 2^%d digits per workgroup" % d: case(M.small_large(True), cap_log2=19, digits_log2=d) for d in (0, 11, 12, 16)},
    "many, shape rule off": case(M.MANY, cap_log2=12, shape_rule=False),
    "flag first, shape rule off": case(M.small_large(True), cap_log2=16, shape_rule=False),
    "flag last, shape rule off, two sets": case(M.small_large(False), cap_log2=19, shape_rule=False),
    "bench at 2^20": case(M.bench_mix(1 << 20)),
    "bench at 2^22": case(M.bench_mix(1 << 22)),
    "one FR column of 2^24": case([("FR", 1 << 24)]),
    "one FR column of 2^20, no table": case([("FR", 1 << 20)], nwin=GROUPS),
    "257 columns": case([("FR", 64)] * 200 + [("U8", 64)] * 57),
    "257 columns, shape rule off": case([("FR", 64)] * 200 + [("U8", 64)] * 57, shape_rule=False),
    "17 columns, no table": case([("FR", 64)] * 9 + [("U16", 64)] * 8, nwin=GROUPS),
    "many, serial": case(M.MANY, cap_log2=12, serial=True),
    "many, serial, shape rule off": case(M.MANY, cap_log2=12, serial=True, shape_rule=False),
    "empty columns mixed in": case(MIXED_EMPTY),
    "empty columns mixed in, one column per set": case(MIXED_EMPTY, cap_log2=12),
    "all columns empty": case(ALL_EMPTY),
    "an empty set between others": case([("FR", 4096), ("U16", 0), ("FR", 4096), ("U8", 4096)], cap_log2=12),
    "forms plain": case(M.MANY, cap_log2=12, form="plain"),
    "forms offset": case(M.MANY, cap_log2=12, form="offset"),
    "slices at offsets": case([("FR", 100), ("U16", 50)], n_bases=150, offsets=[50, 100]),
}
REFUSED = {
    "a slice out of range in the last column of many sets": (case(M.MANY, cap_log2=12, n_bases=1024, offsets=[0] * 23 + [1]),
                                                             "msm: base slice out of range"),
    "a slice out of range in the set launched thirteenth": (case(M.MANY, cap_log2=12, n_bases=1024, offsets=[0] * 11 + [1] + [0] * 12),
                                                            "msm: base slice out of range"),
    "2^31 table entries": (case([("U8", 64)], n_bases=1 << 27), "msm: table too large for 31-bit refs"),
    "2^32 references": (case([("FR", 1 << 28)], nwin=GROUPS), "msm: batch too large (reference count exceeds 32 bits)"),
    "LTPB = 100": (case(M.MANY, ltpb="100"), "COZK_MSM_LTPB out of range"),
    "WGS = 0": (case(M.MANY, wgs="0"), "COZK_MSM_WGS out of range (1..1024)"),
    "WG_DIGITS_LOG2 = 9": (case(M.MANY, digits_log2=9), "COZK_MSM_WG_DIGITS_LOG2 must be 0 or 10..24"),
}


def test_schedule_equals_model(exe):
    names = list(SCHEDULED)
    for name, got in zip(names, run(exe, [SCHEDULED[n] for n in names])):
        want = expected(*SCHEDULED[name][1:])
        assert want, name
        assert got == want, name


def test_refusals(exe):
    names = list(REFUSED)
    for name, got in zip(names, run(exe, [REFUSED[n][0] for n in names])):
        assert got == ["REFUSED " + REFUSED[name][1]], name
    # cut into 19 sets, the two trailing flags launched first and the last field-element column thirteenth: executed set by set,
    # its refusal would come after twelve sets had been enqueued
    order = [s["first"] for s in M.batch(M.MANY, cap=1 << 12)[0]]
    assert len(order) == 19 and order.index(22) == 0 and order.index(11) == 12


def test_model_at_the_measured_sizes():
    """what the issue that introduced the host schedule states about the benchmark's commit, on the model (the program equals the model above)"""
    (a,) = M.batch(M.bench_mix(1 << 20))
    assert [s["polys"] for s in a] == [10, 18, 18, 18, 64]
    assert [s["shape"] for s in a] == [M.WIDE, M.WIDE, M.NARROW, M.NARROW, M.NARROW]
    assert [s["L0"] for s in a] == [40, 127, 127, 127, 127] and all(s["fold_levels"] == 1 for s in a)
    (b,) = M.batch(M.bench_mix(1 << 22))
    assert [(s["polys"], s["refs"]) for s in b] == [(64, 128 << 22)] + [(16, 1 << 30)] * 4
    assert [s["fold_levels"] for s in b] == [1, 2, 2, 2, 2]  # the small kinds of the first set place at most 3 x 2^22 digits per column
    (c,), = M.batch([("FR", 1 << 24)])
    assert c["fold_levels"] == 3 and c["shape"] == M.WIDE and not c["pipelined"]
    (d,), = M.batch([("FR", 1 << 20)], table=False)
    assert (d["G"], d["L0"], d["nb"]) == (16, 64, 16 << 15)
    first, second = M.batch([("FR", 64)] * 200 + [("U8", 64)] * 57)
    assert sum(s["polys"] for s in first) == 256 and [(s["polys"], s["shape"], s["first"]) for s in second] == [(1, M.WIDE, 256)]
    assert [sum(s["polys"] for s in blk) for blk in M.batch([("FR", 64)] * 17, table=False)] == [16, 1]
    assert all(s["shape"] == M.WIDE for s in M.batch(M.MANY, cap=1 << 12, serial=True)[0])
    empty = M.batch(MIXED_EMPTY)[0][0]
    assert empty["kinds"] == [("FR", 1, 1), ("U16", 1, 1), ("U32", 1, 1), ("I64", 1, 1)] and empty["elig"] == 0b100100
    assert M.batch(ALL_EMPTY)[0][0]["refs"] == 0
