"""CPU test of the host tail of the dense layer rounds (co-zkvms_amd/csrc/host/layer_tail.hpp): the stand-alone host program
tests/native/layer_tail_check (built by co-zkvms_amd/build.py, no GPU and no project library) runs the tail on the cases below and
returns every round's three sums, the final claims and the eq tables it ends with; all of it is compared with oracle/pyref.py
(interleaved_compute_cubic_evals, interleaved_bind, SplitEq).  The step functions it runs are the ones the kernels run."""
import os
import struct
import subprocess
import sys

import pytest

import pyref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "layer_tail_check")
MONT = 1 << 256
LENGTHS = [4, 6, 10, 96, 100, 128, 130, 250, 256]  # ragged ones included: 6, 10, 100, 130, 250 bind through zero-padded chunks


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "co-zkvms_amd", "build.py"), "--layer-tail"], check=True)
    return EXE


def _fe(x):
    return (x * MONT % O.R).to_bytes(32, "little")


def _ints(raw):
    ri = pow(MONT, -1, O.R)
    return [int.from_bytes(raw[k:k + 32], "little") * ri % O.R for k in range(0, len(raw), 32)]


def _case(length, mode, start, seed):
    """-> (bytes of the case, expected sums per round, expected final claims, expected final E1, E2).
    start: "fresh" the tail takes the layer before its first round (split-eq nested, E1 collapses during the tail);
    "pending" after one round, its challenge still to be bound (what a per-round launch hands over);
    "e1_bound" after as many rounds as it takes to collapse E1, nothing pending (not nested from the first host round on)"""
    rng = O.SplitMix64(seed)
    rep3 = mode == "rep3"
    ref = [(rng.field(), rng.field()) if rep3 else rng.field() for _ in range(length)]
    nv = max(0, ((length + 1) // 2 - 1).bit_length())
    eq = O.SplitEq([rng.field() for _ in range(nv)])
    rs = [rng.field() for _ in range(nv)]
    done, pending = 0, None
    if start == "pending" and nv:
        done, pending = 1, rs[0]
    elif start == "e1_bound":
        while eq.E1_len > 1:
            ref = O.interleaved_bind(ref, rs[done])
            eq.bind(rs[done])
            done += 1
    a = [c[0] for c in ref] if rep3 else ref
    blob = struct.pack("<6Q", 2 if rep3 else 1, len(ref), eq.E1_len, eq.E2_len, 1 if pending is not None else 0, nv - done)
    blob += b"".join(_fe(x) for x in a)
    if rep3:
        blob += b"".join(_fe(c[1]) for c in ref)
    blob += b"".join(_fe(x) for x in eq.E1[:eq.E1_len]) + b"".join(_fe(x) for x in eq.E2[:eq.E2_len])
    if pending is not None:
        blob += _fe(pending)
    blob += b"".join(_fe(r) for r in rs[done:])
    sums = []
    r = pending
    for j in range(done, nv):
        if r is not None:
            ref = O.interleaved_bind(ref, r)
            eq.bind(r)
        ev = O.interleaved_compute_cubic_evals(ref, eq, 0)
        sums.append([ev[0], ev[2], ev[3]])
        r = rs[j]
    if r is not None:
        ref = O.interleaved_bind(ref, r)
        eq.bind(r)
    assert len(ref) == 2
    fin = [ref[0][0], ref[0][1], ref[1][0], ref[1][1]] if rep3 else [ref[0], 0, ref[1], 0]
    return blob, sums, fin, eq.E1[:eq.E1_len], eq.E2[:eq.E2_len]


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_host_tail_matches_oracle(exe, mode):
    cases = [_case(n, mode, start, 1000 * n + 7 * k + (mode == "rep3"))
             for n in LENGTHS for k, start in enumerate(("fresh", "pending", "e1_bound"))]
    out = subprocess.run([exe], input=struct.pack("<Q", len(cases)) + b"".join(c[0] for c in cases), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    raw, pos = out.stdout, 0
    collapsed = 0
    for (blob, sums, fin, e1, e2), (n, start) in zip(cases, [(n, s) for n in LENGTHS for s in ("fresh", "pending", "e1_bound")]):
        what = "length %d, %s, %s" % (n, mode, start)
        for j, want in enumerate(sums):
            assert _ints(raw[pos:pos + 96]) == want, "%s: sums of host round %d" % (what, j)
            pos += 96
        assert _ints(raw[pos:pos + 128]) == fin, what + ": final claims"
        pos += 128
        ln, e1_len, e2_len, binds = struct.unpack("<4Q", raw[pos:pos + 32])
        pos += 32
        header = struct.unpack("<6Q", blob[:48])
        assert (ln, e1_len, e2_len) == (2, len(e1), len(e2)), what + ": lengths after the tail"
        assert binds == header[5] + header[4], what + ": one bind per round and one for a pending challenge"
        assert _ints(raw[pos:pos + 32 * e1_len]) == e1 and _ints(raw[pos + 32 * e1_len:pos + 32 * (e1_len + e2_len)]) == e2, what + ": eq tables"
        pos += 32 * (e1_len + e2_len)
        collapsed += header[2] > 1 and e1_len == 1
    assert pos == len(raw)
    assert collapsed >= 2 * len(LENGTHS)  # the fresh and the pending starts collapse E1 inside the tail
