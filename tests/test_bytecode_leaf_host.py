"""CPU test of the word arithmetic of the bytecode leaf kernels (co-zkvms_amd/csrc/bytecode_arith.hip.hpp): the stand-alone host
program tests/native/bytecode_leaf_check (built by co-zkvms_amd/build.py, no GPU and no project library) runs bc_read_public and
bc_init_final, the functions the kernels call per entry, on the cases below; every word is compared with the big-int leaves of
tests/bytecode_ref.py.  Cases: every entry at 2^64 - 1, all zero, random entries of mixed widths, an I64 imm at its extremes and the
same bits as U64, the row number at 2^32 - 1, with gamma and tau in {0, 1, r - 1} and random."""
import os
import random
import struct
import subprocess
import sys

import pytest

import bytecode_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "bytecode_leaf_check")
R = B.R
M64 = (1 << 64) - 1
WIDTHS = {0: 32, 1: 64}


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "co-zkvms_amd", "build.py"), "--bytecode-leaf-check"], check=True)
    return EXE


def _words(x):
    return [(x >> (64 * i)) & M64 for i in range(4)]


def _cases():
    rng = random.Random(910)
    edge = [0, 1, R - 1]
    out = []
    for g in edge + [rng.randrange(R) for _ in range(6)]:
        for tau in edge + [rng.randrange(R)]:
            shapes = [([M64] * 7, 0x7F, 0, (1 << 32) - 1), ([0] * 7, 0x7F, 0, 0), ([(1 << 32) - 1] * 7, 0, 0, 5)]
            mask = rng.randrange(128)
            shapes.append(([rng.randrange(1 << WIDTHS[(mask >> k) & 1]) for k in range(7)], mask, 0, rng.randrange(1 << 32)))
            for imm in (B.I64_MIN, B.I64_MAX, -1, 0, -rng.randrange(1 << 63), rng.randrange(1 << 63)):
                e = [rng.randrange(1 << 64) for _ in range(7)]
                e[5] = imm & M64
                shapes.append((e, 0x5F, 1, rng.randrange(1 << 32)))  # the imm's own bit clear: imm_signed makes it wide
                shapes.append((e, 0x7F, 0, rng.randrange(1 << 32)))  # the same bits as a U64 column: another value
            out += [(g, tau, e, m, s, i) for e, m, s, i in shapes]
    return out


def test_host_words_equal_the_big_int_leaves(exe):
    cases = _cases()
    blob = struct.pack("<Q", len(cases))
    for g, tau, e, mask, signed, row in cases:
        blob += struct.pack("<19Q", *(_words(B.mont(g)) + _words(B.mont(tau)) + [row] + e + [mask, signed, 0]))
    out = subprocess.run([exe], input=blob, capture_output=True, timeout=120)
    assert out.returncode == 0 and len(out.stdout) == 96 * len(cases), out.stderr
    word = lambda c, k: int.from_bytes(out.stdout[96 * c + 32 * k:96 * c + 32 * k + 32], "little")
    for c, (g, tau, e, mask, signed, row) in enumerate(cases):
        p = B._powers(g)
        what = "case %d: g %x tau %x entries %s mask %x signed %d row %d" % (c, g, tau, e, mask, signed, row)
        seen = [e[k] if (mask >> k) & 1 else e[k] & B.M32 for k in range(7)]  # a column without a high half is read as 32 bits
        assert word(c, 0) == B.mont(sum(seen[k] * p[1 + k] for k in range(7)) - tau), what + ": read"
        imm = e[5] - (1 << 64) if signed and e[5] >> 63 else e[5]
        init = row * p[1] + sum(e[k] * p[2 + k] for k in range(5)) + imm - tau
        assert word(c, 1) == B.mont(init), what + ": init"
        assert word(c, 2) == B.mont(init + e[6] * p[7]), what + ": final"
