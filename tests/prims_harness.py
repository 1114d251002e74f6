"""ctypes front end of the primitive test harness tests/native/prims.hip (built into tests/native/libcozk_prims.so by
co-zkvms_amd/build.py's build_prims): limb packing, the op tables the library exports (the fields, G1, the 9 x 29 layers, the wide
accumulator), the edge operands and big-int expectations that tests/test_gpu_prims.py and tests/test_host_prims.py share, and the SHA-256 / transcript leg that test_host_prims.py runs in
fresh processes (`python prims_harness.py sha`)."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as O  # noqa: E402

LIB_PATH = os.path.join(HERE, "native", "libcozk_prims.so")
MONT = 1 << 256
FIELDS = {"fr": (0, O.R), "fq": (1, O.P)}
_lib = None


def build():
    """build_prims() in a child process under a time limit: a no-op when the library is newer than its sources, loud on failure"""
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "co-zkvms_amd", "build.py"), "--prims"],
                   check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        for name in ("prims_ff_ops", "prims_g1_ops", "prims_f9_ops", "prims_wide_ops"):
            getattr(L, name).restype = ctypes.c_char_p
        L.prims_ff.argtypes = [i, i, vp, vp, vp, vp, vp, vp, sz]
        L.prims_ff_host.argtypes = [i, i, vp, vp, vp, vp, vp, sz]
        L.prims_g1.argtypes = [i, vp, vp, vp, vp, sz]
        L.prims_f9.argtypes = [i, vp, vp, vp, vp, vp, vp, i, sz]
        L.prims_madd9_chain.argtypes = [vp, i, vp, sz]
        L.prims_wide.argtypes = [i, vp, vp, vp, sz]
        L.prims_sha256.argtypes = [vp, vp, sz, vp]
        L.prims_sha256.restype = None
        L.prims_transcript.argtypes = [vp, sz, vp, sz]
        L.prims_verify_sumcheck_rounds.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp]
        L.prims_eq_eval.argtypes = [vp, vp, sz, i, vp]
        L.prims_eq_eval.restype = None
        L.prims_mle_claim_padded.argtypes = [vp, sz, vp, vp, sz]
        _lib = L
    return _lib


def ops(kind):
    names = getattr(lib(), "prims_%s_ops" % kind)().decode().rstrip(",").split(",")
    return {n: k for k, n in enumerate(names)}


def to_limbs(xs, nlimbs=8):
    """ints < 2^(32 nlimbs) -> uint32[n, nlimbs]"""
    b = b"".join(int(x).to_bytes(4 * nlimbs, "little") for x in xs)
    return np.frombuffer(b, dtype="<u4").reshape(len(xs), nlimbs).copy()


def from_limbs(a):
    a = np.ascontiguousarray(a, dtype="<u4")
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def _ptr(a):
    return a.ctypes.data


def check(name, got, want, *operands):
    """lane-by-lane equality, reporting the first lane that differs with its operands"""
    assert len(got) == len(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            fmt = lambda v: hex(v) if isinstance(v, int) else str(v)
            raise AssertionError("%s, lane %d: got %s, want %s; operands %s"
                                 % (name, i, fmt(g), fmt(w), [fmt(o[i]) for o in operands]))


# ------------------------------------------------------------------------------------------------ 8 x 32 fields
def ff(field, op, a, b=None, c=None, d=None, host=False):
    """op over len(a) lanes of raw limb values (Montgomery form where it applies), on the device or through the host path of
    the headers -> (o1, o2) lists of ints"""
    n = len(a)
    z = [0] * n
    A, B, C, D = (to_limbs(v if v is not None else z) for v in (a, b, c, d))
    out = np.zeros((n, 16), dtype=np.uint32)
    code = ops("ff")[op]
    if host:
        assert lib().prims_ff_host(field, code, _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(out), n) == 0, "no host " + op
    else:
        ok = np.zeros(n, dtype=np.uint32)
        rc = lib().prims_ff(field, code, _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(out), _ptr(ok), n)
        assert rc == 0, "HIP error %d" % rc
        assert ok.all(), "no device " + op
    return from_limbs(out[:, :8]), from_limbs(out[:, 8:])


def edges(m):
    """the canonical edge operands of a modulus m (about 1.51 x 2^253)"""
    low7 = (1 << 224) - 1  # the seven low 32-bit limbs all ones
    e = [0, 1, 2, m - 1, m - 2, (m + 1) // 2, MONT % m, MONT * MONT % m, (1 << 253) - (1 << 64), (1 << 253) - 1, 1 << 253,
         (1 << 253) + 1, low7, (1 << 224) | low7, (((m >> 224) - 1) << 224) | low7, O.TWO_INV]
    assert all(0 <= x < m for x in e)
    return e


def lazy_edges(m):
    """the edges plus those of the lazy range [0, 2m)"""
    return edges(m) + [m, m + 1, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, 2 * m - 2, 2 * m - 1]


def operands(vals, bound, nrand, seed):
    """(a, b, c, d) lanes: every pair of vals at the start and again (roles swapped) at the end, nrand random lanes < bound
    between them"""
    rnd = random.Random(seed)
    k = len(vals)
    pa = [x for x in vals for _ in vals]
    pb = [y for _ in vals for y in vals]
    pc = [vals[(7 * i + 3) % k] for i in range(k * k)]
    pd = [vals[(5 * i + 1) % k] for i in range(k * k)]
    r = [[rnd.randrange(bound) for _ in range(nrand)] for _ in range(4)]
    return pa + r[0] + pb, pb + r[1] + pa, pc + r[2] + pd, pd + r[3] + pc


def expect(op, m, a, b, c, d):
    """the big-int value of op on Montgomery-form operands (any integers: the lazy ops are checked against these mod m)"""
    ri = pow(MONT, -1, m)
    one = lambda f: [f(x) for x in a]
    two = lambda f: [f(x, y) for x, y in zip(a, b)]
    four = lambda f: [f(x, y, u, v) for x, y, u, v in zip(a, b, c, d)]
    if op == "mul2":
        return two(lambda x, y: x * y * ri % m), [u * v * ri % m for u, v in zip(c, d)]
    table = {
        "add": lambda: two(lambda x, y: (x + y) % m),
        "sub": lambda: two(lambda x, y: (x - y) % m),
        "neg": lambda: one(lambda x: -x % m),
        "dbl": lambda: one(lambda x: 2 * x % m),
        "mul": lambda: two(lambda x, y: x * y * ri % m),
        "sqr": lambda: one(lambda x: x * x * ri % m),
        "mul_add2": lambda: four(lambda x, y, u, v: (x * y + u * v) * ri % m),
        "mul_sub2": lambda: four(lambda x, y, u, v: (x * y - u * v) * ri % m),
        "to_mont": lambda: one(lambda x: x * MONT % m),
        "from_mont": lambda: one(lambda x: x * ri % m),
        "from_u64": lambda: one(lambda x: (x & 0xFFFFFFFFFFFFFFFF) * MONT % m),
        "pow": lambda: two(lambda x, e: pow(x * ri % m, e, m) * MONT % m),
        "inv": lambda: one(lambda x: pow(x * ri % m, -1, m) * MONT % m if x % m else 0),
        "lcanon": lambda: one(lambda x: x % m),
    }
    return table[op](), [0] * len(a)


# the lazy operations: (the operation whose value they have mod m, the stated bound on the output in hundredths of m)
LAZY = {"mul_nr": ("mul", 176), "mul_add2_nr": ("mul_add2", 252), "lmul": ("mul", 200), "lmul2": ("mul2", 200),
        "ladd": ("add", 200), "lsub": ("sub", 200), "ldbl": ("dbl", 200), "lneg": ("neg", 200),
        "lmul_sub2": ("mul_sub2", 200), "lcanon": ("lcanon", 100)}


# ------------------------------------------------------------------------------------------------ G1
def g1(op, p, q):
    """p, q: lanes of 4-tuples (x, y, zz, zzz limb values; an affine operand is (x, y, 0, 0)) -> lanes of 4-tuples"""
    n = len(p)
    Pa = to_limbs([v for t in p for v in t]).reshape(n, 32)
    Qa = to_limbs([v for t in q for v in t]).reshape(n, 32)
    out = np.zeros((n, 32), dtype=np.uint32)
    ok = np.zeros(n, dtype=np.uint32)
    rc = lib().prims_g1(ops("g1")[op], _ptr(Pa), _ptr(Qa), _ptr(out), _ptr(ok), n)
    assert rc == 0, "HIP error %d" % rc
    assert ok.all(), "no device " + op
    v = from_limbs(out.reshape(4 * n, 8))
    return [tuple(v[4 * i:4 * i + 4]) for i in range(n)]


# ------------------------------------------------------------------------------------------------ 9 x 29
def f9(op, a, b=None, c=None, d=None, terms=0):
    """a..d: lanes of 9-limb lists -> (r, r2) lanes of 9-limb lists"""
    n = len(a)
    z = [[0] * 9] * n
    A, B, C, D = (np.array(v if v is not None else z, dtype=np.uint32).reshape(n, 9) for v in (a, b, c, d))
    out = np.zeros((n, 18), dtype=np.uint32)
    ok = np.zeros(n, dtype=np.uint32)
    rc = lib().prims_f9(ops("f9")[op], _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(out), _ptr(ok), terms, n)
    assert rc == 0, "HIP error %d" % rc
    assert ok.all(), "no device " + op
    return out[:, :9].tolist(), out[:, 9:].tolist()


def fe9(x):
    """an 8 x 32 value in the 9-limb record of the 9 x 29 wrappers"""
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(8)] + [0]


def fe9_value(l):
    return sum(v << (32 * k) for k, v in enumerate(l[:8]))


def madd9_chain(chains):
    """chains: lanes of k points (qx limbs, qy limbs) -> lanes of (accumulator [X, Y, ZZ, ZZZ] limbs, xyzz9_to_xyzz values,
    index of the first addition madd9 refused or k)"""
    n, k = len(chains), len(chains[0])
    pts = np.array([[v for qx, qy in ch for v in list(qx) + list(qy)] for ch in chains], dtype=np.uint32)
    out = np.zeros((n, 69), dtype=np.uint32)
    rc = lib().prims_madd9_chain(_ptr(pts), k, _ptr(out), n)
    assert rc == 0, "HIP error %d" % rc
    return [([row[9 * j:9 * j + 9].tolist() for j in range(4)], from_limbs(row[36:68].reshape(4, 8)), int(row[68]))
            for row in out]


# ------------------------------------------------------------------------------------------------ FrWide
def wide(op, columns, a=None, b=None):
    """columns: lanes of 15 integers below 2^96 (the accumulator state); a, b: lanes of raw limb values.  "wide_reduce" ->
    fr_wide_reduce of the state; "wide_mac" -> of the state after one fr_wide_mac(a, b)"""
    n = len(columns)
    z = [0] * n
    rows = np.zeros((n, 61), dtype=np.uint32)
    for k in range(15):
        rows[:, 3 * k:3 * k + 3] = to_limbs([c[k] for c in columns], 3)
    rows[:, 45:53] = to_limbs(a if a is not None else z)
    rows[:, 53:61] = to_limbs(b if b is not None else z)
    out = np.zeros((n, 8), dtype=np.uint32)
    ok = np.zeros(n, dtype=np.uint32)
    rc = lib().prims_wide(ops("wide")[op], _ptr(rows), _ptr(out), _ptr(ok), n)
    assert rc == 0, "HIP error %d" % rc
    assert ok.all(), "no device " + op
    return from_limbs(out)


# ------------------------------------------------------------------------------------------------ SHA-256 and the transcript
def _mont_bytes(x, m):
    return (x * MONT % m).to_bytes(32, "little")


def sha_leg():
    """every message length 0..260, 1000 and 4097 fed to Sha256::update in random chunks against hashlib, then random
    absorb / challenge sequences of Transcript against pyref.Transcript; reports what this process's Sha256 ran on"""
    import hashlib
    L = lib()
    rnd = random.Random(256)
    nmsg = 0
    for n in list(range(261)) + [1000, 4097]:
        msg = bytes(rnd.getrandbits(8) for _ in range(n))
        chunks, left = [], n
        while left:
            k = min(left, rnd.choice((0, 1, 7, 55, 56, 63, 64, 65, 119, 128, rnd.randrange(1, 300))))
            chunks.append(k)
            left -= k
        ch = (ctypes.c_size_t * max(1, len(chunks)))(*chunks)
        buf = ctypes.create_string_buffer(msg, max(1, n))
        out = (ctypes.c_uint8 * 32)()
        L.prims_sha256(buf, ch, len(chunks), out)
        assert bytes(out) == hashlib.sha256(msg).digest(), "SHA-256 of %d bytes fed in chunks %s" % (n, chunks)
        nmsg += 1
    pts = [None, O.G1_GEN, O.g1_neg(O.G1_GEN), O.g1_mul(O.G1_GEN, 1234567)]
    frs = [0, 1, O.R - 1, O.TWO_INV]
    nch = 0
    for _ in range(24):
        t = O.Transcript()
        script, want = bytearray(), []
        for _ in range(rnd.randrange(1, 40)):
            kind = rnd.choice("SVPC")
            if kind == "S":
                x = rnd.choice(frs + [rnd.randrange(O.R)])
                t.append_scalar(x)
                script += b"S" + _mont_bytes(x, O.R)
            elif kind == "V":
                xs = [rnd.choice(frs + [rnd.randrange(O.R)]) for _ in range(rnd.randrange(0, 6))]
                t.append_scalars(xs)
                script += b"V" + len(xs).to_bytes(4, "little") + b"".join(_mont_bytes(x, O.R) for x in xs)
            elif kind == "P":
                pt = rnd.choice(pts)
                t.append_point(pt)
                script += b"P" + (b"\x01" + bytes(64) if pt is None else
                                  b"\x00" + _mont_bytes(pt[0], O.P) + _mont_bytes(pt[1], O.P))
            else:
                want.append(t.challenge_scalar())
                script += b"C"
        out = (ctypes.c_uint32 * (8 * max(1, len(want))))()
        buf = ctypes.create_string_buffer(bytes(script), len(script))
        assert L.prims_transcript(buf, len(script), out, len(want)) == len(want)
        raw = bytes(out)
        got = [O.from_mont(int.from_bytes(raw[32 * i:32 * i + 32], "little"), O.R) for i in range(len(want))]
        assert got == want, "transcript challenges differ from pyref.Transcript"
        nch += len(want)
    return {"shani": L.prims_sha_uses_shani(), "messages": nmsg, "challenges": nch}


# ------------------------------------------------------------------------------------------------ host protocol helpers
def _fr_mont(xs):
    """canonical Fr values -> uint32[max(1, n), 8] Montgomery limbs"""
    return to_limbs([x * MONT % O.R for x in xs] or [0])


def _fr_canon(a):
    ri = pow(MONT, -1, O.R)
    return [v * ri % O.R for v in from_limbs(a)]


def verify_sumcheck_rounds(polys, rounds, degree, claim):
    """wire.hpp's verify_sumcheck_rounds on a fresh transcript -> (accepted, challenges, final claim, next challenge)"""
    flat = _fr_mont([c for p in polys for c in p])
    lens = np.array([len(p) for p in polys] or [0], dtype=np.uint64)
    cl = _fr_mont([claim])
    rs = np.zeros((max(1, len(polys)), 8), dtype=np.uint32)
    nxt = np.zeros((1, 8), dtype=np.uint32)
    ok = lib().prims_verify_sumcheck_rounds(_ptr(flat), _ptr(lens), len(polys), rounds, degree, _ptr(cl), _ptr(rs), _ptr(nxt))
    return bool(ok), _fr_canon(rs), _fr_canon(cl)[0], _fr_canon(nxt)[0]


def eq_eval(a, b, rev=False):
    out = np.zeros((1, 8), dtype=np.uint32)
    A, B = _fr_mont(a), _fr_mont(b)
    lib().prims_eq_eval(_ptr(A), _ptr(B), len(a), 1 if rev else 0, _ptr(out))
    return _fr_canon(out)[0]


def mle_claim_padded(outputs):
    """wire.hpp's mle_claim_padded on a fresh transcript -> (claim, point)"""
    V = _fr_mont(outputs)
    cl = np.zeros((1, 8), dtype=np.uint32)
    r = np.zeros((64, 8), dtype=np.uint32)
    n = lib().prims_mle_claim_padded(_ptr(V), len(outputs), _ptr(cl), _ptr(r), 64)
    assert n >= 0
    return _fr_canon(cl)[0], _fr_canon(r[:n]) if n else []


if __name__ == "__main__":
    if sys.argv[1:] == ["sha"]:
        print(json.dumps(sha_leg()))
