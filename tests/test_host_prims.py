"""Host arithmetic at edge operands, no GPU, against big-int (oracle/pyref.py): the two host Montgomery products (mul_host on
4 x 64 limbs, mul_host32 on 8 x 32) and the other host field operations through the test harness (tests/native/prims.hip),
SHA-256 on both block paths and the transcript (one fresh process per path: the choice is a per-process static), and libcozk's
host G1 helpers cozk_g1_mul / cozk_g1_sum."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import prims_harness as H
import pyref as O

HOST_OPS = ["add", "sub", "neg", "dbl", "mul", "sqr", "mul2", "mul_add2", "mul_sub2", "to_mont", "from_mont", "from_u64", "pow",
            "inv"]


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_host_products_agree_with_bigint(field):
    """mul_host == mul_host32 == big-int on every pair of edge operands and 10^5 random pairs"""
    f, m = H.FIELDS[field]
    a, b, _, _ = H.operands(H.edges(m), m, 100000, 17 + f)
    want = H.expect("mul", m, a, b, a, b)[0]
    for op in ("mul_host", "mul_host32"):
        H.check("%s host %s" % (field, op), H.ff(f, op, a, b, host=True)[0], want, a, b)


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_host_field_ops_are_exact(field):
    f, m = H.FIELDS[field]
    a, b, c, d = H.operands(H.edges(m), m, 2000, 23 + f)
    for op in HOST_OPS:
        got, want = H.ff(f, op, a, b, c, d, host=True), H.expect(op, m, a, b, c, d)
        for k in range(2):
            H.check("%s host %s (output %d)" % (field, op, k + 1), got[k], want[k], a, b, c, d)


def _sha_leg(no_shani):
    env = dict(os.environ)
    env.pop("COZK_NO_SHANI", None)
    if no_shani:
        env["COZK_NO_SHANI"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [H.__file__, "sha"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_sha256_and_transcript_portable_block():
    res = _sha_leg(no_shani=True)
    assert res["shani"] == 0, "COZK_NO_SHANI=1 did not select the portable block code"
    print("portable SHA-256 block code: %(messages)d messages, %(challenges)d transcript challenges" % res)


def test_sha256_and_transcript_shani_block():
    res = _sha_leg(no_shani=False)
    if not res["shani"]:
        pytest.skip("this CPU has no SHA extensions: Sha256 runs the portable block code here (checked by the portable leg)")
    print("SHA-NI block code: %(messages)d messages, %(challenges)d transcript challenges" % res)


# ------------------------------------------------------------------------------------------------ host G1 helpers
def _g1_mul(cozk, pt, s):
    xy, inf = cozk.point_to_abi(pt)
    sm = cozk.fr_to_mont_limbs([s])[0]
    out = np.zeros(8, dtype=np.uint64)
    oi = ctypes.c_int()
    assert cozk._lib.lib().cozk_g1_mul(None, xy.ctypes.data, inf, sm.ctypes.data, out.ctypes.data, ctypes.byref(oi)) == 0
    return cozk.point_from_abi(out, oi.value)


def _g1_sum(cozk, pts):
    k = len(pts)
    xy = np.zeros((k, 8), dtype=np.uint64)
    inf = np.zeros(k, dtype=np.int32)
    for i, p in enumerate(pts):
        xy[i], inf[i] = cozk.point_to_abi(p)
    out = np.zeros(8, dtype=np.uint64)
    oi = ctypes.c_int()
    assert cozk._lib.lib().cozk_g1_sum(None, xy.ctypes.data, inf.ctypes.data, k, out.ctypes.data, ctypes.byref(oi)) == 0
    return cozk.point_from_abi(out, oi.value)


def test_host_g1_mul(cozk):
    """cozk_g1_mul (null context: it has none) at edge scalars times G, -G, the identity and a random point"""
    rnd = random.Random(31)
    r = O.R
    scalars = [0, 1, 2, r - 1, r - 2, (r + 1) // 2, 1 << 128, rnd.randrange(r)]
    for pt in (O.G1_GEN, O.g1_neg(O.G1_GEN), None, O.g1_mul(O.G1_GEN, rnd.randrange(1, r))):
        for s in scalars:
            assert _g1_mul(cozk, pt, s) == O.g1_mul(pt, s), (pt, s)


def test_host_g1_sum(cozk):
    """cozk_g1_sum on doublings, cancellations, the identity and 100 random points"""
    rnd = random.Random(32)
    p = O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R))
    cases = [[p, p], [p, O.g1_neg(p)], [None, p], [p, None], [p, p, O.g1_neg(p)],
             [O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R)) for _ in range(100)]]
    for pts in cases:
        want = None
        for q in pts:
            want = O.g1_add(want, q)
        assert _g1_sum(cozk, pts) == want, pts[:4]
