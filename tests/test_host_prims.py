"""Host arithmetic at edge operands, no GPU, against big-int (oracle/pyref.py): the two host Montgomery products (mul_host on
4 x 64 limbs, mul_host32 on 8 x 32) and the other host field operations through the test harness (tests/native/prims.hip),
SHA-256 on both block paths and the transcript (one fresh process per path: the choice is a per-process static), libcozk's
host G1 helpers cozk_g1_mul / cozk_g1_sum, and the host protocol helpers of wire.hpp (verify_sumcheck_rounds, eq_eval, eq_eval_rev,
mle_claim_padded) against pyref's transcript and polynomials."""
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


# ------------------------------------------------------------------------------------------------ host protocol helpers (wire.hpp)
FR_EDGES = [0, 1, O.R - 1]


def _sumcheck_script(rnd, degree, rounds):
    """an honest sumcheck of `rounds` rounds of degree-`degree` polys with seeded and edge operands, replayed on pyref.Transcript:
    -> (starting claim, compressed polys, challenges, final claim, the next challenge of the transcript)"""
    pick = lambda: rnd.choice(FR_EDGES) if rnd.random() < 0.4 else rnd.randrange(O.R)
    t = O.Transcript()
    claim0 = claim = pick()
    polys, rs = [], []
    for _ in range(rounds):
        g0 = pick()
        evals = [g0, (claim - g0) % O.R] + [pick() for _ in range(degree - 1)]  # g(0) + g(1) = claim
        poly = O.unipoly_from_evals(evals)
        comp = O.unipoly_compress(poly)
        assert len(comp) == degree
        t.append_scalars(comp)
        r = t.challenge_scalar()
        polys.append(comp)
        rs.append(r)
        claim = O.unipoly_eval(poly, r)
    return claim0, polys, rs, claim, t.challenge_scalar()


@pytest.mark.parametrize("degree", [2, 3])
def test_verify_sumcheck_rounds_replays_like_pyref(degree):
    """same challenges, same final claim and same transcript state (one more challenge) as the Python replay, for 1..12 rounds"""
    rnd = random.Random(1000 + degree)
    for rounds in range(1, 13):
        for _ in range(4):
            claim0, polys, rs, claim, nxt = _sumcheck_script(rnd, degree, rounds)
            ok, got_rs, got_claim, got_next = H.verify_sumcheck_rounds(polys, rounds, degree, claim0)
            assert ok, (degree, rounds)
            assert got_rs == rs, (degree, rounds)
            assert got_claim == claim, (degree, rounds)
            assert got_next == nxt, (degree, rounds)


@pytest.mark.parametrize("degree", [2, 3])
def test_verify_sumcheck_rounds_rejects_wrong_shape(degree):
    rnd = random.Random(2000 + degree)
    for rounds in (1, 2, 5, 12):
        claim0, polys, _, _, _ = _sumcheck_script(rnd, degree, rounds)
        assert H.verify_sumcheck_rounds(polys, rounds, degree, claim0)[0]
        for wrong in (rounds - 1, rounds + 1):
            assert not H.verify_sumcheck_rounds(polys, wrong, degree, claim0)[0], "accepted %d polys as %d rounds" % (rounds, wrong)
        assert not H.verify_sumcheck_rounds(polys[:-1], rounds, degree, claim0)[0]
        assert not H.verify_sumcheck_rounds(polys + [polys[0]], rounds, degree, claim0)[0]
        for wrong in (degree - 1, degree + 1):
            assert not H.verify_sumcheck_rounds(polys, rounds, wrong, claim0)[0], "accepted degree %d polys as degree %d" % (degree, wrong)
        for k in sorted({0, rounds // 2, rounds - 1}):
            longer = [p + [rnd.randrange(O.R)] if i == k else p for i, p in enumerate(polys)]
            shorter = [p[:-1] if i == k else p for i, p in enumerate(polys)]
            assert not H.verify_sumcheck_rounds(longer, rounds, degree, claim0)[0], "accepted a poly of degree %d" % (degree + 1)
            assert not H.verify_sumcheck_rounds(shorter, rounds, degree, claim0)[0], "accepted a poly of degree %d" % (degree - 1)


def test_eq_eval_both_argument_orders():
    """eq_eval(a, b) = prod (1 - a_i - b_i + 2 a_i b_i) and eq_eval_rev(a, b) = eq_eval(a, reversed(b)) for lengths 0..20"""
    rnd = random.Random(3000)
    pick = lambda: rnd.choice(FR_EDGES) if rnd.random() < 0.3 else rnd.randrange(O.R)
    for n in range(21):
        for _ in range(3):
            a, b = [pick() for _ in range(n)], [pick() for _ in range(n)]
            want = want_rev = 1
            for i in range(n):
                want = want * (1 - a[i] - b[i] + 2 * a[i] * b[i]) % O.R
                want_rev = want_rev * (1 - a[i] - b[n - 1 - i] + 2 * a[i] * b[n - 1 - i]) % O.R
            assert H.eq_eval(a, b) == want, (n, a, b)
            assert H.eq_eval(a, b, rev=True) == want_rev, (n, a, b)
    bits = [rnd.randrange(2) for _ in range(20)]  # on the hypercube eq is the indicator of equality
    assert H.eq_eval(bits, bits) == 1 and H.eq_eval(bits, bits[::-1], rev=True) == 1
    assert H.eq_eval(bits, [1 - bits[0]] + bits[1:]) == 0


@pytest.mark.parametrize("count", [1, 2, 3, 5, 8, 54])
def test_mle_claim_padded(count):
    """claim = sum_i eq_evals(r)[i] * padded[i] at the point the transcript gives, outputs zero-padded to a power of two"""
    rnd = random.Random(4000 + count)
    outputs = [rnd.choice(FR_EDGES) if rnd.random() < 0.3 else rnd.randrange(O.R) for _ in range(count)]
    nv = (count - 1).bit_length()
    r = O.Transcript().challenge_vector(nv)
    padded = outputs + [0] * ((1 << nv) - count)
    eq = O.eq_evals(r)
    assert len(eq) == len(padded)
    want = sum(e * v for e, v in zip(eq, padded)) % O.R
    claim, point = H.mle_claim_padded(outputs)
    assert point == r
    assert claim == want
