"""The device arithmetic primitives one at a time, through the test harness tests/native/prims.hip (which includes the product
headers), against big-int (oracle/pyref.py) and the 9 x 29 CPU models (test_fr9_model / test_fq9_model):
  * the 8 x 32 Montgomery fields (ff.hip.hpp): canonical operations exact; lazy operations congruent and below their stated
    bounds; the lazy zero test true for exactly 0 and m;
  * the XYZZ G1 formulas (ec.hip.hpp) on edge points, lazy coordinates, P + P, P - P, the identity and chains;
  * the 9 x 29 Fr / Fq layers (fr9.hip.hpp, fq9.hip.hpp) limb for limb against the models, the folded accumulator chain and the
    madd9 chain;
  * the wide dot-product accumulator (poly.hip.hpp FrWide) at the term counts and column states of its stated bound.
Edge operands sit at the start and at the end of every launch.  The 8 x 32 launches put 2^16 random lanes between them, the
9 x 29 launches 2^12, because each of their lanes also runs through the Python model."""
import random

import pytest

import prims_harness as H
import pyref as O
import reduction_ref as W
import test_fq9_model as Q9
import test_fr9_model as R9

pytestmark = pytest.mark.gpu

P, R, MONT = O.P, O.R, H.MONT
NRAND = 1 << 16
NRAND9 = 1 << 12
CANONICAL = ["add", "sub", "neg", "dbl", "mul", "sqr", "mul2", "mul_add2", "mul_sub2", "to_mont", "from_mont", "from_u64",
             "pow", "inv"]


@pytest.fixture(scope="module", autouse=True)
def prims():
    return H.lib()


# ------------------------------------------------------------------------------------------------ 8 x 32 fields
@pytest.mark.parametrize("field", ["fr", "fq"])
def test_canonical_ops_are_exact(field):
    """exact, canonical results on every pair of edge operands and 2^16 random pairs; from_u64 of 2^64 - 1 (the low limbs of
    2^253 - 1) is the regression case of the early-clobber accumulators of ff_macc.inc"""
    f, m = H.FIELDS[field]
    a, b, c, d = H.operands(H.edges(m), m, NRAND, 1 + f)
    for op in CANONICAL:
        got, want = H.ff(f, op, a, b, c, d), H.expect(op, m, a, b, c, d)
        for k in range(2):
            H.check("%s %s (output %d)" % (field, op, k + 1), got[k], want[k], a, b, c, d)


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_lazy_ops_are_congruent_and_bounded(field):
    f, m = H.FIELDS[field]
    a, b, c, d = H.operands(H.lazy_edges(m), 2 * m, NRAND, 11 + f)
    for op, (ref, bound) in H.LAZY.items():
        got, want = H.ff(f, op, a, b, c, d), H.expect(ref, m, a, b, c, d)
        for k in range(2 if op == "lmul2" else 1):
            H.check("%s %s mod m (output %d)" % (field, op, k + 1), [g % m for g in got[k]], want[k], a, b, c, d)
            over = [i for i, g in enumerate(got[k]) if 100 * g >= bound * m]
            assert not over, "%s %s, lane %d: %#x is not below %d/100 m" % (field, op, over[0], got[k][over[0]], bound)
    H.check(field + " lis_zero", H.ff(f, "lis_zero", a)[0], [int(x in (0, m)) for x in a], a)


# ------------------------------------------------------------------------------------------------ G1
RI = pow(MONT, -1, P)


def _mont(x):
    return x % P * MONT % P


def _sqrt(a):
    r = pow(a, (P + 1) // 4, P)  # p = 3 mod 4
    return r if r * r % P == a % P else None


def _cbrt(a):
    """a cube root mod p, or None: p - 1 = 3^s t, and a^(3^-1 mod t) is one up to an element of the (order 3^s) 3-Sylow subgroup"""
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    x = pow(a, pow(3, -1, t), P)
    g = next(g for g in range(2, 1000) if pow(g, (P - 1) // 3, P) != 1)
    h, z = pow(g, t, P), 1
    for _ in range(3 ** s):
        if pow(x * z, 3, P) == a % P:
            return x * z % P
        z = z * h % P
    raise AssertionError("no cube root of a cubic residue")


def _random_point(rnd):
    while True:
        x = rnd.randrange(P)
        y = _sqrt(x ** 3 + 3)
        if y is not None:
            return x, (y if rnd.random() < 0.5 else -y % P)


def _edge_points():
    """G, -G, 2G, and points whose x or y lies within 2^32 of 0 or p (the first ones a search finds)"""
    pts = [O.G1_GEN, O.g1_neg(O.G1_GEN), O.g1_mul(O.G1_GEN, 2)]
    for xs in (range(0, 200), range(P - 1, P - 200, -1)):
        found = [(x, y) for x, y in ((x, _sqrt(x ** 3 + 3)) for x in xs) if y is not None][:2]
        pts += [p for x, y in found for p in ((x, y), (x, -y % P))]
    for ys in (range(1, 200), range(P - 1, P - 200, -1)):
        pts += [(x, y) for x, y in ((_cbrt(y * y - 3), y) for y in ys) if x is not None][:2]
    assert len(pts) == 15 and all(O.g1_is_on_curve(p) for p in pts)
    return pts


def _xyzz(pt, z, lazy):
    """(x z^2, y z^3, z^2, z^3) in Montgomery form; the coordinates flagged in lazy get + p (still below 2p)"""
    if pt is None:
        return (0, 0, 0, 0)
    zz = z * z % P
    zzz = zz * z % P
    t = (_mont(pt[0] * zz), _mont(pt[1] * zzz), _mont(zz), _mont(zzz))
    return tuple(v + P if lazy >> k & 1 else v for k, v in enumerate(t))


def _aff(pt):
    return (0, 0, 0, 0) if pt is None else (_mont(pt[0]), _mont(pt[1]), 0, 0)


def _z(rnd):
    return 1 if rnd.random() < 0.25 else rnd.randrange(1, P)


def _check_xyzz(name, got, want):
    """XYZZ outputs (Montgomery, lazy range) against the affine points they must be; ZZ^3 = ZZZ^2 on every one"""
    assert len(got) == len(want)
    for i, (t, w) in enumerate(zip(got, want)):
        where = "%s, lane %d (want %s): got %s" % (name, i, w, [hex(v) for v in t])
        assert all(v < 2 * P for v in t), where + ": a coordinate is not below 2p"
        if w is None:
            assert t[2] == 0, where + ": not the identity"
            continue
        X, Y, ZZ, ZZZ = (v * RI % P for v in t)
        assert ZZ != 0 and pow(ZZ, 3, P) == pow(ZZZ, 2, P), where + ": ZZ^3 != ZZZ^2"
        assert (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P) == w, where


def test_g1_formulas_on_edge_points():
    """every pair of edge points (P + Q, P + P, P - P, the identity on either side) at both ends, random pairs between, each
    XYZZ operand with a random or unit z and random coordinates replaced by their lazy representative (+ p)"""
    rnd = random.Random(3)
    S = _edge_points() + [_random_point(rnd) for _ in range(6)] + [None]
    pool = [_random_point(rnd) for _ in range(64)]
    pairs = [(A, B) for A in S for B in S]
    pairs = pairs + [(rnd.choice(pool), rnd.choice(pool)) for _ in range(4096)] + pairs[::-1]
    pA = [_xyzz(A, _z(rnd), rnd.randrange(16)) for A, _ in pairs]
    pB = [_xyzz(B, _z(rnd), rnd.randrange(16)) for _, B in pairs]
    qA, qB = [_aff(A) for A, _ in pairs], [_aff(B) for _, B in pairs]
    sums = [O.g1_add(A, B) for A, B in pairs]
    dbls = [O.g1_add(A, A) for A, _ in pairs]
    _check_xyzz("add_mixed", H.g1("add_mixed", pA, qB), sums)
    _check_xyzz("add", H.g1("add", pA, pB), sums)
    _check_xyzz("dbl", H.g1("dbl", pA, pA), dbls)
    _check_xyzz("dbl_affine", H.g1("dbl_affine", qA, qA), dbls)
    _check_xyzz("neg (XYZZ)", H.g1("neg_xyzz", pA, pA), [O.g1_neg(A) for A, _ in pairs])
    H.check("to_affine", H.g1("to_affine", pA, pA), qA)
    H.check("neg (affine)", H.g1("neg_affine", qA, qA), [_aff(O.g1_neg(A)) for A, _ in pairs])
    H.check("on_curve", [t[0] for t in H.g1("on_curve", qA, qA)], [1] * len(qA))
    off = [(_mont(A[0]), _mont(A[1] + 1), 0, 0) for A in S if A is not None]
    H.check("on_curve (off the curve)", [t[0] for t in H.g1("on_curve", off, off)], [0] * len(off))


def test_g1_chains_of_mixed_additions_and_doublings():
    """each lane carries one lazy XYZZ accumulator through 30 steps -- mixed additions, doublings, full additions -- where some
    steps add the accumulator itself (a doubling inside the addition), its negation (the identity) or the identity"""
    rnd = random.Random(4)
    pool = [_random_point(rnd) for _ in range(64)]
    ref = [rnd.choice(pool) for _ in range(1024)]
    acc = [_xyzz(A, _z(rnd), rnd.randrange(16)) for A in ref]
    for step in range(30):
        kind = ("add_mixed", "dbl", "add")[step % 3]
        if kind == "dbl":
            acc, ref = H.g1("dbl", acc, acc), [O.g1_add(A, A) for A in ref]
        else:
            q = []
            for A in ref:
                u = rnd.random()
                q.append(A if u < 0.1 else O.g1_neg(A) if u < 0.2 else None if u < 0.25 else rnd.choice(pool))
            enc = [_aff(B) for B in q] if kind == "add_mixed" else [_xyzz(B, _z(rnd), rnd.randrange(16)) for B in q]
            acc, ref = H.g1(kind, acc, enc), [O.g1_add(A, B) for A, B in zip(ref, q)]
        _check_xyzz("%s, step %d" % (kind, step), acc, ref)


# ------------------------------------------------------------------------------------------------ 9 x 29 Fr
RPI_R = pow(R9.RP, -1, R)
RPI_P = pow(Q9.RP, -1, P)


def _rot(xs, k):
    return xs[k:] + xs[:k]


def _spread(l):
    """the same value with limbs 0..7 lifted into [2^29, 2^30) where the next limb can give 1"""
    l = list(l)
    for i in range(8):
        if l[i + 1] > 0:
            l[i] += 1 << 29
            l[i + 1] -= 1
    return l


def _values(name, got, want, mod):
    H.check(name + " (value)", [R9.val(g) % mod for g in got], want)


def test_fr9_matches_the_model_limb_for_limb():
    rnd = random.Random(9)
    X = R9.Exact
    fam = [R - 1, R9.MAXLIMB]  # the model's all-(r - 1) and max-limb operands, next to its random ones
    vals = H.edges(R) + fam + [rnd.randrange(R) for _ in range(NRAND9)] + fam[::-1]
    A, B, C, D = ([R9.limbs(v) for v in _rot(vals, k)] for k in range(4))
    # 8 x 32 <-> 9 x 29
    w = vals + H.edges(P) + [MONT - 1, 1 << 255] + [rnd.randrange(MONT) for _ in range(64)]
    H.check("f9_from_fe", H.f9("from_fe", [H.fe9(v) for v in w])[0], [R9.limbs(v) for v in w], w)
    H.check("f9_to_fe", [H.fe9_value(l) for l in H.f9("to_fe", [R9.limbs(v) for v in w])[0]], w, w)
    # first operands with every limb just below the documented bounds (2^30.6; 1.5 x 2^30 for the two-product form)
    amax, a2max = [R9.MUL_A_MAX - 1] * 9, [R9.MUL2_A_MAX - 1] * 9
    Am, Bm = [amax, a2max] + A + [a2max, amax], B[:2] + B + B[-2:]
    got = H.f9("fr9_mul", Am, Bm)[0]
    H.check("fr9_mul", got, [X.mul(a, b) for a, b in zip(Am, Bm)], Am, Bm)
    _values("fr9_mul", got, [R9.val(a) * R9.val(b) * RPI_R % R for a, b in zip(Am, Bm)], R)
    A2, C2, B2, D2 = [a2max] * 2 + A + [a2max] * 2, [a2max] * 2 + C + [a2max] * 2, B[:2] + B + B[-2:], D[:2] + D + D[-2:]
    got = H.f9("fr9_mul_add2", A2, B2, C2, D2)[0]
    H.check("fr9_mul_add2", got, [X.mul_add2(*t) for t in zip(A2, B2, C2, D2)], A2, B2, C2, D2)
    _values("fr9_mul_add2", got, [(R9.val(a) * R9.val(b) + R9.val(c) * R9.val(d)) * RPI_R % R
                                  for a, b, c, d in zip(A2, B2, C2, D2)], R)
    for k in ("rp", "k1", "k2", "k3"):  # fr9_mul_sc with the wave-uniform constants the kernels pass
        H.check("fr9_mul_sc " + k, H.f9("fr9_mul_sc_" + k, Am)[0], [X.mul(a, X.const("FR9_" + k.upper())) for a in Am], Am)
    # the fold at the accumulator bound (~138 r, top limb) with max limbs below it
    Af = [[R9.MASK] * 8 + [(138 * R) >> 232]] + Am
    H.check("fr9_fold", H.f9("fr9_fold", Af)[0], [R9.fold(X, a) for a in Af], Af)
    H.check("fr9_add", H.f9("fr9_add", A, B)[0], [X.add(a, b) for a, b in zip(A, B)], A, B)
    un = [X.add(X.add(a, b), c) for a, b, c in zip(A, B, C)] + [[(1 << 32) - 9] * 8 + [1000]]
    H.check("f9_norm", H.f9("norm", un)[0], [X.norm(a) for a in un], un)
    # a + C - b for subtrahends at each constant's stated bound: canonical; < 2.1 r, limbs < 2^30; < 4.3 r, limbs < 2^31
    for cname, k, spread in (("c2", 100, False), ("c3", 209, True), ("c5", 429, True)):
        Bs = [_spread(R9.limbs(v)) if spread else R9.limbs(v) for v in (v * k // 100 for v in _rot(vals, 5))]
        got = H.f9("fr9_sub_" + cname, A, Bs)[0]
        H.check("f9_sub FR9_" + cname.upper(), got, [X.sub(a, R9.C["FR9_" + cname.upper()], b) for a, b in zip(A, Bs)], A, Bs)
        _values("f9_sub FR9_" + cname.upper(), got, [(R9.val(a) - R9.val(b)) % R for a, b in zip(A, Bs)], R)
    # to canonical: values < 3 r, limbs normalised or lifted
    cv = [0, R - 1, R, 2 * R - 1, 2 * R, 3 * R - 1] + [rnd.randrange(3 * R) for _ in range(NRAND9)]
    Cv = [R9.limbs(v) for v in cv] + [_spread(R9.limbs(v)) for v in cv]
    H.check("fr9_to_canonical", [H.fe9_value(l) for l in H.f9("fr9_to_canonical", Cv)[0]], [X.canonical(a) for a in Cv], Cv)


def test_fr9_folded_accumulator_chain():
    """one chain per lane of 4 FR9_FOLD_PERIOD + 3 terms acc = norm(acc + a b), folded every period as the kernels fold: the
    model's limbs, and the big-int sum"""
    n = 4 * R9.FOLD + 3
    rnd = random.Random(12)
    pairs = [(R - 1, R - 1)] * 4 + [(R9.MAXLIMB, R9.MAXLIMB), (R - 1, R9.MAXLIMB)] + \
            [(rnd.randrange(R), rnd.randrange(R)) for _ in range(10)] + [(R - 1, R - 1)] * 2
    A, B = [R9.limbs(a) for a, _ in pairs], [R9.limbs(b) for _, b in pairs]
    got = H.f9("fr9_chain", A, B, terms=n)[0]
    X = R9.Exact
    want = []
    for a, b in zip(A, B):
        acc = X.zero()
        for it in range(n):
            if it and it % R9.FOLD == 0:
                acc = R9.fold(X, acc)
            acc = X.norm(X.add(acc, X.mul(a, b)))
        want.append(acc)
    H.check("fr9 chain", got, want, A, B)
    _values("fr9 chain", got, [n * a * b * RPI_R % R for a, b in pairs], R)


# ------------------------------------------------------------------------------------------------ 9 x 29 Fq
# the worst-case limb patterns of test_fq9_model.test_worst_case_limbs_do_not_overflow
FULL = [Q9.MASK] * 8 + [(6 * P) >> (29 * 8)]
U = [3 * (1 << 29) - 1] * 8 + [(9 * P) >> (29 * 8)]
NY = [(1 << 30) - 1] * 8 + [(3 * P) >> (29 * 8)]


def test_fq9_matches_the_model_limb_for_limb():
    """every product shape against the model, the worst-case limb patterns at both ends; (U, FULL) next to (FULL, FULL) in the
    interleaved forms is the regression case of their second product's top limb (it was the first product's)"""
    rnd = random.Random(10)
    vals = H.edges(P) + [6 * P - 1] + [rnd.randrange(6 * P) for _ in range(NRAND9)] + [P - 1, 6 * P - 1]
    A, B, C, D = ([Q9.limbs(v) for v in _rot(vals, k)] for k in range(4))
    Aw, Bw = [FULL, FULL, U] + A + [U, FULL, FULL], [FULL, U, FULL] + B + [FULL, U, FULL]
    Cw, Dw = [FULL, U, FULL] + C + [FULL, U, FULL], [FULL, FULL, FULL] + D + [FULL, FULL, FULL]
    got = H.f9("fq9_mul", Aw, Bw)[0]
    H.check("f9_mul", got, [Q9.mul(a, b) for a, b in zip(Aw, Bw)], Aw, Bw)
    _values("f9_mul", got, [Q9.val(a) * Q9.val(b) * RPI_P % P for a, b in zip(Aw, Bw)], P)
    got = H.f9("fq9_mul_x2", Aw, Bw, Cw, Dw)
    H.check("f9_mul_x2 (1)", got[0], [Q9.mul(a, b) for a, b in zip(Aw, Bw)], Aw, Bw)
    H.check("f9_mul_x2 (2)", got[1], [Q9.mul(c, d) for c, d in zip(Cw, Dw)], Cw, Dw)
    An, Cn = [FULL] + A + [FULL], [FULL] + C + [FULL]  # f9_sqr takes normalised operands
    got = H.f9("fq9_sqr", An)[0]
    H.check("f9_sqr", got, [Q9.sqr(a) for a in An], An)
    _values("f9_sqr", got, [Q9.val(a) ** 2 * RPI_P % P for a in An], P)
    got = H.f9("fq9_sqr_x2", An, None, Cn)
    H.check("f9_sqr_x2 (1)", got[0], [Q9.sqr(a) for a in An], An)
    H.check("f9_sqr_x2 (2)", got[1], [Q9.sqr(c) for c in Cn], Cn)
    # the fused Y3 product Rd T + NY PPP at its worst-case limbs
    Ma, Mb, Mc, Md = [FULL] + A + [FULL], [U] + B + [U], [NY] + C + [NY], [FULL] + D + [FULL]
    got = H.f9("fq9_mul_add2", Ma, Mb, Mc, Md)[0]
    H.check("f9_mul_add2", got, [Q9.mul(*t) for t in zip(Ma, Mb, Mc, Md)], Ma, Mb, Mc, Md)
    _values("f9_mul_add2", got, [(Q9.val(a) * Q9.val(b) + Q9.val(c) * Q9.val(d)) * RPI_P % P
                                 for a, b, c, d in zip(Ma, Mb, Mc, Md)], P)
    # a + C - b for subtrahends up to each constant's stated bound (< p, < 2.99 p, < 6.99 p)
    for cname, k in (("c2", 100), ("c3", 299), ("c7", 699)):
        Bs = [Q9.limbs(v % (k * P // 100)) for v in _rot(vals, 5)] + [Q9.limbs(k * P // 100 - 1)]
        As = A + [A[0]]
        got = H.f9("fq9_sub_" + cname, As, Bs)[0]
        name = "f9_sub F9_" + cname.upper()
        H.check(name, got, [Q9.sub(a, Q9.C["F9_" + cname.upper()], b) for a, b in zip(As, Bs)], As, Bs)
        _values(name, got, [(Q9.val(a) - Q9.val(b)) % P for a, b in zip(As, Bs)], P)


def test_fq9_zero_test_on_normalised_products():
    """f9_is_zero_mod_p, specified for normalised product outputs below 2p: true on 0 and p, false on 1, p - 1, p + 1 and on
    values that share p's lowest limb but differ above it"""
    rnd = random.Random(13)
    p0 = Q9.C["F9_P"][0]
    zero = [[0] * 9, list(Q9.C["F9_P"])]
    nonzero = [Q9.limbs(v) for v in (1, P - 1, P + 1, p0, p0 + (1 << 29), P + (1 << 29), P + (5 << 232), P - (1 << 29))]
    rand = [Q9.limbs(rnd.randrange(1, P) + rnd.randrange(2) * P) for _ in range(NRAND9)]
    a = zero + nonzero + rand + nonzero + zero
    H.check("f9_is_zero_mod_p", [r[0] for r in H.f9("fq9_is_zero_mod_p", a)[0]], [int(x in zero) for x in a], a)


def _madd_lane(pts):
    """(point, negated) entries -> the lane's device points, the model's accumulator, refusal index and affine sum"""
    ch, ref, acc, fail = [], None, None, len(pts)
    for j, (pt, neg) in enumerate(pts):
        qx, qy = Q9.limbs(_mont(pt[0])), Q9.limbs(_mont(pt[1]))
        if neg:  # a negative digit: 2p - y limb-wise, as k_msm_accum0_f9 forms it
            qy = [Q9.C["F9_C2"][i] - qy[i] for i in range(9)]
            pt = O.g1_neg(pt)
        ch.append((qx, qy))
        if fail < len(pts):
            continue
        nxt = Q9.from_affine(qx, qy) if acc is None else Q9.madd(acc, qx, qy)
        if nxt is None:
            fail = j
        else:
            acc, ref = nxt, O.g1_add(ref, pt)
    return ch, acc, fail, ref


def test_madd9_chain_matches_the_model_and_the_affine_sum():
    """48-point madd9 chains (every third point negated as 2p - y): the model's accumulator limb for limb, xyzz9_to_xyzz equal
    to the model's outgoing products, the affine sum, ZZ^3 = ZZZ^2; P + P and P - P are refused at the right step"""
    rnd = random.Random(7)
    k = 48
    pool = [_random_point(rnd) for _ in range(256)] + _edge_points()
    lanes = [[(rnd.choice(pool), j % 3 == 1) for j in range(k)] for _ in range(30)]
    p, q = pool[0], pool[1]
    s = O.g1_add(p, q)
    fill = [(rnd.choice(pool), False) for _ in range(k)]
    lanes += [([(p, False), (p, False)] + fill)[:k], ([(p, False), (p, True)] + fill)[:k],
              ([(p, False), (q, False), (s, False)] + fill)[:k], ([(p, False), (q, False), (s, True)] + fill)[:k]]
    model = [_madd_lane(pts) for pts in lanes]
    assert [m[2] for m in model[-4:]] == [1, 1, 2, 2]
    got = H.madd9_chain([m[0] for m in model])
    for i, ((ch, acc, fail, ref), (dacc, dxyzz, dfail)) in enumerate(zip(model, got)):
        assert dfail == fail, "lane %d: madd9 refused step %d, the model step %d" % (i, dfail, fail)
        assert dacc == acc, "lane %d: accumulator limbs differ from the model's" % i
        assert dxyzz == Q9.to_std(acc), "lane %d: xyzz9_to_xyzz differs from the model's outgoing products" % i
        X, Y, ZZ, ZZZ = (v * RI % P for v in dxyzz)
        assert pow(ZZ, 3, P) == pow(ZZZ, 2, P), "lane %d: ZZ^3 != ZZZ^2" % i
        assert (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P) == ref, "lane %d: not the affine sum" % i


# ------------------------------------------------------------------------------------------------ FrWide
# Only states the accumulator can reach are fed: N identical terms of a canonical pair, or the hand-made words below.  All columns
# at 2^96 - 1 is NOT one of them: no sum of terms produces it, and its total needs a word t[17] that fr_wide_reduce sets to zero
# by design.
def _wide_pairs():
    e = H.edges(R)
    return [(a, b) for a in e for b in e]


def test_wide_reduce_at_the_term_counts_of_its_bound():
    """bound: 2^29 terms of 96-bit columns, three words T0 + T1 R + T2 R^2 (poly.hip.hpp:84-90 and the carry chain at
    :123-137): N = 1, 27, 28 (T2 starts), 2^16, 2^29 and the last N that fits, every pair of edge operands"""
    lanes = [(a, b, n) for a, b in _wide_pairs() for n in W.WIDE_N + (W.wide_n_max(a, b),)]
    assert all(n >= 1 << 29 for _, _, n in lanes[5::6])
    cols = [W.wide_columns(a, b, n) for a, b, n in lanes]
    assert any(W.wide_value(c) >> 512 for c in cols)  # T2 is exercised
    got = H.wide("wide_reduce", cols)
    H.check("fr_wide_reduce", got, [n * a * b * W.RINV % R for a, b, n in lanes], *zip(*lanes))


def test_wide_mac_onto_a_nearly_full_accumulator():
    """bound: the last term that fits (poly.hip.hpp:86-87, fr_wide_mac's carry-out folded into hi): one real multiply-add onto the
    state of wide_n_max - 1 terms, so every column's low 64 bits carry into its high word at the top of the range"""
    pairs = _wide_pairs()
    nmax = [W.wide_n_max(a, b) for a, b in pairs]
    cols = [W.wide_columns(a, b, n - 1) for (a, b), n in zip(pairs, nmax)]
    got = H.wide("wide_mac", cols, [a for a, _ in pairs], [b for _, b in pairs])
    H.check("fr_wide_mac + fr_wide_reduce", got, [n * a * b * W.RINV % R for (a, b), n in zip(pairs, nmax)], *zip(*pairs))
    few = [W.wide_columns(a, b, 27) for a, b in pairs]  # and across the 27 -> 28 step, where T2 becomes non-zero
    got = H.wide("wide_mac", few, [a for a, _ in pairs], [b for _, b in pairs])
    H.check("fr_wide_mac, term 28", got, [28 * a * b * W.RINV % R for a, b in pairs], *zip(*pairs))


def test_wide_reduce_words_at_multiples_of_r():
    """bound: from_mont(T0) and T1 mod r take ANY 256-bit word, not a canonical one (poly.hip.hpp:146-147): T0 and T1 at r, 2r, 3r, 4r, 5r (2^256 // r = 5) and 2^256 - 1, every combination, the other columns zero"""
    words = (0,) + W.WIDE_WORDS
    lanes = [(t0, t1) for t0 in words for t1 in words]
    got = H.wide("wide_reduce", [W.wide_columns_of_words(t0, t1) for t0, t1 in lanes])
    H.check("fr_wide_reduce (words)", got, [(t0 + (t1 << 256)) * W.RINV % R for t0, t1 in lanes], *zip(*lanes))
