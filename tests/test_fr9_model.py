"""CPU model of the 9 x 29-bit unsaturated Fr arithmetic of the GKR / toggle / outer round-sum kernels (co-zkvms_amd/csrc/fr9.hip.hpp):
the multiplier's column schedule with the constants parsed from the generated fr9_consts.inc and the fold period from the header, an
assertion on every 64-bit column accumulator, every 32-bit limb and every documented operand precondition.  Checks (no GPU):
  (i) the generated constants are what their comments say;
  (ii) each kernel's per-lane chain (layer9_terms / layer9_group_flush, k_toggle_cubic9's heavy(), k_outer_round_act9), written as the
       kernel writes it, gives the exact big-int sum mod r for N terms per lane around and far beyond the fold period, with random,
       all-(r - 1) and max-limb operands;
  (iii) a bound tracker -- the same chains over (value bound, per-limb bound) -- reaches a fixed point after one fold period, which
       proves the accumulators stay in range for EVERY N; without the fold the same tracker rejects a chain of 4096 terms."""
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "co-zkvms_amd", "csrc")
RMOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
W, N = 29, 9
MASK = (1 << W) - 1
R, RP = 1 << 256, 1 << 261
U32, U64 = 1 << 32, 1 << 64
MUL_A_MAX = int(2 ** 30.6)  # fr9_mul: first operand's limbs
MUL2_A_MAX = 3 << 29        # fr9_mul_add2: first operands' limbs (1.5 x 2^30)
R_INV = pow(R, -1, RMOD)


def _consts():
    txt = open(os.path.join(CSRC, "fr9_consts.inc")).read()
    out = {}
    for name, body in re.findall(r"(FR9_\w+)\[9\] = \{([^}]*)\}", txt):
        out[name] = [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
    out["FR9_INV"] = int(re.search(r"FR9_INV = (0x[0-9a-f]+)u", txt).group(1), 16)
    return out


C = _consts()
FOLD = int(re.search(r"FR9_FOLD_PERIOD = (\d+);", open(os.path.join(CSRC, "fr9.hip.hpp")).read()).group(1))
PL = C["FR9_P"]


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def limbs(x):
    return [(x >> (W * i)) & MASK for i in range(N)]


def test_generated_constants():
    assert val(PL) == RMOD and all(x <= MASK for x in PL)
    assert (C["FR9_INV"] * RMOD + 1) % (1 << W) == 0 and C["FR9_INV"] <= MASK
    # k r spread so that limb-wise a + C - b never borrows for any b of the stated limb / value bounds
    for name, k, lift, bound in (("FR9_C2", 2, 1, 1.0), ("FR9_C3", 3, 2, 2.1), ("FR9_C5", 5, 4, 4.3)):
        assert val(C[name]) == k * RMOD
        assert all(lift << W <= x < (lift + 1) << W for x in C[name][:-1]), name
        assert C[name][8] > int(bound * RMOD) >> (W * 8), name
    for name, e in (("FR9_K1", 5), ("FR9_K2", 10), ("FR9_K3", 15)):
        assert val(C[name]) == RP * (1 << e) % RMOD and all(x <= MASK for x in C[name]), name
    assert val(C["FR9_RP"]) == RP % RMOD and all(x <= MASK for x in C["FR9_RP"])
    assert FOLD > 0 and FOLD & (FOLD - 1) == 0  # the kernels test the counter with a mask


# ---------------------------------------------------------------------------------------------------------------- exact limbs
class Exact:
    """the kernels' limb arithmetic on concrete values (lists of 9 limbs)"""

    @staticmethod
    def _mul(a, b, c=None, d=None):
        acc, m, r = 0, [0] * 9, [0] * 9
        for k in range(17):
            lo, hi = max(0, k - 8), min(k, 8)
            for i in range(lo, hi + 1):
                acc += a[i] * b[k - i]
                if c is not None:
                    acc += c[i] * d[k - i]
            if k < 9:
                for i in range(k):
                    acc += m[i] * PL[k - i]
                m[k] = ((acc & 0xFFFFFFFF) * C["FR9_INV"]) & MASK
                acc += m[k] * PL[0]
                assert acc < U64 and acc & MASK == 0
            else:
                for i in range(lo, 9):
                    acc += m[i] * PL[k - i]
                assert acc < U64
                r[k - 9] = acc & MASK
            acc >>= W
        assert acc < U32
        r[8] = acc
        return r

    @classmethod
    def mul(cls, a, b):
        assert all(x < MUL_A_MAX for x in a), "fr9_mul: first operand's limbs >= 2^30.6"
        assert all(x <= MASK for x in b), "fr9_mul: second operand not normalised"
        return cls._mul(a, b)

    @classmethod
    def mul_add2(cls, a, b, c, d):
        assert all(x < MUL2_A_MAX for x in a + c), "fr9_mul_add2: first operands' limbs >= 1.5 x 2^30"
        assert all(x <= MASK for x in b + d), "fr9_mul_add2: second operands not normalised"
        return cls._mul(a, b, c, d)

    @staticmethod
    def add(a, b):
        r = [x + y for x, y in zip(a, b)]
        assert all(x < U32 for x in r)
        return r

    @staticmethod
    def sub(a, Cc, b):
        assert all(Cc[i] >= b[i] for i in range(9)), "f9_sub: constant does not dominate the subtrahend"
        r = [a[i] + Cc[i] - b[i] for i in range(9)]
        assert all(0 <= x < U32 for x in r)
        return r

    @staticmethod
    def norm(a):
        r, c = [0] * 9, 0
        for i in range(8):
            t = a[i] + c
            assert t < U32
            r[i], c = t & MASK, t >> W
        r[8] = a[8] + c
        assert r[8] < U32
        return r

    @classmethod
    def canonical(cls, a):
        """fr9_to_canonical: f9_norm, re-limb to 8 x 32 (bits >= 256 would be lost), two reduce_once"""
        v = val(cls.norm(a))
        assert v < R, "fr9_to_canonical: value >= 2^256"
        for _ in range(2):
            if v >= RMOD:
                v -= RMOD
        assert v < RMOD, "fr9_to_canonical: input >= 3r"
        return v

    @staticmethod
    def load(x):
        assert 0 <= x < RMOD
        return limbs(x)

    @staticmethod
    def const(name):
        return list(C[name])

    @staticmethod
    def zero():
        return [0] * 9


# ---------------------------------------------------------------------------------------------------------------- bounds
class B:
    """an upper bound on a lazy value: its value and each limb"""

    def __init__(self, v, l):
        self.v, self.l = v, list(l)

    def le(self, o):
        return self.v <= o.v and all(x <= y for x, y in zip(self.l, o.l))


class Bound:
    """the same operations over bounds, with the same assertions: monotone, so a chain that passes here passes for every
    operand below the bounds"""

    @staticmethod
    def _mul(a, b, c=None, d=None):
        acc = 0
        for k in range(17):
            lo, hi = max(0, k - 8), min(k, 8)
            for i in range(lo, hi + 1):
                acc += a.l[i] * b.l[k - i]
                if c is not None:
                    acc += c.l[i] * d.l[k - i]
            if k < 9:
                acc += sum(MASK * PL[k - i] for i in range(k + 1))
            else:
                acc += sum(MASK * PL[k - i] for i in range(lo, 9))
            assert acc < U64, "column accumulator overflows 64 bits"
            acc >>= W
        assert acc < U32
        v = a.v * b.v + (c.v * d.v if c is not None else 0)
        v = (v + (RP - 1) * RMOD) // RP
        return B(v, [MASK] * 8 + [min(acc, v >> (W * 8))])

    @classmethod
    def mul(cls, a, b):
        assert all(x < MUL_A_MAX for x in a.l), "fr9_mul: first operand's limbs >= 2^30.6"
        assert all(x <= MASK for x in b.l), "fr9_mul: second operand not normalised"
        return cls._mul(a, b)

    @classmethod
    def mul_add2(cls, a, b, c, d):
        assert all(x < MUL2_A_MAX for x in a.l + c.l), "fr9_mul_add2: first operands' limbs >= 1.5 x 2^30"
        assert all(x <= MASK for x in b.l + d.l), "fr9_mul_add2: second operands not normalised"
        return cls._mul(a, b, c, d)

    @staticmethod
    def add(a, b):
        r = B(a.v + b.v, [x + y for x, y in zip(a.l, b.l)])
        assert all(x < U32 for x in r.l)
        return r

    @staticmethod
    def sub(a, Cc, b):
        assert all(Cc[i] >= b.l[i] for i in range(9)), "f9_sub: constant does not dominate the subtrahend"
        r = B(a.v + val(Cc), [a.l[i] + Cc[i] for i in range(9)])
        assert all(x < U32 for x in r.l)
        return r

    @staticmethod
    def norm(a):
        r, c = [0] * 9, 0
        for i in range(8):
            t = a.l[i] + c
            assert t < U32
            r[i], c = min(t, MASK), t >> W
        r[8] = min(a.l[8] + c, a.v >> (W * 8))
        assert a.l[8] + c < U32
        return B(a.v, r)

    @classmethod
    def canonical(cls, a):
        a = cls.norm(a)
        assert a.v < R, "fr9_to_canonical: value >= 2^256"
        assert a.v < 3 * RMOD, "fr9_to_canonical: input >= 3r"
        return None

    @staticmethod
    def load(x):
        return B(RMOD - 1, [MASK] * 8 + [(RMOD - 1) >> (W * 8)])

    @staticmethod
    def const(name):
        return B(val(C[name]), C[name])

    @staticmethod
    def zero():
        return B(0, [0] * 9)


# ---------------------------------------------------------------------------------------------------------------- the chains
def fold(X, s):
    """the periodic fold: one product by R' mod r -- the same field element, value back below ~1.8 r"""
    return X.mul(s, X.const("FR9_RP"))


def sh9_local_mul(X, x, y):
    if len(x) == 1:
        return X.mul(x[0], X.norm(y[0]))
    return X.mul_add2(x[0], X.norm(X.add(y[0], y[1])), x[1], X.norm(y[0]))


def sh9_lerp(X, lo, hi, r5):
    return [X.add(lo[k], X.mul(X.sub(hi[k], C["FR9_C2"], lo[k]), r5)) for k in range(len(lo))]


def layer9_terms(X, l0, r0, l1, r1, e0, e1, acc):
    """layer9_terms after the eq pair is formed: s_k += e_k x (l_k x r_k) at X = 0, 2, 3"""
    me = X.norm(X.sub(e1, C["FR9_C2"], e0))
    e2 = X.add(e1, me)
    e3 = X.add(e2, me)
    ml = [X.norm(X.sub(l1[k], C["FR9_C3"], l0[k])) for k in range(len(l0))]
    mr = [X.norm(X.sub(r1[k], C["FR9_C3"], r0[k])) for k in range(len(r0))]
    l2 = [X.norm(X.add(l1[k], ml[k])) for k in range(len(l0))]
    r2 = [X.norm(X.add(r1[k], mr[k])) for k in range(len(r0))]
    l3 = [X.norm(X.add(l2[k], ml[k])) for k in range(len(l0))]
    r3 = [X.norm(X.add(r2[k], mr[k])) for k in range(len(r0))]
    acc[0] = X.norm(X.add(acc[0], X.mul(e0, sh9_local_mul(X, l0, r0))))
    acc[1] = X.norm(X.add(acc[1], X.mul(e2, sh9_local_mul(X, l2, r2))))
    acc[2] = X.norm(X.add(acc[2], X.mul(e3, sh9_local_mul(X, l3, r3))))


def layer_lane(X, items, nc, nested, bind, period, state=None, worst=False):
    """one lane of k_layer_cubic9 (bind = None) / k_layer_bind_cubic9 (bind = r5): items are per-iteration tuples
    (inputs, E-table values, group index).  Returns (s, grp) before the final flush.  worst (bounds only): NESTED = 2 flushes the
    never-reset group every iteration -- an upper bound on every group schedule."""
    s, grp, gx, gsc = state if state is not None else ([X.zero()] * 3, [X.zero()] * 3, None, None)
    s, grp = list(s), list(grp)
    for it, (u, ev, x2) in enumerate(items):
        if period and it > 0 and it % period == 0:
            s = [fold(X, v) for v in s]
            grp = [fold(X, v) for v in grp]
        if bind is not None:
            # k_layer_bind_cubic9: 8 inputs per component -> 4 bound values, stored canonical
            ld = [[X.load(c) for c in e] for e in u]
            v = [sh9_lerp(X, ld[0], ld[2], bind), sh9_lerp(X, ld[1], ld[3], bind), sh9_lerp(X, ld[4], ld[6], bind),
                 sh9_lerp(X, ld[5], ld[7], bind)]
            for q in v:
                for c in q:
                    X.canonical(c)
        else:
            v = [[X.load(c) for c in e] for e in u]
        if nested == 2:
            if worst or x2 != gx:  # layer9_group_flush of the previous group, then a fresh group
                if gx is not None:
                    s = [X.norm(X.add(s[k], X.mul(grp[k], X.load(gsc)))) for k in range(3)]
                if not worst:
                    grp = [X.zero()] * 3
                gx, gsc = x2, ev[2]
            layer9_terms(X, v[0], v[1], v[2], v[3], X.load(ev[0]), X.load(ev[1]), grp)
        else:
            if nested == 1:
                sc = X.load(ev[2])
                e0, e1 = X.mul(X.load(ev[0]), sc), X.mul(X.load(ev[1]), sc)
            else:
                e0, e1 = X.load(ev[0]), X.load(ev[1])
            layer9_terms(X, v[0], v[1], v[2], v[3], e0, e1, s)
    return s, grp, gx, gsc


def layer_finish(X, s, grp, gx, gsc, nested):
    if nested == 2 and gx is not None:
        s = [X.norm(X.add(s[k], X.mul(grp[k], X.load(gsc)))) for k in range(3)]
    K = X.const("FR9_K3" if nested else "FR9_K2")
    return [X.canonical(X.mul(v, K)) for v in s]


def line3(X, v0, v1, cs="FR9_C2"):
    m = X.norm(X.sub(v1, C[cs], v0))
    x2 = X.add(v1, m)
    return v0, x2, X.add(x2, m)


def toggle_lane(X, items, nc, nested, period, state=None):
    """the heavy() calls of one lane of k_toggle_cubic9: item = (E values, flag pair, fingerprint pair)"""
    A, Cs = (list(x) for x in state) if state is not None else ([X.zero()] * 3, [X.zero()] * 3)
    for it, (ev, fl, fp) in enumerate(items):
        if period and it > 0 and it % period == 0:
            A = [fold(X, v) for v in A]
            Cs = [fold(X, v) for v in Cs]
        if nested:
            r = line3(X, X.load(ev[0]), X.load(ev[1]))
            sc = X.load(ev[2])
            e = [X.mul(x, sc) for x in r]
        else:
            r = line3(X, X.load(ev[0]), X.load(ev[1]))
            e = [r[0], X.norm(r[1]), X.norm(r[2])]
        g = line3(X, X.load(fl[0]), X.load(fl[1]))
        q = [[X.load(c) for c in f] for f in fp]
        s0 = X.norm(X.add(q[0][0], q[0][1])) if nc == 2 else q[0][0]
        s1 = X.norm(X.add(q[1][0], q[1][1])) if nc == 2 else q[1][0]
        p = line3(X, s0, s1, "FR9_C3" if nc == 2 else "FR9_C2")
        for k in range(3):
            c = X.mul(g[k], e[k])
            Cs[k] = X.norm(X.add(Cs[k], c))
            A[k] = X.norm(X.add(A[k], X.mul(p[k], c)))
    return A, Cs


def toggle_finish(X, A, Cs, nested):
    KC, KA = X.const("FR9_K2" if nested else "FR9_K1"), X.const("FR9_K3" if nested else "FR9_K2")
    return [X.canonical(X.mul(a, KA)) for a in A] + [X.canonical(X.mul(c, KC)) for c in Cs]


def outer_lane(X, items, nc, want_t0, period, state=None):
    """one lane of k_outer_round_act9: item = (E_out, E_in, a0, b0, a1, b1, c0) with a1 = b1 = zeros when the pair has no high row"""
    s = list(state) if state is not None else [X.zero()] * 3
    for it, (eo, ei, a0, b0, a1, b1, c0) in enumerate(items):
        if period and it > 0 and it % period == 0:
            s = [fold(X, v) for v in s]
        e = X.mul(X.load(eo), X.load(ei))
        a0, b0, a1, b1 = ([X.load(c) for c in x] for x in (a0, b0, a1, b1))
        da = [X.sub(a1[k], C["FR9_C2"], a0[k]) for k in range(nc)]
        db = [X.sub(b1[k], C["FR9_C2"], b0[k]) for k in range(nc)]
        s[2] = X.norm(X.add(s[2], X.mul(e, sh9_local_mul(X, da, db))))
        if want_t0:
            s[0] = X.norm(X.add(s[0], X.mul(e, sh9_local_mul(X, a0, b0))))
            cc = [X.load(c) for c in c0]
            s[1] = X.norm(X.add(s[1], X.mul(X.add(cc[0], cc[1]) if nc == 2 else cc[0], e)))
    return s


def outer_finish(X, s):
    return [X.canonical(X.mul(s[0], X.const("FR9_K3"))), X.canonical(X.mul(s[1], X.const("FR9_K2"))),
            X.canonical(X.mul(s[2], X.const("FR9_K3")))]


# ---------------------------------------------------------------------------------------------------------------- references
def std(x):
    """stored (R-form) -> the field element"""
    return x * R_INV % RMOD


def lmul(x, y):
    """the Rep3 local product as an additive share (plain: the product)"""
    return x[0] * y[0] % RMOD if len(x) == 1 else (x[0] * (y[0] + y[1]) + x[1] * y[0]) % RMOD


def line(v0, v1, X):
    return (v0 + X * (v1 - v0)) % RMOD


def ref_layer(items, nc, nested, bind_r):
    s = [0, 0, 0]
    for u, ev, _ in items:
        u = [[std(c) for c in e] for e in u]
        if bind_r is not None:
            u = [[line(u[i][k], u[i + 2][k], bind_r) for k in range(nc)] for i in (0, 1, 4, 5)]
        l0, r0, l1, r1 = u
        e0, e1 = std(ev[0]), std(ev[1])
        sc = std(ev[2]) if nested else 1
        for k, X in enumerate((0, 2, 3)):
            l = [line(l0[c], l1[c], X) for c in range(nc)]
            r = [line(r0[c], r1[c], X) for c in range(nc)]
            s[k] = (s[k] + line(e0, e1, X) * sc * lmul(l, r)) % RMOD
    return [x * R % RMOD for x in s]


def ref_toggle(items, nc, nested):
    A, Cs = [0, 0, 0], [0, 0, 0]
    for ev, fl, fp in items:
        sc = std(ev[2]) if nested else 1
        f = [sum(std(c) for c in x) % RMOD for x in fp]
        for k, X in enumerate((0, 2, 3)):
            c = line(std(ev[0]), std(ev[1]), X) * sc * line(std(fl[0]), std(fl[1]), X) % RMOD
            Cs[k] = (Cs[k] + c) % RMOD
            A[k] = (A[k] + c * line(f[0], f[1], X)) % RMOD
    return [x * R % RMOD for x in A + Cs]


def ref_outer(items, nc, want_t0):
    s = [0, 0, 0]
    for eo, ei, a0, b0, a1, b1, c0 in items:
        e = std(eo) * std(ei) % RMOD
        a0, b0, a1, b1 = ([std(c) for c in x] for x in (a0, b0, a1, b1))
        s[2] = (s[2] + e * lmul([a1[k] - a0[k] for k in range(nc)], [b1[k] - b0[k] for k in range(nc)])) % RMOD
        if want_t0:
            s[0] = (s[0] + e * lmul(a0, b0)) % RMOD
            s[1] = (s[1] + e * sum(std(c) for c in c0)) % RMOD
    return [x * R % RMOD for x in s]


# ---------------------------------------------------------------------------------------------------------------- operands
MAXLIMB = (((RMOD >> (W * 8)) - 1) << (W * 8)) | ((1 << (W * 8)) - 1)  # < r with limbs 0..7 all 2^29 - 1
assert MAXLIMB < RMOD


def operand_source(kind, seed):
    rnd = random.Random(seed)
    if kind == "random":
        return lambda: rnd.randrange(RMOD)
    if kind == "rmax":
        return lambda: RMOD - 1
    return lambda: MAXLIMB if rnd.random() < 0.9 else RMOD - 1


def layer_items(n, nc, nested, bind, kind, seed, group=3):
    g = operand_source(kind, seed)
    nin = 8 if bind else 4
    sc = [g() for _ in range(n // group + 2)]
    return [([[g() for _ in range(nc)] for _ in range(nin)], (g(), g(), sc[i // group]), i // group) for i in range(n)]


def toggle_items(n, nc, kind, seed):
    g = operand_source(kind, seed)
    one = R % RMOD
    out = []
    for i in range(n):
        fl = (g(), g()) if i % 3 else (one, one if i % 2 else 0)  # bound flags, or the first round's 0 / 1 pairs
        out.append(((g(), g(), g()), fl, [[g() for _ in range(nc)] for _ in range(2)]))
    return out


def outer_items(n, nc, kind, seed):
    g = operand_source(kind, seed)
    z = [0] * nc
    out = []
    for i in range(n):
        hi = i % 5 != 4  # some pairs have no high row (odd active row count)
        a1 = [g() for _ in range(nc)] if hi else z
        b1 = [g() for _ in range(nc)] if hi else z
        out.append((g(), g(), [g() for _ in range(nc)], [g() for _ in range(nc)], a1, b1, [g() for _ in range(nc)]))
    return out


SIZES = [1, FOLD - 1, FOLD, FOLD + 1, 4 * FOLD + 3]


def sizes(kind):
    return SIZES + [5000] if kind == "random" else SIZES
LAYER_VARIANTS = [(nc, ne, bind) for nc in (1, 2) for ne in (0, 1, 2) for bind in (False, True)]
R5 = (123456789 * R % RMOD) * 32 % RMOD  # the bind challenge times 2^5, R-form (what the launcher passes)


def _run_layer(nc, ne, bind, items):
    got = layer_finish(Exact, *layer_lane(Exact, items, nc, ne, limbs(R5) if bind else None, FOLD), ne)
    assert got == ref_layer(items, nc, ne, 123456789 if bind else None)


@pytest.mark.parametrize("nc,nested,bind", LAYER_VARIANTS)
@pytest.mark.parametrize("kind", ["random", "rmax", "maxlimb"])
def test_layer_chain_is_exact(nc, nested, bind, kind):
    for n in sizes(kind):
        _run_layer(nc, nested, bind, layer_items(n, nc, nested, bind, kind, 1000 * n + nc))


@pytest.mark.parametrize("nc,nested", [(1, 0), (1, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("kind", ["random", "rmax", "maxlimb"])
def test_toggle_chain_is_exact(nc, nested, kind):
    for n in sizes(kind):
        items = toggle_items(n, nc, kind, 77 + n)
        A, Cs = toggle_lane(Exact, items, nc, nested, FOLD)
        assert toggle_finish(Exact, A, Cs, nested) == ref_toggle(items, nc, nested), n


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("want_t0", [0, 1])
@pytest.mark.parametrize("kind", ["random", "rmax", "maxlimb"])
def test_outer_chain_is_exact(nc, want_t0, kind):
    for n in sizes(kind):
        items = outer_items(n, nc, kind, 55 + n)
        assert outer_finish(Exact, outer_lane(Exact, items, nc, want_t0, FOLD)) == ref_outer(items, nc, want_t0), n


def test_long_chains_are_exact():
    """5000 terms per lane (39 folds) through one variant of each kernel with the all-(r - 1) and max-limb operands"""
    n = 5000
    _run_layer(2, 1, False, layer_items(n, 2, 1, False, "rmax", 1))
    _run_layer(1, 2, True, layer_items(n, 1, 2, True, "random", 2, group=7))
    items = toggle_items(n, 2, "rmax", 3)
    assert toggle_finish(Exact, *toggle_lane(Exact, items, 2, 1, FOLD), 1) == ref_toggle(items, 2, 1)
    items = outer_items(n, 2, "maxlimb", 4)
    assert outer_finish(Exact, outer_lane(Exact, items, 2, 1, FOLD)) == ref_outer(items, 2, 1)


def test_toggle_rep3_fingerprint_line_at_the_edge():
    """a Rep3 fingerprint's a + b reaches 2r - 2, whose top limb is one above FR9_C2's: the line through two such sums needs
    FR9_C3 (with FR9_C2 the top limb of v1 + C - v0 wraps when v1 < 2^232)"""
    one = R % RMOD
    items = [((5, 7, 9), (one, one), [[RMOD - 1, RMOD - 1], [0, 3]]), ((11, 13, 17), (one, 0), [[1, 2], [RMOD - 1, RMOD - 2]])]
    for nested in (0, 1):
        assert toggle_finish(Exact, *toggle_lane(Exact, items, 2, nested, FOLD), nested) == ref_toggle(items, 2, nested)
    with pytest.raises(AssertionError):
        Exact.sub(limbs(3), C["FR9_C2"], limbs(2 * RMOD - 2))


def test_long_chain_without_the_fold_fails():
    """teeth: the unfolded accumulator of 4096 all-(r - 1) terms overflows (what the kernels did before the fold)"""
    items = layer_items(4096, 1, 0, False, "rmax", 5)
    with pytest.raises(AssertionError):
        layer_finish(Exact, *layer_lane(Exact, items, 1, 0, None, None), 0)


# ---------------------------------------------------------------------------------------------------------------- bound tracker
DUMMY_LAYER = [([[0, 0]] * 8, (0, 0, 0), 0)]
DUMMY_TOGGLE = [((0, 0, 0), (0, 0), [[0, 0], [0, 0]])]
DUMMY_OUTER = [(0, 0, [0, 0], [0, 0], [0, 0], [0, 0], [0, 0])]


def _layer_kernel(nc, nested, bind):
    r5 = Bound.load(0) if bind else None
    run = lambda st, n, period=None: layer_lane(Bound, DUMMY_LAYER * n, nc, nested, r5, period, st, worst=True)
    fold_all = lambda st: ([fold(Bound, v) for v in st[0]], [fold(Bound, v) for v in st[1]], st[2], st[3])
    finish = lambda st: layer_finish(Bound, *st, nested)
    return run, fold_all, finish, ([Bound.zero()] * 3, [Bound.zero()] * 3, None, None)


def _toggle_kernel(nc, nested):
    run = lambda st, n, period=None: toggle_lane(Bound, DUMMY_TOGGLE * n, nc, nested, period, st)
    fold_all = lambda st: ([fold(Bound, v) for v in st[0]], [fold(Bound, v) for v in st[1]])
    finish = lambda st: toggle_finish(Bound, st[0], st[1], nested)
    return run, fold_all, finish, ([Bound.zero()] * 3, [Bound.zero()] * 3)


def _outer_kernel(nc):
    run = lambda st, n, period=None: outer_lane(Bound, DUMMY_OUTER * n, nc, 1, period, st)
    fold_all = lambda st: [fold(Bound, v) for v in st]
    finish = lambda st: outer_finish(Bound, st)
    return run, fold_all, finish, [Bound.zero()] * 3


KERNELS = [("layer%d_nc%d%s" % (ne, nc, "_bind" if b else ""), lambda nc=nc, ne=ne, b=b: _layer_kernel(nc, ne, b))
           for nc, ne, b in LAYER_VARIANTS]
KERNELS += [("toggle%d_nc%d" % (ne, nc), lambda nc=nc, ne=ne: _toggle_kernel(nc, ne)) for nc in (1, 2) for ne in (0, 1)]
KERNELS += [("outer_nc%d" % nc, lambda nc=nc: _outer_kernel(nc)) for nc in (1, 2)]


def _states(st):
    """the accumulators of a chain state, flattened"""
    out = []
    for x in st:
        if isinstance(x, B):
            out.append(x)
        elif isinstance(x, list):
            out += _states(x)
    return out


def _inflate(st):
    """a state with 1/64 of slack on every value bound: the candidate invariant"""
    if isinstance(st, B):
        v = st.v + st.v // 64
        return B(v, [MASK] * 8 + [max(st.l[8], v >> (W * 8))])
    if isinstance(st, (list, tuple)):
        return type(st)(_inflate(x) for x in st)
    return st


@pytest.mark.parametrize("name,make", KERNELS, ids=[k[0] for k in KERNELS])
def test_bounds_reach_a_fixed_point_after_one_fold_period(name, make):
    """from zero, FOLD terms and a fold give a state; with some slack that is S, and from S, FOLD terms and a fold stay below S.
    The operations are monotone in their bounds and zero is below S, so every fold period starts below S: no accumulator, column or limb overflows and the final product is
    canonical after two conditional subtractions, for ANY number of terms per lane.  The finish is checked from the largest state
    (S + FOLD terms, then the NESTED = 2 last group flush)."""
    run, fold_all, finish, zero = make()
    S = _inflate(fold_all(run(zero, FOLD)))
    S2 = fold_all(run(S, FOLD))
    assert all(b.le(a) for a, b in zip(_states(S), _states(S2))), name
    finish(run(S, FOLD))
    finish(zero)
    top = max(b.v for b in _states(run(S, FOLD)))
    assert top < 200 * RMOD  # ~138 r at the default period: far from the 2^30.6 first-operand limb bound (~512 r)


@pytest.mark.parametrize("name,make", KERNELS, ids=[k[0] for k in KERNELS])
def test_bound_tracker_rejects_the_chain_without_the_fold(name, make):
    """teeth: the same tracker with the fold disabled fails at 4096 terms per lane"""
    run, fold_all, finish, zero = make()
    with pytest.raises(AssertionError):
        finish(run(zero, 4096))
