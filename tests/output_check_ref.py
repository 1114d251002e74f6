"""Plain-Python restatement of the windowed output check (co-zkvms_amd/memory_proof.py OutputCheck, csrc/output_check.inc), shared by
tests/test_output_check_model.py (CPU) and tests/test_gpu_output_check.py:

  * `dense_rounds`: the yardstick -- the plain dense product sumcheck of degree 3, HighToLow, over the three MEM-entry vectors
    eq(r_eq, .), io_range and d = v_final - v_io: every round's evaluations at X = 0, 2, 3 and the three final values.
  * `Windowed` / `windowed_rounds`: the same numbers by the windowed algorithm of the device calls: the io window [lo, hi) of W words,
    W' = 2^lw the power of two at or above W; while the half length h >= W' (rounds 0 .. m-lw-1, the sparse rounds) the window has at
    most two sides, a side's bound range is ONE scalar rho[s], its upper eq bits ONE scalar H[s], the low eq bits ONE table Llow of W'
    entries, and the round polynomial is c l_k(t) sum_s H[s] rho[s] w_s(t) (A_s + t (B_s - A_s)) from at most four windowed dot products;
    only d is folded whole; after round m-lw-1 the length is W' and the rest is the dense sumcheck on W'-entry vectors (the dense tail).
  * `first_fold_words`: the word model of the first fold's exact integer accumulation (k_oc_first_fold): D_1[y] = (1 - r) d[y] + r d[y + h]
    as two non-negative 11-limb sums of Montgomery operand x 32-bit word products (the v_final terms and the v_io terms), each below
    2^289 -- limb 9 is at most 1 and limb 10 stays 0 -- reduced once each and subtracted in the field.
Every value is a canonical field element, so the two give equal integers and the device gives equal bytes."""
import pyref as O

R = O.R
MONT = 1 << 256
M32 = (1 << 32) - 1
CO_LIMBS = 11
TS = (0, 2, 3)


def _window_vectors(v_final, v_io, lo):
    MEM, W = len(v_final), len(v_io)
    assert MEM >= 2 and MEM & (MEM - 1) == 0 and 1 <= W and lo + W <= MEM
    rng = [1 if lo <= x < lo + W else 0 for x in range(MEM)]
    d = [(v_final[x] - (v_io[x - lo] if rng[x] else 0)) % R for x in range(MEM)]
    return rng, d


def _bind(v, r):
    h = len(v) // 2
    return [(v[i] + r * (v[i + h] - v[i])) % R for i in range(h)]


def _prod_evals(polys):
    """cozk_prod_sumcheck_evals(polys, degree 3): the sums at X = 0, 2, 3 over the HighToLow pairs (i, i + h)"""
    h = len(polys[0]) // 2
    out = []
    for t in TS:
        acc = 0
        for i in range(h):
            term = 1
            for p in polys:
                term = term * (p[i] + t * (p[i + h] - p[i])) % R
            acc += term
        out.append(acc % R)
    return out


def dense_rounds(v_final, v_io, lo, r_eq, rs):
    """-> ([[s_k(0), s_k(2), s_k(3)] for every round k], (eq(r), io_range(r), d(r))); round k + 1 is bound with rs[k]"""
    m = len(r_eq)
    assert len(v_final) == 1 << m and len(rs) == m
    rng, d = _window_vectors(v_final, v_io, lo)
    polys = [O.eq_evals(r_eq), rng, d]
    rounds = []
    for k in range(m):
        rounds.append(_prod_evals(polys))
        polys = [_bind(p, rs[k]) for p in polys]
    return rounds, tuple(p[0] for p in polys)


def _eq1(a, b):
    return (a * b + (1 - a) * (1 - b)) % R


class Windowed:
    """the device handle's state machine: round_evals() is cozk_output_check_round's `out`, bind(r) what the next call does first"""

    def __init__(self, v_final, v_io, lo, r_eq):
        self.vf, self.vio, self.lo, self.r_eq = list(v_final), list(v_io), lo, list(r_eq)
        self.m, self.MEM, self.W = len(r_eq), len(v_final), len(v_io)
        assert self.MEM == 1 << self.m and self.m >= 1 and 1 <= self.W and lo + self.W <= self.MEM
        self.hi = lo + self.W
        self.lw = (self.W - 1).bit_length()
        self.Wp = 1 << self.lw
        c = (lo // self.Wp + 1) * self.Wp  # the one multiple of W' the window can hold inside
        self.sides = [(lo, c), (c, self.hi)] if c < self.hi else [(lo, self.hi)]
        self.Llow = O.eq_evals(self.r_eq[self.m - self.lw:])
        self.c, self.rho, self.k = 1, [1] * len(self.sides), 0
        self.D = None  # None: the two U32 columns are d
        self.E = self.Rg = None
        self.peak_fr = self.Wp  # Fr entries alive at once (the allocation claim)
        if self.lw == self.m:  # no sparse round: d materialised once
            rng, self.D = _window_vectors(self.vf, self.vio, lo)
            self.E, self.Rg = list(self.Llow), rng
            self.peak_fr = 3 * self.MEM

    def sparse(self):
        return self.k < self.m - self.lw

    def _bit(self, s, i):
        return (self.sides[s][0] >> (self.m - 1 - i)) & 1

    def _d(self, x):
        return self.vf[x] - (self.vio[x - self.lo] if self.lo <= x < self.hi else 0)

    def dots(self):
        """the windowed dot products of a sparse round: [(A_s, B_s)]"""
        h = (self.MEM >> self.k) // 2
        assert h >= self.Wp
        out = []
        for (a, b) in self.sides:
            A = B = 0
            for x in range(a, b):
                y, L = x % h, self.Llow[x % self.Wp]
                if self.D is None:
                    A, B = A + L * self._d(y), B + L * self._d(y + h)
                else:
                    A, B = A + L * self.D[y], B + L * self.D[y + h]
            out.append((A % R, B % R))
        return out

    def round_evals(self):
        if not self.sparse():
            return _prod_evals([self.E, self.Rg, self.D])
        k, m, lw = self.k, self.m, self.lw
        out = []
        dots = self.dots()
        for t in TS:
            acc = 0
            for s, (A, B) in enumerate(dots):
                H = 1
                for i in range(k + 1, m - lw):
                    H = H * _eq1(self.r_eq[i], self._bit(s, i)) % R
                w = t if self._bit(s, k) else 1 - t
                acc += H * self.rho[s] * w * (A + t * (B - A))
            l = (1 - self.r_eq[k]) * (1 - t) + self.r_eq[k] * t
            out.append(self.c * l * acc % R)
        return out

    def bind(self, r):
        k = self.k
        if self.sparse():
            h = (self.MEM >> k) // 2
            self.c = self.c * _eq1(self.r_eq[k], r) % R
            self.rho = [rho * (r if self._bit(s, k) else 1 - r) % R for s, rho in enumerate(self.rho)]
            if self.D is None:  # the first fold, straight from the columns
                self.D = [((1 - r) * self._d(y) + r * self._d(y + h)) % R for y in range(h)]
                self.peak_fr = max(self.peak_fr, h + 2 * self.Wp)
            else:
                self.D = _bind(self.D, r)
            self.k += 1
            if not self.sparse():  # the dense tail begins: length W'
                assert len(self.D) == self.Wp
                self.E = [self.c * L % R for L in self.Llow]
                self.Rg = [0] * self.Wp
                for s, (a, b) in enumerate(self.sides):
                    for x in range(a, b):
                        assert self.Rg[x % self.Wp] == 0
                        self.Rg[x % self.Wp] = self.rho[s]
        else:
            self.E, self.Rg, self.D = _bind(self.E, r), _bind(self.Rg, r), _bind(self.D, r)
            self.k += 1

    def final(self, r):
        assert self.k == self.m - 1
        self.bind(r)
        return (self.E[0], self.Rg[0], self.D[0])


def windowed_rounds(v_final, v_io, lo, r_eq, rs):
    """what dense_rounds returns, by the windowed algorithm; also the largest count of Fr entries alive at once"""
    w = Windowed(v_final, v_io, lo, r_eq)
    rounds = []
    for k in range(w.m):
        if k:
            w.bind(rs[k - 1])
        rounds.append(w.round_evals())
    return rounds, w.final(rs[-1]), w.peak_fr


# ------------------------------------------------------------------------------------------------ k_oc_first_fold, exact form
def _limbs32(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def _mac(acc, coeff, v):
    """co_mac<0>: acc += coeff * v on 32-bit words, every carry propagated with its term"""
    assert 0 <= coeff < MONT and 0 <= v <= M32
    c, carry = _limbs32(coeff, 8), 0
    for k in range(8):
        t = c[k] * v + acc[k] + carry
        assert t < 1 << 64  # (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        acc[k], carry = t & M32, t >> 32
    for k in range(8, CO_LIMBS):
        t = acc[k] + carry
        acc[k], carry = t & M32, t >> 32
    assert carry == 0


def _reduce(acc):
    """co_reduce: S = T0 + 2^256 T1, S mod r as to_mont(from_mont(T0)) + to_mont(T1): the Montgomery form stays a Montgomery form"""
    S = sum(w << (32 * i) for i, w in enumerate(acc))
    t0, t1 = S & (MONT - 1), S >> 256
    inv = pow(MONT, -1, R)
    got = (t0 * inv % R * MONT + t1 * MONT) % R
    assert got == S % R
    return got


def first_fold_words(vf_lo, vf_hi, io_lo, io_hi, r):
    """the 256-bit word k_oc_first_fold stores for one pair: Montgomery form of (1 - r) (vf_lo - io_lo) + r (vf_hi - io_hi); io_* None: that
    word lies outside the window.  The limb bound the kernel states is asserted: two terms below 2^288 each keep a sum below 2^289."""
    a, b = (1 - r) % R * MONT % R, r % R * MONT % R
    pos, neg = [0] * CO_LIMBS, [0] * CO_LIMBS
    _mac(pos, a, vf_lo)
    _mac(pos, b, vf_hi)
    if io_lo is not None:
        _mac(neg, a, io_lo)
    if io_hi is not None:
        _mac(neg, b, io_hi)
    for acc in (pos, neg):
        assert sum(w << (32 * i) for i, w in enumerate(acc)) < 1 << 289 and acc[9] <= 1 and acc[10] == 0
    return (_reduce(pos) - _reduce(neg)) % R


def windows(m, seed):
    """the windows the tests cover at MEM = 2^m, as (lo, W), without repeats"""
    import random
    MEM = 1 << m
    out = [(0, 1), (0, MEM), (MEM - 1, 1), (0, MEM // 2), (MEM // 2, MEM // 2), (MEM // 2 - 1, 2)]
    for j in range(m):
        W = (1 << j) + 1
        if W <= MEM:
            mid = (MEM - W) // 2 | 1  # an odd start, where it fits
            out += [(0, W), (MEM - W, W), (mid if mid + W <= MEM else 0, W)]
    rnd = random.Random(seed)
    for _ in range(4):
        W = rnd.randint(1, MEM)
        out.append((rnd.randint(0, MEM - W), W))
    seen, uniq = set(), []
    for lo, W in out:
        if lo >= 0 and W >= 1 and lo + W <= MEM and (lo, W) not in seen:
            seen.add((lo, W))
            uniq.append((lo, W))
    return uniq
