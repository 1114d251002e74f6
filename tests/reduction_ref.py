"""Bit-level models of the two hand-written Fr reductions whose correctness rests on a bound argued in a comment, and the
directed operand sets that sit on those bounds:
  * fr_mul_small_add (co-zkvms_amd/csrc/shamir.hip): a * p + c mod r for a plain p <= 32 through ONE 32-bit quotient estimate
    q = T // D in {Q - 1, Q} and one conditional subtraction;
  * FrWide / fr_wide_reduce (co-zkvms_amd/csrc/poly.hip.hpp): 15 column accumulators of 96 bits, carried into 17 words and reduced
    once as from_mont(T0) + (T1 mod r) + to_mont(T2).
The models repeat the kernels' word arithmetic (so a test can say which path an operand takes) and assert the invariants the
comments claim; the expected VALUES of every test come from plain big-int arithmetic, never from these models.  Shared by
tests/test_reduction_models.py (CPU) and the directed GPU tests."""
import numpy as np

import pyref as O

R = O.R
MONT = 1 << 256
RINV = pow(MONT, -1, R)
M32 = (1 << 32) - 1
SMALL_SHIFT = 228
SMALL_D = (R >> SMALL_SHIFT) + 1  # D = floor(r / 2^228) + 1
SMALL_P_MAX = 32
WIDE_COLUMN_BOUND = 1 << 96


def _limbs32(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


# ------------------------------------------------------------------------------------------------ fr_mul_small_add
def small_mul_add_model(a, p, c):
    """the 9-word arithmetic of fr_mul_small_add on residues a, c < r and a plain 0 <= p <= 32 -> (result, q, t // r)"""
    assert 0 <= a < R and 0 <= c < R and 0 <= p <= SMALL_P_MAX
    A, C, M = _limbs32(a), _limbs32(c), _limbs32(R)
    t, carry = [0] * 9, 0
    for i in range(8):
        m = A[i] * p + C[i] + carry
        assert m < 1 << 64
        t[i] = m & M32
        carry = m >> 32
    assert carry < 16  # t < 2^260: (t[8] << 28) keeps every bit
    t[8] = carry
    tv = sum(w << (32 * i) for i, w in enumerate(t))
    assert tv == a * p + c
    T = ((t[8] << 28) & M32) | (t[7] >> 4)
    assert T == tv >> SMALL_SHIFT
    q = T // SMALL_D
    s, mc, borrow = [0] * 8, 0, 0
    for i in range(8):
        m = q * M[i] + mc
        mc = m >> 32
        d = (t[i] - (m & M32) - borrow) & ((1 << 64) - 1)
        s[i] = d & M32
        borrow = (d >> 63) & 1
    sv = sum(w << (32 * i) for i, w in enumerate(s))
    assert 0 <= tv - q * R < 1 << 256 and sv == tv - q * R  # word 8 of t - q r is zero: the eight words are the value
    return (sv - R if sv >= R else sv), q, tv // R  # reduce_once


def small_mul_add_cases(deltas=None):
    """the directed set: (p, Q, a, c) with t = a p + c = Q r + delta for Q = 0..p and delta around 0 (a negative one lands under
    the multiple: floor(t / r) = Q - 1 there), around d* = Q (D 2^228 - r) -- the first delta at which the estimate reaches Q --
    and at the top of the interval; `deltas` (a function of d*) picks another subset"""
    if deltas is None:
        deltas = lambda ds: (-2, -1, 0, 1, 2, ds - 1, ds, ds + 1, R - 2, R - 1)
    out, seen = [], set()
    for p in range(1, SMALL_P_MAX + 1):
        for Q in range(p + 1):
            ds = Q * ((SMALL_D << SMALL_SHIFT) - R)
            for delta in deltas(ds):
                t = Q * R + delta
                if not 0 <= t <= p * (R - 1) + (R - 1):
                    continue
                a = min(R - 1, t // p)
                c = t - a * p
                if 0 <= c < R and (p, Q, a, c) not in seen:  # d* = 0 at Q = 0: its neighbours repeat those of 0
                    seen.add((p, Q, a, c))
                    out.append((p, Q, a, c))
    return out


def small_boundary_deltas(ds):
    """the subset the deeper Horner chains use: either side of a multiple of r and of the estimate's switch"""
    return (-1, 0, ds - 1, ds)


# ------------------------------------------------------------------------------------------------ FrWide
def wide_columns(a, b, n_terms):
    """the accumulator state after n_terms identical terms a * b: N * sum_{i + j = k} A_i B_j, k = 0..14"""
    A, B = _limbs32(a), _limbs32(b)
    return [n_terms * sum(A[i] * B[k - i] for i in range(8) if 0 <= k - i < 8) for k in range(15)]


def wide_n_columns(a, b):
    """the largest N for which every column of wide_columns(a, b, N) stays below 2^96 (2^96 - 1 where every column is 0)"""
    top = max(wide_columns(a, b, 1))
    return (WIDE_COLUMN_BOUND - 1) // top if top else WIDE_COLUMN_BOUND - 1


def wide_n_max(a, b):
    """the largest N that fr_wide_reduce takes: every column TOGETHER WITH THE CARRY THAT REACHES IT below 2^96, which is what
    keeps the running carry of its chain in 64 bits.  Column k plus its carry is floor(N S_k / 2^(32 k)) with S_k the value of
    columns 0..k, so N S_k < 2^(96 + 32 k).  At most wide_n_columns(a, b), and short of it by a few units for some operands."""
    cols = wide_columns(a, b, 1)
    n, s = WIDE_COLUMN_BOUND - 1, 0
    for k in range(15):
        s += cols[k] << (32 * k)
        if s:
            n = min(n, ((WIDE_COLUMN_BOUND << (32 * k)) - 1) // s)
    return n


def wide_value(columns):
    return sum(c << (32 * k) for k, c in enumerate(columns))


def wide_reduce_model(columns):
    """the carry chain of fr_wide_reduce into t[0..17] and its three-part reduction -> T / R mod r"""
    assert len(columns) == 15 and all(0 <= c < WIDE_COLUMN_BOUND for c in columns)
    t, carry = [0] * 18, 0
    for k in range(15):
        lo, hi = columns[k] & ((1 << 64) - 1), columns[k] >> 64
        s = lo + carry
        h = hi + (s >> 64)
        s &= (1 << 64) - 1
        t[k] = s & M32
        carry = (s >> 32) | (h << 32)
        assert carry < 1 << 64  # the kernel's running carry is a uint64_t (and its h a uint32_t): column + carry < 2^96
    t[15], t[16], t[17] = carry & M32, (carry >> 32) & M32, carry >> 64
    assert t[17] == 0 and sum(w << (32 * i) for i, w in enumerate(t)) == wide_value(columns)
    t0 = sum(t[i] << (32 * i) for i in range(8))
    t1 = sum(t[8 + i] << (32 * i) for i in range(8))
    t2 = t[16] | (t[17] << 32)
    from_mont = lambda x: x * RINV % R  # of any x < 2^256: the Montgomery product with 1, then one subtraction
    to_mont = lambda x: x * MONT % R
    return (from_mont(t0) + to_mont(from_mont(t1)) + to_mont(t2)) % R


def wide_columns_of_words(t0, t1):
    """a hand-made state whose words T0 and T1 are the given values below 2^256: columns 0..7 carry T0's limbs, 8..14 T1's
    (its top limb rides in bits 32..63 of column 14)"""
    assert 0 <= t0 < MONT and 0 <= t1 < MONT
    A, B = _limbs32(t0), _limbs32(t1)
    return A + B[:6] + [B[6] | (B[7] << 32)]


WIDE_N = (1, 27, 28, 1 << 16, 1 << 29)  # and wide_n_max(a, b); T2 is non-zero from 28 worst-case terms: 28 (r - 1)^2 >= 2^512
WIDE_WORDS = (R, 2 * R, 3 * R, 4 * R, 5 * R, MONT - 1)  # 2^256 // r = 5: every multiple of r a 256-bit word can hold


# ------------------------------------------------------------------------------------------------ raw residues on the device
def to_raw(xs):
    """integers below 2^256 -> uint64[n, 4], the in-memory layout of an FR vector, WITHOUT the Montgomery conversion: the device
    then multiplies exactly these words (Vec.from_numpy)"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).copy()


def from_raw(arr):
    """uint64[n, 4] (Vec.to_numpy) -> the 256-bit integers as stored: a canonical output is its residue, nothing is reduced"""
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(arr))]
