"""Exact references for the opening-seam kernels at lengths where a walk over canonical values costs too much: sums over the RAW
Montgomery residues of device-generated vectors.

A device FR vector stores x~ = x * 2^256 mod r.  A Montgomery product of two residues is x~ y~ / 2^256, a sum of such products is
read back through another 1 / 2^256, so the canonical value of sum_i x_i y_i is (sum_i x~_i y~_i) * RINV^2 mod r with the sum
taken over the plain integers -- one big-int dot product and one reduction, no per-element conversion.  The inputs come from
Vec.random / Vec.to_numpy (reduction_ref.from_raw), never from the kernel under test.

tests/test_opening_ref_model.py checks every function here against oracle/pyref.py's own at small sizes, on the CPU.
Plain Python, no GPU."""
import pyref as O
import reduction_ref as X

R = O.R
MONT = X.MONT
RINV = X.RINV
RINV2 = RINV * RINV % R


def residues(values):
    """canonical values -> the Montgomery residues a device vector stores"""
    return [v % R * MONT % R for v in values]


def values(raw):
    """stored residues -> canonical values"""
    return [x * RINV % R for x in raw]


def open_quadratic_pyref(poly, eq):
    """(eval_0, eval_2) of one opening by the share arithmetic of oracle/pyref.py, term by term (the inner sums of
    O.opening_compute_quadratic): poly is a list of (a, b) shares or of plain values, eq a list of plain values, both CANONICAL"""
    h = len(poly) // 2
    e0 = e2 = 0
    for i in range(h):
        e0 += O.sh_into_additive(O.sh_mul_public(poly[i], eq[i]))
        pb = O.sh_sub(O.sh_add(poly[i + h], poly[i + h]), poly[i])
        e2 += O.sh_into_additive(O.sh_mul_public(pb, (2 * eq[i + h] - eq[i]) % R))
    return e0 % R, e2 % R


def open_quadratic_raw(a, b, eq):
    """the same from RAW residues: a, b (None: a plain polynomial) and eq are lists of stored integers of length 2h.  Rep3:
    TWO_INV (a + b) is the additive share, so the factor is a + b and TWO_INV scales the sum"""
    h = len(a) // 2
    s = a if b is None else [x + y for x, y in zip(a, b)]
    e0 = sum(s[i] * eq[i] for i in range(h))
    e2 = sum((2 * s[i + h] - s[i]) * (2 * eq[i + h] - eq[i]) for i in range(h))
    scale = RINV2 * (O.TWO_INV if b is not None else 1) % R
    return e0 * scale % R, e2 * scale % R


def pst_fold(r, p):
    """one fold of PST13 `open` on canonical values (the loop body of O.pst_open): (q, r') with q[b] = r[2b + 1] - r[2b] and
    r'[b] = r[2b] (1 - p) + r[2b + 1] p"""
    half = len(r) // 2
    q = [(r[2 * b + 1] - r[2 * b]) % R for b in range(half)]
    rn = [(r[2 * b] * (1 - p) + r[2 * b + 1] * p) % R for b in range(half)]
    return q, rn


def indicator(n, index):
    return [1 if i == index else 0 for i in range(n)]


def big_endian_index(bits):
    """the table index of a Boolean point: bits[0] is the MOST significant bit (EqPolynomial::evals)"""
    x = 0
    for b in bits:
        x = 2 * x + b
    return x
