"""Big-int restatement of the reference's Shamir sharing (mpc-types/src/protocols/shamir.rs), the yardstick of
tests/test_shamir_host.py and tests/test_gpu_shamir.py.  Values are canonical integers mod r; party p (0-based) evaluates
at x = p + 1.  Coefficients of the engine's dealing are PRF streams: coef_c[i] = prf_fr(keys[c - 1], counter + i)."""
import pyref as O

R = O.R


def evaluate_poly(poly, x):
    """shamir.rs:166-175 -- Horner from the leading coefficient"""
    it = reversed(poly)
    ev = next(it)
    for c in it:
        ev = (ev * x + c) % R
    return ev


def share(coeffs, num_shares):
    """shamir.rs:190-207 with the coefficients given (coeffs[0] = the secret): evaluations at x = 1..=num_shares"""
    return [evaluate_poly(coeffs, i) for i in range(1, num_shares + 1)]


def eval_vec(coeff_vecs, num_parties):
    """cozk_shamir_eval_vec: coeff_vecs[c][i] is coefficient c of element i; returns shares[p][i]"""
    n = len(coeff_vecs[0])
    per_elem = [share([cv[i] for cv in coeff_vecs], num_parties) for i in range(n)]
    return [[per_elem[i][p] for i in range(n)] for p in range(num_parties)]


def prf_coeffs(keys, degree, counter, n):
    assert len(keys) == degree
    return [O.prf_fr_vec(keys[c], counter, n) for c in range(degree)]


def share_vec(v, keys, degree, num_parties, counter=0):
    """cozk_shamir_share_vec (share_field_elements, shamir.rs:58-77, with PRF coefficients): shares[p][i]"""
    return eval_vec([list(v)] + prf_coeffs(keys, degree, counter, len(v)), num_parties)


def lagrange_from_coeff(points):
    """shamir.rs:273-291"""
    res = []
    for i in points:
        num, den = 1, 1
        for j in points:
            if i != j:
                num = num * j % R
                den = den * (j - i) % R
        res.append(num * pow(den, -1, R) % R)
    return res


def reconstruct(shares, lagrange):
    """shamir.rs:314-322"""
    assert len(shares) == len(lagrange)
    return sum(s * l for s, l in zip(shares, lagrange)) % R


def combine_vec(share_vecs, points, degree):
    """combine_field_elements (shamir.rs:80-124): only the first degree + 1 shares / points are used"""
    assert len(share_vecs) == len(points) and len(share_vecs) > degree
    lam = lagrange_from_coeff(points[:degree + 1])
    n = len(share_vecs[0])
    return [reconstruct([share_vecs[j][i] for j in range(degree + 1)], lam) for i in range(n)]


def keys_for(seed, degree):
    return [O.harness_prf_key(seed, c) for c in range(degree)]
