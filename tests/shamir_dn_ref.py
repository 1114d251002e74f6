"""Big-int restatement of the Shamir multiplication with a king and preprocessed double-random pairs (Damgard-Nielsen,
semi-honest): cozk_shamir_rand_{deal, extract, inproc, vec}, cozk_shamir_mul_mask, cozk_shamir_mul_king_{inproc, vec}, on top of
tests/shamir_ref.py.  The reference has no Shamir network, so this file IS the statement the device code is held to.

t = degree, n = parties, party p evaluates at p + 1; 1 <= t, 2t + 1 <= n.

Offline.  Party p holds 3t + 1 keys: keys[0] gives its secret stream s_p[i] = prf_fr(keys[0], counter + i), keys[1..t] the
coefficients of a degree-t polynomial f_i, keys[t + 1..3t] those of a degree-2t polynomial g_i, f_i(0) = g_i(0) = s_p[i].  It deals
u_{p->q}[i] = f_i(q + 1), w_{p->q}[i] = g_i(q + 1).  Party q computes, for k = 0..n - t - 1,
  rt_q^k[i] = sum_p (p + 1)^k u_{p->q}[i],   r2t_q^k[i] = sum_p (p + 1)^k w_{p->q}[i]:
a linear combination of degree-t (degree-2t) sharings is one, of sum_p (p + 1)^k s_p; the (n - t) x n Vandermonde matrix is
what makes the n - t values unknown to any t parties.

Online, with ONE pair (rt, r2t).  Senders are parties 0..2t:
  1. sender p: m_p[i] = a_p[i] b_p[i] + r2t_p[i]            (values at p + 1 of a degree-2t polynomial with constant term a b + r)
  2. the king: z = sum_{p<=2t} lambda_p m_p, lambda = lagrange_from_coeff(1..2t + 1)                              (z = a b + r)
  3. party q: c_q[i] = z[i] - rt_q[i]                                                    (a degree-t sharing of a b + r - r)"""
import pyref as O
import shamir_ref as S

R = S.R


def senders(degree):
    return 2 * degree + 1


def num_keys(degree):
    return 3 * degree + 1


def party_keys(seed, num_parties, degree):
    """private key blocks of 3t + 1 keys, one per party, all distinct"""
    return [S.keys_for(1000 * seed + p, num_keys(degree)) for p in range(num_parties)]


def rand_deal(keys_p, degree, num_parties, n, counter=0):
    """one party's dealing: (u, w) with u[q][i] = f_i(q + 1), w[q][i] = g_i(q + 1)"""
    assert len(keys_p) == num_keys(degree) and degree >= 1 and num_parties >= senders(degree)
    s = O.prf_fr_vec(keys_p[0], counter, n)
    u = S.eval_vec([s] + S.prf_coeffs(keys_p[1:degree + 1], degree, counter, n), num_parties)
    w = S.eval_vec([s] + S.prf_coeffs(keys_p[degree + 1:], 2 * degree, counter, n), num_parties)
    return u, w


def extract(received, count):
    """the Vandermonde step on one party's received vectors: out[k][i] = sum_j (j + 1)^k received[j][i], k < count"""
    assert 1 <= count <= len(received) - 1
    n = len(received[0])
    pw = [[pow(j + 1, k, R) for j in range(len(received))] for k in range(count)]
    return [[sum(c * v[i] for c, v in zip(pw[k], received)) % R for i in range(n)] for k in range(count)]


def rand(keys_per_party, degree, n, counter=0):
    """all parties: pairs[q][k] = (rt_q^k, r2t_q^k), k < n_parties - degree"""
    num_parties = len(keys_per_party)
    dealt = [rand_deal(keys_per_party[p], degree, num_parties, n, counter) for p in range(num_parties)]
    pairs = []
    for q in range(num_parties):
        rt = extract([dealt[p][0][q] for p in range(num_parties)], num_parties - degree)
        r2t = extract([dealt[p][1][q] for p in range(num_parties)], num_parties - degree)
        pairs.append(list(zip(rt, r2t)))
    return pairs


def secrets(keys_per_party, n, counter=0):
    """s_p[i]: what nobody holds; pair k is a sharing of sum_p (p + 1)^k s_p"""
    return [O.prf_fr_vec(k[0], counter, n) for k in keys_per_party]


def pair_value(keys_per_party, k, n, counter=0):
    s = secrets(keys_per_party, n, counter)
    return [sum(pow(p + 1, k, R) * s[p][i] for p in range(len(s))) % R for i in range(n)]


def mul_mask(a_p, b_p, r2t_p):
    """step 1 for one sender"""
    return [(x * y + m) % R for x, y, m in zip(a_p, b_p, r2t_p)]


def mul_king(a_shares, b_shares, r_t, r_2t, degree, king=0):
    """all parties, one pair: r_t[q], r_2t[p] are the parties' halves; a_shares[p], b_shares[p], r_2t[p] are read for p <= 2t only
    (and may be None above); returns c[q][i].  The king changes who computes, not what"""
    num_parties = len(r_t)
    k = senders(degree)
    assert k <= num_parties and 0 <= king < num_parties
    m = [mul_mask(a_shares[p], b_shares[p], r_2t[p]) for p in range(k)]  # steps 1 and 2: the king now holds m[0..2t]
    z = S.combine_vec(m, list(range(1, k + 1)), 2 * degree)              # step 3
    return [[(zi - ri) % R for zi, ri in zip(z, r_t[q])] for q in range(num_parties)]  # step 4
