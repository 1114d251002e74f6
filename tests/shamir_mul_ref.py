"""Big-int restatement of the Shamir multiplication with degree reduction (cozk_shamir_mul_{deal, inproc, vec}), on top of
tests/shamir_ref.py: the classic one-round resharing (Gennaro-Rabin-Rabin's simplification of BGW).  The reference has no
Shamir network and no degree reduction, so this file IS the statement the device code is held to.

Parties 0..2t are the dealers (the first 2t + 1 evaluation points, the convention of combine_field_elements):
  1. dealer p shares d_p[i] = a_p[i] b_p[i] with degree t, coefficient c of element i being PRF(keys_p[c - 1], counter + i);
  2. party q receives h_{p -> q} from every dealer p;
  3. c_q[i] = sum_p lambda_p h_{p -> q}[i] with lambda = lagrange_from_coeff(1..2t + 1).
a_p b_p are the values at p + 1 of a polynomial of degree 2t whose constant term is a b, so sum_p lambda_p d_p = a b; the sum of
the dealers' fresh degree-t polynomials, weighted by lambda, is a degree-t polynomial with that constant term."""
import shamir_ref as S

R = S.R


def dealers(degree):
    return 2 * degree + 1


def mul_deal(a_p, b_p, keys_p, degree, num_parties, counter=0):
    """step 1 for one dealer: h[q][i], the share of a_p[i] b_p[i] for party q"""
    return S.share_vec([x * y % R for x, y in zip(a_p, b_p)], keys_p, degree, num_parties, counter=counter)


def mul_finish(received, degree):
    """step 3 for one party: received[p] = the vector dealer p sent, p = 0..2t"""
    k = dealers(degree)
    assert len(received) == k
    return S.combine_vec(received, list(range(1, k + 1)), 2 * degree)


def mul(a_shares, b_shares, keys_per_party, degree, counter=0):
    """all parties: a_shares[p], b_shares[p] are party p's share vectors (ignored, and possibly None, for p > 2t), keys_per_party[p]
    its `degree` keys; returns c[q][i]"""
    num_parties = len(a_shares)
    k = dealers(degree)
    assert k <= num_parties
    h = [mul_deal(a_shares[p], b_shares[p], keys_per_party[p], degree, num_parties, counter) for p in range(k)]
    return [mul_finish([h[p][q] for p in range(k)], degree) for q in range(num_parties)]


def party_keys(seed, num_parties, degree):
    """private key blocks, one per party, all distinct"""
    return [S.keys_for(1000 * seed + p, degree) for p in range(num_parties)]
