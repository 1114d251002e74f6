"""Big-int restatement of co-noir-spartan proved by n Shamir parties (cozk_shamir_spartan_*, csrc/host/shamir_spartan.hpp), on top of
oracle/pyspartan.py (the instance, the plain prover), pyref's round functions and PST13, tests/shamir_ref.py and the mask derivation of
tests/shamir_gp_ref.py.  The reference has no Shamir prover, so this file IS the statement the device code is held to.

t = degree, n = parties, party p evaluates at p + 1; 1 <= t, 2t + 1 <= n.  Every step of the worker is linear in the witness share or
multiplies at most two secret factors, so a party runs the plain prover's functions on its degree-t share of z:

  witness     shamir_ref.share_vec(z, share keys, t, n, share_counter), share key c = harness key (seed ^ 0x53484152, c)
  zero_round  per sender p <= 2t: (A, B, C) z_p, degree-t sharings of Az, Bz, Cz
  commit      parties 0..t commit to z_p; C = sum lambda_p C_p, lambda = lagrange(1..t + 1)
  masks       M = 4 log_n openings of degree 2t: shamir_gp_ref.zero_masks(rand keys, t, M, rand_counter); party p's rand key j = harness
              key (seed ^ 0x52414E44, 64 p + j), j <= 3t
  sumcheck 1  sender p sends spartan_first_round_evals(za_p, zb_p, zc_p, eq)[e] + zero_p[4 round + e]: a degree-2t share of the plain
              message, opened with lagrange(1..2t + 1); za, zb, zc(rx) from parties 0..t with lagrange(1..t + 1); eq(tau, rx) is public
  sumcheck 2  parties 0..t send spartan_second_round_evals(z_p, A(rx, .), B(rx, .), C(rx, .), abc): degree t, unmasked, as z's final value
  opening     z_p(ry) and pst_open(z_p, ry) per party 0..t, combined with lagrange(1..t + 1)
  transcript  and proof: those of pyspartan.run"""
import hashlib

import pyref as O
import pyspartan as SP
import shamir_gp_ref as G
import shamir_ref as S

R = O.R
SHARE_TAG, RAND_TAG = 0x53484152, 0x52414E44


def share_keys(seed, degree):
    return [O.harness_prf_key(seed ^ SHARE_TAG, c) for c in range(degree)]


def rand_keys(seed, num_parties, degree):
    return [[O.harness_prf_key(seed ^ RAND_TAG, 64 * p + j) for j in range(3 * degree + 1)] for p in range(num_parties)]


def num_openings(log_n):
    return 4 * log_n


def open_shares(shares, lam):
    return S.reconstruct(list(shares), lam)


def combine_points(points, lam):
    acc = None
    for pt, l in zip(points, lam):
        acc = O.g1_add(acc, O.g1_mul(pt, l))
    return acc


def ck_for(seed, nv):
    """the SRS of pyspartan.run"""
    t = O.synthetic_fr(seed ^ 0x7A7A7A7A, nv)
    powers = []
    for i in range(nv):
        ev = [1]
        for tj in t[i:]:
            ev = [e * (1 - tj) % R for e in ev] + [e * tj % R for e in ev]
        powers.append([O.g1_mul(O.G1_GEN, e) for e in ev])
    return {"nv": nv, "t": t, "g": O.G1_GEN, "powers_of_g": powers}


def prove(log_n, seed, num_parties, degree, share_counter=0, rand_counter=0, first_senders=None):
    """all parties and the coordinator.  Returns dict(proof_bytes, digest, msgs[m][p <= 2t] (masked), locals[m][p] (before the mask),
    zero[p][m], finals[value][p <= t], sc1, sc2).  first_senders = k opens the first sumcheck's messages from only k senders (a
    test's probe: k = 2t does not reconstruct them)."""
    nv, n, t = log_n, 1 << log_n, degree
    k2, k1 = 2 * t + 1, t + 1
    assert 1 <= t and k2 <= num_parties and nv >= 1
    lam2 = S.lagrange_from_coeff(list(range(1, (first_senders or k2) + 1)))
    lam1 = S.lagrange_from_coeff(list(range(1, k1 + 1)))
    z, entries = SP.build_instance(seed, nv)
    zs = S.share_vec(z, share_keys(seed, t), t, num_parties, counter=share_counter)
    ck = ck_for(seed, nv)
    finals = []

    def open_t(shares):
        finals.append(list(shares))
        return open_shares(shares, lam1)

    # zero_round
    mats = [[(e[0], e[1], e[k]) for e in entries] for k in (2, 3, 4)]
    za = [O.sparse_matvec(mats[0], zs[p], n) for p in range(k2)]
    zb = [O.sparse_matvec(mats[1], zs[p], n) for p in range(k2)]
    zc = [O.sparse_matvec(mats[2], zs[p], n) for p in range(k2)]
    # commit
    cz = combine_points([O.pst_commit(ck, zs[p]) for p in range(k1)], lam1)
    tr = O.Transcript(b"cozk-spartan")
    tr.append_point(cz)
    tau = tr.challenge_vector(nv)
    # masks
    M = num_openings(nv)
    zero = G.zero_masks(rand_keys(seed, num_parties, t), t, M, rand_counter=rand_counter)
    # first sumcheck
    eq = SP.eq_le(tau)
    msgs, locs, sc1, rx = [], [], [], []
    for j in range(nv):
        evs = [O.spartan_first_round_evals(za[p], zb[p], zc[p], eq) for p in range(k2)]
        ev = []
        for e in range(4):
            loc = [evs[p][e] for p in range(k2)]
            msg = [(loc[p] + zero[p][4 * j + e]) % R for p in range(k2)]
            locs.append(loc)
            msgs.append(msg)
            ev.append(open_shares(msg[:len(lam2)], lam2))
        tr.append_scalars(ev)
        r = tr.challenge_scalar()
        sc1.append(ev)
        rx.append(r)
        za = [SP.fix_low(v, r) for v in za]
        zb = [SP.fix_low(v, r) for v in zb]
        zc = [SP.fix_low(v, r) for v in zc]
        eq = SP.fix_low(eq, r)
    fin1 = [open_t([v[p][0] for p in range(k1)]) for v in (za, zb, zc)] + [eq[0]]
    tr.append_scalars(fin1[:3])
    abc = tr.challenge_vector(3)
    # A(rx, .), B(rx, .), C(rx, .): public
    eq_rx = SP.eq_le(rx)
    arx, brx, crx = [0] * n, [0] * n, [0] * n
    for row, col, a_, b_, c_ in entries:
        arx[col] = (arx[col] + a_ * eq_rx[row]) % R
        brx[col] = (brx[col] + b_ * eq_rx[row]) % R
        crx[col] = (crx[col] + c_ * eq_rx[row]) % R
    # second sumcheck on copies of the openers' shares
    zw = [list(zs[p]) for p in range(k1)]
    sc2, ry = [], []
    for j in range(nv):
        evs = [O.spartan_second_round_evals(zw[p], arx, brx, crx, abc) for p in range(k1)]
        ev = [open_t([evs[p][e] for p in range(k1)]) for e in range(3)]
        tr.append_scalars(ev)
        r = tr.challenge_scalar()
        sc2.append(ev)
        ry.append(r)
        zw = [SP.fix_low(v, r) for v in zw]
        arx, brx, crx = SP.fix_low(arx, r), SP.fix_low(brx, r), SP.fix_low(crx, r)
    fin2 = [open_t([zw[p][0] for p in range(k1)]), arx[0], brx[0], crx[0]]
    # z(ry) and the opening
    z_eval = open_t([O.pst_evaluate_le(zs[p], ry) for p in range(k1)])
    opened = [O.pst_open(ck, zs[p], ry)[0] for p in range(k1)]
    proofs = [combine_points([opened[p][i] for p in range(k1)], lam1) for i in range(nv)]
    blob = SP._ser_u64(nv) + SP._ser_g1(cz)
    blob += SP._ser_u64(len(sc1)) + b"".join(SP._ser_vec(e) for e in sc1) + SP._ser_vec(fin1)
    blob += SP._ser_u64(len(sc2)) + b"".join(SP._ser_vec(e) for e in sc2) + SP._ser_vec(fin2)
    blob += SP._ser_fr(z_eval) + SP._ser_u64(len(proofs)) + b"".join(SP._ser_g1(p) for p in proofs)
    return {"proof_bytes": blob, "digest": hashlib.sha256(blob).hexdigest(), "msgs": msgs, "locals": locs, "zero": zero, "finals": finals,
            "sc1": sc1, "sc2": sc2}
