"""Big-int restatement of co-jolt's Spartan worker proved by n Shamir parties (cozk_shamir_jolt_spartan_*,
csrc/host/shamir_jolt_spartan.hpp), on top of oracle/pyspartan_outer.py (the instance, Gruen split-eq, the cubic from its hint, the
inner matrix, eq_plus_one, the serialisation), oracle/pyjolt_r1cs.py, tests/shamir_ref.py and the mask derivation of
tests/shamir_gp_ref.py.  The reference has no Shamir prover, so this file IS the statement the device code is held to.

t = degree, n = parties, party p evaluates at p + 1; 1 <= t, 2t + 1 <= n.  Every step of the worker is linear in the witness share or
multiplies exactly two secret factors, so a party runs the plain prover's steps on its degree-t shares of the columns:

  witness     public columns stay public; shared column v: shamir_ref.share_vec(col_v, share keys, t, n, share_counter + v num_steps),
              share key c = harness key (seed ^ 0x53484152, c)
  Az, Bz, Cz  DENSE, per party, row by row from its columns: a constant or a public column is added to EVERY party's value (the constant
              sharing), so Az_p, Bz_p, Cz_p are degree-t sharings.  Cz is evaluated from its own linear combination: on shares
              Cz_p != Az_p Bz_p.
  masks       M = 4 (steps_bits + constr_bits) openings of degree 2t: shamir_gp_ref.zero_masks(rand keys, t, M, rand_counter); party p's
              rand key j = harness key (seed ^ 0x52414E44, 64 p + j), j <= 3t
  outer       sender p <= 2t: t(0)_p = sum e (Az_p Bz_p - Cz_p) (0 in the first round, for every party), t(inf)_p = sum e dAz_p dBz_p, the
              cubic from (t(0)_p, t(inf)_p, the PUBLIC running claim as hint); coefficient i + zero_p[4 round + i] is opened with
              lagrange(1..2t + 1).  Az, Bz, Cz(r) from parties 0..t with lagrange(1..t + 1), unmasked.
  inner       parties 0..t: bind_z / bind_shift_z from their columns (the constant column is 1 at every party), the quadratic against the
              public ABC with the public running claim; each of the 3 coefficients opened with lagrange(1..t + 1)
  shift       z_ry_p = sum_i eq_ry[i] col_p,i; shift_claim opened from parties 0..t (not appended to the transcript); the rounds with the
              public running claim, opened from parties 0..t
  claims      col_p,i(rx_step), col_p,i(shift_r) per party 0..t, every column opened with lagrange(1..t + 1)
  transcript  and proof: those of pyspartan_outer.run_full(mode = plain)"""
import hashlib

import pyjolt_r1cs as J
import pyref as O
import pyspartan_outer as SO
import shamir_gp_ref as G
import shamir_ref as S

R = O.R
SHARE_TAG, RAND_TAG = 0x53484152, 0x52414E44


def share_keys(seed, degree):
    return [O.harness_prf_key(seed ^ SHARE_TAG, c) for c in range(degree)]


def rand_keys(seed, num_parties, degree):
    return [[O.harness_prf_key(seed ^ RAND_TAG, 64 * p + j) for j in range(3 * degree + 1)] for p in range(num_parties)]


def instance(system, seed, log_steps):
    """the outer harness's own instance -> (uniform, cross, padded, clear columns, is_public)"""
    n = 1 << log_steps
    if system == "jolt":
        uniform, cross, padded = J.build_system()
        return uniform, cross, padded, J.synthetic_columns(seed, n), list(J.IS_PUBLIC)
    uniform, cross, padded = SO.synthetic_system()
    return uniform, cross, padded, SO.synthetic_columns(seed, n), list(SO.IS_PUBLIC)


def num_openings(system, log_steps):
    padded = 128 if system == "jolt" else 8
    return 4 * (log_steps + padded.bit_length() - 1)


def finals_len(system, log_steps):
    """values in `finals` (each of t + 1 shares), in proof order"""
    nvars = 78 if system == "jolt" else 14
    V = 1
    while V < nvars:
        V <<= 1
    return 3 + 3 * ((4 * V).bit_length() - 1) + 1 + 3 * log_steps + 2 * nvars


def party_columns(cols, is_public, seed, num_parties, degree, share_counter):
    """out[p][v]: party p's column v (the clear column where it is public)"""
    n = len(cols[0])
    keys = share_keys(seed, degree)
    out = [[None] * len(cols) for _ in range(num_parties)]
    for v, col in enumerate(cols):
        sh = [col] * num_parties if is_public[v] else S.share_vec(col, keys, degree, num_parties, counter=share_counter + v * n)
        for p in range(num_parties):
            out[p][v] = sh[p]
    return out


def _lc(lc, cols, row):
    """a linear combination on one party's columns: constants (and public columns, which hold the clear value) enter as they are"""
    return sum(c if v is None else c * cols[v][row] for v, c in lc) % R


def _offset_lc(olc, cols, step, num_steps):
    off, lc = olc
    if not off:
        return _lc(lc, cols, step)
    if step + 1 < num_steps:
        return _lc(lc, cols, step + 1)
    return SO.lc_constant(lc)  # the last step: the constant alone


def dense_azbzcz(uniform, cross, padded, cols, num_steps):
    """one party's dense Az, Bz, Cz (row = step * padded + constraint), as k_r1cs_rows builds them in PLAIN mode"""
    L = num_steps * padded
    az, bz, cz = [0] * L, [0] * L, [0] * L
    for step in range(num_steps):
        for ci, (a, b, c) in enumerate(uniform):
            row = step * padded + ci
            az[row], bz[row], cz[row] = _lc(a, cols, step), _lc(b, cols, step), _lc(c, cols, step)
        for ci, (a, b, cond) in enumerate(cross):
            row = step * padded + len(uniform) + ci
            az[row] = (_offset_lc(a, cols, step, num_steps) - _offset_lc(b, cols, step, num_steps)) % R
            bz[row] = _offset_lc(cond, cols, step, num_steps)
    return az, bz, cz


def _quadratic(az, bz, cz, eq, first):
    E_in, E_out = eq.E_in_current(), eq.E_out_current()
    nbits = len(E_in).bit_length() - 1
    mask = (1 << nbits) - 1
    t0 = tinf = 0
    for k in range(len(az) // 2):
        a0, a1, b0, b1 = az[2 * k], az[2 * k + 1], bz[2 * k], bz[2 * k + 1]
        if not (a0 or a1 or b0 or b1 or cz[2 * k]):
            continue
        e = E_out[k >> nbits] * E_in[k & mask] % R
        tinf = (tinf + (a1 - a0) * (b1 - b0) % R * e) % R
        if not first:
            t0 = (t0 + (a0 * b0 - cz[2 * k]) % R * e) % R
    return t0, tinf


def _bind_low(v, r):
    return [(v[2 * k] + r * (v[2 * k + 1] - v[2 * k])) % R for k in range(len(v) // 2)]


def _bind_top(v, r):
    h = len(v) // 2
    return [(v[i] + r * (v[i + h] - v[i])) % R for i in range(h)]


def _evals_0_2(z, pub):
    """sumcheck_evals at 0 and 2, HighToLow, of z x pub"""
    h = len(z) // 2
    e0 = sum(z[i] * pub[i] for i in range(h)) % R
    e2 = sum((2 * z[i + h] - z[i]) * (2 * pub[i + h] - pub[i]) for i in range(h)) % R
    return e0, e2


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def prove(system, log_steps, seed, num_parties, degree, share_counter=0, rand_counter=0, first_senders=None):
    """all parties and the coordinator.  Returns dict(proof_bytes, digest, proof, msgs[m][p <= 2t] (masked), locals[m][p] (before the
    mask), zero[p][m], finals[value][p <= t], outer_polys[round] (the opened cubics)).  first_senders = k opens the outer messages from
    only k senders (a test's probe: k = 2t does not reconstruct them)."""
    t, num_steps = degree, 1 << log_steps
    k2, k1 = 2 * t + 1, t + 1
    assert 1 <= t and k2 <= num_parties and log_steps >= 0
    lam2 = S.lagrange_from_coeff(list(range(1, (first_senders or k2) + 1)))
    lam1 = S.lagrange_from_coeff(list(range(1, k1 + 1)))
    uniform, cross, padded, clear, is_public = instance(system, seed, log_steps)
    nvars = len(clear)
    cols = party_columns(clear, is_public, seed, num_parties, t, share_counter)
    steps_bits, constr_bits = log_steps, padded.bit_length() - 1
    V = 1
    while V < nvars:
        V <<= 1
    finals = []

    def open_t(shares):
        finals.append(list(shares))
        return S.reconstruct(list(shares), lam1)

    tr = O.Transcript(b"cozk-spartan")
    n_tau = steps_bits + constr_bits
    tau = tr.challenge_vector(n_tau)
    zero = G.zero_masks(rand_keys(seed, num_parties, t), t, 4 * n_tau, rand_counter=rand_counter)
    # ---- outer
    abc_p = [dense_azbzcz(uniform, cross, padded, cols[p], num_steps) for p in range(k2)]
    eq = SO.GruenSplitEq(tau)
    claim = 0
    msgs, locs, comps, rs, outer_polys = [], [], [], [], []
    for rnd in range(n_tau):
        sw = eq.current_scalar * eq.w[eq.current_index - 1] % R
        l0, l1 = (eq.current_scalar - sw) % R, (2 * sw - eq.current_scalar) % R
        cubics = []
        for p in range(k2):
            t0, tinf = _quadratic(*abc_p[p], eq, rnd == 0)
            cubics.append(SO.cubic_from_linear_times_quadratic_with_hint(l0, l1, t0, tinf, claim))
        poly = []
        for i in range(4):
            loc = [cubics[p][i] for p in range(k2)]
            msg = [(loc[p] + zero[p][4 * rnd + i]) % R for p in range(k2)]
            locs.append(loc)
            msgs.append(msg)
            poly.append(S.reconstruct(msg[:len(lam2)], lam2))
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_i = tr.challenge_scalar()
        rs.append(r_i)
        comps.append(comp)
        outer_polys.append(poly)
        claim = O.unipoly_eval(poly, r_i)
        eq.bind(r_i)
        abc_p = [tuple(_bind_low(v, r_i) for v in abc_p[p]) for p in range(k2)]
    outer_claims = [open_t([abc_p[p][q][0] for p in range(k1)]) for q in range(3)]
    tr.append_scalars(outer_claims)
    outer_r = list(reversed(rs))
    rx_step, rx_constr = outer_r[:steps_bits], outer_r[steps_bits:]
    rlc = tr.challenge_scalar()
    claim = (outer_claims[0] + rlc * outer_claims[1] + rlc * rlc * outer_claims[2]) % R
    # ---- inner
    eq_step, eqp1_step = SO.eq_plus_one_evals(rx_step)
    abc = SO.matrix_mle_partial(uniform, cross, padded, V, rx_constr, rlc)
    zs = []
    for p in range(k1):
        z = [0] * (4 * V)
        for i in range(nvars):
            z[i] = _dot(cols[p][i], eq_step)
            z[2 * V + i] = _dot(cols[p][i], eqp1_step)
        z[V] = 1
        zs.append(z)
    inner_comps, inner_r = [], []
    for _ in range((4 * V).bit_length() - 1):
        cfs = []
        for p in range(k1):
            e0, e2 = _evals_0_2(zs[p], abc)
            cfs.append(O.unipoly_from_evals([e0, (claim - e0) % R, e2]))
        poly = [open_t([cfs[p][i] for p in range(k1)]) for i in range(3)]
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_j = tr.challenge_scalar()
        inner_comps.append(comp)
        inner_r.append(r_j)
        claim = O.unipoly_eval(poly, r_j)
        abc = _bind_top(abc, r_j)
        zs = [_bind_top(z, r_j) for z in zs]
    # ---- shift
    eq_ry = O.eq_evals(inner_r[1:])
    zry = [[sum(eq_ry[i] * cols[p][i][s] for i in range(nvars)) % R for s in range(num_steps)] for p in range(k1)]
    shift_claim = claim = open_t([_dot(zry[p], eqp1_step) for p in range(k1)])
    pub = list(eqp1_step)
    shift_comps, shift_r = [], []
    for _ in range(steps_bits):
        cfs = []
        for p in range(k1):
            e0, e2 = _evals_0_2(zry[p], pub)
            cfs.append(O.unipoly_from_evals([e0, (claim - e0) % R, e2]))
        poly = [open_t([cfs[p][i] for p in range(k1)]) for i in range(3)]
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_j = tr.challenge_scalar()
        shift_comps.append(comp)
        shift_r.append(r_j)
        claim = O.unipoly_eval(poly, r_j)
        pub = _bind_top(pub, r_j)
        zry = [_bind_top(z, r_j) for z in zry]
    # ---- the two claim exchanges
    evals = []
    for point in (rx_step, shift_r):
        chi = O.eq_evals(point)
        evals.append([open_t([_dot(cols[p][i], chi) for p in range(k1)]) for i in range(nvars)])
        tr.challenge_scalar()  # receive_claims draws rho
    proof = {"outer": {"round_polys": comps, "claims": outer_claims}, "inner_polys": inner_comps, "shift_claim": shift_claim,
             "shift_polys": shift_comps, "witness_evals": evals[0], "shift_witness_evals": evals[1]}
    blob = SO.serialize_full(proof)
    return {"proof_bytes": blob, "digest": hashlib.sha256(blob).hexdigest(), "proof": proof, "msgs": msgs, "locals": locs, "zero": zero,
            "finals": finals, "outer_polys": outer_polys}
