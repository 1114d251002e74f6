"""Plain-Python restatement of the read-write memory proof (co-zkvms_amd/rw_proof.py, csrc/host/rw_memory_proof.hpp,
csrc/rw_memory_leaves.hip), shared by tests/test_rw_proof_model.py (CPU) and the GPU tests:

  * `rw_leaves` / `if_leaves`: the 2 n_slots + 2 grand-product circuits in the layout of cozk_rw_memory_leaves and
    cozk_rw_memory_init_final_leaves, h(a, v, t) = a + v g + t g^2 - tau (rw_witness_ref.fingerprint), from big-int arithmetic;
    `multiset_holds` is the identity hash[init] * prod hash[write_s] == prod hash[read_s] * hash[final].
  * `leaf_word_model`: the word arithmetic of the exact-sum kernels (rl_term, rl_reduce): the leaf as an exact 9-limb integer sum of
    32 x 256-bit products reduced by a short Barrett quotient, with the carry and quotient bounds the kernel's comment claims as
    asserts.  Expected VALUES in the tests come from big-int arithmetic, never from the model.
  * `prove` / `verify`: the whole proof -- prover with its coordinator under one transcript, the proof bytes, the plain verifier with
    the harness's reasons -- from oracle/pyflow.py, oracle/pyharness.py and tests/ts_proof_ref.py.  jolt-core is not in the reference
    tree: this file and the harness's verifier are what pins the protocol (parity unpinned)."""
import pyref as O
import rw_witness_ref as W
import ts_proof_ref as TP
import ts_range_ref as TR

R = O.R
MONT = 1 << 256
M32 = (1 << 32) - 1
RL_LIMBS = 9
RL_MU = (1 << 288) // R
LABEL = b"cozk-rw-memory"
REASON_MULTISET = "multiset equality"
REASON_GP = "grand product"
REASON_LEAF = "leaf claim"
REASON_TS = "timestamp: "
REASON_OPENING = "opening"

h = W.fingerprint


def rw_leaves(addr, v_read, t_read, v_written, g, tau):
    """columns per slot (v_written[s] None: the slot only reads) -> 2 n_slots lists of n leaves"""
    out = []
    for s in range(len(addr)):
        n = len(addr[s])
        w = v_written[s] if v_written[s] is not None else v_read[s]
        out.append([h(addr[s][j], v_read[s][j], t_read[s][j], g, tau) for j in range(n)])
        out.append([h(addr[s][j], w[j], j, g, tau) for j in range(n)])
    return out


def if_leaves(v_init, v_final, t_final, g, tau):
    return [[h(a, v_init[a], 0, g, tau) for a in range(len(v_init))], [h(a, v_final[a], t_final[a], g, tau) for a in range(len(v_init))]]


def multiset_holds(rw_hashes, if_hashes):
    lhs, rhs = if_hashes[0], if_hashes[1]
    for s in range(len(rw_hashes) // 2):
        lhs, rhs = lhs * rw_hashes[2 * s + 1] % R, rhs * rw_hashes[2 * s] % R
    return lhs == rhs


# ------------------------------------------------------------------------------------------------ rw_memory_leaves.hip, exact form
def _limbs32(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def _term(acc, coeff, v):
    """rl_term: acc += coeff * v on 32-bit words, the carry walked into limb 8"""
    assert 0 <= coeff < MONT and 0 <= v <= M32
    c, carry = _limbs32(coeff, 8), 0
    for k in range(8):
        t = c[k] * v + acc[k] + carry
        assert t < 1 << 64  # (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        acc[k], carry = t & M32, t >> 32
    acc[8] += carry
    assert acc[8] <= M32  # the sum stays below 2^288


def _reduce(acc):
    """rl_reduce: S mod r by qh = floor(floor(S / 2^253) MU / 2^35), q - 2 <= qh <= q, then T = S - qh r on 8 limbs and two
    conditional subtractions"""
    S = sum(w << (32 * i) for i, w in enumerate(acc))
    assert S < 3 << (32 + 254) and S < 1 << 288
    s1 = (acc[8] << 3) | (acc[7] >> 29)
    assert s1 == S >> 253 and s1 < 1 << 35 and RL_MU < 1 << 35
    prod = s1 * RL_MU
    hi, lo = prod >> 64, prod & ((1 << 64) - 1)  # __umul64hi and the low product
    assert hi < 1 << 6
    q = ((hi << 29) | (lo >> 35)) & ((1 << 64) - 1)
    assert q == prod >> 35 and S // R - 2 <= q <= S // R
    q_lo, q_hi = q & M32, q >> 32
    assert q_hi < 8
    m = _limbs32(R, 8)
    p, carry = [0] * 8, 0
    for k in range(8):
        t = m[k] * q_lo + carry
        assert t < 1 << 64
        p[k], carry = t & M32, t >> 32
    carry = 0
    for k in range(1, 8):
        t = m[k - 1] * q_hi + p[k] + carry
        assert t < 1 << 64
        p[k], carry = t & M32, t >> 32
    assert sum(w << (32 * i) for i, w in enumerate(p)) == q * R % MONT
    d, borrow = [0] * 8, 0
    for k in range(8):
        t = acc[k] - p[k] - borrow
        d[k], borrow = t & M32, 1 if t < 0 else 0
    T = sum(w << (32 * i) for i, w in enumerate(d))
    assert T == S - q * R and 0 <= T < 3 * R < MONT
    for _ in range(2):  # reduce_once twice
        if T >= R:
            T -= R
    assert T < R
    return T


def leaf_word_model(a, v, t, g, tau):
    """the 256-bit word the exact-sum kernels store for h(a, v, t): Montgomery form of the leaf"""
    one, g1, g2, c = MONT % R, g * MONT % R, g * g % R * MONT % R, (R - tau) % R * MONT % R
    acc = _limbs32(c, 8) + [0]
    _term(acc, one, a)
    _term(acc, g1, v)
    _term(acc, g2, t)
    return _reduce(acc)


def mont(x):
    return x % R * MONT % R


# ------------------------------------------------------------------------------------------------ the whole proof
def default_cfg(**kw):
    cfg = dict(log_n=3, log_mem=5, n_slots=4, seed=1, with_ts=1, tamper=0)
    cfg.update(kw)
    return cfg


def witness(cfg):
    """the harness's trace restricted to the first n_slots slots and its witness columns, tampers 1 and 3 applied"""
    N, MEM, ns = 1 << cfg["log_n"], 1 << cfg["log_mem"], cfg["n_slots"]
    addr, vw, iw, vi = W.jolt_instance(cfg["seed"], N, MEM, store_pct=30, n_regs=32)
    addr, vw, iw = addr[:ns], vw[:ns], iw[:ns]
    v_read, t_read, v_written, v_final, t_final = W.replay(addr, vw, iw, vi)
    # the word a writing slot leaves behind: rd writes every step (its v_write), ram where flagged
    v_written = [v_written[s] if v_written[s] is not None else vw[s] for s in range(ns)]
    wit = dict(addr=addr, v_read=v_read, t_read=t_read, v_written=v_written, v_init=vi, v_final=v_final, t_final=t_final)
    if cfg["with_ts"]:
        wit["rc_rt"], wit["rc_gmr"], wit["fc_rt"], wit["fc_gmr"] = TR.ts_range(t_read, N)
    if cfg["tamper"] == 1:
        wit["v_read"] = [list(c) for c in v_read]
        wit["v_read"][ns - 1][N // 2] = (wit["v_read"][ns - 1][N // 2] + 1) & M32  # a U32 word: 0xFFFFFFFF wraps to 0, as on the device
    if cfg["tamper"] == 3:
        wit["fc_rt"] = [list(c) for c in wit["fc_rt"]]
        wit["fc_rt"][0][t_read[0][N // 2]] += 1
    return wit


def _bits(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def _open(cols, point, tr, tamper_claim=False):
    """compact_open_worker + receive_claims: -> (claims, the opening for the accumulator)"""
    import pyspartan_outer as S
    eq = O.eq_evals(point)
    claims = [sum(a * b for a, b in zip(c, eq)) % R for c in cols]
    if tamper_claim:
        claims[0] = (claims[0] + 1) % R
    claims, rho, batched = S.receive_claims([claims], tr)
    joint, pw = [0] * len(cols[0]), 1
    for c in cols:
        for i, v in enumerate(c):
            joint[i] = (joint[i] + v * pw) % R
        pw = pw * rho % R
    return claims, {"poly": joint, "eq": list(eq), "point": list(point), "claim": batched}


def prove(cfg):
    """-> dict(proof_bytes, commitments, rw_hashes, if_hashes, rw_gp, if_gp, rw_claims, if_claims, [ts_hashes, ts_gp, ts_claims],
    reduced, reduced_claims, joint_proofs)"""
    import pyflow as F
    import pyharness as H
    cfg = default_cfg(**cfg)
    ns, N, MEM = cfg["n_slots"], 1 << cfg["log_n"], 1 << cfg["log_mem"]
    nv = max(cfg["log_n"], cfg["log_mem"])
    wit = witness(cfg)
    writers = [wit["v_written"][s] for s in range(ns) if s >= 2]
    rw_cols = wit["addr"] + wit["v_read"] + writers + wit["t_read"]
    if_cols = [wit["v_final"], wit["t_final"]]
    ts_fams = wit["rc_rt"] + wit["rc_gmr"] + wit["fc_rt"] + wit["fc_gmr"] if cfg["with_ts"] else []
    ck = H._pst_setup(cfg["seed"], nv)
    tr = O.Transcript(LABEL)
    # 1. commit
    committed = rw_cols + if_cols + ts_fams
    commitments = [H._commit(ck, c) for c in committed]
    for c in commitments:
        tr.append_point(c)
    out = O.ser_u64(len(committed)) + b"".join(O.ser_u64(_bits(len(col))) + O.ser_g1(c) for col, c in zip(committed, commitments))
    # 2. gamma, tau, leaves
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    w = [wit["v_written"][s] if s >= 2 else None for s in range(ns)]
    rwl = [x for c in rw_leaves(wit["addr"], wit["v_read"], wit["t_read"], w, g, tau) for x in c]
    ifl = [x for c in if_leaves(wit["v_init"], wit["v_final"], wit["t_final"], g, tau) for x in c]
    # 3. the two grand products
    rw_layers, rw_hashes = F.dense_gp([rwl], 2 * ns, tr)
    if_layers, if_hashes = F.dense_gp([ifl], 2, tr)
    tr.append_scalars(rw_hashes)
    tr.append_scalars(if_hashes)
    rw_gp, r_rw = O.gp_prove(rw_layers, tr)
    if_gp, r_if = O.gp_prove(if_layers, tr)
    # 4. two openings
    openings = []
    rw_claims, op = _open(rw_cols, r_rw[_bits(2 * ns):], tr, cfg["tamper"] == 2)
    openings.append(op)
    if_claims, op = _open(if_cols, r_if[1:], tr)
    openings.append(op)
    out += O.ser_vec_fr(rw_hashes) + O.ser_vec_fr(if_hashes) + F.ser_gp(rw_gp) + F.ser_gp(if_gp) + O.ser_vec_fr(rw_claims) + O.ser_vec_fr(if_claims)
    res = {"commitments": commitments, "rw_hashes": rw_hashes, "if_hashes": if_hashes, "rw_gp": rw_gp, "if_gp": if_gp, "rw_claims": rw_claims, "if_claims": if_claims}
    # 5. the timestamp range check under the same transcript
    if cfg["with_ts"]:
        tg, ttau = tr.challenge_scalar(), tr.challenge_scalar()
        circuits = 6 * ns + 1
        leaves = [x for c in TP.range_leaves(wit["t_read"], wit["rc_rt"], wit["rc_gmr"], wit["fc_rt"], wit["fc_gmr"], tg, ttau) for x in c]
        layers, hashes = F.dense_gp([leaves], circuits, tr)
        tr.append_scalars(hashes)
        gp, r = O.gp_prove(layers, tr)
        ts_claims, op = _open(ts_fams + wit["t_read"], r[_bits(circuits):], tr)
        openings.append(op)
        out += O.ser_vec_fr(hashes) + F.ser_gp(gp) + O.ser_vec_fr(ts_claims)
        res.update(ts_hashes=hashes, ts_gp=gp, ts_claims=ts_claims)
    # 6. ONE reduce_and_prove
    r_red, red_claims, red = O.opening_reduce([openings], tr)
    gamma = tr.challenge_scalar()
    joint, pw = [0] * (1 << nv), 1
    for op in openings:
        for i, v in enumerate(op["poly"]):
            joint[i] = (joint[i] + v * pw) % R
        pw = pw * gamma % R
    proofs, _ = O.pst_open(ck, joint, list(reversed(r_red)))
    out += O.ser_u64(len(red["round_polys"])) + b"".join(O.ser_vec_fr(c) for c in red["round_polys"]) + O.ser_vec_fr(red_claims)
    out += O.ser_u64(len(proofs)) + b"".join(O.ser_g1(p) for p in proofs)
    res.update(proof_bytes=out, reduced=red, reduced_claims=red_claims, joint_proofs=proofs)
    return res


def _iota(point):
    acc = 0
    for rj in point:
        acc = (2 * acc + rj) % R
    return acc


def _batch_eval(values, hi):
    return sum(e * v for e, v in zip(O.eq_evals(hi), values + [0] * ((1 << len(hi)) - len(values)))) % R


def verify(proof, cfg):
    """the plain verifier: replays the transcript and runs every check -> (ok, reason of the first that fails or None, {check: bool});
    a check after a failed grand product cannot be replayed and counts as failed.  The timestamp reasons are prefixed."""
    import pyharness as H
    cfg = default_cfg(**cfg)
    ns, with_ts = cfg["n_slots"], cfg["with_ts"]
    nw = max(0, ns - 2)
    n_rw = 3 * ns + nw
    ix = dict(addr=0, v_read=ns, v_written=2 * ns, t_read=2 * ns + nw, v_final=n_rw, t_final=n_rw + 1, rc_rt=n_rw + 2)
    nv = max(cfg["log_n"], cfg["log_mem"])
    ck = H._pst_setup(cfg["seed"], nv)
    tr = O.Transcript(LABEL)
    order = [REASON_MULTISET, REASON_GP, REASON_LEAF]
    if with_ts:
        order += [REASON_TS + k for k in (TP.REASON_MULTISET, TP.REASON_GP, TP.REASON_LEAF)]
    order.append(REASON_OPENING)
    checks = {k: False for k in order}

    def result():
        first = next((k for k in order if not checks[k]), None)
        return first is None, first, checks
    assert len(proof["commitments"]) == n_rw + 2 + (4 * ns if with_ts else 0)
    assert len(proof["rw_hashes"]) == 2 * ns and len(proof["if_hashes"]) == 2 and len(proof["rw_claims"]) == n_rw and len(proof["if_claims"]) == 2
    for c in proof["commitments"]:
        tr.append_point(c)
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    tr.append_scalars(proof["rw_hashes"])
    tr.append_scalars(proof["if_hashes"])
    checks[REASON_MULTISET] = multiset_holds(proof["rw_hashes"], proof["if_hashes"])
    if proof["rw_gp"]["outputs"] != proof["rw_hashes"] or proof["if_gp"]["outputs"] != proof["if_hashes"]:
        return result()
    out_rw = O.gp_verify(proof["rw_gp"], 2 * ns, tr)
    out_if = O.gp_verify(proof["if_gp"], 2, tr) if out_rw is not None else None
    if out_rw is None or out_if is None:
        return result()
    checks[REASON_GP] = True
    (rw_claim, r_rw), (if_claim, r_if) = out_rw, out_if
    k = _bits(2 * ns)
    hi, lo, hi2, lo2 = r_rw[:k], r_rw[k:], r_if[:1], r_if[1:]
    opens = [dict(point=lo, polys=list(range(n_rw)), claims=proof["rw_claims"], rho=tr.challenge_scalar())]
    opens.append(dict(point=lo2, polys=[ix["v_final"], ix["t_final"]], claims=proof["if_claims"], rho=tr.challenge_scalar()))
    cl = proof["rw_claims"]
    step, leaves = _iota(lo), []
    for s in range(ns):
        w = cl[ix["v_written"] + s - 2] if s >= 2 else cl[ix["v_read"] + s]
        leaves.append(h(cl[ix["addr"] + s], cl[ix["v_read"] + s], cl[ix["t_read"] + s], g, tau))
        leaves.append(h(cl[ix["addr"] + s], w, step, g, tau))
    v_init = W.jolt_instance(cfg["seed"], 1 << cfg["log_n"], 1 << cfg["log_mem"], store_pct=30, n_regs=32)[3]  # public preprocessing
    io = _iota(lo2)
    init = h(io, sum(a * b for a, b in zip(v_init, O.eq_evals(lo2))) % R, 0, g, tau)
    fin = h(io, proof["if_claims"][0], proof["if_claims"][1], g, tau)
    checks[REASON_LEAF] = _batch_eval(leaves, hi) == rw_claim and _batch_eval([init, fin], hi2) == if_claim
    if with_ts:
        circuits = 6 * ns + 1
        assert len(proof["ts_hashes"]) == circuits and len(proof["ts_claims"]) == 5 * ns
        tg, ttau = tr.challenge_scalar(), tr.challenge_scalar()
        tr.append_scalars(proof["ts_hashes"])
        checks[REASON_TS + TP.REASON_MULTISET] = TP.multiset_holds(proof["ts_hashes"], ns)
        out = O.gp_verify(proof["ts_gp"], circuits, tr) if proof["ts_gp"]["outputs"] == proof["ts_hashes"] else None
        if out is None:
            return result()
        checks[REASON_TS + TP.REASON_GP] = True
        claim, r = out
        kk = _bits(circuits)
        lv = TP.leaf_values(proof["ts_claims"], ns, _iota(r[kk:]), tg, ttau)
        checks[REASON_TS + TP.REASON_LEAF] = _batch_eval(lv, r[:kk]) == claim
        polys = [ix["rc_rt"] + i for i in range(4 * ns)] + [ix["t_read"] + s for s in range(ns)]  # t_read: the step-1 commitments
        opens.append(dict(point=r[kk:], polys=polys, claims=proof["ts_claims"], rho=tr.challenge_scalar()))
    # the reduced opening: the reduction sumcheck over all openings, then one PST13 check with the trapdoor
    pws, batched = [], []
    for o in opens:
        pw = [1]
        for _ in range(1, len(o["claims"])):
            pw.append(pw[-1] * o["rho"] % R)
        pws.append(pw)
        batched.append(sum(p * c for p, c in zip(pw, o["claims"])) % R)
    rho2 = tr.challenge_scalar()
    coeffs = [1]
    for _ in range(1, len(opens)):
        coeffs.append(coeffs[-1] * rho2 % R)
    e = sum(c * b * (1 << (nv - len(o["point"]))) for c, b, o in zip(coeffs, batched, opens)) % R
    rs, ok = [], len(proof["reduced"]["round_polys"]) == nv and len(proof["reduced_claims"]) == len(opens)
    for comp in proof["reduced"]["round_polys"] if ok else []:
        poly = [comp[0], (e - 2 * comp[0] - sum(comp[1:])) % R] + list(comp[1:])
        tr.append_scalars(comp)
        rj = tr.challenge_scalar()
        rs.append(rj)
        e = O.unipoly_eval(poly, rj)
    if ok:
        expect = 0
        for c, o, rc in zip(coeffs, opens, proof["reduced_claims"]):
            eqv = 1
            for a, b in zip(o["point"], rs[nv - len(o["point"]):]):
                eqv = eqv * ((a * b + (1 - a) * (1 - b)) % R) % R
            expect = (expect + c * eqv * rc) % R
        ok = expect == e
    if ok:
        tr.append_scalars(proof["reduced_claims"])
        gamma = tr.challenge_scalar()
        scal, gp, joint_claim = [0] * len(proof["commitments"]), 1, 0
        for o, pw, rc in zip(opens, pws, proof["reduced_claims"]):
            for idx, p in zip(o["polys"], pw):
                scal[idx] = (scal[idx] + gp * p) % R
            sc = 1
            for j in range(nv - len(o["point"])):
                sc = sc * (1 - rs[j]) % R
            joint_claim = (joint_claim + gp * sc * rc) % R
            gp = gp * gamma % R
        joint_c = None
        for c, sc in zip(proof["commitments"], scal):
            if sc:
                joint_c = O.g1_add(joint_c, O.g1_mul(c, sc))
        ok = O.pst_check_with_trapdoor(ck, joint_c, list(reversed(rs)), joint_claim, proof["joint_proofs"])
    checks[REASON_OPENING] = ok
    return result()
