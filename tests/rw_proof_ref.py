"""Plain-Python restatement of the read-write memory proof (co-zkvms_amd/rw_proof.py, csrc/host/rw_memory_proof.hpp,
csrc/rw_memory_leaves.hip), shared by tests/test_rw_proof_model.py (CPU) and the GPU tests:

  * `rw_leaves` / `if_leaves`: the 2 n_slots + 2 grand-product circuits in the layout of cozk_rw_memory_leaves and
    cozk_rw_memory_init_final_leaves, h(a, v, t) = a + v g + t g^2 - tau (rw_witness_ref.fingerprint), from big-int arithmetic;
    `multiset_holds` is the identity hash[init] * prod hash[write_s] == prod hash[read_s] * hash[final].
  * `leaf_word_model`: the word arithmetic of the exact-sum kernels (rl_term, rl_reduce): the leaf as an exact 9-limb integer sum of
    32 x 256-bit products reduced by a short Barrett quotient, with the carry and quotient bounds the kernel's comment claims as
    asserts.  Expected VALUES in the tests come from big-int arithmetic, never from the model.
  * `prove` / `verify`: the whole proof -- prover with its coordinator under one transcript, the proof bytes, the plain verifier with
    the harness's reasons -- in the two steps of csrc/host/rw_memory_proof.hpp, which tests/memory_proof_ref.py calls as they stand
    around its output check: `prove_memory_check` / `verify_memory_check` (the commit through the two openings) and
    `prove_range_check_and_open` / `verify_range_check_and_open` (the range check of tests/ts_proof_ref.py and the ending), on the
    shared steps of tests/memcheck_ref.py.  jolt-core is not in the reference tree: this file and the harness's verifier are what
    pins the protocol (parity unpinned)."""
import memcheck_ref as MC
import pyref as O
import rw_witness_ref as W
import ts_proof_ref as TP
import ts_range_ref as TR

R = O.R
MONT, M32, mont = MC.MONT, MC.M32, MC.mont
RL_LIMBS = 9
RL_MU = (1 << 288) // R
LABEL = b"cozk-rw-memory"
REASON_MULTISET, REASON_GP, REASON_LEAF, REASON_OPENING = MC.REASON_MULTISET, MC.REASON_GP, MC.REASON_LEAF, MC.REASON_OPENING
REASON_TS = "timestamp: "

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
def _term(acc, coeff, v):
    """rl_term: acc += coeff * v on 32-bit words, the carry walked into limb 8"""
    assert 0 <= coeff < MONT and 0 <= v <= M32
    c, carry = MC.limbs32(coeff, 8), 0
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
    m = MC.limbs32(R, 8)
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
    acc = MC.limbs32(c, 8) + [0]
    _term(acc, one, a)
    _term(acc, g1, v)
    _term(acc, g2, t)
    return _reduce(acc)


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


def slot_index(ns):
    """RwProofIdx: where each committed column sits in the proof's order (v_written: the writing slots 2.. only)"""
    nw = max(0, ns - 2)
    n_rw = 3 * ns + nw
    return dict(n_rw=n_rw, addr=0, v_read=ns, v_written=2 * ns, t_read=2 * ns + nw, v_final=n_rw, t_final=n_rw + 1, rc_rt=n_rw + 2)


def _ts_families(cfg, wit):
    return [wit[k] for k in ("rc_rt", "rc_gmr", "fc_rt", "fc_gmr")] if cfg["with_ts"] else []


def prove_memory_check(cfg, wit, ck, tr):
    """steps 1-4 (rw_proof_memory_check_worker + rw_proof_coordinate_memory_check): the commit, gamma and tau, the leaves, the two grand
    products and the two openings -> (the proof's values so far, its openings, its bytes)"""
    ns = cfg["n_slots"]
    rw_cols = wit["addr"] + wit["v_read"] + wit["v_written"][2:] + wit["t_read"]
    if_cols = [wit["v_final"], wit["t_final"]]
    commitments, out = MC.commit_columns(ck, rw_cols + if_cols + [c for fam in _ts_families(cfg, wit) for c in fam], tr)
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    w = [wit["v_written"][s] if s >= 2 else None for s in range(ns)]
    rwl = [x for c in rw_leaves(wit["addr"], wit["v_read"], wit["t_read"], w, g, tau) for x in c]
    ifl = [x for c in if_leaves(wit["v_init"], wit["v_final"], wit["t_final"], g, tau) for x in c]
    res, r_rw, r_if, part = MC.memory_checking(rwl, 2 * ns, ifl, 2, tr)
    rw_claims, op_rw = MC.open_columns(rw_cols, r_rw, tr, cfg["tamper"] == 2)
    if_claims, op_if = MC.open_columns(if_cols, r_if, tr)
    res.update(commitments=commitments, rw_claims=rw_claims, if_claims=if_claims)
    return res, [op_rw, op_if], out + part + O.ser_vec_fr(rw_claims) + O.ser_vec_fr(if_claims)


def prove_range_check_and_open(cfg, wit, ck, tr, res, openings, out):
    """steps 5 and 6 (rw_proof_range_check_and_open_worker + its coordinator): with with_ts the timestamp range check under the same
    transcript (t_read is not committed again), then ONE reduce_and_prove -> res, completed with proof_bytes"""
    if cfg["with_ts"]:
        hashes, gp, ts_claims, op, part = TP.range_check_prove(wit["t_read"], *_ts_families(cfg, wit), tr)
        openings, out = openings + [op], out + part
        res.update(ts_hashes=hashes, ts_gp=gp, ts_claims=ts_claims)
    ending, part = MC.reduce_and_prove(ck, openings, max(cfg["log_n"], cfg["log_mem"]), tr)
    res.update(ending, proof_bytes=out + part)
    return res


def prove(cfg):
    """-> dict(proof_bytes, commitments, rw_hashes, if_hashes, rw_gp, if_gp, rw_claims, if_claims, [ts_hashes, ts_gp, ts_claims],
    reduced, reduced_claims, joint_proofs)"""
    import pyharness as H
    cfg = default_cfg(**cfg)
    wit = witness(cfg)
    ck = H._pst_setup(cfg["seed"], max(cfg["log_n"], cfg["log_mem"]))
    tr = O.Transcript(LABEL)
    res, openings, out = prove_memory_check(cfg, wit, ck, tr)
    return prove_range_check_and_open(cfg, wit, ck, tr, res, openings, out)


def check_order(with_ts, between=()):
    """the verifier's checks in the order it runs them; `between`: what a caller checks between the memory check and the range check"""
    ts = [REASON_TS + k for k in (TP.REASON_MULTISET, TP.REASON_GP, TP.REASON_LEAF)] if with_ts else []
    return [REASON_MULTISET, REASON_GP, REASON_LEAF] + list(between) + ts + [REASON_OPENING]


def verify_memory_check(proof, cfg, tr, checks):
    """rw_proof_verify_memory_check: sets the first three checks -> its two openings, or None after a failed grand product"""
    ns = cfg["n_slots"]
    ix = slot_index(ns)
    assert len(proof["commitments"]) == ix["n_rw"] + 2 + (4 * ns if cfg["with_ts"] else 0)
    assert len(proof["rw_hashes"]) == 2 * ns and len(proof["if_hashes"]) == 2 and len(proof["rw_claims"]) == ix["n_rw"] and len(proof["if_claims"]) == 2
    for c in proof["commitments"]:
        tr.append_point(c)
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    checks[REASON_MULTISET] = multiset_holds(proof["rw_hashes"], proof["if_hashes"])
    pts = MC.verify_grand_products(proof, 2 * ns, 2, tr)
    if pts is None:
        return None
    checks[REASON_GP] = True
    (rw_claim, hi, lo), (if_claim, hi2, lo2) = pts
    cl = proof["rw_claims"]
    opens = [MC.take_opening(list(range(ix["n_rw"])), lo, cl, tr), MC.take_opening([ix["v_final"], ix["t_final"]], lo2, proof["if_claims"], tr)]
    step, leaves = MC.iota_eval(lo), []
    for s in range(ns):
        w = cl[ix["v_written"] + s - 2] if s >= 2 else cl[ix["v_read"] + s]
        leaves.append(h(cl[ix["addr"] + s], cl[ix["v_read"] + s], cl[ix["t_read"] + s], g, tau))
        leaves.append(h(cl[ix["addr"] + s], w, step, g, tau))
    v_init = W.jolt_instance(cfg["seed"], 1 << cfg["log_n"], 1 << cfg["log_mem"], store_pct=30, n_regs=32)[3]  # public preprocessing
    io = MC.iota_eval(lo2)
    init = h(io, sum(a * b for a, b in zip(v_init, O.eq_evals(lo2))) % R, 0, g, tau)
    fin = h(io, proof["if_claims"][0], proof["if_claims"][1], g, tau)
    checks[REASON_LEAF] = MC.batch_eval(leaves, hi) == rw_claim and MC.batch_eval([init, fin], hi2) == if_claim
    return opens


def verify_range_check_and_open(proof, cfg, tr, checks, opens):
    """rw_proof_verify_range_check_and_open: the range check (with with_ts, its reasons prefixed) and the reduced opening over `opens`
    and the range check's own"""
    import pyharness as H
    ns, nv = cfg["n_slots"], max(cfg["log_n"], cfg["log_mem"])
    if cfg["with_ts"]:
        ix = slot_index(ns)
        polys = [ix["rc_rt"] + i for i in range(4 * ns)] + [ix["t_read"] + s for s in range(ns)]  # t_read: the step-1 commitments
        opening = TP.range_check_verify(proof["ts_hashes"], proof["ts_gp"], proof["ts_claims"], ns, polys, tr, checks, REASON_TS)
        if opening is None:
            return
        opens = opens + [opening]
    checks[REASON_OPENING] = MC.reduced_opening_holds(proof, opens, nv, H._pst_setup(cfg["seed"], nv), tr)


def verify(proof, cfg):
    """the plain verifier: replays the transcript and runs every check -> (ok, reason of the first that fails or None, {check: bool});
    a check after a failed grand product cannot be replayed and counts as failed.  The timestamp reasons are prefixed."""
    cfg = default_cfg(**cfg)
    tr = O.Transcript(LABEL)
    checks = MC.Checks(check_order(cfg["with_ts"]))
    opens = verify_memory_check(proof, cfg, tr, checks)
    if opens is not None:
        verify_range_check_and_open(proof, cfg, tr, checks, opens)
    return checks.result()
