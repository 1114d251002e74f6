"""Plain-Python restatement of the whole read-write memory proof (co-zkvms_amd/memory_proof.py MemoryProof, csrc/host/memory_proof.hpp)
on the helpers of tests/rw_proof_ref.py: its witness, leaves, openings and checks, with the output check of tests/output_check_ref.py
between the memory check and the timestamp range check, under the one transcript "cozk-rw-memory" and ONE reduce_and_prove.  `prove`
gives the proof bytes and `prefix_len`, the offset at which the output check's part begins (everything before it is rw_proof_ref.prove's
bytes at the same config); `verify` replays the transcript with rw_proof_ref's reasons plus the output check's two.  jolt-core is not in
the reference tree: this file and the harness's verifier are what pins the protocol (parity unpinned)."""
import output_check_ref as OC
import pyref as O
import rw_proof_ref as P
import ts_proof_ref as TP

R = O.R
M32 = P.M32
REASON_OUT_SHAPE = "output check: shape"
REASON_OUT_FINAL = "output check: final claim"


def default_cfg(**kw):
    cfg = dict(P.default_cfg(), io_start=3, io_len=5)
    cfg.update(kw)
    return cfg


def _rw_cfg(cfg):
    """the config rw_proof_ref sees: tamper 4 is the output check's, the witness stays honest"""
    c = {k: cfg[k] for k in ("log_n", "log_mem", "n_slots", "seed", "with_ts", "tamper")}
    if c["tamper"] == 4:
        c["tamper"] = 0
    return c


def v_io_of(cfg, v_final):
    lo, W = cfg["io_start"], cfg["io_len"]
    v_io = list(v_final[lo:lo + W])
    if cfg["tamper"] == 4:
        v_io[W // 2] = (v_io[W // 2] + 1) & M32
    return v_io


def prove(cfg):
    """-> rw_proof_ref.prove's dict plus out_comps, out_claims, v_io, prefix_len"""
    import pyflow as F
    import pyharness as H
    cfg = default_cfg(**cfg)
    rcfg = _rw_cfg(cfg)
    ns, N, MEM = cfg["n_slots"], 1 << cfg["log_n"], 1 << cfg["log_mem"]
    nv = max(cfg["log_n"], cfg["log_mem"])
    wit = P.witness(rcfg)
    writers = [wit["v_written"][s] for s in range(ns) if s >= 2]
    rw_cols = wit["addr"] + wit["v_read"] + writers + wit["t_read"]
    if_cols = [wit["v_final"], wit["t_final"]]
    ts_fams = wit["rc_rt"] + wit["rc_gmr"] + wit["fc_rt"] + wit["fc_gmr"] if cfg["with_ts"] else []
    ck = H._pst_setup(cfg["seed"], nv)
    tr = O.Transcript(P.LABEL)
    # 1-4. the memory check, as rw_proof_ref.prove
    committed = rw_cols + if_cols + ts_fams
    commitments = [H._commit(ck, c) for c in committed]
    for c in commitments:
        tr.append_point(c)
    out = O.ser_u64(len(committed)) + b"".join(O.ser_u64(P._bits(len(col))) + O.ser_g1(c) for col, c in zip(committed, commitments))
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    w = [wit["v_written"][s] if s >= 2 else None for s in range(ns)]
    rwl = [x for c in P.rw_leaves(wit["addr"], wit["v_read"], wit["t_read"], w, g, tau) for x in c]
    ifl = [x for c in P.if_leaves(wit["v_init"], wit["v_final"], wit["t_final"], g, tau) for x in c]
    rw_layers, rw_hashes = F.dense_gp([rwl], 2 * ns, tr)
    if_layers, if_hashes = F.dense_gp([ifl], 2, tr)
    tr.append_scalars(rw_hashes)
    tr.append_scalars(if_hashes)
    rw_gp, r_rw = O.gp_prove(rw_layers, tr)
    if_gp, r_if = O.gp_prove(if_layers, tr)
    openings = []
    rw_claims, op = P._open(rw_cols, r_rw[P._bits(2 * ns):], tr, cfg["tamper"] == 2)
    openings.append(op)
    if_claims, op = P._open(if_cols, r_if[1:], tr)
    openings.append(op)
    out += O.ser_vec_fr(rw_hashes) + O.ser_vec_fr(if_hashes) + F.ser_gp(rw_gp) + F.ser_gp(if_gp) + O.ser_vec_fr(rw_claims) + O.ser_vec_fr(if_claims)
    res = {"commitments": commitments, "rw_hashes": rw_hashes, "if_hashes": if_hashes, "rw_gp": rw_gp, "if_gp": if_gp, "rw_claims": rw_claims, "if_claims": if_claims,
           "prefix_len": len(out)}
    # the output check: r_eq, log_mem rounds of the windowed sumcheck in prove_arbitrary_worker's messages, the opening of v_final
    v_io = v_io_of(cfg, wit["v_final"])
    r_eq = tr.challenge_vector(cfg["log_mem"])
    oc = OC.Windowed(wit["v_final"], v_io, cfg["io_start"], r_eq)
    comps, r_out, claim = [], [], 0
    for k in range(cfg["log_mem"]):
        if k:
            oc.bind(r_out[-1])
        s0, s2, s3 = oc.round_evals()
        poly = O.unipoly_from_evals([s0, (claim - s0) % R, s2, s3])
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_out.append(tr.challenge_scalar())
        comps.append(comp)
        claim = O.unipoly_eval(poly, r_out[-1])
    out_claims, op = P._open([wit["v_final"]], r_out, tr)
    openings.append(op)
    out += O.ser_u64(len(comps)) + b"".join(O.ser_vec_fr(c) for c in comps) + O.ser_vec_fr(out_claims)
    res.update(out_comps=comps, out_claims=out_claims, v_io=v_io)
    # 5. the timestamp range check under the same transcript, as rw_proof_ref.prove
    if cfg["with_ts"]:
        tg, ttau = tr.challenge_scalar(), tr.challenge_scalar()
        circuits = 6 * ns + 1
        leaves = [x for c in TP.range_leaves(wit["t_read"], wit["rc_rt"], wit["rc_gmr"], wit["fc_rt"], wit["fc_gmr"], tg, ttau) for x in c]
        layers, hashes = F.dense_gp([leaves], circuits, tr)
        tr.append_scalars(hashes)
        gp, r = O.gp_prove(layers, tr)
        ts_claims, op = P._open(ts_fams + wit["t_read"], r[P._bits(circuits):], tr)
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


def window_evals(v_io, lo, r):
    """io_range(r) and v_io(r) over the window only: O(W m)"""
    m, rng, val = len(r), 0, 0
    for j, v in enumerate(v_io):
        x, e = lo + j, 1
        for i in range(m):
            e = e * (r[i] if (x >> (m - 1 - i)) & 1 else 1 - r[i]) % R
        rng, val = (rng + e) % R, (val + e * v) % R
    return rng, val


def verify(proof, cfg):
    """the plain verifier -> (ok, reason of the first check that fails or None, {check: bool}); rw_proof_ref.verify with the output check
    between the leaf claim and the range check, and its opening in the reduced opening"""
    import pyharness as H
    cfg = default_cfg(**cfg)
    ns, with_ts = cfg["n_slots"], cfg["with_ts"]
    nw = max(0, ns - 2)
    n_rw = 3 * ns + nw
    ix = dict(addr=0, v_read=ns, v_written=2 * ns, t_read=2 * ns + nw, v_final=n_rw, t_final=n_rw + 1, rc_rt=n_rw + 2)
    nv = max(cfg["log_n"], cfg["log_mem"])
    ck = H._pst_setup(cfg["seed"], nv)
    tr = O.Transcript(P.LABEL)
    order = [P.REASON_MULTISET, P.REASON_GP, P.REASON_LEAF, REASON_OUT_SHAPE, REASON_OUT_FINAL]
    if with_ts:
        order += [P.REASON_TS + k for k in (TP.REASON_MULTISET, TP.REASON_GP, TP.REASON_LEAF)]
    order.append(P.REASON_OPENING)
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
    checks[P.REASON_MULTISET] = P.multiset_holds(proof["rw_hashes"], proof["if_hashes"])
    if proof["rw_gp"]["outputs"] != proof["rw_hashes"] or proof["if_gp"]["outputs"] != proof["if_hashes"]:
        return result()
    out_rw = O.gp_verify(proof["rw_gp"], 2 * ns, tr)
    out_if = O.gp_verify(proof["if_gp"], 2, tr) if out_rw is not None else None
    if out_rw is None or out_if is None:
        return result()
    checks[P.REASON_GP] = True
    (rw_claim, r_rw), (if_claim, r_if) = out_rw, out_if
    k = P._bits(2 * ns)
    hi, lo, hi2, lo2 = r_rw[:k], r_rw[k:], r_if[:1], r_if[1:]
    opens = [dict(point=lo, polys=list(range(n_rw)), claims=proof["rw_claims"], rho=tr.challenge_scalar())]
    opens.append(dict(point=lo2, polys=[ix["v_final"], ix["t_final"]], claims=proof["if_claims"], rho=tr.challenge_scalar()))
    cl = proof["rw_claims"]
    step, leaves = P._iota(lo), []
    for s in range(ns):
        w = cl[ix["v_written"] + s - 2] if s >= 2 else cl[ix["v_read"] + s]
        leaves.append(P.h(cl[ix["addr"] + s], cl[ix["v_read"] + s], cl[ix["t_read"] + s], g, tau))
        leaves.append(P.h(cl[ix["addr"] + s], w, step, g, tau))
    v_init = P.W.jolt_instance(cfg["seed"], 1 << cfg["log_n"], 1 << cfg["log_mem"], store_pct=30, n_regs=32)[3]  # public preprocessing
    io = P._iota(lo2)
    init = P.h(io, sum(a * b for a, b in zip(v_init, O.eq_evals(lo2))) % R, 0, g, tau)
    fin = P.h(io, proof["if_claims"][0], proof["if_claims"][1], g, tau)
    checks[P.REASON_LEAF] = P._batch_eval(leaves, hi) == rw_claim and P._batch_eval([init, fin], hi2) == if_claim
    # the output check
    r_eq = tr.challenge_vector(cfg["log_mem"])
    comps = proof["out_comps"]
    checks[REASON_OUT_SHAPE] = len(comps) == cfg["log_mem"] and all(len(c) == 3 for c in comps) and len(proof["out_claims"]) == 1
    if not checks[REASON_OUT_SHAPE]:
        return result()
    e, r_out = 0, []
    for comp in comps:
        poly = [comp[0], (e - 2 * comp[0] - sum(comp[1:])) % R] + list(comp[1:])
        tr.append_scalars(comp)
        r_out.append(tr.challenge_scalar())
        e = O.unipoly_eval(poly, r_out[-1])
    eqv = 1
    for a, b in zip(r_eq, r_out):
        eqv = eqv * ((a * b + (1 - a) * (1 - b)) % R) % R
    rng, vio_r = window_evals(proof["v_io"], cfg["io_start"], r_out)
    checks[REASON_OUT_FINAL] = eqv * rng % R * ((proof["out_claims"][0] - vio_r) % R) % R == e
    opens.append(dict(point=r_out, polys=[ix["v_final"]], claims=proof["out_claims"], rho=tr.challenge_scalar()))
    if with_ts:
        circuits = 6 * ns + 1
        assert len(proof["ts_hashes"]) == circuits and len(proof["ts_claims"]) == 5 * ns
        tg, ttau = tr.challenge_scalar(), tr.challenge_scalar()
        tr.append_scalars(proof["ts_hashes"])
        checks[P.REASON_TS + TP.REASON_MULTISET] = TP.multiset_holds(proof["ts_hashes"], ns)
        out = O.gp_verify(proof["ts_gp"], circuits, tr) if proof["ts_gp"]["outputs"] == proof["ts_hashes"] else None
        if out is None:
            return result()
        checks[P.REASON_TS + TP.REASON_GP] = True
        claim, r = out
        kk = P._bits(circuits)
        lv = TP.leaf_values(proof["ts_claims"], ns, P._iota(r[kk:]), tg, ttau)
        checks[P.REASON_TS + TP.REASON_LEAF] = P._batch_eval(lv, r[:kk]) == claim
        polys = [ix["rc_rt"] + i for i in range(4 * ns)] + [ix["t_read"] + s for s in range(ns)]
        opens.append(dict(point=r[kk:], polys=polys, claims=proof["ts_claims"], rho=tr.challenge_scalar()))
    checks[P.REASON_OPENING] = reduced_opening_holds(proof, opens, nv, ck, tr)
    return result()


def reduced_opening_holds(proof, opens, nv, ck, tr):
    """the reduction sumcheck over all openings, then one PST13 check with the trapdoor (rw_proof_ref.verify's ending)"""
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
    rs = []
    if len(proof["reduced"]["round_polys"]) != nv or len(proof["reduced_claims"]) != len(opens):
        return False
    for comp in proof["reduced"]["round_polys"]:
        poly = [comp[0], (e - 2 * comp[0] - sum(comp[1:])) % R] + list(comp[1:])
        tr.append_scalars(comp)
        rj = tr.challenge_scalar()
        rs.append(rj)
        e = O.unipoly_eval(poly, rj)
    expect = 0
    for c, o, rc in zip(coeffs, opens, proof["reduced_claims"]):
        eqv = 1
        for a, b in zip(o["point"], rs[nv - len(o["point"]):]):
            eqv = eqv * ((a * b + (1 - a) * (1 - b)) % R) % R
        expect = (expect + c * eqv * rc) % R
    if expect != e:
        return False
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
    return O.pst_check_with_trapdoor(ck, joint_c, list(reversed(rs)), joint_claim, proof["joint_proofs"])
