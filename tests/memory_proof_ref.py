"""Plain-Python restatement of the whole read-write memory proof (co-zkvms_amd/memory_proof.py MemoryProof, csrc/host/memory_proof.hpp)
on the two steps of tests/rw_proof_ref.py, called as they stand -- the memory check, and the timestamp range check with the ending --
with the output check of tests/output_check_ref.py between them, under the one transcript "cozk-rw-memory" and ONE reduce_and_prove.  `prove`
gives the proof bytes and `prefix_len`, the offset at which the output check's part begins (everything before it is rw_proof_ref.prove's
bytes at the same config); `verify` replays the transcript with rw_proof_ref's reasons plus the output check's two.  jolt-core is not in
the reference tree: this file and the harness's verifier are what pins the protocol (parity unpinned)."""
import memcheck_ref as MC
import output_check_ref as OC
import pyref as O
import rw_proof_ref as P

R = O.R
M32 = MC.M32
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
    import pyharness as H
    cfg = default_cfg(**cfg)
    rcfg = _rw_cfg(cfg)
    wit = P.witness(rcfg)
    ck = H._pst_setup(cfg["seed"], max(cfg["log_n"], cfg["log_mem"]))
    tr = O.Transcript(P.LABEL)
    # 1-4. the memory check: rw_proof_ref's step
    res, openings, out = P.prove_memory_check(rcfg, wit, ck, tr)
    res["prefix_len"] = len(out)
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
    out_claims, op = MC.open_columns([wit["v_final"]], r_out, tr)
    out += O.ser_u64(len(comps)) + b"".join(O.ser_vec_fr(c) for c in comps) + O.ser_vec_fr(out_claims)
    res.update(out_comps=comps, out_claims=out_claims, v_io=v_io)
    # 5, 6. the range check and ONE reduce_and_prove: rw_proof_ref's step
    return P.prove_range_check_and_open(rcfg, wit, ck, tr, res, openings + [op], out)


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
    """the plain verifier -> (ok, reason of the first check that fails or None, {check: bool}): rw_proof_ref's two verifier steps with the
    output check between them, and its opening in the reduced opening"""
    cfg = default_cfg(**cfg)
    tr = O.Transcript(P.LABEL)
    checks = MC.Checks(P.check_order(cfg["with_ts"], [REASON_OUT_SHAPE, REASON_OUT_FINAL]))
    opens = P.verify_memory_check(proof, cfg, tr, checks)
    if opens is None:
        return checks.result()
    # the output check
    r_eq = tr.challenge_vector(cfg["log_mem"])
    comps = proof["out_comps"]
    shape = len(comps) == cfg["log_mem"] and all(len(c) == 3 for c in comps) and len(proof["out_claims"]) == 1
    checks[REASON_OUT_SHAPE] = shape
    if not shape:
        return checks.result()
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
    opens.append(MC.take_opening([P.slot_index(cfg["n_slots"])["v_final"]], r_out, proof["out_claims"], tr))
    P.verify_range_check_and_open(proof, cfg, tr, checks, opens)
    return checks.result()
