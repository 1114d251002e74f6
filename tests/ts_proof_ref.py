"""Plain-Python restatement of the timestamp range-check proof (co-zkvms_amd/ts_proof.py, csrc/host/ts_range_proof.hpp), shared by
tests/test_ts_proof_model.py (CPU) and the GPU tests:

  * `range_check_prove` / `range_check_verify` and `prove` / `verify` (second half of the file): the range check as a step under a
    caller's transcript, and the whole proof -- prover with its coordinator, proof bytes, plain verifier with the harness's
    reasons -- on the shared steps of tests/memcheck_ref.py.

  * `range_leaves`: the 6 n_slots + 1 grand-product circuits of the range check, circuit-major, in the layout of
    cozk_timestamp_range_leaves.  h(key, count) = count g^2 + key (g + 1) - tau is ts_range_ref.fingerprint of the tuple
    (key, key, count).  jolt-core is not in the reference tree: the circuit order is this project's (parity unpinned); what pins the
    leaves is the multiset identity init * write == read * final of every (slot, kind), which `multiset_hashes` evaluates.
  * `compact_sum_model`: the word arithmetic of csrc/compact_open.inc -- an exact 11-limb integer accumulator of Montgomery-form
    operands times plain column entries, every carry propagated with its term, reduced once as to_mont(from_mont(T0)) + to_mont(T1).
    It asserts the invariants the kernel's comment claims.  Expected VALUES in the tests come from big-int arithmetic, never from
    the model."""
import memcheck_ref as MC
import pyref as O
import ts_range_ref as TR

R = O.R
MONT, M32, mont = MC.MONT, MC.M32, MC.mont
RINV = pow(MONT, -1, R)
CO_LIMBS = 11
CO_TERMS_BOUND = 1 << 32  # terms an accumulator holds: (2^32) * 2^320 = 2^352


def h(key, count, g, tau):
    return TR.fingerprint(key, key, count, g, tau)


def range_leaves(t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, g, tau):
    """every column a list of n entries per slot (the witness with M == n) -> 6 n_slots + 1 lists of n leaves"""
    ns, n = len(t_read), len(t_read[0])
    g2 = g * g % R
    out = [None] * (6 * ns + 1)
    init = [h(j, 0, g, tau) for j in range(n)]
    out[4 * ns] = init
    for s in range(ns):
        rt = [h(t_read[s][j], rc_rt[s][j], g, tau) for j in range(n)]
        gmr = [h(j - t_read[s][j], rc_gmr[s][j], g, tau) for j in range(n)]
        out[4 * s], out[4 * s + 1] = rt, [(x + g2) % R for x in rt]
        out[4 * s + 2], out[4 * s + 3] = gmr, [(x + g2) % R for x in gmr]
        out[4 * ns + 1 + 2 * s] = [(init[j] + fc_rt[s][j] * g2) % R for j in range(n)]
        out[4 * ns + 2 + 2 * s] = [(init[j] + fc_gmr[s][j] * g2) % R for j in range(n)]
    return out


def _prod(xs):
    p = 1
    for x in xs:
        p = p * x % R
    return p


def multiset_hashes(leaves):
    """the product of every circuit's leaves: what the grand product claims"""
    return [_prod(c) for c in leaves]


def multiset_holds(hashes, ns):
    """for every slot and both kinds: hash[init] * hash[write] == hash[read] * hash[final]"""
    init = hashes[4 * ns]
    return all(init * hashes[4 * s + 2 * kind + 1] % R == hashes[4 * s + 2 * kind] * hashes[4 * ns + 1 + 2 * s + kind] % R for s in range(ns) for kind in range(2))


# ------------------------------------------------------------------------------------------------ compact_open.inc
def _mac(acc, a_limbs, v, off):
    """co_mac<off>: acc += a * v * 2^(32 off) on 32-bit words, the carry walked to the top limb"""
    carry = 0
    for k in range(8):
        t = a_limbs[k] * v + acc[off + k] + carry
        assert t < 1 << 64  # (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        acc[off + k] = t & M32
        carry = t >> 32
    for k in range(off + 8, CO_LIMBS):
        t = acc[k] + carry
        acc[k] = t & M32
        carry = t >> 32
    assert carry == 0  # the sum fits 352 bits


def compact_sum_model(operands, entries, bits):
    """sum of operands[i] * entries[i] mod r: operands are residues in Montgomery form (any 256-bit words), entries plain integers
    below 2^bits (bits = 8, 16, 32: one limb; 64: two) -> the canonical 256-bit word the kernel stores"""
    assert len(operands) == len(entries) and len(operands) < CO_TERMS_BOUND
    acc = [0] * CO_LIMBS
    for a, v in zip(operands, entries):
        assert 0 <= a < MONT and 0 <= v < 1 << bits
        A = MC.limbs32(a, 8)
        _mac(acc, A, v & M32, 0)
        if bits == 64:
            _mac(acc, A, v >> 32, 1)
    s = sum(w << (32 * i) for i, w in enumerate(acc))
    assert s == sum(a * v for a, v in zip(operands, entries))
    t0, t1 = s & (MONT - 1), s >> 256
    assert t1 < 1 << 96
    from_mont_t0 = t0 * RINV % R
    return (from_mont_t0 * MONT + t1 * MONT) % R  # to_mont(from_mont(T0)) + to_mont(T1)


# ------------------------------------------------------------------------------------------------ the whole proof
# csrc/host/ts_range_proof.hpp restated on the steps of tests/memcheck_ref.py: the range check as a step under a caller's transcript
# (tests/rw_proof_ref.py chains it behind the memory check), then the proof around it.  jolt-core is not in the reference tree: this
# file and the harness's verifier are what pins the protocol.
LABEL = b"cozk-ts-range"
REASON_MULTISET, REASON_GP, REASON_LEAF, REASON_OPENING = MC.REASON_MULTISET, MC.REASON_GP, MC.REASON_LEAF, MC.REASON_OPENING


def default_cfg(**kw):
    cfg = dict(log_n=3, log_mem=5, n_slots=4, seed=1, tamper=0)
    cfg.update(kw)
    return cfg


def witness(cfg):
    """the harness's trace and columns in the proof's order: rc_rt[0..], rc_gmr[0..], fc_rt[0..], fc_gmr[0..], t_read[0..]"""
    import rw_witness_ref as W
    N, ns = 1 << cfg["log_n"], cfg["n_slots"]
    addr, vw, iw, vi = W.jolt_instance(cfg["seed"], N, 1 << cfg["log_mem"], store_pct=30, n_regs=32)
    t_read = W.replay(addr, vw, iw, vi)[1][:ns]
    rc_rt, rc_gmr, fc_rt, fc_gmr = TR.ts_range(t_read, N)
    if cfg["tamper"] == 1:
        fc_rt = [list(c) for c in fc_rt]
        fc_rt[0][t_read[0][N // 2]] += 1
    return t_read, rc_rt, rc_gmr, fc_rt, fc_gmr


def leaf_values(claims, ns, iota, g, tau):
    """the 6 ns + 1 leaf values at a point from the 5 ns claims there and the identity column's value"""
    g1, g2 = (g + 1) % R, g * g % R
    init = (iota * g1 - tau) % R
    out = [0] * (6 * ns + 1)
    for s in range(ns):
        rc_rt, rc_gmr, fc_rt, fc_gmr, t = claims[s], claims[ns + s], claims[2 * ns + s], claims[3 * ns + s], claims[4 * ns + s]
        out[4 * s] = (t * g1 + rc_rt * g2 - tau) % R
        out[4 * s + 1] = (out[4 * s] + g2) % R
        out[4 * s + 2] = (init - t * g1 + rc_gmr * g2) % R
        out[4 * s + 3] = (out[4 * s + 2] + g2) % R
        out[4 * ns + 1 + 2 * s] = (init + fc_rt * g2) % R
        out[4 * ns + 2 + 2 * s] = (init + fc_gmr * g2) % R
    out[4 * ns] = init
    return out


def range_check_prove(t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, tr, tamper_claim=False):
    """ts_range_check_worker + ts_range_check_coordinate, after the commit: gamma and tau, the leaves, ONE dense batched grand product
    whose claimed outputs are the multiset hashes, ONE opening of the families and t_read -> (hashes, gp, claims, the opening, bytes)"""
    import pyflow as F
    circuits = 6 * len(t_read) + 1
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    leaves = [x for c in range_leaves(t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, g, tau) for x in c]
    layers, hashes = F.dense_gp([leaves], circuits, tr)
    tr.append_scalars(hashes)
    gp, r = O.gp_prove(layers, tr)
    claims, op = MC.open_columns(rc_rt + rc_gmr + fc_rt + fc_gmr + t_read, r[MC.bits(circuits):], tr, tamper_claim)
    return hashes, gp, claims, op, O.ser_vec_fr(hashes) + F.ser_gp(gp) + O.ser_vec_fr(claims)


def range_check_verify(hashes, gp, claims, ns, polys, tr, checks, prefix=""):
    """ts_range_check_verify, after the commitments are in the transcript: sets the first three checks (their reasons behind `prefix`)
    -> the opening of the commitments `polys` (family-major, then t_read), or None after a failed grand product"""
    circuits = 6 * ns + 1
    assert len(hashes) == circuits and len(claims) == 5 * ns
    g, tau = tr.challenge_scalar(), tr.challenge_scalar()
    tr.append_scalars(hashes)
    checks[prefix + REASON_MULTISET] = multiset_holds(hashes, ns)
    out = MC.verify_grand_product(gp, hashes, circuits, tr)
    if out is None:
        return None
    checks[prefix + REASON_GP] = True
    claim, hi, lo = out
    checks[prefix + REASON_LEAF] = MC.batch_eval(leaf_values(claims, ns, MC.iota_eval(lo), g, tau), hi) == claim
    return MC.take_opening(polys, lo, claims, tr)


def prove(cfg):
    """-> dict(proof_bytes, commitments, hashes, gp, claims, reduced, reduced_claims, joint_proofs)"""
    import pyharness as H
    cfg = default_cfg(**cfg)
    t_read, rc_rt, rc_gmr, fc_rt, fc_gmr = witness(cfg)
    ck = H._pst_setup(cfg["seed"], cfg["log_n"])
    tr = O.Transcript(LABEL)
    commitments, out = MC.commit_columns(ck, rc_rt + rc_gmr + fc_rt + fc_gmr + t_read, tr)
    hashes, gp, claims, op, part = range_check_prove(t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, tr, cfg["tamper"] == 2)
    res, ending = MC.reduce_and_prove(ck, [op], cfg["log_n"], tr)
    res.update(proof_bytes=out + part + ending, commitments=commitments, hashes=hashes, gp=gp, claims=claims)
    return res


def verify(proof, cfg):
    """the plain verifier: replays the transcript and runs all four checks -> (ok, reason of the first that fails or None,
    {check: bool}); a check after a failed grand product cannot be replayed and counts as failed"""
    import pyharness as H
    cfg = default_cfg(**cfg)
    nv, ncols = cfg["log_n"], 5 * cfg["n_slots"]
    tr = O.Transcript(LABEL)
    checks = MC.Checks([REASON_MULTISET, REASON_GP, REASON_LEAF, REASON_OPENING])
    assert len(proof["commitments"]) == ncols
    for c in proof["commitments"]:
        tr.append_point(c)
    opening = range_check_verify(proof["hashes"], proof["gp"], proof["claims"], cfg["n_slots"], list(range(ncols)), tr, checks)
    if opening is not None:
        checks[REASON_OPENING] = MC.reduced_opening_holds(proof, [opening], nv, H._pst_setup(cfg["seed"], nv), tr)
    return checks.result()
