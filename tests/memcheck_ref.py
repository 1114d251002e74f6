"""The steps that more than one plain-Python restatement of a memory-check proof runs, each written once, in the vocabulary of
csrc/host/memcheck_steps.hpp: tests/ts_proof_ref.py, tests/rw_proof_ref.py, tests/memory_proof_ref.py and tests/bytecode_ref.py call
them under their own transcripts and keep what is their own (the instance, the witness, the leaves, the word model of their kernel,
the leaf check).  A prover step takes the transcript and returns its values and its bytes; a verifier step replays the transcript.
From oracle/pyflow.py, oracle/pyharness.py and oracle/pyspartan_outer.py, imported where they are used: they pull in the whole flow
oracle.  jolt-core is not in the reference tree: these steps and the harnesses' plain verifiers are what pins the protocols (parity
unpinned).  The timestamp range check as a step under a caller's transcript (ts_range_check_worker, ts_range_check_verify) is
tests/ts_proof_ref.py's, next to its leaves, as in csrc/host/ts_range_proof.hpp."""
import pyref as O

R = O.R
MONT = 1 << 256
M32 = (1 << 32) - 1
REASON_MULTISET = "multiset equality"
REASON_GP = "grand product"
REASON_LEAF = "leaf claim"
REASON_OPENING = "opening"


def bits(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def iota_eval(point):
    """mc_iota_eval: the identity column 0, 1, 2, .. at a big-endian point"""
    acc = 0
    for rj in point:
        acc = (2 * acc + rj) % R
    return acc


def batch_eval(values, hi):
    """mc_batch_eval with pad 0: the MLE of circuit-major leaf values at the circuit variables"""
    return sum(e * v for e, v in zip(O.eq_evals(hi), values + [0] * ((1 << len(hi)) - len(values)))) % R


def limbs32(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def mont(x):
    return x % R * MONT % R


class Checks:
    """a plain verifier's verdict over the checks of `order`: each counts as failed until it is set, so one that cannot be replayed
    after a failed grand product stays failed; result() -> (ok, reason of the first that fails or None, {check: bool})"""

    def __init__(self, order):
        self.order = list(order)
        self.passed = {k: False for k in self.order}

    def __setitem__(self, check, holds):
        assert check in self.passed
        self.passed[check] = holds

    def result(self):
        first = next((k for k in self.order if not self.passed[k]), None)
        return first is None, first, self.passed


# ------------------------------------------------------------------------------------------------ prover (worker with its coordinator)
def commit_columns(ck, cols, tr):
    """mc_commit_worker + mc_receive_commitments -> (commitments, bytes): u64(count), then u64(bits(len)) + g1 per column"""
    import pyharness as H
    commitments = [H._commit(ck, c) for c in cols]
    for c in commitments:
        tr.append_point(c)
    return commitments, O.ser_u64(len(cols)) + b"".join(O.ser_u64(bits(len(col))) + O.ser_g1(c) for col, c in zip(cols, commitments))


def open_columns(cols, point, tr, tamper_claim=False):
    """compact_open_worker + receive_claims: -> (claims, the opening for reduce_and_prove); the claims' bytes are ser_vec_fr"""
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


def memory_checking(rw_leaves, rw_batch, if_leaves, if_batch, tr):
    """mc_memory_checking + mc_coordinate_memory_checking up to the claims, over circuit-major leaves: both dense grand products, the
    hashes into the transcript, both proofs -> (dict(rw_hashes, if_hashes, rw_gp, if_gp), the opening point of each: the challenges
    after the batch bits, bytes)"""
    import pyflow as F
    rw_layers, rw_hashes = F.dense_gp([rw_leaves], rw_batch, tr)
    if_layers, if_hashes = F.dense_gp([if_leaves], if_batch, tr)
    tr.append_scalars(rw_hashes)
    tr.append_scalars(if_hashes)
    rw_gp, r_rw = O.gp_prove(rw_layers, tr)
    if_gp, r_if = O.gp_prove(if_layers, tr)
    out = O.ser_vec_fr(rw_hashes) + O.ser_vec_fr(if_hashes) + F.ser_gp(rw_gp) + F.ser_gp(if_gp)
    return dict(rw_hashes=rw_hashes, if_hashes=if_hashes, rw_gp=rw_gp, if_gp=if_gp), r_rw[bits(rw_batch):], r_if[bits(if_batch):], out


def reduce_and_prove(ck, openings, nv, tr):
    """reduce_and_prove over every opening of the proof: the reduction sumcheck, gamma, the joint polynomial over gamma^i, one PST13
    opening -> (dict(reduced, reduced_claims, joint_proofs), bytes)"""
    r_red, red_claims, red = O.opening_reduce([openings], tr)
    gamma = tr.challenge_scalar()
    joint, pw = [0] * (1 << nv), 1
    for op in openings:
        for i, v in enumerate(op["poly"]):
            joint[i] = (joint[i] + v * pw) % R
        pw = pw * gamma % R
    proofs, _ = O.pst_open(ck, joint, list(reversed(r_red)))
    out = O.ser_u64(len(red["round_polys"])) + b"".join(O.ser_vec_fr(c) for c in red["round_polys"]) + O.ser_vec_fr(red_claims)
    out += O.ser_u64(len(proofs)) + b"".join(O.ser_g1(p) for p in proofs)
    return dict(reduced=red, reduced_claims=red_claims, joint_proofs=proofs), out


# ------------------------------------------------------------------------------------------------ plain verifier
def verify_grand_product(gp, hashes, batch, tr):
    """mc_verify_grand_product: the outputs are the hashes and every round and layer reduction holds -> (claim, hi, lo), the point
    split after the batch bits, or None"""
    out = O.gp_verify(gp, batch, tr) if gp["outputs"] == hashes else None
    if out is None:
        return None
    claim, r = out
    k = bits(batch)
    return claim, r[:k], r[k:]


def verify_grand_products(proof, rw_batch, if_batch, tr):
    """mc_verify_grand_products: the hashes go into the transcript first -> ((rw_claim, hi, lo), (if_claim, hi2, lo2)) or None"""
    tr.append_scalars(proof["rw_hashes"])
    tr.append_scalars(proof["if_hashes"])
    rw = verify_grand_product(proof["rw_gp"], proof["rw_hashes"], rw_batch, tr)
    inf = verify_grand_product(proof["if_gp"], proof["if_hashes"], if_batch, tr) if rw is not None else None
    return None if inf is None else (rw, inf)


def take_opening(polys, point, claims, tr):
    """VerifierOpenings::take: one claim exchange of the commitments `polys` at `point`; its batching challenge is drawn here"""
    return dict(point=point, polys=polys, claims=claims, rho=tr.challenge_scalar())


def reduced_opening_holds(proof, opens, nv, ck, tr):
    """verify_reduced_opening: the reduction sumcheck over openings of any lengths up to nv, then one PST13 check with the trapdoor of
    the joint commitment over gamma^i rho_i^j"""
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
