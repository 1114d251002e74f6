"""CPU tests of tests/memory_proof_ref.py: the restated prover and verifier of the whole read-write memory proof accept their own proof
(4 slots with the range check, 3 slots without and log_mem > log_n), the bytes before prefix_len are rw_proof_ref.prove's bytes at the
same config, the output check's rounds are those of the dense product sumcheck, tamper 4 is rejected by the output check's final claim
alone, and the window evaluations in O(W m) are the MLEs of the MEM-entry vectors."""
import pytest

import memory_proof_ref as MP
import output_check_ref as OC
import pyref as O
import rw_proof_ref as P

R = O.R


@pytest.fixture(scope="module")
def proofs():
    """every proof of this file, made once: (log_n, log_mem, n_slots, with_ts, io_start, io_len, tamper) -> (cfg, proof)"""
    out = {}
    for key in [(1, 5, 4, 1, 3, 5, 0), (3, 7, 3, 0, 61, 6, 0), (3, 5, 4, 1, 3, 5, 4)]:
        log_n, log_mem, ns, with_ts, lo, W, tamper = key
        cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, with_ts=with_ts, io_start=lo, io_len=W, tamper=tamper, seed=9)
        out[key] = (cfg, MP.prove(cfg))
    return out


@pytest.mark.parametrize("key", [(1, 5, 4, 1, 3, 5, 0), (3, 7, 3, 0, 61, 6, 0)])
def test_the_reference_proves_and_verifies_and_its_prefix_is_the_rw_proof(proofs, key):
    cfg, proof = proofs[key]
    ok, reason, checks = MP.verify(proof, cfg)
    assert ok and reason is None and all(checks.values()), (reason, checks)
    assert len(proof["reduced_claims"]) == (4 if cfg["with_ts"] else 3)  # one opening more than the rw proof
    rw = P.prove({k: cfg[k] for k in ("log_n", "log_mem", "n_slots", "with_ts", "seed")})
    n = proof["prefix_len"]
    assert 0 < n < len(proof["proof_bytes"]) and proof["proof_bytes"][:n] == rw["proof_bytes"][:n]
    assert proof["rw_claims"] == rw["rw_claims"] and proof["if_claims"] == rw["if_claims"]
    assert len(proof["out_comps"]) == cfg["log_mem"] and proof["out_comps"][0][0] == 0  # the honest sum is zero


def test_output_rounds_are_the_dense_sumchecks(proofs):
    cfg, proof = proofs[(3, 7, 3, 0, 61, 6, 0)]
    wit = P.witness(MP._rw_cfg(MP.default_cfg(**cfg)))
    # replay the transcript up to r_eq through the verifier's own steps: the challenges are in the compressed polynomials' hashes, so
    # take r_eq and r_out from a verifier run instrumented by the same calls
    tr = O.Transcript(P.LABEL)
    for c in proof["commitments"]:
        tr.append_point(c)
    tr.challenge_scalar(), tr.challenge_scalar()
    tr.append_scalars(proof["rw_hashes"])
    tr.append_scalars(proof["if_hashes"])
    assert O.gp_verify(proof["rw_gp"], 2 * cfg["n_slots"], tr) is not None and O.gp_verify(proof["if_gp"], 2, tr) is not None
    tr.challenge_scalar(), tr.challenge_scalar()
    r_eq = tr.challenge_vector(cfg["log_mem"])
    r_out = []
    for comp in proof["out_comps"]:
        tr.append_scalars(comp)
        r_out.append(tr.challenge_scalar())
    rounds, fin = OC.dense_rounds(wit["v_final"], proof["v_io"], cfg["io_start"], r_eq, r_out)
    assert [c[0] for c in proof["out_comps"]] == [s[0] for s in rounds]
    claim = 0
    for (s0, s2, s3), comp, r in zip(rounds, proof["out_comps"], r_out):
        poly = O.unipoly_from_evals([s0, (claim - s0) % R, s2, s3])
        assert O.unipoly_compress(poly) == comp
        claim = O.unipoly_eval(poly, r)
    assert fin[2] == (proof["out_claims"][0] - MP.window_evals(proof["v_io"], cfg["io_start"], r_out)[1]) % R
    assert fin[1] == MP.window_evals(proof["v_io"], cfg["io_start"], r_out)[0] and claim == fin[0] * fin[1] * fin[2] % R


def test_tamper_4_is_rejected_by_the_output_checks_final_claim_alone(proofs):
    cfg, proof = proofs[(3, 5, 4, 1, 3, 5, 4)]
    ok, reason, checks = MP.verify(proof, cfg)
    assert not ok and reason == MP.REASON_OUT_FINAL == "output check: final claim"
    assert [k for k, v in checks.items() if not v] == [reason]
    honest = P.witness(MP._rw_cfg(MP.default_cfg(**cfg)))["v_final"][3:8]
    assert [(a - b) & MP.M32 for a, b in zip(proof["v_io"], honest)] == [0, 0, 1, 0, 0]


def test_window_evals_are_the_mles():
    rnd = O.SplitMix64(77)
    m, lo, W = 6, 29, 7
    v_io = [rnd.next() & MP.M32 for _ in range(W)]
    r = [rnd.field() for _ in range(m)]
    eq = O.eq_evals(r)
    assert MP.window_evals(v_io, lo, r) == (sum(eq[lo:lo + W]) % R, sum(e * v for e, v in zip(eq[lo:lo + W], v_io)) % R)
