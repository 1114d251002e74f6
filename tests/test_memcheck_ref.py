"""CPU tests of tests/memcheck_ref.py's reduced opening, the one verifier ending that the four restated proofs rest on, on proofs whose
openings have different lengths: the read-write memory proof at (log_n, log_mem, n_slots, with_ts) = (3, 7, 3, 0) has two, of 3 and 7
variables, and the whole memory proof at the same config three, of 3, 7 and 7.  The honest proof is accepted; a reduced claim or a
round coefficient plus one, a PST13 proof point replaced by another curve point and a removed round are each rejected by the opening
check alone; and the helper itself rejects two openings in swapped order."""
import pytest

import memcheck_ref as MC
import memory_proof_ref as MP
import pyref as O
import rw_proof_ref as P

R = O.R
NV = 7
CFG = dict(log_n=3, log_mem=NV, n_slots=3, with_ts=0, seed=5)
MODULES = {"rw": (P, CFG), "memory": (MP, dict(CFG, io_start=61, io_len=6))}


@pytest.fixture(scope="module")
def proofs():
    """both proofs, made once and left unchanged: name -> proof"""
    return {name: mod.prove(cfg) for name, (mod, cfg) in MODULES.items()}


@pytest.fixture(scope="module")
def ck():
    import pyharness as H  # pulls in the whole flow oracle
    return H._pst_setup(CFG["seed"], NV)


def _rejected_by_the_opening_alone(name, proof):
    mod, cfg = MODULES[name]
    ok, reason, checks = mod.verify(proof, cfg)
    return not ok and reason == MC.REASON_OPENING and [k for k, v in checks.items() if not v] == [MC.REASON_OPENING]


def _before_the_ending(name, proof):
    """the verifier's openings and its transcript as they stand when the reduced opening begins"""
    mod, cfg = MODULES[name]
    cfg = mod.default_cfg(**cfg)
    tr = O.Transcript(P.LABEL)
    checks = MC.Checks(P.check_order(0))
    opens = P.verify_memory_check(proof, cfg, tr, checks)
    assert checks.result()[0] is False and checks.result()[1] == MC.REASON_OPENING  # the memory check holds; the opening is still to come
    if name == "memory":  # the output check's rounds, then its opening of v_final
        tr.challenge_vector(NV)
        r_out = []
        for comp in proof["out_comps"]:
            tr.append_scalars(comp)
            r_out.append(tr.challenge_scalar())
        opens.append(MC.take_opening([P.slot_index(cfg["n_slots"])["v_final"]], r_out, proof["out_claims"], tr))
    return opens, tr


@pytest.mark.parametrize("name,lengths", [("rw", [3, 7]), ("memory", [3, 7, 7])])
def test_the_honest_proof_is_accepted(proofs, ck, name, lengths):
    mod, cfg = MODULES[name]
    proof = proofs[name]
    ok, reason, checks = mod.verify(proof, cfg)
    assert ok and reason is None and all(checks.values())
    opens, tr = _before_the_ending(name, proof)
    assert [len(o["point"]) for o in opens] == lengths and len(proof["reduced_claims"]) == len(lengths)
    assert len(proof["reduced"]["round_polys"]) == len(proof["joint_proofs"]) == NV
    assert MC.reduced_opening_holds(proof, opens, NV, ck, tr) is True


@pytest.mark.parametrize("name,i", [("rw", 0), ("rw", 1), ("memory", 0), ("memory", 2)])
def test_a_reduced_claim_plus_one_is_rejected(proofs, name, i):
    claims = list(proofs[name]["reduced_claims"])
    claims[i] = (claims[i] + 1) % R
    assert _rejected_by_the_opening_alone(name, dict(proofs[name], reduced_claims=claims))


@pytest.mark.parametrize("name,j,k", [("rw", 0, 0), ("rw", NV - 1, -1), ("memory", 3, 1)])
def test_a_round_coefficient_plus_one_is_rejected(proofs, name, j, k):
    rounds = [list(c) for c in proofs[name]["reduced"]["round_polys"]]
    rounds[j][k] = (rounds[j][k] + 1) % R
    assert _rejected_by_the_opening_alone(name, dict(proofs[name], reduced=dict(proofs[name]["reduced"], round_polys=rounds)))


@pytest.mark.parametrize("name,i", [("rw", 0), ("memory", NV - 1)])
def test_another_curve_point_in_the_pst13_proof_is_rejected(proofs, name, i):
    points = list(proofs[name]["joint_proofs"])
    other = O.g1_add(points[i], proofs[name]["commitments"][0])
    assert other is not None and other != points[i]
    points[i] = other
    assert _rejected_by_the_opening_alone(name, dict(proofs[name], joint_proofs=points))


@pytest.mark.parametrize("name,j", [("rw", NV - 1), ("memory", 0)])
def test_a_removed_round_is_rejected(proofs, name, j):
    rounds = list(proofs[name]["reduced"]["round_polys"])
    del rounds[j]
    assert _rejected_by_the_opening_alone(name, dict(proofs[name], reduced=dict(proofs[name]["reduced"], round_polys=rounds)))


@pytest.mark.parametrize("name,a,b", [("rw", 0, 1), ("memory", 0, 1), ("memory", 1, 2)])
def test_swapped_openings_are_rejected(proofs, ck, name, a, b):
    opens, tr = _before_the_ending(name, proofs[name])
    opens[a], opens[b] = opens[b], opens[a]
    assert MC.reduced_opening_holds(proofs[name], opens, NV, ck, tr) is False
