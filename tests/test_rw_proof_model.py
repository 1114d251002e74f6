"""CPU tests of tests/rw_proof_ref.py: the big-int leaves in the layout of cozk_rw_memory_leaves / cozk_rw_memory_init_final_leaves
satisfy the multiset identity on jolt_instance and stop satisfying it after tamper 1; the restated prover and verifier accept their own
proof at log_n = 1 and 3 (4 slots with the range check, 3 slots without and log_mem > log_n, one slot) and reject every tamper with its
reason; the word model of the exact-sum kernels agrees with big-int arithmetic at columns of 2^32 - 1 and gamma, tau in {0, 1, r - 1}."""
import pytest

import pyref as O
import rw_proof_ref as P
import rw_witness_ref as W
import ts_proof_ref as TP

R = O.R
TOP = (1 << 32) - 1


@pytest.mark.parametrize("ns,log_n,log_mem", [(4, 3, 5), (4, 1, 5), (3, 3, 7), (2, 4, 5), (1, 3, 5)])
def test_leaves_satisfy_the_multiset_identity_and_tamper_1_breaks_it(ns, log_n, log_mem):
    cfg = P.default_cfg(log_n=log_n, log_mem=log_mem, n_slots=ns, seed=300 + ns, with_ts=0)
    rng = O.SplitMix64(301)
    g, tau = rng.field(), rng.field()

    def hashes(wit):
        w = [wit["v_written"][s] if s >= 2 else None for s in range(ns)]
        rw = P.rw_leaves(wit["addr"], wit["v_read"], wit["t_read"], w, g, tau)
        inf = P.if_leaves(wit["v_init"], wit["v_final"], wit["t_final"], g, tau)
        assert len(rw) == 2 * ns and all(len(c) == 1 << log_n for c in rw) and [len(c) for c in inf] == [1 << log_mem] * 2
        return TP.multiset_hashes(rw), TP.multiset_hashes(inf)
    wit = P.witness(cfg)
    rw_h, if_h = hashes(wit)
    assert P.multiset_holds(rw_h, if_h)
    # the four products are those of the witness reference
    full = [wit["v_written"][s] if s >= 2 else wit["v_read"][s] for s in range(ns)]
    init, wr, rd, fin = W.hashes(wit["addr"], wit["v_init"], wit["v_read"], wit["t_read"], full, wit["v_final"], wit["t_final"], g, tau)
    prod = lambda xs: TP._prod(xs)
    assert (if_h[0], prod(rw_h[1::2]), prod(rw_h[0::2]), if_h[1]) == (init, wr, rd, fin)
    rw_t, if_t = hashes(P.witness(dict(cfg, tamper=1)))
    assert not P.multiset_holds(rw_t, if_t)


@pytest.mark.parametrize("g", [0, 1, R - 1, None], ids=["zero", "one", "minus_one", "random"])
@pytest.mark.parametrize("tau", [0, 1, R - 1, None], ids=["zero", "one", "minus_one", "random"])
def test_leaf_word_model_at_extreme_operands(g, tau):
    rng = O.SplitMix64(310)
    g = rng.field() if g is None else g
    tau = rng.field() if tau is None else tau
    for a, v, t in [(TOP, TOP, TOP), (0, 0, 0), (TOP, 0, 0), (0, TOP, 0), (0, 0, TOP), (1, 1, 1), (rng.next() & TOP, rng.next() & TOP, rng.next() & TOP)]:
        assert P.leaf_word_model(a, v, t, g, tau) == P.mont(P.h(a, v, t, g, tau))


def test_leaf_word_model_bounds():
    """the sum of three terms and the constant fits 9 limbs, the quotient 35 bits, and S - qh r stays below 2^256"""
    top = 3 * TOP * (R - 1) + (R - 1)
    assert top < 3 << (32 + 254) and top < 1 << (32 * P.RL_LIMBS)
    assert top // R < 3 << 32 and P.RL_MU == (1 << 288) // R and P.RL_MU < 1 << 35
    assert 3 * R < 1 << 256
    # coefficients that are not residues (any 256-bit words) are outside the kernel's precondition: the model refuses what overflows
    with pytest.raises(AssertionError):
        acc = [P.M32] * 8 + [0]
        for _ in range(4):
            P._term(acc, (1 << 256) - 1, TOP)
        P._reduce(acc)


@pytest.fixture(scope="module")
def proofs():
    """every proof of this file, made once: (log_n, log_mem, n_slots, with_ts, tamper) -> (cfg, proof)"""
    out = {}
    for key in [(1, 5, 4, 1, 0), (3, 5, 4, 1, 0), (3, 7, 3, 0, 0), (3, 5, 1, 1, 0), (3, 5, 4, 1, 1), (3, 5, 4, 1, 2), (3, 5, 4, 1, 3), (1, 5, 4, 1, 1), (1, 5, 4, 1, 2),
                (1, 5, 4, 1, 3)]:
        log_n, log_mem, ns, with_ts, tamper = key
        cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, with_ts=with_ts, tamper=tamper, seed=9)
        out[key] = (cfg, P.prove(cfg))
    return out


@pytest.mark.parametrize("key", [(1, 5, 4, 1, 0), (3, 5, 4, 1, 0), (3, 7, 3, 0, 0), (3, 5, 1, 1, 0)])
def test_the_reference_proves_and_verifies(proofs, key):
    log_n, log_mem, ns, with_ts, _ = key
    cfg, proof = proofs[key]
    ok, reason, checks = P.verify(proof, cfg)
    assert ok and reason is None and all(checks.values()), (reason, checks)
    ncom = 3 * ns + max(0, ns - 2) + 2 + (4 * ns if with_ts else 0)
    nv = max(log_n, log_mem)
    b = proof["proof_bytes"]
    assert b[:8] == ncom.to_bytes(8, "little") and b[8:16] == log_n.to_bytes(8, "little")
    assert b[-(8 + 64 * nv):][:8] == nv.to_bytes(8, "little")  # one PST13 opening of max(log_n, log_mem) points at the end
    assert proof["rw_hashes"] == proof["rw_gp"]["outputs"] and proof["if_hashes"] == proof["if_gp"]["outputs"]
    assert len(proof["reduced_claims"]) == (3 if with_ts else 2)


def test_a_verifier_with_another_seed_rejects(proofs):
    cfg, proof = proofs[(3, 5, 4, 1, 0)]
    ok, reason, checks = P.verify(proof, dict(cfg, seed=10))  # another v_init and another trapdoor
    assert not ok and reason == P.REASON_LEAF and checks[P.REASON_MULTISET] and checks[P.REASON_GP] and not checks[P.REASON_OPENING]


@pytest.mark.parametrize("log_n", [1, 3])
def test_tamper_1_is_rejected_by_the_multiset_check_alone(proofs, log_n):
    cfg, proof = proofs[(log_n, 5, 4, 1, 1)]
    ok, reason, checks = P.verify(proof, cfg)
    assert not ok and reason == P.REASON_MULTISET
    assert [k for k, v in checks.items() if not v] == [P.REASON_MULTISET]


@pytest.mark.parametrize("log_n", [1, 3])
def test_tamper_2_is_rejected_by_the_leaf_check(proofs, log_n):
    cfg, proof = proofs[(log_n, 5, 4, 1, 2)]
    ok, reason, checks = P.verify(proof, cfg)
    assert not ok and reason == P.REASON_LEAF and checks[P.REASON_MULTISET] and checks[P.REASON_GP] and not checks[P.REASON_LEAF]
    honest = proofs[(log_n, 5, 4, 1, 0)][1]
    assert proof["rw_claims"][0] == (honest["rw_claims"][0] + 1) % R and proof["rw_claims"][1:] == honest["rw_claims"][1:] and proof["rw_hashes"] == honest["rw_hashes"]


@pytest.mark.parametrize("log_n", [1, 3])
def test_tamper_3_is_rejected_by_the_timestamp_multiset_check_alone(proofs, log_n):
    cfg, proof = proofs[(log_n, 5, 4, 1, 3)]
    ok, reason, checks = P.verify(proof, cfg)
    assert not ok and reason == P.REASON_TS + TP.REASON_MULTISET == "timestamp: multiset equality"
    assert [k for k, v in checks.items() if not v] == [reason]
