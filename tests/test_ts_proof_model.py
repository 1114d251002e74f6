"""CPU tests of tests/ts_proof_ref.py: the whole proof proves and verifies at log_n = 1, 3, 5 with 4 slots and at log_n = 3 with one
slot, tamper 1 is rejected by the multiset check alone (the grand product and the opening still verify) and tamper 2 by the leaf check;
the range-check leaves in the layout of cozk_timestamp_range_leaves satisfy the multiset identity
of the memory checking for a consistent witness and stop satisfying it once one final counter is bumped, and the word-level model
of the compact-column accumulator (csrc/compact_open.inc) agrees with big-int arithmetic at the operands that sit on its bounds."""
import numpy as np
import pytest

import pyref as O
import ts_proof_ref as P
import ts_range_ref as TR

R = O.R


def _t_read(seed, ns, n):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(0, j + 1)) for j in range(n)] for _ in range(ns)]


@pytest.mark.parametrize("ns,n", [(4, 2), (4, 8), (4, 32), (1, 8), (8, 5)])
def test_leaves_satisfy_the_multiset_identity_and_a_bumped_counter_breaks_it(ns, n):
    t_read = _t_read(400 + ns + n, ns, n)
    rc_rt, rc_gmr, fc_rt, fc_gmr = TR.ts_range(t_read, n)
    rng = O.SplitMix64(401)
    g, tau = rng.field(), rng.field()
    leaves = P.range_leaves(t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, g, tau)
    assert len(leaves) == 6 * ns + 1 and all(len(c) == n for c in leaves)
    hashes = P.multiset_hashes(leaves)
    assert P.multiset_holds(hashes, ns)
    for s in range(ns):  # the four products of each (slot, kind) are the reference's
        for kind, (rc, fc) in enumerate(((rc_rt, fc_rt), (rc_gmr, fc_gmr))):
            keys = t_read[s] if kind == 0 else [j - t for j, t in enumerate(t_read[s])]
            init, wr, rd, fin = TR.hashes(keys, rc[s], fc[s], g, tau)
            assert (hashes[4 * ns], hashes[4 * s + 2 * kind + 1], hashes[4 * s + 2 * kind], hashes[4 * ns + 1 + 2 * s + kind]) == (init, wr, rd, fin)
    k = n // 2
    bumped = [list(c) for c in fc_rt]
    bumped[0][t_read[0][k]] += 1
    assert not P.multiset_holds(P.multiset_hashes(P.range_leaves(t_read, rc_rt, rc_gmr, bumped, fc_gmr, g, tau)), ns)


def test_leaf_of_global_minus_read_needs_no_key_column():
    """(j - x)(g + 1) = j (g + 1) - x (g + 1): the kernel derives the second key's term from the init leaf and the first key's"""
    rng = O.SplitMix64(402)
    g, tau = rng.field(), rng.field()
    for j, x, c in [(0, 0, 0), (7, 7, 3), ((1 << 32) - 1, 0, (1 << 32) - 1), ((1 << 32) - 1, (1 << 32) - 1, 5)]:
        init = (j * (g + 1) - tau) % R
        assert P.h(j - x, c, g, tau) == (init - x * (g + 1) + c * g * g) % R


@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_compact_accumulator_model_at_its_bounds(bits):
    top = (1 << bits) - 1
    rng = O.SplitMix64(410 + bits)
    # operands as the kernel sees them: Montgomery forms of r - 1, 0, 1, random residues, and the all-ones word (any 256-bit word adds exactly)
    for xs, vs in [([R - 1] * 64, [top] * 64), ([0] * 5, [top] * 5), ([1, R - 1, 2], [0, 0, 0]), ([rng.field() for _ in range(33)], [rng.next() & top for _ in range(33)])]:
        ops = [P.mont(x) for x in xs]
        assert P.compact_sum_model(ops, vs, bits) == P.mont(sum(x * v for x, v in zip(xs, vs)))
    ones = [(1 << 256) - 1] * 200
    assert P.compact_sum_model(ones, [top] * 200, bits) == sum(ones) * top % R


def test_compact_accumulator_holds_2_pow_32_terms():
    """a term is < 2^256 * 2^64; 2^32 of them are < 2^352 = the 11 limbs, and both calls refuse n >= 2^32"""
    assert P.CO_TERMS_BOUND * ((1 << 256) - 1) * ((1 << 64) - 1) < 1 << (32 * P.CO_LIMBS)
    assert (P.CO_TERMS_BOUND * ((1 << 256) - 1) * ((1 << 64) - 1)) >> 256 < 1 << 96  # T1 of the reduction is a residue's low three limbs


@pytest.fixture(scope="module")
def proofs():
    """every proof of this file, made once: (log_n, n_slots, tamper) -> (cfg, proof)"""
    out = {}
    for log_n, ns, tamper in [(1, 4, 0), (3, 4, 0), (5, 4, 0), (3, 1, 0), (3, 4, 1), (3, 4, 2)]:
        cfg = dict(log_n=log_n, n_slots=ns, tamper=tamper, seed=7)
        out[(log_n, ns, tamper)] = (cfg, P.prove(cfg))
    return out


@pytest.mark.parametrize("log_n,ns", [(1, 4), (3, 4), (5, 4), (3, 1)])
def test_the_reference_proves_and_verifies(proofs, log_n, ns):
    cfg, proof = proofs[(log_n, ns, 0)]
    ok, reason, checks = P.verify(proof, cfg)
    assert ok and reason is None and all(checks.values())
    # the bytes: 5 ns commitments of 8 + 64 bytes, 6 ns + 1 hashes, ..., log_n points of the one PST13 opening at the end
    b = proof["proof_bytes"]
    assert b[:8] == (5 * ns).to_bytes(8, "little") and b[8:16] == log_n.to_bytes(8, "little")
    assert b[-(8 + 64 * log_n):][:8] == log_n.to_bytes(8, "little")
    assert proof["hashes"] == proof["gp"]["outputs"] and len(proof["hashes"]) == 6 * ns + 1 and P.multiset_holds(proof["hashes"], ns)


def test_a_verifier_with_another_seed_rejects_the_opening(proofs):
    cfg, proof = proofs[(3, 4, 0)]
    ok, reason, checks = P.verify(proof, dict(cfg, seed=8))  # another trapdoor: everything replays, the PST13 check fails
    assert not ok and reason == P.REASON_OPENING and checks[P.REASON_MULTISET] and checks[P.REASON_GP] and checks[P.REASON_LEAF]


def test_tamper_1_is_rejected_by_the_multiset_check_alone(proofs):
    cfg, proof = proofs[(3, 4, 1)]
    ok, reason, checks = P.verify(proof, cfg)
    assert not ok and reason == P.REASON_MULTISET
    assert checks == {P.REASON_MULTISET: False, P.REASON_GP: True, P.REASON_LEAF: True, P.REASON_OPENING: True}


def test_tamper_2_is_rejected_by_the_leaf_check(proofs):
    cfg, proof = proofs[(3, 4, 2)]
    ok, reason, checks = P.verify(proof, cfg)
    assert not ok and reason == P.REASON_LEAF and checks[P.REASON_MULTISET] and checks[P.REASON_GP] and not checks[P.REASON_LEAF]
    honest = proofs[(3, 4, 0)][1]
    assert proof["claims"][0] == (honest["claims"][0] + 1) % R and proof["claims"][1:] == honest["claims"][1:] and proof["hashes"] == honest["hashes"]
