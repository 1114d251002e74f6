"""CPU test of the windowed output check's structure (tests/output_check_ref.py): the windowed algorithm -- sides, rho, H, Llow, the
windowed dots, the folds, the dense tail -- gives every round's evaluations and the three final values of the plain dense product
sumcheck over BN254 Fr, at m = 1, 2, 3, 5, 6 for windows of one word, the whole memory, an aligned half, the last word, windows across an
aligned boundary, W = 2^j + 1 and seeded random windows, with d at both ends of the signed 33-bit range; it never holds MEM Fr entries
unless W' = MEM; and the first fold's word model keeps the limb bound the kernel states."""
import random

import pytest

import output_check_ref as OC

R, M32 = OC.R, OC.M32


def _instance(m, lo, W, seed):
    rnd = random.Random(seed)
    MEM = 1 << m
    edge = [0, M32, 1, M32 - 1]
    vf = [rnd.choice(edge) if rnd.random() < 0.5 else rnd.getrandbits(32) for _ in range(MEM)]
    vio = [rnd.choice(edge) if rnd.random() < 0.5 else rnd.getrandbits(32) for _ in range(W)]
    vf[lo], vio[0] = M32, 0  # d = 2^32 - 1
    if W > 1:
        vf[lo + W - 1], vio[W - 1] = 0, M32  # d = -(2^32 - 1)
    special = [0, 1, R - 1]
    r_eq = [rnd.choice(special) if rnd.random() < 0.2 else rnd.randrange(R) for _ in range(m)]
    rs = [rnd.choice(special) if rnd.random() < 0.2 else rnd.randrange(R) for _ in range(m)]
    return vf, vio, r_eq, rs


@pytest.mark.parametrize("m", [1, 2, 3, 5, 6])
def test_windowed_rounds_equal_the_dense_sumcheck(m):
    MEM, n = 1 << m, 0
    for lo, W in OC.windows(m, 7 + m):
        vf, vio, r_eq, rs = _instance(m, lo, W, 1000 * m + 31 * lo + W)
        want_rounds, want_final = OC.dense_rounds(vf, vio, lo, r_eq, rs)
        got_rounds, got_final, peak = OC.windowed_rounds(vf, vio, lo, r_eq, rs)
        assert got_rounds == want_rounds, (m, lo, W)
        assert got_final == want_final, (m, lo, W)
        Wp = 1 << (W - 1).bit_length()
        assert peak == (3 * MEM if Wp == MEM else max(Wp, MEM // 2 + 2 * Wp)), (m, lo, W)  # no MEM-entry Fr vector unless W' = MEM
        n += 1
    assert n >= min(6, MEM * (MEM + 1) // 2)  # m = 1 has three windows in all


def test_honest_claim_is_zero_and_a_wrong_output_is_not():
    m, lo, W = 5, 9, 11
    vf, _, r_eq, rs = _instance(m, lo, W, 5)
    vio = vf[lo:lo + W]

    def final_claim_holds(vio):
        """the verifier's walk from the claim 0: g_k(1) = claim - g_k(0), claim' = g_k(r_k); at the end claim == eq(r) io_range(r) d(r)"""
        rounds, fin, _ = OC.windowed_rounds(vf, vio, lo, r_eq, rs)
        claim = 0
        for (s0, s2, s3), r in zip(rounds, rs):
            claim = OC.O.unipoly_eval(OC.O.unipoly_from_evals([s0, (claim - s0) % R, s2, s3]), r)
        return claim == fin[0] * fin[1] * fin[2] % R, rounds, fin
    ok, rounds, fin = final_claim_holds(vio)
    assert ok and rounds[0][0] == 0
    assert fin[2] == sum(e * v for e, v in zip(OC.O.eq_evals(rs), [0 if lo <= x < lo + W else vf[x] for x in range(1 << m)])) % R
    vio[W // 2] = (vio[W // 2] + 1) & M32
    assert not final_claim_holds(vio)[0]


def test_sides_of_a_window():
    w = OC.Windowed([0] * 64, [0] * 5, 30, [0] * 6)  # W' = 8: 32 lies inside
    assert w.sides == [(30, 32), (32, 35)] and w.lw == 3
    w = OC.Windowed([0] * 64, [0] * 5, 32, [0] * 6)
    assert w.sides == [(32, 37)]
    w = OC.Windowed([0] * 64, [0] * 8, 24, [0] * 6)  # ends on a multiple: one side
    assert w.sides == [(24, 32)]
    w = OC.Windowed([0] * 2, [0], 1, [0])
    assert w.sides == [(1, 2)] and w.lw == 0 and w.sparse()


def test_first_fold_word_model_keeps_its_limb_bound():
    rnd = random.Random(3)
    words = [0, 1, M32, M32 - 1]
    for r in [0, 1, R - 1, R - 2, (R + 1) // 2] + [rnd.randrange(R) for _ in range(20)]:
        for _ in range(12):
            a, b = rnd.choice(words + [rnd.getrandbits(32)]), rnd.choice(words + [rnd.getrandbits(32)])
            io_lo = rnd.choice([None, 0, M32, rnd.getrandbits(32)])
            io_hi = rnd.choice([None, 0, M32, rnd.getrandbits(32)])
            want = ((1 - r) * (a - (io_lo or 0)) + r * (b - (io_hi or 0))) % R * OC.MONT % R
            assert OC.first_fold_words(a, b, io_lo, io_hi, r) == want
    # the largest sum: both operands r - 1 in Montgomery form cannot happen at once (a + b = R mod r), so take the bound per term
    assert 2 * (OC.MONT - 1) * M32 < 1 << 289
