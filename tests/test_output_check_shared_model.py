"""CPU test of the output check on a shared v_final as a big-int restatement per party (tests/output_check_shared_ref.py): for every
window of output_check_ref.windows(m, seed) at m = 1, 2, 3, 5, 6 and the four roles -- PLAIN and the REP3 parties 0, 1, 2 -- the windowed
form on the one vector T = a (+ b) equals, round by round and in the final values, the dense rounds made from the share components with
(a + b) * 2^-1; and the three parties' messages sum to output_check_ref.dense_rounds of the clear v_final.  The share components include
0 and r - 1, the words 0 and 2^32 - 1, the challenges 0, 1 and r - 1."""
import random

import pytest

import output_check_ref as OC
import output_check_shared_ref as S

R, M32 = OC.R, OC.M32


def _instance(m, lo, W, seed):
    rnd = random.Random(seed)
    MEM = 1 << m
    edge = [0, M32, 1, M32 - 1]
    vf = [rnd.choice(edge) if rnd.random() < 0.5 else rnd.getrandbits(32) for _ in range(MEM)]
    vio = [rnd.choice(edge) if rnd.random() < 0.5 else rnd.getrandbits(32) for _ in range(W)]
    shares = S.share(vf, rnd)
    x0, x2 = shares[0]  # party 0 holds (x_0, x_2): force components 0 and r - 1 at the window's ends, x_1 makes up for them
    for x, (u, v) in ((lo, (0, R - 1)), (lo + W - 1, (R - 1, 0))):
        x0[x], x2[x] = u, v
        shares[1][0][x] = (vf[x] - u - v) % R
    special = [0, 1, R - 1]
    r_eq = [rnd.choice(special) if rnd.random() < 0.25 else rnd.randrange(R) for _ in range(m)]
    rs = [rnd.choice(special) if rnd.random() < 0.25 else rnd.randrange(R) for _ in range(m)]
    return vf, vio, shares, r_eq, rs


def test_the_shares_are_replicated_and_sum_to_the_value():
    rnd = random.Random(3)
    vals = [rnd.getrandbits(32) for _ in range(8)]
    sh = S.share(vals, rnd)
    for i in range(3):
        assert sh[i][1] is sh[(i + 2) % 3][0]  # b_i = a_{i-1}
    assert [sum(sh[i][0][x] for i in range(3)) % R for x in range(8)] == vals


@pytest.mark.parametrize("m", [1, 2, 3, 5, 6])
def test_windowed_equals_dense_per_role_and_the_parties_sum_to_the_clear_rounds(m):
    seen_special = set()
    for lo, W in OC.windows(m, 7 + m):
        vf, vio, shares, r_eq, rs = _instance(m, lo, W, 2000 * m + 31 * lo + W)
        seen_special |= {c for c in r_eq + rs if c in (0, 1, R - 1)}
        clear_rounds, clear_final = OC.dense_rounds(vf, vio, lo, r_eq, rs)
        got = {}
        for role in S.ROLES:
            a, b = S.components(role, vf, shares)
            want = S.dense_rounds(role, a, b, vio, lo, r_eq, rs)
            got[role] = S.windowed_rounds(role, a, b, vio, lo, r_eq, rs)
            for k in range(m):
                assert got[role][0][k] == want[0][k], (m, lo, W, role, k)
            assert got[role][1] == want[1], (m, lo, W, role)
        assert got["plain"] == (clear_rounds, clear_final), (m, lo, W)
        for k in range(m):
            assert [sum(got[p][0][k][e] for p in range(3)) % R for e in range(3)] == clear_rounds[k], (m, lo, W, k)
        assert sum(got[p][1][2] for p in range(3)) % R == clear_final[2], (m, lo, W)
        for p in range(3):
            assert got[p][1][:2] == clear_final[:2]  # eq(r) and io_range(r) are public
    if m >= 5:
        assert seen_special == {0, 1, R - 1}


def test_party_2_never_reads_v_io():
    """sub = 0: party 2's numbers do not depend on the public words"""
    m, lo, W = 5, 9, 11
    vf, vio, shares, r_eq, rs = _instance(m, lo, W, 77)
    a, b = shares[2]
    assert S.windowed_rounds(2, a, b, vio, lo, r_eq, rs) == S.windowed_rounds(2, a, b, [0] * W, lo, r_eq, rs)
    assert S.dense_rounds(2, a, b, vio, lo, r_eq, rs) == S.dense_rounds(2, a, b, [M32] * W, lo, r_eq, rs)
