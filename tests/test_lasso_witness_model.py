"""CPU model of the dealer's Lasso lookup witness (tests/lasso_witness_ref.py): the time-ordered counters make a consistent
offline-memory-checking instance over Fr -- with h(a, v, t) = t g^2 + v g + a - tau,
    prod inits * prod flagged writes == prod flagged reads * prod finals --
for random instances, for addresses hit 0, 1 and many times, and no longer once one counter is off by one."""
import pytest

import lasso_witness_ref as W
import pyref as O


def _instance(seed, n, M, density_pct):
    rng = O.SplitMix64(seed)
    addr = [rng.next() % M for _ in range(n)]
    flag = None if density_pct is None else [1 if rng.next() % 100 < density_pct else 0 for _ in range(n)]
    sub = [rng.next() & 0xFFFFFFFF for _ in range(M)]
    return addr, flag, sub, rng.field(), rng.field()


@pytest.mark.parametrize("seed,n,M,density", [(1, 1, 1, None), (2, 40, 7, None), (3, 200, 16, 50), (4, 300, 64, 10), (5, 64, 5, 0), (6, 257, 3, 90)])
def test_counters_satisfy_the_multiset_check(seed, n, M, density):
    addr, flag, sub, g, tau = _instance(seed, n, M, density)
    read, E, final = W.witness(addr, flag, sub)
    on = [j for j in range(n) if flag is None or flag[j]]
    assert sum(final) == len(on)
    for j in range(n):
        if j in on:
            assert read[j] == sum(1 for k in on if k < j and addr[k] == addr[j]) and E[j] == sub[addr[j]]
        else:
            assert read[j] == 0 and E[j] == 0
    assert W.multiset_equal(addr, flag, sub, read, E, final, g, tau)


def test_addresses_hit_zero_one_and_many_times():
    # address 0: never; 1: once; 2: 50 times; 3: only by unflagged steps (= never)
    addr = [2] * 20 + [1] + [3] * 5 + [2] * 30
    flag = [1] * 21 + [0] * 5 + [1] * 30
    sub = [11, 22, 33, 44]
    read, E, final = W.witness(addr, flag, sub)
    assert final == [0, 1, 50, 0]
    assert read[:21] == list(range(20)) + [0] and read[21:26] == [0] * 5 and read[26:] == list(range(20, 50))
    assert E[21:26] == [0] * 5 and E[20] == 22 and E[0] == 33
    rng = O.SplitMix64(9)
    assert W.multiset_equal(addr, flag, sub, read, E, final, rng.field(), rng.field())


@pytest.mark.parametrize("which", ["final", "read", "final_of_an_unused_address"])
def test_one_bumped_counter_breaks_the_check(which):
    addr, flag, sub, g, tau = _instance(21, 120, 9, 60)
    read, E, final = W.witness(addr, flag, sub)
    assert W.multiset_equal(addr, flag, sub, read, E, final, g, tau)
    if which == "final":
        final[addr[[j for j in range(120) if flag[j]][0]]] += 1
    elif which == "read":
        read[[j for j in range(120) if flag[j]][-1]] += 1
    else:
        addr = [a % 8 for a in addr]  # address 8 is never hit
        read, E, final = W.witness(addr, flag, sub)
        assert final[8] == 0 and W.multiset_equal(addr, flag, sub, read, E, final, g, tau)
        final[8] += 1
    assert not W.multiset_equal(addr, flag, sub, read, E, final, g, tau)


def test_a_flagged_address_past_the_table_is_refused_and_an_unflagged_one_ignored():
    with pytest.raises(ValueError):
        W.witness([0, 4], None, [1, 2, 3, 4])
    assert W.witness([0, 4, 0], [1, 0, 1], [1, 2, 3, 4]) == ([0, 0, 1], [1, 0, 1], [2, 0, 0, 0])
