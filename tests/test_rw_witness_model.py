"""CPU model of the dealer's read-write memory witness (tests/rw_witness_ref.py): the sequential replay and the sort-and-sweep
formulation give the same vectors; those vectors make a consistent offline-memory-checking instance over Fr,
    prod inits * prod writes == prod reads * prod finals   with h(a, v, t) = t g^2 + v g + a - tau,
for random instances and for slots that alias inside a step; and one wrong entry breaks it."""
import pytest

import pyref as O
import rw_witness_ref as W

RANDOM = [(1, 1, 1, 30), (2, 40, 7, 30), (3, 200, 16, 0), (4, 120, 300, 10), (5, 64, 5, 100), (6, 257, 3, 50)]
ALIASING = W.aliasing_instances()


def _cases():
    return [("random_%d" % c[0],) + W.jolt_instance(*c) for c in RANDOM] + ALIASING


def _challenges(seed):
    rng = O.SplitMix64(seed)
    return rng.field(), rng.field()


@pytest.mark.parametrize("case", _cases(), ids=[c[0] for c in _cases()])
def test_replay_equals_sort_and_sweep_and_satisfies_the_multiset_check(case):
    _, addr, v_write, is_write, v_init = case
    out = W.replay(addr, v_write, is_write, v_init)
    assert W.sort_and_sweep(addr, v_write, is_write, v_init) == out
    v_read, t_read, v_written, v_final, t_final = out
    n = len(addr[0])
    for s in range(4):
        assert all(t_read[s][j] <= j for j in range(n))  # what the public timestamp-validity proof needs
    assert v_written[:3] == [None, None, None] and v_written[3] == W.written(v_write, is_write, v_read)[3]
    g, tau = _challenges(500 + n)
    assert W.multiset_equal(addr, v_write, is_write, v_init, v_read, t_read, v_final, t_final, g, tau)


def test_slots_without_a_writer_keep_the_memory_and_one_slot_works():
    addr, _, _, v_init = W.jolt_instance(9, 50, 11)
    v_read, t_read, v_written, v_final, t_final = W.replay(addr, [None] * 4, [None] * 4, v_init)
    assert v_final == v_init and v_written == [None] * 4
    for a in range(11):
        touched = [j for j in range(50) for s in range(4) if addr[s][j] == a]
        assert t_final[a] == (max(touched) if touched else 0)
    g, tau = _challenges(77)
    assert W.multiset_equal(addr, [None] * 4, [None] * 4, v_init, v_read, t_read, v_final, t_final, g, tau)
    one = W.replay([addr[3]], [v_init[:1] * 50], [None], v_init)
    assert W.sort_and_sweep([addr[3]], [v_init[:1] * 50], [None], v_init) == one and one[2] == [None]


@pytest.mark.parametrize("which", ["t_final", "t_final_of_an_untouched_address", "v_read", "slots_exchanged_inside_a_step"])
def test_one_wrong_entry_breaks_the_check(which):
    addr, v_write, is_write, v_init = W.jolt_instance(21, 60, 40, n_regs=8)
    v_read, t_read, _, v_final, t_final = W.replay(addr, v_write, is_write, v_init)
    g, tau = _challenges(33)
    assert W.multiset_equal(addr, v_write, is_write, v_init, v_read, t_read, v_final, t_final, g, tau)
    if which == "t_final":
        t_final[addr[2][7]] += 1
    elif which == "t_final_of_an_untouched_address":
        free = [a for a in range(40) if all(a not in col for col in addr)]
        assert free and t_final[free[0]] == 0
        t_final[free[0]] += 1
    elif which == "v_read":
        v_read[0][30] ^= 1
    else:  # the read tuples of rs1 and rd of one step change places (their addresses differ there)
        j = [k for k in range(60) if addr[0][k] != addr[2][k]][3]
        v_read[0][j], v_read[2][j] = v_read[2][j], v_read[0][j]
        t_read[0][j], t_read[2][j] = t_read[2][j], t_read[0][j]
    assert not W.multiset_equal(addr, v_write, is_write, v_init, v_read, t_read, v_final, t_final, g, tau)


def test_the_slot_order_inside_a_step_decides_the_vectors():
    """with rs1 == rd, rs1 reads the word from before the step's write only because it comes first: the same trace replayed with rd
    ahead of rs1 is another (self-consistent) witness, so the device has to keep the (step, slot) order to be compared exactly"""
    _, addr, v_write, is_write, v_init = ALIASING[0]
    order = [2, 0, 1, 3]
    ref = W.replay(addr, v_write, is_write, v_init)
    alt = W.replay([addr[s] for s in order], [v_write[s] for s in order], [is_write[s] for s in order], v_init)
    assert alt[0][1] != ref[0][0]  # v_read of rs1
    assert alt[0][1][5] == v_write[2][5] != ref[0][0][5]  # rd ahead of rs1: rs1 reads the step's own write
    assert alt[3] == ref[3]  # the final memory does not depend on it here: rd is the only writer of these addresses in a step


def test_an_address_past_the_memory_is_refused_by_step_and_slot():
    addr, v_write, is_write, v_init = W.jolt_instance(5, 10, 6)
    addr[3][4] = 6
    addr[1][7] = 9
    for f in (W.replay, W.sort_and_sweep):
        with pytest.raises(ValueError, match="step 4, slot 3"):
            f(addr, v_write, is_write, v_init)
