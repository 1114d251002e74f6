"""CPU: the references the device tests of the primary sumcheck's forms rely on (tests/test_gpu_primary_forms.py) agree with
each other at the shapes used there.  For every admitted (form, chunk count) pair and for the linear forms, one round message
of oracle/pyprimary.py's prover_message by the plain prover == the sum of three Rep3 parties' == the direct sum
  sum over index pairs of eq(X) (sum_i flag_i(X) g_i(E(X)) - out(X)),  X = 0, 2, .., D
from g_plain alone (tests/primary_ref.py), in the first round (0/1 flags) and after a bind (field flags)."""
import pytest

import primary_ref as PR
import pyprimary as P
import pyref as O

N = 16


def _check(instrs, seed, n=N, **kw):
    inst = PR.Instance(instrs, n, seed, **kw)
    plain, three = PR.RefState.of(inst, 1), PR.RefState.of(inst, 3)
    rng = O.SplitMix64(seed + 1)
    for _ in range(2 if n >= 4 else 1):
        want = plain.direct()
        assert len(want) == P.sumcheck_degree(instrs)
        assert plain.total() == want
        assert three.total() == want
        assert three.direct() == want
        assert plain.n_items() == three.n_items()
        r = rng.field()
        plain.bind(r)
        three.bind(r)
    return inst


def test_the_table_lists_51_pairs():
    assert len(PR.PAIRS) == 51 and len(set(PR.PAIRS)) == 51


@pytest.mark.parametrize("form,C", PR.PAIRS, ids=PR.PAIR_IDS)
def test_pair_plain_equals_three_parties_equals_direct(form, C):
    instr = PR.form_instr(form, C)
    assert len(instr.mems) == PR.n_mems(form, C) <= 20 and instr.chunks() == C
    table = PR.pair_table(form, C)
    assert P.sumcheck_degree(table) == instr.g_degree() + 2 <= 8
    _check(table, 1000 + 16 * form + C)


@pytest.mark.parametrize("name", list(PR.LINEAR_TABLES))
def test_linear_forms_plain_equals_three_parties_equals_direct(name):
    table = PR.LINEAR_TABLES[name]
    assert P.sumcheck_degree(table) == 3
    for n in (2, N):
        _check(table, 77 + len(name), n=n)


def test_concat_weights_are_powers_of_the_shift():
    e = [3, 5, 7]
    assert P.g_plain(P.Instr(P.CONCAT, range(3), 16), e) == (3 << 32) + (5 << 16) + 7
    assert P.g_plain(P.Instr(P.CONCAT, range(3), 0), e) == 15
    assert P.g_plain(P.Instr(P.CONCAT, [0, 0, 1], 4), [3, 3, 5]) == (3 << 8) + (3 << 4) + 5  # g takes one value per listed memory
    assert P.g_plain(P.Instr(P.CONCAT, range(20), 10), [1] + [0] * 19) == 1 << 190


def test_item_count_and_levels_of_the_helper():
    """count_items counts pairs, not entries, and only multiplicative instructions; levels() is the number of reshared
    multiplications that precede an instruction's last one"""
    table = [P.Instr(P.CONCAT, [0], 0), P.Instr(P.PRODUCT, [0, 1])]
    flags = [[1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 5]]
    assert PR.count_items(table, flags) == 2
    want = {(P.PRODUCT, 1): 0, (P.PRODUCT, 2): 0, (P.PRODUCT, 6): 4, (P.LTU, 2): 0, (P.LTU, 6): 4, (P.LTE, 1): 0, (P.DIV0, 2): 0,
            (P.UNSIGNED_REM, 6): 4, (P.SLT, 2): 1, (P.NOT_SLT, 4): 3, (P.SIGNED_REM, 2): 1, (P.SIGNED_REM, 4): 3}
    for (f, C), lv in want.items():
        assert PR.levels(PR.form_instr(f, C)) == lv, (f, C)
    assert max(PR.levels(PR.form_instr(f, C)) for f, C in PR.PAIRS) == 4


def test_all_zero_flags_leave_only_the_outputs():
    """a multiplicative instruction whose flags are all zero contributes nothing: the message is that of the outputs alone"""
    table = [PR.form_instr(P.SIGNED_REM, 4), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, N, 5, zero_flags=(0, 1))
    st = PR.RefState.of(inst, 3)
    assert st.n_items() == 0
    D = P.sumcheck_degree(table)
    want = [0] * D
    for i in range(N // 2):
        for k in range(D):
            X = 0 if k == 0 else k + 1
            at = lambda c: (c[2 * i] + X * (c[2 * i + 1] - c[2 * i])) % O.R
            want[k] = (want[k] - at(inst.eq) * at(inst.outs)) % O.R
    assert st.total() == want == st.direct()
