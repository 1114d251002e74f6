"""GPU: the level groups of the primary sumcheck (cozk_primary_group_*, csrc/primary_group.inc) driven directly.  k = 2t + 1 PLAIN
cozk_primary members hold degree-t Shamir shares of one instance; a twin set of members is driven per member (cozk_primary_level,
cozk_primary_round_finish).  Everything is integer work: every comparison is ==.
  after EVERY level call    every member's level buffer == tests/shamir_primary_ref.py's exchange of the senders' local slot values
                            (which the twins' cozk_primary_level must equal before the exchange)
  after EVERY grouped finish  every row == that member's twin's cozk_primary_round_finish == the reference's message"""
import importlib

import pytest

import primary_ref as PR
import pyprimary as P
import pyref as O
import shamir_primary_ref as SP
import shamir_ref as S

pytestmark = pytest.mark.gpu
R = O.R
INVALID = -1
KMAX = 9  # k = 9 (t = 4) runs the deal kernel's run-time-degree instantiation


@pytest.fixture(scope="module")
def LK():
    return importlib.import_module("co-zkvms_amd.lookups")


@pytest.fixture(scope="module")
def ctxs(cozk):
    """one context per member, all on device 0; the first is the driver"""
    cs = [cozk.Context(0) for _ in range(KMAX)]
    yield cs
    for c in cs:
        c.close()


def _keys(k, seed=3):
    t = (k - 1) // 2
    return [[O.harness_prf_key(seed, 64 * p + c) for c in range(t)] for p in range(k)]


def _shares(inst, k, seed=17):
    """degree-t sharings of the instance's clear columns for k = 2t + 1 members: (E[p][m], outs[p]); any coefficients serve here"""
    t = (k - 1) // 2
    rng = O.SplitMix64(seed)
    cols = [S.eval_vec([list(col)] + [[rng.field() for _ in col] for _ in range(t)], k) for col in list(inst.E) + [inst.outs]]
    return [[cols[m][p] for m in range(len(inst.E))] for p in range(k)], [cols[-1][p] for p in range(k)]


class Rig:
    """k members + k twins on ctxs[0..k), the group on ctxs[0], and the reference state"""

    def __init__(self, cozk, LK, ctxs, inst, k, counter=1000, members=True):
        self.cozk, self.LK, self.k, self.t, self.inst = cozk, LK, k, (k - 1) // 2, inst
        self.ctxs = list(ctxs[:k])
        self.keys = _keys(k)
        self.E, self.outs = _shares(inst, k)
        self.eq, self.flags = list(inst.eq), [list(f) for f in inst.flags]
        rows = PR.rows(LK, inst.instrs)
        mk = lambda p: PR.create(cozk, LK, self.ctxs[p], cozk.MODE_PLAIN, 0, rows, inst.flags, self.E[p], self.outs[p], inst.eq)
        self.members = [mk(p) for p in range(k)]
        self.twins = [mk(p) for p in range(k)]
        self.group = LK.PrimaryGroup(self.ctxs[0], self.members, self.keys)
        self.ctr = counter
        self.D = P.sumcheck_degree(inst.instrs)

    def begin(self, r=None):
        """round_begin on every member and twin -> the reference round"""
        if r is not None:
            self.eq, self.flags, self.E, self.outs = SP.bind_all(self.eq, self.flags, self.E, self.outs, r)
        self.ref = SP.Round(self.inst.instrs, self.eq, self.flags, self.E, self.outs)
        begun = [pr.round_begin(r) for pr in self.members + self.twins]
        assert all(b == (self.ref.n_items, self.ref.n_levels) for b in begun), begun
        assert len(self.group) == len(self.eq)
        return self.ref

    def read(self, p, ptr, n):
        return PR.read_fr(self.cozk, self.ctxs[p], ptr, n)

    def level(self, level):
        """one level through the group, checked member by member; the twins get the exchanged values too -> n_elems"""
        ref = self.ref
        n_el = ref.level_elems[level - 1]
        local = [tw.level(level) for tw in self.twins]  # the per-member local half: (buffer, None, n_elems)
        assert all(o[2] == n_el and o[1] is None for o in local)
        assert self.group.level(level, self.ctr) == n_el
        if not n_el:
            for p in range(self.k):
                assert self.group.level_buffer(p, level) == (None, 0)
                ref.bufs[p][level - 1] = []
            return 0
        z = ref.local_level(level)
        want, _ = SP.exchange(z, self.keys, self.t, self.ctr)
        for p in range(self.k):
            assert self.read(p, local[p][0], n_el) == z[p], ("local slot values", level, p)
            buf, nb = self.group.level_buffer(p, level)
            assert nb == n_el and buf is not None
            assert self.read(p, buf, n_el) == want[p], ("level buffer", level, p)
            PR._copy(self.cozk, self.ctxs[p], local[p][0], buf, 32 * n_el)  # the twin receives what the member received
            ref.bufs[p][level - 1] = want[p]
        self.ctr += n_el
        return n_el

    def finish(self):
        rows = self.group.round_finish()
        assert rows == [tw.round_finish() for tw in self.twins]
        assert rows == self.ref.message()
        return rows

    def round(self, r=None):
        ref = self.begin(r)
        elems = [self.level(level) for level in range(1, ref.n_levels + 1)]
        self.finish()
        return ref.n_items, elems

    def free(self):
        self.group.free()
        for pr in self.members + self.twins:
            pr.free()


def _drive(cozk, LK, ctxs, inst, k, rounds=None, seed=9):
    rig = Rig(cozk, LK, ctxs, inst, k)
    log = []
    try:
        rng = O.SplitMix64(seed)
        r = None
        total = inst.n.bit_length() - 1
        for j in range(total if rounds is None else min(rounds, total)):
            log.append(rig.round(r))
            r = rng.field()
        if rounds is None:  # the members are left as their twins: the final evaluations agree
            assert len(rig.group) == 2
            for pr, tw in zip(rig.members, rig.twins):
                assert pr.final_evals(r) == tw.final_evals(r)
    finally:
        rig.free()
    return log


def _exact_items(n, items, seed):
    """PRODUCT C = 3 with exactly `items` active index pairs beside a CONCAT that runs everywhere else"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), P.Instr(P.CONCAT, [3, 1], 8)]
    inst = PR.Instance(table, n, seed)
    inst.flags = [[1 if j % 2 == 0 and j // 2 < items else 0 for j in range(n)], [0 if j % 2 == 0 and j // 2 < items else 1 for j in range(n)]]
    return inst


# ------------------------------------------------------------------------------------------------ a. members and workgroups
@pytest.mark.parametrize("k,items,n,rounds", [(3, 1, 16, 2), (5, 1, 16, 2), (7, 1, 16, 2), (9, 1, 16, 2), (3, 255, 1024, 2), (3, 256, 1024, 2), (3, 257, 1024, 2),
                                              (5, 257, 1024, 1), (7, 257, 1024, 1)])
def test_item_counts_around_one_workgroup(cozk, LK, ctxs, k, items, n, rounds):
    """1 item, and 255 / 256 / 257: a partial workgroup, a full one, one lane into the second -- round 0 and (k = 3) the round after it"""
    log = _drive(cozk, LK, ctxs, _exact_items(n, items, 100 + items), k, rounds=rounds)
    assert log[0] == (items, [5 * items])
    assert rounds == 1 or log[1][0] == (items + 1) // 2  # bound flags: a pair is live when either of its halves was


def test_several_workgroups_and_a_partial_last_one(cozk, LK, ctxs):
    """about 1500 items from a dense one-hot table of two multiplicative instructions at n = 2048: six workgroups per (point, member)
    in the deal, a partial last one, more than one block partial per row in the grouped finish"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), P.Instr(P.NOT_PRODUCT, [3, 4, 0])]
    inst = PR.Instance(table, 2048, 2048, one_hot=True)
    log = _drive(cozk, LK, ctxs, inst, 3, rounds=1)
    n_items, elems = log[0]
    assert 1400 < n_items <= 2048 and n_items % 256 != 0 and elems == [5 * n_items]


# ------------------------------------------------------------------------------------------------ b. levels
@pytest.mark.parametrize("k", [3, 5])
def test_instruction_without_a_slot_at_a_level_another_has(cozk, LK, ctxs, k):
    """PRODUCT C = 3 (level 1 only) beside SLT C = 4 (three levels, has_add slots, four slots at its last level): all rounds"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 4, first=1), P.Instr(P.CONCAT, [0, 3], 8)]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 16, 71), k)
    assert len(log) == 4 and all(len(e) == 3 and all(x > 0 for x in e) for _, e in log)
    assert all(e[0] > e[1] for _, e in log)  # level 1 holds PRODUCT's slot too


def test_level_with_no_elements(cozk, LK, ctxs):
    """PRODUCT C = 3 has items, SLT C = 4 has all-zero flags: three levels are announced, levels 2 and 3 hold nothing: nothing is
    launched, level_buffer reports (NULL, 0), the counter stays"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 4), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, 16, 72, zero_flags=(1,))
    rig = Rig(cozk, LK, ctxs, inst, 3, counter=500)
    try:
        rng = O.SplitMix64(4)
        r = None
        for j in range(4):
            ctr = rig.ctr
            n_items, elems = rig.round(r)
            assert n_items > 0 and elems[0] == rig.D * n_items and elems[1:] == [0, 0]
            assert rig.ctr == ctr + elems[0]
            r = rng.field()
    finally:
        rig.free()


def test_table_without_multiplicative_instruction_refuses_levels(cozk, LK, ctxs):
    table = [P.Instr(P.CONCAT, [0, 1], 8), P.Instr(P.NOT_FIRST, [1]), P.Instr(P.ZERO, [0])]
    rig = Rig(cozk, LK, ctxs, PR.Instance(table, 16, 73), 3)
    try:
        rng = O.SplitMix64(5)
        r = None
        for j in range(4):
            ref = rig.begin(r)
            assert (ref.n_items, ref.n_levels) == (0, 0)
            with pytest.raises(cozk.CozkError) as err:
                rig.group.level(1, 0)
            assert err.value.code == INVALID and "primary_group_level: bad level / no items" in str(err.value)
            rig.finish()
            r = rng.field()
    finally:
        rig.free()


def test_instruction_index_63(cozk, LK, ctxs):
    table = [P.Instr(P.ZERO, [0]) for _ in range(62)] + [P.Instr(P.CONCAT, [3, 4], 8), PR.form_instr(P.LTU, 3)]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 32, 64), 3, rounds=3)
    assert log[0][0] > 0 and len(log[0][1]) == 1


def test_repeated_memory(cozk, LK, ctxs):
    table = [P.Instr(P.PRODUCT, [2, 2, 0]), P.Instr(P.CONCAT, [1, 1, 1, 0], 8)]
    _drive(cozk, LK, ctxs, PR.Instance(table, 32, 65), 5, rounds=3)


@pytest.mark.parametrize("k", [3, 7, 9])
def test_all_rounds_down_to_length_2(cozk, LK, ctxs, k):
    table = [PR.form_instr(P.UNSIGNED_REM, 3), PR.form_instr(P.SIGNED_REM, 2, first=2), P.Instr(P.CONCAT, [0], 0)]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 32, 66), k)
    assert len(log) == 5 and log[-1][0] > 0


@pytest.mark.parametrize("form,C", PR.PAIRS, ids=PR.PAIR_IDS)
def test_every_form_at_every_chunk_count(cozk, LK, ctxs, form, C):
    """all 51 admitted (form, chunk count) pairs at n = 64, k = 3: round 0 (0/1 flags) and round 1 (bound flags)"""
    assert len(PR.PAIRS) == 51
    inst = PR.Instance(PR.pair_table(form, C), 64, 3000 + 16 * form + C)
    log = _drive(cozk, LK, ctxs, inst, 3, rounds=2)
    assert log[0][0] > 0 and len(log[0][1]) == PR.levels(inst.instrs[0])


def test_nine_members_past_one_workgroup(cozk, LK, ctxs):
    """k = 9, t = 4: the degree is a run-time value in the deal kernel (coefficients through the shift register); 257 items"""
    log = _drive(cozk, LK, ctxs, _exact_items(1024, 257, 357), 9, rounds=1)
    assert log[0] == (257, [5 * 257])


# ------------------------------------------------------------------------------------------------ c. refusals
def _refused(cozk, text, fn):
    with pytest.raises(cozk.CozkError) as err:
        fn()
    assert err.value.code == INVALID and text in str(err.value), str(err.value)


def test_refusals_leave_every_member_as_it_was(cozk, LK, ctxs):
    """every refusal of create and of the calls; after the refused calls the round goes on and every member still matches its twin"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 3, first=1), P.Instr(P.CONCAT, [3, 0], 8)]
    other = [P.Instr(P.PRODUCT, [0, 1, 3]), PR.form_instr(P.SLT, 3, first=1), P.Instr(P.CONCAT, [3, 0], 8)]
    inst = PR.Instance(table, 16, 81)
    rig = Rig(cozk, LK, ctxs, inst, 3)
    ctx = ctxs[0]
    rows, keys = PR.rows(LK, table), rig.keys
    plain = lambda tbl, E, outs, eq, flags: PR.create(cozk, LK, ctx, cozk.MODE_PLAIN, 0, PR.rows(LK, tbl), flags, E, outs, eq)
    odd_table = plain(other, rig.E[0], rig.outs[0], inst.eq, inst.flags)
    short = plain(table, [m[:8] for m in rig.E[0]], rig.outs[0][:8], inst.eq[:8], [f[:8] for f in inst.flags])
    rep3 = PR.create(cozk, LK, ctx, cozk.MODE_REP3, 0, rows, inst.flags, inst.E3[0], inst.outs3[0], inst.eq)
    extra = [plain(table, rig.E[0], rig.outs[0], inst.eq, inst.flags) for _ in range(2)]
    m = rig.members
    group = lambda members, ks=keys: LK.PrimaryGroup(ctx, members, ks)
    try:
        T = "primary_group_create: "
        _refused(cozk, T + "every member must have the same instruction table", lambda: group([m[0], m[1], odd_table]))
        _refused(cozk, T + "every member must have the same length", lambda: group([m[0], m[1], short]))
        _refused(cozk, T + "every member must be PLAIN", lambda: group([m[0], rep3, m[2]]))
        _refused(cozk, T + "duplicate member", lambda: group([m[0], m[1], m[0]]))
        _refused(cozk, T + "null member", lambda: group([m[0], None, m[2]]))
        _refused(cozk, T + "k = 2t + 1", lambda: group(m + extra[:1], _keys(5)[:4]))
        _refused(cozk, T + "k = 2t + 1", lambda: group(m[:1], [[]]))
        # a round with refused calls in it
        ref = rig.begin()
        assert ref.n_levels == 2
        for level in (0, 3, 5, -1):
            _refused(cozk, "primary_group_level: bad level / no items", lambda: rig.group.level(level, 0))
        _refused(cozk, "primary_group_level_buffer: bad level", lambda: rig.group.level_buffer(0, 3))
        _refused(cozk, "primary_group_level_buffer: bad argument", lambda: rig.group.level_buffer(3, 1))
        # members whose item counts differ: a group over two begun members and one that was not
        mixed = group([m[0], m[1], extra[0]])
        _refused(cozk, "primary_group_level: every member must have the same item count", lambda: mixed.level(1, 0))
        _refused(cozk, "primary_group_round_finish: every member must have the same item count", lambda: mixed.round_finish())
        # ... and whose lengths differ after a bind
        extra[0].round_begin()
        extra[0].round_begin(12345)
        _refused(cozk, "primary_group_level: every member must have the same length", lambda: mixed.level(1, 0))
        mixed.free()
        elems = [rig.level(level) for level in (1, 2)]
        assert all(e > 0 for e in elems)
        _refused(cozk, "primary_group_level: bad level / no items", lambda: rig.group.level(3, 0))
        rig.finish()
        rig.round(777)  # and the next round as if nothing had been asked
    finally:
        for pr in [odd_table, short, rep3] + extra:
            pr.free()
        rig.free()


def test_counter_moves_the_dealing_not_the_sharing(cozk, LK, ctxs):
    """two groups over equal members at different counters: every level buffer differs, any t + 1 members open the same slot values"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), P.Instr(P.CONCAT, [3, 0], 8)]
    inst = PR.Instance(table, 16, 91)
    rigs = [Rig(cozk, LK, ctxs, inst, 3, counter=c) for c in (0, 1 << 33)]
    try:
        bufs = []
        for rig in rigs:
            rig.begin()
            assert rig.level(1) > 0
            bufs.append([list(b[0]) for b in rig.ref.bufs])
            rig.finish()
        lam = S.lagrange_from_coeff([1, 2])
        assert all(a != b for a, b in zip(bufs[0], bufs[1]))
        opened = [[S.reconstruct([b[0][i], b[1][i]], lam) for i in range(len(b[0]))] for b in bufs]
        assert opened[0] == opened[1]
    finally:
        for rig in rigs:
            rig.free()
