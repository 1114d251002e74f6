"""GPU: the public exchange plan (cozk_primary_plan) and the king level exchange of the primary level groups
(cozk_primary_group_create_king, cozk_primary_group_level_king, cozk_primary_group_staging_bytes; csrc/primary_group.inc) driven
directly.  k = 2t + 1 PLAIN cozk_primary members on contexts of their own; a twin set is driven per member (cozk_primary_level), which
gives every sender's local slot values z_m.  Everything is integer work: every comparison is ==.
  after EVERY king level   every member's level buffer == sum_m lambda_m (z_m + r2t_m[off + pos]) - rt_q[off + pos] in Python integers
                           (the identity is linear, so it is checked on the Montgomery residues the device stores: canonical, < R)
  the plan                 == the n_elems the resharing level calls report in every round of a full run"""
import importlib

import numpy as np
import pytest

import primary_ref as PR
import pylookups as PL
import pyprimary as P
import pyref as O
import shamir_primary_king_ref as KR
import shamir_ref as S

pytestmark = pytest.mark.gpu
R = O.R
INVALID = -1
KMAX = 9
N_MEM = 20  # the lookups table indexes its memories modulo n_mem: 18 is the widest row


@pytest.fixture(scope="module")
def LK():
    return importlib.import_module("co-zkvms_amd.lookups")


@pytest.fixture(scope="module")
def ctxs(cozk):
    """one context per member, all on device 0; the first is the driver, the last owns nothing but halves"""
    cs = [cozk.Context(0) for _ in range(KMAX + 1)]
    yield cs
    for c in cs:
        c.close()


class Inst:
    """public flags and eq, and per member ANY columns: the exchange is checked against the members' own local values"""

    def __init__(self, instrs, flags, seed):
        self.instrs, self.flags, self.n = list(instrs), [list(f) for f in flags], len(flags[0])
        self.log_n = self.n.bit_length() - 1
        self.n_mem = max(max(i.mems) for i in instrs) + 1
        self.eq = O.eq_evals([O.SplitMix64(seed).field() for _ in range(self.log_n)])
        self.seed = seed

    def columns(self, p):
        rng = O.SplitMix64(1000 * self.seed + p)
        return [[rng.field() for _ in range(self.n)] for _ in range(self.n_mem)], [rng.field() for _ in range(self.n)]


def lookups_inst(log_n, mix, seed=6):
    n = 1 << log_n
    instrs = PL.instr_table(N_MEM)
    which = [PL.mix_instr(mix, v) for v in O.synthetic_small(seed + 1234567, n, 8)]
    return Inst(instrs, [[1 if which[x] == i else 0 for x in range(n)] for i in range(len(instrs))], seed)


def small_inst(table, n, seed, zero_flags=()):
    return Inst(table, PR.Instance(table, n, seed, zero_flags=zero_flags).flags, seed)


def device_plan(cozk, LK, ctx, inst):
    fl = [cozk.Vec.from_ints(ctx, f, kind=cozk._lib.SCALAR_U8) for f in inst.flags]
    try:
        return LK.primary_plan(ctx, PR.rows(LK, inst.instrs), fl, inst.log_n)
    finally:
        for v in fl:
            v.free()


def residues(cozk, ctx, ptr, n):
    """n stored field elements at a device address as a numpy array of Python integers (the Montgomery residues, as stored)"""
    host = np.zeros((max(n, 1), 4), dtype=np.uint64)
    PR._copy(cozk, ctx, host.ctypes.data, ptr, 32 * n)
    o = host[:n].astype(object)
    return o[:, 0] | (o[:, 1] << 64) | (o[:, 2] << 128) | (o[:, 3] << 192)


class KingRig:
    """k members + k twins on ctxs[0..k), the group on ctxs[0] (keyless unless keyed), the halves of one pair of `length` elements on
    their members' contexts or all on `halves_ctx`"""

    def __init__(self, cozk, LK, ctxs, inst, k, length, keyed=False, halves_ctx=None, offset=0):
        self.cozk, self.LK, self.k, self.t, self.inst = cozk, LK, k, (k - 1) // 2, inst
        self.ctxs = list(ctxs[:k])
        rows = PR.rows(LK, inst.instrs)
        cols = [inst.columns(p) for p in range(k)]
        mk = lambda p: PR.create(cozk, LK, self.ctxs[p], cozk.MODE_PLAIN, 0, rows, inst.flags, cols[p][0], cols[p][1], inst.eq)
        self.members = [mk(p) for p in range(k)]
        self.twins = [mk(p) for p in range(k)]
        keys = [[O.harness_prf_key(3, 64 * p + c) for c in range(self.t)] for p in range(k)]
        self.group = LK.PrimaryGroup(self.ctxs[0], self.members, keys if keyed else None)
        self.rt = [cozk.Vec.random(halves_ctx or self.ctxs[p], length, 7000 + p) for p in range(k)]
        self.r2t = [cozk.Vec.random(halves_ctx or self.ctxs[p], length, 8000 + p) for p in range(k)]
        for c in ctxs:
            c.synchronize()  # the halves are read on the driver's stream: ordering that read is the caller's job
        self.off = offset
        self.lam = S.lagrange_from_coeff(list(range(1, k + 1)))
        self.largest = 0

    def begin(self, r=None):
        begun = [pr.round_begin(r) for pr in self.members + self.twins]
        assert all(b == begun[0] for b in begun), begun
        return begun[0]

    def half(self, v, n):
        return residues(self.cozk, v.ctx, v.device_ptr() + 32 * self.off, n)

    def level(self, level, sync=False):
        """one king level, checked member by member; the twins receive what the members received -> n_elems"""
        k = self.k
        local = [tw.level(level) for tw in self.twins]
        n_el = local[0][2]
        assert all(o[2] == n_el and o[1] is None for o in local)
        assert all(m.level_elems(level) == n_el for m in self.members)
        if sync:
            for c in self.ctxs:
                c.synchronize()
        assert self.group.level_king(level, self.rt, self.r2t, self.off) == n_el
        if not n_el:
            assert all(self.group.level_buffer(p, level) == (None, 0) for p in range(k))
            return 0
        self.largest = max(self.largest, n_el)
        masked = [(residues(self.cozk, self.ctxs[m], local[m][0], n_el) + self.half(self.r2t[m], n_el)) % R for m in range(k)]
        zed = sum(self.lam[m] * masked[m] for m in range(k)) % R
        for q in range(k):
            buf, nb = self.group.level_buffer(q, level)
            assert nb == n_el and buf is not None
            got = residues(self.cozk, self.ctxs[q], buf, n_el)
            assert (got < R).all(), ("canonical", level, q)
            assert (got == (zed - self.half(self.rt[q], n_el)) % R).all(), ("level buffer", level, q)
            PR._copy(self.cozk, self.ctxs[q], local[q][0], buf, 32 * n_el)  # the twin receives what the member received
        self.off += n_el
        return n_el

    def finish(self):
        rows = self.group.round_finish()
        assert rows == [tw.round_finish() for tw in self.twins]

    def round(self, r=None):
        n_items, n_levels = self.begin(r)
        elems = [self.level(level) for level in range(1, n_levels + 1)]
        self.finish()
        return elems

    def snapshot(self, levels):
        """the bytes of every member's level buffers"""
        def raw(p, lv):
            buf, n = self.group.level_buffer(p, lv)
            host = np.zeros((max(n, 1), 4), dtype=np.uint64)
            if n:
                PR._copy(self.cozk, self.ctxs[p], host.ctypes.data, buf, 32 * n)
            return host[:n].tobytes()

        return [[raw(p, lv) for lv in levels] for p in range(self.k)]

    def free(self):
        self.group.free()
        for x in self.members + self.twins + self.rt + self.r2t:
            x.free()


def drive(cozk, LK, ctxs, inst, k, rounds=None, offset=0, extra=0, **kw):
    """every round (or the first `rounds`) through king levels at running offsets -> (elems per round, the plan's rows, the rig's
    largest level, staging bytes at the end)"""
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    rig = KingRig(cozk, LK, ctxs, inst, k, offset + total + extra, offset=offset, **kw)
    try:
        rng = O.SplitMix64(9)
        r, log = None, []
        for j in range(inst.log_n if rounds is None else rounds):
            log.append(rig.round(r))
            r = rng.field()
        if rounds is None:
            assert rig.off == offset + total  # every pair element was used once
        return log, rows, rig.largest, rig.group.staging_bytes()
    finally:
        rig.free()


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("log_n,mix", [(5, 0), (5, 1), (11, 0), (11, 1)], ids=["5-uniform", "5-sha2", "11-uniform", "11-sha2"])
def test_plan_is_what_the_resharing_group_levels_report(cozk, LK, ctxs, log_n, mix):
    """a full run of k = 3 members through cozk_primary_group_level: the n_elems of every level of every round"""
    inst = lookups_inst(log_n, mix)
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    assert (rows, total) == KR.plan(inst.instrs, inst.flags, log_n)
    cols = inst.columns(0)
    table = PR.rows(LK, inst.instrs)
    members = [PR.create(cozk, LK, ctxs[p], cozk.MODE_PLAIN, 0, table, inst.flags, cols[0], cols[1], inst.eq) for p in range(3)]
    group = LK.PrimaryGroup(ctxs[0], members, [[O.harness_prf_key(3, 64 * p)] for p in range(3)])
    try:
        rng = O.SplitMix64(5)
        r, ctr, seen = None, 0, 0
        for rnd in range(log_n):
            begun = [m.round_begin(r) for m in members]
            n_levels = begun[0][1]
            got = [group.level(level, ctr + 100 * level) for level in range(1, n_levels + 1)]
            assert got + [0] * (LK.PRIMARY_MAX_LEVELS - n_levels) == rows[rnd], rnd
            assert [members[0].level_elems(level) for level in range(1, 5)] == rows[rnd]
            group.round_finish()
            seen += sum(got)
            ctr += 1000
            r = rng.field()
        assert seen == total > 0
    finally:
        group.free()
        for m in members:
            m.free()


def test_plan_with_a_zero_flag_column_and_with_one_instruction(cozk, LK, ctxs):
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 4), P.Instr(P.CONCAT, [0], 0)]
    inst = small_inst(table, 16, 72, zero_flags=(1,))
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    assert (rows, total) == KR.plan(table, inst.flags, 4) and all(row[0] > 0 and row[1:] == [0, 0, 0] for row in rows)
    log, _, _, _ = drive(cozk, LK, ctxs, inst, 3)
    assert [e + [0] for e in log] == rows  # three levels announced, two of them empty, in every round
    one = Inst([P.Instr(P.PRODUCT, [0, 1, 2])], [[1, 0, 0, 0, 0, 0, 1, 1]], 3)
    assert device_plan(cozk, LK, ctxs[0], one) == ([[10, 0, 0, 0], [10, 0, 0, 0], [5, 0, 0, 0]], 25)
    log, _, _, _ = drive(cozk, LK, ctxs, one, 3)
    assert log == [[10], [10], [5]]
    lin = Inst([P.Instr(P.CONCAT, [0], 0)], [[1] * 8], 4)
    assert device_plan(cozk, LK, ctxs[0], lin) == ([[0] * 4] * 3, 0)


# ------------------------------------------------------------------------------------------------ level_king values
@pytest.mark.parametrize("k,offset,other_ctx", [(3, 0, False), (5, 7, False), (9, 3, True)], ids=["k3", "k5-odd-offset", "k9-other-context"])
def test_every_level_of_every_round_at_log_n_4(cozk, LK, ctxs, k, offset, other_ctx):
    """the lookups table at 16 cycles, all rounds down to length 2 (a level that holds nothing is announced and skipped: the table's
    fourth level never holds anything); halves longer than needed; k = 9 has no degree template in the king kernels and runs for the
    pointer tables"""
    inst = lookups_inst(4, 0)
    log, rows, largest, staging = drive(cozk, LK, ctxs, inst, k, offset=offset, extra=5, halves_ctx=ctxs[KMAX] if other_ctx else None)
    assert [e + [0] * (4 - len(e)) for e in log] == rows and sum(map(sum, rows)) > 0
    assert staging == k * largest * 32


@pytest.mark.parametrize("keyed", [False, True], ids=["keyless", "keyed-group"])
def test_several_item_blocks_and_element_blocks_at_log_n_11(cozk, LK, ctxs, keyed):
    """2048 cycles of the uniform mix: more than one item block per (point, member) in the mask kernel, more than one element block in
    the finish; the first three rounds, at an odd offset"""
    inst = lookups_inst(11, 0)
    log, rows, largest, staging = drive(cozk, LK, ctxs, inst, 3, rounds=3, offset=1, keyed=keyed)
    assert [e + [0] * (4 - len(e)) for e in log] == rows[:3]
    assert max(log[0]) > 256 * 8 and largest == max(max(e) for e in log)  # > 256 items x D
    assert staging == 3 * largest * 32  # [k][n_elems], not [k][k][n_elems]


def test_resharing_levels_on_the_same_group_need_the_larger_staging_block(cozk, LK, ctxs):
    inst = lookups_inst(5, 0)
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    rig = KingRig(cozk, LK, ctxs, inst, 3, total, keyed=True)
    try:
        n_levels = rig.begin()[1]
        n1 = rig.level(1)
        assert rig.group.staging_bytes() == 3 * n1 * 32
        assert rig.group.level(1, 0) == n1  # the resharing form of the same level
        assert rig.group.staging_bytes() == 9 * n1 * 32
    finally:
        rig.free()


# ------------------------------------------------------------------------------------------------ streams
def test_a_king_level_right_behind_round_begin_reads_what_the_members_streams_wrote(cozk, LK, ctxs):
    """every member lives on a context of its own and round_begin returns with launches still enqueued there: a king level issued
    right behind it gives the bytes of one issued after every stream was synchronised (the rig checks both against the formula)"""
    inst = lookups_inst(8, 0)
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    snaps = []
    for sync in (False, True):
        rig = KingRig(cozk, LK, ctxs, inst, 3, total)
        try:
            for c in ctxs:
                c.synchronize()
            begun = [pr.round_begin(None) for pr in rig.twins + rig.members]  # the members last: their streams are the busiest
            if sync:
                for c in ctxs:
                    c.synchronize()
            n_el = rig.group.level_king(1, rig.rt, rig.r2t, 0)
            assert n_el == rows[0][0] > 0
            snaps.append(rig.snapshot([1]))
            assert begun[0][1] >= 1
        finally:
            rig.free()
    assert snaps[0] == snaps[1]
    # the same level through the checked path: the twins' local values, the formula
    rig = KingRig(cozk, LK, ctxs, inst, 3, total)
    try:
        rig.begin()
        assert rig.level(1) == rows[0][0]
        assert rig.snapshot([1]) == snaps[0]
    finally:
        rig.free()


# ------------------------------------------------------------------------------------------------ refusals
def _refused(cozk, text, fn):
    with pytest.raises(cozk.CozkError) as err:
        fn()
    assert err.value.code == INVALID and text in str(err.value), str(err.value)


def test_refusals_leave_every_member_as_it_was(cozk, LK, ctxs):
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 3, first=1), P.Instr(P.CONCAT, [3, 0], 8)]
    inst = small_inst(table, 16, 81)
    rows, total = device_plan(cozk, LK, ctxs[0], inst)
    rig = KingRig(cozk, LK, ctxs, inst, 3, total)
    cols = inst.columns(0)
    extra = PR.create(cozk, LK, ctxs[0], cozk.MODE_PLAIN, 0, PR.rows(LK, table), inst.flags, cols[0], cols[1], inst.eq)
    short = cozk.Vec.random(ctxs[0], rows[0][0] + 2, 1)
    u8 = cozk.Vec.from_ints(ctxs[0], [1] * total, kind=cozk._lib.SCALAR_U8)
    g, T = rig.group, "primary_group_level_king: "
    try:
        assert rig.begin()[1] == 2
        assert rig.level(1) == rows[0][0]  # the level buffers hold values from here on
        before = rig.snapshot([1, 2])
        _refused(cozk, "primary_group_level: the group has no PRF keys", lambda: g.level(1, 0))
        _refused(cozk, T + "r_offset + n_elems <= len of every half", lambda: g.level_king(1, rig.rt, rig.r2t, total - rows[0][0] + 1))
        _refused(cozk, T + "r_offset + n_elems <= len of every half", lambda: g.level_king(1, rig.rt, rig.r2t, 2 ** 64 - 1))
        _refused(cozk, T + "r_offset + n_elems <= len of every half", lambda: g.level_king(1, rig.rt[:2] + [short], rig.r2t, 3))
        _refused(cozk, T + "r_offset + n_elems <= len of every half", lambda: g.level_king(1, rig.rt, [short] + rig.r2t[1:], 3))
        _refused(cozk, T + "2 (2t + 1) FR halves", lambda: g.level_king(1, rig.rt, rig.r2t[:2] + [None], 0))
        _refused(cozk, T + "2 (2t + 1) FR halves", lambda: g.level_king(1, [None] + rig.rt[1:], rig.r2t, 0))
        _refused(cozk, T + "2 (2t + 1) FR halves", lambda: g.level_king(1, rig.rt, rig.r2t[:2] + [u8], 0))
        for level in (0, 3, 5, -1):
            _refused(cozk, T + "bad level / no items", lambda: g.level_king(level, rig.rt, rig.r2t, 0))
        mixed = LK.PrimaryGroup(ctxs[0], [rig.members[0], rig.members[1], extra], None)  # two begun members and one that was not
        _refused(cozk, T + "every member must have the same item count", lambda: mixed.level_king(1, rig.rt, rig.r2t, 0))
        mixed.free()
        _refused(cozk, "primary_group_create_king: duplicate member", lambda: LK.PrimaryGroup(ctxs[0], [rig.members[0], rig.members[1], rig.members[0]], None))
        _refused(cozk, "primary_group_create_king: k = 2t + 1", lambda: LK.PrimaryGroup(ctxs[0], rig.members[:2], None))
        assert rig.snapshot([1, 2]) == before
        assert rig.level(2) == rows[0][1] > 0  # and the round goes on as if nothing had been asked
        rig.finish()
        rig.round(777)
    finally:
        for x in (extra, short, u8):
            x.free()
        rig.free()


def test_a_level_call_without_items_is_refused(cozk, LK, ctxs):
    table = [P.Instr(P.CONCAT, [0, 1], 8), P.Instr(P.NOT_FIRST, [1]), P.Instr(P.ZERO, [0])]
    inst = small_inst(table, 16, 73)
    rig = KingRig(cozk, LK, ctxs, inst, 3, 4)
    try:
        assert rig.begin() == (0, 0)
        _refused(cozk, "primary_group_level_king: bad level / no items", lambda: rig.group.level_king(1, rig.rt, rig.r2t, 0))
        assert rig.group.staging_bytes() == 0
        rig.finish()  # the members still are their twins
    finally:
        rig.free()
