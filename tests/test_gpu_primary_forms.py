"""GPU: the primary sumcheck (cozk_primary_*, csrc/primary_sumcheck.inc) driven directly, round by round, at every collation
form and chunk count that cozk_primary_create admits, at sumcheck degrees 3 .. 8, and at the edges of its item lists and
levels.  Everything is integer work: every comparison is ==.
Expected round messages: oracle/pyprimary.py's prover_message (plain prover, or the sum of three Rep3 parties) AND the direct sum
  sum over index pairs of eq(X) (sum_i flag_i(X) g_i(E(X)) - out(X))  from g_plain alone (tests/primary_ref.py);
tests/test_primary_forms_model.py pins the two against each other on the CPU.  Binds are local, so the final evaluations are
compared per party with that party's bound shares.  Rep3 = three cozk_primary on three contexts of device 0 in lock-step,
the ring reshare of every level done by cozk_copy (tests/primary_ref.py Run)."""
import importlib

import pytest

import primary_ref as PR
import pyprimary as P
import pyref as O

pytestmark = pytest.mark.gpu
R = O.R
MODES = {"plain": 1, "rep3": 3}
INVALID = -1  # COZK_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def LK():
    return importlib.import_module("co-zkvms_amd.lookups")


@pytest.fixture(scope="module")
def ctxs(cozk):
    """the three parties' contexts, all on device 0; the plain prover runs on the first"""
    cs = [cozk.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def _expected_levels(instrs, n_items):
    return max(PR.levels(i) for i in instrs) if n_items else 0


def _drive(cozk, LK, ctxs, inst, nparties, seed=9, **kw):
    """all rounds and the final evaluations of one instance against the oracle; returns per round (n_items, n_levels, n_elems)"""
    E, outs = inst.parties(nparties)
    ref = PR.RefState.of(inst, nparties)
    run = PR.Run(cozk, LK, ctxs, inst.instrs, inst.eq, inst.flags, E, outs, **kw)
    log = []
    try:
        D = P.sumcheck_degree(inst.instrs)
        assert run.degree() == D
        assert all(len(pr) == inst.n for pr in run.prims)
        rng = O.SplitMix64(seed)
        r = None
        for j in range(inst.n.bit_length() - 1):
            msgs, n_items, n_levels, elems = run.round(r)
            want = ref.total()
            assert all(len(m) == D for m in msgs)
            assert PR.total(msgs) == want, ("round", j)
            assert want == ref.direct(), ("round", j)
            assert n_items == ref.n_items(), ("round", j)
            assert n_levels == _expected_levels(inst.instrs, n_items), ("round", j)
            log.append((n_items, n_levels, elems))
            r = rng.field()
            ref.bind(r)
        got = run.finals(r)
        for p in range(nparties):
            Ee, Fe, oe, qe = ref.finals(p)
            assert got[p] == (Ee, Fe, oe, qe), ("party", p)
        assert all(len(pr) == 1 for pr in run.prims)
    finally:
        run.free()
    return log


# ------------------------------------------------------------------------------------------------ a. every (form, C) pair
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form,C", PR.PAIRS, ids=PR.PAIR_IDS)
def test_every_form_at_every_chunk_count(cozk, LK, ctxs, form, C, mode):
    table = PR.pair_table(form, C)
    assert P.sumcheck_degree(table) == table[0].g_degree() + 2
    inst = PR.Instance(table, 32, 3000 + 16 * form + C)
    log = _drive(cozk, LK, ctxs, inst, MODES[mode])
    assert log[0][0] > 0  # the form ran


# ------------------------------------------------------------------------------------------------ b. linear forms, D = 3 .. 7
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [2, 4, 64])
@pytest.mark.parametrize("name", list(PR.LINEAR_TABLES))
def test_linear_tables_have_degree_3_and_no_items(cozk, LK, ctxs, name, n, mode):
    """CONCAT (1, 2, 13, 20 memories, bits 0, a repeated memory), NOT_FIRST (Rep3: the constant enters party 0's and party 1's
    sums only) and ZERO: three evaluations per round from the linear pass alone"""
    table = PR.LINEAR_TABLES[name]
    assert P.sumcheck_degree(table) == 3
    log = _drive(cozk, LK, ctxs, PR.Instance(table, n, 400 + n + len(name)), MODES[mode])
    assert all(entry == (0, 0, []) for entry in log)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("factors", [2, 3, 4, 5])
def test_degrees_4_to_7(cozk, LK, ctxs, factors, mode):
    table = [P.Instr(P.PRODUCT, range(factors)), P.Instr(P.CONCAT, [1, 0], 16)]
    assert P.sumcheck_degree(table) == factors + 2
    _drive(cozk, LK, ctxs, PR.Instance(table, 32, 500 + factors), MODES[mode])


# ------------------------------------------------------------------------------------------------ c. level edges
@pytest.mark.parametrize("mode", list(MODES))
def test_level_free_table_has_items_and_no_levels(cozk, LK, ctxs, mode):
    """PRODUCT of 2, LTU C = 2, DIV0 C = 1 and 2: products only in the last, local step -- no level buffer exists at all"""
    table = [P.Instr(P.PRODUCT, [0, 1]), P.Instr(P.LTU, [1, 2, 3]), P.Instr(P.DIV0, [2, 0]), P.Instr(P.DIV0, [0, 1, 2, 3])]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 32, 61), MODES[mode])
    assert all(n_items > 0 and n_levels == 0 for n_items, n_levels, _ in log)


@pytest.mark.parametrize("mode", list(MODES))
def test_active_level_free_beside_inactive_deep(cozk, LK, ctxs, mode):
    """PRODUCT of 2 has items, SIGNED_REM C = 4 (three levels) has all-zero flags: three levels are announced, nothing is
    exchanged at any of them; zero flags stay zero under the binds, so every round looks the same"""
    table = [P.Instr(P.PRODUCT, [0, 1]), PR.form_instr(P.SIGNED_REM, 4)]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 32, 62, zero_flags=(1,)), MODES[mode])
    assert all(n_items > 0 and n_levels == 3 and elems == [0, 0, 0] for n_items, n_levels, elems in log)


@pytest.mark.parametrize("mode", list(MODES))
def test_no_items_refuses_levels_and_finishes(cozk, LK, ctxs, mode):
    """a multiplicative instruction whose flags are all zero: no items, no levels, cozk_primary_level is refused, the rounds
    are those of the linear pass"""
    nparties = MODES[mode]
    table = [PR.form_instr(P.SLT, 3), P.Instr(P.CONCAT, [0, 1], 8)]
    inst = PR.Instance(table, 16, 63, zero_flags=(0,))
    E, outs = inst.parties(nparties)
    ref = PR.RefState.of(inst, nparties)
    run = PR.Run(cozk, LK, ctxs, table, inst.eq, inst.flags, E, outs)
    try:
        rng = O.SplitMix64(1)
        r = None
        for j in range(4):
            for p, pr in enumerate(run.prims):
                assert pr.round_begin(r) == (0, 0)
                with pytest.raises(cozk.CozkError) as err:
                    pr.level(1, run.keys[p], run.keys[(p + 2) % 3], 0)
                assert err.value.code == INVALID and "primary_level: bad level / no items" in str(err.value)
            assert PR.total([pr.round_finish() for pr in run.prims]) == ref.total() == ref.direct(), j
            r = rng.field()
            ref.bind(r)
        got = run.finals(r)
        assert all(got[p] == ref.finals(p) for p in range(nparties))
    finally:
        run.free()


@pytest.mark.parametrize("mode", list(MODES))
def test_instruction_index_63(cozk, LK, ctxs, mode):
    """64 instructions: the live mask's top bit is a multiplicative instruction, the bit below it a linear one"""
    table = [P.Instr(P.ZERO, [0]) for _ in range(62)] + [P.Instr(P.CONCAT, [3, 4], 8), PR.form_instr(P.LTU, 3)]
    log = _drive(cozk, LK, ctxs, PR.Instance(table, 32, 64), MODES[mode])
    assert log[0][0] > 0 and log[0][1] == 1


@pytest.mark.parametrize("mode", list(MODES))
def test_repeated_memory(cozk, LK, ctxs, mode):
    """PRODUCT over [m, m, k] (a square) and the MOVSIGN-style CONCAT that lists one memory several times"""
    table = [P.Instr(P.PRODUCT, [2, 2, 0]), P.Instr(P.CONCAT, [1, 1, 1, 0], 8)]
    _drive(cozk, LK, ctxs, PR.Instance(table, 32, 65), MODES[mode])


def test_masks_change_the_exchange_and_nothing_else(cozk, LK, ctxs):
    """SLT C = 3 in Rep3 with the parties' keys, then with key_self == key_prev on every party (a zero mask): what goes over
    the ring at round 0, level 1 differs on every party, its position-wise sum over the parties and every message do not"""
    table = [PR.form_instr(P.SLT, 3), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, 32, 66)
    ref = PR.RefState.of(inst, 3)
    runs = [PR.Run(cozk, LK, ctxs, table, inst.eq, inst.flags, inst.E3, inst.outs3, capture=(0, 1), keys=keys)
            for keys in (None, [O.harness_prf_key(7, 0)] * 3)]
    try:
        rng = O.SplitMix64(2)
        r = None
        for j in range(5):
            outs = [run.round(r) for run in runs]
            assert outs[0][1:] == outs[1][1:]
            assert PR.total(outs[0][0]) == PR.total(outs[1][0]) == ref.total(), j
            r = rng.field()
            ref.bind(r)
        masked, bare = runs[0].captured, runs[1].captured
        n = len(masked[0])
        assert n > 0 and all(len(c) == n for c in masked + bare)
        for p in range(3):
            assert masked[p] != bare[p]
            assert sum(1 for a, b in zip(masked[p], bare[p]) if a != b) == n  # a PRF difference is zero with probability 2^-254
        assert PR.total(masked) == PR.total(bare)
        got = [run.finals(r) for run in runs]
        assert got[0] == got[1] and all(got[0][p] == ref.finals(p) for p in range(3))
    finally:
        for run in runs:
            run.free()


# ------------------------------------------------------------------------------------------------ d. one mixed table, n = 2048
MIXED_N = 2048
MIXED = [P.Instr(P.CONCAT, [0, 1, 2, 3], 8), P.Instr(P.NOT_FIRST, [4]), P.Instr(P.ZERO, [5]), P.Instr(P.PRODUCT, [6, 7, 6]),
         PR.form_instr(P.SLT, 3, first=8), PR.form_instr(P.SIGNED_REM, 2, first=10), PR.form_instr(P.LTU, 6, first=0)]


@pytest.fixture(scope="module")
def mixed():
    """the instance and its reference, computed once and only read by the tests below: per round the message (three-party
    prover_message == direct sum) and the item count; after the first bind the whole state of both provers (what the
    FR-flag runs are created from); at the end every party's final evaluations"""
    inst = PR.Instance(MIXED, MIXED_N, 2048, n_mem=20, one_hot=True)
    assert inst.n_mem == 20 and P.sumcheck_degree(MIXED) == 8
    states = {1: PR.RefState.of(inst, 1), 3: PR.RefState.of(inst, 3)}
    rng = O.SplitMix64(11)
    rs, msgs, items, bound = [], [], [], {}
    for j in range(MIXED_N.bit_length() - 1):
        want = states[3].total()
        assert want == states[3].direct(), j
        msgs.append(want)
        items.append(states[3].n_items())
        rs.append(rng.field())
        for st in states.values():
            st.bind(rs[-1])
        if j == 0:
            bound = {k: PR.RefState(MIXED, st.eq, st.flags, st.E, st.outs) for k, st in states.items()}
    finals = {k: [st.finals(p) for p in range(k)] for k, st in states.items()}
    return dict(inst=inst, rs=rs, msgs=msgs, items=items, bound=bound, finals=finals)


def _replay(run, mixed, first, nparties):
    r = None
    for j in range(first, len(mixed["rs"])):
        msgs, n_items, n_levels, elems = run.round(r)
        assert PR.total(msgs) == mixed["msgs"][j], ("round", j)
        assert n_items == mixed["items"][j] and n_levels == 4, ("round", j)  # LTU C = 6 is the deepest
        assert len(elems) == 4 and all(e > 0 for e in elems)
        r = mixed["rs"][j]
    got = run.finals(r)
    assert all(got[p] == mixed["finals"][nparties][p] for p in range(nparties))


@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_table_2048(cozk, LK, ctxs, mixed, mode):
    """seven instructions of every kind over 20 shared memories, one-hot flags: four workgroups in the linear pass, item groups
    of more than 256, more than one block partial in both reductions; after round 0 the bound flags make almost every
    instruction live at every index"""
    nparties = MODES[mode]
    inst = mixed["inst"]
    assert all(PR.count_items([ins], [f]) > 256 for ins, f in zip(MIXED, inst.flags) if ins.form not in PR.LINEAR)
    E, outs = inst.parties(nparties)
    run = PR.Run(cozk, LK, ctxs, MIXED, inst.eq, inst.flags, E, outs)
    try:
        assert run.degree() == 8
        _replay(run, mixed, 0, nparties)
    finally:
        run.free()


@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_table_created_from_bound_flags(cozk, LK, ctxs, mixed, mode):
    """the already-bound path: the flags bound once on the host and handed over as FR vectors, everything else bound alike --
    the primary of length 1024 gives rounds 1 .. of the run above"""
    nparties = MODES[mode]
    st = mixed["bound"][nparties]
    assert len(st.eq) == MIXED_N // 2
    run = PR.Run(cozk, LK, ctxs, MIXED, st.eq, st.flags, st.E, st.outs, flags_fr=True)
    try:
        _replay(run, mixed, 1, nparties)
    finally:
        run.free()


# ------------------------------------------------------------------------------------------------ e. refusals
T_LARGE = "primary: collation program too large (chunk count C too high for this form)"
T_FIT = "primary_create: the memory count does not fit the instruction form"
T_FORM = "primary_create: instruction form / memory count"
BAD_TABLES = {
    # just beyond the limits
    "product-7": ([(P.PRODUCT, range(7), 0)], T_LARGE),
    "ltu-C7": ([(P.LTU, range(13), 0)], T_LARGE),
    "lte-C7": ([(P.LTE, range(14), 0)], T_LARGE),
    "div0-C7": ([(P.DIV0, range(14), 0)], T_LARGE),
    "unsigned-rem-C7": ([(P.UNSIGNED_REM, range(20), 0)], T_LARGE),
    "slt-C5": ([(P.SLT, range(11), 0)], "primary_create: degree too high"),
    "signed-rem-22": ([(P.SIGNED_REM, list(range(20)) + [0, 1], 0)], T_FORM),
    # counts that fit no chunk count
    "ltu-2": ([(P.LTU, range(2), 0)], T_FIT),
    "slt-3": ([(P.SLT, range(3), 0)], T_FIT),
    "slt-6": ([(P.SLT, range(6), 0)], T_FIT),
    "lte-3": ([(P.LTE, range(3), 0)], T_FIT),
    "unsigned-rem-3": ([(P.UNSIGNED_REM, range(3), 0)], T_FIT),
    "signed-rem-6": ([(P.SIGNED_REM, range(6), 0)], T_FIT),
    "signed-rem-12": ([(P.SIGNED_REM, range(12), 0)], T_FIT),
    # other bad tables
    "form-13": ([(13, range(2), 0)], T_FORM),
    "no-memory": ([(P.PRODUCT, [], 0)], T_FORM),
    "21-memories": ([(P.CONCAT, list(range(20)) + [0], 0)], T_FORM),
    "memory-index-n_mem": ([(P.PRODUCT, [0, 20], 0)], "primary_create: memory index out of range"),
    "concat-shift-200": ([(P.CONCAT, range(11), 20)], "primary_create: CONCAT shift"),
    "65-instructions": ([(P.ZERO, [0], 0)] * 65, "primary_create: bad argument"),
    "33-multiplicative": ([(P.PRODUCT, [0, 1], 0)] * 33, "primary_create: at most 32 multiplicative instructions"),
}
GOOD = [P.Instr(P.PRODUCT, [0, 1]), P.Instr(P.CONCAT, [2, 3], 8)]  # the valid create that follows every refusal


@pytest.fixture(scope="module")
def base(cozk, ctxs):
    """plain columns of length 8 on the first context, shared by the refusal tests and only read"""
    ctx = ctxs[0]
    inst = PR.Instance(GOOD, 8, 90, n_mem=20)
    Vec, Poly = cozk.Vec, cozk.Rep3DensePolynomial
    d = dict(ctx=ctx, inst=inst, flag=Vec.from_ints(ctx, inst.flags[0], kind=cozk.SCALAR_U8), flag2=Vec.from_ints(ctx, inst.flags[1], kind=cozk.SCALAR_U8),
             E=[Poly.new(ctx, m) for m in inst.E], outs=Poly.new(ctx, inst.outs), eq=Vec.from_ints(ctx, inst.eq),
             first=PR.RefState.of(inst, 1).total())
    assert d["first"] == PR.RefState.of(inst, 1).direct()
    yield d
    for x in [d["flag"], d["flag2"], d["outs"], d["eq"]] + d["E"]:
        x.free()


def _refused(cozk, text, fn):
    with pytest.raises(cozk.CozkError) as err:
        fn()
    assert err.value.code == INVALID and text in str(err.value), str(err.value)


def _valid_create_still_works(cozk, LK, base):
    pr = LK.PrimarySumcheck.create(base["ctx"], cozk.MODE_PLAIN, 0, PR.rows(LK, GOOD), [base["flag"], base["flag2"]], base["E"], base["outs"], base["eq"])
    try:
        assert pr.degree() == 4 and len(pr) == 8
        n_items, n_levels = pr.round_begin()
        assert (n_items, n_levels) == (PR.count_items(GOOD, base["inst"].flags), 0)
        assert pr.round_finish() == base["first"]
    finally:
        pr.free()


@pytest.mark.parametrize("name", list(BAD_TABLES))
def test_bad_table_is_refused(cozk, LK, base, name):
    spec, text = BAD_TABLES[name]
    table = [LK.PrimaryInstr.of(f, m, b) for f, m, b in spec]
    _refused(cozk, text, lambda: LK.PrimarySumcheck.create(base["ctx"], cozk.MODE_PLAIN, 0, table, [base["flag"]] * len(table), base["E"], base["outs"],
                                                           base["eq"]))
    _valid_create_still_works(cozk, LK, base)


def test_bad_inputs_are_refused(cozk, LK, base):
    ctx, inst = base["ctx"], base["inst"]
    Vec, Poly = cozk.Vec, cozk.Rep3DensePolynomial
    table = PR.rows(LK, GOOD)
    flags = [base["flag"], base["flag2"]]
    create = lambda fl=flags, E=base["E"], outs=base["outs"], eq=base["eq"]: LK.PrimarySumcheck.create(ctx, cozk.MODE_PLAIN, 0, table, fl, E, outs, eq)
    T_EQ = "primary_create: eq must be an FR vector of power-of-two length"
    eq1, eq6 = Vec.from_ints(ctx, inst.eq[:1]), Vec.from_ints(ctx, inst.eq[:6])
    shared_outs = Poly.new(ctx, inst.outs3[0])
    short = Poly.new(ctx, inst.E[5][:4])
    fr_flag = Vec.from_ints(ctx, inst.flags[1])
    cases = [(T_EQ, lambda: create(eq=eq1)), (T_EQ, lambda: create(eq=eq6)),
             ("primary_create: lookup_outputs shape / mode", lambda: create(outs=shared_outs)),
             ("primary_create: E polynomial shape / mode", lambda: create(E=base["E"][:5] + [short] + base["E"][6:])),
             ("primary_create: every flag column is a U8 vector of n entries", lambda: create(fl=[base["flag"], fr_flag])),
             ("primary_create: every flag vector has n entries of one kind", lambda: create(fl=[fr_flag, base["flag"]]))]
    for text, fn in cases:
        _refused(cozk, text, fn)
        _valid_create_still_works(cozk, LK, base)
    for x in (eq1, eq6, shared_outs, short, fr_flag):
        x.free()


def test_level_and_final_evals_out_of_turn_are_refused(cozk, LK, ctxs):
    """a level outside 1 .. n_levels, final_evals while more than one variable is unbound, final_evals twice: refused, and the
    rounds go on as if nothing had been asked"""
    table = [PR.form_instr(P.SLT, 3), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, 4, 91)
    ref = PR.RefState.of(inst, 1)
    run = PR.Run(cozk, LK, ctxs, table, inst.eq, inst.flags, [inst.E], [inst.outs])
    try:
        pr = run.prims[0]
        r0, r1 = 12345, R - 2
        n_items, n_levels = pr.round_begin()
        assert n_items > 0 and n_levels == 2
        for level in (0, 3, 5):
            _refused(cozk, "primary_level: bad level / no items", lambda: pr.level(level))
        T_FINAL = "primary_final_evals: one unbound variable must be left"
        _refused(cozk, T_FINAL, lambda: pr.final_evals(r0))
        assert len(pr) == 4
        for level in (1, 2):
            pr.level(level)
        # cozk_primary_round_finish without an output: its one refusal, and the whole message follows
        _refused(cozk, "primary_round_finish: bad argument", lambda: pr.ctx.check(pr._l.cozk_primary_round_finish(pr.ctx.h, pr.h, None)))
        assert pr.round_finish() == ref.total()
        ref.bind(r0)
        msgs, _, _, _ = run.round(r0)
        assert msgs[0] == ref.total()
        ref.bind(r1)
        assert pr.final_evals(r1) == ref.finals(0)
        _refused(cozk, T_FINAL, lambda: pr.final_evals(r1))
        assert len(pr) == 1
        _refused(cozk, "primary_round_begin: nothing left to sum", lambda: pr.round_begin())
        _refused(cozk, "primary_round_begin: fully bound", lambda: pr.round_begin(r0))
    finally:
        run.free()


@pytest.mark.parametrize("mode", list(MODES))
def test_round_begin_refusal_at_two_entries_leaves_the_primary_untouched(cozk, LK, ctxs, mode):
    """with two entries left the last challenge belongs to cozk_primary_final_evals: cozk_primary_round_begin with a challenge
    is refused BEFORE it binds -- the length stays 2, the round's message can still be read, and the final_evals that follows
    equals the twin's that saw no refusal and the oracle's.  (A level-free table: one party runs alone.)"""
    nparties = MODES[mode]
    party = 1 if nparties == 3 else 0
    table = [P.Instr(P.PRODUCT, [0, 1]), P.Instr(P.NOT_FIRST, [1])]
    inst = PR.Instance(table, 4, 92)
    E, outs = inst.parties(nparties)
    ref = PR.RefState.of(inst, nparties)
    m = cozk.MODE_PLAIN if nparties == 1 else cozk.MODE_REP3
    dev, twin = (PR.create(cozk, LK, ctxs[0], m, party, PR.rows(LK, table), inst.flags, E[party], outs[party], inst.eq) for _ in range(2))
    try:
        r0, r1 = 777, R - 5
        for pr in (dev, twin):
            assert pr.round_begin() == (ref.n_items(), 0)
        assert dev.round_finish() == twin.round_finish()
        ref.bind(r0)
        for pr in (dev, twin):
            assert pr.round_begin(r0) == (ref.n_items(), 0)
        last = twin.round_finish()
        assert dev.round_finish() == last
        assert len(dev) == 2
        _refused(cozk, "primary_round_begin: nothing left to sum", lambda: dev.round_begin(r1))
        assert len(dev) == 2
        assert dev.round_finish() == last
        ref.bind(r1)
        got = dev.final_evals(r1)
        assert got == twin.final_evals(r1) == ref.finals(party)
    finally:
        dev.free()
        twin.free()
