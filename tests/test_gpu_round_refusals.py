"""A refused call on a round handle changes nothing ("Refusals of the stateful calls").  cozk_outer_round and
cozk_prodlist_round bind with the previous challenge before they form the next message; every check of theirs comes before that
bind, so a call out of turn -- the last challenge handed to `round` instead of `final`, `final` too early, anything on a handle
that is fully bound -- is COZK_ERR_INVALID_ARG and leaves the handle where it was.

The pattern, for each handle: a SUBJECT and a TWIN from the same inputs; the twin never sees a refused call.  Both are driven to a
point, the subject is snapshot (length and download(), where the wrapper has them), the refused calls are made -- each must raise
CozkError with code COZK_ERR_INVALID_ARG and the expected text -- and the snapshot must not have moved.  Then the protocol goes on:
every later message and the final values of the subject equal the twin's and the Python oracle's (oracle/pyspartan_outer.py,
oracle/pylogup.py), bit for bit.  Every bad argument here is refused on the host; none reaches a kernel."""
import functools
import importlib

import numpy as np
import pytest

import pylogup as G
import pyref as O
import pyspartan_outer as S

pytestmark = pytest.mark.gpu
R = O.R
INVALID = -1  # COZK_ERR_INVALID_ARG (include/cozk.h)


def _refused(cozk, text, fn):
    with pytest.raises(cozk.CozkError) as err:
        fn()
    assert err.value.code == INVALID and text in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------------------ SpartanOuter
T_OUTER_LAST = "outer_round: nothing left to sum after this bind (the last challenge goes to cozk_outer_final_evals)"
T_OUTER_BOUND = "outer_round: fully bound"
T_OUTER_ARG = "outer_round: bad argument"
T_OUTER_FINAL = "outer_final_evals: one unbound variable must be left"
# the synthetic system has 8 rows per step: log_steps + 3 variables (3 to 6); 1 party: k_outer_round<1>, 3 parties: <2>
OUTER_CASES = [(log_steps, nparties) for log_steps in (0, 1, 3) for nparties in (1, 3)]


@functools.lru_cache(maxsize=None)
def _outer_oracle(log_steps, nparties):
    """the round loop of test_gpu_outer.py::test_rows_and_every_round_match_the_sparse_oracle on the oracle alone, computed once per
    shape: the inputs, every party's message and claim of every round, the challenges, every party's final claims"""
    n, seed = 1 << log_steps, 40 + log_steps
    uniform, cross, padded = S.synthetic_system()
    assert padded == 8
    polys = S.party_columns(seed, S.synthetic_columns(seed, n), nparties)
    rng = O.SplitMix64(17)
    nv = log_steps + 3
    tau = [rng.field() for _ in range(nv)]
    sparse = [S.build_sparse(uniform, cross, polys[p], padded, n, p) for p in range(nparties)]
    eqs = [S.GruenSplitEq(tau) for _ in range(nparties)]
    claims, msgs, rs = [[0] * nparties], [], []
    for rnd in range(nv):
        row = []
        for p in range(nparties):
            t0, tinf = S.quadratic_evals(sparse[p], eqs[p], p, rnd == 0)
            eq = eqs[p]
            sw = eq.current_scalar * eq.w[eq.current_index - 1] % R
            row.append(S.cubic_from_linear_times_quadratic_with_hint((eq.current_scalar - sw) % R, (2 * sw - eq.current_scalar) % R, t0, tinf, claims[rnd][p]))
        msgs.append(row)
        rs.append(rng.field())
        nxt = O.unipoly_eval(O.combine_additive(row), rs[rnd])
        claims.append([O.additive_promote_from_trivial(nxt, p) for p in range(nparties)])
        for p in range(nparties):
            eqs[p].bind(rs[rnd])
            sparse[p] = S.bind_sparse(sparse[p], rs[rnd], p)
    finals = [S.final_evals(sparse[p], p) for p in range(nparties)]
    return dict(uniform=uniform, cross=cross, padded=padded, polys=polys, tau=tau, nv=nv, msgs=msgs, rs=rs, claims=claims, finals=finals)


class _OuterPair:
    """subject and twin of every party, and the oracle of the shape"""

    def __init__(self, cozk, ctx, log_steps, nparties):
        self.cozk, self.ctx, self.nparties = cozk, ctx, nparties
        self.ref = _outer_oracle(log_steps, nparties)
        self.subject, self.twin = self.create(), self.create()

    def create(self):
        OU = importlib.import_module("co-zkvms_amd.outer")
        ref = self.ref
        mode = "plain" if self.nparties == 1 else "rep3"
        out = []
        for p in range(self.nparties):
            dp = [self.cozk.Rep3DensePolynomial.new(self.ctx, col) for _kind, col in ref["polys"][p]]
            out.append(OU.SpartanOuter(self.ctx, mode, p, ref["uniform"], ref["cross"], dp, ref["padded"], ref["tau"]))
        return out

    def check_round(self, devs, rnd):
        """round `rnd` of one family of handles (all parties) against the oracle; the messages"""
        ref = self.ref
        r_prev = ref["rs"][rnd - 1] if rnd else None
        got = [devs[p].round(r_prev, ref["claims"][rnd][p]) for p in range(self.nparties)]
        assert O.combine_additive(got) == O.combine_additive(ref["msgs"][rnd]), rnd
        if self.nparties == 1:
            assert got == ref["msgs"][rnd]
        return got

    def round(self, rnd):
        """round `rnd` on subject and twin: equal message shares, equal to the oracle's"""
        assert self.check_round(self.subject, rnd) == self.check_round(self.twin, rnd), rnd

    def check_final(self, devs):
        ref = self.ref
        got = [devs[p].final_evals(ref["rs"][-1]) for p in range(self.nparties)]
        assert O.combine_additive(got) == O.combine_additive(ref["finals"])
        if self.nparties == 1:
            assert got == ref["finals"]
        return got

    def final(self):
        assert self.check_final(self.subject) == self.check_final(self.twin)

    def unchanged_by(self, calls):
        """every (text, fn(handle)) is refused on every party's subject and leaves its length and its Az, Bz, Cz where they were"""
        for p, dev in enumerate(self.subject):
            before = (len(dev), dev.download())
            for text, fn in calls:
                _refused(self.cozk, text, lambda: fn(dev, p))
                assert (len(dev), dev.download()) == before, text
            assert before == (len(self.twin[p]), self.twin[p].download())

    def free(self):
        for d in self.subject + self.twin:
            d.free()


def _raw_outer_round(dev, r, claim, out):
    """cozk_outer_round with pointers of the test's choosing (None = NULL)"""
    bufs = [None if x is None else np.array(x, dtype=np.uint64) for x in (r, claim, out)]
    dev.ctx.check(dev._l.cozk_outer_round(dev.ctx.h, dev.h, *[None if b is None else b.ctypes.data for b in bufs]))


@pytest.mark.parametrize("log_steps,nparties", OUTER_CASES)
def test_outer_round_refused_with_two_entries_left_then_final_evals(cozk, ctx, log_steps, nparties):
    """with two entries left the last challenge belongs to cozk_outer_final_evals: cozk_outer_round with a challenge is refused
    BEFORE it binds (a bind in front of the check halves the tables, moves the split-eq state on and leaves a handle that
    cozk_outer_final_evals refuses).  Length and rows stay, and final_evals follows on the same handle and equals twin and oracle."""
    pair = _OuterPair(cozk, ctx, log_steps, nparties)
    try:
        ref = pair.ref
        for rnd in range(ref["nv"]):
            pair.round(rnd)
        assert [len(d) for d in pair.subject] == [2] * nparties
        r_last = ref["rs"][-1]
        pair.unchanged_by([(T_OUTER_LAST, lambda dev, p: dev.round(r_last, ref["claims"][-1][p])),
                           (T_OUTER_LAST, lambda dev, p: dev.round(R - 1, 0))])
        pair.final()
    finally:
        pair.free()


@pytest.mark.parametrize("log_steps,nparties", OUTER_CASES)
def test_outer_calls_out_of_turn_change_nothing(cozk, ctx, log_steps, nparties):
    """before the first round and after every round: final_evals with more than two entries left and a round with a NULL claim or
    output pointer are refused and move nothing.  At log_steps = 3 (8 rows per step, 64 entries) this falls on compact storage
    (rows per step 8, 4, 2: k_outer_bind_act has run from the second point on) and on dense storage (after three binds).  Then
    everything on the fully bound handle: refused, nothing moves, and a fresh handle on the same context goes through create,
    round and final."""
    pair = _OuterPair(cozk, ctx, log_steps, nparties)
    try:
        ref = pair.ref
        nv = ref["nv"]
        zero, out16 = [0, 0, 0, 0], [[0] * 4] * 4
        null_args = [(T_OUTER_ARG, lambda dev, p: _raw_outer_round(dev, None, None, out16)),
                     (T_OUTER_ARG, lambda dev, p: _raw_outer_round(dev, None, zero, None)),
                     (T_OUTER_ARG, lambda dev, p: _raw_outer_round(dev, zero, None, None))]
        for rnd in range(nv + 1):  # point `rnd`: rnd rounds done, 2^(nv - max(rnd - 1, 0)) entries left
            left = len(pair.subject[0])
            assert left == 1 << (nv - max(rnd - 1, 0))
            calls = list(null_args)
            if left > 2:
                calls += [(T_OUTER_FINAL, lambda dev, p: dev.final_evals(ref["rs"][max(rnd - 1, 0)])), (T_OUTER_FINAL, lambda dev, p: dev.final_evals(0))]
            pair.unchanged_by(calls)
            if rnd < nv:
                pair.round(rnd)
        pair.final()
        # fully bound
        assert [len(d) for d in pair.subject] == [1] * nparties
        r = ref["rs"][-1]
        pair.unchanged_by([(T_OUTER_BOUND, lambda dev, p: dev.round(None, ref["claims"][-1][p])),
                           (T_OUTER_BOUND, lambda dev, p: dev.round(r, ref["claims"][-1][p])),
                           (T_OUTER_FINAL, lambda dev, p: dev.final_evals(r))] + null_args)
        fresh = pair.create()
        try:
            for rnd in range(nv):
                pair.check_round(fresh, rnd)
            pair.check_final(fresh)
        finally:
            for d in fresh:
                d.free()
    finally:
        pair.free()


# ------------------------------------------------------------------------------------------------ ProdList
T_PL_LAST = "prodlist_round: nothing left to sum after this fix (the last randomness goes to cozk_prodlist_final)"
T_PL_FIXED = "prodlist_round: fully fixed"
T_PL_NONE = "prodlist_round: no variable left"
T_PL_ARG = "prodlist_round: bad argument"
T_PL_FINAL = "prodlist_final: one variable must be left"
# (variables, polynomials, products): two and three polynomials, degree 2 with polynomial 0 twice in one product, degree 3
PRODLIST_CASES = {
    "nv1-2polys-square": (1, 2, [(5, [0, 0]), (R - 1, [1])]),
    "nv3-2polys-square": (3, 2, [(R - 2, [0, 0]), (1, [0, 1]), (7, [1])]),
    "nv1-3polys": (1, 3, [(1, [0, 1, 2]), (R - 1, [2, 2])]),
    "nv3-3polys": (3, 3, [(3, [0, 0]), (R - 1, [1, 2]), (1, [2])]),
}


class _ProdListPair:
    """subject, twin and the oracle's tables; ProdList has no download: what a refused call left is seen in every later message"""

    def __init__(self, cozk, ctx, case):
        LG = importlib.import_module("co-zkvms_amd.logup")
        self.nv, n_polys, self.products = PRODLIST_CASES[case]
        rng = O.SplitMix64(500 + 10 * self.nv + n_polys)
        self.ref0 = [[rng.field() for _ in range(1 << self.nv)] for _ in range(n_polys)]
        self.rs = [rng.field() for _ in range(self.nv)]  # rs[j]: fixed by round j + 1, the last one by final
        self.degree = max(len(f) for _, f in self.products)
        self.make = lambda: LG.ProdList(ctx, [cozk.Vec.from_ints(ctx, p) for p in self.ref0], self.products)
        self.ref = self.ref0  # the oracle's tables of subject and twin
        self.subject, self.twin = self.make(), self.make()
        assert self.subject.degree == self.degree

    def round(self, rnd):
        r = self.rs[rnd - 1] if rnd else None
        if rnd:
            self.ref = G.fix_variables(self.ref, r)
        want = G.prove_round(self.ref, self.products, self.degree)
        assert self.subject.round(r) == want, rnd
        assert self.twin.round(r) == want, rnd

    def final(self):
        want = [p[0] for p in G.fix_variables(self.ref, self.rs[-1])]
        assert self.subject.final(self.rs[-1]) == want
        assert self.twin.final(self.rs[-1]) == want

    def free(self):
        self.subject.free()
        self.twin.free()


def _raw_prodlist_round(pl, r, out):
    """cozk_prodlist_round with pointers of the test's choosing (None = NULL)"""
    bufs = [None if x is None else np.array(x, dtype=np.uint64) for x in (r, out)]
    pl.ctx.check(pl._l.cozk_prodlist_round(pl.ctx.h, pl.h, *[None if b is None else b.ctypes.data for b in bufs]))


@pytest.mark.parametrize("case", list(PRODLIST_CASES))
def test_prodlist_round_refused_with_one_variable_left_then_final(cozk, ctx, case):
    """with one variable left (two elements per polynomial) the last randomness belongs to cozk_prodlist_final: cozk_prodlist_round
    with it is refused BEFORE it fixes the variable (a fix in front of the check flips the ping-pong and leaves a list
    that cozk_prodlist_final refuses).  The final that follows on the same list equals twin and oracle."""
    pair = _ProdListPair(cozk, ctx, case)
    try:
        for rnd in range(pair.nv):
            pair.round(rnd)
        assert len(pair.ref[0]) == 2
        _refused(cozk, T_PL_LAST, lambda: pair.subject.round(pair.rs[-1]))
        _refused(cozk, T_PL_LAST, lambda: pair.subject.round(R - 1))
        pair.final()
    finally:
        pair.free()


@pytest.mark.parametrize("case", list(PRODLIST_CASES))
def test_prodlist_calls_out_of_turn_change_nothing(cozk, ctx, case):
    """before the first round and after every round: a round with a NULL output and, with more than one variable left, final are
    refused, and the messages that follow equal twin and oracle.  Then everything on the fully fixed list is refused, and a fresh
    list on the same context goes through its rounds and its final."""
    pair = _ProdListPair(cozk, ctx, case)
    try:
        null_out = [(T_PL_ARG, lambda: _raw_prodlist_round(pair.subject, None, None)),
                    (T_PL_ARG, lambda: _raw_prodlist_round(pair.subject, [1, 0, 0, 0], None))]
        for rnd in range(pair.nv + 1):  # point `rnd`: rnd rounds done, len(pair.ref[0]) elements per polynomial left
            calls = list(null_out)
            if len(pair.ref[0]) > 2:
                calls += [(T_PL_FINAL, lambda: pair.subject.final(pair.rs[max(rnd - 1, 0)])), (T_PL_FINAL, lambda: pair.subject.final(0))]
            for text, fn in calls:
                _refused(cozk, text, fn)
            if rnd < pair.nv:
                pair.round(rnd)
        pair.final()
        for text, fn in [(T_PL_FIXED, lambda: pair.subject.round(pair.rs[-1])), (T_PL_NONE, lambda: pair.subject.round()),
                         (T_PL_FINAL, lambda: pair.subject.final(pair.rs[-1]))] + null_out:
            _refused(cozk, text, fn)
        fresh = pair.make()
        try:
            ref = pair.ref0
            for rnd in range(pair.nv):
                if rnd:
                    ref = G.fix_variables(ref, pair.rs[rnd - 1])
                assert fresh.round(pair.rs[rnd - 1] if rnd else None) == G.prove_round(ref, pair.products, pair.degree)
            assert fresh.final(pair.rs[-1]) == [p[0] for p in G.fix_variables(ref, pair.rs[-1])]
        finally:
            fresh.free()
    finally:
        pair.free()


# ------------------------------------------------------------------------------------------------ the binds of the dense seam
def _raw_bind(ctx, fn, h, r, *more):
    """a bind entry point with a challenge pointer of the test's choosing (None = NULL)"""
    rr = None if r is None else np.array(r, dtype=np.uint64)
    ctx.check(fn(ctx.h, h, None if rr is None else rr.ctypes.data, *more))


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_poly_bind_refusals_leave_the_polynomial_untouched(cozk, ctx, mode):
    """cozk_poly_bind has one check ("poly_bind: bad argument": a NULL challenge, an order that is neither, a single element) in front
    of everything: four elements stay four elements with their values, both binds follow and equal twin and oracle, and the
    single element that is left stays too"""
    rng = O.SplitMix64(61 + (mode == "rep3"))
    coeffs = [(rng.field(), rng.field()) for _ in range(4)] if mode == "rep3" else [rng.field() for _ in range(4)]
    poly, twin = cozk.Rep3DensePolynomial.new(ctx, coeffs), cozk.Rep3DensePolynomial.new(ctx, coeffs)
    l = ctx._l
    ref = coeffs
    for order, o_order in ((cozk.HIGH_TO_LOW, O.HIGH_TO_LOW), (cozk.LOW_TO_HIGH, O.LOW_TO_HIGH)):
        r = rng.field()
        for bad in (lambda: _raw_bind(ctx, l.cozk_poly_bind, poly.h, None, order), lambda: poly.bind(r, 7), lambda: poly.bind(r, -1)):
            _refused(cozk, "poly_bind: bad argument", bad)
            assert poly.coeffs() == ref
        poly.bind(r, order)
        twin.bind(r, order)
        ref = O.dense_bind(ref, r, o_order)
        assert poly.coeffs() == twin.coeffs() == ref
    assert len(poly) == 1
    for order in (cozk.HIGH_TO_LOW, cozk.LOW_TO_HIGH):
        _refused(cozk, "poly_bind: bad argument", lambda: poly.bind(rng.field(), order))
        assert poly.coeffs() == twin.coeffs() == ref
    poly.free()
    twin.free()


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_layer_bind_and_spliteq_bind_refusals_leave_their_handle_untouched(cozk, ctx, mode):
    """cozk_layer_bind ("layer_bind: bad argument": a NULL challenge) and cozk_spliteq_bind ("spliteq_bind: bad argument", and
    "polynomial already fully bound" after the last variable) check before they move a ping-pong side: coefficients, table lengths
    and tables stay, and the binds that follow equal twin and oracle"""
    rng = O.SplitMix64(63 + (mode == "rep3"))
    coeffs = [(rng.field(), rng.field()) for _ in range(8)] if mode == "rep3" else [rng.field() for _ in range(8)]
    layer, twin = cozk.Rep3DenseInterleavedPolynomial.new(ctx, coeffs), cozk.Rep3DenseInterleavedPolynomial.new(ctx, coeffs)
    w = [rng.field() for _ in range(2)]
    eq, eq_twin, eq_ref = cozk.SplitEqPolynomial(ctx, w), cozk.SplitEqPolynomial(ctx, w), O.SplitEq(w)
    l = ctx._l
    ref = coeffs
    for _ in range(2):
        _refused(cozk, "layer_bind: bad argument", lambda: _raw_bind(ctx, l.cozk_layer_bind, layer.h, None))
        _refused(cozk, "spliteq_bind: bad argument", lambda: _raw_bind(ctx, l.cozk_spliteq_bind, eq.h, None))
        assert l.cozk_layer_round(ctx.h, layer.h, eq.h, None, None, None) == INVALID  # a NULL claim and output: the first statement
        assert layer.coeffs() == ref and (eq.lens(), eq.download()) == (eq_twin.lens(), eq_twin.download())
        r = rng.field()
        for x in (layer, twin, eq, eq_twin, eq_ref):
            x.bind(r)
        ref = O.interleaved_bind(ref, r)
        assert layer.coeffs() == twin.coeffs() == ref
        assert eq.lens() == eq_twin.lens() == (eq_ref.E1_len, eq_ref.E2_len)
        assert eq.download() == eq_twin.download() == (eq_ref.E1[:eq_ref.E1_len], eq_ref.E2[:eq_ref.E2_len])
    assert eq.lens() == (1, 1)
    _refused(cozk, "spliteq_bind: polynomial already fully bound", lambda: eq.bind(rng.field()))
    assert (eq.lens(), eq.download()) == (eq_twin.lens(), eq_twin.download())
    for x in (layer, twin, eq, eq_twin):
        x.free()


# ------------------------------------------------------------------------------------------------ ToggleLayer
@pytest.mark.parametrize("nparties", [1, 3])
def test_toggle_calls_on_the_last_bind_and_fully_bound_change_nothing(cozk, ctx, nparties):
    """the refusals of cozk_toggle_round and cozk_toggle_bind at the end of the rounds (tests/test_gpu_lookups.py has those about
    the eq polynomial): with two coalesced entries left a binding round is refused -- that bind belongs to cozk_toggle_bind -- and
    on the fully bound layer every round and every bind is; flags and fingerprints stay each time, and the final claims equal the
    twin's and the oracle's (oracle/pysparse.py)."""
    import pysparse as SP
    LK = importlib.import_module("co-zkvms_amd.lookups")
    batch, n = 2, 4
    party = 1 if nparties == 3 else 0
    rng = O.SplitMix64(71)
    cols = [[1, 0, 1, 1]]
    vals = [[rng.field() for _ in range(n)] for _ in range(batch)]
    shared = [[O.rep3_share(v, rng) for v in row] for row in vals]
    fps = [vals] if nparties == 1 else [[[s[p] for s in row] for row in shared] for p in range(3)]
    nv = (batch * n).bit_length() - 1
    w, rs = [rng.field() for _ in range(nv)], [rng.field() for _ in range(nv)]
    ref = SP.ToggleLayer([[i for i, f in enumerate(c) if f] for c in cols], fps[party], party, nparties)
    dev, twin = LK.ToggleLayer(ctx, cols, fps[party]), LK.ToggleLayer(ctx, cols, fps[party])
    eq, eq_twin, eq_ref = cozk.SplitEqPolynomial(ctx, w), cozk.SplitEqPolynomial(ctx, w), O.SplitEq(w)
    spare = cozk.SplitEqPolynomial(ctx, w)  # never bound: the refusals below are about the layer
    for j in range(nv):
        ev = ref.compute_cubic_evals(eq_ref, 0)
        r = rs[j - 1] if j else None
        assert dev.round(eq, r, party=party) == twin.round(eq_twin, r, party=party) == [ev[0], ev[2], ev[3]], j
        ref.bind(rs[j])
        eq_ref.bind(rs[j])

    def unchanged_by(calls):
        before = (dev.download(), eq.lens(), eq.download(), spare.lens())
        for text, fn in calls:
            _refused(cozk, text, fn)
            assert (dev.download(), eq.lens(), eq.download(), spare.lens()) == before, text
        assert before[0] == twin.download()

    assert ctx._l.cozk_toggle_round(ctx.h, dev.h, eq.h, None, party, None) == INVALID  # a NULL output: the first statement
    unchanged_by([("toggle_round: the bind leaves the layer fully bound", lambda: dev.round(eq, rs[-1], party=party)),
                  ("toggle_round: the bind leaves the layer fully bound", lambda: dev.round(spare, rs[-1], party=party)),
                  ("toggle_bind: bad argument", lambda: _raw_bind(ctx, ctx._l.cozk_toggle_bind, dev.h, None))])
    dev.bind(rs[-1])
    twin.bind(rs[-1])
    unchanged_by([("toggle_round: fully bound", lambda: dev.round(spare, None, party=party)),
                  ("toggle_round: fully bound", lambda: dev.round(spare, rs[-1], party=party)),
                  ("toggle_bind: fully bound", lambda: dev.bind(rs[-1]))])
    fl, fp = dev.final_claims()
    rfl, rfp = ref.final_claims()
    assert (fl, fp) == twin.final_claims()
    assert fp == rfp and fl == (rfl if nparties == 1 else ref.coalesced_flags[0])
    for x in (dev, twin, eq, eq_twin, spare):
        x.free()
