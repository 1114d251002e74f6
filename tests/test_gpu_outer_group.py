"""GPU tests of the outer groups (cozk_outer_group_*) and the shift groups (cozk_shift_group_*): one round of co-jolt's Spartan outer
sumcheck / of a (share, public) product sumcheck for several members with one challenge.  The yardstick is the per-member path --
cozk_outer_round / cozk_outer_final_evals, which test_gpu_outer.py holds to the oracle, and cozk_prod_sumcheck_evals +
cozk_poly_bind(.., HIGH_TO_LOW), which test_gpu_poly.py holds to it -- on twins with the same data.  Bar: bit-exact, raw Montgomery
limbs through the C ABI (ctypes).  The members hold DISTINCT random columns (not shares of one witness), so a member mix-up shows.
No test provokes a device fault: every bad argument is refused on the host before any launch."""
import ctypes
import importlib

import numpy as np
import pytest

import pyjolt_r1cs as J
import pyref as O
import pyspartan_outer as S

pytestmark = pytest.mark.gpu
INVALID = -1  # COZK_ERR_INVALID_ARG
SENT = 0x5A5A
R = O.R
HIGH_TO_LOW = 1


@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def OU():
    return importlib.import_module("co-zkvms_amd.outer")


def _fr(cozk, x):
    return np.ascontiguousarray(cozk.fr_to_mont_limbs([x])[0])


def _poly(cozk, c, length, seed, mode=None):
    return cozk.Rep3DensePolynomial.random(c, length, seed, mode=cozk.MODE_PLAIN if mode is None else mode)


def _system(name):
    if name == "jolt":
        return J.build_system() + (J.NUM_INPUTS,)
    return S.synthetic_system() + (14,)


# ------------------------------------------------------------------------------------------------ outer groups
def _outer_raw(st):
    """Az, Bz, Cz of a PLAIN cozk_outer as cozk_outer_download shows them: (3, L, 4) limbs"""
    n = len(st)
    bufs = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
    st.ctx.check(st._l.cozk_outer_download(st.ctx.h, st.h, bufs[0].ctypes.data, None, bufs[1].ctypes.data, None, bufs[2].ctypes.data, None))
    return np.stack(bufs)


def _twin_round(st, r, claim):
    out = np.zeros((4, 4), dtype=np.uint64)
    st.ctx.check(st._l.cozk_outer_round(st.ctx.h, st.h, r.ctypes.data if r is not None else None, claim.ctypes.data, out.ctypes.data))
    return out


def _twin_final(st, r):
    out = np.zeros((3, 4), dtype=np.uint64)
    st.ctx.check(st._l.cozk_outer_final_evals(st.ctx.h, st.h, r.ctypes.data, out.ctypes.data))
    return out


class OuterSide:
    """k members, twice from the same seeds: `grp` for the group, `one` for the per-member calls"""

    def __init__(self, cozk, OU, pcs, system, log_steps, k, seed, tau_seed=None):
        self.cozk, self.k = cozk, k
        uniform, cross, padded, ncols = _system(system)
        n = 1 << log_steps
        self.n_tau = log_steps + padded.bit_length() - 1
        rng = O.SplitMix64(seed if tau_seed is None else tau_seed)
        self.tau = [rng.field() for _ in range(self.n_tau)]

        def mk():
            out = []
            for m in range(k):
                c = pcs[m % len(pcs)]
                cols = [_poly(cozk, c, n, seed + 1000 * m + v) for v in range(ncols)]
                out.append(OU.SpartanOuter(c, "plain", 0, uniform, cross, cols, padded, self.tau))
            return out

        self.grp, self.one = mk(), mk()
        self.d = pcs[0]
        self.g = cozk.OuterGroup(self.d, self.grp)

    def same_state(self, members=None):
        for m in range(self.k) if members is None else members:
            assert len(self.grp[m]) == len(self.one[m]), "member %d" % m
            assert np.array_equal(_outer_raw(self.grp[m]), _outer_raw(self.one[m])), "member %d" % m

    def check_round(self, r, rng):
        claims = np.ascontiguousarray(self.cozk.fr_to_mont_limbs([rng.field() for _ in range(self.k)]))
        got = self.g.round_raw(r, claims)
        for m in range(self.k):
            assert np.array_equal(got[m], _twin_round(self.one[m], r, np.ascontiguousarray(claims[m]))), "member %d" % m
        self.same_state()
        assert len(self.g) == len(self.one[0])

    def check_final(self, r, k_final):
        before = [_outer_raw(self.grp[m]) for m in range(k_final, self.k)]
        got = self.g.final_raw(r, k_final)
        for m in range(k_final):
            assert np.array_equal(got[m], _twin_final(self.one[m], r)), "member %d" % m
            assert len(self.grp[m]) == 1
        self.same_state(range(k_final))
        for m, b in zip(range(k_final, self.k), before):  # left untouched
            assert len(self.grp[m]) == 2 and np.array_equal(_outer_raw(self.grp[m]), b)

    def free(self):
        self.g.free()
        for st in self.grp + self.one:
            st.free()


def _run_outer(cozk, OU, pcs, system, log_steps, k, k_final=None):
    s = OuterSide(cozk, OU, pcs, system, log_steps, k, seed=100 * log_steps + 10 * k + (1 if system == "jolt" else 0))
    rng = O.SplitMix64(log_steps + 7 * k)
    s.same_state()
    r = None
    for _ in range(s.n_tau):
        s.check_round(r, rng)
        r = _fr(cozk, rng.field())
    s.check_final(r, k if k_final is None else k_final)
    s.g.free()
    s.same_state(range(k if k_final is None else k_final))  # the members outlive the group
    s.free()


# toy (7 of 8 rows): act 7 -> 4 -> 2 -> 1: compact rows inside a step (per_step 8, 4), the round whose output rows are whole steps
# (per_step 2), the dense tail; log_steps 0, 1, 3: one workgroup per member (L <= 2048); 12: L = 2^15, 2^12 x 4 pairs: gx > 1 and the
# finishing launch until the members are down to 2048 rows.  jolt (72 of 128 rows): 72 -> 36 -> 18 -> 9 -> 5 -> 3 -> 2 -> 1, act odd
# three times on the read side and the write side; log_steps 6: L = 8192, 64 x 36 = 2304 pairs in the first round: gx > 1.
SHAPES = [("toy", 0), ("toy", 1), ("toy", 3), ("toy", 12), ("jolt", 0), ("jolt", 2), ("jolt", 6)]


@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("system,log_steps", SHAPES)
def test_outer_group_rounds_equal_per_member_rounds(cozk, OU, party_ctxs, system, log_steps, k):
    _run_outer(cozk, OU, party_ctxs, system, log_steps, k)


def test_outer_final_of_the_first_members_only(cozk, OU, party_ctxs):
    _run_outer(cozk, OU, party_ctxs, "toy", 1, 5, k_final=3)
    _run_outer(cozk, OU, party_ctxs, "jolt", 0, 3, k_final=0)
    _run_outer(cozk, OU, party_ctxs, "toy", 0, 4, k_final=1)


def test_outer_sum_grid_cap_gives_the_same_sums(cozk, OU, party_ctxs, monkeypatch):
    monkeypatch.setenv("COZK_SUM_GRID_MAX", "2")  # 2 workgroups per member: a lane adds up to 32 (toy) / 5 (jolt) terms per sum
    _run_outer(cozk, OU, party_ctxs, "toy", 12, 3)
    _run_outer(cozk, OU, party_ctxs, "jolt", 6, 3)


def test_outer_group_against_big_ints(cozk, OU, party_ctxs):
    """the group against a dense big-int walk (not the per-member kernels): toy system, 2 steps, 3 members"""
    import shamir_jolt_spartan_ref as JS
    uniform, cross, padded, ncols = _system("toy")
    k, n = 3, 2
    rng = O.SplitMix64(4242)
    cols = [[[rng.field() for _ in range(n)] for _ in range(ncols)] for _ in range(k)]
    tau = [rng.field() for _ in range(4)]
    members = [OU.SpartanOuter(party_ctxs[m], "plain", 0, uniform, cross, [cozk.Rep3DensePolynomial.new(party_ctxs[m], c) for c in cols[m]], padded, tau)
               for m in range(k)]
    g = cozk.OuterGroup(party_ctxs[0], members)
    abc = [JS.dense_azbzcz(uniform, cross, padded, cols[m], n) for m in range(k)]
    eq = S.GruenSplitEq(tau)
    r = None
    for rnd in range(4):
        if r is not None:
            eq.bind(r)
            abc = [tuple(JS._bind_low(v, r) for v in abc[m]) for m in range(k)]
        claims = [rng.field() for _ in range(k)]
        sw = eq.current_scalar * eq.w[eq.current_index - 1] % R
        l0, l1 = (eq.current_scalar - sw) % R, (2 * sw - eq.current_scalar) % R
        want = [S.cubic_from_linear_times_quadratic_with_hint(l0, l1, *JS._quadratic(*abc[m], eq, rnd == 0), claims[m]) for m in range(k)]
        assert g.round(r, claims) == want
        assert [st.download() for st in members] == [[list(v) for v in abc[m]] for m in range(k)]
        r = rng.field()
    assert g.final(r, k) == [[JS._bind_low(v, r)[0] for v in abc[m]] for m in range(k)]
    g.free()
    for st in members:
        st.free()


# ------------------------------------------------------------------------------------------------ shift groups
def _raw(p):
    n = len(p)
    a = np.zeros((n, 4), dtype=np.uint64)
    b = np.zeros((n, 4), dtype=np.uint64)
    p.ctx.check(p.ctx._l.cozk_poly_download(p.ctx.h, p.h, a.ctypes.data, b.ctypes.data))
    return a


class ShiftSide:
    """k members and the public polynomial, twice from the same seeds; every twin member has a public twin on its own context"""

    def __init__(self, cozk, pcs, k, length, seed):
        self.cozk, self.k = cozk, k
        mk = lambda: [_poly(cozk, pcs[m % len(pcs)], length, seed + 10 * m) for m in range(k)]
        self.grp, self.one = mk(), mk()
        self.d = pcs[0]
        self.pub_g = _poly(cozk, self.d, length, seed + 5000)
        self.pub_s = [_poly(cozk, p.ctx, length, seed + 5000) for p in self.one]
        self.g = cozk.ShiftGroup(self.d, self.grp, self.pub_g)

    def _bind_twin(self, m, r):
        c = self.one[m].ctx
        for p in (self.one[m], self.pub_s[m]):
            c.check(c._l.cozk_poly_bind(c.h, p.h, r.ctypes.data, HIGH_TO_LOW))

    def single_round(self, m, r):
        c = self.one[m].ctx
        if r is not None:
            self._bind_twin(m, r)
        out = np.zeros((2, 4), dtype=np.uint64)
        arr = (ctypes.c_void_p * 2)(self.one[m].h, self.pub_s[m].h)
        c.check(c._l.cozk_prod_sumcheck_evals(c.h, arr, 2, 2, out.ctypes.data))
        return out

    def same_planes(self, members):
        for m in members:
            assert len(self.grp[m]) == len(self.one[m]) and np.array_equal(_raw(self.grp[m]), _raw(self.one[m])), "member %d" % m

    def check_round(self, r):
        got = self.g.round_raw(r)
        for m in range(self.k):
            assert np.array_equal(got[m], self.single_round(m, r)), "member %d" % m
        self.same_planes(range(self.k))
        assert len(self.g) == len(self.pub_s[0]) and np.array_equal(self.g.pub_raw(), _raw(self.pub_s[0]))

    def check_final(self, r, k_final):
        before = [_raw(self.grp[m]) for m in range(k_final, self.k)]
        got = self.g.final_raw(r, k_final)
        for m in range(self.k):
            self._bind_twin(m, r)
        for m in range(k_final):
            assert np.array_equal(got[m], _raw(self.one[m])[0]) and len(self.grp[m]) == 1
        self.same_planes(range(k_final))
        for m, b in zip(range(k_final, self.k), before):  # left untouched
            assert len(self.grp[m]) == 2 and np.array_equal(_raw(self.grp[m]), b)
        pub = _raw(self.pub_s[0])
        assert len(self.g) == 1 and np.array_equal(self.g.pub_raw(), pub) and np.array_equal(got[-1:], pub)


def _run_shift(cozk, pcs, k, length, k_final=None):
    s = ShiftSide(cozk, pcs, k, length, seed=1000 * length + 10 * k)
    rng = O.SplitMix64(length + 3 * k)
    r = None
    for _ in range(length.bit_length() - 1):
        s.check_round(r)
        r = _fr(cozk, rng.field())
    s.check_final(r, k if k_final is None else k_final)
    s.g.free()
    s.same_planes(range(k if k_final is None else k_final))  # the members outlive the group


# 2: no binding round; 4: one; 2048 = 2^11: the single-launch bound; 4096 = 2^12: the first multi-workgroup size (the sums as they
# stand, one fused bind), then the hand-over to the single launch; 8192: two multi-workgroup fused binds before the hand-over
@pytest.mark.parametrize("length", [2, 4, 2048, 4096, 8192])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_shift_group_rounds_equal_per_poly_rounds(cozk, party_ctxs, k, length):
    _run_shift(cozk, party_ctxs, k, length)


def test_shift_final_of_the_first_members_only_and_grid_cap(cozk, party_ctxs, monkeypatch):
    _run_shift(cozk, party_ctxs, 4, 8, k_final=2)
    _run_shift(cozk, party_ctxs, 3, 4, k_final=0)
    monkeypatch.setenv("COZK_SUM_GRID_MAX", "2")
    _run_shift(cozk, party_ctxs, 3, 8192)


def test_shift_group_against_big_ints(cozk, party_ctxs):
    import shamir_jolt_spartan_ref as JS
    k, length = 3, 8
    rng = O.SplitMix64(77)
    vals = [[rng.field() for _ in range(length)] for _ in range(k)]
    pub = [rng.field() for _ in range(length)]
    members = [cozk.Rep3DensePolynomial.new(party_ctxs[m], v) for m, v in enumerate(vals)]
    g = cozk.ShiftGroup(party_ctxs[0], members, cozk.Rep3DensePolynomial.new(party_ctxs[0], pub))
    r = None
    for _ in range(3):
        if r is not None:
            vals, pub = [JS._bind_top(v, r) for v in vals], JS._bind_top(pub, r)
        assert g.round(r) == [list(JS._evals_0_2(v, pub)) for v in vals]
        assert [p.coeffs() for p in members] == vals
        r = rng.field()
    finals, pub_final = g.final(r, k)
    assert finals == [JS._bind_top(v, r)[0] for v in vals] and pub_final == JS._bind_top(pub, r)[0]
    g.free()


# ------------------------------------------------------------------------------------------------ refusals
def _expect_invalid(cozk, driver, rc, *texts):
    assert rc == INVALID
    msg = cozk._lib.lib().cozk_last_error(driver.h).decode()
    assert msg and all(t in msg for t in texts), msg


def _arr(objs, n=40):
    return (ctypes.c_void_p * n)(*([x.h.value if x is not None else None for x in objs] + [None] * (n - len(objs))))


def test_outer_refusals_leave_the_members_untouched(cozk, OU, party_ctxs):
    l = cozk._lib.lib()
    pcs = party_ctxs
    d = pcs[0]
    rng = O.SplitMix64(12)
    s = OuterSide(cozk, OU, pcs, "toy", 1, 3, seed=7)
    members = s.grp
    before = [_outer_raw(m) for m in members]
    uniform, cross, padded, ncols = _system("toy")
    rep3 = OU.SpartanOuter(d, "rep3", 0, uniform, cross, [_poly(cozk, d, 2, 50 + v, mode=cozk.MODE_REP3) for v in range(ncols)], padded, s.tau)
    other_tau = OuterSide(cozk, OU, pcs, "toy", 1, 1, seed=7, tau_seed=8)
    longer = OuterSide(cozk, OU, pcs, "toy", 2, 1, seed=7)
    many = members * 11

    def create(driver, mem, k, text, out=True):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_outer_group_create(driver.h if driver else None, _arr(mem) if mem is not None else None, k, ctypes.byref(h) if out else None)
        if driver:
            _expect_invalid(cozk, driver, rc, "outer_group_create: ", text)
        assert rc == INVALID and (not out or h.value is None)

    create(None, members, 3, "null argument")  # no driver: nowhere to leave the text
    create(d, None, 3, "null argument")
    create(d, members, 3, "null argument", out=False)
    for k in (0, -1, 33):
        create(d, many, k, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, members[:1] + [None] + members[2:], 3, "null member")
    create(d, members[:1] + [rep3] + members[2:], 3, "every member must be PLAIN")
    create(d, members[:2] + [members[0]], 3, "duplicate member")
    create(d, members[:2] + other_tau.grp, 3, "every member must have been made with the same tau")
    create(d, members[:2] + longer.grp, 3, "every member must be in the same state")
    assert all(np.array_equal(b, _outer_raw(m)) for b, m in zip(before, members))

    g = s.g
    r = _fr(cozk, rng.field())
    claims = np.ascontiguousarray(cozk.fr_to_mont_limbs([rng.field() for _ in range(3)]))
    out = np.zeros((3, 4, 4), dtype=np.uint64)
    assert l.cozk_outer_group_round(None, None, claims.ctypes.data, out.ctypes.data) == INVALID
    assert l.cozk_outer_group_final(None, r.ctypes.data, 0, out.ctypes.data) == INVALID
    assert l.cozk_outer_group_len(None) == 0
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, None, None, out.ctypes.data), "outer_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, None, claims.ctypes.data, None), "outer_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_outer_group_final(g.h, None, 3, out.ctypes.data), "outer_group_final: null argument")
    _expect_invalid(cozk, d, l.cozk_outer_group_final(g.h, r.ctypes.data, 3, None), "outer_group_final: null argument")
    for k_final in (-1, 4):
        _expect_invalid(cozk, d, l.cozk_outer_group_final(g.h, r.ctypes.data, k_final, out.ctypes.data), "outer_group_final: 0 <= k_final <= k")
    _expect_invalid(cozk, d, l.cozk_outer_group_final(g.h, r.ctypes.data, 3, out.ctypes.data), "outer_group_final: one unbound variable must be left")
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, r.ctypes.data, claims.ctypes.data, out.ctypes.data), "outer_group_round: the first round takes no challenge")
    assert (out == 0).all() and all(np.array_equal(b, _outer_raw(m)) for b, m in zip(before, members))
    # a member that was driven on its own is in another state: refused, the others untouched
    _twin_round(members[1], None, np.ascontiguousarray(claims[1]))
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, None, claims.ctypes.data, out.ctypes.data), "outer_group_round: every member must be in the same state")
    assert (out == 0).all() and all(np.array_equal(b, _outer_raw(m)) for i, (b, m) in enumerate(zip(before, members)) if i != 1)
    g.free()
    s.free()

    # ... a fresh set: every round to the end, with the refusals of the later rounds on the way
    s = OuterSide(cozk, OU, pcs, "toy", 1, 3, seed=9)
    g = s.g
    s.check_round(None, rng)
    live = [_outer_raw(m) for m in s.grp]
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, None, claims.ctypes.data, out.ctypes.data), "outer_group_round: every round after the first binds")
    assert all(np.array_equal(b, _outer_raw(m)) for b, m in zip(live, s.grp))
    for _ in range(s.n_tau - 1):
        s.check_round(r, rng)
        r = _fr(cozk, rng.field())
    live = [_outer_raw(m) for m in s.grp]
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, r.ctypes.data, claims.ctypes.data, out.ctypes.data), "outer_group_round: the members are fully bound")
    assert (out == 0).all() and all(np.array_equal(b, _outer_raw(m)) for b, m in zip(live, s.grp)) and len(g) == 2
    s.check_final(r, 2)  # member 2 stays at length 2: the members' states differ from here on
    for call in (lambda: l.cozk_outer_group_round(g.h, r.ctypes.data, claims.ctypes.data, out.ctypes.data),
                 lambda: l.cozk_outer_group_final(g.h, r.ctypes.data, 3, out.ctypes.data)):
        _expect_invalid(cozk, d, call(), "every member must be in the same state")
    assert (out == 0).all()
    g.free()
    g = cozk.OuterGroup(d, s.grp[:2])  # fully bound members
    _expect_invalid(cozk, d, l.cozk_outer_group_round(g.h, r.ctypes.data, claims.ctypes.data, out.ctypes.data), "outer_group_round: the members are fully bound")
    _expect_invalid(cozk, d, l.cozk_outer_group_final(g.h, r.ctypes.data, 2, out.ctypes.data), "outer_group_final: one unbound variable must be left")
    s.same_state(range(2))
    g.free()
    assert l.cozk_outer_group_free(None) == 0
    s.free()
    rep3.free()
    other_tau.free()
    longer.free()


def test_shift_refusals_leave_members_and_public_polynomial_untouched(cozk, party_ctxs):
    l = cozk._lib.lib()
    pcs = party_ctxs
    d = pcs[0]
    rng = O.SplitMix64(13)
    s = ShiftSide(cozk, pcs, 3, 16, seed=7)
    members, pub = s.grp, s.pub_g
    before = [_raw(p) for p in members + [pub]]
    rep3 = _poly(cozk, d, 16, 8, mode=cozk.MODE_REP3)
    short, twelve, single = _poly(cozk, d, 8, 9), [_poly(cozk, d, 12, 10 + j) for j in range(2)], [_poly(cozk, d, 1, 20 + j) for j in range(2)]
    many = [_poly(cozk, d, 16, 100 + j) for j in range(33)]

    def create(driver, mem, k, p, text, out=True):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shift_group_create(driver.h if driver else None, _arr(mem) if mem is not None else None, k, p.h if p is not None else None,
                                       ctypes.byref(h) if out else None)
        if driver:
            _expect_invalid(cozk, driver, rc, "shift_group_create: ", text)
        assert rc == INVALID and (not out or h.value is None)

    create(None, members, 3, pub, "null argument")
    create(d, None, 3, pub, "null argument")
    create(d, members, 3, None, "null argument")
    create(d, members, 3, pub, "null argument", out=False)
    for k in (0, -1, 33):
        create(d, many, k, pub, "1 <= k <= COZK_LAYER_GROUP_MAX")
    create(d, members[:1] + [None] + members[2:], 3, pub, "null member")
    create(d, members[:1] + [rep3] + members[2:], 3, pub, "every member must be PLAIN")
    create(d, members, 3, rep3, "the public polynomial must be PLAIN")
    create(d, members[:1] + [short] + members[2:], 3, pub, "must have one length")
    create(d, members, 3, short, "must have one length")
    create(d, twelve[:1], 1, twelve[1], "the length must be a power of two >= 2")
    create(d, single[:1], 1, single[1], "the length must be a power of two >= 2")
    create(d, members[:2] + [members[1]], 3, pub, "duplicate member")
    create(d, [members[0], pub], 2, pub, "a member is the public polynomial")
    assert all(np.array_equal(x, _raw(p)) for x, p in zip(before, members + [pub]))

    g = s.g
    r = _fr(cozk, rng.field())
    out = np.zeros((3 * 2 + 1, 4), dtype=np.uint64)
    pub_before = g.pub_raw()
    assert l.cozk_shift_group_round(None, None, out.ctypes.data) == INVALID
    assert l.cozk_shift_group_final(None, None, 0, out.ctypes.data) == INVALID
    assert l.cozk_shift_group_pub_download(None, out.ctypes.data) == INVALID and l.cozk_shift_group_len(None) == 0
    _expect_invalid(cozk, d, l.cozk_shift_group_round(g.h, None, None), "shift_group_round: null argument")
    _expect_invalid(cozk, d, l.cozk_shift_group_final(g.h, r.ctypes.data, 3, None), "shift_group_final: null argument")
    _expect_invalid(cozk, d, l.cozk_shift_group_pub_download(g.h, None), "shift_group_pub_download: null argument")
    for k_final in (-1, 4):
        _expect_invalid(cozk, d, l.cozk_shift_group_final(g.h, r.ctypes.data, k_final, out.ctypes.data), "shift_group_final: 0 <= k_final <= k")
    for rr in (None, r):  # 16 elements do not end at one, with a bind or without
        _expect_invalid(cozk, d, l.cozk_shift_group_final(g.h, rr.ctypes.data if rr is not None else None, 3, out.ctypes.data),
                        "shift_group_final: the bind must leave one element")
    # a member that was driven on its own has another length: refused
    c1 = members[1].ctx
    twin = _poly(cozk, c1, 16, 7 + 10 * 1)
    c1.check(l.cozk_poly_bind(c1.h, members[1].h, r.ctypes.data, HIGH_TO_LOW))
    _expect_invalid(cozk, d, l.cozk_shift_group_round(g.h, None, out.ctypes.data), "shift_group_round: every member must have the group's current length")
    assert (out == 0).all() and np.array_equal(pub_before, g.pub_raw()) and len(g) == 16
    assert all(np.array_equal(x, _raw(p)) for i, (x, p) in enumerate(zip(before, members)) if i != 1)
    g.free()

    # ... and the members still work: every round to the end by a new group, against the per-poly calls
    s.grp[1] = twin
    s.g = cozk.ShiftGroup(d, s.grp, pub)
    r = None
    for _ in range(4):
        s.check_round(r)
        r = _fr(cozk, rng.field())
    live = [_raw(p) for p in s.grp] + [s.g.pub_raw()]
    _expect_invalid(cozk, d, l.cozk_shift_group_round(s.g.h, r.ctypes.data, out.ctypes.data), "shift_group_round: a binding round on members that the bind leaves fully bound")
    assert all(np.array_equal(x, y) for x, y in zip(live, [_raw(p) for p in s.grp] + [s.g.pub_raw()]))
    s.check_final(r, 3)
    for rr in (None, r):
        _expect_invalid(cozk, d, l.cozk_shift_group_round(s.g.h, rr.ctypes.data if rr is not None else None, out.ctypes.data),
                        "shift_group_round: the members are fully bound")
    _expect_invalid(cozk, d, l.cozk_shift_group_final(s.g.h, r.ctypes.data, 3, out.ctypes.data), "shift_group_final: the bind must leave one element")
    assert (out == 0).all()
    s.same_planes(range(3))
    d.check(l.cozk_shift_group_final(s.g.h, None, 3, out.ctypes.data))  # without a bind: the final values again
    assert np.array_equal(out[:3], np.concatenate([_raw(p) for p in s.grp])) and np.array_equal(out[3:4], s.g.pub_raw())
    s.g.free()
    assert l.cozk_shift_group_free(None) == 0


def test_member_on_another_device_is_refused(cozk, OU, party_ctxs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    l = cozk._lib.lib()
    d = party_ctxs[0]
    other = cozk.Context(1)
    here, there, pub, pub_there = _poly(cozk, d, 8, 1), _poly(cozk, other, 8, 2), _poly(cozk, d, 8, 3), _poly(cozk, other, 8, 3)
    for mem, p, text in (([here, there], pub, "every member must live on the driver's device"), ([here], pub_there, "the public polynomial must live on the driver's device")):
        h = ctypes.c_void_p(SENT)
        rc = l.cozk_shift_group_create(d.h, _arr(mem), len(mem), p.h, ctypes.byref(h))
        _expect_invalid(cozk, d, rc, "shift_group_create: ", text)
        assert h.value is None
    uniform, cross, padded, ncols = _system("toy")
    tau = [5, 6, 7]
    mk = lambda c: OU.SpartanOuter(c, "plain", 0, uniform, cross, [_poly(cozk, c, 1, 30 + v) for v in range(ncols)], padded, tau)
    a, b = mk(d), mk(other)
    h = ctypes.c_void_p(SENT)
    _expect_invalid(cozk, d, l.cozk_outer_group_create(d.h, _arr([a, b]), 2, ctypes.byref(h)), "outer_group_create: every member must live on the driver's device")
    assert h.value is None
    g = cozk.OuterGroup(d, [a])  # the member here still serves
    g.free()
    a.free()
    b.free()
    del there, pub_there
    other.close()
