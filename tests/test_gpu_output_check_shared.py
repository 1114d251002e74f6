"""GPU tests of the windowed output check on a shared v_final (cozk_output_check_shared_create, csrc/output_check.inc): for a PLAIN
polynomial and for the REP3 parties 0, 1 and 2, every round and the final of the device calls equal, as integers, a twin driven on the
device by Rep3DensePolynomial.from_vec_shares, linear_combination([v_final, v_io], [1, -1], mode, party), cozk_eq_evals,
prod_sumcheck_evals(.., 3) and bind(.., HIGH_TO_LOW) -- for the final (a + b) * 2^-1 of get_bound_coeff(0) -- and at m <= 6 the
plain-Python restatement tests/output_check_shared_ref.py.  log_mem = 1, 2, 5, 12 with the window families of the U32 test (one word, the
whole memory, the last word, an aligned half, across an aligned boundary, W = 2^j + 1, seeded random windows) and one case at 14 with
(0, 1), (0, MEM), (MEM - 1, 1), (MEM/2 - 1, 2), (0, 257) and (8192 - 2500, 5000): two sides, dots and folds past one workgroup.  Share
components in {0, r - 1} against v_io all 0xFFFFFFFF or all 0; challenges 0, 1 and r - 1 among random ones; for a real sharing of U32
words the three parties' round values sum to the rounds of OutputCheck on the U32 column; every refusal with its text; a handle freed
mid-way.  A vector on another device is checked where a second device exists."""
import ctypes
import random

import numpy as np
import pytest

import output_check_ref as OC
import output_check_shared_ref as S

pytestmark = pytest.mark.gpu
R, M32, TWO_INV = OC.R, OC.M32, S.TWO_INV
INVALID_ARG = -1


def _windows(m):
    MEM = 1 << m
    if m <= 6:
        return OC.windows(m, 40 + m)
    if m == 14:
        return [(0, 1), (0, MEM), (MEM - 1, 1), (MEM // 2 - 1, 2), (0, 257), (8192 - 2500, 5000)]
    rnd = random.Random(50 + m)
    out = [(0, 1), (0, MEM), (MEM - 1, 1), (0, MEM // 2), (MEM // 2, MEM // 2), (MEM // 2 - 1, 2)]
    for j in (0, 1, 7, 8):  # 2^7 + 1 = 129 and 2^8 + 1 = 257: one workgroup of dots and the first past it
        W = (1 << j) + 1
        out += [(0, W), (MEM - W, W), ((MEM - W) // 2 | 1, W)]
    for _ in range(3):
        W = rnd.randint(1, MEM)
        out.append((rnd.randint(0, MEM - W), W))
    return [w for i, w in enumerate(out) if w[0] + w[1] <= MEM and w not in out[:i]]


def _challenges(rnd, m):
    special = [0, 1, R - 1]
    return [rnd.choice(special) if rnd.random() < 0.25 else rnd.randrange(R) for _ in range(m)]


def _words(rnd, n):
    edge = [0, M32, 1, M32 - 1]
    return [rnd.choice(edge) if rnd.random() < 0.3 else rnd.getrandbits(32) for _ in range(n)]


class Instance:
    """one v_final of 2^m entries per role on the device: comps[role] = (a, b) as int lists (b None for "plain"), or None where the
    components are the device's own random fill (the twin needs no host copy)"""

    def __init__(self, cozk, ctx, m, comps=None, seed=0):
        self.cozk, self.ctx, self.m, self.comps = cozk, ctx, m, comps
        V, P, n = cozk.Vec, cozk.Rep3DensePolynomial, 1 << m
        self.poly = {}
        for i, role in enumerate(S.ROLES):
            if comps is None:
                a, b = V.random(ctx, n, seed + 10 * i), None if role == "plain" else V.random(ctx, n, seed + 10 * i + 1)
            else:
                a, b = V.from_ints(ctx, comps[role][0]), None if role == "plain" else V.from_ints(ctx, comps[role][1])
            self.poly[role] = P.from_vec_shares(ctx, a, b)
        self.one = cozk.fr_to_mont_limbs([1])[0]

    def twin(self, role, vio, lo, r_eq):
        cozk, ctx, W, n = self.cozk, self.ctx, len(vio), 1 << self.m
        P, V = cozk.Rep3DensePolynomial, cozk.Vec
        pub = np.zeros((n, 4), dtype=np.uint64)
        pub[lo:lo + W] = cozk.fr_to_mont_limbs(vio)
        rng = np.zeros_like(pub)
        rng[lo:lo + W] = self.one
        pio = P.from_vec_shares(ctx, V.from_numpy(ctx, pub))
        mode, party = (cozk.MODE_PLAIN, 0) if role == "plain" else (cozk.MODE_REP3, role)
        d = P.linear_combination([self.poly[role], pio], [1, R - 1], mode, party)
        pio.free()
        return [P.from_vec_shares(ctx, cozk.eq_evals(ctx, r_eq)), P.from_vec_shares(ctx, V.from_numpy(ctx, rng)), d]

    def check(self, role, vio, lo, seed, model=False):
        """-> the rounds and the final of the device calls for `role`, checked against the twin (and the model)"""
        cozk, ctx, m = self.cozk, self.ctx, self.m
        rnd = random.Random(seed)
        r_eq, rs = _challenges(rnd, m), _challenges(rnd, m)
        polys = self.twin(role, vio, lo, r_eq)
        d_vio = cozk.Vec.from_ints(ctx, vio, cozk.SCALAR_U32)
        oc = cozk.OutputCheck.shared(ctx, self.poly[role], d_vio, lo, r_eq, party=0 if role == "plain" else role)
        got_rounds = []
        for k in range(m):
            if k:
                for p in polys:
                    p.bind(rs[k - 1], cozk.HIGH_TO_LOW)
            got = oc.round(rs[k - 1] if k else None)
            assert got == cozk.prod_sumcheck_evals(polys, 3), (m, lo, len(vio), role, k)
            assert len(oc) == len(polys[0]) == 1 << (m - k)
            got_rounds.append(got)
        for p in polys:
            p.bind(rs[-1], cozk.HIGH_TO_LOW)
        fin = oc.final(rs[-1])
        dd = polys[2].get_bound_coeff(0)
        want_d = dd if role == "plain" else (dd[0] + dd[1]) * TWO_INV % R
        assert fin == (polys[0].get_bound_coeff(0), polys[1].get_bound_coeff(0), want_d), (m, lo, len(vio), role)
        assert len(oc) == 1 and len(self.poly[role]) == 1 << m  # v_final is only read
        if model:
            a, b = self.comps[role]
            rounds, want_fin = S.windowed_rounds(role, a, b, vio, lo, r_eq, rs)
            assert got_rounds == rounds and fin == want_fin, (m, lo, len(vio), role)
        oc.free()
        for p in polys:
            p.free()
        return got_rounds, fin, r_eq, rs


def _shared_instance(cozk, ctx, m, rnd, vf=None):
    vf = _words(rnd, 1 << m) if vf is None else vf
    shares = S.share(vf, rnd)
    return Instance(cozk, ctx, m, {role: S.components(role, vf, shares) for role in S.ROLES}), vf


@pytest.mark.parametrize("m", [1, 2, 5, 12, 14])
def test_rounds_and_final_equal_the_dense_twin_for_every_role(cozk, ctx, m):
    rnd = random.Random(600 + m)
    inst = _shared_instance(cozk, ctx, m, rnd)[0] if m <= 6 else Instance(cozk, ctx, m, seed=9000 + m)
    for i, (lo, W) in enumerate(_windows(m)):
        vio = _words(rnd, W)
        for role in S.ROLES:
            inst.check(role, vio, lo, 1000 * m + i, model=m <= 6)


@pytest.mark.parametrize("m", [1, 5, 12])
def test_components_at_both_ends_of_the_field(cozk, ctx, m):
    MEM = 1 << m
    # at 12: no sparse round, one word, and two sides with dots and folds past one workgroup
    wins = [(0, MEM), (MEM - 1, 1), (2048 - 300, 600)] if m == 12 else [(0, MEM), (MEM // 2 - 1, 2), (MEM - 1, 1), (1, MEM - 1)] + ([(3, 5)] if m >= 5 else [])
    top, zero = [R - 1] * MEM, [0] * MEM
    insts = [Instance(cozk, ctx, m, {role: (a, None if role == "plain" else b) for role in S.ROLES}) for a, b in ((top, top), (zero, zero), (top, zero), (zero, top))]
    for i, (lo, W) in enumerate(w for w in wins if w[1] >= 1 and w[0] + w[1] <= MEM):
        for j, inst in enumerate(insts):
            for role in S.ROLES:
                inst.check(role, [M32 if (i + j) % 2 else 0] * W, lo, 7000 + 10 * m + i, model=m <= 6)
                if m <= 6:
                    inst.check(role, [0 if (i + j) % 2 else M32] * W, lo, 7500 + 10 * m + i, model=True)


@pytest.mark.parametrize("m,lo,W", [(5, 13, 9), (12, 2048 - 300, 600)])
def test_three_parties_sum_to_the_rounds_on_the_u32_column(cozk, ctx, m, lo, W):
    rnd = random.Random(800 + m)
    inst, vf = _shared_instance(cozk, ctx, m, rnd)
    vio = _words(rnd, W)
    seed = 8100 + m
    got = {role: inst.check(role, vio, lo, seed) for role in S.ROLES}
    _, _, r_eq, rs = got["plain"]
    oc = cozk.OutputCheck(ctx, cozk.Vec.from_ints(ctx, vf, cozk.SCALAR_U32), cozk.Vec.from_ints(ctx, vio, cozk.SCALAR_U32), lo, r_eq)
    for k in range(m):
        want = oc.round(rs[k - 1] if k else None)
        assert want == got["plain"][0][k], k
        assert [sum(got[p][0][k][e] for p in range(3)) % R for e in range(3)] == want, k
    fin = oc.final(rs[-1])
    assert fin == got["plain"][1] and sum(got[p][1][2] for p in range(3)) % R == fin[2]
    assert all(got[p][1][:2] == fin[:2] for p in range(3))
    oc.free()


def test_refusals(cozk, ctx):
    V, P, U32 = cozk.Vec, cozk.Rep3DensePolynomial, cozk.SCALAR_U32
    rnd = random.Random(4)
    vals = [rnd.randrange(R) for _ in range(8)]
    a, b = [rnd.randrange(R) for _ in range(8)], [rnd.randrange(R) for _ in range(8)]
    plain, rep3 = P.from_vec_shares(ctx, V.from_ints(ctx, vals)), P.from_vec_shares(ctx, V.from_ints(ctx, a), V.from_ints(ctx, b))
    vio, r_eq = V.from_ints(ctx, [1, 2, 3], U32), [5, 6, 7]

    def refused(text, *args, **kw):
        with pytest.raises(cozk.CozkError) as e:
            cozk.OutputCheck.shared(ctx, *args, **kw)
        assert e.value.code == INVALID_ARG and "output_check_shared_create: " in str(e.value) and text in str(e.value), str(e.value)
    refused("null argument", None, vio, 0, r_eq)
    refused("null argument", rep3, None, 0, r_eq)
    refused("null argument", rep3, vio, 0, None)
    refused("v_final has 2^m entries", P.from_vec_shares(ctx, V.from_ints(ctx, vals[:6])), vio, 0, r_eq)
    refused("v_final has 2^m entries", P.from_vec_shares(ctx, V.from_ints(ctx, [9])), V.from_ints(ctx, [9], U32), 0, [])
    bound = P.from_vec_shares(ctx, V.from_ints(ctx, vals), V.from_ints(ctx, a))
    bound.bind(3, cozk.HIGH_TO_LOW)
    refused("v_final is bound", bound, vio, 0, r_eq[:2], party=1)
    refused("party is 0..2 for a REP3 v_final and 0 for a PLAIN one", rep3, vio, 0, r_eq, party=3)
    refused("party is 0..2 for a REP3 v_final and 0 for a PLAIN one", rep3, vio, 0, r_eq, party=-1)
    refused("party is 0..2 for a REP3 v_final and 0 for a PLAIN one", plain, vio, 0, r_eq, party=1)
    refused("v_io is a U32 vector", rep3, V.from_ints(ctx, [1, 2, 3], cozk.SCALAR_U8), 0, r_eq)
    refused("v_io is a U32 vector", plain, V.from_ints(ctx, [1, 2, 3]), 0, r_eq)
    refused("io_len is 0", rep3, V.alloc(ctx, 0, U32), 0, r_eq)
    refused("io_start + io_len > MEM", rep3, vio, 6, r_eq, party=2)
    refused("io_start + io_len > MEM", plain, vio, 9, r_eq)
    refused("io_start + io_len > MEM", rep3, vio, 2 ** 64 - 1, r_eq)
    n_dev = ctypes.c_int(0)
    cozk._lib.lib().cozk_device_count(ctypes.byref(n_dev))
    if n_dev.value >= 2:
        other = cozk.Context(1)
        refused("live on the context's device", P.from_vec_shares(other, V.from_ints(other, vals)), vio, 0, r_eq)
        refused("live on the context's device", rep3, V.from_ints(other, [1, 2, 3], U32), 0, r_eq)
        other.close()
    oc = cozk.OutputCheck.shared(ctx, rep3, vio, 5, r_eq, party=1)

    def call_refused(text, f, *args):
        with pytest.raises(cozk.CozkError) as e:
            f(*args)
        assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
    call_refused("round 0 takes no challenge", oc.round, 11)
    call_refused("more than one variable is left", oc.final, 11)
    first = oc.round()
    call_refused("binds the previous variable", oc.round, None)
    oc.round(11)
    oc.round(12)
    call_refused("one variable is left", oc.round, 13)
    call_refused("null argument", oc.final, None)
    fin = oc.final(13)
    call_refused("more than one variable is left", oc.final, 13)  # nothing is left
    # the refused calls changed nothing: the same numbers as the restatement, and the context works on
    rounds, want_fin = S.windowed_rounds(1, a, b, [1, 2, 3], 5, r_eq, [11, 12, 13])
    assert first == rounds[0] and fin == want_fin
    oc.free()


def test_a_handle_freed_mid_way_leaves_the_context_working(cozk, ctx):
    rnd = random.Random(9)
    m, lo, W = 12, 1000, 300
    inst = Instance(cozk, ctx, m, seed=77)
    vio = _words(rnd, W)
    oc = cozk.OutputCheck.shared(ctx, inst.poly[2], cozk.Vec.from_ints(ctx, vio, cozk.SCALAR_U32), lo, _challenges(rnd, m), party=2)
    oc.round()
    oc.round(3)
    oc.round(R - 1)
    oc.free()
    oc.free()
    for role in S.ROLES:
        inst.check(role, vio, lo, 91)
