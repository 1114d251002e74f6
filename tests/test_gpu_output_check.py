"""GPU tests of the windowed output check (cozk_output_check_*, csrc/output_check.inc): every round and the final of the device calls
equal, as integers, a twin driven by cozk_eq_evals, cozk_prod_sumcheck_evals and cozk_poly_bind on Fr copies of the three MEM-entry
vectors, and at m <= 6 the plain-Python restatement tests/output_check_ref.py, at log_mem = 1, 2, 5, 12 and 14 for windows of one word,
the whole memory (no sparse round), the last word, an aligned half, windows across an aligned boundary (two sides), W = 2^j + 1 and
seeded random windows -- at 14 also 5000 words across a multiple of 8192, where the dots and the folds go past one workgroup -- with
v_final all 0xFFFFFFFF against v_io 0 and the converse (d at both ends of the signed 33-bit range) and challenges 0, 1 and p - 1 among
random ones; every refusal with its text; a handle freed mid-way.  A vector on another device is checked where a second device exists."""
import ctypes
import random

import numpy as np
import pytest

import output_check_ref as OC

pytestmark = pytest.mark.gpu
R, M32 = OC.R, OC.M32
INVALID_ARG = -1


def _windows(m):
    MEM = 1 << m
    if m <= 6:
        return OC.windows(m, 40 + m)
    rnd = random.Random(50 + m)
    out = [(0, 1), (0, MEM), (MEM - 1, 1), (0, MEM // 2), (MEM // 2, MEM // 2), (MEM // 2 - 1, 2)]
    for j in (0, 1, 7, 8, m - 2, m - 1):  # 2^7 + 1 = 129 and 2^8 + 1 = 257: one workgroup of dots and the first past it
        W = (1 << j) + 1
        out += [(0, W), (MEM - W, W), ((MEM - W) // 2 | 1, W)]
    for _ in range(3):
        W = rnd.randint(1, MEM)
        out.append((rnd.randint(0, MEM - W), W))
    if m == 14:
        out.append((8192 - 2500, 5000))
    return [w for i, w in enumerate(out) if w[0] + w[1] <= MEM and w not in out[:i]]


def _challenges(rnd, m):
    special = [0, 1, R - 1]
    return [rnd.choice(special) if rnd.random() < 0.25 else rnd.randrange(R) for _ in range(m)]


def _limbs(cozk, values):
    return cozk.fr_to_mont_limbs(values)


class Instance:
    """one v_final of 2^m words on the device, with its Montgomery limbs kept for the twin's Fr copies"""

    def __init__(self, cozk, ctx, m, vf):
        self.cozk, self.ctx, self.m, self.vf = cozk, ctx, m, vf
        self.d_vf = cozk.Vec.from_ints(ctx, vf, cozk.SCALAR_U32)
        self.vf_limbs = _limbs(cozk, vf)
        self.one = _limbs(cozk, [1])[0]

    def twin(self, vio, lo, r_eq):
        cozk, ctx, W = self.cozk, self.ctx, len(vio)
        d = self.vf_limbs.copy()
        d[lo:lo + W] = _limbs(cozk, [(a - b) % R for a, b in zip(self.vf[lo:lo + W], vio)])
        rng = np.zeros_like(d)
        rng[lo:lo + W] = self.one
        P = cozk.Rep3DensePolynomial
        return [P.from_vec_shares(ctx, cozk.eq_evals(ctx, r_eq)), P.from_vec_shares(ctx, cozk.Vec.from_numpy(ctx, rng)), P.from_vec_shares(ctx, cozk.Vec.from_numpy(ctx, d))]

    def check(self, vio, lo, seed, model=False):
        cozk, ctx, m = self.cozk, self.ctx, self.m
        rnd = random.Random(seed)
        r_eq, rs = _challenges(rnd, m), _challenges(rnd, m)
        polys = self.twin(vio, lo, r_eq)
        d_vio = cozk.Vec.from_ints(ctx, vio, cozk.SCALAR_U32)
        oc = cozk.OutputCheck(ctx, self.d_vf, d_vio, lo, r_eq)
        got_rounds = []
        for k in range(m):
            if k:
                for p in polys:
                    p.bind(rs[k - 1], cozk.HIGH_TO_LOW)
            got = oc.round(rs[k - 1] if k else None)
            assert got == cozk.prod_sumcheck_evals(polys, 3), (m, lo, len(vio), k)
            assert len(oc) == len(polys[0]) == 1 << (m - k)
            got_rounds.append(got)
        for p in polys:
            p.bind(rs[-1], cozk.HIGH_TO_LOW)
        fin = oc.final(rs[-1])
        assert fin == tuple(p.get_bound_coeff(0) for p in polys), (m, lo, len(vio))
        assert len(oc) == 1
        if model:
            rounds, want_fin, _ = OC.windowed_rounds(self.vf, vio, lo, r_eq, rs)
            assert got_rounds == rounds and fin == want_fin, (m, lo, len(vio))
        oc.free()
        for p in polys:
            p.free()


def _words(rnd, n):
    edge = [0, M32, 1, M32 - 1]
    return [rnd.choice(edge) if rnd.random() < 0.3 else rnd.getrandbits(32) for _ in range(n)]


@pytest.mark.parametrize("m", [1, 2, 5, 12, 14])
def test_rounds_and_final_equal_the_dense_twin(cozk, ctx, m):
    rnd = random.Random(600 + m)
    inst = Instance(cozk, ctx, m, _words(rnd, 1 << m))
    for i, (lo, W) in enumerate(_windows(m)):
        inst.check(_words(rnd, W), lo, 1000 * m + i, model=m <= 6)


@pytest.mark.parametrize("m", [1, 5, 12, 14])
def test_d_at_both_ends_of_its_range(cozk, ctx, m):
    MEM = 1 << m
    wins = [(0, MEM), (MEM // 2 - 1, 2), (MEM - 1, 1), (1, MEM - 1)] + ([(3, 5)] if m >= 5 else []) + ([(8192 - 2500, 5000)] if m == 14 else [])
    top, zero = Instance(cozk, ctx, m, [M32] * MEM), Instance(cozk, ctx, m, [0] * MEM)
    for i, (lo, W) in enumerate(w for w in wins if w[1] >= 1 and w[0] + w[1] <= MEM):
        top.check([0] * W, lo, 7000 + 10 * m + i, model=m <= 6)   # d = 2^32 - 1 everywhere
        zero.check([M32] * W, lo, 7500 + 10 * m + i, model=m <= 6)  # d = -(2^32 - 1) in the window


def test_refusals(cozk, ctx):
    V, U32 = cozk.Vec, cozk.SCALAR_U32
    vf, vio = V.from_ints(ctx, list(range(8)), U32), V.from_ints(ctx, [1, 2, 3], U32)
    r_eq = [5, 6, 7]

    def refused(text, *args):
        with pytest.raises(cozk.CozkError) as e:
            cozk.OutputCheck(ctx, *args)
        assert e.value.code == INVALID_ARG and "output_check_create: " in str(e.value) and text in str(e.value), str(e.value)
    refused("null argument", None, vio, 0, r_eq)
    refused("null argument", vf, None, 0, r_eq)
    refused("null argument", vf, vio, 0, None)
    refused("v_final is a U32 vector", V.from_ints(ctx, list(range(8)), cozk.SCALAR_U64), vio, 0, r_eq)
    refused("v_final is a U32 vector", V.from_ints(ctx, list(range(8))), vio, 0, r_eq)
    refused("v_final has 2^m entries", V.from_ints(ctx, list(range(6)), U32), vio, 0, r_eq)
    refused("v_final has 2^m entries", V.from_ints(ctx, [9], U32), V.from_ints(ctx, [9], U32), 0, [])
    refused("v_io is a U32 vector", vf, V.from_ints(ctx, [1, 2, 3], cozk.SCALAR_U8), 0, r_eq)
    refused("io_len is 0", vf, V.alloc(ctx, 0, U32), 0, r_eq)
    refused("io_start + io_len > MEM", vf, vio, 6, r_eq)
    refused("io_start + io_len > MEM", vf, vio, 9, r_eq)
    refused("io_start + io_len > MEM", vf, vio, 2 ** 64 - 1, r_eq)
    n_dev = ctypes.c_int(0)
    cozk._lib.lib().cozk_device_count(ctypes.byref(n_dev))
    if n_dev.value >= 2:
        other = cozk.Context(1)
        refused("live on the context's device", V.from_ints(other, list(range(8)), U32), vio, 0, r_eq)
        refused("live on the context's device", vf, V.from_ints(other, [1, 2, 3], U32), 0, r_eq)
        other.close()
    oc = cozk.OutputCheck(ctx, vf, vio, 5, r_eq)

    def call_refused(text, f, *args):
        with pytest.raises(cozk.CozkError) as e:
            f(*args)
        assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
    call_refused("round 0 takes no challenge", oc.round, 11)
    call_refused("more than one variable is left", oc.final, 11)
    first = oc.round()
    call_refused("binds the previous variable", oc.round, None)
    call_refused("more than one variable is left", oc.final, 11)
    oc.round(11)
    oc.round(12)
    call_refused("one variable is left", oc.round, 13)
    call_refused("null argument", oc.final, None)
    fin = oc.final(13)
    call_refused("more than one variable is left", oc.final, 13)  # nothing is left
    call_refused("one variable is left", oc.round, 13)
    # the refused calls changed nothing: the same numbers as the restatement, and the context works on
    rounds, want_fin, _ = OC.windowed_rounds(list(range(8)), [1, 2, 3], 5, r_eq, [11, 12, 13])
    assert first == rounds[0] and fin == want_fin
    oc.free()


def test_a_handle_freed_mid_way_leaves_the_context_working(cozk, ctx):
    rnd = random.Random(9)
    m, lo, W = 12, 1000, 300
    vf, vio = _words(rnd, 1 << m), _words(rnd, W)
    inst = Instance(cozk, ctx, m, vf)
    oc = cozk.OutputCheck(ctx, inst.d_vf, cozk.Vec.from_ints(ctx, vio, cozk.SCALAR_U32), lo, _challenges(rnd, m))
    oc.round()
    oc.round(3)
    oc.round(R - 1)
    oc.free()
    oc.free()
    inst.check(vio, lo, 91)
