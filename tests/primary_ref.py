"""What the primary sumcheck's form tests share (tests/test_primary_forms_model.py on the CPU, tests/test_gpu_primary_forms.py on
the device):
  * the table of collation forms that cozk_primary_create admits -- memory count and chunk range per form (include/cozk.h);
  * the DIRECT reference of a round message: sum over index pairs of eq(X) (sum_i flag_i(X) g_i(E(X)) - out(X)) at
    X = 0, 2, .., D from pyprimary.g_plain on opened values alone -- no item lists, no multiplication schedule, no shares;
  * instances (public eq and flags, E and lookup_outputs as plain values and as Rep3 shares), the reference state that
    oracle/pyprimary.py's prover_message runs on, and a driver that runs one plain cozk_primary, or three Rep3 ones on three
    contexts of one device in lock-step, with the ring reshare done by cozk_copy between the levels.
Expected values come from the oracle and the direct sum only; the driver holds no protocol logic beyond the exchange."""
import ctypes

import numpy as np

import pyprimary as P
import pyref as O

R = O.R
L2H = O.LOW_TO_HIGH
LINEAR = (P.CONCAT, P.NOT_FIRST, P.ZERO)

# form -> (name, memory count as a function of the chunk count C, admitted C)
FORMS = {
    P.PRODUCT: ("PRODUCT", lambda C: C, range(1, 7)),
    P.NOT_PRODUCT: ("NOT_PRODUCT", lambda C: C, range(1, 7)),
    P.LTU: ("LTU", lambda C: 2 * C - 1, range(1, 7)),
    P.NOT_LTU: ("NOT_LTU", lambda C: 2 * C - 1, range(1, 7)),
    P.LTE: ("LTE", lambda C: 2 * C, range(1, 7)),
    P.DIV0: ("DIV0", lambda C: 2 * C, range(1, 7)),
    P.UNSIGNED_REM: ("UNSIGNED_REM", lambda C: 3 * C - 1, range(1, 7)),
    P.SLT: ("SLT", lambda C: 2 * C + 1, range(2, 5)),
    P.NOT_SLT: ("NOT_SLT", lambda C: 2 * C + 1, range(2, 5)),
    P.SIGNED_REM: ("SIGNED_REM", lambda C: 4 * C + 2, range(2, 5)),
}
PAIRS = [(f, C) for f, (_, _, cs) in FORMS.items() for C in cs]
PAIR_IDS = ["%s-C%d" % (FORMS[f][0], C) for f, C in PAIRS]


# tables of linear forms only: sumcheck degree 3
LINEAR_TABLES = {
    "concat-1": [P.Instr(P.CONCAT, [0], 16)],
    "concat-2": [P.Instr(P.CONCAT, [1, 0], 16)],
    "concat-13": [P.Instr(P.CONCAT, range(13), 16)],
    "concat-20": [P.Instr(P.CONCAT, range(20), 10)],
    "concat-bits0": [P.Instr(P.CONCAT, range(4), 0)],
    "concat-repeated": [P.Instr(P.CONCAT, [2, 2, 0, 1], 8)],
    "not-first": [P.Instr(P.NOT_FIRST, [1, 0])],
    "zero": [P.Instr(P.ZERO, [0])],
    "all-three": [P.Instr(P.CONCAT, [0, 1], 16), P.Instr(P.NOT_FIRST, [1]), P.Instr(P.ZERO, [0])],
}


def n_mems(form, C):
    return FORMS[form][1](C)


def form_instr(form, C, first=0):
    """the form at chunk count C over the memories first .. first + n_mems - 1"""
    return P.Instr(form, range(first, first + n_mems(form, C)))


def pair_table(form, C):
    """the form alone beside a one-memory CONCAT, which keeps the linear pass non-trivial"""
    return [form_instr(form, C), P.Instr(P.CONCAT, [0], 0)]


def levels(instr):
    """exchanges per round of one instruction: the reshared multiplications that precede its last, local one (a chain of t
    factors reshares t - 2 prefix products; SLT and SIGNED_REM reshare their sum after the C - 2 links of its EQ chain)"""
    C = instr.chunks()
    if instr.form in LINEAR:
        return 0
    if instr.form in (P.SLT, P.NOT_SLT, P.SIGNED_REM):
        return C - 1
    return max(C - 2, 0)


def count_items(instrs, flags):
    """(index pair, multiplicative instruction) with a non-zero flag in the pair"""
    half = len(flags[0]) // 2
    return sum(1 for ii, ins in enumerate(instrs) if ins.form not in LINEAR for i in range(half) if flags[ii][2 * i] % R or flags[ii][2 * i + 1] % R)


def direct_message(instrs, eq, flags, E, outs):
    """the round message from opened values: E[m], outs plain coefficient lists"""
    D = P.sumcheck_degree(instrs)
    ev = [0] * D
    for i in range(len(eq) // 2):
        for k in range(D):
            X = 0 if k == 0 else k + 1
            at = lambda c: (c[2 * i] + X * (c[2 * i + 1] - c[2 * i])) % R
            cache = {}
            inner = 0
            for ii, ins in enumerate(instrs):
                f = at(flags[ii])
                if f == 0:
                    continue
                for m in ins.mems:
                    if m not in cache:
                        cache[m] = at(E[m])
                inner += f * P.g_plain(ins, [cache[m] for m in ins.mems])
            ev[k] = (ev[k] + at(eq) * (inner - at(outs))) % R
    return ev


class Instance:
    """public eq and flag columns, E and lookup_outputs as plain values (.E, .outs) and as three parties' Rep3 shares
    (.E3[p][m], .outs3[p]); flags random 0/1 (not one-hot: the message is defined regardless), one-hot, or all zero for the
    instructions listed in `zero_flags`"""

    def __init__(self, instrs, n, seed, n_mem=None, one_hot=False, zero_flags=()):
        rng = O.SplitMix64(seed)
        self.instrs, self.n = list(instrs), n
        self.n_mem = n_mem if n_mem is not None else max(max(i.mems) for i in instrs) + 1
        self.eq = O.eq_evals([rng.field() for _ in range(n.bit_length() - 1)])
        k = len(self.instrs)
        if one_hot:
            live = [ii for ii in range(k) if ii not in zero_flags]
            hot = [live[rng.next() % len(live)] for _ in range(n)]
            self.flags = [[1 if hot[j] == ii else 0 for j in range(n)] for ii in range(k)]
        else:
            self.flags = [[0 if ii in zero_flags else rng.next() & 1 for _ in range(n)] for ii in range(k)]
        self.E = [[rng.field() for _ in range(n)] for _ in range(self.n_mem)]
        self.outs = [rng.field() for _ in range(n)]
        sh = [[O.rep3_share(v, rng) for v in col] for col in self.E]
        so = [O.rep3_share(v, rng) for v in self.outs]
        self.E3 = [[[s[p] for s in col] for col in sh] for p in range(3)]
        self.outs3 = [[s[p] for s in so] for p in range(3)]

    def parties(self, nparties):
        """(E[p][m], outs[p]) as prover_message and the driver take them"""
        return ([self.E], [self.outs]) if nparties == 1 else (self.E3, self.outs3)


class RefState:
    """the state of prove_primary_sumcheck_inner in big integers: messages by oracle/pyprimary.py, binds LowToHigh"""

    def __init__(self, instrs, eq, flags, E, outs):
        self.instrs = list(instrs)
        self.eq, self.flags = list(eq), [list(f) for f in flags]
        self.E = [[list(m) for m in Ep] for Ep in E]
        self.outs = [list(o) for o in outs]

    @classmethod
    def of(cls, inst, nparties):
        E, outs = inst.parties(nparties)
        return cls(inst.instrs, inst.eq, inst.flags, E, outs)

    def total(self):
        """the coordinator's sum of the parties' prover_message"""
        return O.combine_additive(P.prover_message(self.instrs, self.eq, self.flags, self.E, self.outs))

    def opened(self, cols):
        """cols[p] = one column per party -> the plain column (Rep3: the sum of the a components)"""
        if len(cols) == 1:
            return [v % R for v in cols[0]]
        return [sum(c[j][0] for c in cols) % R for j in range(len(cols[0]))]

    def direct(self):
        E = [self.opened([Ep[m] for Ep in self.E]) for m in range(len(self.E[0]))]
        return direct_message(self.instrs, self.eq, self.flags, E, self.opened(self.outs))

    def n_items(self):
        return count_items(self.instrs, self.flags)

    def bind(self, r):
        self.eq = O.public_bind(self.eq, r, L2H)
        self.flags = [O.public_bind(f, r, L2H) for f in self.flags]
        self.E = [[O.dense_bind(m, r, L2H) for m in Ep] for Ep in self.E]
        self.outs = [O.dense_bind(o, r, L2H) for o in self.outs]

    def finals(self, p):
        """party p's final_evals of the fully bound state"""
        return [m[0] for m in self.E[p]], [f[0] for f in self.flags], self.outs[p][0], self.eq[0]


def rows(LK, instrs):
    return [LK.PrimaryInstr.of(i.form, i.mems, i.bits) for i in instrs]


def _copy(cozk, ctx, dst, src, nbytes):
    lib = cozk._lib.lib()
    lib.cozk_copy.restype = ctypes.c_int
    lib.cozk_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    ctx.check(lib.cozk_copy(ctx.h, dst, src, nbytes))


def read_fr(cozk, ctx, ptr, n):
    """n field elements at a device address, as canonical ints"""
    host = np.zeros((max(n, 1), 4), dtype=np.uint64)
    _copy(cozk, ctx, host.ctypes.data, ptr, 32 * n)
    return cozk.mont_limbs_to_int(host[:n])


class Run:
    """one plain cozk_primary on ctxs[0], or three Rep3 ones on ctxs[0..2], driven in lock-step.  `flags` = 0/1 columns (uploaded
    as U8) unless flags_fr (FR vectors: the already-bound path); keys[p] = party p's PRF key (party p masks with keys[p] and
    keys[p - 1]); capture = (round, level): keep the parties' send buffers of that exchange in .captured"""

    def __init__(self, cozk, LK, ctxs, instrs, eq, flags, E, outs, seed=1, keys=None, flags_fr=False, capture=None):
        self.cozk, self.LK = cozk, LK
        self.np_ = len(E)
        assert self.np_ in (1, 3) and len(ctxs) >= self.np_
        self.ctxs = list(ctxs[:self.np_])
        self.mode = cozk._lib.MODE_PLAIN if self.np_ == 1 else cozk._lib.MODE_REP3
        self.keys = keys if keys is not None else [O.harness_prf_key(seed, p) for p in range(3)]
        self.counter, self.round_no, self.capture, self.captured = 0, 0, capture, None
        self.prims = [create(cozk, LK, self.ctxs[p], self.mode, p, rows(LK, instrs), flags, E[p], outs[p], eq, flags_fr) for p in range(self.np_)]

    def degree(self):
        d = {pr.degree() for pr in self.prims}
        assert len(d) == 1
        return d.pop()

    def round(self, r=None):
        """one round on every party -> (the parties' messages, n_items, n_levels, n_elems per level)"""
        begun = [pr.round_begin(r) for pr in self.prims]
        assert all(b == begun[0] for b in begun), begun
        n_items, n_levels = begun[0]
        elems = []
        for level in range(1, n_levels + 1):
            out = [self.prims[p].level(level, self.keys[p], self.keys[(p + 2) % 3], self.counter) if self.np_ == 3 else self.prims[p].level(level)
                   for p in range(self.np_)]
            n = out[0][2]
            assert all(o[2] == n for o in out), out
            elems.append(n)
            if self.np_ == 3 and n:
                for c in self.ctxs:
                    c.synchronize()
                if self.capture == (self.round_no, level):
                    self.captured = [read_fr(self.cozk, self.ctxs[p], out[p][0], n) for p in range(3)]
                for p in range(3):  # the ring reshare: party p's new additive shares become the next party's b components
                    q = (p + 1) % 3
                    _copy(self.cozk, self.ctxs[q], out[q][1], out[p][0], 32 * n)
                self.counter += n
        msgs = [pr.round_finish() for pr in self.prims]
        self.round_no += 1
        return msgs, n_items, n_levels, elems

    def finals(self, r):
        return [pr.final_evals(r) for pr in self.prims]

    def free(self):
        for pr in self.prims:
            pr.free()


def create(cozk, LK, ctx, mode, party, table, flags, E, outs, eq, flags_fr=False):
    """uploads one party's columns and creates its cozk_primary; everything is copied by the create, so the uploads are freed"""
    Vec, Poly = cozk.Vec, cozk.Rep3DensePolynomial
    kind = cozk._lib.SCALAR_FR if flags_fr else cozk._lib.SCALAR_U8
    fl = [Vec.from_ints(ctx, f, kind=kind) for f in flags]
    Ep = [Poly.new(ctx, m) for m in E]
    op, ev = Poly.new(ctx, outs), Vec.from_ints(ctx, eq)
    try:
        return LK.PrimarySumcheck.create(ctx, mode, party, table, fl, Ep, op, ev)
    finally:
        for x in fl + Ep + [op, ev]:
            x.free()


def total(msgs):
    return O.combine_additive(msgs)
