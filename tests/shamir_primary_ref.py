"""Big-int restatement of Lasso's primary sumcheck proved by n Shamir parties (cozk_shamir_primary_*, csrc/host/shamir_primary.hpp) and
of the level groups its exchanges run as (cozk_primary_group_*, csrc/primary_group.inc), on top of oracle/pyprimary.py (forms, g_plain,
the coordinator's step), oracle/pylookups.py (the lookups harness's instance), tests/primary_ref.py, tests/shamir_ref.py,
tests/shamir_mul_ref.py and the mask derivation of tests/shamir_gp_ref.py.  The reference has no Shamir prover, so this file IS the
statement the device code is held to.

t = degree, n = parties, party p evaluates at p + 1; 1 <= t, 2t + 1 <= n; the senders are parties 0..2t.

  programs    compile(instr): the straight-line program of csrc/primary_sumcheck.inc prim_compile -- every reshared value (a SLOT) is a
              sum of products of TWO affine forms (+ one affine form), slots are grouped in LEVELS, the last step stays local.
  items       flags are public: (index pair, multiplicative instruction) with a non-zero flag in the pair, grouped by instruction;
              slot q of level L of item j of instruction group s at evaluation point k lives at
                  pos = base[L][s] + ((j * nq_s[L] + q) * D + k)                                    (prim_slot_pos)
  level       sender p evaluates the slots of the level on ITS values (memories: its shares; earlier slots: its level buffers; a
              constant is added to every party's value: the constant sharing): z_p[pos], a point of a degree-2t sharing
  exchange    shamir_mul_ref's re-deal of z_p with mul keys, counter + pos: h[p -> q] = shamir_ref.share_vec(z_p, keys_p, t, 2t + 1,
              counter); receiver q stores sum_p lambda_p h[p -> q][pos], lambda = lagrange(1..2t + 1): a degree-t sharing again.
              Exchange e (only those with n_elems > 0, in the order they happen) uses mul_counter + sum of the earlier n_elems.
  message     sender p's D evaluations from the last, local step + the linear pass; + zero_p[D round + k], opened with lagrange(1..2t + 1)
  finals      E_m(r), lookup_outputs(r) from parties 0..t with lagrange(1..t + 1), unmasked; flags(r) public
  transcript  "cozk-lookups", r_eq first; the proof is oracle/pyprimary.prove's"""
import hashlib

import pylookups as LK
import pyprimary as P
import pyref as O
import shamir_gp_ref as G
import shamir_ref as S

R = O.R
L2H = O.LOW_TO_HIGH
SHARE_TAG, RAND_TAG, MUL_TAG = 0x53484152, 0x52414E44, 0x4D554C54
LINEAR = (P.CONCAT, P.NOT_FIRST, P.ZERO)
MAX_LEVELS = 4


def share_keys(seed, degree):
    return [O.harness_prf_key(seed ^ SHARE_TAG, c) for c in range(degree)]


def rand_keys(seed, num_parties, degree):
    return [[O.harness_prf_key(seed ^ RAND_TAG, 64 * p + j) for j in range(3 * degree + 1)] for p in range(num_parties)]


def mul_keys(seed, num_parties, degree):
    return [[O.harness_prf_key(seed ^ MUL_TAG, 64 * p + c) for c in range(degree)] for p in range(num_parties)]


# ------------------------------------------------------------------------------------------------ programs
# an affine form: (c0, [(coef, kind, index)]) with kind "m" (position in the instruction's memories) or "s" (slot number)
def _mem(pos, c=1):
    return (0, [(c, "m", pos)])


def _slot(s, c=1):
    return (0, [(c, "s", s)])


def _neg(l):
    return (-l[0], [(-c, k, i) for c, k, i in l[1]])


def _one_minus(l):
    n = _neg(l)
    return (n[0] + 1, n[1])


def _plus(a, b):
    return (a[0] + b[0], a[1] + b[1])


class Program:
    """slots: dicts (level, q, prods = [(x, y)], add = affine form or None); fin: [(x, y)]; fin_add: affine form"""

    def __init__(self):
        self.slots, self.nq, self.fin, self.fin_add = [], [0] * MAX_LEVELS, [], (0, [])

    @property
    def n_levels(self):
        return max([s["level"] for s in self.slots], default=0)

    def add_slot(self, level, prods, add=None):
        assert 1 <= level <= MAX_LEVELS
        q = self.nq[level - 1]
        self.nq[level - 1] += 1
        self.slots.append(dict(level=level, q=q, prods=list(prods), add=add))
        return len(self.slots) - 1

    def prefix(self, pos, count):
        """prefix products P_0 = m_0, P_t = P_{t-1} m_t (level t)"""
        out = []
        if count <= 0:
            return out
        out.append(_mem(pos[0]))
        for t in range(1, count):
            out.append(_slot(self.add_slot(t, [(out[t - 1], _mem(pos[t]))])))
        return out

    def ltu_part(self, C, l0, e0, n_eq):
        self.fin_add = _plus(self.fin_add, _mem(l0))
        Pr = self.prefix([e0 + t for t in range(n_eq)], min(n_eq, C - 1))
        for i in range(1, C):
            self.fin.append((_mem(l0 + i), Pr[i - 1]))
        return Pr

    def product_part(self, p0, n, negated):
        if n == 1:
            self.fin_add = _plus(self.fin_add, _mem(p0, -1 if negated else 1))
            return
        Pr = self.prefix([p0 + t for t in range(n)], n - 1)
        self.fin.append((_neg(Pr[n - 2]) if negated else Pr[n - 2], _mem(p0 + n - 1)))

    def negate_result(self):
        self.fin = [(_neg(x), y) for x, y in self.fin]
        self.fin_add = _one_minus(self.fin_add)


def compile(instr):
    """prim_compile for a multiplicative form"""
    f, n, C = instr.form, len(instr.mems), instr.chunks()
    assert f not in LINEAR
    b = Program()
    if f in (P.PRODUCT, P.NOT_PRODUCT):
        b.product_part(0, n, False)
    elif f in (P.LTU, P.NOT_LTU):
        b.ltu_part(C, 0, C, C - 1)
    elif f == P.LTE:
        if C == 1:
            b.fin_add = _plus(_mem(0), _mem(1))
        else:
            Pr = b.ltu_part(C, 0, C, C)
            b.fin.append((Pr[C - 2], _mem(2 * C - 1)))
    elif f == P.UNSIGNED_REM:
        b.ltu_part(C, 0, C, C - 1)
        b.product_part(2 * C - 1, C, False)
    elif f == P.DIV0:
        b.fin_add = (1, [])
        b.product_part(0, C, True)
        b.product_part(C, C, False)
    elif f in (P.SLT, P.NOT_SLT):
        l, r, ltu0, eq0, lt_abs, eq_abs = 0, 1, 2, C + 1, 2 * C - 1, 2 * C
        Pr = b.prefix([eq_abs] + [eq0 + t for t in range(C - 2)], C - 1)
        Lr = max(1, C - 1)
        lnr = b.add_slot(Lr, [(_mem(l), _one_minus(_mem(r)))])
        lr = b.add_slot(Lr, [(_mem(l), _mem(r))])
        nlnr = b.add_slot(Lr, [(_one_minus(_mem(l)), _one_minus(_mem(r)))])
        Ss = b.add_slot(Lr, [(_mem(ltu0 + i), Pr[i]) for i in range(C - 1)], _mem(lt_abs))
        b.fin_add = _slot(lnr)
        b.fin.append((_plus(_slot(lr), _slot(nlnr)), _slot(Ss)))
    else:
        assert f == P.SIGNED_REM
        l, r, eq0, ltu0, eq_abs, lt_abs, lz0, rz0 = 0, 1, 2, C + 1, 2 * C, 2 * C + 1, 2 * C + 2, 3 * C + 2
        Pr = b.prefix([eq_abs] + [eq0 + t for t in range(C - 1)], C)
        LZ = b.prefix([lz0 + t for t in range(C)], C)
        lr = b.add_slot(1, [(_mem(l), _mem(r))])
        nlr = b.add_slot(1, [(_one_minus(_mem(l)), _mem(r))])
        Ss = b.add_slot(max(1, C - 1), [(_mem(ltu0 + i), Pr[i]) for i in range(C - 1)], _mem(lt_abs))
        b.fin.append((_plus(_one_minus(_mem(l)), _mem(r, -1)), _slot(Ss)))
        b.fin.append((_slot(lr), _one_minus(Pr[C - 1])))
        b.fin.append((_slot(nlr), LZ[C - 1]))
        b.product_part(rz0, C, False)
    if f in (P.NOT_PRODUCT, P.NOT_LTU, P.NOT_SLT):
        b.negate_result()
    return b


# ------------------------------------------------------------------------------------------------ one round on the senders' values
def _at(col, i, X):
    return (col[2 * i] + X * (col[2 * i + 1] - col[2 * i])) % R


class Round:
    """the public shape of one round (items, level buffers) and the senders' arithmetic on it.  E[p][m], outs[p]: sender p's current
    columns; eq, flags public"""

    def __init__(self, instrs, eq, flags, E, outs):
        self.instrs, self.eq, self.flags, self.E, self.outs = instrs, eq, flags, E, outs
        self.k = len(E)
        self.D = P.sumcheck_degree(instrs)
        self.half = len(eq) // 2
        self.mul = [ii for ii, ins in enumerate(instrs) if ins.form not in LINEAR]
        self.progs = {ii: compile(instrs[ii]) for ii in self.mul}
        self.max_levels = max([self.progs[ii].n_levels for ii in self.mul], default=0)
        self.items = [[i for i in range(self.half) if flags[ii][2 * i] % R or flags[ii][2 * i + 1] % R] for ii in self.mul]
        self.n_items = sum(len(g) for g in self.items)
        self.n_levels = self.max_levels if self.n_items else 0
        self.base, self.level_elems = [], []
        for t in range(MAX_LEVELS):
            run, bs = 0, []
            for s, ii in enumerate(self.mul):
                bs.append(run)
                run += len(self.items[s]) * self.progs[ii].nq[t] * self.D
            self.base.append(bs)
            self.level_elems.append(run if self.n_items and t < self.max_levels else 0)
        self.bufs = [[None] * MAX_LEVELS for _ in range(self.k)]  # bufs[p][level - 1]: sender p's level buffer

    def pos(self, level, s, j, q, k):
        return self.base[level - 1][s] + ((j * self.progs[self.mul[s]].nq[level - 1] + q) * self.D + k)

    def _lc(self, p, s, j, k, lc):
        """an affine form on sender p's values of item j of group s at point k; the constant is added as it is (the constant sharing)"""
        ii = self.mul[s]
        ins, prog = self.instrs[ii], self.progs[ii]
        i, X = self.items[s][j], (0 if k == 0 else k + 1)
        v = lc[0]
        for c, kind, idx in lc[1]:
            if kind == "m":
                v += c * _at(self.E[p][ins.mems[idx]], i, X)
            else:
                sl = prog.slots[idx]
                v += c * self.bufs[p][sl["level"] - 1][self.pos(sl["level"], s, j, sl["q"], k)]
        return v % R

    def _prods(self, p, s, j, k, prods):
        return sum(self._lc(p, s, j, k, x) * self._lc(p, s, j, k, y) for x, y in prods) % R

    def local_level(self, level):
        """z[p][pos]: every sender's unreduced slot values of the level, from its shares and its earlier level buffers"""
        z = [[0] * self.level_elems[level - 1] for _ in range(self.k)]
        for s, ii in enumerate(self.mul):
            for sl in self.progs[ii].slots:
                if sl["level"] != level:
                    continue
                for j in range(len(self.items[s])):
                    for k in range(self.D):
                        at = self.pos(level, s, j, sl["q"], k)
                        for p in range(self.k):
                            v = self._prods(p, s, j, k, sl["prods"])
                            if sl["add"] is not None:
                                v = (v + self._lc(p, s, j, k, sl["add"])) % R
                            z[p][at] = v
        return z

    def message(self):
        """msgs[p][k]: sender p's D evaluations (cozk_primary_round_finish): the linear pass + the last step of the multiplicative items"""
        msgs = []
        for p in range(self.k):
            ev = [0] * self.D
            for k in range(self.D):
                X = 0 if k == 0 else k + 1
                acc = 0
                for i in range(self.half):
                    inner = 0
                    for ii, ins in enumerate(self.instrs):
                        if ins.form not in LINEAR:
                            continue
                        f = _at(self.flags[ii], i, X)
                        if f:
                            inner += f * P.g_plain(ins, [_at(self.E[p][m], i, X) for m in ins.mems])
                    acc += _at(self.eq, i, X) * (inner - _at(self.outs[p], i, X))
                for s, ii in enumerate(self.mul):
                    prog = self.progs[ii]
                    for j, i in enumerate(self.items[s]):
                        g = (self._lc(p, s, j, k, prog.fin_add) + self._prods(p, s, j, k, prog.fin)) % R
                        acc += _at(self.eq, i, X) * _at(self.flags[ii], i, X) * g
                ev[k] = acc % R
            msgs.append(ev)
        return msgs


def exchange(z, keys, degree, counter):
    """the degree reduction of one level for the 2t + 1 senders: z[p] -> (what receiver q stores, the dealt values h[p][q])"""
    k = 2 * degree + 1
    assert len(z) == k
    h = [S.share_vec(z[p], keys[p], degree, k, counter=counter) for p in range(k)]
    lam = S.lagrange_from_coeff(list(range(1, k + 1)))
    n = len(z[0])
    return [[sum(lam[p] * h[p][q][i] for p in range(k)) % R for i in range(n)] for q in range(k)], h


def run_round(rnd, keys, degree, counter, reduce=True, record=None):
    """every level of a round -> (msgs[p][k], the counter after it, n_elems per level).  reduce = False: the levels run on UNREDUCED
    values (no exchange) -- what a prover without the degree reduction would compute.  record: a list that receives, per level,
    the senders' level buffers after the exchange"""
    elems = []
    for level in range(1, rnd.n_levels + 1):
        n_el = rnd.level_elems[level - 1]
        elems.append(n_el)
        if not n_el:
            for p in range(rnd.k):
                rnd.bufs[p][level - 1] = []
            if record is not None:
                record.append([[] for _ in range(rnd.k)])
            continue
        z = rnd.local_level(level)
        if reduce:
            out, _ = exchange(z, keys, degree, counter)
            counter += n_el
        else:
            out = z
        for p in range(rnd.k):
            rnd.bufs[p][level - 1] = out[p]
        if record is not None:
            record.append([list(o) for o in out])
    return rnd.message(), counter, elems


def bind_all(eq, flags, E, outs, r):
    return (O.public_bind(eq, r, L2H), [O.public_bind(f, r, L2H) for f in flags], [[O.dense_bind(m, r, L2H) for m in Ep] for Ep in E],
            [O.dense_bind(o, r, L2H) for o in outs])


# ------------------------------------------------------------------------------------------------ the prover
def lookups_instance(seed, log_n, n_mem, mix):
    """the lookups harness's own instance (oracle/pylookups.py run_primary): (instrs, flags, E clear, lookup_outputs clear)"""
    n = 1 << log_n
    instrs = LK.instr_table(n_mem)
    which = [LK.mix_instr(mix, v) for v in O.synthetic_small(seed + 1234567, n, 8)]
    flags = [[1 if which[x] == i else 0 for x in range(n)] for i in range(len(instrs))]
    Ep = [O.synthetic_fr(seed + 9000 * (m + 1), n) for m in range(n_mem)]
    out = [P.g_plain(instrs[which[x]], [Ep[m][x] for m in instrs[which[x]].mems]) for x in range(n)]
    return instrs, flags, Ep, out


def deal_columns(Ep, out, keys, degree, num_parties, share_counter):
    """E[p][m], outs[p]: column v at share_counter + v n, lookup_outputs = column n_mem"""
    n = len(out)
    cols = [S.share_vec(col, keys, degree, num_parties, counter=share_counter + v * n) for v, col in enumerate(list(Ep) + [out])]
    return [[cols[m][p] for m in range(len(Ep))] for p in range(num_parties)], [cols[len(Ep)][p] for p in range(num_parties)]


def prove_instance(instrs, r_eq_len, flags, Ep, out, num_parties, degree, skeys, mkeys, rkeys, share_counter=0, mul_counter=0, rand_counter=0,
                   label=b"cozk-lookups", first_senders=None, reduce=True, masked=True):
    """the whole prover on a clear instance.  first_senders: open the round messages from only that many senders (a test's probe: 2t
    do not reconstruct them); reduce = False: no exchange between the levels; masked = False: no zero masks"""
    t = degree
    k2, k1 = 2 * t + 1, t + 1
    assert 1 <= t and k2 <= num_parties
    lam2 = S.lagrange_from_coeff(list(range(1, (first_senders or k2) + 1)))
    lam1 = S.lagrange_from_coeff(list(range(1, k1 + 1)))
    E_all, outs_all = deal_columns(Ep, out, skeys, t, num_parties, share_counter)
    E, outs = E_all[:k2], outs_all[:k2]
    tr = O.Transcript(label)
    r_eq = tr.challenge_vector(r_eq_len)
    eq = O.eq_evals(r_eq)
    flags = [list(f) for f in flags]
    D = P.sumcheck_degree(instrs)
    zero = G.zero_masks(rkeys, t, D * r_eq_len, rand_counter=rand_counter) if masked else [[0] * (D * r_eq_len) for _ in range(k2)]
    ctr, claim = mul_counter, 0
    msgs, locs, comps, rs, polys, levels, elems_log, counters = [], [], [], [], [], [], [], []
    for rnd_no in range(r_eq_len):
        rnd = Round(instrs, eq, flags, E, outs)
        rec = []
        counters.append(ctr)
        loc, ctr, elems = run_round(rnd, mkeys, t, ctr, reduce=reduce, record=rec)
        levels.append(rec)
        elems_log.append(elems)
        opened = []
        for k in range(D):
            msg = [(loc[p][k] + zero[p][D * rnd_no + k]) % R for p in range(k2)]
            locs.append([loc[p][k] for p in range(k2)])
            msgs.append(msg)
            opened.append(S.reconstruct(msg[:len(lam2)], lam2))
        poly = P.from_evals_with_claim(opened, claim)
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_j = tr.challenge_scalar()
        rs.append(r_j)
        comps.append(comp)
        polys.append(poly)
        claim = O.unipoly_eval(poly, r_j)
        eq, flags, E, outs = bind_all(eq, flags, E, outs, r_j)
    finals = [[E[p][m][0] for p in range(k1)] for m in range(len(Ep))] + [[outs[p][0] for p in range(k1)]]
    opened = [S.reconstruct(f, lam1) for f in finals]
    openings = opened[:-1] + [f[0] for f in flags] + [opened[-1]]
    tr.append_scalars(openings)
    proof = {"round_polys": comps, "openings": openings}
    blob = serialize(proof)
    return {"proof_bytes": blob, "digest": hashlib.sha256(blob).hexdigest(), "proof": proof, "msgs": msgs, "locals": locs, "zero": zero,
            "finals": finals, "rs": rs, "r_eq": r_eq, "levels": levels, "elems": elems_log, "counters": counters, "mul_counter_end": ctr,
            "polys": polys, "degree": D}


def serialize(proof):
    """PrimarySumcheckProof::write"""
    return O.ser_u64(len(proof["round_polys"])) + b"".join(O.ser_vec_fr(c) for c in proof["round_polys"]) + O.ser_vec_fr(proof["openings"])


def prove(seed, log_n, n_mem, mix, num_parties, degree, share_counter=0, mul_counter=0, rand_counter=0, **kw):
    """cozk_shamir_primary_prove on the lookups harness's instance, with the harness-key conventions"""
    instrs, flags, Ep, out = lookups_instance(seed, log_n, n_mem, mix)
    return prove_instance(instrs, log_n, flags, Ep, out, num_parties, degree, share_keys(seed, degree), mul_keys(seed, num_parties, degree),
                          rand_keys(seed, num_parties, degree), share_counter, mul_counter, rand_counter, **kw)


def stats(ref, degree, grouped):
    """(group_rounds, single_rounds, group_finals, single_finals) as include/cozk.h states them"""
    log_n = len(ref["elems"])
    X = sum(1 for e in ref["elems"] for n_el in e if n_el)
    L = sum(len(e) for e in ref["elems"])
    return (X + log_n, 0, 0, 0) if grouped else (0, (2 * degree + 1) * (L + log_n), 0, 0)
