"""Big-int restatement of the KING construct of the Lasso primary sumcheck proved by n Shamir parties (cozk_primary_plan,
cozk_primary_group_level_king, cozk_shamir_primary_prep, cozk_shamir_primary_prove_king; csrc/primary_group.inc,
csrc/host/shamir_primary.hpp), built on tests/shamir_primary_ref.py (programs, rounds, the prover), tests/shamir_dn_ref.py (rand: the
double-random pairs) and tests/shamir_gp_ref.py (zero_masks).  The reference has no Shamir prover, so this file IS the statement the
device code is held to.

  plan        which (index, instruction) items are live in a round depends on the public flags alone: instruction i is live at index j
              of round r iff one of the 2^(r + 1) cycles below j carries its flag (a bound flag is non-zero iff one of its pair was, up
              to a negligible probability): an OR pyramid over round 0's live pairs.  Item counts become level sizes through
              shamir_primary_ref.Round's formula: rows[r][level - 1] = n_elems, zero where a level holds nothing; total = their sum.
  prep        D = the table's sumcheck degree, M = D log_n.  (A) shamir_gp_ref.zero_masks of M elements at rand_counter: the resharing
              prover's masks.  (B) ONE shamir_dn_ref.rand of `total` elements at rand_counter + M, pair 0 only, both halves for
              parties 0..2t only.
  exchange e  (only those with n_elems > 0, in the order they happen) lives at the element offset off = the sum of the earlier
              exchanges' n_elems: masked_m[pos] = z_m[pos] + r2t_m[off + pos]; zed[pos] = sum_m lambda_m masked_m[pos], lambda =
              lagrange(1..2t + 1); receiver q stores zed[pos] - rt_q[off + pos]
  prove       shamir_primary_ref.prove_instance with that exchange in place of the re-deal: the same transcript, masks, openings,
              finals and proof"""
import pyprimary as P
import pyref as O
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_primary_ref as SP
import shamir_ref as S

R = O.R
MAX_LEVELS = SP.MAX_LEVELS


def plan(instrs, flags, log_n):
    """cozk_primary_plan: (rows[round][level - 1], total) from the instruction table and the 0/1 flag columns alone"""
    n = 1 << log_n
    assert all(len(f) == n for f in flags)
    deg = P.sumcheck_degree(instrs)
    mul = [ii for ii, ins in enumerate(instrs) if ins.form not in SP.LINEAR]
    progs = [SP.compile(instrs[ii]) for ii in mul]
    max_levels = max([pr.n_levels for pr in progs], default=0)
    live = [[1 if flags[ii][2 * j] or flags[ii][2 * j + 1] else 0 for j in range(n // 2)] for ii in mul]
    rows = []
    for r in range(log_n):
        if r:
            live = [[g[2 * j] | g[2 * j + 1] for j in range(len(g) // 2)] for g in live]
        counts = [sum(g) for g in live]
        rows.append([sum(c * pr.nq[t] * deg for c, pr in zip(counts, progs)) if sum(counts) and t < max_levels else 0 for t in range(MAX_LEVELS)])
    return rows, sum(sum(row) for row in rows)


def exchanges(rows):
    """[(round, level, offset, n_elems)] of the exchanges with n_elems > 0, in the order they happen"""
    out, off = [], 0
    for r, row in enumerate(rows):
        for lv, n_el in enumerate(row):
            if n_el:
                out.append((r, lv + 1, off, n_el))
                off += n_el
    return out


def prep(rand_keys, degree, instrs, flags, log_n, rand_counter=0):
    """cozk_shamir_primary_prep: dict M, plan, total, zero[p][m], rt[q], r2t[q] for the senders q <= 2t (pair 0 of the dealing)"""
    rows, total = plan(instrs, flags, log_n)
    M = P.sumcheck_degree(instrs) * log_n
    k = 2 * degree + 1
    pairs = D.rand(rand_keys, degree, total, counter=rand_counter + M) if total else [[([], [])] for _ in rand_keys]
    return dict(M=M, plan=rows, total=total, zero=G.zero_masks(rand_keys, degree, M, rand_counter), rt=[pairs[q][0][0] for q in range(k)],
                r2t=[pairs[q][0][1] for q in range(k)], used=False)


def level_king(z, r_t, r_2t, degree, offset=0):
    """cozk_primary_group_level_king on the senders' local slot values z[m]: (masked[m], zed, what receiver q stores)"""
    k = 2 * degree + 1
    n = len(z[0])
    assert len(z) == k and all(offset + n <= len(v) for v in list(r_t[:k]) + list(r_2t[:k]))
    lam = S.lagrange_from_coeff(list(range(1, k + 1)))
    masked = [[(z[m][i] + r_2t[m][offset + i]) % R for i in range(n)] for m in range(k)]
    zed = [sum(lam[m] * masked[m][i] for m in range(k)) % R for i in range(n)]
    return masked, zed, [[(zed[i] - r_t[q][offset + i]) % R for i in range(n)] for q in range(k)]


def prove_instance(instrs, log_n, flags, Ep, out, num_parties, degree, skeys, rkeys, pre, share_counter=0, rand_counter=0, king=0, record=None):
    """cozk_shamir_primary_prove_king on a clear instance, consuming `pre`.  record: a list that receives, per exchange, dict(off, z,
    masked, zed, out).  The king only relays: any party 0 <= king < n gives the same values"""
    assert 0 <= king < num_parties and not pre["used"]
    pre["used"] = True
    plan_left = exchanges(pre["plan"])

    def king_exchange(z, keys, deg, counter):
        # shamir_primary_ref.run_round advances `counter` by n_elems from mul_counter = 0: the element offset into the pair
        _, _, off, n_el = plan_left.pop(0)
        assert (off, n_el) == (counter, len(z[0])), "the exchange differs from the plan"
        masked, zed, outv = level_king(z, pre["rt"], pre["r2t"], deg, counter)
        if record is not None:
            record.append(dict(off=counter, z=z, masked=masked, zed=zed, out=outv))
        return outv, None

    plain_exchange = SP.exchange
    SP.exchange = king_exchange
    try:
        res = SP.prove_instance(instrs, log_n, flags, Ep, out, num_parties, degree, skeys, None, rkeys, share_counter=share_counter, mul_counter=0,
                                rand_counter=rand_counter)
    finally:
        SP.exchange = plain_exchange
    assert not plan_left and res["mul_counter_end"] == pre["total"] and res["zero"] == pre["zero"]
    return res


def prove(seed, log_n, n_mem, mix, num_parties, degree, share_counter=0, rand_counter=0, king=0, **kw):
    """prep + prove_king on the lookups harness's instance, with the harness-key conventions"""
    instrs, flags, Ep, out = SP.lookups_instance(seed, log_n, n_mem, mix)
    rkeys = SP.rand_keys(seed, num_parties, degree)
    pre = prep(rkeys, degree, instrs, flags, log_n, rand_counter)
    return prove_instance(instrs, log_n, flags, Ep, out, num_parties, degree, SP.share_keys(seed, degree), rkeys, pre, share_counter, rand_counter,
                          king=king, **kw)
