"""CPU tests of the protocol claim behind the KING construct of the Shamir primary prover (cozk_primary_plan,
cozk_primary_group_level_king, cozk_shamir_primary_prep, cozk_shamir_primary_prove_king; tests/shamir_primary_king_ref.py): the sizes
of all exchanges follow from the public flags, one preprocessed double-random pair of their sum serves them at running offsets, and
the proof is the plain prover's, byte for byte."""
import itertools

import pytest

import primary_ref as PR
import pyprimary as P
import pyref as O
import shamir_dn_ref as D
import shamir_primary_king_ref as KR
import shamir_primary_ref as SP
import shamir_ref as S

R = S.R
TABLE = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 3, first=1), P.Instr(P.CONCAT, [3, 0], 8)]
N_LEN, LOG_N = 8, 3
PARTIES = [(3, 1), (8, 2), (10, 4)]
SEED = 5
SHARE_COUNTER, RAND_COUNTER = 7, 11


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("mix", [0, 1], ids=["uniform", "sha2"])
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_plan_is_the_sequence_of_exchange_sizes_of_the_prover(log_n, mix):
    """the plan reads the flags alone; the big-int resharing prover reports, round by round, what it exchanged"""
    n_mem = 54
    instrs, flags, Ep, out = SP.lookups_instance(SEED, log_n, n_mem, mix)
    rows, total = KR.plan(instrs, flags, log_n)
    ref = SP.prove_instance(instrs, log_n, flags, Ep, out, 3, 1, SP.share_keys(SEED, 1), SP.mul_keys(SEED, 3, 1), SP.rand_keys(SEED, 3, 1), masked=False)
    assert len(rows) == log_n and all(len(row) == KR.MAX_LEVELS for row in rows)
    for row, elems in zip(rows, ref["elems"]):
        assert row == elems + [0] * (KR.MAX_LEVELS - len(elems))
    assert total == ref["mul_counter_end"] > 0
    ex = KR.exchanges(rows)
    assert [e[3] for e in ex] == [n_el for elems in ref["elems"] for n_el in elems if n_el]
    assert [e[2] for e in ex] == [sum(x[3] for x in ex[:i]) for i in range(len(ex))]  # running offsets


def test_plan_with_an_all_zero_flag_column_and_with_one_instruction():
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 4), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, 8, 41, zero_flags=(1,))
    rows, total = KR.plan(table, inst.flags, 3)
    out = SP.prove_instance(table, 3, inst.flags, inst.E, inst.outs, 3, 1, SP.share_keys(SEED, 1), SP.mul_keys(SEED, 3, 1), SP.rand_keys(SEED, 3, 1))
    assert [row[:3] for row in rows] == out["elems"] and all(row[0] > 0 and row[1:] == [0, 0, 0] for row in rows)
    one = [P.Instr(P.PRODUCT, [0, 1, 2])]
    flags = [[1, 0, 0, 0, 0, 0, 1, 1]]
    assert KR.plan(one, flags, 3) == ([[5 * 2, 0, 0, 0], [5 * 2, 0, 0, 0], [5, 0, 0, 0]], 25)  # D = 5: pairs {0, 3} -> {0, 1} -> {0}
    assert KR.plan([P.Instr(P.CONCAT, [0], 0)], [[1] * 8], 3) == ([[0] * 4] * 3, 0)


# ------------------------------------------------------------------------------------------------ the king prove
def _instance():
    inst = PR.Instance(TABLE, N_LEN, 700 + N_LEN)
    return inst.flags, inst.E, inst.outs


@pytest.fixture(scope="module")
def plain():
    """oracle/pyprimary.prove of the clear witness, and per round the plain prover's slot values (one 'sender' holding the clear
    columns, no exchange)"""
    flags, E, outs = _instance()
    tr = O.Transcript(b"cozk-lookups")
    r_eq = tr.challenge_vector(LOG_N)
    proof, rs, _ = P.prove(TABLE, r_eq, flags, [E], [outs], tr)
    eq, fl, Ec, oc = O.eq_evals(r_eq), [list(f) for f in flags], [E], [outs]
    levels = []
    for r_j in rs:
        rnd = SP.Round(TABLE, eq, fl, Ec, oc)
        rec = []
        SP.run_round(rnd, None, 0, 0, reduce=False, record=rec)
        levels.extend(lv[0] for lv in rec if lv[0])
        eq, fl, Ec, oc = SP.bind_all(eq, fl, Ec, oc, r_j)
    return dict(blob=SP.serialize(proof), rs=rs, slots=levels)


@pytest.fixture(scope="module")
def runs():
    out = {}
    flags, E, outs = _instance()
    for n, t in PARTIES:
        rkeys = SP.rand_keys(SEED, n, t)
        pre = KR.prep(rkeys, t, TABLE, flags, LOG_N, RAND_COUNTER)
        kept = dict(pre, used=False)
        rec = []
        res = KR.prove_instance(TABLE, LOG_N, flags, E, outs, n, t, SP.share_keys(SEED, t), rkeys, pre, SHARE_COUNTER, RAND_COUNTER, king=n - 1, record=rec)
        out[(n, t)] = dict(res=res, rec=rec, pre=kept, rkeys=rkeys)
    return out


@pytest.mark.parametrize("case", PARTIES, ids=lambda c: "p%d-t%d" % c)
def test_king_proof_is_the_plain_proof_and_the_resharing_provers(runs, plain, case):
    n, t = case
    res = runs[case]["res"]
    assert res["proof_bytes"] == plain["blob"] and res["rs"] == plain["rs"]
    flags, E, outs = _instance()
    other = SP.prove_instance(TABLE, LOG_N, flags, E, outs, n, t, SP.share_keys(SEED, t), SP.mul_keys(SEED, n, t), runs[case]["rkeys"],
                              share_counter=SHARE_COUNTER, mul_counter=13, rand_counter=RAND_COUNTER)
    assert other["proof_bytes"] == res["proof_bytes"]
    assert other["finals"] == res["finals"]  # evaluations of the dealt columns: the construct does not enter
    assert other["zero"] == res["zero"] and other["msgs"] != res["msgs"]
    lam = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    assert [S.reconstruct(m, lam) for m in other["msgs"]] == [S.reconstruct(m, lam) for m in res["msgs"]]
    assert other["elems"] == res["elems"] and res["mul_counter_end"] == runs[case]["pre"]["total"]


@pytest.mark.parametrize("case", PARTIES, ids=lambda c: "p%d-t%d" % c)
def test_every_exchange_leaves_degree_t_sharings_masked_by_the_pairs_secret(runs, plain, case):
    n, t = case
    k = 2 * t + 1
    run = runs[case]
    pre, rec = run["pre"], run["rec"]
    ex = KR.exchanges(pre["plan"])
    assert len(rec) == len(ex) == len(plain["slots"]) > 0
    secret = D.pair_value(run["rkeys"], 0, pre["total"], counter=RAND_COUNTER + pre["M"])  # what no t parties know
    lam2 = S.lagrange_from_coeff(list(range(1, k + 1)))
    combos = list(itertools.combinations(range(k), t + 1))
    for (_, _, off, n_el), step, want in zip(ex, rec, plain["slots"]):
        assert step["off"] == off and len(want) == n_el
        # the senders' local values are a degree-2t sharing of the plain slots, and so are the pair's second halves of its secret
        assert [S.reconstruct([step["z"][m][i] for m in range(k)], lam2) for i in range(n_el)] == want
        assert [S.reconstruct([pre["r2t"][m][off + i] for m in range(k)], lam2) for i in range(n_el)] == secret[off:off + n_el]
        # what the king opens is the slot masked by the secret: zed - slot = r
        assert [(z - w) % R for z, w in zip(step["zed"], want)] == secret[off:off + n_el]
        assert step["zed"] != want
        for members in combos[:: max(1, len(combos) // 12)] + combos[-1:]:  # ANY t + 1 receivers (a spread of them for t = 4)
            lam = S.lagrange_from_coeff([m + 1 for m in members])
            assert [S.reconstruct([step["out"][m][i] for m in members], lam) for i in range(n_el)] == want


def test_a_pair_element_used_for_two_positions_exposes_the_difference_of_the_slots(runs, plain):
    """why the prep is single-use and every exchange has an offset of its own: two exchanges masked with the SAME pair elements open
    zed_a = slot_a + r and zed_b = slot_b + r, and the king -- or anyone who sees both -- learns slot_a - slot_b"""
    n, t = 8, 2
    run = runs[(n, t)]
    pre, rec = run["pre"], run["rec"]
    a, b = rec[0], rec[1]
    m = min(len(a["z"][0]), len(b["z"][0]))
    cut = lambda z: [v[:m] for v in z]
    _, zed_a, _ = KR.level_king(cut(a["z"]), pre["rt"], pre["r2t"], t, offset=0)
    _, zed_b, _ = KR.level_king(cut(b["z"]), pre["rt"], pre["r2t"], t, offset=0)  # the mistake: offset 0 again
    diff = [(x - y) % R for x, y in zip(zed_a, zed_b)]
    assert diff == [(x - y) % R for x, y in zip(plain["slots"][0][:m], plain["slots"][1][:m])] and any(diff)
    _, zed_ok, _ = KR.level_king(cut(b["z"]), pre["rt"], pre["r2t"], t, offset=b["off"])  # at its own offset the difference is masked
    assert [(x - y) % R for x, y in zip(zed_a, zed_ok)] != diff
    with pytest.raises(AssertionError):  # and the restated prover refuses a used prep
        flags, E, outs = _instance()
        KR.prove_instance(TABLE, LOG_N, flags, E, outs, n, t, SP.share_keys(SEED, t), run["rkeys"], dict(pre, used=True))


def test_the_king_only_relays(runs):
    n, t = 3, 1
    flags, E, outs = _instance()
    base = runs[(n, t)]
    pre = dict(base["pre"], used=False)
    res = KR.prove_instance(TABLE, LOG_N, flags, E, outs, n, t, SP.share_keys(SEED, t), base["rkeys"], pre, SHARE_COUNTER, RAND_COUNTER, king=0)
    assert (res["proof_bytes"], res["msgs"], res["finals"], res["levels"]) == tuple(base["res"][x] for x in ("proof_bytes", "msgs", "finals", "levels"))
