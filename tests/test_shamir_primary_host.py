"""CPU tests of the protocol claim behind cozk_shamir_primary_* and cozk_primary_group_*: Lasso's primary sumcheck run by n Shamir
parties on their shares, with a degree reduction between the multiplication levels of the collation programs
(tests/shamir_primary_ref.py), gives the plain prover's proof, byte for byte (oracle/pyprimary.py) -- and WITHOUT that exchange it
does not, which is why the feature is needed."""
import itertools

import pytest

import primary_ref as PR
import pyprimary as P
import pyref as O
import shamir_primary_ref as SP
import shamir_ref as S

R = S.R
# PRODUCT C = 3 (one level), SLT C = 3 (two levels, a slot with an affine part), one CONCAT
TABLE = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 3, first=1), P.Instr(P.CONCAT, [3, 0], 8)]
PARTIES = [(3, 1), (4, 1), (5, 2), (6, 2)]
CASES = [(n_len, n, t) for n_len in (8, 16) for n, t in PARTIES]
SEED = 5
COUNTERS = dict(share_counter=7, mul_counter=13, rand_counter=11)


def _instance(n_len):
    inst = PR.Instance(TABLE, n_len, 700 + n_len)
    return inst.flags, inst.E, inst.outs


def _prove(n_len, n, t, **kw):
    flags, E, outs = _instance(n_len)
    args = dict(COUNTERS)
    args.update(kw)
    return SP.prove_instance(TABLE, n_len.bit_length() - 1, flags, E, outs, n, t, SP.share_keys(SEED, t), SP.mul_keys(SEED, n, t),
                             SP.rand_keys(SEED, n, t), **args)


@pytest.fixture(scope="module")
def runs():
    return {c: _prove(*c) for c in CASES}


@pytest.fixture(scope="module")
def plain():
    """oracle/pyprimary.prove of the clear witness under the prover's transcript, and per round the plain prover's message and slot
    values (one 'sender' holding the clear columns, no exchange)"""
    out = {}
    for n_len in (8, 16):
        flags, E, outs = _instance(n_len)
        tr = O.Transcript(b"cozk-lookups")
        r_eq = tr.challenge_vector(n_len.bit_length() - 1)
        proof, rs, _ = P.prove(TABLE, r_eq, flags, [E], [outs], tr)
        eq, fl, Ec, oc = O.eq_evals(r_eq), [list(f) for f in flags], [E], [outs]
        msgs, levels = [], []
        for r_j in rs:
            rnd = SP.Round(TABLE, eq, fl, Ec, oc)
            rec = []
            m, _, _ = SP.run_round(rnd, None, 0, 0, reduce=False, record=rec)
            assert m[0] == O.combine_additive(P.prover_message(TABLE, eq, fl, Ec, oc))  # the programs compute g
            msgs.append(m[0])
            levels.append([lv[0] for lv in rec])
            eq, fl, Ec, oc = SP.bind_all(eq, fl, Ec, oc, r_j)
        out[n_len] = dict(proof=proof, blob=SP.serialize(proof), rs=rs, msgs=msgs, levels=levels)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-t%d" % c)
def test_shamir_proof_is_the_plain_proof(runs, plain, case):
    out = runs[case]
    assert out["proof_bytes"] == plain[case[0]]["blob"]
    assert out["rs"] == plain[case[0]]["rs"]
    assert out["degree"] == P.sumcheck_degree(TABLE) == 7


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-t%d" % c)
def test_every_exchange_leaves_degree_t_sharings_of_the_plain_slots(runs, plain, case):
    n_len, n, t = case
    out = runs[case]
    k = 2 * t + 1
    seen = 0
    for rnd_no, per_level in enumerate(out["levels"]):
        assert len(per_level) == 2  # SLT C = 3
        for lv, bufs in enumerate(per_level):
            want = plain[n_len]["levels"][rnd_no][lv]
            assert len(bufs) == k and all(len(b) == len(want) == out["elems"][rnd_no][lv] for b in bufs)
            for members in itertools.combinations(range(k), t + 1):  # ANY t + 1 members: so all 2t + 1 lie on one degree-t polynomial
                lam = S.lagrange_from_coeff([m + 1 for m in members])
                assert [S.reconstruct([bufs[m][i] for m in members], lam) for i in range(len(want))] == want
            seen += len(want)
    assert seen > 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-t%d" % c)
def test_locals_are_degree_2t_sharings_and_the_masks_hide_them(runs, plain, case):
    """the round message of sender p is a sum of products of two degree-t values: the 2t + 1 of them open the plain message, t + 1 do
    not (it is no degree-t sharing), and what is sent differs from it by a sharing of zero: the unmasked message is a function of the
    dealt shares alone, not a fresh sharing"""
    n_len, n, t = case
    out = runs[case]
    D = out["degree"]
    lam2 = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    lam1 = S.lagrange_from_coeff(list(range(1, t + 2)))
    assert len(out["msgs"]) == len(out["locals"]) == D * (n_len.bit_length() - 1)
    for m, loc in enumerate(out["locals"]):
        want = plain[n_len]["msgs"][m // D][m % D]
        assert S.reconstruct(loc, lam2) == want
        assert S.reconstruct([out["zero"][p][m] for p in range(2 * t + 1)], lam2) == 0
        assert S.reconstruct(out["msgs"][m], lam2) == want and out["msgs"][m] != loc
        assert S.reconstruct(loc[:t + 1], lam1) != want
    assert len(out["finals"]) == 8 + 1 and all(len(f) == t + 1 for f in out["finals"])


@pytest.mark.parametrize("case", [(8, 3, 1), (16, 6, 2)], ids=lambda c: "n%d-p%d-t%d" % c)
def test_an_unmasked_message_is_a_function_of_the_dealt_shares(runs, case):
    """why the messages are masked: a sender's unmasked message is recomputed here from what was DEALT alone -- the witness shares,
    the public flags and eq and the exchanged level values -- with no fresh randomness.  So the 2t + 1 of them are not a degree-2t
    sharing of anything dealt for the opening: t of them are fixed by what the holders of the other t + 1 shares already know about
    the witness, instead of being uniform.  Other masks (another rand_counter) leave them as they are and change what is sent"""
    n_len, n, t = case
    out = runs[case]
    k, D = 2 * t + 1, out["degree"]
    flags, E, outs = _instance(n_len)
    Es, os_ = SP.deal_columns(E, outs, SP.share_keys(SEED, t), t, n, COUNTERS["share_counter"])
    tr = O.Transcript(b"cozk-lookups")
    eq, fl, Es, os_ = O.eq_evals(tr.challenge_vector(n_len.bit_length() - 1)), [list(f) for f in flags], Es[:k], os_[:k]
    for rnd_no, r_j in enumerate(out["rs"]):
        rnd = SP.Round(TABLE, eq, fl, Es, os_)
        for lv, bufs in enumerate(out["levels"][rnd_no]):  # what the exchange dealt to every sender
            for p in range(k):
                rnd.bufs[p][lv] = bufs[p]
        msg = rnd.message()
        assert [[msg[p][kk] for p in range(k)] for kk in range(D)] == out["locals"][D * rnd_no:D * (rnd_no + 1)]
        eq, fl, Es, os_ = SP.bind_all(eq, fl, Es, os_, r_j)
    other = _prove(n_len, n, t, rand_counter=COUNTERS["rand_counter"] + 10 ** 6)
    assert other["locals"] == out["locals"] and other["levels"] == out["levels"]
    assert all(a != b for a, b in zip(other["msgs"], out["msgs"])) and other["proof_bytes"] == out["proof_bytes"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-t%d" % c)
def test_without_the_exchange_the_senders_do_not_open_the_plain_message(plain, case):
    """THE REASON FOR THE FEATURE: levels run on unreduced values give slot values of degree 2t, the next level multiplies them again
    (3t, 4t), and the Lagrange combination of the 2t + 1 local messages is not the plain prover's message"""
    n_len, n, t = case
    bare = _prove(n_len, n, t, reduce=False)
    D = bare["degree"]
    lam2 = S.lagrange_from_coeff(list(range(1, 2 * t + 2)))
    first = [S.reconstruct(bare["locals"][k], lam2) for k in range(D)]
    assert first != plain[n_len]["msgs"][0]
    assert bare["proof_bytes"] != plain[n_len]["blob"]
    assert bare["mul_counter_end"] == COUNTERS["mul_counter"]  # nothing was dealt
    # the level-1 values themselves are still degree-2t sharings of the plain slots: it is the NEXT multiplication that breaks
    lv1 = bare["levels"][0][0]
    assert [S.reconstruct([lv1[p][i] for p in range(2 * t + 1)], lam2) for i in range(len(lv1[0]))] == plain[n_len]["levels"][0][0]


@pytest.mark.parametrize("case", [(8, 3, 1), (16, 5, 2)], ids=lambda c: "n%d-p%d-t%d" % c)
def test_2t_senders_do_not_open_the_messages(runs, plain, case):
    n_len, n, t = case
    out = runs[case]
    D = out["degree"]
    lam_short = S.lagrange_from_coeff(list(range(1, 2 * t + 1)))
    for m in (0, 1, D - 1, D, 2 * D + 1):
        for src in ("msgs", "locals"):
            assert S.reconstruct(out[src][m][:2 * t], lam_short) != plain[n_len]["msgs"][m // D][m % D]
    short = _prove(n_len, n, t, first_senders=2 * t)
    assert short["proof_bytes"] != out["proof_bytes"]


def test_counter_arithmetic(runs):
    """exchange e uses mul_counter + the sum of the earlier exchanges' n_elems; other counters change shares and masks, not the proof"""
    case = (16, 5, 2)
    base = runs[case]
    ctr = COUNTERS["mul_counter"]
    for rnd_no, elems in enumerate(base["elems"]):
        assert base["counters"][rnd_no] == ctr
        assert len(elems) == 2 and all(e > 0 for e in elems)
        ctr += sum(elems)
    assert base["mul_counter_end"] == ctr
    for kw, same_finals in ((dict(share_counter=1000), False), (dict(mul_counter=5000), True), (dict(rand_counter=2000), True)):
        other = _prove(*case, **kw)
        assert other["proof_bytes"] == base["proof_bytes"]
        assert other["msgs"] != base["msgs"]
        assert (other["finals"] == base["finals"]) == same_finals
    moved = _prove(*case, mul_counter=5000)
    assert moved["levels"] != base["levels"] and moved["zero"] == base["zero"]


def test_a_round_with_an_empty_level_does_not_advance_the_counter():
    """PRODUCT C = 3 (level 1 only) active beside SLT C = 4 (three levels) whose flags are all zero: three levels are announced,
    levels 2 and 3 hold nothing, and the counter advances by level 1 alone"""
    table = [P.Instr(P.PRODUCT, [0, 1, 2]), PR.form_instr(P.SLT, 4), P.Instr(P.CONCAT, [0], 0)]
    inst = PR.Instance(table, 8, 41, zero_flags=(1,))
    n, t = 3, 1
    out = SP.prove_instance(table, 3, inst.flags, inst.E, inst.outs, n, t, SP.share_keys(SEED, t), SP.mul_keys(SEED, n, t), SP.rand_keys(SEED, n, t),
                            mul_counter=100)
    tr = O.Transcript(b"cozk-lookups")
    proof, _, _ = P.prove(table, tr.challenge_vector(3), inst.flags, [inst.E], [inst.outs], tr)
    assert out["proof_bytes"] == SP.serialize(proof)
    ctr = 100
    for rnd_no, elems in enumerate(out["elems"]):
        assert len(elems) == 3 and elems[0] > 0 and elems[1:] == [0, 0]
        assert out["counters"][rnd_no] == ctr
        ctr += elems[0]
    assert out["mul_counter_end"] == ctr
    assert SP.stats(out, t, True) == (3 + 3, 0, 0, 0) and SP.stats(out, t, False) == (0, 3 * (9 + 3), 0, 0)


def test_programs_match_the_admitted_forms():
    """every admitted (form, C) pair: the program's level count is the exchange count of tests/primary_ref.py and its slots multiply
    exactly two affine forms"""
    for form, C in PR.PAIRS:
        ins = PR.form_instr(form, C)
        prog = SP.compile(ins)
        assert prog.n_levels == PR.levels(ins), (form, C)
        assert sum(prog.nq) == len(prog.slots)
        assert all(len(pr) == 2 for sl in prog.slots for pr in sl["prods"])
