"""Plain-Python restatement of the output check on a shared v_final (co-zkvms_amd/memory_proof.py OutputCheck.shared,
cozk_output_check_shared_create in csrc/output_check.inc), per party, in two forms, shared by tests/test_output_check_shared_model.py
(CPU) and tests/test_gpu_output_check_shared.py:

  * `dense_rounds`: what a party of the dense composition sends.  Its difference polynomial is cozk_poly_linear_combination({v_final,
    v_io}, {1, -1}, mode, party) on the share COMPONENTS -- the public v_io goes into party 0's a and party 1's b -- and every round
    message is into_additive of the product sumcheck with that one shared factor: the sums over (a + b), times 2^-1.  The final values are
    eq(r), io_range(r) and (a + b) * 2^-1 of the bound difference.
  * `windowed_rounds`: the same numbers by the windowed algorithm of the device calls, on the ONE vector T = a + b (REP3) or a (PLAIN):
    d = T - sub * v_io inside the window with sub = 1 for PLAIN and REP3 parties 0 and 1 and 0 for party 2, output_check_ref.Windowed on d
    unchanged, and for REP3 the three round values and d's final value times 2^-1.
A role is "plain" or a REP3 party 0, 1, 2.  `share(values, rnd)` deals replicated shares: party i holds (x_i, x_{i-1}) of x_0 + x_1 + x_2."""
import output_check_ref as OC

R = OC.R
TWO_INV = (R + 1) // 2
ROLES = ("plain", 0, 1, 2)


def share(values, rnd):
    """-> [(a, b) component lists of party 0, 1, 2]: a_i = x_i, b_i = x_{i-1}"""
    x0 = [rnd.randrange(R) for _ in values]
    x1 = [rnd.randrange(R) for _ in values]
    x2 = [(v - s - t) % R for v, s, t in zip(values, x0, x1)]
    xs = [x0, x1, x2]
    return [(xs[i], xs[(i + 2) % 3]) for i in range(3)]


def components(role, v_final, shares):
    """the (a, b) of a role: b is None for "plain" """
    return (list(v_final), None) if role == "plain" else shares[role]


def dense_rounds(role, a, b, v_io, lo, r_eq, rs):
    """the dense composition of one party from its share components -> (rounds, (eq(r), io_range(r), additive share of d(r)))"""
    MEM, W = len(a), len(v_io)
    rng = [1 if lo <= x < lo + W else 0 for x in range(MEM)]
    da, db = list(a), None if b is None else list(b)
    for j, v in enumerate(v_io):  # the linear combination's public term: PLAIN's only component, party 0's a, party 1's b
        if role in ("plain", 0):
            da[lo + j] = (da[lo + j] - v) % R
        elif role == 1:
            db[lo + j] = (db[lo + j] - v) % R
    scale = 1 if b is None else TWO_INV
    eq, rounds = OC.O.eq_evals(r_eq), []
    for k in range(len(r_eq)):
        t = da if db is None else [(x + y) % R for x, y in zip(da, db)]  # the shared factor enters k_prod_round as (a + b)
        rounds.append([s * scale % R for s in OC._prod_evals([eq, rng, t])])
        eq, rng, da = OC._bind(eq, rs[k]), OC._bind(rng, rs[k]), OC._bind(da, rs[k])
        if db is not None:
            db = OC._bind(db, rs[k])
    fin = da[0] if db is None else (da[0] + db[0]) * TWO_INV % R
    return rounds, (eq[0], rng[0], fin)


def windowed_rounds(role, a, b, v_io, lo, r_eq, rs):
    """the device calls' algorithm for one party -> (rounds, final), as dense_rounds"""
    T = list(a) if b is None else [(x + y) % R for x, y in zip(a, b)]
    sub = 0 if role == 2 else 1
    scale = 1 if b is None else TWO_INV
    rounds, fin, _ = OC.windowed_rounds(T, [sub * v for v in v_io], lo, r_eq, rs)
    return [[s * scale % R for s in rd] for rd in rounds], (fin[0], fin[1], fin[2] * scale % R)
