"""Big-int restatement of the dense batched grand product proved by n Shamir parties (cozk_shamir_gp_prove_inproc,
csrc/host/shamir_gp.hpp; cozk_shamir_mul_deal_pairs / cozk_shamir_mul_pairs_inproc), on top of pyref's plain-prover pieces and
tests/shamir_ref.py, shamir_mul_ref.py, shamir_dn_ref.py.  The reference has no Shamir prover, so this file IS the statement the
device code is held to.

t = degree, n = parties, party p evaluates at p + 1; 1 <= t, 2t + 1 <= n.  eq is public, so every term of the sumcheck multiplies
at most two secret factors: a party that runs the plain prover's round function on its degree-t share vectors, with the PUBLIC
claim as its previous claim, holds a degree-2t share of the plain prover's round message.

  construct   layer[0] = the leaves; layer[i + 1] = the resharing multiplication (shamir_mul_ref.mul) of the interleaved halves
              L[j] = layer[i][2j], R[j] = layer[i][2j + 1], counter = mul_counter + the sum of the earlier levels' output lengths
  masks       M = batch + 4 sum_layers rounds(layer); ONE shamir_dn_ref.rand of M elements at rand_counter; pair 0 only:
              zero_p[m] = r2t_p^0[m] - rt_p^0[m], a degree-2t sharing of zero
  openings    of degree 2t, m = 0, 1, .. in the order opened -- the outputs, then layer by layer from the top, round by round,
              coefficients 0..3: sender p <= 2t sends local_p + zero_p[m]; the coordinator combines with lagrange(1..2t + 1)
  finals      L, R after the last bind, degree t: opened from parties 0..t with lagrange(1..t + 1), unmasked
  transcript  and proof: those of pyref.gp_prove"""
import pyref as O
import shamir_dn_ref as D
import shamir_mul_ref as M
import shamir_ref as S

R = O.R


def senders(degree):
    return 2 * degree + 1


def pair_products(v):
    """what a tree level multiplies: v[2j] v[2j + 1]"""
    return [x * y % R for x, y in zip(v[0::2], v[1::2])]


def mul_deal_pairs(v_p, keys_p, degree, num_parties, counter=0):
    """cozk_shamir_mul_deal_pairs for one dealer: h[q][j], the share of v_p[2j] v_p[2j + 1] for party q"""
    assert len(v_p) % 2 == 0
    return M.mul_deal(v_p[0::2], v_p[1::2], keys_p, degree, num_parties, counter=counter)


def mul_pairs(layer_shares, keys_per_party, degree, counter=0):
    """cozk_shamir_mul_pairs_inproc: layer_shares[p] is read for p <= 2t only"""
    halves = lambda k: [None if v is None else v[k::2] for v in layer_shares]
    return M.mul(halves(0), halves(1), keys_per_party, degree, counter=counter)


def num_layers(n_leaves, batch_size):
    per = n_leaves // batch_size
    assert n_leaves % batch_size == 0 and per >= 2 and per & (per - 1) == 0
    return per.bit_length() - 1


def rounds_per_layer(n_leaves, batch_size):
    """from the top: the top layer's point has ceil(log2(batch)) variables, every layer below one more"""
    nv = (batch_size - 1).bit_length()
    return [nv + k for k in range(num_layers(n_leaves, batch_size))]


def num_openings(n_leaves, batch_size):
    return batch_size + 4 * sum(rounds_per_layer(n_leaves, batch_size))


def construct(leaf_shares, batch_size, mul_keys, degree, mul_counter=0):
    """layers[i][p]: party p's share vector of level i"""
    layers = [[list(v) for v in leaf_shares]]
    ctr = mul_counter
    for _ in range(num_layers(len(leaf_shares[0]), batch_size) - 1):
        layers.append(mul_pairs(layers[-1], mul_keys, degree, counter=ctr))
        ctr += len(layers[-1][0])
    return layers


def zero_masks(rand_keys, degree, count, rand_counter=0):
    """zero[p][m] for the senders p <= 2t"""
    pairs = D.rand(rand_keys, degree, count, counter=rand_counter)
    return [[(pairs[p][0][1][m] - pairs[p][0][0][m]) % R for m in range(count)] for p in range(senders(degree))]


def ser_proof(proof):
    """GrandProductProof::write of a pyref.gp_prove proof dict"""
    out = O.ser_vec_fr(proof["outputs"]) + O.ser_u64(len(proof["layers"]))
    for lp in proof["layers"]:
        out += O.ser_u64(len(lp["round_polys"])) + b"".join(O.ser_vec_fr(c) for c in lp["round_polys"]) + O.ser_fr(lp["left"]) + O.ser_fr(lp["right"])
    return out


def prove(leaf_shares, batch_size, mul_keys, rand_keys, degree, mul_counter=0, rand_counter=0, label=b"cozk"):
    """all parties and the coordinator.  Returns a dict: proof (pyref.gp_prove's layout), claim, r, msgs[m][p] (masked, p <= 2t),
    locals[m][p] (the same before the mask), finals[layer, top first][p] = (L, R) for p <= t, layers (the construction)"""
    t, k2, k1 = degree, senders(degree), degree + 1
    lam2t = S.lagrange_from_coeff(list(range(1, k2 + 1)))
    lamt = S.lagrange_from_coeff(list(range(1, k1 + 1)))
    layers = construct(leaf_shares, batch_size, mul_keys, t, mul_counter)
    count = num_openings(len(leaf_shares[0]), batch_size)
    zero = zero_masks(rand_keys, t, count, rand_counter)
    msgs, local_vals = [], []

    def open_2t(local):
        m = len(msgs)
        local_vals.append([x % R for x in local])
        msgs.append([(local[p] + zero[p][m]) % R for p in range(k2)])
        return S.reconstruct(msgs[-1], lam2t)

    tr = O.Transcript(label)
    top = layers[-1]
    outputs = [open_2t([top[p][2 * i] * top[p][2 * i + 1] % R for p in range(k2)]) for i in range(batch_size)]
    tr.append_scalars(outputs)
    padded = list(outputs)
    while len(padded) & (len(padded) - 1):
        padded.append(0)
    r = tr.challenge_vector(len(padded).bit_length() - 1)
    claim = sum(e * v for e, v in zip(O.eq_evals(r), padded)) % R
    proof = {"outputs": outputs, "layers": []}
    finals = []
    for level in reversed(layers):
        work = [list(level[p]) for p in range(k2)]
        eqs = [O.SplitEq(r) for _ in range(k2)]
        r_sumcheck, round_polys = [], []
        for _ in range(len(r)):
            co = [O.interleaved_compute_cubic(work[p], eqs[p], claim) for p in range(k2)]  # every party's previous claim is public
            poly = [open_2t([co[p][c] for p in range(k2)]) for c in range(4)]
            comp = O.unipoly_compress(poly)
            tr.append_scalars(comp)
            r_j = tr.challenge_scalar()
            r_sumcheck.append(r_j)
            claim = O.unipoly_eval(poly, r_j)
            for p in range(k2):
                work[p] = O.interleaved_bind(work[p], r_j)
                eqs[p].bind(r_j)
            round_polys.append(comp)
        assert all(len(w) == 2 for w in work)
        finals.append([(work[p][0], work[p][1]) for p in range(k1)])
        left = S.reconstruct([f[0] for f in finals[-1]], lamt)
        right = S.reconstruct([f[1] for f in finals[-1]], lamt)
        tr.append_scalar(left)
        tr.append_scalar(right)
        r = list(reversed(r_sumcheck))
        r_layer = tr.challenge_scalar()
        claim = (left + r_layer * (right - left)) % R
        r.append(r_layer)
        proof["layers"].append({"round_polys": round_polys, "left": left, "right": right})
    assert len(msgs) == count
    return dict(proof=proof, claim=claim, r=r, msgs=msgs, locals=local_vals, finals=finals, layers=layers)


def leaves(seed, batch_size, per):
    """interleaved plain leaves: uniform elements, and 1 and r - 1 among them where there is room (no 0: it would zero a circuit)"""
    n = batch_size * per
    return (O.synthetic_fr(seed, n) + [1, R - 1])[-n:] if n > 4 else O.synthetic_fr(seed, n)
