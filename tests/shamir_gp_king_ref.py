"""Big-int restatement of the Shamir grand product with the KING construct and offline preprocessing
(cozk_shamir_mul_mask_pairs, cozk_shamir_king_finish, cozk_shamir_mul_king_pairs_inproc, cozk_shamir_gp_prep_inproc,
cozk_shamir_gp_prove_king_inproc; csrc/host/shamir_gp.hpp), built from tests/shamir_dn_ref.py (rand, mul_mask, mul_king) and
tests/shamir_gp_ref.py.  The reference has no Shamir prover, so this file IS the statement the device code is held to.

  prep        before the leaves exist.  M = shamir_gp_ref.num_openings.  (A) shamir_gp_ref.zero_masks of M elements at rand_counter:
              the resharing prover's masks.  (B) ONE shamir_dn_ref.rand of n_leaves / 2 elements at rand_counter + M; pair 0 serves
              tree level 0 whole, pair 1 serves level i >= 1 at the element offset n_leaves / 2 - n_leaves / 2^i (the sum of the
              output lengths of levels 1..i - 1; the last level ends at n_leaves / 2 - 2 batch).  No pair for 2 leaves per circuit,
              one for 4, two otherwise.
  construct   layer[0] = the leaves; layer[i + 1] = the king multiplication (shamir_dn_ref.mul_king) of the interleaved halves
              L[j] = layer[i][2j], R[j] = layer[i][2j + 1] with that level's slice of its pair
  prove       shamir_gp_ref.prove's openings, rounds, finals, transcript and proof, restated over GIVEN layers and masks"""
import pyref as O
import shamir_dn_ref as D
import shamir_gp_ref as G
import shamir_ref as S

R = O.R


def levels(n_leaves, batch_size):
    """the multiplications of the tree: one per layer above the leaves"""
    return G.num_layers(n_leaves, batch_size) - 1


def pairs_needed(n_leaves, batch_size):
    return min(levels(n_leaves, batch_size), 2)


def level_slices(n_leaves, batch_size):
    """per tree level i: (pair, offset, products)"""
    half = n_leaves // 2
    return [(0, 0, half) if i == 0 else (1, half - (n_leaves >> i), n_leaves >> (i + 1)) for i in range(levels(n_leaves, batch_size))]


def prep(rand_keys, degree, n_leaves, batch_size, rand_counter=0):
    """dict: M, zero[p][m] for the senders, pairs[q][k] = (rt, r2t) of n_leaves / 2 elements for k < pairs_needed"""
    M = G.num_openings(n_leaves, batch_size)
    k = pairs_needed(n_leaves, batch_size)
    pairs = [q[:k] for q in D.rand(rand_keys, degree, n_leaves // 2, counter=rand_counter + M)] if k else [[] for _ in rand_keys]
    return dict(M=M, zero=G.zero_masks(rand_keys, degree, M, rand_counter), pairs=pairs)


def mul_mask_pairs(v_p, r2t_p, offset=0):
    """cozk_shamir_mul_mask_pairs for one sender: v_p[2j] v_p[2j + 1] + r2t_p[offset + j]"""
    assert len(v_p) % 2 == 0 and offset + len(v_p) // 2 <= len(r2t_p)
    return D.mul_mask(v_p[0::2], v_p[1::2], r2t_p[offset:offset + len(v_p) // 2])


def king_finish(masked, degree, r_t, offset=0):
    """cozk_shamir_king_finish: (z, [z - r_t[q][offset:]])"""
    k = D.senders(degree)
    z = S.combine_vec(masked[:k], list(range(1, k + 1)), 2 * degree)
    return z, [[(zi - ri) % R for zi, ri in zip(z, r[offset:offset + len(z)])] for r in r_t]


def mul_king_pairs(layer_shares, r_t, r_2t, degree, offset=0, king=0):
    """cozk_shamir_mul_king_pairs_inproc: layer_shares[p] and r_2t[p] are read for p <= 2t only"""
    k = D.senders(degree)
    m = len(layer_shares[0]) // 2
    cut = lambda v: None if v is None else v[offset:offset + m]
    half = lambda j: [layer_shares[p][j::2] if p < k else None for p in range(len(r_t))]
    return D.mul_king(half(0), half(1), [cut(v) for v in r_t], [cut(r_2t[p]) if p < k else None for p in range(len(r_t))], degree, king=king)


def construct(leaf_shares, batch_size, pre, degree, king=0):
    """layers[i][p]: party p's share vector of level i (every party; the senders' are what the prover reads)"""
    n_leaves = len(leaf_shares[0])
    layers = [[None if v is None else list(v) for v in leaf_shares]]
    for pair, off, m in level_slices(n_leaves, batch_size):
        rt = [q[pair][0] for q in pre["pairs"]]
        r2t = [q[pair][1] for q in pre["pairs"]]
        layers.append(mul_king_pairs(layers[-1], rt, r2t, degree, offset=off, king=king))
        assert len(layers[-1][0]) == m
    return layers


def prove_layers(layers, batch_size, zero, degree, label=b"cozk"):
    """shamir_gp_ref.prove behind its construction and its masks: the same openings, rounds, finals, transcript and proof"""
    k2, k1 = G.senders(degree), degree + 1
    lam2t = S.lagrange_from_coeff(list(range(1, k2 + 1)))
    lamt = S.lagrange_from_coeff(list(range(1, k1 + 1)))
    count = len(zero[0])
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


def prove(leaf_shares, batch_size, pre, degree, king=0, label=b"cozk"):
    """cozk_shamir_gp_prove_king_inproc: all parties and the coordinator, consuming the preprocessing `pre`"""
    return prove_layers(construct(leaf_shares, batch_size, pre, degree, king=king), batch_size, pre["zero"], degree, label=label)
