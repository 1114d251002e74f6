"""Big-int restatement of the TOGGLED batched grand product proved by n Shamir parties (cozk_shamir_tgp_prove_inproc,
cozk_shamir_tgp_prep_inproc, cozk_shamir_tgp_prove_king_inproc; csrc/host/shamir_gp.hpp), built on tests/shamir_gp_ref.py,
tests/shamir_gp_king_ref.py and oracle/pysparse.py's ToggleLayer with one party.  The reference has no Shamir prover, so this file
IS the statement the device code is held to.

The toggle layer's flags are public, so its output flag ? fingerprint : 1 and its round polynomial eq (flag fingerprint + 1 - flag)
are AFFINE in the fingerprint share.  A party that runs the plain toggle layer (pysparse.ToggleLayer(.., party 0, nparties = 1)) on
its degree-t share, with the PUBLIC claim as its previous claim, holds a degree-t sharing of the plain prover's values: the share of
a public constant is that constant for every party, which is what the one-party layer adds.

  construct   level 0 = every party's toggle output; above it shamir_gp_ref.construct or shamir_gp_king_ref.construct
  masks       batch B = 2 n_pairs, nv = ceil_log2(B), N = 2^d: the toggle layer has nv + d rounds, so
              M = shamir_gp_ref.num_openings(B N, B) + 4 (nv + d); ONE dealing at rand_counter, pair 0.  The king's pairs begin at
              rand_counter + M for this M
  rounds      the dense layers as shamir_gp_ref.prove runs them; then the toggle layer: no r_layer, no claim fold; each sender's
              four coefficients unipoly_from_evals(g0, claim - g0, g2, g3) are opened from senders 0..2t with the same zero masks
              (a degree-t sharing plus a degree-2t sharing of zero opens with lagrange(1..2t + 1))
  finals      the flag claim is public (sender 0's); the fingerprint claim is opened from parties 0..t, unmasked; the t + 1 pairs
              (flag, share) are appended to the dense layers' finals
  transcript  and proof: those of pysparse.toggled_prove"""
import pyref as O
import pysparse as SP
import shamir_dn_ref as D
import shamir_gp_king_ref as K
import shamir_gp_ref as G
import shamir_ref as S

R = O.R


def toggle_rounds(n_pairs, n):
    return (2 * n_pairs - 1).bit_length() + n.bit_length() - 1


def num_openings(n_pairs, n):
    return G.num_openings(2 * n_pairs * n, 2 * n_pairs) + 4 * toggle_rounds(n_pairs, n)


def instance(seed, n_pairs, n, density):
    """(flag_indices per pair, fingerprints per circuit): uniform elements with 0, 1, r - 1, r - 2 among the first"""
    rng = O.SplitMix64(seed)
    flags = [sorted(i for i in range(n) if rng.next() % 100 < density) for _ in range(n_pairs)]
    vals = [[rng.field() for _ in range(n)] for _ in range(2 * n_pairs)]
    for k, e in enumerate((0, 1, R - 1, R - 2)[:n]):
        vals[0][k] = e
    return flags, vals


def rows(flat, n):
    return [flat[b * n:(b + 1) * n] for b in range(len(flat) // n)]


def toggle_layer(flag_indices, fp_share, n):
    """one party's plain toggle layer over its flat share vector of the fingerprints (circuit-major)"""
    return SP.ToggleLayer(flag_indices, rows(fp_share, n), 0, 1)


def toggle_output(flag_indices, fp_share, n):
    """cozk_toggle_layer_output / cozk_toggle_group_layer_outputs for one party, dense: flag ? fingerprint : 1"""
    sp = toggle_layer(flag_indices, fp_share, n).layer_output()
    if sp.coalesced is not None:
        return list(sp.coalesced)
    out = [sp.one] * sp.dense_len
    for seg in sp.coeffs:
        for idx, val in seg:
            out[idx] = val
    return out


def prove_layers(layers, toggles, batch_size, zero, degree, label=b"cozk"):
    """openings, rounds, finals, transcript and proof over GIVEN dense layers (layers[i][p]), toggle layers (toggles[p], p <= 2t)
    and masks.  Returns shamir_gp_ref.prove's dict plus flag / fingerprint (the toggle layer's final claims) and toggle_locals[j][c][p],
    sender p's unmasked coefficient c of toggle round j"""
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
    # the toggle layer: no r_layer, no claim fold
    eqs = [O.SplitEq(r) for _ in range(k2)]
    r_sumcheck, round_polys, toggle_locals = [], [], []
    for _ in range(len(r)):
        co = [O.unipoly_from_evals(toggles[p].compute_cubic_evals(eqs[p], claim)) for p in range(k2)]
        toggle_locals.append([[co[p][c] % R for p in range(k2)] for c in range(4)])
        poly = [open_2t([co[p][c] for p in range(k2)]) for c in range(4)]
        comp = O.unipoly_compress(poly)
        tr.append_scalars(comp)
        r_j = tr.challenge_scalar()
        r_sumcheck.append(r_j)
        claim = O.unipoly_eval(poly, r_j)
        for p in range(k2):
            toggles[p].bind(r_j)
            eqs[p].bind(r_j)
        round_polys.append(comp)
    fc = [toggles[p].final_claims() for p in range(k1)]
    flag = fc[0][0] % R
    assert all(f[0] % R == flag for f in fc)  # public
    finals.append([(flag, f[1] % R) for f in fc])
    fingerprint = S.reconstruct([f[1] for f in finals[-1]], lamt)
    tr.append_scalar(flag)
    tr.append_scalar(fingerprint)
    r = list(reversed(r_sumcheck))
    proof["layers"].append({"round_polys": round_polys, "left": flag, "right": fingerprint})
    assert len(msgs) == count
    return dict(proof=proof, claim=claim, r=r, msgs=msgs, locals=local_vals, finals=finals, layers=layers, flag=flag, fingerprint=fingerprint,
                toggle_locals=toggle_locals)


def _level0(flag_indices, fp_shares, n):
    return [None if v is None else toggle_output(flag_indices, v, n) for v in fp_shares]


def _toggles(flag_indices, fp_shares, n, degree):
    return [toggle_layer(flag_indices, fp_shares[p], n) for p in range(G.senders(degree))]


def prove(flag_indices, fp_shares, n, mul_keys, rand_keys, degree, mul_counter=0, rand_counter=0, label=b"cozk"):
    """cozk_shamir_tgp_prove_inproc: fp_shares[p] = party p's flat share vector of the 2 n_pairs x n fingerprints"""
    batch = 2 * len(flag_indices)
    layers = G.construct(_level0(flag_indices, fp_shares, n), batch, mul_keys, degree, mul_counter)
    zero = G.zero_masks(rand_keys, degree, num_openings(len(flag_indices), n), rand_counter)
    return prove_layers(layers, _toggles(flag_indices, fp_shares, n, degree), batch, zero, degree, label=label)


def prep(rand_keys, degree, n_pairs, n, rand_counter=0):
    """cozk_shamir_tgp_prep_inproc: shamir_gp_king_ref.prep for the larger M; marked toggled"""
    batch, n_leaves = 2 * n_pairs, 2 * n_pairs * n
    M = num_openings(n_pairs, n)
    k = K.pairs_needed(n_leaves, batch)
    pairs = [q[:k] for q in D.rand(rand_keys, degree, n_leaves // 2, counter=rand_counter + M)] if k else [[] for _ in rand_keys]
    return dict(M=M, zero=G.zero_masks(rand_keys, degree, M, rand_counter), pairs=pairs, toggled=True)


def prove_king(flag_indices, fp_shares, n, pre, degree, king=0, label=b"cozk"):
    """cozk_shamir_tgp_prove_king_inproc, consuming the toggled preprocessing `pre`"""
    assert pre.get("toggled")
    batch = 2 * len(flag_indices)
    layers = K.construct(_level0(flag_indices, fp_shares, n), batch, pre, degree, king=king)
    return prove_layers(layers, _toggles(flag_indices, fp_shares, n, degree), batch, pre["zero"], degree, label=label)
