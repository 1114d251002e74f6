"""Time the Shamir seam on the GPU and print (and optionally write) one JSON:
  (i)   the fused share: cozk_shamir_share_vec, one kernel for all parties;
  (ii)  the same sharing composed from the entry points that existed before it -- cozk_vec_fill_prf per coefficient, then
        per party and Horner step cozk_vec_scale + cozk_vec_binop -- alternating with (i) in this process, outputs compared once;
  (iii) the per-party element-wise product of two shared vectors;
  (iv)  cozk_shamir_combine_vec of the products from 2T + 1 parties (of one sharing from T + 1 where 2T + 1 > parties).
Device events around each repetition; enough repetitions of each leg to fill a second.  Fails without a device.
  python tools/run_shamir.py --log-n 24 --parties 8 --degree 2 [--out FILE]
With --mul, instead, the multiplication with degree reduction (needs 2 * degree + 1 <= parties):
  (v)   the fused re-deal cozk_shamir_mul_deal, one kernel (product folded into the dealing);
  (vi)  the same from the entry points that existed before it -- cozk_vec_binop(MUL), then cozk_shamir_share_vec -- alternating
        with (v) in this process, outputs compared once;
  (vii) the whole in-process multiplication cozk_shamir_mul_inproc, one context per party on this GPU: from a device event
        recorded while every stream is idle to the last of the events recorded behind each party's finish.
  python tools/run_shamir.py --mul --log-n 22 --parties 8 --degree 2 [--out FILE]
With --mul --king, instead, the multiplication with a king and double-random pairs (needs 2 * degree <= 15 too):
  (viii) the Vandermonde extraction cozk_shamir_rand_extract (parties inputs, parties - degree outputs) against the same from
         cozk_vec_scale + cozk_vec_binop, alternating in this process, outputs compared once;
  (ix)   the whole online step cozk_shamir_mul_king_inproc against the whole cozk_shamir_mul_inproc, one context per party on
         this GPU, alternating, each timed as (vii) is; both open to the product of the secrets;
  (x)    the whole offline step cozk_shamir_rand_inproc, timed the same way, and its cost per pair.
  python tools/run_shamir.py --mul --king --log-n 22 --parties 8 --degree 2 [--out FILE]
With --gp, instead, the Shamir grand product prover over 2^log_n interleaved leaves in --gp-batch circuits:
  (xi)   the fused re-deal of a tree level cozk_shamir_mul_deal_pairs on the leaf layer against cozk_layer_output_local (PLAIN,
         unmasked) + cozk_shamir_share_vec, alternating in this process, outputs compared raw;
  (xii)  the whole construct: cozk_shamir_mul_pairs_inproc level by level, one context per party on this GPU, timed as (vii) is;
  (xiii) the whole cozk_shamir_gp_prove_inproc (construct + masks + rounds), timed the same way, with the driver's own split, and as
         context the PLAIN single-party grand product of the same opened leaves in the same run (this script drives its rounds
         through cozk_layer_round and hashes the transcript itself: its proof must equal the Shamir parties' byte for byte).
  python tools/run_shamir.py --gp --log-n 22 --parties 8 --degree 2 [--out FILE]
With --gp --king, instead, the king construct of that prover and its offline preprocessing, the legs of a pair alternating:
  (xiv)   the mask of a tree level cozk_shamir_mul_mask_pairs on the leaf layer against cozk_layer_output_local (PLAIN, unmasked) +
          cozk_vec_binop(ADD), outputs compared raw;
  (xv)    the king's open and every party's unmask cozk_shamir_king_finish (2 * degree + 1 masked vectors, parties outputs) against
          cozk_shamir_combine_vec + parties x cozk_vec_binop(SUB), outputs compared raw;
  (xvi)   the whole king construct, cozk_shamir_mul_king_pairs_inproc level by level on preprocessed pairs, against the whole resharing
          construct of (xii), timed as (vii) is; both top layers open to the same values;
  (xvii)  the preprocessing cozk_shamir_gp_prep_inproc, reported on its own: offline time is never netted against online time;
  (xviii) the whole cozk_shamir_gp_prove_king_inproc (a fresh preprocessing per repetition, made outside the timed call) against the
          whole cozk_shamir_gp_prove_inproc; the proofs are equal byte for byte.
  python tools/run_shamir.py --gp --king --log-n 22 --parties 8 --degree 2 [--out FILE]
Both --gp and --gp --king end with a pair of legs of their prover:
  (xix)   the whole prove with the rounds on layer groups (cozk_layer_group_round: one launch per round for all senders) against the
          whole prove with COZK_SHAMIR_GP_GROUP=0 (the per-sender loop: one launch and one fetch per sender and round), alternating
          in this process, proofs, messages and final-claim shares compared.
--only-group runs nothing but (xix), for both provers:
  python tools/run_shamir.py --gp --only-group --log-n 22 --parties 8 --degree 2 --out profiles/shamir_gp_group_2p22_n8_t2.json
With --tgp, instead, the TOGGLED Shamir grand product over --pairs flag columns of 2^log_n entries (2 * pairs circuits), a share of
--density percent of the flags set; the resharing construct, or the king's with --king:
  (xx)    the first round of the toggle layer as ONE cozk_toggle_group_round over the senders' fingerprints against the senders'
          cozk_toggle_round calls, each with an eq of its own, alternating in this process, outputs compared raw;
  (xxi)   the whole prove with the toggle layer as one toggle group and the dense rounds on layer groups against the whole prove with
          COZK_SHAMIR_GP_GROUP=0, as (xix): alternating, proofs, messages, final-claim shares and toggle claims compared.
--only-group runs nothing but (xxi):
  python tools/run_shamir.py --tgp --only-group --log-n 18 --pairs 8 --density 10 --parties 8 --degree 2 --out profiles/shamir_tgp_group_2p18_p8_n8_t2.json
With --spartan, instead, co-noir-spartan of 2^log_n constraints proved by the Shamir parties (cozk_shamir_spartan_*):
  (xxii)  the first two rounds of the first sumcheck (the sums, then the bind with a challenge and the sums) as ONE cozk_spartan_group over
          the senders' (za, zb, zc) against the senders' cozk_spartan_first_round + 4 x cozk_poly_bind calls, each with an eq of its own,
          alternating in this process on fresh polynomials, outputs compared raw;
  (xxiii) the whole prove with both sumchecks as Spartan groups against the whole prove with COZK_SHAMIR_GP_GROUP=0 (the per-poly calls),
          alternating in this process, proofs, messages and final shares compared; the ungrouped leg is the yardstick.
--only-group runs nothing but (xxiii):
  python tools/run_shamir.py --spartan --only-group --log-n 18 --parties 8 --degree 2 --out FILE
With --jolt-spartan, instead, co-jolt's Spartan worker over 2^log_steps steps proved by the Shamir parties (cozk_shamir_jolt_spartan_*):
  (xxiv)  the first two rounds of the outer sumcheck (the sums, then the bind with a challenge and the sums) as ONE cozk_outer_group over
          the senders' cozk_outer states against the senders' cozk_outer_round calls, alternating in this process on fresh states over
          random columns, outputs compared raw;
  (xxv)   the whole prove with the outer and shift sumchecks as groups against the whole prove with COZK_SHAMIR_GP_GROUP=0 (the per-sender
          calls), alternating in this process, >= 30 repetitions each, proofs, messages and final shares compared; the ungrouped leg is
          the yardstick.
--only-group runs nothing but (xxv):
  python tools/run_shamir.py --jolt-spartan --only-group --system jolt --log-steps 18 --parties 8 --degree 2 --out FILE
With --primary, instead, Lasso's primary sumcheck of 2^log_n cycles proved by the Shamir parties (cozk_shamir_primary_*):
  (xxvi)  the first round's multiplication levels and its finish as ONE cozk_primary_group over the senders' PLAIN cozk_primary states
          (two launches per level, two per finish) against the per-sender composition (cozk_primary_level, the level buffer copied into a
          vector, cozk_shamir_scatter to the senders, cozk_shamir_combine_vec per receiver, the copy back, cozk_primary_round_finish),
          alternating in this process on fresh states over random share columns, level buffers and messages compared raw;
  (xxvii) the whole prove with the exchanges and finishes as level groups against the whole prove with COZK_SHAMIR_GP_GROUP=0 (the
          per-sender composition), alternating in this process, >= 10 repetitions each, proofs, messages and final shares compared; the
          ungrouped leg is the yardstick.  Also reported: the staging block's bytes, (2t + 1)^2 x the largest level's n_elems x 32.
--only-group runs nothing but (xxvii):
  python tools/run_shamir.py --primary --only-group --log-n 18 --mix uniform --parties 8 --degree 2 --out FILE
With --primary --king, instead, the KING level exchange of that prover on a preprocessed double-random pair (cozk_primary_plan,
cozk_primary_group_level_king, cozk_shamir_primary_prep, cozk_shamir_primary_prove_king):
  (xxviii) the first round's levels as cozk_primary_group_level_king calls on a keyless group against the composed king exchange
           (cozk_primary_level, the r_2t slice added with cozk_vec_binop, one cozk_shamir_king_finish at the offset, the copies back),
           outputs compared raw, and against the same levels as cozk_primary_group_level calls (the resharing group), alternating; the
           staging block's bytes of both forms;
  (xxix)   the whole king prove grouped against COZK_SHAMIR_GP_GROUP=0: proofs, messages and final shares compared;
  (xxx)    the grouped king prove against the grouped resharing prove -- the yardstick --, alternating in this process, a fresh handle
           and a fresh preprocessing per king repetition; online time and offline preprocessing time reported apart.
--only-group runs nothing but (xxix) and (xxx):
  python tools/run_shamir.py --primary --king --log-n 18 --mix uniform --parties 8 --degree 2 --out profiles/shamir_primary_king_2p18_n8_t2_uniform.json"""
import argparse, ctypes, hashlib, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=24)
ap.add_argument("--parties", type=int, default=8)
ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--min-seconds", type=float, default=1.0)
ap.add_argument("--mul", action="store_true", help="time the multiplication with degree reduction instead")
ap.add_argument("--king", action="store_true", help="with --mul: time the king / double-random variant against the resharing; with --gp / --tgp / --primary: the king construct")
ap.add_argument("--gp", action="store_true", help="time the Shamir grand product prover instead")
ap.add_argument("--gp-batch", type=int, default=2, help="with --gp: circuits in the grand product")
ap.add_argument("--only-group", action="store_true", help="with --gp: only the grouped against the ungrouped prove, resharing and king prover; with --tgp: only (xxi)")
ap.add_argument("--tgp", action="store_true", help="time the toggled Shamir grand product prover instead (--king: the king construct)")
ap.add_argument("--spartan", action="store_true", help="time co-noir-spartan proved by the Shamir parties instead (--only-group: only the whole prove)")
ap.add_argument("--jolt-spartan", action="store_true", help="time co-jolt's Spartan worker proved by the Shamir parties instead (--only-group: only the whole prove)")
ap.add_argument("--primary", action="store_true", help="time Lasso's primary sumcheck proved by the Shamir parties instead (--only-group: only the whole prove)")
ap.add_argument("--mix", default="uniform", choices=["uniform", "sha2"], help="with --primary: the instruction mix of the trace")
ap.add_argument("--mems", type=int, default=54, help="with --primary: E polynomials")
ap.add_argument("--system", default="jolt", choices=["toy", "jolt"], help="with --jolt-spartan: the constraint system")
ap.add_argument("--log-steps", type=int, default=18, help="with --jolt-spartan: log2 of the steps")
ap.add_argument("--seed", type=int, default=2030, help="with --spartan / --jolt-spartan: the instance's seed")
ap.add_argument("--pairs", type=int, default=8, help="with --tgp: flag columns (pairs of circuits)")
ap.add_argument("--density", type=int, default=10, help="with --tgp: percent of the flags that are set")
args = ap.parse_args()
if args.jolt_spartan:
    args.log_n = args.log_steps
cozk = importlib.import_module("co-zkvms_amd")
L = cozk._lib
if not torch.cuda.is_available():
    raise SystemExit("run_shamir: no GPU visible; there is no CPU path")
N, T, n = args.parties, args.degree, 1 << args.log_n
# leg (iv) opens the product from 2T + 1 parties; where the sharing has fewer ((10, 6)), it opens one sharing from T + 1
OPEN_PRODUCT = 2 * T + 1 <= N
K, OPEN_DEGREE = (2 * T + 1, 2 * T) if OPEN_PRODUCT else (T + 1, T)
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12  # spec / float4-copy figure of the MI355X microarchitecture notes

ctx = cozk.Context(0)
sp = ctypes.c_void_p()
ctx.check(ctx._l.cozk_ctx_stream(ctx.h, ctypes.byref(sp)))
stream = torch.cuda.ExternalStream(sp.value)


def key(i):
    return bytes((37 * i + 11 * j + 5) & 0xFF for j in range(32))


keys_a, keys_b = [key(c) for c in range(T)], [key(100 + c) for c in range(T)]
A, B = cozk.Vec.random(ctx, n, seed=2026), cozk.Vec.random(ctx, n, seed=2027)


def fused(V, keys):
    return V.shamir_share(keys, T, N, counter=0)


def composed(V, keys):
    """Horner per party from existing entry points: acc = c_T; acc = acc * x + c_k ...; acc = acc * x + v"""
    coefs = [cozk.Vec.prf(ctx, n, k, counter=0) for k in keys]
    lead = coefs[T - 1]  # scaled in place from c_T (p - 1) to c_T p, so that the first step too is one scale + one binop
    out = []
    for p in range(1, N + 1):
        x = cozk.fr_to_mont_limbs([p])[0]
        step = cozk.fr_to_mont_limbs([p * pow(p - 1, -1, cozk.FR_MOD) if p > 1 else 1])[0]
        ctx.check(ctx._l.cozk_vec_scale(ctx.h, lead.h, step.ctypes.data))
        lower = list(reversed(coefs[:T - 1])) + [V]
        acc = lead.binop(cozk.OP_ADD, lower[0])
        for lo in lower[1:]:
            ctx.check(ctx._l.cozk_vec_scale(ctx.h, acc.h, x.ctypes.data))
            nxt = acc.binop(cozk.OP_ADD, lo)
            acc.free()
            acc = nxt
        out.append(acc)
    for c in coefs:
        c.free()
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def free(vs):
    for v in vs if isinstance(vs, list) else [vs]:
        v.free()


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "repetitions": len(ts)}


med = lambda ts: sorted(ts)[len(ts) // 2]


def emit(res):
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


def mul_legs():
    if 2 * T + 1 > N:
        raise SystemExit("run_shamir --mul: 2 * degree + 1 parties re-deal the product; %d > %d" % (2 * T + 1, N))

    def fused_deal():
        return A.shamir_mul_deal(B, keys_a, T, N, counter=0)

    def composed_deal():
        prod = A.binop(cozk.OP_MUL, B)
        out = prod.shamir_share(keys_a, T, N, counter=0)
        prod.free()
        return out

    f, c = fused_deal(), composed_deal()  # correctness once, which is also the warm-up of both legs
    equal = all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(f, c))
    free(f), free(c)
    assert equal, "the fused re-deal and binop(MUL) + shamir_share differ"
    for _ in range(2):
        free(timed(fused_deal)[1]), free(timed(composed_deal)[1])
    t_f, t_c = [], []
    while sum(t_f) < args.min_seconds * 1e3 or sum(t_c) < args.min_seconds * 1e3 or len(t_f) < 5:  # alternating
        ms, r = timed(fused_deal); t_f.append(ms); free(r)
        ms, r = timed(composed_deal); t_c.append(ms); free(r)

    # (vii): one context per party on this GPU; a, b dealt onto them
    pcs = [cozk.Context(0) for _ in range(N)]
    streams = []
    for pc in pcs:
        h = ctypes.c_void_p()
        pc.check(pc._l.cozk_ctx_stream(pc.h, ctypes.byref(h)))
        streams.append(torch.cuda.ExternalStream(h.value))
    sa, sb = A.shamir_scatter(keys_a, T, pcs, counter=0), B.shamir_scatter(keys_b, T, pcs, counter=0)
    party_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]

    def whole():
        for pc in pcs:
            pc.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])  # every stream is idle: the call starts by draining them
        out = cozk.shamir_mul(pcs, sa, sb, party_keys, T, counter=n)
        ends = []
        for st in streams:
            e = torch.cuda.Event(enable_timing=True)
            e.record(st)
            ends.append(e)
        for e in ends:
            e.synchronize()
        return max(e0.elapsed_time(e) for e in ends), out

    ms, out = whole()  # warm-up and correctness: t + 1 parties from the high end open a x b
    for pc in pcs:
        pc.synchronize()
    pts = list(range(N, N - T - 1, -1))
    opened = cozk.shamir_combine([out[p - 1] for p in pts], pts, T)
    want = A.binop(cozk.OP_MUL, B)
    opens = bool(np.array_equal(opened.to_numpy(), want.to_numpy()))
    free([opened, want]), free(out)
    assert opens, "the in-process multiplication did not open the product of the secrets from degree + 1 parties"
    t_w = []
    while sum(t_w) < args.min_seconds * 1e3 or len(t_w) < 5:
        ms, out = whole(); t_w.append(ms); free(out)
    free(sa), free(sb)
    for pc in pcs:
        pc.close()

    D = 2 * T + 1
    fused_bytes, comp_bytes = (2 + N) * 32 * n, (3 + 1 + N) * 32 * n
    whole_bytes = D * (2 + N) * 32 * n + N * (D + 1) * 32 * n
    spread = lambda ts: round((sorted(ts)[-1] - sorted(ts)[0]) / med(ts), 4)
    emit({
        "what": "Shamir multiplication with degree reduction: fused re-deal vs binop(MUL) + shamir_share, whole in-process multiplication",
        "log_n": args.log_n, "parties": N, "degree": T, "dealers": D, "device": torch.cuda.get_device_name(0),
        "fused_mul_deal": dict(stats(t_f), algorithmic_bytes=fused_bytes, bytes_per_s=round(fused_bytes / (med(t_f) * 1e-3), 1),
                               spread_max_minus_min_over_median=spread(t_f), launches=1),
        "composed_mul_then_share": dict(stats(t_c), bytes_moved_by_the_composition=comp_bytes, spread_max_minus_min_over_median=spread(t_c), launches=2),
        "fused_vs_composed_speedup": round(med(t_c) / med(t_f), 3),
        "fused_not_slower_beyond_spread": bool(med(t_f) <= med(t_c) + max(sorted(t_f)[-1] - sorted(t_f)[0], sorted(t_c)[-1] - sorted(t_c)[0])),
        "outputs_equal": bool(equal),
        "inproc_mul": dict(stats(t_w), algorithmic_bytes=whole_bytes, bytes_per_s=round(whole_bytes / (med(t_w) * 1e-3), 1),
                           launches=D + N, contexts=N, opens_from_degree_plus_1=opens),
        "timing": "device events around each repetition (allocation from the contexts' pools included); legs (v) and (vi) alternating on one stream; "
                  "(vii) from an event on party 0's idle stream before the call to the last of the events behind the parties' finishes, host-side "
                  "stream synchronisations of the call included",
    })


def king_legs():
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --mul --king: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    CNT, D = N - T, 2 * T + 1
    spread = lambda ts: round((sorted(ts)[-1] - sorted(ts)[0]) / med(ts), 4)

    # (viii): extraction, one kernel against scale + binop
    recv = [cozk.Vec.random(ctx, n, seed=3000 + j) for j in range(N)]
    zero = cozk.Vec.from_numpy(ctx, np.zeros((n, 4), dtype=np.uint64))

    def fused_extract():
        return cozk.shamir_rand_extract(ctx, recv, CNT)

    def composed_extract():
        """w_j = s_j; per output: the sum of the w_j by binop(ADD), then w_j *= j + 1 by scale"""
        w = [v.binop(cozk.OP_ADD, zero) for v in recv]  # copies: scale works in place
        out = []
        for k in range(CNT):
            acc = w[0].binop(cozk.OP_ADD, w[1])
            for j in range(2, N):
                nxt = acc.binop(cozk.OP_ADD, w[j])
                acc.free()
                acc = nxt
            out.append(acc)
            if k + 1 < CNT:
                for j in range(1, N):
                    w[j].scale(j + 1)
        free(w)
        return out

    f, c = fused_extract(), composed_extract()
    equal = all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(f, c))
    free(f), free(c)
    assert equal, "the extraction kernel and scale + binop differ"
    for _ in range(2):
        free(timed(fused_extract)[1]), free(timed(composed_extract)[1])
    t_f, t_c = [], []
    while sum(t_f) < args.min_seconds * 1e3 or sum(t_c) < args.min_seconds * 1e3 or len(t_f) < 5:  # alternating
        ms, r = timed(fused_extract); t_f.append(ms); free(r)
        ms, r = timed(composed_extract); t_c.append(ms); free(r)
    free(recv), free(zero)

    # (ix), (x): one context per party on this GPU
    pcs = [cozk.Context(0) for _ in range(N)]
    streams = []
    for pc in pcs:
        h = ctypes.c_void_p()
        pc.check(pc._l.cozk_ctx_stream(pc.h, ctypes.byref(h)))
        streams.append(torch.cuda.ExternalStream(h.value))
    sa, sb = A.shamir_scatter(keys_a, T, pcs, counter=0), B.shamir_scatter(keys_b, T, pcs, counter=0)
    grr_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]
    dn_keys = [[key(2000 + 32 * p + c) for c in range(3 * T + 1)] for p in range(N)]

    def whole(fn):
        for pc in pcs:
            pc.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])  # every stream is idle: the call starts by draining them
        out = fn()
        ends = []
        for st in streams:
            e = torch.cuda.Event(enable_timing=True)
            e.record(st)
            ends.append(e)
        for e in ends:
            e.synchronize()
        return max(e0.elapsed_time(e) for e in ends), out

    flat = lambda pairs: [h for p in pairs for xy in p for h in xy]
    rand = lambda: cozk.shamir_rand(pcs, dn_keys, n, T, counter=0)
    ms, pairs = whole(rand)  # warm-up; these pairs feed the online leg
    r_t, r_2t = [p[0][0] for p in pairs], [p[0][1] for p in pairs]
    grr = lambda: cozk.shamir_mul(pcs, sa, sb, grr_keys, T, counter=n)
    king = lambda: cozk.shamir_mul_king(pcs, sa, sb, r_t, r_2t, T, king=0)  # the pair is reused across repetitions: timing only
    pts = list(range(N, N - T - 1, -1))
    want = A.binop(cozk.OP_MUL, B)
    opens = {}
    for name, fn in (("grr", grr), ("king", king)):  # warm-up and correctness: t + 1 parties from the high end open a x b
        ms, out = whole(fn)
        for pc in pcs:
            pc.synchronize()
        opened = cozk.shamir_combine([out[p - 1] for p in pts], pts, T)
        opens[name] = bool(np.array_equal(opened.to_numpy(), want.to_numpy()))
        free(opened), free(out)
        assert opens[name], "the in-process %s multiplication did not open the product of the secrets from degree + 1 parties" % name
    free(want)
    t_g, t_k = [], []
    while sum(t_g) < args.min_seconds * 1e3 or sum(t_k) < args.min_seconds * 1e3 or len(t_g) < 5:  # alternating
        ms, out = whole(grr); t_g.append(ms); free(out)
        ms, out = whole(king); t_k.append(ms); free(out)
    t_r = []
    while sum(t_r) < args.min_seconds * 1e3 or len(t_r) < 5:
        ms, out = whole(rand); t_r.append(ms); free(flat(out))
    free(flat(pairs)), free(sa), free(sb)
    for pc in pcs:
        pc.close()

    ext_bytes = (N + CNT) * 32 * n
    comp_bytes = (N * 96 + CNT * (N - 1) * 96 + (CNT - 1) * (N - 1) * 64) * n
    grr_bytes = D * (2 + N) * 32 * n + N * (D + 1) * 32 * n
    king_bytes = D * 128 * n + (D + 1) * 32 * n + N * 96 * n
    rand_bytes = (N * N * 32 + N * (N + CNT) * 32) * 2 * n
    emit({
        "what": "Shamir multiplication with a king and double-random pairs: extraction kernel vs scale + binop, whole online step vs the "
                "resharing multiplication, whole offline step",
        "log_n": args.log_n, "parties": N, "degree": T, "senders": D, "pairs_per_exchange": CNT, "device": torch.cuda.get_device_name(0),
        "extract": dict(stats(t_f), algorithmic_bytes=ext_bytes, bytes_per_s=round(ext_bytes / (med(t_f) * 1e-3), 1),
                        spread_max_minus_min_over_median=spread(t_f), launches=-(-CNT // 8), inputs=N, outputs=CNT),
        "composed_scale_and_add": dict(stats(t_c), bytes_moved_by_the_composition=comp_bytes, spread_max_minus_min_over_median=spread(t_c),
                                       launches=N + CNT * (N - 1) + (CNT - 1) * (N - 1)),
        "extract_vs_composed_speedup": round(med(t_c) / med(t_f), 3),
        "outputs_equal": bool(equal),
        "inproc_mul_king": dict(stats(t_k), algorithmic_bytes=king_bytes, bytes_per_s=round(king_bytes / (med(t_k) * 1e-3), 1),
                                launches=D + 1 + N, contexts=N, king=0, opens_from_degree_plus_1=opens["king"]),
        "inproc_mul_grr_same_run": dict(stats(t_g), algorithmic_bytes=grr_bytes, bytes_per_s=round(grr_bytes / (med(t_g) * 1e-3), 1),
                                        launches=D + N, contexts=N, opens_from_degree_plus_1=opens["grr"]),
        "king_vs_grr_time_ratio": round(med(t_k) / med(t_g), 3),
        "vectors_on_the_online_path": {"king": 2 * T + N - 1, "grr": D * (N - 1)},
        "inproc_rand": dict(stats(t_r), algorithmic_bytes=rand_bytes, bytes_per_s=round(rand_bytes / (med(t_r) * 1e-3), 1),
                            launches=2 * N + 2 * N * -(-CNT // 8), contexts=N, pairs=CNT, median_ms_per_pair=round(med(t_r) / CNT, 4)),
        "timing": "device events around each repetition (allocation from the contexts' pools included); the extraction legs alternating on one "
                  "stream; the in-process legs from an event on party 0's idle stream before the call to the last of the events behind the "
                  "parties' last kernels, host-side stream synchronisations of the call included, king and resharing alternating; the online "
                  "leg reuses one pair across repetitions (timing only: a pair must never be used twice)",
    })


def gp_legs():
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --gp: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    P = importlib.import_module("co-zkvms_amd.poly")
    batch, m = args.gp_batch, n // 2
    spread = lambda ts: round((sorted(ts)[-1] - sorted(ts)[0]) / med(ts), 4)

    # (xi): the leaf layer, 2^log_n elements -> 2^(log_n - 1) products
    layer = P.Rep3DenseInterleavedPolynomial.from_vecs(ctx, A)

    def fused_deal():
        return A.shamir_mul_deal_pairs(keys_a, T, N, counter=0)

    def composed_deal():
        prod = layer.layer_output_local()
        out = prod.shamir_share(keys_a, T, N, counter=0)
        prod.free()
        return out

    f, c = fused_deal(), composed_deal()  # correctness once, which is also the warm-up of both legs
    equal = all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(f, c))
    free(f), free(c)
    assert equal, "the fused re-deal of a layer and layer_output_local + shamir_share differ"
    for _ in range(2):
        free(timed(fused_deal)[1]), free(timed(composed_deal)[1])
    t_f, t_c = [], []
    while sum(t_f) < args.min_seconds * 1e3 or sum(t_c) < args.min_seconds * 1e3 or len(t_f) < 5:  # alternating
        ms, r = timed(fused_deal); t_f.append(ms); free(r)
        ms, r = timed(composed_deal); t_c.append(ms); free(r)
    layer.free()

    # (xii), (xiii): one context per party on this GPU
    pcs = [cozk.Context(0) for _ in range(N)]
    streams = []
    for pc in pcs:
        h = ctypes.c_void_p()
        pc.check(pc._l.cozk_ctx_stream(pc.h, ctypes.byref(h)))
        streams.append(torch.cuda.ExternalStream(h.value))
    leaves = A.shamir_scatter(keys_a, T, pcs, counter=0)
    mul_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]
    rand_keys = [[key(2000 + 32 * p + c) for c in range(3 * T + 1)] for p in range(N)]
    levels = (n // batch).bit_length() - 2  # multiplications: log2(leaves per circuit) - 1

    def whole(fn):
        for pc in pcs:
            pc.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])  # every stream is idle: the calls start by draining them
        out = fn()
        ends = []
        for st in streams:
            e = torch.cuda.Event(enable_timing=True)
            e.record(st)
            ends.append(e)
        for e in ends:
            e.synchronize()
        return max(e0.elapsed_time(e) for e in ends), out

    def construct():
        cur, ctr = leaves, 0
        for _ in range(levels):
            nxt = cozk.shamir_mul_pairs(pcs, cur, mul_keys, T, counter=ctr)
            ctr += len(nxt[0])
            if cur is not leaves:
                free(cur)
            cur = nxt
        return cur

    def prove():
        return cozk.shamir_gp_prove(pcs, leaves, batch, mul_keys, rand_keys, T, mul_counter=0, rand_counter=0)  # keys reused across repetitions: timing only

    # the PLAIN prover of the same leaves, driven from here: cozk_layer_output_local per level, cozk_layer_round per round
    R_MOD = cozk.FR_MOD
    ser = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)
    u64 = lambda v: int(v).to_bytes(8, "little")

    class Tr:  # the harness transcript: SHA-256 sponge, u32 round counter, 128-bit challenges
        def __init__(self):
            self.s, self.k = hashlib.sha256(b"cozk").digest(), 0

        def absorb(self, data):
            self.s = hashlib.sha256(self.s + self.k.to_bytes(4, "little") + data).digest()
            self.k += 1

        def challenge(self):
            self.absorb(b"challenge")
            return int.from_bytes(self.s[:16], "little")

    def plain_prove():
        ctx.synchronize()
        t0 = time.perf_counter()
        layers = [P.Rep3DenseInterleavedPolynomial.from_vecs(ctx, A)]
        for _ in range(levels):
            layers.append(P.Rep3DenseInterleavedPolynomial.from_vecs(ctx, layers[-1].layer_output_local(), take_ownership=True))
        ctx.synchronize()
        t1 = time.perf_counter()
        tr = Tr()
        outs = layers[-1].claimed_outputs()
        tr.absorb(ser(outs))
        r = [tr.challenge() for _ in range((batch - 1).bit_length())]
        eq = [1]
        for rj in r:
            eq = [x for e in eq for x in ((e - e * rj) % R_MOD, e * rj % R_MOD)]
        claim = sum(e * v for e, v in zip(eq, outs)) % R_MOD
        blob = u64(len(outs)) + ser(outs) + u64(len(layers))
        for layer in reversed(layers):
            eqp = P.SplitEqPolynomial(ctx, r)
            rs, rj = [], None
            blob += u64(len(r))
            for _ in range(len(r)):
                co = layer.round(eqp, rj, claim)
                comp = [co[0], co[2], co[3]]
                tr.absorb(ser(comp))
                rj = tr.challenge()
                rs.append(rj)
                claim = (co[0] + rj * (co[1] + rj * (co[2] + rj * co[3]))) % R_MOD
                blob += u64(3) + ser(comp)
            if rs:
                layer.bind(rj)
            left, right = layer.final_claims()
            tr.absorb(ser([left]))
            tr.absorb(ser([right]))
            rl = tr.challenge()
            claim = (left + rl * (right - left)) % R_MOD
            r = rs[::-1] + [rl]
            blob += ser([left, right])
            eqp.free()
            layer.free()
        ctx.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, blob

    ms, top = whole(construct)  # warm-up
    free(top)
    ms, g = whole(prove)        # warm-up and correctness
    assert g.result.verified == 1, "the Shamir grand product proof was rejected"
    pc_ms, pp_ms, plain_blob = plain_prove()
    same = plain_blob == g.proof_bytes
    assert same, "the Shamir parties' proof differs from the plain prover's proof of the same leaves"
    t_con, t_all, t_dc, t_dp, t_pc, t_pp = [], [], [], [], [], []
    while sum(t_con) < args.min_seconds * 1e3 or len(t_con) < 5:
        ms, top = whole(construct); t_con.append(ms); free(top)
    while sum(t_all) < args.min_seconds * 1e3 or len(t_all) < 5:  # the Shamir prover and the plain prover alternating
        ms, g = whole(prove); t_all.append(ms); t_dc.append(g.result.t_construct_ms); t_dp.append(g.result.t_prove_ms)
        a, b, _ = plain_prove(); t_pc.append(a); t_pp.append(b)
    grouped = group_pair(lambda: whole(prove))  # (xix)
    free(leaves)
    for pc in pcs:
        pc.close()

    D = 2 * T + 1
    fused_bytes, comp_bytes = (2 + N) * 32 * m, (2 + 1 + 1 + N) * 32 * m
    emit({
        "what": "Shamir grand product prover: fused re-deal of a layer vs layer_output_local + shamir_share, whole construct, whole prove, "
                "the PLAIN prover of the same leaves in the same run",
        "log_n": args.log_n, "interleaved_leaves": n, "batch": batch, "layers": levels + 1, "parties": N, "degree": T, "senders": D,
        "openings_of_degree_2t": int(g.result.n_opened), "proof_len": int(g.result.proof_len), "device": torch.cuda.get_device_name(0),
        "fused_mul_deal_pairs": dict(stats(t_f), products=m, algorithmic_bytes=fused_bytes, bytes_per_s=round(fused_bytes / (med(t_f) * 1e-3), 1),
                                     spread_max_minus_min_over_median=spread(t_f), launches=1),
        "composed_output_local_then_share": dict(stats(t_c), bytes_moved_by_the_composition=comp_bytes, spread_max_minus_min_over_median=spread(t_c), launches=2),
        "fused_vs_composed_speedup": round(med(t_c) / med(t_f), 3),
        "fused_slower_than_composed_by_ms": round(med(t_f) - med(t_c), 4),
        "composed_min_max_spread_ms": round(sorted(t_c)[-1] - sorted(t_c)[0], 4),
        "fused_not_slower_beyond_composed_spread": bool(med(t_f) - med(t_c) <= sorted(t_c)[-1] - sorted(t_c)[0]),
        "outputs_equal": bool(equal),
        "inproc_construct": dict(stats(t_con), levels=levels, launches=levels * (D + N), contexts=N),
        "inproc_prove_whole_call": dict(stats(t_all), contexts=N, verified=int(g.result.verified)),
        "inproc_prove_driver_split": {"construct": stats(t_dc), "masks_openings_rounds": stats(t_dp),
                                      "note": "the driver's host clock around stream-drained phases; one thread drives the parties in turn on "
                                              "one GPU, so the rounds are a SUM over the 2t + 1 senders, not what one party per GPU would take"},
        "plain_prover_same_run": {"construct": stats(t_pc), "prove": stats(t_pp), "proof_equals_shamir_proof": bool(same),
                                  "note": "host clock; rounds driven from this script through cozk_layer_round (one launch and one fetch per "
                                          "round, transcript hashed in Python): neither prover here uses the resident tail kernel"},
        "grouped_vs_ungrouped_rounds": grouped,
        "timing": "device events around each repetition for (xi), legs alternating on one stream; (xii) and the whole call of (xiii) from an event "
                  "on party 0's idle stream before the call to the last of the events behind the parties' streams, host-side synchronisations "
                  "included; the Shamir and the PLAIN prover alternating; keys and counters reused across repetitions (timing only)",
    })


def party_contexts():
    """one context per party on this GPU, and their streams"""
    pcs = [cozk.Context(0) for _ in range(N)]
    streams = []
    for pc in pcs:
        h = ctypes.c_void_p()
        pc.check(pc._l.cozk_ctx_stream(pc.h, ctypes.byref(h)))
        streams.append(torch.cuda.ExternalStream(h.value))
    return pcs, streams


def whole_call(pcs, streams, fn):
    """fn() from an event on party 0's idle stream to the last of the events behind the parties' streams"""
    for pc in pcs:
        pc.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record(streams[0])  # every stream is idle: the calls start by draining them
    out = fn()
    ends = []
    for st in streams:
        e = torch.cuda.Event(enable_timing=True)
        e.record(st)
        ends.append(e)
    for e in ends:
        e.synchronize()
    return max(e0.elapsed_time(e) for e in ends), out


GROUP_SWITCH = "COZK_SHAMIR_GP_GROUP"


def group_pair(timed_prove):
    """(xix): timed_prove() -> (ms, ShamirGpProof) with the rounds on layer groups and with COZK_SHAMIR_GP_GROUP=0, alternating.  The
    yardstick is the ungrouped leg of this run; the verdict allows the grouped median that leg's own min .. max spread"""
    def leg(ungrouped):
        if ungrouped:
            os.environ[GROUP_SWITCH] = "0"  # read by the library on every call
        try:
            return timed_prove()
        finally:
            os.environ.pop(GROUP_SWITCH, None)

    def calls(g):
        c = {k: int(getattr(g.stats, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}
        if g.toggle_claims is not None:  # a toggled proof: how the toggle layer's rounds ran
            c.update({k: int(getattr(g.toggle_stats, k)) for k in ("toggle_group_rounds", "toggle_single_rounds")})
        return c

    _, gg = leg(False)  # warm-up and correctness
    _, gu = leg(True)
    assert gg.result.verified == 1 and gu.result.verified == 1, "a Shamir grand product proof was rejected"
    equal = gg.proof_bytes == gu.proof_bytes and gg.msgs == gu.msgs and gg.finals == gu.finals and gg.toggle_claims == gu.toggle_claims
    if gg.toggle_claims is not None:
        assert gg.toggle_stats.toggle_single_rounds == 0 and gg.toggle_stats.toggle_group_rounds > 0 and gu.toggle_stats.toggle_group_rounds == 0, \
            "the switch did not select the toggle legs"
    assert equal, "the grouped and the ungrouped prove differ in proof, messages or final-claim shares"
    assert gg.stats.single_rounds == 0 and gg.stats.group_rounds > 0 and gu.stats.group_rounds == 0, "the switch did not select the legs"
    t_g, t_u, t_gc, t_gp, t_uc, t_up = [], [], [], [], [], []
    while sum(t_g) < args.min_seconds * 1e3 or sum(t_u) < args.min_seconds * 1e3 or len(t_g) < 6:
        ms, g = leg(False); t_g.append(ms); t_gc.append(g.result.t_construct_ms); t_gp.append(g.result.t_prove_ms)
        equal = equal and g.proof_bytes == gu.proof_bytes
        ms, g = leg(True); t_u.append(ms); t_uc.append(g.result.t_construct_ms); t_up.append(g.result.t_prove_ms)
        equal = equal and g.proof_bytes == gu.proof_bytes
    assert equal, "a repetition's proof differs"
    spread_u = sorted(t_u)[-1] - sorted(t_u)[0]
    return {
        "grouped_whole_call": dict(stats(t_g), driver_split={"construct": stats(t_gc), "openings_rounds": stats(t_gp)}, calls=calls(gg)),
        "ungrouped_whole_call_same_run": dict(stats(t_u), driver_split={"construct": stats(t_uc), "openings_rounds": stats(t_up)}, calls=calls(gu)),
        "grouped_vs_ungrouped_speedup": round(med(t_u) / med(t_g), 3),
        "openings_rounds_grouped_vs_ungrouped_speedup": round(med(t_up) / med(t_gp), 3),
        "grouped_slower_than_ungrouped_by_ms": round(med(t_g) - med(t_u), 4),
        "ungrouped_min_max_spread_ms": round(spread_u, 4),
        "grouped_not_slower_beyond_ungrouped_spread": bool(med(t_g) - med(t_u) <= spread_u),
        "proofs_messages_finals_equal": bool(equal),
    }


def group_legs_only():
    """--only-group: (xix) for the resharing prover and for the king prover, one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --gp --only-group: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    batch = args.gp_batch
    pcs, streams = party_contexts()
    whole = lambda fn: whole_call(pcs, streams, fn)
    leaves = A.shamir_scatter(keys_a, T, pcs, counter=0)
    mul_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]
    rand_keys = [[key(2000 + 32 * p + c) for c in range(3 * T + 1)] for p in range(N)]

    def king_prove():  # a fresh preprocessing per repetition, made outside the timed call
        prep = cozk.shamir_gp_prep(pcs, rand_keys, n, batch, T, rand_counter=0)
        try:
            return whole(lambda: cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=0))
        finally:
            prep.close()

    reshare = group_pair(lambda: whole(lambda: cozk.shamir_gp_prove(pcs, leaves, batch, mul_keys, rand_keys, T, mul_counter=0, rand_counter=0)))
    king = group_pair(king_prove)
    free(leaves)
    for pc in pcs:
        pc.close()
    emit({
        "what": "Shamir grand product provers: the rounds on layer groups (one launch per round for all senders) against the per-sender loop "
                "(COZK_SHAMIR_GP_GROUP=0), whole prove, resharing and king construct",
        "log_n": args.log_n, "interleaved_leaves": n, "batch": batch, "parties": N, "degree": T, "senders": 2 * T + 1, "king": 0,
        "device": torch.cuda.get_device_name(0),
        "resharing_prover": reshare, "king_prover": king,
        "timing": "from an event on party 0's idle stream before the call to the last of the events behind the parties' streams, host-side "
                  "synchronisations included; the grouped and the ungrouped leg alternating in one process, the ungrouped leg being the "
                  "yardstick; keys and counters reused across repetitions (timing only); the king prover's preprocessing is made outside "
                  "the timed call",
    })


def gp_king_legs():
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --gp --king: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    P = importlib.import_module("co-zkvms_amd.poly")
    batch, m, D = args.gp_batch, n // 2, 2 * T + 1
    levels = (n // batch).bit_length() - 2  # multiplications: log2(leaves per circuit) - 1
    if levels < 2:
        raise SystemExit("run_shamir --gp --king: needs at least 8 leaves per circuit (two tree levels)")
    spread = lambda ts: round(sorted(ts)[-1] - sorted(ts)[0], 4)
    raw_equal = lambda xs, ys: all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(xs, ys))

    def pair_of_legs(fused, composed, what):
        """both legs alternating on the context's stream; their outputs compared raw in the warm-up"""
        f, c = fused(), composed()
        equal = raw_equal(f, c)
        free(f), free(c)
        assert equal, what
        for _ in range(2):
            free(timed(fused)[1]), free(timed(composed)[1])
        t_f, t_c = [], []
        while sum(t_f) < args.min_seconds * 1e3 or sum(t_c) < args.min_seconds * 1e3 or len(t_f) < 5:
            ms, r = timed(fused); t_f.append(ms); free(r)
            ms, r = timed(composed); t_c.append(ms); free(r)
        return t_f, t_c, equal

    def verdict(t_f, t_c):
        return {"fused_vs_composed_speedup": round(med(t_c) / med(t_f), 3), "fused_slower_than_composed_by_ms": round(med(t_f) - med(t_c), 4),
                "composed_min_max_spread_ms": spread(t_c), "fused_not_slower_beyond_composed_spread": bool(med(t_f) - med(t_c) <= spread(t_c))}

    # (xiv): the leaf layer, 2^log_n elements -> 2^(log_n - 1) masked products
    layer = P.Rep3DenseInterleavedPolynomial.from_vecs(ctx, A)
    mask = cozk.Vec.random(ctx, m + 3, seed=2028)
    mask_cut = cozk.Vec.from_numpy(ctx, mask.to_numpy()[3:])

    def composed_mask():
        prod = layer.layer_output_local()
        out = prod.binop(cozk.OP_ADD, mask_cut)
        prod.free()
        return [out]

    t_mf, t_mc, mask_equal = pair_of_legs(lambda: [A.shamir_mul_mask_pairs(mask, 3)], composed_mask,
                                          "the mask of a layer and layer_output_local + binop(ADD) differ")
    layer.free(), free([mask, mask_cut])

    # (xv): 2t + 1 masked vectors of 2^(log_n - 1) elements -> parties outputs
    masked = [cozk.Vec.random(ctx, m, seed=3100 + j) for j in range(D)]
    rts = [cozk.Vec.random(ctx, m, seed=3200 + q) for q in range(N)]
    pts = list(range(1, D + 1))

    def composed_finish():
        z = cozk.shamir_combine(masked, pts, 2 * T)
        out = [z.binop(cozk.OP_SUB, r) for r in rts]
        z.free()
        return out

    t_ff, t_fc, finish_equal = pair_of_legs(lambda: cozk.shamir_king_finish(ctx, masked, T, rts), composed_finish,
                                            "the king finish and combine + binop(SUB) differ")
    free(masked), free(rts)

    # (xvi) .. (xviii): one context per party on this GPU
    pcs, streams = party_contexts()
    whole = lambda fn: whole_call(pcs, streams, fn)
    leaves = A.shamir_scatter(keys_a, T, pcs, counter=0)
    mul_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]
    rand_keys = [[key(2000 + 32 * p + c) for c in range(3 * T + 1)] for p in range(N)]
    pairs = cozk.shamir_rand(pcs, rand_keys, m, T, counter=1 << 40)  # reused across repetitions: timing only
    flat = lambda ps: [h for p in ps for xy in p for h in xy]

    def construct_grr():
        cur, ctr = leaves, 0
        for _ in range(levels):
            nxt = cozk.shamir_mul_pairs(pcs, cur, mul_keys, T, counter=ctr)
            ctr += len(nxt[0])
            if cur is not leaves:
                free(cur)
            cur = nxt
        return cur

    def construct_king():
        cur = leaves
        for i in range(levels):
            k, off = (1, m - (n >> i)) if i else (0, 0)
            nxt = cozk.shamir_mul_king_pairs(pcs, cur, [p[k][0] for p in pairs], [p[k][1] for p in pairs], T, r_offset=off, king=0)
            if cur is not leaves:
                free(cur)
            cur = nxt
        return cur

    high = list(range(N, N - T - 1, -1))
    tops = []
    for fn in (construct_grr, construct_king):  # warm-up and correctness: both top layers open to the same values
        ms, top = whole(fn)
        for pc in pcs:
            pc.synchronize()
        tops.append(cozk.shamir_combine([top[p - 1] for p in high], high, T))
        free(top)
    tops_equal = raw_equal(tops[:1], tops[1:])
    free(tops)
    assert tops_equal, "the king construct and the resharing construct open to different top layers"
    t_cg, t_ck = [], []
    while sum(t_cg) < args.min_seconds * 1e3 or sum(t_ck) < args.min_seconds * 1e3 or len(t_cg) < 5:  # alternating
        ms, top = whole(construct_grr); t_cg.append(ms); free(top)
        ms, top = whole(construct_king); t_ck.append(ms); free(top)
    free(flat(pairs))

    prove_grr = lambda: cozk.shamir_gp_prove(pcs, leaves, batch, mul_keys, rand_keys, T, mul_counter=0, rand_counter=0)  # keys reused: timing only
    make_prep = lambda: cozk.shamir_gp_prep(pcs, rand_keys, n, batch, T, rand_counter=0)
    t_prep, t_off, t_pg, t_pk, t_kc, t_kp, t_gc, t_gp = [], [], [], [], [], [], [], []
    proofs_equal, first = True, True
    while first or sum(t_pg) < args.min_seconds * 1e3 or sum(t_pk) < args.min_seconds * 1e3 or len(t_pg) < 6:
        ms_prep, prep = whole(make_prep)
        off_ms, held = prep.result.t_offline_ms, prep.result.pairs_held
        ms_k, gk = whole(lambda: cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=0))
        prep.close()
        ms_g, gg = whole(prove_grr)
        assert gk.result.verified == 1 and gg.result.verified == 1, "a Shamir grand product proof was rejected"
        proofs_equal = proofs_equal and gk.proof_bytes == gg.proof_bytes
        assert proofs_equal, "the king prover's proof differs from the resharing prover's"
        if first:  # warm-up
            first = False
            continue
        t_prep.append(ms_prep); t_off.append(off_ms); t_pk.append(ms_k); t_pg.append(ms_g)
        t_kc.append(gk.result.t_construct_ms); t_kp.append(gk.result.t_prove_ms); t_gc.append(gg.result.t_construct_ms); t_gp.append(gg.result.t_prove_ms)

    def king_prove():  # (xix): a fresh preprocessing per repetition, made outside the timed call
        prep = make_prep()
        try:
            return whole(lambda: cozk.shamir_gp_prove_king(pcs, leaves, batch, prep, king=0))
        finally:
            prep.close()

    grouped = group_pair(king_prove)
    free(leaves)
    for pc in pcs:
        pc.close()

    M = int(gk.result.n_opened)
    emit({
        "what": "Shamir grand product, king construct: mask kernel vs layer_output_local + binop(ADD), finish kernel vs combine + subtractions, whole "
                "king construct vs whole resharing construct, the preprocessing on its own, whole prove both ways",
        "log_n": args.log_n, "interleaved_leaves": n, "batch": batch, "layers": levels + 1, "parties": N, "degree": T, "senders": D, "king": 0,
        "openings_of_degree_2t": M, "proof_len": int(gk.result.proof_len), "device": torch.cuda.get_device_name(0),
        "mask_pairs": dict(stats(t_mf), products=m, algorithmic_bytes=128 * m, bytes_per_s=round(128 * m / (med(t_mf) * 1e-3), 1), launches=1),
        "composed_output_local_then_add": dict(stats(t_mc), bytes_moved_by_the_composition=(96 + 96) * m, launches=2),
        "mask_verdict": verdict(t_mf, t_mc), "mask_outputs_equal": bool(mask_equal),
        "king_finish": dict(stats(t_ff), elements=m, algorithmic_bytes=(D + 2 * N) * 32 * m, bytes_per_s=round((D + 2 * N) * 32 * m / (med(t_ff) * 1e-3), 1), launches=1),
        "composed_combine_then_subtract": dict(stats(t_fc), bytes_moved_by_the_composition=((D + 1) * 32 + N * 96) * m, launches=1 + N),
        "finish_verdict": verdict(t_ff, t_fc), "finish_outputs_equal": bool(finish_equal),
        "inproc_construct_king": dict(stats(t_ck), levels=levels, launches=levels * (D + 1), contexts=N),
        "inproc_construct_resharing_same_run": dict(stats(t_cg), levels=levels, launches=levels * (D + N), contexts=N),
        "king_vs_resharing_construct_time_ratio": round(med(t_ck) / med(t_cg), 3),
        "king_construct_not_slower_than_resharing": bool(med(t_ck) <= med(t_cg)),
        "constructs_open_to_equal_top_layers": bool(tops_equal),
        "offline_prep": dict(stats(t_prep), driver_host_clock=stats(t_off), mask_elements=M, pair_elements=m, pairs_extracted=int(held), contexts=N,
                             note="reported on its own: never netted against an online figure"),
        "inproc_prove_king_whole_call": dict(stats(t_pk), driver_split={"construct": stats(t_kc), "openings_rounds": stats(t_kp)}),
        "inproc_prove_resharing_whole_call_same_run": dict(stats(t_pg), driver_split={"construct": stats(t_gc), "masks_openings_rounds": stats(t_gp)}),
        "king_vs_resharing_prove_time_ratio": round(med(t_pk) / med(t_pg), 3),
        "proofs_equal": bool(proofs_equal),
        "grouped_vs_ungrouped_rounds": grouped,
        "timing": "device events around each repetition for (xiv) and (xv), legs alternating on one stream (allocation from the context's pool "
                  "included); the in-process legs from an event on party 0's idle stream before the call to the last of the events behind the "
                  "parties' streams, host-side synchronisations included, the legs of a pair alternating; the construct legs reuse two "
                  "preprocessed pairs and the provers their keys and counters across repetitions (timing only: a pair must never be used twice); "
                  "peer-copy legs (parties on other GPUs) are not exercised by a one-GPU run",
    })


def tgp_legs():
    """--tgp: (xx) unless --only-group, then (xxi); one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --tgp: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    lookups = importlib.import_module("co-zkvms_amd.lookups")
    pairs, senders = args.pairs, 2 * T + 1
    total = 2 * pairs * n
    pcs, streams = party_contexts()
    whole = lambda fn: whole_call(pcs, streams, fn)
    rng = np.random.default_rng(2028)
    flags = [cozk.Vec.from_ints(pcs[0], (rng.integers(0, 100, n) < args.density).astype(np.uint8).tolist(), kind=L.SCALAR_U8) for _ in range(pairs)]
    fps = cozk.Vec.random(ctx, total, seed=2029).shamir_scatter(keys_a, T, pcs, counter=0)
    mul_keys = [[key(1000 + 16 * p + c) for c in range(T)] for p in range(N)]
    rand_keys = [[key(2000 + 32 * p + c) for c in range(3 * T + 1)] for p in range(N)]
    res = {
        "what": "toggled Shamir grand product: the toggle layer as one toggle group (one launch set and one fetch per round for all senders, one "
                "pass over the public flags and eq tables) against a PLAIN toggle layer per sender (COZK_SHAMIR_GP_GROUP=0), "
                + ("king construct" if args.king else "resharing construct"),
        "log_n": args.log_n, "pairs": pairs, "circuits": 2 * pairs, "fingerprints": total, "density_pct": args.density, "parties": N, "degree": T,
        "senders": senders, "device": torch.cuda.get_device_name(0),
    }
    if not args.only_group:
        nv = (2 * pairs - 1).bit_length() + args.log_n
        w = [pow(3, 5 + i, cozk.FR_MOD) for i in range(nv)]
        group = lookups.ToggleGroup(pcs[0], flags, fps[:senders])
        singles = [lookups.ToggleLayer.from_vecs(pcs[p], flags, fps[p]) for p in range(senders)]
        eq_g = cozk.SplitEqPolynomial(pcs[0], w)
        eq_s = [cozk.SplitEqPolynomial(pcs[p], w) for p in range(senders)]
        run_g = lambda: whole(lambda: group.round(eq_g))
        run_s = lambda: whole(lambda: [singles[p].round(eq_s[p]) for p in range(senders)])
        assert run_g()[1] == run_s()[1], "the group round and the per-sender rounds differ"
        t_g, t_s = [], []
        while sum(t_g) < args.min_seconds * 1e3 or sum(t_s) < args.min_seconds * 1e3 or len(t_g) < 6:
            t_g.append(run_g()[0])
            t_s.append(run_s()[0])
        res["first_round"] = {"group_round": stats(t_g), "per_sender_rounds_same_run": stats(t_s), "group_vs_per_sender_speedup": round(med(t_s) / med(t_g), 3),
                              "outputs_equal": True}
        group.free()
        for t in singles:
            t.free()

    def king_prove():  # a fresh preprocessing per repetition, made outside the timed call
        prep = cozk.shamir_tgp_prep(pcs, rand_keys, pairs, n, T, rand_counter=0)
        try:
            return whole(lambda: cozk.shamir_tgp_prove_king(pcs, flags, fps, prep, king=0))
        finally:
            prep.close()

    prove = king_prove if args.king else (lambda: whole(lambda: cozk.shamir_tgp_prove(pcs, flags, fps, mul_keys, rand_keys, T, mul_counter=0, rand_counter=0)))
    res["king_prover" if args.king else "resharing_prover"] = group_pair(prove)
    res["timing"] = ("from an event on party 0's idle stream before the call to the last of the events behind the parties' streams, host-side "
                     "synchronisations included; the grouped and the ungrouped leg alternating in one process, the ungrouped leg being the yardstick; "
                     "keys and counters reused across repetitions (timing only); the king prover's preprocessing is made outside the timed call")
    free(fps), free(flags)
    for pc in pcs:
        pc.close()
    emit(res)


def spartan_legs():
    """--spartan: (xxii) unless --only-group, then (xxiii); the harness owns one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --spartan: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    P = importlib.import_module("co-zkvms_amd.poly")
    senders = 2 * T + 1
    res = {
        "what": "co-noir-spartan by Shamir parties: both sumchecks as Spartan groups (one fused bind + sums launch, one finishing launch and one "
                "fetch per round for all senders, one public polynomial) against the per-poly calls per sender (COZK_SHAMIR_GP_GROUP=0)",
        "log_n": args.log_n, "constraints": n, "parties": N, "degree": T, "senders": senders, "openers": T + 1, "seed": args.seed,
        "device": torch.cuda.get_device_name(0),
    }
    if not args.only_group:
        pcs, streams = party_contexts()
        whole = lambda fn: whole_call(pcs, streams, fn)
        base = [[cozk.Vec.random(pcs[p], n, seed=3000 + 10 * p + j) for j in range(3)] for p in range(senders)]
        eq_base = [cozk.Vec.random(pcs[p], n, seed=2999) for p in range(senders)]
        r = cozk.fr_to_mont_limbs([pow(3, 77, cozk.FR_MOD)])[0]
        mk = lambda: [tuple(P.Rep3DensePolynomial.from_vec_shares(pcs[p], v) for v in base[p]) for p in range(senders)]

        def run_g():
            members, eq = mk(), P.Rep3DensePolynomial.from_vec_shares(pcs[0], eq_base[0])
            g = cozk.SpartanGroup(pcs[0], 1, members, eq)
            ms, out = whole(lambda: [g.round_raw(None), g.round_raw(r)])
            g.free()
            return ms, out

        def run_s():
            members, eqs = mk(), [P.Rep3DensePolynomial.from_vec_shares(pcs[p], eq_base[p]) for p in range(senders)]

            def rounds():
                outs = [np.zeros((senders, 4, 4), dtype=np.uint64) for _ in range(2)]
                for j in range(2):
                    for p in range(senders):
                        c = pcs[p]
                        if j:
                            for q in members[p] + (eqs[p],):
                                c.check(c._l.cozk_poly_bind(c.h, q.h, r.ctypes.data, L.LOW_TO_HIGH))
                        za, zb, zc = members[p]
                        c.check(c._l.cozk_spartan_first_round(c.h, za.h, zb.h, zc.h, eqs[p].h, outs[j][p].ctypes.data))
                return outs
            return whole(rounds)

        og, os_ = run_g()[1], run_s()[1]
        assert all(np.array_equal(x, y) for x, y in zip(og, os_)), "the group rounds and the per-sender rounds differ"
        t_g, t_s = [], []
        while sum(t_g) < args.min_seconds * 1e3 or sum(t_s) < args.min_seconds * 1e3 or len(t_g) < 6:
            t_g.append(run_g()[0])
            t_s.append(run_s()[0])
        res["first_two_rounds"] = {"group_rounds": stats(t_g), "per_sender_rounds_same_run": stats(t_s),
                                   "group_vs_per_sender_speedup": round(med(t_s) / med(t_g), 3), "outputs_equal": True}
        for vs in base:
            free(vs)
        free(eq_base)
        for pc in pcs:
            pc.close()

    h = cozk.ShamirSpartanHarness(log_n=args.log_n, parties=N, degree=T, devices=0, seed=args.seed)
    split = ("t_zero_round_ms", "t_commit_ms", "t_masks_ms", "t_sumcheck1_ms", "t_matrix_build_ms", "t_sumcheck2_ms", "t_open_ms")

    def leg(ungrouped):
        if ungrouped:
            os.environ[GROUP_SWITCH] = "0"  # read by the library on every prove
        try:
            r_ = h.prove(verify=False)
            st = h.stats()
            return r_, {k: int(getattr(st, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}
        finally:
            os.environ.pop(GROUP_SWITCH, None)

    rg = h.prove(verify=True)  # warm-up and correctness
    pg = (h.proof_bytes(rg), h.msgs(), h.finals())
    os.environ[GROUP_SWITCH] = "0"
    try:
        ru = h.prove(verify=True)
    finally:
        os.environ.pop(GROUP_SWITCH, None)
    pu = (h.proof_bytes(ru), h.msgs(), h.finals())
    assert rg.verified == 1 and ru.verified == 1, "a Shamir Spartan proof was rejected: " + h.last_error()
    assert rg.grouped == 1 and ru.grouped == 0, "the switch did not select the legs"
    assert pg == pu, "the grouped and the ungrouped prove differ in proof, messages or final shares"
    digest = bytes(rg.proof_digest)
    legs = {False: [], True: []}
    calls = {}
    while sum(x.wall_ms for x in legs[False]) < args.min_seconds * 1e3 or sum(x.wall_ms for x in legs[True]) < args.min_seconds * 1e3 or len(legs[False]) < 6:
        for u in (False, True):
            r_, calls[u] = leg(u)
            assert bytes(r_.proof_digest) == digest, "a repetition's proof differs"
            legs[u].append(r_)
    sums = lambda x: x.t_sumcheck1_ms + x.t_sumcheck2_ms
    rep = lambda rs, c: dict(stats([x.wall_ms for x in rs]), driver_split={k: stats([getattr(x, k) for x in rs]) for k in split},
                             sumchecks=stats([sums(x) for x in rs]), calls=c)
    t_g, t_u = [x.wall_ms for x in legs[False]], [x.wall_ms for x in legs[True]]
    spread_u = max(t_u) - min(t_u)
    res["prover"] = {
        "grouped_whole_prove": rep(legs[False], calls[False]),
        "ungrouped_whole_prove_same_run": rep(legs[True], calls[True]),
        "grouped_vs_ungrouped_speedup": round(med(t_u) / med(t_g), 3),
        "sumchecks_grouped_vs_ungrouped_speedup": round(med([sums(x) for x in legs[True]]) / med([sums(x) for x in legs[False]]), 3),
        "grouped_slower_than_ungrouped_by_ms": round(med(t_g) - med(t_u), 4),
        "ungrouped_min_max_spread_ms": round(spread_u, 4),
        "grouped_not_slower_beyond_ungrouped_spread": bool(med(t_g) - med(t_u) <= spread_u),
        "proofs_messages_finals_equal": True,
        "proof_sha256": digest.hex(),
    }
    res["timing"] = ("whole prove: the driver's host clock from every party's stream drained to every party's stream drained (one thread drives the "
                     "parties in turn: sums over parties), setup (instance, SRS, sharing) outside; first two rounds: from an event on party 0's idle "
                     "stream to the last of the events behind the parties' streams, polynomial and group creation outside; the grouped and the "
                     "ungrouped leg alternating in one process, the ungrouped leg being the yardstick; the seed's keys and counters reused across "
                     "repetitions (timing only)")
    h.close()
    emit(res)


def jolt_spartan_legs():
    """--jolt-spartan: (xxiv) unless --only-group, then (xxv); the harness owns one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --jolt-spartan: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    senders = 2 * T + 1
    res = {
        "what": "co-jolt's Spartan worker by Shamir parties: the outer and shift sumchecks as groups (one fused bind + sums launch, one finishing "
                "launch and one fetch per round for all senders) against the per-sender calls (COZK_SHAMIR_GP_GROUP=0)",
        "system": args.system, "log_steps": args.log_steps, "steps": n, "parties": N, "degree": T, "senders": senders, "openers": T + 1,
        "seed": args.seed, "device": torch.cuda.get_device_name(0),
    }
    if not args.only_group:
        OU = importlib.import_module("co-zkvms_amd.outer")
        if args.system == "jolt":
            import pyjolt_r1cs as J
            (uniform, cross, padded), ncols = J.build_system(), J.NUM_INPUTS
        else:
            import pyspartan_outer as SO
            (uniform, cross, padded), ncols = SO.synthetic_system(), 14
        n_tau = args.log_steps + padded.bit_length() - 1
        pcs, streams = party_contexts()
        whole = lambda fn: whole_call(pcs, streams, fn)
        cols = [[cozk.Rep3DensePolynomial.random(pcs[p], n, 3000 + 100 * p + v, mode=cozk.MODE_PLAIN) for v in range(ncols)] for p in range(senders)]
        tau = [pow(5, 3 + i, cozk.FR_MOD) for i in range(n_tau)]
        r = cozk.fr_to_mont_limbs([pow(3, 77, cozk.FR_MOD)])[0]
        claims = np.ascontiguousarray(cozk.fr_to_mont_limbs([pow(7, 11 + p, cozk.FR_MOD) for p in range(senders)]))
        mk = lambda: [OU.SpartanOuter(pcs[p], "plain", 0, uniform, cross, cols[p], padded, tau) for p in range(senders)]

        def run_g():
            members = mk()
            g = cozk.OuterGroup(pcs[0], members)
            ms, out = whole(lambda: [g.round_raw(None, claims), g.round_raw(r, claims)])
            g.free()
            for st in members:
                st.free()
            return ms, out

        def run_s():
            members = mk()

            def rounds():
                outs = [np.zeros((senders, 4, 4), dtype=np.uint64) for _ in range(2)]
                for j in range(2):
                    for p in range(senders):
                        c = pcs[p]
                        c.check(c._l.cozk_outer_round(c.h, members[p].h, r.ctypes.data if j else None, claims[p].ctypes.data, outs[j][p].ctypes.data))
                return outs
            out = whole(rounds)
            for st in members:
                st.free()
            return out

        og, os_ = run_g()[1], run_s()[1]
        assert all(np.array_equal(x, y) for x, y in zip(og, os_)), "the group rounds and the per-sender rounds differ"
        t_g, t_s = [], []
        while sum(t_g) < args.min_seconds * 1e3 or sum(t_s) < args.min_seconds * 1e3 or len(t_g) < 6:
            t_g.append(run_g()[0])
            t_s.append(run_s()[0])
        res["first_two_rounds"] = {"group_rounds": stats(t_g), "per_sender_rounds_same_run": stats(t_s),
                                   "group_vs_per_sender_speedup": round(med(t_s) / med(t_g), 3), "outputs_equal": True}
        cols = None
        for pc in pcs:
            pc.close()

    h = cozk.ShamirJoltSpartanHarness(log_steps=args.log_steps, system=args.system, parties=N, degree=T, devices=0, seed=args.seed)
    split = ("t_build_ms", "t_masks_ms", "t_outer_ms", "t_inner_ms", "t_shift_ms", "t_openings_ms")

    def leg(ungrouped):
        if ungrouped:
            os.environ[GROUP_SWITCH] = "0"  # read by the library on every prove
        try:
            r_ = h.prove(verify=False)
            st = h.stats()
            return r_, {k: int(getattr(st, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}
        finally:
            os.environ.pop(GROUP_SWITCH, None)

    rg = h.prove(verify=True)  # warm-up and correctness
    pg = (h.proof_bytes(rg), h.msgs(), h.finals())
    os.environ[GROUP_SWITCH] = "0"
    try:
        ru = h.prove(verify=True)
    finally:
        os.environ.pop(GROUP_SWITCH, None)
    pu = (h.proof_bytes(ru), h.msgs(), h.finals())
    assert rg.verified == 1 and ru.verified == 1, "a Shamir Jolt-Spartan proof was rejected: " + h.last_error()
    assert rg.grouped == 1 and ru.grouped == 0, "the switch did not select the legs"
    assert pg == pu, "the grouped and the ungrouped prove differ in proof, messages or final shares"
    digest = bytes(rg.proof_digest)
    legs = {False: [], True: []}
    calls = {}
    while sum(x.wall_ms for x in legs[False]) < args.min_seconds * 1e3 or sum(x.wall_ms for x in legs[True]) < args.min_seconds * 1e3 or len(legs[False]) < 30:
        for u in (False, True):
            r_, calls[u] = leg(u)
            assert bytes(r_.proof_digest) == digest, "a repetition's proof differs"
            legs[u].append(r_)
    sums = lambda x: x.t_outer_ms + x.t_shift_ms
    rep = lambda rs, c: dict(stats([x.wall_ms for x in rs]), driver_split={k: stats([getattr(x, k) for x in rs]) for k in split},
                             outer_and_shift=stats([sums(x) for x in rs]), calls=c)
    t_g, t_u = [x.wall_ms for x in legs[False]], [x.wall_ms for x in legs[True]]
    spread_u = max(t_u) - min(t_u)
    res["prover"] = {
        "grouped_whole_prove": rep(legs[False], calls[False]),
        "ungrouped_whole_prove_same_run": rep(legs[True], calls[True]),
        "grouped_vs_ungrouped_speedup": round(med(t_u) / med(t_g), 3),
        "outer_and_shift_grouped_vs_ungrouped_speedup": round(med([sums(x) for x in legs[True]]) / med([sums(x) for x in legs[False]]), 3),
        "grouped_slower_than_ungrouped_by_ms": round(med(t_g) - med(t_u), 4),
        "ungrouped_min_max_spread_ms": round(spread_u, 4),
        "grouped_not_slower_beyond_ungrouped_spread": bool(med(t_g) - med(t_u) <= spread_u),
        "proofs_messages_finals_equal": True,
        "proof_sha256": digest.hex(),
    }
    res["timing"] = ("whole prove: the driver's host clock from every party's stream drained to every party's stream drained (one thread drives the "
                     "parties in turn: sums over parties), setup (instance, sharing) outside, Az / Bz / Cz of every sender inside (t_build); first "
                     "two rounds: from an event on party 0's idle stream to the last of the events behind the parties' streams, state and group "
                     "creation outside; the grouped and the ungrouped leg alternating in one process, the ungrouped leg being the yardstick; the "
                     "seed's keys and counters reused across repetitions (timing only)")
    h.close()
    emit(res)


def primary_legs():
    """--primary: (xxvi) unless --only-group, then (xxvii); the harness owns one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --primary: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
    senders = 2 * T + 1
    res = {
        "what": "Lasso's primary sumcheck by Shamir parties: the degree reduction between the multiplication levels and the round finishes as "
                "level groups (two launches per exchange, two per finish, for all senders) against the per-sender composition "
                "(COZK_SHAMIR_GP_GROUP=0)",
        "log_n": args.log_n, "cycles": n, "n_mem": args.mems, "mix": args.mix, "parties": N, "degree": T, "senders": senders, "openers": T + 1,
        "seed": args.seed, "device": torch.cuda.get_device_name(0),
    }
    if not args.only_group:
        import pylookups, primary_ref as PR
        LK = importlib.import_module("co-zkvms_amd.lookups")
        import pyref as O
        instrs = pylookups.instr_table(args.mems)
        which = [pylookups.mix_instr(1 if args.mix == "sha2" else 0, v) for v in O.synthetic_small(args.seed + 1234567, n, 8)]
        pcs, streams = party_contexts()
        pcs, streams = pcs[:senders], streams[:senders]
        whole = lambda fn: whole_call(pcs, streams, fn)
        rows = PR.rows(LK, instrs)
        flag_cols = [np.array([1 if w == i else 0 for w in which], dtype=np.uint8) for i in range(len(instrs))]
        flags = [[cozk.Vec.from_numpy(pcs[p], c, kind=cozk.SCALAR_U8) for c in flag_cols] for p in range(senders)]
        E = [[cozk.Rep3DensePolynomial.random(pcs[p], n, 3000 + 100 * p + m, mode=cozk.MODE_PLAIN) for m in range(args.mems)] for p in range(senders)]
        outs = [cozk.Rep3DensePolynomial.random(pcs[p], n, 2900 + p, mode=cozk.MODE_PLAIN) for p in range(senders)]
        eqs = [cozk.eq_evals(pcs[p], [pow(5, 3 + i, cozk.FR_MOD) for i in range(args.log_n)]) for p in range(senders)]
        keys = [[key(16 * p + c) for c in range(T)] for p in range(senders)]
        pts = list(range(1, senders + 1))

        def mk():
            prims = [LK.PrimarySumcheck.create(pcs[p], cozk.MODE_PLAIN, 0, rows, flags[p], E[p], outs[p], eqs[p]) for p in range(senders)]
            begun = [pr.round_begin() for pr in prims]
            assert all(b == begun[0] for b in begun)
            return prims, begun[0][1]

        def read(p, ptr, cnt):
            return np.array(PR.read_fr(cozk, pcs[p], ptr, cnt), dtype=object)

        def run_g(keep=False):
            prims, n_levels = mk()
            g = LK.PrimaryGroup(pcs[0], prims, keys)
            D = prims[0].degree()

            def body():
                ctr, el = 0, []
                for level in range(1, n_levels + 1):
                    el.append(g.level(level, ctr))
                    ctr += el[-1]
                return el, g.round_finish_raw(D)
            ms, (el, msg) = whole(body)
            bufs = [[read(p, *g.level_buffer(p, lv)) for p in range(senders)] for lv in range(1, n_levels + 1) if el[lv - 1]] if keep else None
            g.free()
            for pr in prims:
                pr.free()
            return ms, (el, msg, bufs)

        def run_s(keep=False):
            prims, n_levels = mk()
            D = prims[0].degree()

            def body():
                ctr, el, ptrs = 0, [], []
                for level in range(1, n_levels + 1):
                    out = [pr.level(level) for pr in prims]
                    cnt = out[0][2]
                    el.append(cnt)
                    if not cnt:
                        continue
                    dealt = []
                    for p in range(senders):
                        v = cozk.Vec.alloc(pcs[p], cnt)
                        PR._copy(cozk, pcs[p], v.device_ptr(), out[p][0], 32 * cnt)
                        dealt.append(v.shamir_scatter(keys[p], T, pcs, counter=ctr))
                        v.free()
                    for q in range(senders):
                        c = cozk.shamir_combine([dealt[p][q] for p in range(senders)], pts, 2 * T)
                        PR._copy(cozk, pcs[q], out[q][0], c.device_ptr(), 32 * cnt)
                        c.free()
                    for d in dealt:
                        free(d)
                    ptrs.append([o[0] for o in out])
                    ctr += cnt
                msg = np.zeros((senders, D, 4), dtype=np.uint64)
                for p in range(senders):
                    pcs[p].check(pcs[p]._l.cozk_primary_round_finish(pcs[p].h, prims[p].h, msg[p].ctypes.data))
                return el, msg, ptrs
            ms, (el, msg, ptrs) = whole(body)
            bufs = [[read(p, ptrs[i][p], cnt) for p in range(senders)] for i, cnt in enumerate(c for c in el if c)] if keep else None
            for pr in prims:
                pr.free()
            return ms, (el, msg, bufs)

        keep = n <= (1 << 12)  # the level buffers are compared as integers on the host: small sizes only; the messages always
        og, os_ = run_g(keep)[1], run_s(keep)[1]
        assert og[0] == os_[0] and np.array_equal(og[1], os_[1]), "the group round and the per-sender composition differ"
        if keep:
            assert all(np.array_equal(a, b) for la, lb in zip(og[2], os_[2]) for a, b in zip(la, lb)), "the level buffers differ"
        t_g, t_s = [], []
        while sum(t_g) < args.min_seconds * 1e3 or sum(t_s) < args.min_seconds * 1e3 or len(t_g) < 6:
            t_g.append(run_g()[0])
            t_s.append(run_s()[0])
        res["first_round"] = {"group_levels_and_finish": stats(t_g), "per_sender_composition_same_run": stats(t_s),
                              "group_vs_per_sender_speedup": round(med(t_s) / med(t_g), 3), "n_elems_per_level": og[0], "messages_equal": True,
                              "staging_block_bytes": senders * senders * max(og[0] + [0]) * 32,
                              "level_buffers_compared": bool(keep),
                              "note": "the composition copies every level buffer into a vector before it deals it; the prover's own ungrouped path deals "
                                      "a view of the buffer"}
        flags = E = outs = eqs = None
        for pc in pcs:
            pc.close()

    h = cozk.ShamirPrimary(log_n=args.log_n, n_mem=args.mems, mix=args.mix, parties=N, degree=T, devices=0, seed=args.seed)
    split = ("t_build_ms", "t_masks_ms", "t_rounds_ms", "t_finals_ms")

    def leg(ungrouped):
        if ungrouped:
            os.environ[GROUP_SWITCH] = "0"  # read by the library on every prove
        try:
            r_ = h.prove(verify=False)
            st = h.stats()
            return r_, {k: int(getattr(st, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}
        finally:
            os.environ.pop(GROUP_SWITCH, None)

    rg = h.prove(verify=True)  # warm-up and correctness
    pg = (h.proof_bytes(rg), h.msgs(), h.finals())
    os.environ[GROUP_SWITCH] = "0"
    try:
        ru = h.prove(verify=True)
    finally:
        os.environ.pop(GROUP_SWITCH, None)
    pu = (h.proof_bytes(ru), h.msgs(), h.finals())
    assert rg.verified == 1 and ru.verified == 1, "a Shamir primary proof was rejected: " + h.last_error()
    assert rg.grouped == 1 and ru.grouped == 0, "the switch did not select the legs"
    assert pg == pu, "the grouped and the ungrouped prove differ in proof, messages or final shares"
    digest = bytes(rg.proof_digest)
    legs = {False: [], True: []}
    calls = {}
    while sum(x.wall_ms for x in legs[False]) < args.min_seconds * 1e3 or sum(x.wall_ms for x in legs[True]) < args.min_seconds * 1e3 or len(legs[False]) < 10:
        for u in (False, True):
            r_, calls[u] = leg(u)
            assert bytes(r_.proof_digest) == digest, "a repetition's proof differs"
            legs[u].append(r_)
    rep = lambda rs, c: dict(stats([x.wall_ms for x in rs]), driver_split={k: stats([getattr(x, k) for x in rs]) for k in split}, calls=c)
    t_g, t_u = [x.wall_ms for x in legs[False]], [x.wall_ms for x in legs[True]]
    r_g, r_u = [x.t_rounds_ms for x in legs[False]], [x.t_rounds_ms for x in legs[True]]
    spread_u = max(t_u) - min(t_u)
    res["prover"] = {
        "grouped_whole_prove": rep(legs[False], calls[False]),
        "ungrouped_whole_prove_same_run": rep(legs[True], calls[True]),
        "grouped_vs_ungrouped_speedup": round(med(t_u) / med(t_g), 3),
        "rounds_grouped_vs_ungrouped_speedup": round(med(r_u) / med(r_g), 3),
        "grouped_slower_than_ungrouped_by_ms": round(med(t_g) - med(t_u), 4),
        "ungrouped_min_max_spread_ms": round(spread_u, 4),
        "grouped_not_slower_beyond_ungrouped_spread": bool(med(t_g) - med(t_u) <= spread_u),
        "proofs_messages_finals_equal": True,
        "proof_sha256": digest.hex(),
        "sumcheck_degree": int(rg.degree), "exchanges": int(rg.n_exchanges), "elements_exchanged_per_pair": int(rg.n_exchanged),
    }
    res["timing"] = ("whole prove: the driver's host clock from every party's stream drained to every party's stream drained (one thread drives the "
                     "parties in turn: sums over parties), setup (instance, sharing) outside, eq and cozk_primary_create of every sender inside "
                     "(t_build); first round: from an event on party 0's idle stream to the last of the events behind the senders' streams, state "
                     "and group creation and round_begin outside; the grouped and the ungrouped leg alternating in one process, the ungrouped "
                     "leg being the yardstick; the seed's keys and counters reused across repetitions (timing only)")
    h.close()
    emit(res)


def primary_king_legs():
    """--primary --king: (xxviii) unless --only-group, then (xxix) and (xxx); one context per party on this GPU"""
    if 2 * T + 1 > N or 2 * T > 15:
        raise SystemExit("run_shamir --primary --king: needs 2 * degree + 1 <= parties and 2 * degree <= 15")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
    senders = 2 * T + 1
    res = {
        "what": "Lasso's primary sumcheck by Shamir parties, the KING level exchange on a preprocessed double-random pair "
                "(cozk_primary_group_level_king, cozk_shamir_primary_prep + cozk_shamir_primary_prove_king) against the resharing exchange "
                "(cozk_primary_group_level, cozk_shamir_primary_prove), which is the yardstick",
        "log_n": args.log_n, "cycles": n, "n_mem": args.mems, "mix": args.mix, "parties": N, "degree": T, "senders": senders, "openers": T + 1,
        "seed": args.seed, "device": torch.cuda.get_device_name(0),
    }
    if not args.only_group:
        import pylookups, primary_ref as PR
        LK = importlib.import_module("co-zkvms_amd.lookups")
        import pyref as O
        instrs = pylookups.instr_table(args.mems)
        which = [pylookups.mix_instr(1 if args.mix == "sha2" else 0, v) for v in O.synthetic_small(args.seed + 1234567, n, 8)]
        pcs, streams = party_contexts()
        pcs, streams = pcs[:senders], streams[:senders]
        whole = lambda fn: whole_call(pcs, streams, fn)
        rows = PR.rows(LK, instrs)
        flag_cols = [np.array([1 if w == i else 0 for w in which], dtype=np.uint8) for i in range(len(instrs))]
        flags = [[cozk.Vec.from_numpy(pcs[p], c, kind=cozk.SCALAR_U8) for c in flag_cols] for p in range(senders)]
        E = [[cozk.Rep3DensePolynomial.random(pcs[p], n, 3000 + 100 * p + m, mode=cozk.MODE_PLAIN) for m in range(args.mems)] for p in range(senders)]
        outs = [cozk.Rep3DensePolynomial.random(pcs[p], n, 2900 + p, mode=cozk.MODE_PLAIN) for p in range(senders)]
        eqs = [cozk.eq_evals(pcs[p], [pow(5, 3 + i, cozk.FR_MOD) for i in range(args.log_n)]) for p in range(senders)]
        keys = [[key(16 * p + c) for c in range(T)] for p in range(senders)]
        plan, total = LK.primary_plan(pcs[0], rows, flags[0], args.log_n)
        first = sum(plan[0])  # the first round's exchanges use the pair's first elements
        rt = [cozk.Vec.random(pcs[p], first, seed=5100 + p) for p in range(senders)]
        r2t = [cozk.Vec.random(pcs[p], first, seed=5200 + p) for p in range(senders)]

        def mk():
            prims = [LK.PrimarySumcheck.create(pcs[p], cozk.MODE_PLAIN, 0, rows, flags[p], E[p], outs[p], eqs[p]) for p in range(senders)]
            begun = [pr.round_begin() for pr in prims]
            assert all(b == begun[0] for b in begun)
            return prims, begun[0][1]

        def raw(p, ptr, cnt):
            host = np.zeros((max(cnt, 1), 4), dtype=np.uint64)
            PR._copy(cozk, pcs[p], host.ctypes.data, ptr, 32 * cnt)
            return host[:cnt]

        def run_group(king, keep=False):
            """the first round's levels as ONE group: king levels on a keyless group, or the resharing levels"""
            prims, n_levels = mk()
            g = LK.PrimaryGroup(pcs[0], prims, None if king else keys)

            def body():
                off, el = 0, []
                for level in range(1, n_levels + 1):
                    el.append(g.level_king(level, rt, r2t, off) if king else g.level(level, off))
                    off += el[-1]
                return el
            ms, el = whole(body)
            bufs = [[raw(p, *g.level_buffer(p, lv)) for p in range(senders)] for lv in range(1, n_levels + 1) if el[lv - 1]] if keep else None
            staging = g.staging_bytes()
            g.free()
            for pr in prims:
                pr.free()
            return ms, (el, bufs, staging)

        def run_composed(keep=False):
            """the king exchange from the existing calls: cozk_primary_level per sender, its r_2t slice added (cozk_vec_binop), ONE
            cozk_shamir_king_finish at the offset on the king's context, each result copied into that sender's level buffer"""
            prims, n_levels = mk()

            def body():
                off, el, ptrs = 0, [], []
                for level in range(1, n_levels + 1):
                    out = [pr.level(level) for pr in prims]
                    cnt = out[0][2]
                    el.append(cnt)
                    if not cnt:
                        continue
                    masked = []
                    for p in range(senders):
                        v, s = cozk.Vec.alloc(pcs[p], cnt), cozk.Vec.alloc(pcs[p], cnt)
                        PR._copy(cozk, pcs[p], v.device_ptr(), out[p][0], 32 * cnt)
                        PR._copy(cozk, pcs[p], s.device_ptr(), r2t[p].device_ptr() + 32 * off, 32 * cnt)
                        masked.append(v.binop(cozk.OP_ADD, s))
                        v.free(), s.free()
                        pcs[p].synchronize()
                    fin = cozk.shamir_king_finish(pcs[0], masked, T, rt, r_offset=off)
                    for q in range(senders):
                        PR._copy(cozk, pcs[0], out[q][0], fin[q].device_ptr(), 32 * cnt)
                    pcs[0].synchronize()
                    free(masked), free(fin)
                    ptrs.append([o[0] for o in out])
                    off += cnt
                return el, ptrs
            ms, (el, ptrs) = whole(body)
            bufs = [[raw(p, ptrs[i][p], cnt) for p in range(senders)] for i, cnt in enumerate(c for c in el if c)] if keep else None
            for pr in prims:
                pr.free()
            return ms, (el, bufs)

        keep = n <= (1 << 14)  # the level buffers are compared raw on the host: small sizes only
        ok, oc = run_group(True, keep)[1], run_composed(keep)[1]
        assert ok[0] == oc[0] == plan[0][:len(ok[0])], "the first round's exchanges differ from the plan"
        if keep:
            assert all(np.array_equal(a, b) for la, lb in zip(ok[1], oc[1]) for a, b in zip(la, lb)), "the level buffers differ"
        run_group(False)
        t_k, t_c, t_r = [], [], []
        staging = {}
        while sum(t_k) < args.min_seconds * 1e3 or sum(t_r) < args.min_seconds * 1e3 or len(t_k) < 6:
            ms, (_, _, staging["king"]) = run_group(True)
            t_k.append(ms)
            ms, (_, _, staging["resharing"]) = run_group(False)
            t_r.append(ms)
            t_c.append(run_composed()[0])
        res["first_round"] = {"king_levels_one_group": stats(t_k), "resharing_levels_one_group_same_run": stats(t_r),
                              "king_composed_per_sender_same_run": stats(t_c),
                              "king_vs_resharing_group_speedup": round(med(t_r) / med(t_k), 3),
                              "king_group_vs_composed_speedup": round(med(t_c) / med(t_k), 3), "n_elems_per_level": ok[0],
                              "staging_block_bytes": staging, "level_buffers_compared": bool(keep),
                              "note": "levels only (no round finish); random halves stand in for the preprocessed pair; the composition "
                                      "copies every level buffer and every slice of a half into a vector before it adds them"}
        free(rt), free(r2t)
        flags = E = outs = eqs = None
        for pc in pcs:
            pc.close()

    mkh = lambda: cozk.ShamirPrimary(log_n=args.log_n, n_mem=args.mems, mix=args.mix, parties=N, degree=T, devices=0, seed=args.seed)
    split = ("t_build_ms", "t_masks_ms", "t_rounds_ms", "t_finals_ms")

    def king_prove(ungrouped=False, verify=False, king=0):
        """a fresh handle and a fresh preprocessing per repetition, both outside the timed prove"""
        hk = mkh()
        pre = hk.prep()
        if ungrouped:
            os.environ[GROUP_SWITCH] = "0"  # read by the library on every prove
        try:
            r_ = hk.prove_king(king=king, verify=verify)
            st = hk.stats()
            got = (hk.proof_bytes(r_), hk.msgs(), hk.finals()) if verify else None
            return r_, pre, {k: int(getattr(st, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}, got
        finally:
            os.environ.pop(GROUP_SWITCH, None)
            hk.close()

    h = mkh()  # the resharing prover: the code as it stands without the king construct
    rr = h.prove(verify=True)
    assert rr.verified == 1 and rr.grouped == 1, "the resharing proof was rejected: " + h.last_error()
    digest = bytes(rr.proof_digest)
    kg, pre, _, got_g = king_prove(verify=True, king=N - 1)
    ku, _, _, got_u = king_prove(ungrouped=True, verify=True, king=0)
    assert kg.verified == 1 and ku.verified == 1 and kg.grouped == 1 and ku.grouped == 0, "a king proof was rejected or the switch did not select the legs"
    assert got_g == got_u, "the grouped and the ungrouped king prove differ in proof, messages or final shares"
    assert bytes(kg.proof_digest) == digest and got_g[2] == h.finals(), "the king proof is not the resharing prover's"
    assert kg.n_exchanged == pre.pair_elems == rr.n_exchanged
    legs = {"king": [], "king_ungrouped": [], "resharing": []}
    offline, calls = [], {}
    enough = lambda k: sum(x.wall_ms for x in legs[k]) >= args.min_seconds * 1e3 and len(legs[k]) >= 6
    while not (enough("king") and enough("resharing")):
        r_, p_, calls["king"], _ = king_prove()
        legs["king"].append(r_)
        offline.append(p_.t_offline_ms)
        r_ = h.prove(verify=False)
        st = h.stats()
        calls["resharing"] = {k: int(getattr(st, k)) for k in ("group_rounds", "single_rounds", "group_finals", "single_finals")}
        legs["resharing"].append(r_)
        if len(legs["king_ungrouped"]) < 3:
            r_, _, calls["king_ungrouped"], _ = king_prove(ungrouped=True)
            legs["king_ungrouped"].append(r_)
        assert all(bytes(x[-1].proof_digest) == digest for x in legs.values()), "a repetition's proof differs"
    rep = lambda rs, c: dict(stats([x.wall_ms for x in rs]), driver_split={k: stats([getattr(x, k) for x in rs]) for k in split}, calls=c)
    w = {k: [x.wall_ms for x in v] for k, v in legs.items()}
    rounds = {k: [x.t_rounds_ms for x in v] for k, v in legs.items()}
    spread_r = max(w["resharing"]) - min(w["resharing"])
    res["prover"] = {
        "king_online_whole_prove_grouped": rep(legs["king"], calls["king"]),
        "resharing_whole_prove_grouped_same_run": rep(legs["resharing"], calls["resharing"]),
        "king_online_whole_prove_ungrouped_same_run": rep(legs["king_ungrouped"], calls["king_ungrouped"]),
        "king_offline_prep": stats(offline),
        "king_online_vs_resharing_speedup": round(med(w["resharing"]) / med(w["king"]), 3),
        "rounds_king_vs_resharing_speedup": round(med(rounds["resharing"]) / med(rounds["king"]), 3),
        "king_grouped_vs_ungrouped_speedup": round(med(w["king_ungrouped"]) / med(w["king"]), 3),
        "king_online_slower_than_resharing_by_ms": round(med(w["king"]) - med(w["resharing"]), 4),
        "resharing_min_max_spread_ms": round(spread_r, 4),
        "king_online_not_slower_beyond_resharing_spread": bool(med(w["king"]) - med(w["resharing"]) <= spread_r),
        "proofs_equal_finals_equal_grouped_ungrouped_equal": True,
        "proof_sha256": digest.hex(),
        "sumcheck_degree": int(rr.degree), "exchanges": int(rr.n_exchanges), "pair_elems": int(pre.pair_elems),
        "online_elements_per_slot_value": {"king": 2, "resharing": senders * senders},
    }
    res["timing"] = ("whole prove: the driver's host clock from every party's stream drained to every party's stream drained (one thread drives the "
                     "parties in turn: sums over parties), setup (instance, sharing) outside, eq and cozk_primary_create of every sender inside "
                     "(t_build); the king prove's preprocessing is OFFLINE and reported on its own (plan + both dealings, host clock, every "
                     "stream drained at both ends), a fresh handle and preprocessing per repetition; first round: from an event on party 0's "
                     "idle stream to the last of the events behind the senders' streams, state and group creation and round_begin outside; "
                     "the legs alternate in one process, the grouped resharing prove being the yardstick; the seed's keys and counters "
                     "reused across repetitions (timing only)")
    h.close()
    emit(res)


if args.primary and args.king:
    primary_king_legs()
    ctx.close()
    raise SystemExit(0)

if args.primary:
    primary_legs()
    ctx.close()
    raise SystemExit(0)

if args.jolt_spartan:
    jolt_spartan_legs()
    ctx.close()
    raise SystemExit(0)

if args.spartan:
    spartan_legs()
    ctx.close()
    raise SystemExit(0)

if args.tgp:
    tgp_legs()
    ctx.close()
    raise SystemExit(0)

if args.gp and args.only_group:
    group_legs_only()
    ctx.close()
    raise SystemExit(0)

if args.gp and args.king:
    gp_king_legs()
    ctx.close()
    raise SystemExit(0)

if args.gp:
    gp_legs()
    ctx.close()
    raise SystemExit(0)

if args.mul and args.king:
    king_legs()
    ctx.close()
    raise SystemExit(0)

if args.mul:
    mul_legs()
    ctx.close()
    raise SystemExit(0)

# correctness once, which is also the warm-up of both legs
f, c = fused(A, keys_a), composed(A, keys_a)
equal = all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(f, c))
free(f), free(c)
assert equal, "the fused share and the composed share differ"
for _ in range(2):
    free(timed(lambda: fused(A, keys_a))[1]), free(timed(lambda: composed(A, keys_a))[1])

t_f, t_c = [], []
while sum(t_f) < args.min_seconds * 1e3 or sum(t_c) < args.min_seconds * 1e3 or len(t_f) < 5:  # alternating
    ms, r = timed(lambda: fused(A, keys_a)); t_f.append(ms); free(r)
    ms, r = timed(lambda: composed(A, keys_a)); t_c.append(ms); free(r)

sa, sb = fused(A, keys_a), fused(B, keys_b)
pts = list(range(N, N - K, -1))


def products():
    return [sa[p - 1].binop(cozk.OP_MUL, sb[p - 1]) for p in range(1, N + 1)]


free(timed(products)[1])
t_m = []
while sum(t_m) < args.min_seconds * 1e3 or len(t_m) < 5:
    ms, r = timed(products); t_m.append(ms); free(r)
prod = products()
sel = [(prod if OPEN_PRODUCT else sa)[p - 1] for p in pts]
free(timed(lambda: cozk.shamir_combine(sel, pts, OPEN_DEGREE))[1])
t_o = []
while sum(t_o) < args.min_seconds * 1e3 or len(t_o) < 5:
    ms, r = timed(lambda: cozk.shamir_combine(sel, pts, OPEN_DEGREE)); t_o.append(ms); free(r)
opened = cozk.shamir_combine(sel, pts, OPEN_DEGREE)
opens = bool(np.array_equal(opened.to_numpy(), (A.binop(cozk.OP_MUL, B) if OPEN_PRODUCT else A).to_numpy()))
assert opens, "the combine leg did not open " + ("the product of the secrets" if OPEN_PRODUCT else "the secret")


share_bytes, comp_bytes = (1 + N) * 32 * n, 32 * T * n + N * T * (64 + 96) * n
mul_bytes, comb_bytes = N * 96 * n, (K + 1) * 32 * n
share_bps = share_bytes / (med(t_f) * 1e-3)
res = {
    "what": "Shamir seam: fused share vs the same sharing composed from earlier entry points, per-party product, combine",
    "log_n": args.log_n, "parties": N, "degree": T, "combine_from": K, "device": torch.cuda.get_device_name(0),
    "fused_share": dict(stats(t_f), algorithmic_bytes=share_bytes, bytes_per_s=round(share_bps, 1)),
    "composed_share": dict(stats(t_c), algorithmic_bytes_of_the_fused_form=share_bytes, bytes_moved_by_the_composition=comp_bytes,
                           launches=T + 2 * N * T),
    "fused_vs_composed_speedup": round(med(t_c) / med(t_f), 3),
    "outputs_equal": bool(equal),
    "fused_share_fraction_of_hbm": {"of_spec_8.0_TB_s": round(share_bps / HBM_PEAK, 4), "of_measured_copy_6.29_TB_s": round(share_bps / HBM_MEASURED, 4)},
    "fused_share_nearer_bound": "hbm" if share_bps / HBM_MEASURED >= 0.5 else "int_alu",
    "product_per_party": dict(stats(t_m), algorithmic_bytes=mul_bytes, bytes_per_s=round(mul_bytes / (med(t_m) * 1e-3), 1)),
    "combine": dict(stats(t_o), algorithmic_bytes=comb_bytes, bytes_per_s=round(comb_bytes / (med(t_o) * 1e-3), 1)),
    "combine_opens": "share x share, degree 2T" if OPEN_PRODUCT else "one sharing, degree T (2T + 1 > parties)", "combine_equals_expected": opens,
    "timing": "device events on the context's stream around each repetition (allocation from the context's pool included), legs (i) and (ii) alternating",
}
emit(res)
ctx.close()
