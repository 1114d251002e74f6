"""Time the output check of the read-write memory proof and the whole proof at 2^log_n steps over a memory of 2^log_mem words, 4 slots, an
io window of --io-len words at word --io-start (default 2050 at 64: not a power of two, W' = 4096, the order of Jolt's default layout;
jolt-core is not in the reference tree, so the shape is this project's choice), in one process, the variants of each comparison
alternating, outputs compared equal at the measured size:
  calls   the device calls alone: OutputCheck (create, log_mem rounds, final, free) against its dense twin, the chained flow's
          composition on Fr vectors of MEM entries (eq_evals, three poly_create, the linear combination v_final - v_io, log_mem rounds
          of prod_sumcheck_evals + three binds, three get_coeff); random challenges, every round's evaluations and the finals compared;
          a host clock around calls that each end with the stream drained
  prove   the whole proof (cozk_memory_proof_*, seed --seed) with windowed 1 and 0: two handles alternating, each verified once, digests
          compared: wall and per phase (commit, leaves, grand products, output check, timestamp check, open), and the peak device
          allocation of the output sumcheck on either path as the context's allocator counted it (first prove of each handle)
--warmup runs, then the median and spread of --runs runs.  Prints one JSON line.
  python tools/run_memory_proof.py --log-n 20 --log-mem 20 --runs 7 [--out profiles/memory_proof_2p20.json]
--bench <file> adds recorded bench.py lines ({"this_change": {...}, "parent": {...}}).
--rep3 measures the three-party form instead and prints its own JSON line (without the flag the output is unchanged; run_rep3): the
shared device calls (OutputCheck.shared) against the dense composition in REP3 for a party of each kind, and the three-party prove
(cozk_memory_proof_rep3_*) with windowed 1 and 0: its output-check phase, its peak device memory, every phase and the ring traffic.
  python tools/run_memory_proof.py --rep3 --log-n 20 --log-mem 20 --runs 7 [--out profiles/memory_proof_rep3_2p20.json]
Per-kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_memory_proof.py --rep3 --skip-prove ..., in a run
of its own; merge with --kernel-stats <the stats csv>: k_ocs_first_fold's launch against its bytes over the measured copy rate."""
import argparse, csv, importlib, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--log-mem", type=int, default=20)
ap.add_argument("--io-start", type=int, default=64)
ap.add_argument("--io-len", type=int, default=2050)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-prove", action="store_true")
ap.add_argument("--rep3", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--bench", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
M, MEM, LO, W = args.log_mem, 1 << args.log_mem, args.io_start, args.io_len

Z = importlib.import_module("co-zkvms_amd")
R = Z.FR_MOD
ctx = Z.Context(0)


def stats(xs):
    return {"runs": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def ab(variants):
    """variants: {name: call}; alternating rounds -> ({name: ms list}, {name: last output})"""
    ms, out = {k: [] for k in variants}, {}
    for it in range(args.warmup + args.runs):
        for name, call in variants.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            out[name] = call()
            ctx.synchronize()
            if it >= args.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms, out


HBM_MEASURED = 6.29e12  # B/s: the project's measured copy rate


def run_rep3():
    """--rep3: per party kind the shared calls (create, log_mem rounds, final, free) against the dense composition on that party's
    polynomials (the eq table, the two public vectors of MEM entries as polynomials, the linear combination, prod_sumcheck_evals and the
    binds), alternating, every round and the final compared; then the three-party prove with windowed 1 and 0, two handles alternating,
    each verified once, digests compared with each other and with the plain proof of the same seed and window."""
    P, inv2 = Z.Rep3DensePolynomial, (R + 1) // 2
    rng = np.random.default_rng(args.seed)
    sm = np.random.default_rng(args.seed + 1)
    fr = lambda: int.from_bytes(sm.bytes(40), "little") % R
    vio = rng.integers(0, 1 << 32, size=W, dtype=np.uint64).astype(np.uint32)
    d_vio = Z.Vec.from_numpy(ctx, vio, Z.SCALAR_U32)
    r_eq, rs = [fr() for _ in range(M)], [fr() for _ in range(M)]
    rng_l, vio_l = np.zeros((MEM, 4), dtype=np.uint64), np.zeros((MEM, 4), dtype=np.uint64)
    rng_l[LO:LO + W] = Z.fr_to_mont_limbs([1])[0]
    vio_l[LO:LO + W] = Z.fr_to_mont_limbs([int(x) for x in vio])
    d_rng, d_vio_fr = Z.Vec.from_numpy(ctx, rng_l), Z.Vec.from_numpy(ctx, vio_l)
    rng_l = vio_l = None
    lw = max(W - 1, 0).bit_length()
    fold_bytes = (2 * 64 + 32) * (MEM // 2)  # k_ocs_first_fold<2>: two pairs of components read, one Fr written, per output
    out = {"what": "the output check on a shared v_final: the shared device calls against the dense composition in REP3 for a party of each kind, the "
                   "three-party prove's output-check phase, peak memory and phases on either path",
           "log_n": args.log_n, "log_mem": M, "slots": 4, "io_start": LO, "io_len": W, "W_prime": 1 << lw, "sparse_rounds": max(M - lw, 0), "runs": args.runs,
           "warmup": args.warmup, "calls": {}}
    round1 = []  # the timed runs' round-1 calls of every party
    for party in range(3):
        mine = []
        # a party's two components: uniform field elements, as a share's are (the three parties' components here are independent draws)
        pv = P.from_vec_shares(ctx, Z.Vec.random(ctx, MEM, args.seed + 100 * party), Z.Vec.random(ctx, MEM, args.seed + 100 * party + 1))

        def windowed():
            oc = Z.OutputCheck.shared(ctx, pv, d_vio, LO, r_eq, party=party)
            res = [oc.round()]
            if M > 1:
                t0 = time.perf_counter()
                res.append(oc.round(rs[0]))  # the first fold, the dots on it, the sums and their fetch
                mine.append((time.perf_counter() - t0) * 1e3)
            res += [oc.round(rs[k - 1]) for k in range(2, M)]
            res.append(oc.final(rs[-1]))
            oc.free()
            return res

        def dense():
            pe, pr, pio = P.from_vec_shares(ctx, Z.eq_evals(ctx, r_eq)), P.from_vec_shares(ctx, d_rng), P.from_vec_shares(ctx, d_vio_fr)
            polys = [pe, pr, P.linear_combination([pv, pio], [1, R - 1], Z.MODE_REP3, party)]
            res = []
            for k in range(M):
                if k:
                    for p in polys:
                        p.bind(rs[k - 1], Z.HIGH_TO_LOW)
                res.append(Z.prod_sumcheck_evals(polys, 3))
            for p in polys:
                p.bind(rs[-1], Z.HIGH_TO_LOW)
            a, b = polys[2].get_bound_coeff(0)
            res.append((polys[0].get_bound_coeff(0), polys[1].get_bound_coeff(0), (a + b) * inv2 % R))
            for p in polys + [pio]:
                p.free()
            return res

        ms, last = ab({"windowed": windowed, "dense": dense})
        assert last["windowed"] == last["dense"], "the shared output check differs from the dense composition (party %d)" % party
        out["calls"]["party_%d" % party] = {
            "windowed_ms": stats(ms["windowed"]), "dense_ms": stats(ms["dense"]), "dense_over_windowed": round(statistics.median(ms["dense"]) / statistics.median(ms["windowed"]), 3),
            "slowest_windowed_below_fastest_dense": max(ms["windowed"]) < min(ms["dense"]), "outputs_equal": True}
        round1 += mine[args.warmup:]  # one call per iteration: the warm-up iterations come first
        pv.free()
    out["calls"].update({"includes": "create / the polynomials' creation and the linear combination, every round, the final values, free; python call overhead on either side",
                         "windowed_fr_entries": (MEM // 2 + 2 * (1 << lw)) if lw < M else 3 * MEM, "dense_fr_entries": "5 MEM: eq, io_range, v_io, two components of the difference",
                         "windowed_is_the_default": all(out["calls"]["party_%d" % p]["slowest_windowed_below_fastest_dense"] for p in range(3))})
    fold = {"bytes": fold_bytes, "floor_ms_at_6.29_TB_s": round(fold_bytes / HBM_MEASURED * 1e3, 4),
            "round_1_call_ms": stats(round1) if round1 else "not measured",
            "round_1_call_is": "the host clock around the call that runs k_ocs_first_fold<2>, k_oc_dots_fr and k_finish_sums and fetches the sums, the timed runs of every party: an upper bound of the kernel"}
    if args.kernel_stats:
        rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "k_ocs_" in r.get("Name", "")]
        fold["kernels"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)} for r in rows}
        ff = [float(r["AverageNs"]) for r in rows if "k_ocs_first_fold<2>" in r["Name"]]
        fold["fraction_of_copy_rate"] = round(fold_bytes / HBM_MEASURED / (ff[0] * 1e-9), 3) if ff else "not measured"
        fold["source"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_memory_proof.py --rep3 --skip-prove, a run of its own: avg_ms is one launch"
    else:
        fold["fraction_of_copy_rate"] = "not measured"
    out["k_ocs_first_fold"] = fold
    d_vio = d_rng = d_vio_fr = None
    if args.skip_prove:
        out["prove"] = "not measured"
    else:
        handles = {w: Z.MemoryProofRep3(log_n=args.log_n, log_mem=M, seed=args.seed, io_start=LO, io_len=W, windowed=(w == "windowed")) for w in ("windowed", "dense")}
        phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_out_ms", "t_open_ms")
        pm = {k: {ph: [] for ph in phases} for k in handles}
        digest, peak, last = {}, {}, {}
        for it in range(args.warmup + args.runs):
            for k, hd in handles.items():
                r = hd.prove(verify=(it == 0))
                assert it > 0 or r.verified == 1, hd.last_error()
                assert digest.setdefault(k, bytes(r.proof_digest)) == bytes(r.proof_digest)
                peak.setdefault(k, int(r.out_peak_bytes))
                last[k] = r
                if it >= args.warmup:
                    for ph in phases:
                        pm[k][ph].append(getattr(r, ph))
        assert digest["windowed"] == digest["dense"], "the two output-check paths give different proofs"
        plain = Z.MemoryProof(log_n=args.log_n, log_mem=M, seed=args.seed, io_start=LO, io_len=W, with_ts=False)
        plain_digest = bytes(plain.prove(verify=False).proof_digest)
        plain.close()
        assert plain_digest == digest["windowed"], "the Rep3 proof differs from the plain proof of the same seed and window"
        out["prove"] = {k: dict({ph: stats(pm[k][ph]) for ph in phases}, out_peak_bytes_first_prove=peak[k], t_witness_ms_of_create=round(last[k].t_witness_ms, 3),
                                t_share_ms_of_create=round(last[k].t_share_ms, 3), ring_bytes=int(last[k].ring_bytes), proof_bytes=int(last[k].proof_len),
                                prefix_len=int(last[k].prefix_len)) for k in handles}
        out["prove"].update({"verified": True, "digests_equal": True, "equal_to_the_plain_proof": True, "parties": "three contexts on one device",
                             "dense_over_windowed_t_out": round(statistics.median(pm["dense"]["t_out_ms"]) / statistics.median(pm["windowed"]["t_out_ms"]), 3),
                             "clock": "host clock around each phase of a worker, the maximum over the three parties; t_out_ms is the output sumcheck plus the opening of "
                                      "the shared v_final at its point; out_peak_bytes is the maximum over the parties; the dense path's public vectors are made in create"})
        for hd in handles.values():
            hd.close()
    out["bench_py_gpus1_steps3_warmup1"] = json.load(open(args.bench)) if args.bench else "not measured"
    print(json.dumps(out), flush=True)
    if args.out:
        open(args.out, "w").write(json.dumps(out, indent=1) + "\n")


if args.rep3:
    run_rep3()
    sys.exit(0)

# ---- the device calls alone against the dense twin
rng = np.random.default_rng(args.seed)
sm = np.random.default_rng(args.seed + 1)
fr = lambda: int.from_bytes(sm.bytes(40), "little") % R
vf = rng.integers(0, 1 << 32, size=MEM, dtype=np.uint64).astype(np.uint32)
vio = vf[LO:LO + W].copy()
d_vf, d_vio = Z.Vec.from_numpy(ctx, vf, Z.SCALAR_U32), Z.Vec.from_numpy(ctx, vio, Z.SCALAR_U32)
r_eq, rs = [fr() for _ in range(M)], [fr() for _ in range(M)]
one = Z.fr_to_mont_limbs([1])[0]
rng_l, vio_l = np.zeros((MEM, 4), dtype=np.uint64), np.zeros((MEM, 4), dtype=np.uint64)
rng_l[LO:LO + W] = one
vio_l[LO:LO + W] = Z.fr_to_mont_limbs([int(x) for x in vio])
d_rng, d_vio_fr = Z.Vec.from_numpy(ctx, rng_l), Z.Vec.from_numpy(ctx, vio_l)
p_vf = Z.Rep3DensePolynomial.from_vec_shares(ctx, Z.compact_linear_combination(ctx, [d_vf], [1]))  # the flow holds v_final as an Fr polynomial
rng_l = vio_l = None


def windowed():
    oc = Z.OutputCheck(ctx, d_vf, d_vio, LO, r_eq)
    out = [oc.round(rs[k - 1] if k else None) for k in range(M)]
    out.append(oc.final(rs[-1]))
    oc.free()
    return out


def dense():
    P = Z.Rep3DensePolynomial
    pe, pr, pio = P.from_vec_shares(ctx, Z.eq_evals(ctx, r_eq)), P.from_vec_shares(ctx, d_rng), P.from_vec_shares(ctx, d_vio_fr)
    polys = [pe, pr, P.linear_combination([p_vf, pio], [1, R - 1])]
    out = []
    for k in range(M):
        if k:
            for p in polys:
                p.bind(rs[k - 1], Z.HIGH_TO_LOW)
        out.append(Z.prod_sumcheck_evals(polys, 3))
    for p in polys:
        p.bind(rs[-1], Z.HIGH_TO_LOW)
    out.append(tuple(p.get_bound_coeff(0) for p in polys))
    for p in polys + [pio]:
        p.free()
    return out


ms, out = ab({"windowed": windowed, "dense": dense})
assert out["windowed"] == out["dense"], "the windowed output check differs from the dense composition"
lw = max(W - 1, 0).bit_length()
res = {"what": "the output check: the device calls against the dense composition, the proof's phase on either path, the prove per phase",
       "log_n": args.log_n, "log_mem": M, "io_start": LO, "io_len": W, "W_prime": 1 << lw, "sparse_rounds": max(M - lw, 0), "runs": args.runs, "warmup": args.warmup,
       "calls": {"windowed_ms": stats(ms["windowed"]), "dense_ms": stats(ms["dense"]),
                 "dense_over_windowed": round(statistics.median(ms["dense"]) / statistics.median(ms["windowed"]), 3), "outputs_equal": True,
                 "includes": "create / the Fr polynomials' creation, every round, the final values, free; python call overhead on either side",
                 "windowed_fr_entries": (MEM // 2 + 2 * (1 << lw)) if lw < M else 3 * MEM, "dense_fr_entries": 4 * MEM}}
d_vf = d_vio = d_rng = d_vio_fr = p_vf = None

# ---- the whole proof, per phase, windowed against dense
if args.skip_prove:
    res["prove"] = "not measured"
else:
    handles = {w: Z.MemoryProof(log_n=args.log_n, log_mem=M, seed=args.seed, io_start=LO, io_len=W, windowed=(w == "windowed")) for w in ("windowed", "dense")}
    phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_out_ms", "t_ts_ms", "t_open_ms")
    pm = {k: {ph: [] for ph in phases} for k in handles}
    digest, peak, extra = {}, {}, {}
    for it in range(args.warmup + args.runs):
        for k, hd in handles.items():
            r = hd.prove(verify=(it == 0))
            assert it > 0 or r.verified == 1, hd.last_error()
            assert digest.setdefault(k, bytes(r.proof_digest)) == bytes(r.proof_digest)
            peak.setdefault(k, int(r.out_peak_bytes))
            extra[k] = {"t_witness_ms_of_create": round(r.t_witness_ms, 3), "proof_bytes": int(r.proof_len), "prefix_len": int(r.prefix_len)}
            if it >= args.warmup:
                for ph in phases:
                    pm[k][ph].append(getattr(r, ph))
    assert digest["windowed"] == digest["dense"], "the two output-check paths give different proofs"
    res["prove"] = {k: dict({ph: stats(pm[k][ph]) for ph in phases}, out_peak_bytes_first_prove=peak[k], **extra[k]) for k in handles}
    res["prove"].update({"verified": True, "digests_equal": True,
                         "dense_over_windowed_t_out": round(statistics.median(pm["dense"]["t_out_ms"]) / statistics.median(pm["windowed"]["t_out_ms"]), 3),
                         "clock": "host clock around each phase of the worker; every phase ends in a device synchronise or a host exchange; t_out_ms is the "
                                  "output sumcheck plus the compact opening of v_final at its point; the dense path's Fr copies are made in create"})
    for hd in handles.values():
        hd.close()
res["bench_py_gpus1_steps3_warmup1"] = json.load(open(args.bench)) if args.bench else "not measured"
print(json.dumps(res), flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
