"""Time the device calls of the timestamp range-check proof at 2^log_n steps, 4 slots, each against the composition it replaces, in one
process, runs alternating, outputs compared equal at the measured size:
  leaves    cozk_timestamp_range_leaves (one launch, 25 circuits) against 25 cozk_fingerprint_leaves calls with a materialised iota column
  openings  cozk_compact_batch_evaluate_at_chi / cozk_compact_linear_combination over the 20 compact U32 columns against
            cozk_poly_batch_evaluate_at_chi / cozk_poly_linear_combination over Fr copies of them (made on the device before the
            clock starts: 32 bytes per entry, which is what the compact calls exist to avoid)
Both sides of the leaves A/B include one host synchronise (the fused call fetches its violation word and waits for the stream; the
composition's 25 launches are followed by a context synchronise), so its ratio is of whole calls, not of kernel time alone: the
per-kernel figures of the trace run say what the kernels take.
t_read is a seeded column with t_read[j] <= j; the counters come from cozk_timestamp_range_witness (M = N) and stay on the device.
Device events on the context's stream around each call; --warmup runs, then the median and spread of --runs runs.  The byte floors
are the algorithmic bytes below over the HBM rates of the MI355X (8.0 TB/s datasheet, 6.29 TB/s measured copy).
  prove     the whole proof (cozk_ts_proof_*: log_mem = log_n, seed --seed) with the fused leaves and with the composition, two handles
            alternating, each prove verified once and its digest compared: wall and per phase (commit, leaves, grand product, open;
            a host clock around work that ends in a synchronise or a host exchange), and the witness time of create
Prints one JSON line.
  python tools/run_ts_proof.py --log-n 20 --runs 7 [--out profiles/ts_range_proof_2p20.json]
Per-kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_ts_proof.py ..., in a run of its own; merge
with --kernel-stats <the stats csv>.  --bench <file> adds recorded bench.py lines ({"this_change": {...}, "parent": {...}})."""
import argparse, csv, ctypes, importlib, json, os, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--bench", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, NS = 1 << args.log_n, 4
NCIRC, NCOLS = 6 * NS + 1, 5 * NS
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12

import torch
Z = importlib.import_module("co-zkvms_amd")
R = Z.FR_MOD
ctx = Z.Context(0)
sp = ctypes.c_void_p()
ctx.check(ctx._l.cozk_ctx_stream(ctx.h, ctypes.byref(sp)))
stream = torch.cuda.ExternalStream(sp.value)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def ab(variants):
    """variants: {name: call}; alternating rounds -> ({name: ms list}, {name: last output})"""
    ms, outs = {k: [] for k in variants}, {}
    for it in range(args.warmup + args.runs):
        for name, call in variants.items():
            outs[name] = None  # the previous output goes back to the context's pool
            t, outs[name] = timed(call)
            if it >= args.warmup:
                ms[name].append(t)
    return ms, outs


def stats(xs, alg_bytes=None):
    med = statistics.median(xs)
    d = {"runs": [round(x, 4) for x in xs], "median": round(med, 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    if alg_bytes:
        d.update({"algorithmic_bytes": alg_bytes, "floor_ms_at_8.0_TBps": round(alg_bytes / HBM_SPEC * 1e3, 4), "floor_ms_at_6.29_TBps": round(alg_bytes / HBM_MEASURED * 1e3, 4),
                  "achieved_TBps": round(alg_bytes / med / 1e9, 3), "share_of_6.29_TBps": round(alg_bytes / med / 1e9 / 6.29, 3)})
    return d


rng = np.random.default_rng(args.seed)
u32 = lambda a: Z.Vec.from_numpy(ctx, np.ascontiguousarray(a, dtype=np.uint32), Z.SCALAR_U32)
t_read = [u32(rng.integers(0, 1 << 62, size=N) % (np.arange(N) + 1)) for _ in range(NS)]
rc_rt, rc_gmr, fc_rt, fc_gmr = Z.timestamp_range_witness(ctx, t_read, N)
sm = np.random.default_rng(args.seed + 1)
fr = lambda: int.from_bytes(sm.bytes(40), "little") % R
gamma, tau = fr(), fr()
g1, g2 = (1 + gamma) % R, gamma * gamma % R

# ---- leaves
iota = u32(np.arange(N))
out_fused, out_comp = Z.Vec.alloc(ctx, NCIRC * N), Z.Vec.alloc(ctx, NCIRC * N)


def leaves_fused():
    Z.timestamp_range_leaves(ctx, t_read, rc_rt, rc_gmr, fc_rt, fc_gmr, gamma, tau, out_fused)


def leaves_composed():
    leaf = lambda c, cols, coeffs, const: Z.fingerprint_leaves(ctx, cols, coeffs, [], [], const % R, "plain", 0, out_comp, offset=c * N, n=N)
    for s in range(NS):
        leaf(4 * s, [t_read[s], rc_rt[s]], [g1, g2], -tau)
        leaf(4 * s + 1, [t_read[s], rc_rt[s]], [g1, g2], g2 - tau)
        leaf(4 * s + 2, [iota, t_read[s], rc_gmr[s]], [g1, (-g1) % R, g2], -tau)
        leaf(4 * s + 3, [iota, t_read[s], rc_gmr[s]], [g1, (-g1) % R, g2], g2 - tau)
        leaf(4 * NS + 1 + 2 * s, [iota, fc_rt[s]], [g1, g2], -tau)
        leaf(4 * NS + 2 + 2 * s, [iota, fc_gmr[s]], [g1, g2], -tau)
    leaf(4 * NS, [iota], [g1], -tau)
    ctx.synchronize()


ms, _ = ab({"fused": leaves_fused, "composition": leaves_composed})
leaves_equal = bool(np.array_equal(out_fused.to_numpy(), out_comp.to_numpy()))
assert leaves_equal, "the fused leaves differ from the composition"
leaf_bytes = NCOLS * 4 * N + NCIRC * 32 * N  # every column in once, every circuit out once
res = {"what": "device calls of the timestamp range-check proof: fused leaves and compact-column openings, each against the composition it replaces",
       "log_n": args.log_n, "slots": NS, "circuits": NCIRC, "columns": NCOLS, "runs": args.runs, "warmup": args.warmup,
       "leaves": {"fused_ms": stats(ms["fused"], leaf_bytes), "composition_ms": stats(ms["composition"]), "composition_launches": NCIRC,
                  "composition_over_fused": round(statistics.median(ms["composition"]) / statistics.median(ms["fused"]), 3), "outputs_equal": leaves_equal,
                  "transient_bytes_fused": 8, "transient_bytes_composition": 4 * N}}
out_fused = out_comp = None

# ---- openings: the 20 columns in the proof's order, chi = eq(r_lo), the rho powers as coefficients
cols = rc_rt + rc_gmr + fc_rt + fc_gmr + t_read
chi = Z.eq_evals(ctx, [fr() for _ in range(args.log_n)])
rho = fr()
coeffs = [pow(rho, i, R) for i in range(NCOLS)]


def fr_copy(col):
    v = Z.Vec.alloc(ctx, N)
    Z.fingerprint_leaves(ctx, [col], [1], [], [], 0, "plain", 0, v, n=N)
    return Z.Rep3DensePolynomial.from_vec_shares(ctx, v)


polys = [fr_copy(c) for c in cols]
ctx.synchronize()


ev = lambda: Z.compact_batch_evaluate_at_chi(ctx, cols, chi, raw=True).tobytes()
ms, outs = ab({"compact": ev, "fr": lambda: Z.Rep3DensePolynomial.batch_evaluate_at_chi(polys, chi)})
assert Z.mont_limbs_to_int(np.frombuffer(outs["compact"], dtype=np.uint64).reshape(-1, 4)) == outs["fr"]
eval_bytes, eval_bytes_fr = 32 * N + 4 * N * NCOLS, 32 * N + 32 * N * NCOLS
res["evaluate_at_chi"] = {"compact_ms": stats(ms["compact"], eval_bytes), "fr_polynomials_ms": stats(ms["fr"], eval_bytes_fr), "outputs_equal": True,
                          "fr_over_compact": round(statistics.median(ms["fr"]) / statistics.median(ms["compact"]), 3),
                          "includes": "the finishing kernel and the fetch of the k results, in both variants"}

ms, outs = ab({"compact": lambda: Z.compact_linear_combination(ctx, cols, coeffs), "fr": lambda: Z.Rep3DensePolynomial.linear_combination(polys, coeffs)})
lin_equal = bool(np.array_equal(outs["compact"].to_numpy(), outs["fr"].copy_share_a().to_numpy()))
assert lin_equal, "the compact linear combination differs from the Fr call"
lin_bytes, lin_bytes_fr = 4 * N * NCOLS + 32 * N, 32 * N * NCOLS + 32 * N
res["linear_combination"] = {"compact_ms": stats(ms["compact"], lin_bytes), "fr_polynomials_ms": stats(ms["fr"], lin_bytes_fr), "outputs_equal": lin_equal,
                             "fr_over_compact": round(statistics.median(ms["fr"]) / statistics.median(ms["compact"]), 3)}
res["column_bytes"] = {"compact": 4 * N * NCOLS, "fr_copies_avoided": 32 * N * NCOLS}

# ---- the whole proof, per phase, fused leaves against the composition
cols = polys = chi = None
handles = {name: Z.TsProof(log_n=args.log_n, log_mem=args.log_n, seed=args.seed, leaves_fused=fused) for name, fused in (("fused", True), ("composition", False))}
phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_open_ms")
pm = {name: {ph: [] for ph in phases} for name in handles}
digest = {}
for it in range(args.warmup + args.runs):
    for name, hd in handles.items():
        r = hd.prove(verify=(it == 0))
        assert it > 0 or r.verified == 1, hd.last_error()
        assert digest.setdefault(name, bytes(r.proof_digest)) == bytes(r.proof_digest)
        if it >= args.warmup:
            for ph in phases:
                pm[name][ph].append(getattr(r, ph))
assert digest["fused"] == digest["composition"], "the two leaves paths give different proofs"
res["prove"] = {name: dict({ph: stats(pm[name][ph]) for ph in phases}, t_witness_ms_of_create=round(hd.prove(verify=False).t_witness_ms, 3)) for name, hd in handles.items()}
res["prove"].update({"verified": True, "digests_equal": True, "proof_bytes": int(handles["fused"].prove(verify=False).proof_len), "log_mem": args.log_n,
                     "clock": "host clock around each phase of the worker; every phase ends in a device synchronise or a host exchange"})
for hd in handles.values():
    hd.close()

if args.kernel_stats:
    names = ("k_ts_range_leaves", "k_compact_", "k_fingerprint_leaves", "k_poly_eval_chi", "k_poly_lincomb", "k_finish_sums")
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if any(n in r.get("Name", "") for n in names)]
    res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_ts_proof.py, a run of its own: avg_ms is one launch"}
    res["kernels"].update({r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                                     "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)} for r in rows})
else:
    res["kernels"] = "not measured"
res["bench_py_gpus1_steps3_warmup1"] = json.load(open(args.bench)) if args.bench else "not measured"
print(json.dumps(res), flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
