"""Time cozk_lasso_witness (read_cts / E / final_cts of every memory of the instruction lookups) at Jolt's shape on the flow's own
trace, beside a plain host loop of the same walk (tools/lasso_witness_host.cpp, one thread per memory, at most 16 at a time), and
print one JSON line.  Device events on the context's stream around the call; warm-up, then the median and spread of --runs runs.
  python tools/run_lasso_witness.py --log-n 20 [--n-mem 54] [--n-subtables 26] [--runs 7] [--out profiles/lasso_witness_2p20.json]
  python tools/run_lasso_witness.py --make-inputs --log-n 20     (CPU only: generate and cache the trace's addresses and flags)
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/run_lasso_witness.py --no-host ..., in a run of its own
(k_lasso_rank / k_lasso_scan / k_lasso_finish; merge them with --kernel-stats <the stats csv>)."""
import argparse, csv, ctypes, importlib, json, os, statistics, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--n-mem", type=int, default=54)
ap.add_argument("--n-subtables", type=int, default=26)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--make-inputs", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--cache-dir", default=os.path.join(ROOT, "bench_out"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, M = 1 << args.log_n, 1 << 16
cache = os.path.join(args.cache_dir, "lasso_inputs_2p%d_m%d_s%d.npz" % (args.log_n, args.n_mem, args.seed))


def make_inputs():
    """the four query-chunk columns and the memory flags of the flow's synthetic trace (csrc/host/jolt_r1cs.hpp, restated by
    oracle/pyjolt_r1cs.py; memory m is live where the step's instruction uses it, oracle/pylookups.py instr_table)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyjolt_r1cs as J
    import pylookups as PL
    r1 = J.synthetic_columns(args.seed, N)
    dims = np.array([r1[J.IDX["ChunksQuery%d" % i]] for i in range(4)], dtype=np.uint32)
    instrs = PL.instr_table(args.n_mem)
    iflags = np.array([r1[J.IDX["I_" + nm]] for nm in J.INSTRUCTIONS], dtype=np.uint8)
    flags = np.zeros((args.n_mem, N), dtype=np.uint8)
    for i, ins in enumerate(instrs):
        for m in set(ins.mems):
            flags[m] |= iflags[i]
    os.makedirs(args.cache_dir, exist_ok=True)
    np.savez_compressed(cache, dims=dims, flags=np.packbits(flags, axis=1))
    return dims, flags


if os.path.exists(cache):
    z = np.load(cache)
    dims, flags = z["dims"], np.unpackbits(z["flags"], axis=1)[:, :N]
else:
    dims, flags = make_inputs()
if args.make_inputs:
    print("inputs: %s, flag density %.3f" % (cache, float(flags.mean())))
    sys.exit(0)
flags = np.ascontiguousarray(flags)
rng = np.random.default_rng(args.seed)
subs = rng.integers(0, 1 << 32, size=(args.n_subtables, M), dtype=np.uint64).astype(np.uint32)
mem_dim = [m % 4 for m in range(args.n_mem)]
mem_sub = [m % args.n_subtables for m in range(args.n_mem)]

import torch
Z = importlib.import_module("co-zkvms_amd")
LS = importlib.import_module("co-zkvms_amd.lasso")
ctx = Z.Context(0)
sp = ctypes.c_void_p()
ctx.check(ctx._l.cozk_ctx_stream(ctx.h, ctypes.byref(sp)))
stream = torch.cuda.ExternalStream(sp.value)
d = [Z.Vec.from_numpy(ctx, dims[i], Z.SCALAR_U32) for i in range(4)]
s = [Z.Vec.from_numpy(ctx, subs[i], Z.SCALAR_U32) for i in range(args.n_subtables)]
f = [Z.Vec.from_numpy(ctx, flags[m], Z.SCALAR_U8) for m in range(args.n_mem)]
dev_ms, out = [], None
for it in range(args.warmup + args.runs):
    out = None  # the previous outputs go back to the context's pool
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = LS.lasso_witness(ctx, d, s, f, mem_dim, mem_sub)
    e1.record(stream)
    e1.synchronize()
    if it >= args.warmup:
        dev_ms.append(e0.elapsed_time(e1))

tiles = (N + LS.LASSO_TILE - 1) // LS.LASSO_TILE
on = int(flags.sum())
# algorithmic bytes: per step and memory a flag byte in, read_cts and E out (8 B), + per flagged step its address in (4 B) and the
# subtable entry (4 B); per memory final_cts out (4 M).  The in-tile rank and the tile tables are the method's, not the problem's.
alg_bytes = args.n_mem * N * 9 + on * 8 + args.n_mem * M * 4
transient_per_mem = tiles * M * 6
batch = max(1, min(args.n_mem, (256 << 20) // transient_per_mem))
res = {"what": "cozk_lasso_witness: read_cts / E / final_cts of every memory on the flow's synthetic trace", "log_n": args.log_n, "M": M, "memories": args.n_mem,
       "dims": 4, "subtables": args.n_subtables, "flag_density": round(float(flags.mean()), 4), "tile_steps": LS.LASSO_TILE, "tiles": tiles,
       "memories_per_batch": batch, "transient_bytes": batch * transient_per_mem, "algorithmic_bytes": alg_bytes,
       "device_ms": {"runs": [round(x, 3) for x in dev_ms], "median": round(statistics.median(dev_ms), 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3)},
       "achieved_GBps_vs_algorithmic_bytes": round(alg_bytes / statistics.median(dev_ms) / 1e6, 1)}

if not args.no_host:
    so = os.path.join(args.cache_dir, "liblasso_witness_host.so")
    src = os.path.join(ROOT, "tools", "lasso_witness_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(args.cache_dir, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-pthread", src, "-o", so])
    hl = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    hl.lasso_witness_host.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp, vp, vp]
    hl.lasso_witness_host.restype = ctypes.c_int
    md, ms = np.array(mem_dim, dtype=np.int32), np.array(mem_sub, dtype=np.int32)
    hrc, hE, hfc = (np.empty((args.n_mem, n), dtype=np.uint32) for n in (N, N, M))
    host_ms = []
    for it in range(1 + args.runs):
        t0 = time.perf_counter()
        bad = hl.lasso_witness_host(dims.ctypes.data, N, subs.ctypes.data, M, flags.ctypes.data, md.ctypes.data, ms.ctypes.data, args.n_mem, args.threads,
                                    hrc.ctypes.data, hE.ctypes.data, hfc.ctypes.data)
        if it >= 1:
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert bad == 0
    for m in range(args.n_mem):  # the device's vectors are the host loop's, bit for bit, at the measured size
        assert np.array_equal(out[0][m].to_numpy(), hrc[m]) and np.array_equal(out[1][m].to_numpy(), hE[m]) and np.array_equal(out[2][m].to_numpy(), hfc[m]), m
    res["host_loop_ms"] = {"threads": args.threads, "runs": [round(x, 2) for x in host_ms], "median": round(statistics.median(host_ms), 2), "min": round(min(host_ms), 2),
                           "max": round(max(host_ms), 2)}
    res["device_equals_host_loop"] = True

if args.kernel_stats:
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "k_lasso" in r.get("Name", "")]
    res["kernels"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                               "avg_ms": round(float(r["AverageNs"]) / 1e6, 3)} for r in rows}
line = json.dumps(res)
print(line, flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
