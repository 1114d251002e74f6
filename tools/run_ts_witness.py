"""Time cozk_timestamp_range_witness (read_cts / final_cts of the read timestamps and of global time minus the read timestamp, 4 slots
over an identity table as long as the trace) on the flow's own trace: t_read comes from cozk_rw_memory_witness on the cached inputs
of tools/run_rw_witness.py (made by its --make-inputs if they are missing), stays on the device, and goes into the call as it is.
Beside it the plain host loop of the same walk (tools/ts_witness_host.cpp, one thread); the outputs are compared for equality at the
measured size.  Device events on the context's stream around the call; warm-up, then the median and spread of --runs runs.  Prints
one JSON line.
  python tools/run_ts_witness.py --log-n 20 [--runs 7] [--out profiles/ts_range_witness_2p20.json]
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/run_ts_witness.py --no-host ..., in a run of its own
(the k_ts_* kernels; merge them with --kernel-stats <the stats csv>).  --bench <file> adds recorded bench.py lines
(a JSON object {"this_change": {...}, "parent": {...}}) to the written profile."""
import argparse, csv, ctypes, importlib, json, os, statistics, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--log-mem", type=int, default=20)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--bench", default=None)
ap.add_argument("--cache-dir", default=os.path.join(ROOT, "bench_out"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, MEM, NS = 1 << args.log_n, 1 << args.log_mem, 4
M = N  # the identity table is as long as the trace
cache = os.path.join(args.cache_dir, "rw_inputs_2p%d_s%d.npz" % (args.log_n, args.seed))
if not os.path.exists(cache):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "run_rw_witness.py"), "--make-inputs", "--log-n", str(args.log_n), "--log-mem", str(args.log_mem),
                           "--seed", str(args.seed), "--cache-dir", args.cache_dir])
z = dict(np.load(cache))
addr, store = np.ascontiguousarray(z["addr"] & np.uint32(MEM - 1)), np.ascontiguousarray(z["store"])
v_write = [None, None, np.ascontiguousarray(z["rd_write"]), np.ascontiguousarray(z["ram_write"])]
is_write = [None, None, None, store]
v_init = np.random.default_rng(args.seed).integers(0, 1 << 32, size=MEM, dtype=np.uint64).astype(np.uint32)

import torch
Z = importlib.import_module("co-zkvms_amd")
ctx = Z.Context(0)
sp = ctypes.c_void_p()
ctx.check(ctx._l.cozk_ctx_stream(ctx.h, ctypes.byref(sp)))
stream = torch.cuda.ExternalStream(sp.value)
d_addr = [Z.Vec.from_numpy(ctx, addr[s].astype(np.uint8), Z.SCALAR_U8) if int(addr[s].max()) < 256 else Z.Vec.from_numpy(ctx, addr[s], Z.SCALAR_U32) for s in range(NS)]
d_vw = [None if v is None else Z.Vec.from_numpy(ctx, v, Z.SCALAR_U32) for v in v_write]
d_iw = [None if v is None else Z.Vec.from_numpy(ctx, v, Z.SCALAR_U8) for v in is_write]
t_read = Z.rw_memory_witness(ctx, d_addr, d_vw, d_iw, Z.Vec.from_numpy(ctx, v_init, Z.SCALAR_U32))[1]
dev_ms, out = [], None
for it in range(args.warmup + args.runs):
    out = None  # the previous outputs go back to the context's pool
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = Z.timestamp_range_witness(ctx, t_read, M)
    e1.record(stream)
    e1.synchronize()
    if it >= args.warmup:
        dev_ms.append(e0.elapsed_time(e1))

h_t_read = [np.ascontiguousarray(v.to_numpy()) for v in t_read]
cols = 2 * NS
tile = Z.lasso.LASSO_TILE
tiles = (N + tile - 1) // tile
passes = 2 if M > 65536 else 1
D = max(min(M, 65536), (M + 65535) // 65536 if passes == 2 else 0)
D += D & 1
batch = max(1, min(cols, (256 << 20) // (6 * tiles * D)))
# algorithmic bytes: per slot t_read in once, two read_cts columns and two final_cts columns out.  The sort is the method's.
alg_bytes = NS * (4 * N + 2 * 4 * N + 2 * 4 * M)
transient = batch * (6 * tiles * D + 2 * N + ((4 * D + 12 * N) if passes == 2 else 0))
res = {"what": "cozk_timestamp_range_witness: read_cts / final_cts of t_read and of j - t_read, t_read made by cozk_rw_memory_witness on the flow's synthetic trace",
       "log_n": args.log_n, "slots": NS, "columns": cols, "M": M, "MEM": MEM, "sort_passes": passes, "tile_steps": tile, "tiles": tiles, "columns_per_batch": batch,
       "distinct_keys": {"read_timestamp": [int(len(np.unique(t))) for t in h_t_read],
                         "global_minus_read": [int(len(np.unique(np.arange(N, dtype=np.uint32) - t))) for t in h_t_read]},
       "transient_bytes": transient, "algorithmic_bytes": alg_bytes,
       "device_ms": {"runs": [round(x, 3) for x in dev_ms], "median": round(statistics.median(dev_ms), 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3)},
       "achieved_GBps_vs_algorithmic_bytes": round(alg_bytes / statistics.median(dev_ms) / 1e6, 1)}

if not args.no_host:
    so = os.path.join(args.cache_dir, "libts_witness_host.so")
    src = os.path.join(ROOT, "tools", "ts_witness_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(args.cache_dir, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", src, "-o", so])
    hl = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    hl.ts_witness_host.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp, vp, vp, vp]
    hl.ts_witness_host.restype = ctypes.c_size_t
    ptrs = lambda arrs: (vp * NS)(*[a.ctypes.data for a in arrs])
    h_out = [[np.empty(N if k < 2 else M, dtype=np.uint32) for _ in range(NS)] for k in range(4)]
    host_ms = []
    for it in range(1 + args.runs):
        t0 = time.perf_counter()
        bad = hl.ts_witness_host(ptrs(h_t_read), NS, N, M, *[ptrs(g) for g in h_out])
        if it >= 1:
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert bad == 0
    for k in range(4):  # the device's vectors are the host loop's, bit for bit, at the measured size
        for s in range(NS):
            assert np.array_equal(out[k][s].to_numpy(), h_out[k][s]), (k, s)
    res["host_loop_ms"] = {"threads": 1, "runs": [round(x, 2) for x in host_ms], "median": round(statistics.median(host_ms), 2), "min": round(min(host_ms), 2),
                           "max": round(max(host_ms), 2)}
    res["host_loop_over_device"] = round(statistics.median(host_ms) / statistics.median(dev_ms), 1)
    res["device_equals_host_loop"] = True

if args.kernel_stats:
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "k_ts_" in r.get("Name", "")]
    res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_ts_witness.py --no-host, a run of its own: "
                                "avg_ms is one launch, total_ms all launches of all of that run's calls"}
    res["kernels"].update({r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                                     "avg_ms": round(float(r["AverageNs"]) / 1e6, 3)} for r in rows})
if args.bench:
    res["bench_py_gpus1_steps3_warmup1"] = json.load(open(args.bench))
line = json.dumps(res)
print(line, flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
