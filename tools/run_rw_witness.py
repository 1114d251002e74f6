"""Time cozk_rw_memory_witness (v_read / t_read / v_written / v_final / t_final of the register + RAM memory) at Jolt's shape on the
flow's own trace -- slots rs1, rs2, rd, ram; the register indices and the 20-bit RAM address into ONE memory of 2^20 words; rd writes
at every step, ram where the store flag is set -- beside the plain host loop of the same walk (tools/rw_witness_host.cpp, one thread:
the walk cannot be split), and print one JSON line.  Device events on the context's stream around the call; warm-up, then the median
and spread of --runs runs.  The trace's columns are synthetic (they satisfy the R1CS, they are no program's execution): the walk is
the same whatever the values, and the outputs are compared with the host loop's for equality.
  python tools/run_rw_witness.py --log-n 20 [--runs 7] [--out profiles/rw_witness_2p20.json]
  python tools/run_rw_witness.py --make-inputs --log-n 20     (CPU only: generate and cache the trace's addresses, values and flags)
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/run_rw_witness.py --no-host ..., in a run of its own
(the k_rw_* kernels; merge them with --kernel-stats <the stats csv>)."""
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
ap.add_argument("--make-inputs", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--cache-dir", default=os.path.join(ROOT, "bench_out"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, MEM, NS = 1 << args.log_n, 1 << args.log_mem, 4
cache = os.path.join(args.cache_dir, "rw_inputs_2p%d_s%d.npz" % (args.log_n, args.seed))
SLOTS = ["Bytecode_RS1", "Bytecode_RS2", "Bytecode_RD", "RAM_Address"]


def make_inputs():
    """the register and RAM address columns, the written values and the store flag of the flow's synthetic trace
    (csrc/host/jolt_r1cs.hpp, restated by oracle/pyjolt_r1cs.py)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyjolt_r1cs as J
    r1 = J.synthetic_columns(args.seed, N)
    col = lambda name: np.array([int(x) & 0xFFFFFFFF for x in r1[J.IDX[name]][:N]], dtype=np.uint32)
    z = dict(addr=np.array([col(nm) for nm in SLOTS]), rd_write=col("RD_Write"), ram_write=col("RAM_Write"), store=col("Op_Store").astype(np.uint8))
    os.makedirs(args.cache_dir, exist_ok=True)
    np.savez_compressed(cache, **z)
    return z


z = dict(np.load(cache)) if os.path.exists(cache) else make_inputs()
addr, store = np.ascontiguousarray(z["addr"] & np.uint32(MEM - 1)), np.ascontiguousarray(z["store"])
v_write = [None, None, np.ascontiguousarray(z["rd_write"]), np.ascontiguousarray(z["ram_write"])]
is_write = [None, None, None, store]
if args.make_inputs:
    print("inputs: %s, store density %.3f, distinct addresses %d" % (cache, float(store.mean()), len(np.unique(addr))))
    sys.exit(0)
v_init = np.random.default_rng(args.seed).integers(0, 1 << 32, size=MEM, dtype=np.uint64).astype(np.uint32)

import torch
Z = importlib.import_module("co-zkvms_amd")
RW = importlib.import_module("co-zkvms_amd.rw_memory")
LS = importlib.import_module("co-zkvms_amd.lasso")
ctx = Z.Context(0)
sp = ctypes.c_void_p()
ctx.check(ctx._l.cozk_ctx_stream(ctx.h, ctypes.byref(sp)))
stream = torch.cuda.ExternalStream(sp.value)
# the register columns are one byte wide, as the flow commits them
d_addr = [Z.Vec.from_numpy(ctx, addr[s].astype(np.uint8), Z.SCALAR_U8) if int(addr[s].max()) < 256 else Z.Vec.from_numpy(ctx, addr[s], Z.SCALAR_U32) for s in range(NS)]
d_vw = [None if v is None else Z.Vec.from_numpy(ctx, v, Z.SCALAR_U32) for v in v_write]
d_iw = [None if v is None else Z.Vec.from_numpy(ctx, v, Z.SCALAR_U8) for v in is_write]
d_init = Z.Vec.from_numpy(ctx, v_init, Z.SCALAR_U32)
dev_ms, out = [], None
for it in range(args.warmup + args.runs):
    out = None  # the previous outputs go back to the context's pool
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = RW.rw_memory_witness(ctx, d_addr, d_vw, d_iw, d_init)
    e1.record(stream)
    e1.synchronize()
    if it >= args.warmup:
        dev_ms.append(e0.elapsed_time(e1))

ops = N * NS
tile = LS.LASSO_TILE
tiles = (ops + tile - 1) // tile
passes = 2 if MEM > 65536 else 1
D = max(min(MEM, 65536), (MEM + 65535) // 65536 if passes == 2 else 0)
addr_bytes = sum(1 if int(addr[s].max()) < 256 else 4 for s in range(NS))
# algorithmic bytes: per step the addresses, the two written values and the store flag in, v_read and t_read of every slot and
# v_written of the flagged slot out; per word v_init in, v_final and t_final out.  The sort is the method's, not the problem's.
alg_bytes = N * (addr_bytes + 2 * 4 + 1 + NS * 8 + 4) + MEM * 12
transient = 4 * ops * passes + 2 * ops + 6 * tiles * D + 4 * D + 8 * ((ops + 4095) // 4096)
res = {"what": "cozk_rw_memory_witness: v_read / t_read / v_written / v_final / t_final of the register + RAM memory on the flow's synthetic trace",
       "log_n": args.log_n, "slots": NS, "operations": ops, "MEM": MEM, "sort_passes": passes, "store_density": round(float(store.mean()), 4),
       "distinct_addresses": int(len(np.unique(addr))), "address_kinds": ["U8" if int(addr[s].max()) < 256 else "U32" for s in range(NS)], "tile_operations": tile,
       "tiles": tiles, "transient_bytes": transient, "algorithmic_bytes": alg_bytes,
       "device_ms": {"runs": [round(x, 3) for x in dev_ms], "median": round(statistics.median(dev_ms), 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3)},
       "achieved_GBps_vs_algorithmic_bytes": round(alg_bytes / statistics.median(dev_ms) / 1e6, 1)}

if not args.no_host:
    so = os.path.join(args.cache_dir, "librw_witness_host.so")
    src = os.path.join(ROOT, "tools", "rw_witness_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(args.cache_dir, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", src, "-o", so])
    hl = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    hl.rw_witness_host.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp, vp, vp, vp]
    hl.rw_witness_host.restype = ctypes.c_size_t
    ptrs = lambda arrs: (vp * NS)(*[None if a is None else a.ctypes.data for a in arrs])
    h_vr, h_tr = [np.empty(N, dtype=np.uint32) for _ in range(NS)], [np.empty(N, dtype=np.uint32) for _ in range(NS)]
    h_vw = [None if f is None else np.empty(N, dtype=np.uint32) for f in is_write]
    h_vf, h_tf = np.empty(MEM, dtype=np.uint32), np.empty(MEM, dtype=np.uint32)
    host_ms = []
    for it in range(1 + args.runs):
        t0 = time.perf_counter()
        bad = hl.rw_witness_host(ptrs(list(addr)), ptrs(v_write), ptrs(is_write), NS, N, v_init.ctypes.data, MEM, ptrs(h_vr), ptrs(h_tr), ptrs(h_vw), h_vf.ctypes.data,
                                 h_tf.ctypes.data)
        if it >= 1:
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert bad == 0
    for s in range(NS):  # the device's vectors are the host loop's, bit for bit, at the measured size
        assert np.array_equal(out[0][s].to_numpy(), h_vr[s]) and np.array_equal(out[1][s].to_numpy(), h_tr[s]), s
        assert (out[2][s] is None) == (h_vw[s] is None) and (h_vw[s] is None or np.array_equal(out[2][s].to_numpy(), h_vw[s])), s
    assert np.array_equal(out[3].to_numpy(), h_vf) and np.array_equal(out[4].to_numpy(), h_tf)
    res["host_loop_ms"] = {"threads": 1, "runs": [round(x, 2) for x in host_ms], "median": round(statistics.median(host_ms), 2), "min": round(min(host_ms), 2),
                           "max": round(max(host_ms), 2)}
    res["device_equals_host_loop"] = True

if args.kernel_stats:
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "k_rw_" in r.get("Name", "")]
    res["kernels"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                               "avg_ms": round(float(r["AverageNs"]) / 1e6, 3)} for r in rows}
line = json.dumps(res)
print(line, flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
