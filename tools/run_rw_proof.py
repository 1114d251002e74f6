"""Time the read-write memory proof at 2^log_n steps over a memory of 2^log_mem words, 4 slots, in one process, the variants of each
comparison alternating, outputs compared equal at the measured size:
  leaves    cozk_rw_memory_leaves + cozk_rw_memory_init_final_leaves (two launches, 10 circuits) against the ten cozk_fingerprint_leaves
            calls of the chained flow's phase 4 with materialised iota columns; both sides end in one context synchronise
  launch    each of the two fused calls alone, device events around the launch (the product forms that were measured against the kept
            one and removed are recorded in the profile under *_not_kept; the tool measures the form that was kept)
  prove     the whole proof (cozk_rw_proof_*, seed --seed), fused leaves and composition, with_ts 1 and 0: four handles alternating, each
            verified once, digests of the two leaves paths compared: wall and per phase (commit, leaves, grand products, timestamp
            check, open; a host clock around work that ends in a synchronise or a host exchange), and the witness time of create
The columns of the leaves A/B come from cozk_rw_memory_witness over a Jolt-shaped trace (U8 register addresses, U32 ram addresses) and
stay on the device.  --warmup runs, then the median and spread of --runs runs.  The byte floors are the algorithmic bytes below over the
HBM rates of the MI355X (8.0 TB/s datasheet, 6.29 TB/s measured copy).  Prints one JSON line.
  python tools/run_rw_proof.py --log-n 20 --log-mem 20 --runs 7 [--out profiles/rw_proof_2p20.json]
Per-kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_rw_proof.py ..., in a run of its own; merge
with --kernel-stats <the stats csv>.  --bench <file> adds recorded bench.py lines ({"this_change": {...}, "parent": {...}}).
--rep3 measures the three-party form instead and prints its own JSON line (without the flag the output is unchanged): the shared fused
leaves against the composition in REP3 for a party of each kind, and the whole three-party prove with either leaves path (run_rep3):
  python tools/run_rw_proof.py --rep3 --log-n 20 --log-mem 20 --runs 7 [--out profiles/rw_proof_rep3_2p20.json]"""
import argparse, csv, ctypes, importlib, json, os, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--log-mem", type=int, default=20)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-prove", action="store_true")
ap.add_argument("--rep3", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--bench", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, MEM, NS = 1 << args.log_n, 1 << args.log_mem, 4
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
    """variants: {name: call}; alternating rounds -> {name: ms list}"""
    ms = {k: [] for k in variants}
    for it in range(args.warmup + args.runs):
        for name, call in variants.items():
            t, _ = timed(call)
            if it >= args.warmup:
                ms[name].append(t)
    return ms


def stats(xs, alg_bytes=None):
    med = statistics.median(xs)
    d = {"runs": [round(x, 4) for x in xs], "median": round(med, 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    if alg_bytes:
        d.update({"algorithmic_bytes": alg_bytes, "floor_ms_at_8.0_TBps": round(alg_bytes / HBM_SPEC * 1e3, 4), "floor_ms_at_6.29_TBps": round(alg_bytes / HBM_MEASURED * 1e3, 4),
                  "achieved_TBps": round(alg_bytes / med / 1e9, 3), "share_of_6.29_TBps": round(alg_bytes / med / 1e9 / 6.29, 3)})
    return d


rng = np.random.default_rng(args.seed)
u32 = lambda a: Z.Vec.from_numpy(ctx, np.ascontiguousarray(a, dtype=np.uint32), Z.SCALAR_U32)
u8 = lambda a: Z.Vec.from_numpy(ctx, np.ascontiguousarray(a, dtype=np.uint8), Z.SCALAR_U8)
r32 = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
addr = [u8(rng.integers(0, 32, size=N)) for _ in range(3)] + [u32(rng.integers(0, MEM, size=N))]
v_init = u32(r32(MEM))
rd_write = u32(r32(N))
v_read, t_read, v_written, v_final, t_final = Z.rw_memory_witness(ctx, addr, [None, None, rd_write, u32(r32(N))], [None, None, None, u8(rng.integers(0, 100, size=N) < 30)], v_init)
written = [None, None, rd_write, v_written[3]]
sm = np.random.default_rng(args.seed + 1)
fr = lambda: int.from_bytes(sm.bytes(40), "little") % R
gamma, tau = fr(), fr()
g2 = gamma * gamma % R


def run_rep3():
    """--rep3: the shared leaves (cozk_rw_memory_shared_leaves + cozk_rw_memory_shared_init_final_leaves) against the ten
    cozk_fingerprint_leaves calls they replace, in REP3 for one party of each kind (0: the public part in a, 1: in b, 2: none), the two
    paths alternating and their outputs compared; then the whole three-party prove (cozk_rw_proof_rep3_*) with either leaves path, two
    handles alternating, per phase (the maximum over the parties).  The address and timestamp columns are the witness's; the value
    polynomials are random share components of N (MEM) entries, v_init a public polynomial, as the harness passes them."""
    MODE_REP3 = Z._lib.MODE_REP3
    widen = lambda col: Z.Rep3DensePolynomial.from_vec_shares(ctx, Z.compact_linear_combination(ctx, [col], [1]))
    shared = lambda n, seed: Z.Rep3DensePolynomial.random(ctx, n, seed, MODE_REP3)
    p_read = [shared(N, 100 + s) for s in range(NS)]
    p_written = [None, None, shared(N, 200), shared(N, 201)]
    p_init, p_final = widen(v_init), shared(MEM, 300)
    iota_n, iota_mem = u32(np.arange(N)), u32(np.arange(MEM))
    outs = lambda n: [Z.Vec.alloc(ctx, n), Z.Vec.alloc(ctx, n)]
    rw_fused, rw_comp, if_fused, if_comp = outs(2 * NS * N), outs(2 * NS * N), outs(2 * MEM), outs(2 * MEM)
    out = {"what": "the read-write memory proof by three Rep3 parties: the shared fused leaves against the composition for a party of each kind, the three-party prove per phase",
           "log_n": args.log_n, "log_mem": args.log_mem, "slots": NS, "circuits": 2 * NS + 2, "runs": args.runs, "warmup": args.warmup, "leaves": {}, "launch_alone": {}}
    for party in (0, 1, 2):
        def fused_rw():
            Z.rw_memory_shared_leaves(ctx, addr, p_read, t_read, p_written, gamma, tau, "rep3", party, *rw_fused)

        def fused_if():
            Z.rw_memory_shared_init_final_leaves(ctx, p_init, p_final, t_final, gamma, tau, "rep3", party, *if_fused)

        def fused():
            fused_rw()
            fused_if()
            ctx.synchronize()

        def composed():
            leaf = lambda o, off, n, cols, coeffs, poly: Z.fingerprint_leaves(ctx, cols, coeffs, [poly], [gamma], -tau % R, "rep3", party, *o, offset=off, n=n)
            for s in range(NS):
                leaf(rw_comp, 2 * s * N, N, [t_read[s], addr[s]], [g2, 1], p_read[s])
                leaf(rw_comp, (2 * s + 1) * N, N, [iota_n, addr[s]], [g2, 1], p_read[s] if p_written[s] is None else p_written[s])
            leaf(if_comp, 0, MEM, [iota_mem], [1], p_init)
            leaf(if_comp, MEM, MEM, [t_final, iota_mem], [g2, 1], p_final)
            ctx.synchronize()

        ms = ab({"fused": fused, "composition": composed})
        equal = all(bool(np.array_equal(x.to_numpy(), y.to_numpy())) for x, y in zip(rw_fused + if_fused, rw_comp + if_comp))
        assert equal, "party %d: the fused shared leaves differ from the composition" % party
        # in: the public columns (a party that adds no public part reads none; only parties 0 and 1 read the public v_init), both
        # components of the 6 shared columns of N entries and of v_final; out: both components of every circuit
        pub = party < 2
        rw_bytes = ((3 * 1 + 1 * 4 + 4 * NS) * pub + 2 * 32 * (NS + 2)) * N + 2 * 2 * NS * 32 * N
        if_bytes = ((4 + 32) * pub + 2 * 32) * MEM + 2 * 2 * 32 * MEM
        # the composition: every launch reads its own columns (every party, the iota columns among them) and one polynomial, writes one circuit
        comp_bytes = (2 * (3 * 1 + 1 * 4) + (4 + 4) * NS + 2 * NS * 2 * 32 + 2 * NS * 2 * 32) * N + (4 + 4 + 4 + 32 * pub + 2 * 32 + 2 * 2 * 32) * MEM
        out["leaves"]["party_%d" % party] = {
            "fused_ms": stats(ms["fused"], rw_bytes + if_bytes), "composition_ms": stats(ms["composition"], comp_bytes),
            "composition_launches": 2 * NS + 2, "fused_launches": 2, "composition_over_fused": round(statistics.median(ms["composition"]) / statistics.median(ms["fused"]), 3),
            "outputs_equal": equal, "includes": "one context synchronise on either side"}
        ms = ab({"rw": fused_rw, "init_final": fused_if})
        out["launch_alone"]["party_%d" % party] = {"rw_memory_shared_leaves_ms": stats(ms["rw"], rw_bytes), "rw_memory_shared_init_final_leaves_ms": stats(ms["init_final"], if_bytes)}
    if args.skip_prove:
        out["prove"] = "not measured"
    else:
        rw_fused = rw_comp = if_fused = if_comp = p_read = p_written = p_init = p_final = None
        handles = {lv: Z.RwProofRep3(log_n=args.log_n, log_mem=args.log_mem, seed=args.seed, leaves_fused=(lv == "fused")) for lv in ("fused", "composition")}
        phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_open_ms")
        pm = {k: {ph: [] for ph in phases} for k in handles}
        digest, last = {}, {}
        for it in range(args.warmup + args.runs):
            for k, hd in handles.items():
                r = hd.prove(verify=(it == 0))
                assert it > 0 or r.verified == 1, hd.last_error()
                assert digest.setdefault(k, bytes(r.proof_digest)) == bytes(r.proof_digest)
                last[k] = r
                if it >= args.warmup:
                    for ph in phases:
                        pm[k][ph].append(getattr(r, ph))
        assert digest["fused"] == digest["composition"], "the two leaves paths give different proofs"
        plain = Z.RwProof(log_n=args.log_n, log_mem=args.log_mem, seed=args.seed, with_ts=False)
        plain_digest = bytes(plain.prove(verify=False).proof_digest)
        plain.close()
        assert plain_digest == digest["fused"], "the Rep3 proof differs from the plain proof of the same seed"
        out["prove"] = {lv: dict({ph: stats(pm[lv][ph]) for ph in phases}, t_witness_ms_of_create=round(last[lv].t_witness_ms, 3), t_share_ms_of_create=round(last[lv].t_share_ms, 3),
                                 ring_bytes=int(last[lv].ring_bytes), proof_bytes=int(last[lv].proof_len)) for lv in handles}
        out["prove"].update({"verified": True, "digests_equal": True, "equal_to_the_plain_proof": True, "parties": "three contexts on one device",
                             "clock": "host clock around each phase of a worker, the maximum over the three parties; t_open_ms is the two joint openings plus reduce_and_prove"})
        for hd in handles.values():
            hd.close()
    print(json.dumps(out), flush=True)
    if args.out:
        open(args.out, "w").write(json.dumps(out, indent=1) + "\n")


if args.rep3:
    run_rep3()
    sys.exit(0)

# ---- leaves: the two fused calls against the ten calls of the composition
iota_n, iota_mem = u32(np.arange(N)), u32(np.arange(MEM))
rw_fused, rw_comp = Z.Vec.alloc(ctx, 2 * NS * N), Z.Vec.alloc(ctx, 2 * NS * N)
if_fused, if_comp = Z.Vec.alloc(ctx, 2 * MEM), Z.Vec.alloc(ctx, 2 * MEM)


def leaves_fused():
    Z.rw_memory_leaves(ctx, addr, v_read, t_read, written, gamma, tau, rw_fused)
    Z.rw_memory_init_final_leaves(ctx, v_init, v_final, t_final, gamma, tau, if_fused)
    ctx.synchronize()


def leaves_composed():
    leaf = lambda out, off, n, cols, coeffs: Z.fingerprint_leaves(ctx, cols, coeffs, [], [], -tau % R, "plain", 0, out, offset=off, n=n)
    for s in range(NS):
        leaf(rw_comp, 2 * s * N, N, [v_read[s], t_read[s], addr[s]], [gamma, g2, 1])
        leaf(rw_comp, (2 * s + 1) * N, N, [v_read[s] if written[s] is None else written[s], iota_n, addr[s]], [gamma, g2, 1])
    leaf(if_comp, 0, MEM, [v_init, iota_mem], [gamma, 1])
    leaf(if_comp, MEM, MEM, [v_final, t_final, iota_mem], [gamma, g2, 1])
    ctx.synchronize()


ms = ab({"fused": leaves_fused, "composition": leaves_composed})
ref_rw, ref_if = rw_comp.to_numpy(), if_comp.to_numpy()
leaves_equal = bool(np.array_equal(rw_fused.to_numpy(), ref_rw) and np.array_equal(if_fused.to_numpy(), ref_if))
assert leaves_equal, "the fused leaves differ from the composition"
rw_bytes = (3 * 1 + 1 * 4 + 2 * 4 * NS + 2 * 4) * N + 2 * NS * 32 * N  # addresses, v_read and t_read, the two written columns in once; every circuit out once
if_bytes = 3 * 4 * MEM + 2 * 32 * MEM
res = {"what": "the read-write memory proof: fused leaves against the composition, each fused call alone, the prove per phase",
       "log_n": args.log_n, "log_mem": args.log_mem, "slots": NS, "circuits": 2 * NS + 2, "runs": args.runs, "warmup": args.warmup,
       "leaves": {"fused_ms": stats(ms["fused"], rw_bytes + if_bytes), "composition_ms": stats(ms["composition"]), "composition_launches": 2 * NS + 2,
                  "fused_launches": 2, "composition_over_fused": round(statistics.median(ms["composition"]) / statistics.median(ms["fused"]), 3),
                  "outputs_equal": leaves_equal, "includes": "one context synchronise on either side",
                  "transient_bytes_fused": 0, "transient_bytes_composition": 4 * N + 4 * MEM}}

# ---- each call alone, device events around the launch (no synchronise inside the clock)
ms = ab({"rw": lambda: Z.rw_memory_leaves(ctx, addr, v_read, t_read, written, gamma, tau, rw_fused),
         "init_final": lambda: Z.rw_memory_init_final_leaves(ctx, v_init, v_final, t_final, gamma, tau, if_fused)})
res["launch_alone"] = {"rw_memory_leaves_ms": stats(ms["rw"], rw_bytes), "rw_memory_init_final_leaves_ms": stats(ms["init_final"], if_bytes)}
rw_fused = rw_comp = if_fused = if_comp = ref_rw = ref_if = None
addr = v_read = t_read = v_written = written = v_final = t_final = v_init = iota_n = iota_mem = rd_write = None

# ---- the whole proof, per phase: fused leaves against the composition, with and without the timestamp check
if args.skip_prove:
    res["prove"] = "not measured"
else:
    handles = {(lv, ts): Z.RwProof(log_n=args.log_n, log_mem=args.log_mem, seed=args.seed, leaves_fused=(lv == "fused"), with_ts=bool(ts))
               for ts in (1, 0) for lv in ("fused", "composition")}
    phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_ts_ms", "t_open_ms")
    pm = {k: {ph: [] for ph in phases} for k in handles}
    digest = {}
    for it in range(args.warmup + args.runs):
        for k, hd in handles.items():
            r = hd.prove(verify=(it == 0))
            assert it > 0 or r.verified == 1, hd.last_error()
            assert digest.setdefault(k, bytes(r.proof_digest)) == bytes(r.proof_digest)
            if it >= args.warmup:
                for ph in phases:
                    pm[k][ph].append(getattr(r, ph))
    assert digest[("fused", 1)] == digest[("composition", 1)] and digest[("fused", 0)] == digest[("composition", 0)], "the two leaves paths give different proofs"
    res["prove"] = {"with_ts_%d" % ts: {lv: dict({ph: stats(pm[(lv, ts)][ph]) for ph in phases}, t_witness_ms_of_create=round(handles[(lv, ts)].prove(verify=False).t_witness_ms, 3),
                                             proof_bytes=int(handles[(lv, ts)].prove(verify=False).proof_len)) for lv in ("fused", "composition")} for ts in (1, 0)}
    res["prove"].update({"verified": True, "digests_equal": True,
                         "clock": "host clock around each phase of the worker; every phase ends in a device synchronise or a host exchange; t_open_ms is the two compact openings plus reduce_and_prove"})
    for hd in handles.values():
        hd.close()

if args.kernel_stats:
    knames = ("k_rw_leaves", "k_rw_if_leaves", "k_fingerprint_leaves", "k_ts_range_leaves", "k_compact_")
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if any(n in r.get("Name", "") for n in knames)]
    res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/run_rw_proof.py, a run of its own: avg_ms is one launch"}
    res["kernels"].update({r["Name"]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                       "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)} for r in rows})
else:
    res["kernels"] = "not measured"
res["bench_py_gpus1_steps3_warmup1"] = json.load(open(args.bench)) if args.bench else "not measured"
print(json.dumps(res), flush=True)
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
