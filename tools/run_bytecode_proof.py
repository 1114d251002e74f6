"""Time the bytecode proof and its device calls at 2^log_n steps over tables of 2^b rows for every b in --log-b, in one process, the
variants of each comparison alternating, outputs compared equal at the measured size:
  leaves    cozk_bytecode_leaves + cozk_bytecode_init_final_leaves (two launches, four circuits) against the four
            cozk_fingerprint_leaves calls of the chained flow's phase 2 with a materialised iota column; both sides end in one context
            synchronise
  launch    each of the two fused calls alone, device events around the launch, with its byte floor
  witness   cozk_bytecode_witness (the counters' launches and the gather), a host clock around the call, which returns after the
            device has finished
  prove     the whole proof (cozk_bytecode_proof_*, seed --seed) with fused leaves and with the composition: two handles per table size
            alternating, each verified once, digests of the two leaves paths compared: wall and per phase (commit, leaves, grand
            products, open; a host clock around work that ends in a synchronise or a host exchange), and the witness time of create
  --flow-ab the chained flow's t_bytecode_ms (and wall) with COZK_BYTECODE_FUSED at 0 and 1, alternating on one harness of bench.py's
            shape at --flow-log-n, in plain and rep3 mode, digests compared
The table and the trace are Jolt-shaped (address U64, bitflags U64, rd / rs1 / rs2 U8, imm I64 about half negative; a walk with a
jump every eighth step, the last eighth padding at row 0); the read columns come from cozk_bytecode_witness and stay on the device; imm
is a PLAIN polynomial.  --warmup runs, then the median and spread of --runs runs.  The byte floors are the algorithmic bytes below over
the HBM rates of the MI355X (8.0 TB/s datasheet, 6.29 TB/s measured copy).  Prints one JSON line.
  python tools/run_bytecode_proof.py --log-n 20 --log-b 16 20 --runs 7 --flow-ab [--out profiles/bytecode_proof_2p20.json]"""
import argparse, ctypes, importlib, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--log-b", type=int, nargs="+", default=[16, 20])
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--flow-ab", action="store_true")
ap.add_argument("--skip-prove", action="store_true")
ap.add_argument("--flow-log-n", type=int, default=18)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = 1 << args.log_n
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
    d = {"runs": [round(x, 4) for x in xs], "median": round(med, 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
         "spread_pct_of_median": round(100 * (max(xs) - min(xs)) / med, 1)}
    if alg_bytes:
        d.update({"algorithmic_bytes": alg_bytes, "floor_ms_at_8.0_TBps": round(alg_bytes / HBM_SPEC * 1e3, 4), "floor_ms_at_6.29_TBps": round(alg_bytes / HBM_MEASURED * 1e3, 4),
                  "achieved_TBps": round(alg_bytes / med / 1e9, 3), "share_of_6.29_TBps": round(alg_bytes / med / 1e9 / 6.29, 3)})
    return d


def instance(rng, B):
    """the table and the trace, vectorised: a jump with probability 1/8 to a row in [1, B), else the next row, wrapping to 1"""
    table = [np.zeros(B, dtype=d) for d in (np.uint64, np.uint64, np.uint8, np.uint8, np.uint8, np.int64)]
    rows = np.arange(1, B, dtype=np.uint64)
    table[0][1:] = 0x80000000 + 4 * rows
    table[1][1:] = rng.integers(0, 1 << 64, size=B - 1, dtype=np.uint64)
    for k in (2, 3, 4):
        table[k][1:] = rng.integers(0, 32, size=B - 1)
    table[5][1:] = rng.integers(-(1 << 63), 1 << 63, size=B - 1, dtype=np.int64)
    live = N - N // 8
    jump = rng.integers(0, 8, size=live) == 0
    jump[0] = True
    target = rng.integers(0, B - 1, size=live)
    target[0] = 0
    last = np.maximum.accumulate(np.where(jump, np.arange(live), 0))
    a = np.zeros(N, dtype=np.uint32)
    a[:live] = 1 + (target[last] + np.arange(live) - last) % (B - 1)
    return a, table


KINDS = (Z.SCALAR_U64, Z.SCALAR_U64, Z.SCALAR_U8, Z.SCALAR_U8, Z.SCALAR_U8, Z.SCALAR_I64)
rng = np.random.default_rng(args.seed)
sm = np.random.default_rng(args.seed + 1)
fr = lambda: int.from_bytes(sm.bytes(40), "little") % R
gamma, tau = fr(), fr()
pw = [pow(gamma, k, R) for k in range(8)]
res = {"what": "the bytecode proof: fused leaves against the composition, each fused call alone, the witness call, the prove per phase, the flow's phase 2 behind its switch",
       "log_n": args.log_n, "runs": args.runs, "warmup": args.warmup, "tables": {}}

for log_b in args.log_b:
    B = 1 << log_b
    a, table = instance(rng, B)
    d_a = Z.Vec.from_numpy(ctx, a, Z.SCALAR_U32)
    d_table = [Z.Vec.from_numpy(ctx, c, k) for c, k in zip(table, KINDS)]
    wall = []
    for it in range(args.warmup + args.runs):
        ctx.synchronize()
        t0 = time.perf_counter()
        v_read, v_imm, t_read, t_final = Z.bytecode_witness(ctx, d_a, d_table)
        if it >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    imm = Z.Rep3DensePolynomial.from_vec_shares(ctx, v_imm)
    imm_u64 = Z.Vec.from_numpy(ctx, table[5].view(np.uint64), Z.SCALAR_U64)  # the composition takes no I64 column: the same bits as U64
    table_u = d_table[:5] + [imm_u64]
    iota = Z.Vec.from_numpy(ctx, np.arange(B, dtype=np.uint32), Z.SCALAR_U32)
    rw_fused, rw_comp = Z.Vec.alloc(ctx, 2 * N), Z.Vec.alloc(ctx, 2 * N)
    if_fused, if_comp = Z.Vec.alloc(ctx, 2 * B), Z.Vec.alloc(ctx, 2 * B)
    read_cols = [d_a] + v_read + [t_read]

    def leaves_fused():
        Z.bytecode_leaves(ctx, d_a, v_read, t_read, imm, gamma, tau, "plain", 0, rw_fused)
        Z.bytecode_init_final_leaves(ctx, table_u, t_final, gamma, tau, "plain", 0, if_fused)
        ctx.synchronize()

    def leaves_composed():  # flow_bytecode_worker's four launches
        Z.fingerprint_leaves(ctx, read_cols, pw[1:8], [imm], [1], -tau % R, "plain", 0, rw_comp, offset=0, n=N)
        Z.fingerprint_leaves(ctx, read_cols, pw[1:8], [imm], [1], (pw[7] - tau) % R, "plain", 0, rw_comp, offset=N, n=N)
        Z.fingerprint_leaves(ctx, [iota] + table_u, pw[1:7] + [1], [], [], -tau % R, "plain", 0, if_comp, offset=0, n=B)
        Z.fingerprint_leaves(ctx, [iota] + table_u + [t_final], pw[1:7] + [1, pw[7]], [], [], -tau % R, "plain", 0, if_comp, offset=B, n=B)
        ctx.synchronize()

    ms = ab({"fused": leaves_fused, "composition": leaves_composed})
    equal = bool(np.array_equal(rw_fused.to_numpy(), rw_comp.to_numpy()) and np.array_equal(if_fused.to_numpy(), if_comp.to_numpy()))
    assert equal, "the fused leaves differ from the composition"
    rw_bytes = (4 + 8 + 8 + 3 * 1 + 4 + 32) * N + 2 * 32 * N  # a, address, bitflags, rd / rs1 / rs2, t_read, imm in once; both circuits out once
    if_bytes = (8 + 8 + 3 * 1 + 8 + 4) * B + 2 * 32 * B       # the six table columns and t_final in once; both circuits out once
    f, c = statistics.median(ms["fused"]), statistics.median(ms["composition"])
    entry = {"log_b": log_b,
             "leaves": {"fused_ms": stats(ms["fused"], rw_bytes + if_bytes), "composition_ms": stats(ms["composition"]), "composition_launches": 4, "fused_launches": 2,
                        "composition_over_fused": round(c / f, 3), "outputs_equal": equal, "includes": "one context synchronise on either side",
                        "fused_beats_composition_by_more_than_the_spread": bool(max(ms["fused"]) < min(ms["composition"])),
                        "transient_bytes_fused": 0, "transient_bytes_composition": 4 * B}}
    ms = ab({"rw": lambda: Z.bytecode_leaves(ctx, d_a, v_read, t_read, imm, gamma, tau, "plain", 0, rw_fused),
             "init_final": lambda: Z.bytecode_init_final_leaves(ctx, table_u, t_final, gamma, tau, "plain", 0, if_fused),
             "init_final_i64": lambda: Z.bytecode_init_final_leaves(ctx, d_table, t_final, gamma, tau, "plain", 0, if_fused)})
    entry["launch_alone"] = {"bytecode_leaves_ms": stats(ms["rw"], rw_bytes), "bytecode_init_final_leaves_ms": stats(ms["init_final"], if_bytes),
                             "bytecode_init_final_leaves_i64_imm_ms": stats(ms["init_final_i64"], if_bytes)}
    entry["witness_ms"] = dict(stats(wall), clock="host clock around the call, which returns after the device has finished",
                               passes=1 if B <= 65536 else 2)
    res["tables"]["2p%d" % log_b] = entry
    rw_fused = rw_comp = if_fused = if_comp = imm = imm_u64 = iota = v_read = v_imm = t_read = t_final = d_a = d_table = table_u = read_cols = None

# ---- the whole proof, per phase: fused leaves against the composition
if args.skip_prove:
    res["prove"] = "not measured"
else:
    res["prove"] = {"clock": "host clock around each phase of the worker; every phase ends in a device synchronise or a host exchange; t_open_ms is the two openings plus reduce_and_prove"}
    phases = ("wall_ms", "t_commit_ms", "t_leaves_ms", "t_gp_ms", "t_open_ms")
    for log_b in args.log_b:
        handles = {lv: Z.BytecodeProof(log_n=args.log_n, log_b=log_b, seed=args.seed, leaves_fused=(lv == "fused")) for lv in ("fused", "composition")}
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
        res["prove"]["2p%d" % log_b] = {lv: dict({ph: stats(pm[lv][ph]) for ph in phases}, t_witness_ms_of_create=round(last[lv].t_witness_ms, 3), proof_bytes=int(last[lv].proof_len))
                                         for lv in handles}
        res["prove"]["2p%d" % log_b].update(verified=True, digests_equal=True)
        for hd in handles.values():
            hd.close()

if args.flow_ab:
    FL = importlib.import_module("co-zkvms_amd.flow")
    ln = args.flow_log_n
    res["flow_ab"] = {"log_n": ln, "shape": "bench.py's: log_m min(16, log_n), log_b min(14, log_n), log_mem min(17, log_n), 54 memories, 26 subtables"}
    for mode in ("plain", "rep3"):
        h = FL.FlowHarness(mode=mode, log_n=ln, log_m=min(16, ln), log_b=min(14, ln), log_mem=min(17, ln), n_mem=54, n_subtables=26, seed=args.seed)
        legs = {"0": dict(bytecode=[], wall=[]), "1": dict(bytecode=[], wall=[])}
        digest = {}
        for it in range(args.warmup + args.runs):
            for sw, leg in legs.items():
                os.environ["COZK_BYTECODE_FUSED"] = sw
                r = h.prove(verify=(it == 0))
                assert it > 0 or r.verified == 1, h.last_error()
                assert digest.setdefault(sw, bytes(r.proof_digest)) == bytes(r.proof_digest)
                if it >= args.warmup:
                    leg["bytecode"].append(r.t_bytecode_ms)
                    leg["wall"].append(r.wall_ms)
        os.environ.pop("COZK_BYTECODE_FUSED", None)
        assert digest["0"] == digest["1"], "the switch changes the proof"
        h.close()
        res["flow_ab"][mode] = {"switch_%s" % sw: {"t_bytecode_ms": stats(leg["bytecode"]), "wall_ms": stats(leg["wall"])} for sw, leg in legs.items()}
        res["flow_ab"][mode]["digests_equal"] = True
else:
    res["flow_ab"] = "not measured"
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
