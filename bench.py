#!/usr/bin/env python
"""bench.py -- RISC-V cycles proved / second on the sumcheck + polynomial-commitment hot path.

Workload (BASELINE.json configs[1], restated synthetically per SURVEY.md 8d): one 2^20-cycle trace,
plain prover on one MI355X, "kernels only": 128 committed polynomials (64 uniform-Fr, 32 u16, 16 u32,
16 0/1 flags; PST13 = BN254 multilinear KZG -- the reference has no Hyrax) -> batch MSM,
one dense grand product of 8 circuits x 2^21 leaves (construct + GKR prove), batch_evaluate + RLC of
all 128 polynomials at two points, the opening-reduction sumcheck and the PST13 opening (20 MSMs).
A "step" = one full pass over that trace with the witness and SRS already resident in HBM.
N > 1 (one process per GPU), `--shard worker` (default): ONE proof of a 2^20 * N-cycle trace sharded over the
N GPUs as worker sub-nets -- every polynomial chunked over its high variables (the reference's split_poly,
co-jolt/src/poly/dense_mlpoly.rs:275-301), the 8 grand-product circuits divided among the workers, the last
log2(N) sumcheck rounds / PST folds finished on the gathered finals; each GPU keeps 2^20 cycles of work (weak
scaling).  The only exchange step is the per-round star gather (a few hundred bytes per rank), carried as an
all-gather through libcozk's shared-memory hub with a replicated coordinator on every rank; there is no bulk
collective on this axis (RCCL carries the Rep3 ring of the party axis: tools/dist_prove.py).
`--shard segment`: N independent 2^20-cycle segments instead (no exchange at all).

Launch: `python bench.py --gpus N` starts its own N rank processes (fresh children, spawned before anything
touches the GPU; the parent only relays rank 0's JSON line and the exit codes); under torch.distributed.run
(RANK / LOCAL_RANK / WORLD_SIZE in the environment) the process IS one rank.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the headline; `--full` adds
the rest below.  `roofline` is for the dominant kernel (MSM bucket accumulation,
k_msm_accum0_f9), timed live with HIP events on the stream it is launched on; `roofline.kernels` holds the same
figures for the HBM-bound kernels of the polynomial seam; `cpu_baseline` is the oracle's plain-C restatement
(OpenMP, all host cores) on a bounded sample of the same workload, with the reference's own trace-derived
numbers beside it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec

# one mixed XYZZ addition in the gather kernel (csrc/fq9.hip.hpp madd9) = 6 products (2 x 81 mads each: limb products +
# Montgomery reduction) + 2 squarings (45 + 81) + Y3's two products under one reduction (81 + 81 + 81) = 1467 mads
# = 9.06 stand-alone products of 162 mads, which is what the measured multiplier peak counts
MADS_PER_MADD = 6 * 162 + 2 * 126 + 243
MADS_PER_MUL = 162


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log-n", type=int, default=20, help="log2 of the padded trace length (cycles)")
    ap.add_argument("--cpu-sample-log-n", type=int, default=18, help="trace length of the bounded CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--leaf-fingerprints", action="store_true",
                    help="compute the grand-product leaves as K11 fingerprints of committed columns (not available with --shard worker)")
    ap.add_argument("--lookups", action="store_true",
                    help="add SURVEY 8(f)1 to every step: Lasso's primary sumcheck over the 27 RV32I collations + the toggled / sparse grand "
                         "product of the instruction lookups (54 memories = 108 circuits, 10 %% flags) on the same 2^log_n-cycle trace (N = 1)")
    ap.add_argument("--outer", action="store_true",
                    help="add SURVEY 8(f)2 to every step: the whole co-jolt Spartan worker (outer + inner + shift sumchecks, two opening appends) on the "
                         "reference's constraint set (128 rows per step) over the same number of steps (N = 1)")
    ap.add_argument("--host-witness", action="store_true",
                    help="also time the H2D upload of a host-resident witness of the same size (pinned memory) and report the "
                         "PCIe-inclusive step beside `value` (which never includes PCIe)")
    ap.add_argument("--witness-scatter", action="store_true",
                    help="also time the device-to-device witness scatter (SURVEY 8(f)3): Rep3 shares of the 64 Fr polynomials for three "
                         "parties generated on the dealer's GPU and delivered into the parties' contexts (cozk_rep3_scatter)")
    ap.add_argument("--no-full-step", action="store_true",
                    help="skip the `full_step` leg (N = 1 only, outside the timed region): ONE chained co-jolt worker flow of the same trace "
                         "length -- commit-all (250 polynomials), bytecode / instruction-lookups / read-write-memory checking, Spartan, one "
                         "batched opening -- reported beside `value`, which stays SURVEY 8(d) config 2")
    ap.add_argument("--hub", choices=["shm", "gloo"], default="shm", help="transport of the per-round star messages (--shard worker)")
    ap.add_argument("--shard", choices=["worker", "segment"], default="worker",
                    help="N>1: one proof sharded as worker sub-nets (default) or N independent trace segments")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="no proving: ranks rendezvous, run the barrier / max-over-ranks / digest-gather plumbing and rank 0 prints a JSON "
                         "line (the CPU test of the self-launch path; needs no GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: per-kernel HIP-event timing in the timed steps and the "
                         "`roofline` block (with the multiplier micro-benchmark), the `full_step` leg and the `cpu_baseline` leg "
                         "(--no-full-step / --no-cpu-baseline still drop those two); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (the proof bytes of every proof in the step, "
                         "as float32 byte values) to DIR/<name>.npy (rank 0)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    return args


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N rank processes ourselves.  The parent has not imported
    torch or libcozk and never touches the GPU; the children are fresh processes (no exec from a GPU-initialised one).
    Rank 0's stdout carries the JSON line; every child's stderr passes through.  Returns the exit code."""
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # drain rank 0's stdout on a thread and poll EVERY child: the first rank that fails ends the run at once (the others
    # would otherwise sit in the rendezvous or a collective until its timeout, which can be minutes)
    import threading
    import time as _time
    buf = []
    reader = threading.Thread(target=lambda: buf.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    codes = [None] * n
    while any(c is None for c in codes):
        for i, p in enumerate(procs):
            if codes[i] is None:
                codes[i] = p.poll()
        if any(c not in (None, 0) for c in codes):
            for p in procs:  # fresh children of this process, no exec involved: safe to end on a GPU box
                if p.poll() is None:
                    p.kill()
            codes = [p.wait() for p in procs]
            break
        _time.sleep(0.05)
    reader.join(timeout=10)
    out0 = (buf[0] if buf else b"").decode(errors="replace")
    if any(codes):
        sys.stderr.write("bench.py: rank exit codes %s\n" % codes)
        sys.stdout.write(out0)
        return next((c for c in codes if c and c > 0), 1)
    lines = [ln for ln in out0.splitlines() if ln.startswith("{")]
    if len(lines) != 1:
        sys.stderr.write("bench.py: expected one JSON line from rank 0, got %d\n" % len(lines))
        sys.stdout.write(out0)
        return 1
    print(lines[0], flush=True)
    return 0


def main():
    args = parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%s but --gpus %d: launch one rank per GPU (or run `python bench.py --gpus N` "
                         "without a launcher and let it start its own ranks)" % (env_world, args.gpus))
    run_rank(args)


def run_plumbing(args):
    """--plumbing-only: everything of a multi-rank run except the proving (CPU-only rehearsal of launch + rendezvous)"""
    import importlib
    if os.environ.get("COZK_BENCH_TEST_FAIL_RANK") == os.environ.get("RANK", "0"):
        sys.exit(3)  # test hook (tests/test_dist_cpu.py): this rank dies before the rendezvous
    dist = importlib.import_module("co-zkvms_amd.dist")
    grp = dist.Group(backend="gloo", device=None)
    grp.barrier()
    t = grp.max_over_ranks(1.0 + grp.rank)
    digs = grp.all_gather_bytes(bytes([grp.rank]) * 32)
    # the star exchange of a worker-sharded proof: libcozk's shared-memory hub (host-only code, needs no GPU), 64 rounds of a few
    # hundred bytes from every rank, each rank checking every other rank's bytes of every round
    hub_ok = None
    if args.hub == "shm":
        pd = importlib.import_module("co-zkvms_amd.party_dist")
        hub = pd.ShmHub(grp.rank, grp.world, grp.cpu_group())
        hub_ok = True
        for rnd in range(64):
            got = hub.all_gather(bytes([(grp.rank * 31 + rnd + k) & 0xFF for k in range(136 + grp.rank)]), cap=4096)
            for q in range(grp.world):
                hub_ok = hub_ok and got[q] == bytes([(q * 31 + rnd + k) & 0xFF for k in range(136 + q)])
        oks = grp.all_gather_bytes(bytes([1 if hub_ok else 0]) * 32)
        hub_ok = all(o[0] == 1 for o in oks)
        hub.close()
    grp.barrier()
    if grp.rank == 0:
        print(json.dumps({"plumbing_only": True, "n_gpus": grp.world, "max_over_ranks": t, "ranks_seen": [d[0] for d in digs],
                          "shm_hub_64_rounds_ok": hub_ok}), flush=True)
    grp.close()


def run_rank(args):
    if args.plumbing_only:
        return run_plumbing(args)
    import importlib
    import torch
    pkg = importlib.import_module("co-zkvms_amd")
    dist = importlib.import_module("co-zkvms_amd.dist")
    hprof = importlib.import_module("co-zkvms_amd.harness_prof")
    rank, local_rank, world = dist.env_world()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the engine has no CPU path")
    ndev = torch.cuda.device_count()
    dev = local_rank % ndev
    torch.cuda.set_device(dev)
    grp = dist.Group(device=dev)

    log_n = args.log_n
    split = world > 1 and args.shard == "worker"
    if split and (world & (world - 1) or world > 8):
        raise SystemExit("--shard worker needs a power-of-two number of GPUs <= 8")
    logw = world.bit_length() - 1 if split else 0
    total_log_n = log_n + logw  # one proof over the whole 2^(log_n + log2 N)-cycle trace
    workload = dict(n_fr=64, n_u16=32, n_u32=16, n_flags=16, n_small=0, gp_batch=8, gp_log_leaves=total_log_n + 1)
    t_setup = time.time()
    if split:
        pd = importlib.import_module("co-zkvms_amd.party_dist")
        party = pd.DistributedParty(0, device=dev, worker=rank, mode="plain", log_workers=logw, log_n=total_log_n, seed=2026, **workload)
        # star messages are a few hundred bytes per round, ~300 rounds per proof: on one node they go through
        # libcozk's shared-memory mailboxes (~1 us) rather than a socket collective (~100 us)
        hub = pd.ShmHub(rank, world, grp.cpu_group()) if args.hub == "shm" else pd.TorchHub(rank, world, grp.cpu_group())

        class _H:  # same surface as Harness for the timed loop below
            def prove(self, verify=True):
                return party.prove(hub, None, verify=verify)

            def last_error(self):
                return party.last_error()

            def proof_bytes(self, res):  # the participant is a libcozk harness handle: same accessor as Harness
                return pkg.Harness.proof_bytes(party, res)

            def party_ctx_handle(self, _p=0):
                return party.ctx_handle()

            def close(self):
                party.close()
        h = _H()
    else:
        h = pkg.Harness(mode="plain", log_n=log_n, seed=dist.shard_seed(2026, rank), devices=(dev, dev, dev), leaf_fingerprints=args.leaf_fingerprints,
                        **workload)
    t_setup_main = time.time() - t_setup

    # optional 8(f) phases of the step (off by default: the headline is quoted on the 8(a) path above)
    extra = []
    if (args.lookups or args.outer) and world != 1:
        raise SystemExit("--lookups / --outer are single-GPU phases (N = 1)")
    if args.lookups:
        LK = importlib.import_module("co-zkvms_amd.lookups")
        extra.append(("lookups", LK.LookupsHarness(mode="plain", log_n=log_n, n_pairs=54, density_pct=10, seed=2026, devices=(dev, dev, dev), primary=True)))
    if args.outer:
        OU = importlib.import_module("co-zkvms_amd.outer")
        extra.append(("outer", OU.OuterHarness(mode="plain", log_steps=log_n, seed=2026, devices=(dev, dev, dev), system="jolt", full=True)))
    t_setup = t_setup_main

    # correctness gate (untimed): the assembled proof verifies (GKR, leaf evaluation, reduction sumcheck,
    # PST13 opening with the trapdoor)
    res = h.prove(verify=True)
    if res.verified != 1:
        raise SystemExit("proof rejected: " + h.last_error())
    digest0 = bytes(res.proof_digest)
    extra_digest = {}
    for name, eh in extra:
        er = eh.prove(verify=True)
        if er.verified != 1:
            raise SystemExit(name + " proof rejected: " + eh.last_error())
        extra_digest[name] = bytes(er.proof_digest)
    for _ in range(max(0, args.warmup - 1)):
        h.prove(verify=False)
        for _, eh in extra:
            eh.prove(verify=False)

    if args.full:
        hprof.prof_enable(h, 0, True)
    grp.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    phases = dict(commit=0.0, gp_construct=0.0, gp_prove=0.0, evaluate=0.0, open=0.0)
    hub_wait_ms, hub_exchanges = 0.0, 0
    extra_res = {}
    for _ in range(args.steps):
        r = h.prove(verify=False)
        hub_wait_ms += getattr(r, "t_hub_wait_ms", 0.0)
        hub_exchanges += int(getattr(r, "hub_exchanges", 0))
        phases["commit"] += r.t_commit_ms
        phases["gp_construct"] += r.t_gp_construct_ms
        phases["gp_prove"] += r.t_gp_prove_ms
        phases["evaluate"] += r.t_eval_ms
        phases["open"] += r.t_open_ms
        if bytes(r.proof_digest) != digest0:
            raise SystemExit("non-deterministic proof across steps")
        for name, eh in extra:
            er = extra_res[name] = eh.prove(verify=False)
            if bytes(er.proof_digest) != extra_digest[name]:
                raise SystemExit("non-deterministic %s proof across steps" % name)
            if name == "lookups":
                for k, v in (("lookups_primary_sumcheck", er.t_primary_ms), ("lookups_gp_construct", er.t_construct_ms), ("lookups_gp_prove", er.t_prove_ms)):
                    phases[k] = phases.get(k, 0.0) + v
            else:
                for k, v in (("spartan_build_AzBzCz", er.t_build_ms), ("spartan_outer_sumcheck", er.t_outer_ms), ("spartan_inner_sumcheck", er.t_inner_ms),
                             ("spartan_shift_sumcheck", er.t_shift_ms), ("spartan_openings", er.t_openings_ms)):
                    phases[k] = phases.get(k, 0.0) + v
    torch.cuda.synchronize(dev)
    grp.barrier()
    dt = time.perf_counter() - t0
    dt_local = dt
    dt = grp.max_over_ranks(dt)
    if args.full:
        prof = hprof.prof_read(h, 0)
        kprof = hprof.prof_read_kernels(h, 0)
        hprof.prof_enable(h, 0, False)
    digests = grp.all_gather_bytes(digest0)
    # per-rank view (N > 1): every rank's phase times and the time its coordinator copy waited in the hub for the slowest participant
    # of each star exchange -- what makes a scaling curve interpretable (a rank that waits is not the one that limits the step)
    mine = json.dumps({"rank": rank, "device": dev, "ms_per_step": round(dt_local * 1e3 / args.steps, 3),
                       "phases_ms_per_step": {k: round(v / args.steps, 3) for k, v in phases.items()},
                       "hub_wait_ms_per_step": round(hub_wait_ms / args.steps, 3), "hub_exchanges_per_step": hub_exchanges // max(1, args.steps)}).encode()
    per_rank = [json.loads(b.rstrip(b"\0").decode()) for b in grp.all_gather_bytes(mine.ljust(1024, b"\0"), width=1024)] if world > 1 else None

    cycles = (1 << log_n) * args.steps * world
    value = cycles / dt
    ms_per_step = dt * 1e3 / args.steps

    # ---- roofline of the dominant kernel and the per-kernel figures (--full: HIP events in the timed steps + a micro-benchmark)
    roofline = _roofline_leg(pkg, dev, prof, kprof, dt, log_n, world) if args.full else None

    out = {"metric": "RISC-V cycles proved/sec (co-Jolt hot path: PST13 commit + dense GKR grand product + openings)",
           "value": round(value, 1), "unit": "cycles/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "u32-limb BN254 Fr/Fq (254-bit Montgomery integers)", "data": "synthetic",
           "config": {"workload": "configs[1] restated (SURVEY 8d): 2^%d-cycle trace per GPU, plain prover, 128 polys "
                                  "(64 Fr + 32 u16 + 16 u32 + 16 flags) PST13 batch commit, dense grand product 8 x 2^%d leaves, "
                                  "batch evaluate + opening reduction + PST13 open" % (log_n, log_n + 1)
                                  + ("; + 8(f)1 Lasso primary sumcheck (27 RV32I collations) and toggled grand product, 54 memories" if args.lookups else "")
                                  + ("; + 8(f)2 whole Spartan worker on the Jolt constraint set (128 rows/step)" if args.outer else ""),
                      "log_n": log_n, "polys": 128, "gp_batch": 8,
                      "parallelism": ("single GPU" if world == 1 else
                                      ("one proof of a 2^%d-cycle trace sharded over %d worker sub-nets (high-variable chunks), star all-gather per round" % (total_log_n, world)
                                       if split else "independent trace segment per GPU")),
                      "ranks_per_gpu": max(1, -(-world // ndev))},
           "phases_ms_per_step": {k: round(v / args.steps, 3) for k, v in phases.items()},
           "setup_s": round(t_setup, 2), "proof_bytes": int(res.proof_len), "proof_sha256": [d.hex()[:16] for d in digests]}
    if roofline is not None:
        out["roofline"] = roofline
    if per_rank is not None:
        out["per_rank"] = per_rank

    # ---- host-resident witness: what the H2D leg adds when the boundary hands over host buffers (never part of `value`)
    if args.host_witness and rank == 0 and world == 1:
        out["host_witness"] = _host_witness_leg(pkg, torch, dev, log_n, ms_per_step)

    if args.witness_scatter and rank == 0 and world == 1:
        out["witness_scatter"] = _witness_scatter_leg(pkg, torch, dev, log_n)

    # ---- full_step (N = 1): the one chained worker flow of co-jolt/src/jolt/vm/jolt/worker.rs:175-266 on the same trace length; its own
    #      harness, run after the timed region of `value` (it is a different, larger unit of work than the metric's step)
    if args.full and rank == 0 and world == 1 and not args.no_full_step:
        out["full_step"] = _full_step_leg(importlib, torch, dev, log_n, h)
        # the same flow on a witness with the widths of a real trace (a plain prover's commitments fill 2 of the 16 windows)
        rw = _full_step_leg(importlib, torch, dev, log_n, h, small_witness=1)
        out["full_step"]["real_width_witness"] = {k: rw[k] for k in ("witness", "ms", "cycles_per_s", "steps", "verified", "phases_ms", "proof_sha256")}

    # ---- CPU baseline (rank 0, N = 1 only): the oracle's C restatement on a bounded sample
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import coracle  # the checker, used here only as the timed CPU baseline
        s = args.cpu_sample_log_n
        cfg = dict(mode="plain", log_n=s, n_fr=64, n_u16=32, n_u32=16, n_flags=16, n_small=0, gp_batch=8, gp_log_leaves=s + 1, seed=2026)
        cres, _ = coracle.pipeline(cfg, want_proof=False)
        fr_scalar_muls = 64 * (1 << s)
        out["cpu_baseline"] = {"value": round((1 << s) / cres.t_total_s, 1), "unit": "cycles/s", "cores": int(cres.threads), "kind": "port",
                               "sample": "same pipeline and polynomial mix at a 2^%d-cycle trace (%.1f s of CPU work; plain-C OpenMP "
                                         "restatement oracle/c, not arkworks: signed-digit Pippenger with XYZZ buckets on an unrolled no-carry "
                                         "Montgomery product; batch commit = one polynomial's Pippenger per thread, as jolt-core's rayon "
                                         "batch_msm; cores = the CPUs this process may use: affinity capped by the cgroup quota)" % (s, cres.t_total_s),
                               "commit_share": round(cres.t_commit_s / cres.t_total_s, 3),
                               "commit_fr_scalar_muls_per_s_per_core_lower_bound": round(fr_scalar_muls / cres.t_commit_s / max(1, int(cres.threads)), 1),
                               "published": {"note": "the reference's own trace-derived numbers (BASELINE.md; FULL Jolt prover per party, AWS, "
                                                     "not this sub-path): not comparable with `value`, quoted as the contract asks",
                                             "2^20_cycles_8_vcpu": {"cycles_per_s": 5100, "prove_s": 204.6, "commit_s": 155.6},
                                             "2^22_cycles_32_vcpu": {"cycles_per_s": 12200, "prove_s": 345.9, "commit_s": 146.0}}}
    # nothing after the timed steps proves again on these harnesses: their last proofs are still the last timed step's
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, [("proof", h, r)] + [(name + "_proof", eh, extra_res[name]) for name, eh in extra])
    if rank == 0:
        print(json.dumps(out), flush=True)
    for _, eh in extra:
        eh.close()
    h.close()
    grp.close()


def _dump_outputs(out_dir, proofs):
    """--dump-outputs: what a caller of the timed path receives from its last step -- each proof, serialized -- as
    DIR/<name>.npy, one float32 per byte (exact), so that two builds can be compared output for output"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, harness, res in proofs:
        data = np.frombuffer(harness.proof_bytes(res), dtype=np.uint8)
        np.save(os.path.join(out_dir, name + ".npy"), data.astype(np.float32))


def _roofline_leg(pkg, dev, prof, kprof, dt, log_n, world):
    """`roofline`: the dominant kernel's HIP-event figures from the timed steps against HBM and integer-ALU peaks, plus the
    HBM-bound kernels of the polynomial seam"""
    launches = max(1, prof["launches"])
    avg_ms = prof["total_ms"] / launches
    alg_per_launch = prof["alg_bytes"] / launches
    achieved_gbs = alg_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    roofline = {"bound": "hbm", "kernel": "k_msm_accum0_f9", "achieved": round(achieved_gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved_gbs / HBM_PEAK_GBS, 6), "traffic": None,
                "limited_by": "int_alu (254-bit modular arithmetic puts this kernel ~100x above the HBM ridge; see int_alu)",
                "launches": prof["launches"], "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": int(alg_per_launch),
                "kernel_share_of_step": round(prof["total_ms"] / (dt * 1e3), 4),
                "co_run": "the sort of the NEXT launch set (k_msm_hist_lds / k_msm_scatter_lds, 256-thread workgroups on a high-priority "
                          "stream) runs beside this kernel: both launch durations include the time they share the chip, their shares of "
                          "the step add up to more than the commit phase; COZK_MSM_SERIAL=1 runs them back to back (profiles/ holds the "
                          "rocprofv3 summary of this command in both modes)"}
    # HBM traffic of the dominant kernel comes from separate rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE) of this same
    # command: bench.py cannot run rocprofv3 on itself, so the figure is a committed measurement, tagged with its source
    try:
        hbm_file = next(f for f in ("r3_pmc_hbm.json", "r2_pmc_hbm.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        pm = json.load(open(os.path.join(ROOT, "profiles", hbm_file)))
        pmc = next(v for k, v in pm["kernels"].items() if "k_msm_accum0_f9" in k)
        if log_n == 20 and world == 1:
            roofline["traffic"] = int((pmc["FETCH_SIZE_KB_per_launch"] + pmc["WRITE_SIZE_KB_per_launch"]) * 1024)
            roofline["traffic_source"] = "profiles/%s (%s); NOT measured in this run" % (hbm_file, pm.get("measured_at", "rocprofv3 --pmc passes of this command"))
    except Exception:
        pass
    # per-kernel rooflines of the HBM-bound kernels of the polynomial seam (HIP events on the context's streams;
    # algorithmic bytes per DESIGN.md 4 / SURVEY.md 8d)
    roofline["kernels"] = {}
    for name, kp in kprof.items():
        if kp["launches"] and kp["total_ms"] > 0:
            gbs = kp["alg_bytes"] / (kp["total_ms"] * 1e-3) / 1e9
            roofline["kernels"][name] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                                         "launches": kp["launches"], "avg_launch_ms": round(kp["total_ms"] / kp["launches"], 4),
                                         "algorithmic_bytes_per_launch": int(kp["alg_bytes"] / kp["launches"]),
                                         "share_of_step": round(kp["total_ms"] / (dt * 1e3), 4)}
    # the honest ceiling of the dominant kernel is the integer ALU: the measured peak of the multiplier the
    # gather kernel uses (variant 2 = 9 x 29-bit unsaturated limbs, 162 mads per product; fq9.hip.hpp), best of 7 runs so that
    # the denominator does not move between runs; variant 1 = the saturated 8 x 32 multiplier, reported beside it
    ctx = pkg.Context(dev)
    lanes = 256 * 256 * 16
    mm_ms = min(ctx.bench_montmul(lanes, 2000, 2) for _ in range(7))
    peak_gmul = lanes * 2000 / mm_ms / 1e6
    sat_ms = min(ctx.bench_montmul(lanes, 2000, 1) for _ in range(3))
    ctx.close()
    muls_per_madd = MADS_PER_MADD / MADS_PER_MUL
    gmul = prof["point_adds"] * muls_per_madd / (prof["total_ms"] * 1e-3) / 1e9 if prof["total_ms"] > 0 else 0.0
    roofline["int_alu"] = {"achieved": round(gmul, 2), "peak": round(peak_gmul, 2), "unit": "G Fq-montmul/s",
                           "frac": round(gmul / peak_gmul, 4), "saturated_8x32_peak": round(lanes * 2000 / sat_ms / 1e6, 2),
                           "mads_per_point_add": MADS_PER_MADD, "mads_per_product": MADS_PER_MUL,
                           "note": "mixed XYZZ addition = 6 products + 2 squarings + one fused two-product reduction = 1467 v_mad_u64_u32 "
                                   "= 9.06 products of the 9x29-bit multiplier (162 mads); peak = that multiplier's dependent-product "
                                   "micro-benchmark, best of 7 in this run"}
    # how full the vector-issue slots of the gather kernel are: SQ counters of a separate rocprofv3 --pmc pass (committed, tagged)
    try:
        sq_file = next(f for f in ("r3_pmc_sq.json", "r2_pmc_sq.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        sq = json.load(open(os.path.join(ROOT, "profiles", sq_file)))
        ks = next(v for k, v in sq["kernels"].items() if "k_msm_accum0_f9" in k)
        if log_n == 20 and world == 1:
            roofline["int_alu"]["valu_issue_utilisation"] = ks["derived"]["valu_issue_utilisation_same_pass"]
            roofline["int_alu"]["lane_utilisation"] = ks["derived"]["lane_utilisation"]
            roofline["int_alu"]["valu_instructions_per_point_add"] = round(ks["SQ_INSTS_VALU"] * 64.0 / (prof["point_adds"] / launches), 1)
            roofline["int_alu"]["counters_source"] = "profiles/%s (%s); NOT measured in this run" % (sq_file, sq.get("measured_at", ""))
    except Exception:
        pass
    return roofline


def _full_step_leg(importlib, torch, dev, log_n, main_harness, steps=3, small_witness=0):
    """ONE chained co-jolt worker flow (cozk_flow_*): commit-all -> bytecode -> instruction lookups (primary sumcheck, toggled + dense grand
    products) -> read-write memory + output check -> Spartan (outer + inner + shift, the reference's constraint set) -> one reduce_and_prove,
    one transcript, one opening accumulator, Jolt's shape (54 memories, 26 subtables, M = 2^16); verified once, then timed."""
    FL = importlib.import_module("co-zkvms_amd.flow")
    t0 = time.time()
    fh = FL.FlowHarness(mode="plain", log_n=log_n, log_m=min(16, log_n), log_b=min(14, log_n), log_mem=min(17, log_n), n_mem=54, n_subtables=26, seed=2026,
                        devices=(dev, dev, dev), small_witness=small_witness)
    setup_s = time.time() - t0
    r = fh.prove(verify=True)
    if r.verified != 1:
        raise SystemExit("full_step: proof rejected: " + fh.last_error())
    d0 = bytes(r.proof_digest)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ph = {}
    for _ in range(steps):
        r = fh.prove(verify=False)
        if bytes(r.proof_digest) != d0:
            raise SystemExit("full_step: non-deterministic proof across steps")
        for k, v in (("commit", r.t_commit_ms), ("bytecode", r.t_bytecode_ms), ("lookups_primary_sumcheck", r.t_primary_ms),
                     ("lookups_memory_checking", r.t_lookups_gp_ms), ("read_write_memory", r.t_rw_ms), ("spartan", r.t_spartan_ms),
                     ("reduce_and_prove", r.t_open_ms)):
            ph[k] = ph.get(k, 0.0) + v
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    out = {"what": "one chained co-jolt worker flow (jolt/vm/jolt/worker.rs:175-266): commit-all, bytecode + instruction-lookups + read-write-memory "
                   "checking, Spartan on the Jolt constraint set, ONE batched PST13 opening; one transcript, one opening accumulator; NOT the metric's step",
           "witness": ("counters < 2^log_n, E polynomials and memory values 32 bits: the widths of a real trace, what a PLAIN prover commits to"
                       if small_witness else
                       "counters, E polynomials and memory values are uniform field elements: what a Rep3 party commits to (its share of every "
                       "value is uniform), an upper bound for a plain prover"),
           "ms": round(dt * 1e3, 3), "cycles_per_s": round((1 << log_n) / dt, 1), "steps": steps, "verified": 1,
           "phases_ms": {k: round(v / steps, 3) for k, v in ph.items()}, "polys_committed": int(r.n_polys), "openings": int(r.n_openings),
           "memories": 54, "subtables": 26, "proof_bytes": int(r.proof_len), "proof_sha256": d0.hex()[:16], "setup_s": round(setup_s, 1),
           "excluded": "party 0's public TimestampValidityProof and the hashes' multiset-equality check (synthetic counters), see DESIGN.md"}
    fh.close()
    return out


def _host_witness_leg(pkg, torch, dev, log_n, ms_per_step):
    """H2D upload of a host-resident witness of the bench workload's size from pinned memory: 64 Fr polynomials
    (32 B x 2^log_n each) + 32 u16 + 16 u32 + 16 u8 columns, one cozk_vec_upload each, serialized before the step
    (no overlap with compute: an upper bound on what a host-buffer boundary costs)."""
    import ctypes
    n = 1 << log_n
    ctx = pkg.Context(dev)
    lib = pkg._lib.lib()
    specs = [(64, 32, pkg.SCALAR_FR), (32, 2, pkg.SCALAR_U16), (16, 4, pkg.SCALAR_U32), (16, 1, pkg.SCALAR_U8)]
    host = {bytes_per: torch.zeros(n * bytes_per, dtype=torch.uint8).pin_memory() for _, bytes_per, _ in specs}
    total = sum(cnt * n * b for cnt, b, _ in specs)
    best = None
    for _ in range(3):
        vecs = []
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for cnt, b, kind in specs:
            for _i in range(cnt):
                hnd = ctypes.c_void_p()
                ctx.check(lib.cozk_vec_upload(ctx.h, ctypes.c_void_p(host[b].data_ptr()), n, kind, ctypes.byref(hnd)))
                vecs.append(hnd)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        for hnd in vecs:
            lib.cozk_vec_free(hnd)
        best = dt if best is None else min(best, dt)
    ctx.close()
    up_ms = best * 1e3
    return {"upload_bytes": total, "upload_ms": round(up_ms, 3), "upload_GBps": round(total / best / 1e9, 2),
            "ms_per_step_incl_upload": round(ms_per_step + up_ms, 3),
            "value_incl_upload": round((1 << log_n) / ((ms_per_step + up_ms) * 1e-3), 1),
            "note": "pinned host memory, uploads serialized before the step (no overlap); `value` above excludes this"}


def _witness_scatter_leg(pkg, torch, dev, log_n, n_polys=64):
    """the reference's `init` phase (receive_witness_share: 71 s at 2^20) restated device to device: for each
    of the 64 Fr polynomials the dealer's context generates the three parties' Rep3 components (keyed ChaCha12 PRF) and
    they land in the parties' contexts -- on their own GPUs when >= 3 (or >= 2) are visible, else on this one"""
    n = 1 << log_n
    ndev = torch.cuda.device_count()
    devs = [dev, (dev + 1) % ndev, (dev + 2) % ndev] if ndev >= 3 else [dev] * 3
    dealer = pkg.Context(dev)
    parties = [pkg.Context(d) for d in devs]
    secret = [pkg.Vec.random(dealer, n, seed=900 + i) for i in range(4)]  # four distinct secrets, reused round-robin
    k0, k1 = bytes(range(32)), bytes(range(32, 64))
    best = None
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n_polys):
            for p in range(3):
                a, b = secret[i % 4].rep3_scatter(k0, k1, p, parties[p], counter=i * n)
                a.free()
                b.free()
        for c in parties:
            c.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    nbytes = n_polys * 3 * 2 * n * 32
    for c in parties:
        c.close()
    dealer.close()
    return {"polys": n_polys, "parties": 3, "party_devices": devs, "share_bytes_delivered": nbytes, "ms": round(best * 1e3, 3),
            "GBps_delivered": round(nbytes / best / 1e9, 1),
            "note": "shares generated on the dealer's GPU (ChaCha12 PRF, 2 blocks per element) and written into the parties' contexts; "
                    "peer copies over xGMI when the parties have GPUs of their own; not part of `value`"}


if __name__ == "__main__":
    main()
