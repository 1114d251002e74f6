"""Time the instruction-lookups harness (toggled / sparse grand product of Lasso's read / write memory
checking) at Jolt's shape -- 54 memories (108 circuits), ~10 % flag density -- and print one JSON line.
  python tools/run_lookups.py --mode plain --log-n 20 [--pairs 54] [--density 10] [--steps 3]
  python tools/run_lookups.py --sparse-ab --log-n 18 --steps 5 --out profiles/lookups_sparse_ab_2p18.json
--sparse-ab: the whole prove with COZK_TOGGLE_SPARSE at 0 and at 1, alternating in one process on one harness; the proof digests must
agree; medians, min..max and the sparse pair layer counters (cozk_sparse_stats of party 0, one proof) go to --out."""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["plain", "rep3"], default="plain")
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--pairs", type=int, default=54)
ap.add_argument("--density", type=int, default=10)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--primary", action="store_true", help="also run Lasso's primary sumcheck (8f1b)")
ap.add_argument("--mix", choices=["uniform", "sha2"], default="uniform", help="instruction mix of the synthetic trace (sha2: trace-shaped, ~6 %% multiplicative)")
ap.add_argument("--sparse-ab", action="store_true", help="A/B of COZK_TOGGLE_SPARSE=0 / 1, alternating in one process")
ap.add_argument("--out", default=None, help="--sparse-ab: the JSON file the result is written to (it is printed too)")
args = ap.parse_args()
LK = importlib.import_module("co-zkvms_amd.lookups")
ngpu = torch.cuda.device_count()
devs = (0, 1, 2) if ngpu >= 3 else (0, 0, 0)
t0 = time.time()
h = LK.LookupsHarness(mode=args.mode, log_n=args.log_n, n_pairs=args.pairs, density_pct=args.density, seed=2026, devices=devs, primary=args.primary, mix=args.mix)
setup_s = time.time() - t0
if args.sparse_ab:
    import statistics
    legs = {"dense": dict(switch="0", wall=[], construct=[], prove=[]), "sparse": dict(switch="1", wall=[], construct=[], prove=[])}
    digests, stats, hbm = {}, None, {}
    for name, leg in legs.items():  # one verified proof per leg (also the warm-up)
        os.environ["COZK_TOGGLE_SPARSE"] = leg["switch"]
        h.reset_sparse_stats()
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        digests[name] = bytes(r.proof_digest).hex()
        hbm[name] = round((torch.cuda.mem_get_info(0)[1] - torch.cuda.mem_get_info(0)[0]) / 2**30, 2)
        if name == "sparse":
            stats = h.sparse_stats(0).as_dict()
        else:
            assert h.sparse_stats(0).as_dict()["layers_sparse"] == 0
    assert digests["dense"] == digests["sparse"], "the sparse leg's proof differs from the dense leg's"
    for _ in range(args.steps):
        for name, leg in legs.items():
            os.environ["COZK_TOGGLE_SPARSE"] = leg["switch"]
            t0 = time.perf_counter()
            r = h.prove(verify=False)
            leg["wall"].append((time.perf_counter() - t0) * 1e3)
            leg["construct"].append(r.t_construct_ms)
            leg["prove"].append(r.t_prove_ms)
            assert bytes(r.proof_digest).hex() == digests["dense"]
    os.environ.pop("COZK_TOGGLE_SPARSE", None)
    summ = lambda v: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    d, sp = legs["dense"]["wall"], legs["sparse"]["wall"]
    out = {"what": "toggled grand product, COZK_TOGGLE_SPARSE=0 (dense leg: the default path) vs 1 (sparse pair layers), alternating in one process",
           "mode": args.mode, "log_n": args.log_n, "memories": args.pairs, "circuits": 2 * args.pairs, "density_pct": args.density, "devices": list(devs),
           "steps_per_leg": args.steps, "proof_digest": digests["dense"], "digests_equal": True,
           "ms": {name: {k: summ(leg[k]) for k in ("wall", "construct", "prove")} for name, leg in legs.items()},
           "sparse_median_inside_dense_spread": min(d) <= statistics.median(sp) <= max(d),
           "sparse_stats_party0_one_proof": stats,
           "sparse_bytes_over_dense_equivalent": round(stats["bytes_sparse"] / stats["bytes_dense_equivalent"], 4) if stats["bytes_dense_equivalent"] else None,
           "hbm_gib_in_use_after_first_proof": hbm, "setup_s": round(setup_s, 1)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    h.close()
    sys.exit(0)
r = h.prove(verify=True)
assert r.verified == 1, h.last_error()
t0 = time.perf_counter()
for _ in range(args.steps):
    r = h.prove(verify=False)
dt = (time.perf_counter() - t0) / args.steps
print(json.dumps({"what": ("Lasso primary sumcheck + " if args.primary else "") + "toggled grand product (instruction lookups read/write memory checking)", "mode": args.mode, "mix": args.mix, "log_n": args.log_n,
                  "memories": args.pairs, "circuits": 2 * args.pairs, "density_pct": args.density, "devices": list(devs), "verified": 1,
                  "ms_per_proof": round(dt * 1e3, 2), "cycles_per_s": round((1 << args.log_n) / dt, 1),
                  "phases_ms": {"primary_sumcheck": round(r.t_primary_ms, 2), "gp_construct": round(r.t_construct_ms, 2), "gp_prove": round(r.t_prove_ms, 2)},
                  "ring_bytes_all_parties": int(r.bytes_ring), "star_messages": int(r.star_messages), "proof_bytes": int(r.proof_len),
                  "setup_s": round(setup_s, 1), "hbm_gib_in_use": round((torch.cuda.mem_get_info(0)[1] - torch.cuda.mem_get_info(0)[0]) / 2**30, 1)}), flush=True)
h.close()
