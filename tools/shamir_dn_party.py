"""One party of the Shamir multiplication with a king, one process and one GPU per party, over the native ring: the
preprocessing (cozk_shamir_rand_vec) followed by one multiplication that consumes pair 0 (cozk_shamir_mul_king_vec).  The child
process of tests/test_gpu_shamir_dn.py's three-GPU test.
  rank 0:  python tools/shamir_dn_party.py --rank 0 --ranks N --job FILE      (prints "ring-id HEX", then joins)
  others:  python tools/shamir_dn_party.py --rank R --ranks N --job FILE --ring-id HEX
FILE is JSON: {"a": [hex..], "b": [hex..], "keys": [hex of 32 bytes, 3 * degree + 1 of them], "degree": t, "counter": c, "king": k,
"out": PATH}; a and b are this party's share vectors as canonical integers (null on a party above 2 * degree, which then needs
"n", the length).  PATH receives {"pairs": [[r_t, r_2t], ..], "c": [..]}: this party's halves of every pair and its share of the
product.  The GPU is device `--device` (default: the rank)."""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401 - maps librccl first; libcozk reuses that copy

ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int, required=True)
ap.add_argument("--ranks", type=int, required=True)
ap.add_argument("--job", required=True)
ap.add_argument("--ring-id", default=None)
ap.add_argument("--device", type=int, default=None)
args = ap.parse_args()
cozk = importlib.import_module("co-zkvms_amd")
with open(args.job) as fh:
    job = json.load(fh)
if args.ring_id is None:
    if args.rank != 0:
        raise SystemExit("shamir_dn_party: only rank 0 draws the ring id; pass --ring-id")
    ring_id = cozk.Context.ring_unique_id()
    print("ring-id " + ring_id.hex(), flush=True)
else:
    ring_id = bytes.fromhex(args.ring_id)
ctx = cozk.Context(args.rank if args.device is None else args.device)
ctx.ring_init(ring_id, args.rank, args.ranks)  # blocks until every rank has joined
ints = lambda xs: [int(x, 16) for x in xs]
vec = lambda name: cozk.Vec.from_ints(ctx, ints(job[name])) if job.get(name) is not None else None
a, b = vec("a"), vec("b")
n = len(a) if a is not None else job["n"]
keys = [bytes.fromhex(k) for k in job["keys"]]
pairs = ctx.shamir_rand_vec(n, keys, job["degree"], counter=job.get("counter", 0))
r_t, r_2t = pairs[0]
c = ctx.shamir_mul_king_vec(a, b, r_t, r_2t, job["degree"], king=job.get("king", 0))  # pair 0 is spent
hexes = lambda v: [hex(x) for x in v.to_ints()]
with open(job["out"], "w") as fh:
    json.dump({"pairs": [[hexes(x), hexes(y)] for x, y in pairs], "c": hexes(c)}, fh)
ctx.ring_destroy()
ctx.close()
