"""One party of a Shamir multiplication, one process and one GPU per party, over the native ring (cozk_shamir_mul_vec):
the deployment of the reference, and the child process of tests/test_gpu_shamir_mul.py's three-GPU test.
  rank 0:  python tools/shamir_mul_party.py --rank 0 --ranks N --job FILE      (prints "ring-id HEX", then joins)
  others:  python tools/shamir_mul_party.py --rank R --ranks N --job FILE --ring-id HEX
FILE is JSON: {"a": [hex..], "b": [hex..], "keys": [hex of 32 bytes, `degree` of them], "degree": t, "counter": c, "out": PATH};
a and b are this party's share vectors as canonical integers; PATH receives its share of the product the same way.  A party
above 2 * degree may leave "b" and "keys" null.  The GPU is device `--device` (default: the rank)."""
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
        raise SystemExit("shamir_mul_party: only rank 0 draws the ring id; pass --ring-id")
    ring_id = cozk.Context.ring_unique_id()
    print("ring-id " + ring_id.hex(), flush=True)
else:
    ring_id = bytes.fromhex(args.ring_id)
ctx = cozk.Context(args.rank if args.device is None else args.device)
ctx.ring_init(ring_id, args.rank, args.ranks)  # blocks until every rank has joined
ints = lambda xs: [int(x, 16) for x in xs]
a = cozk.Vec.from_ints(ctx, ints(job["a"]))
b = cozk.Vec.from_ints(ctx, ints(job["b"])) if job.get("b") is not None else None
keys = [bytes.fromhex(k) for k in job["keys"]] if job.get("keys") is not None else None
c = ctx.shamir_mul_vec(a, b, keys, job["degree"], counter=job.get("counter", 0))
with open(job["out"], "w") as fh:
    json.dump([hex(x) for x in c.to_ints()], fh)
ctx.ring_destroy()
ctx.close()
