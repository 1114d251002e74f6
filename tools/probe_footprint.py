import sys, torch
gb = int(sys.argv[1])
keep = []
if gb:
    keep.append(torch.empty(gb << 30, dtype=torch.uint8, device="cuda"))
    keep[0].fill_(1)
sys.argv = ["bench.py", "--full", "--steps", "5", "--warmup", "1", "--no-cpu-baseline"]
sys.path.insert(0, ".")
import bench
bench.main()
