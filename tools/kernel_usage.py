"""Registers / scratch / LDS / occupancy of the kernels of one translation unit, from hipcc -Rpass-analysis=kernel-resource-usage:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -c co-zkvms_amd/csrc/poly.hip -o /tmp/poly.o -Rpass-analysis=kernel-resource-usage 2> usage.txt
  python tools/kernel_usage.py usage.txt [name-regex]
The group kernels of the Shamir provers (every one must report 0 bytes of scratch; DESIGN.md 4b quotes their lines):
  python tools/kernel_usage.py usage.txt 'k_(layer|toggle|spartan)_group'
  python tools/kernel_usage.py usage.txt 'k_(outer|shift)_group_(round|final)'
  python tools/kernel_usage.py usage.txt 'k_primary_group_(deal|combine|final)'   (144 bytes of scratch, as k_primary_level<1> and k_primary_final<1>)
  python tools/kernel_usage.py usage.txt 'k_primary_group_mask'                   (the king level: the same 144 bytes, none of its own; its
                                                                                   finish is shamir.hip's k_shamir_king_finish: 0 bytes)"""
import re, sys
txt = open(sys.argv[1]).read()
pat = sys.argv[2] if len(sys.argv) > 2 else "."
for b in re.split(r"Function Name: ", txt)[1:]:
    name = b.split()[0]
    g = lambda k: (re.search(k + r": (\d+)", b) or [None, "?"])[1]
    if re.search(pat, name):
        print("%-90s VGPR %4s AGPR %3s scratch %5s LDS %6s occ %s" % (name[:90], g("VGPRs"), g("AGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
