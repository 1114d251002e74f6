// The time-ordered walk shared by the Lasso lookup witness (lasso_witness.hip) and, through the radix pass of radix_pass.hip.hpp,
// by the read-write memory witness (rw_memory_witness.hip) and the time counters (ts_range_witness.hip): ONE wave takes 64 keys in
// time order (lane = time) and ranks each among the earlier equal keys of its tile, against a u16 table of per-key counts in LDS.
#pragma once
#include "common.hpp"

// One wave step.  Every lane of the wave calls it (the ballots and the shuffle are wave-wide); `valid` lanes carry a key < 2^key_bits.
// The lanes with equal keys find each other with one ballot per key bit; the lowest lane of a group reads and bumps the table
// (distinct leaders have distinct keys: no atomic), the group takes the old value by shuffle and adds the number of its lower lanes.
// Returns, for a valid lane, the number of earlier equal keys since the table was cleared.
__device__ __forceinline__ uint32_t lw_walk_step(uint16_t* tab, bool valid, uint32_t key, int key_bits, unsigned lane) {
    const unsigned long long below = (1ull << lane) - 1;
    unsigned long long peers = __ballot(valid);
    for (int bit = 0; bit < key_bits; bit++) {
        const bool set = (key >> bit) & 1;
        const unsigned long long bal = __ballot(set);
        peers &= set ? bal : ~bal;
    }
    if (!valid) peers = 1ull << lane;
    const int leader = __ffsll((long long)peers) - 1;
    uint32_t old = 0;
    if (valid && leader == (int)lane) {
        old = tab[key];
        tab[key] = (uint16_t)(old + (uint32_t)__popcll(peers));
    }
    old = __shfl(old, leader);
    // the next wave step reads what this one wrote: keep the table accesses in program order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return old + (uint32_t)__popcll(peers & below);
}
