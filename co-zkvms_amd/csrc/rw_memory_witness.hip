// The dealer's read-write memory witness on the device: v_read / t_read / v_final / t_final of Jolt's register + RAM memory
// (jolt-core's ReadWriteMemoryPolynomials::generate_witness, which the coordinator runs before read_write_memory/witness.rs:34-93
// shares the result): one strictly sequential host pass over the n * n_slots memory operations, ordered by (step j, slot s), with
// random access into a table of MEM words.  Starting from v = v_init, t = 0, for each operation with a = addr[s][j]:
//
//   v_read[s][j] = v[a];   t_read[s][j] = t[a];
//   w = (slot s writes at step j) ? v_write[s][j] : v[a];
//   v[a] = w;   t[a] = j;   (v_written[s][j] = w)               and at the end   v_final = v, t_final = t
//
// Here the walk is a stable sort of the operations by address and a sweep over the sorted operations: the previous access to an
// address is the sorted neighbour (t_read), the previous write is the last write before it if that write has the same address
// (v_read; v_init[a] otherwise), the last operation of an address gives v_final / t_final.  With N = n * n_slots operations,
// operation i = j * n_slots + s:
//
//   sort: least-significant-digit radix passes of 16 bits, one for MEM <= 65536, else two (the second over the high digit's actual
//   range).  The pass itself -- the tile walk, the scan over the tiles, the offsets scan -- is radix_pass.hip.hpp's; here are its
//   entry points and what is this witness's own, over tiles of RP_TILE positions and D digit values:
//     k_rw_rank     rp_rank_tile with the digit of a position: the address of the operation there (in the second pass a gather
//                   through the first pass's order), of one of n_slots interleaved columns of two widths.  The first pass also
//                   checks every address against MEM.
//     k_rw_scan     rp_scan_tiles per digit value; total -> count[digit]
//     k_rw_offsets  rp_offsets over count[]
//     k_rw_scatter  per position: order_out[offset[digit] + base[tile][digit] + rank] = the operation at the position
//   sweep: an exclusive max-scan of one u32 per sorted position q, q + 1 where the operation writes and 0 otherwise, as reduce /
//   scan / apply launches (no workgroup waits for another):
//     k_rw_last_write  per block of RW_BLOCK positions: the block's last write
//     k_rw_carry       one workgroup: exclusive max-scan of the blocks' words
//     k_rw_gather      per position: the last write before it (wave ballots + the waves' words + the block's carry), the
//                      neighbours; v_read / t_read / v_written back at (s, j), v_final / t_final from a segment's last operation.
//                      v_final / t_final start as v_init / 0, which is what an untouched address keeps.
//   The scanned word is q + 1 <= N < 2^32 and needs no segment starts: a write of another address is told apart by comparing its
//   address with the reader's, so one 32-bit scan serves every N the call takes (2 q + 1 with the segment start folded in needs 33).
//
// Nothing ranks by the return order of an atomic, so the outputs are bit-for-bit deterministic.  An address >= MEM is used as 0 by
// every kernel (no load or store leaves its buffer) and reported through one device word, the smallest (step, slot) of a violation
// (an atomicMin: its result does not depend on the order of arrival); the call then returns no vector.
//
// Transient device memory, with tiles = ceil(N / RP_TILE), D1 = min(MEM, 65536), D2 = ceil(MEM / 65536) (0 for one pass),
// D = max(D1, D2) rounded up to even, blocks = ceil(N / RW_BLOCK):
//   4 N (8 N for two passes) sorted operation indices + 2 N ranks + 6 tiles D histograms and bases + 4 D counts + 8 blocks
//   = 16 MiB + 8 MiB + 48 MiB at n = 2^20 with 4 slots and MEM = 2^16, 16 MiB more at MEM = 2^20.
#include "common.hpp"
#include "radix_pass.hip.hpp"

static constexpr int RW_WAVES = RP_PT / 64;
static constexpr int RW_ROWS = 16;               // rows of RP_PT positions per sweep block
static constexpr int RW_BLOCK = RP_PT * RW_ROWS;
static constexpr size_t RW_MAX_SLOTS = COZK_RW_MEMORY_MAX_SLOTS;

struct RwSlot {
    const void* addr;
    const uint32_t* vw;  // null: the slot only reads
    const uint8_t* iw;   // null: every step writes (if vw)
    uint32_t *vr, *tr, *vwr;
    int addr_u8;
};

// the address of operation (j, s); one >= MEM is used as 0 everywhere (and reported by k_rw_rank)
__device__ __forceinline__ uint32_t rw_raw_addr(const RwSlot& sl, uint32_t j) {
    return sl.addr_u8 ? (uint32_t)((const uint8_t*)sl.addr)[j] : ((const uint32_t*)sl.addr)[j];
}
__device__ __forceinline__ uint32_t rw_addr(const RwSlot& sl, uint32_t j, uint32_t MEM) {
    const uint32_t a = rw_raw_addr(sl, j);
    return a < MEM ? a : 0;
}
__device__ __forceinline__ bool rw_writes(const RwSlot& sl, uint32_t j) { return sl.vw && (sl.iw ? sl.iw[j] != 0 : true); }

// order: the operations in the order of the previous pass; null = operation i at position i
__global__ void __launch_bounds__(RP_PT) k_rw_rank(const RwSlot* __restrict__ slots, uint32_t n_slots, uint32_t N, uint32_t MEM, const uint32_t* __restrict__ order,
                                                   int shift, uint32_t Dp, int key_bits, uint16_t* __restrict__ rank, uint16_t* __restrict__ hist,
                                                   unsigned long long* __restrict__ viol) {
    const size_t tile = blockIdx.x;
    auto digit = [&](size_t p) {
        const uint32_t i = order ? order[p] : (uint32_t)p;
        const uint32_t j = i / n_slots, s = i - j * n_slots;
        const uint32_t raw = rw_raw_addr(slots[s], j);
        if (!order && raw >= MEM) atomicMin(viol, ((unsigned long long)j << 32) | s);
        return (uint16_t)((raw < MEM ? raw : 0) >> shift);
    };
    rp_rank_tile(tile, (size_t)N, digit, Dp, key_bits, rank, hist + tile * Dp);
}

__global__ void __launch_bounds__(RP_PT) k_rw_scan(uint32_t D, uint32_t Dp, size_t tiles, const uint16_t* __restrict__ hist, uint32_t* __restrict__ bases,
                                                   uint32_t* __restrict__ count) {
    const uint32_t d = blockIdx.x * RP_PT + threadIdx.x;
    if (d >= D) return;
    count[d] = rp_scan_tiles(tiles, Dp, hist + d, bases + d);
}

__global__ void __launch_bounds__(RP_SCAN_PT) k_rw_offsets(uint32_t D, uint32_t* __restrict__ count) { rp_offsets(D, count); }

__global__ void __launch_bounds__(RP_PT) k_rw_scatter(const RwSlot* __restrict__ slots, uint32_t n_slots, uint32_t N, uint32_t MEM, const uint32_t* __restrict__ order,
                                                      int shift, uint32_t Dp, const uint16_t* __restrict__ rank, const uint32_t* __restrict__ bases,
                                                      const uint32_t* __restrict__ offset, uint32_t* __restrict__ order_out) {
    const size_t p = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (p >= N) return;
    const uint32_t i = order ? order[p] : (uint32_t)p;
    const uint32_t j = i / n_slots, s = i - j * n_slots;
    const uint32_t d = (rw_addr(slots[s], j, MEM) >> shift) & 0xffff;
    order_out[offset[d] + bases[(p / RP_TILE) * Dp + d] + rank[p]] = i;  // a permutation of 0..N: the counts are of these same digits
}

__global__ void __launch_bounds__(RP_PT) k_rw_last_write(const RwSlot* __restrict__ slots, uint32_t n_slots, uint32_t N, const uint32_t* __restrict__ order,
                                                         uint32_t* __restrict__ blast) {
    __shared__ uint32_t wmax[RW_WAVES];
    const size_t base = (size_t)blockIdx.x * RW_BLOCK;
    uint32_t m = 0;
#pragma unroll 4
    for (int it = 0; it < RW_ROWS; it++) {
        const size_t q = base + (size_t)(it * RP_PT) + threadIdx.x;
        if (q < N) {
            const uint32_t i = order[q], j = i / n_slots, s = i - j * n_slots;
            if (rw_writes(slots[s], j)) m = (uint32_t)q + 1;  // q grows with it
        }
    }
    for (int off = 32; off; off >>= 1) {
        const uint32_t y = __shfl_xor(m, off);
        m = m > y ? m : y;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RW_WAVES; w++) m = m > wmax[w] ? m : wmax[w];
        blast[blockIdx.x] = m;
    }
}

// blast[0..nb) -> bcarry: the last write before each block (exclusive max-scan)
__global__ void __launch_bounds__(RP_SCAN_PT) k_rw_carry(size_t nb, const uint32_t* __restrict__ blast, uint32_t* __restrict__ bcarry) {
    __shared__ uint32_t sh[RP_SCAN_PT];
    uint32_t carry = 0;
    for (size_t c = 0; c < nb; c += RP_SCAN_PT) {  // uniform over the workgroup
        const size_t b = c + threadIdx.x;
        uint32_t total;
        const uint32_t excl = rw_block_scan<true>(b < nb ? blast[b] : 0, sh, &total);
        if (b < nb) bcarry[b] = carry > excl ? carry : excl;
        carry = carry > total ? carry : total;
    }
}

__global__ void __launch_bounds__(RP_PT) k_rw_gather(const RwSlot* __restrict__ slots, uint32_t n_slots, uint32_t N, uint32_t MEM, const uint32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ bcarry, const uint32_t* __restrict__ v_init, uint32_t* __restrict__ v_final,
                                                     uint32_t* __restrict__ t_final) {
    __shared__ uint32_t wlast[2][RW_WAVES];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    const size_t base = (size_t)blockIdx.x * RW_BLOCK;
    uint32_t carry = bcarry[blockIdx.x];  // the last write before the row, + 1 (0: none): the same value in every thread
    for (int it = 0; it < RW_ROWS; it++) {  // every bound of this loop is uniform over the workgroup
        const size_t row = base + (size_t)(it * RP_PT);
        if (row >= N) break;
        const size_t q = row + threadIdx.x;
        const bool valid = q < N;
        uint32_t i = 0, j = 0, s = 0, a = 0;
        bool w = false;
        if (valid) {
            i = order[q];
            j = i / n_slots;
            s = i - j * n_slots;
            a = rw_addr(slots[s], j, MEM);
            w = rw_writes(slots[s], j);
        }
        const unsigned long long b = __ballot(w);
        if (lane == 0) wlast[it & 1][wave] = b ? (uint32_t)(row + wave * 64 + (63 - __clzll((long long)b))) + 1 : 0;
        __syncthreads();  // one barrier per row: row it + 2 rewrites wlast[it & 1] only after every thread has left row it + 1's
        uint32_t prev = carry;
#pragma unroll
        for (int k = 0; k < RW_WAVES; k++) {
            const uint32_t x = wlast[it & 1][k];
            if (x) {
                carry = x;
                if (k < (int)wave) prev = x;
            }
        }
        const unsigned long long mine = b & below;
        if (mine) prev = (uint32_t)(row + wave * 64 + (63 - __clzll((long long)mine))) + 1;
        if (!valid) continue;  // no barrier and no ballot below
        const RwSlot sl = slots[s];
        // the last write before q, if it is to this address; else the initial word
        uint32_t vr = v_init[a];
        if (prev) {
            const uint32_t ip = order[prev - 1], jp = ip / n_slots, sp = ip - jp * n_slots;
            if (rw_addr(slots[sp], jp, MEM) == a) vr = slots[sp].vw[jp];
        }
        // the previous access is the sorted neighbour
        uint32_t tr = 0;
        if (q > 0) {
            const uint32_t in = order[q - 1], jn = in / n_slots, sn = in - jn * n_slots;
            if (rw_addr(slots[sn], jn, MEM) == a) tr = jn;
        }
        const uint32_t vw = w ? sl.vw[j] : vr;
        sl.vr[j] = vr;
        sl.tr[j] = tr;
        if (sl.vwr) sl.vwr[j] = vw;
        bool last = q + 1 == N;
        if (!last) {
            const uint32_t in = order[q + 1], jn = in / n_slots, sn = in - jn * n_slots;
            last = rw_addr(slots[sn], jn, MEM) != a;
        }
        if (last) {
            v_final[a] = vw;
            t_final[a] = j;
        }
    }
}

extern "C" {

int cozk_rw_memory_witness(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_vec* const* v_write, const cozk_vec* const* is_write, size_t n_slots,
                           const cozk_vec* v_init, cozk_vec** v_read, cozk_vec** t_read, cozk_vec** v_written, cozk_vec** v_final, cozk_vec** t_final) {
    if (!v_read || !t_read || !v_written || !v_final || !t_final) return COZK_ERR_INVALID_ARG;
    *v_final = *t_final = nullptr;
    if (n_slots <= RW_MAX_SLOTS)
        for (size_t s = 0; s < n_slots; s++) v_read[s] = t_read[s] = v_written[s] = nullptr;
    size_t n = 0, MEM = 0;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && addr && v_init && n_slots >= 1 && n_slots <= RW_MAX_SLOTS, "rw_memory_witness: ctx, addr, v_init; 1 <= n_slots <= 8");
        for (size_t s = 0; s < n_slots; s++) {
            COZK_REQUIRE(addr[s] && (addr[s]->kind == COZK_SCALAR_U8 || addr[s]->kind == COZK_SCALAR_U32), "rw_memory_witness: addr[s] is a U8 or U32 vector");
            COZK_REQUIRE(addr[s]->n == addr[0]->n, "rw_memory_witness: addr[s] has n entries (one length for every slot)");
        }
        n = addr[0]->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32) && n * n_slots < ((size_t)1 << 32), "rw_memory_witness: 1 <= n and n * n_slots < 2^32");
        COZK_REQUIRE(v_init->kind == COZK_SCALAR_U32, "rw_memory_witness: v_init is a U32 vector");
        MEM = v_init->n;
        COZK_REQUIRE(MEM >= 1 && MEM < ((size_t)1 << 32), "rw_memory_witness: 1 <= MEM < 2^32");
        for (size_t s = 0; s < n_slots; s++) {
            const cozk_vec* vw = v_write ? v_write[s] : nullptr;
            const cozk_vec* iw = is_write ? is_write[s] : nullptr;
            COZK_REQUIRE(!iw || vw, "rw_memory_witness: is_write[s] given without v_write[s]");
            COZK_REQUIRE(!vw || vw->kind == COZK_SCALAR_U32, "rw_memory_witness: v_write[s] is a U32 vector");
            COZK_REQUIRE(!iw || iw->kind == COZK_SCALAR_U8, "rw_memory_witness: is_write[s] is a U8 vector");
            COZK_REQUIRE((!vw || vw->n == n) && (!iw || iw->n == n), "rw_memory_witness: v_write[s] and is_write[s] have n entries");
        }
    });
    if (rc != COZK_OK) return rc;
    for (size_t s = 0; s < n_slots && rc == COZK_OK; s++) {
        rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, &v_read[s]);
        if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, &t_read[s]);
        if (rc == COZK_OK && is_write && is_write[s]) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, &v_written[s]);
    }
    if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, MEM, COZK_SCALAR_U32, v_final);
    if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, MEM, COZK_SCALAR_U32, t_final);
    void *d_slots = nullptr, *d_ord[2] = {nullptr, nullptr}, *d_rank = nullptr, *d_hist = nullptr, *d_bases = nullptr, *d_count = nullptr, *d_blast = nullptr,
         *d_bcarry = nullptr, *d_viol = nullptr;
    if (rc == COZK_OK) rc = cozk_guard(ctx, [&] {
        RwSlot hs[RW_MAX_SLOTS];
        for (size_t s = 0; s < n_slots; s++)
            hs[s] = RwSlot{addr[s]->d, v_write && v_write[s] ? (const uint32_t*)v_write[s]->d : nullptr, is_write && is_write[s] ? (const uint8_t*)is_write[s]->d : nullptr,
                           (uint32_t*)v_read[s]->d, (uint32_t*)t_read[s]->d, v_written[s] ? (uint32_t*)v_written[s]->d : nullptr, addr[s]->kind == COZK_SCALAR_U8};
        const uint32_t N = (uint32_t)(n * n_slots), ns = (uint32_t)n_slots, mem = (uint32_t)MEM;
        const RadixPlan plan(N, MEM);
        const size_t tiles = plan.tiles, nb = ((size_t)N + RW_BLOCK - 1) / RW_BLOCK;
        const int passes = plan.passes;
        d_slots = ctx_dev_alloc(ctx, n_slots * sizeof(RwSlot));
        for (int k = 0; k < passes; k++) d_ord[k] = ctx_dev_alloc(ctx, (size_t)N * sizeof(uint32_t));
        d_rank = ctx_dev_alloc(ctx, (size_t)N * sizeof(uint16_t));
        d_hist = ctx_dev_alloc(ctx, tiles * plan.Dmax * sizeof(uint16_t));
        d_bases = ctx_dev_alloc(ctx, tiles * plan.Dmax * sizeof(uint32_t));
        d_count = ctx_dev_alloc(ctx, (size_t)plan.Dmax * sizeof(uint32_t));
        d_blast = ctx_dev_alloc(ctx, nb * sizeof(uint32_t));
        d_bcarry = ctx_dev_alloc(ctx, nb * sizeof(uint32_t));
        unsigned long long* viol = viol_begin(ctx, &d_viol);
        const RwSlot* ds = (const RwSlot*)d_slots;
        hipStream_t st = ctx->stream;
        HIP_TRY(hipMemcpyAsync(d_slots, hs, n_slots * sizeof(RwSlot), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync((*v_final)->d, v_init->d, MEM * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync((*t_final)->d, 0, MEM * sizeof(uint32_t), st));
        const unsigned pos_grid = (unsigned)(((size_t)N + RP_PT - 1) / RP_PT);
        for (int k = 0; k < passes; k++) {
            const uint32_t D = plan.D[k], Dp = plan.Dp(k);
            const uint32_t* in = k ? (const uint32_t*)d_ord[0] : nullptr;
            k_rw_rank<<<(unsigned)tiles, RP_PT, 0, st>>>(ds, ns, N, mem, in, 16 * k, Dp, plan.key_bits(k), (uint16_t*)d_rank, (uint16_t*)d_hist, viol);
            HIP_TRY(hipGetLastError());
            k_rw_scan<<<(D + RP_PT - 1) / RP_PT, RP_PT, 0, st>>>(D, Dp, tiles, (const uint16_t*)d_hist, (uint32_t*)d_bases, (uint32_t*)d_count);
            HIP_TRY(hipGetLastError());
            k_rw_offsets<<<1, RP_SCAN_PT, 0, st>>>(D, (uint32_t*)d_count);
            HIP_TRY(hipGetLastError());
            k_rw_scatter<<<pos_grid, RP_PT, 0, st>>>(ds, ns, N, mem, in, 16 * k, Dp, (const uint16_t*)d_rank, (const uint32_t*)d_bases, (const uint32_t*)d_count,
                                                    (uint32_t*)d_ord[k]);
            HIP_TRY(hipGetLastError());
        }
        const uint32_t* sorted = (const uint32_t*)d_ord[passes - 1];
        k_rw_last_write<<<(unsigned)nb, RP_PT, 0, st>>>(ds, ns, N, sorted, (uint32_t*)d_blast);
        HIP_TRY(hipGetLastError());
        k_rw_carry<<<1, RP_SCAN_PT, 0, st>>>(nb, (const uint32_t*)d_blast, (uint32_t*)d_bcarry);
        HIP_TRY(hipGetLastError());
        k_rw_gather<<<(unsigned)nb, RP_PT, 0, st>>>(ds, ns, N, mem, sorted, (const uint32_t*)d_bcarry, (const uint32_t*)v_init->d, (uint32_t*)(*v_final)->d,
                                                   (uint32_t*)(*t_final)->d);
        HIP_TRY(hipGetLastError());
        const unsigned long long bad = viol_read(ctx, viol);
        if (bad != ~0ull) {
            char buf[160];
            snprintf(buf, sizeof buf, "rw_memory_witness: step %llu, slot %llu: the address is >= MEM = %zu", bad >> 32, bad & 0xffffffffull, MEM);
            throw CozkError(COZK_ERR_INVALID_ARG, buf);
        }
    });
    for (void* p : {d_slots, d_ord[0], d_ord[1], d_rank, d_hist, d_bases, d_count, d_blast, d_bcarry, d_viol}) ctx_dev_free(ctx, p);
    if (rc != COZK_OK) {
        for (size_t s = 0; s < n_slots; s++)
            for (cozk_vec** v : {&v_read[s], &t_read[s], &v_written[s]}) {
                cozk_vec_free(*v);
                *v = nullptr;
            }
        for (cozk_vec** v : {v_final, t_final}) {
            cozk_vec_free(*v);
            *v = nullptr;
        }
    }
    return rc;
}

}  // extern "C"
