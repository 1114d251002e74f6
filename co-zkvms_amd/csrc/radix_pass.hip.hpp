// One stable 16-bit least-significant-digit radix pass over tiles of RP_TILE positions, shared by the read-write memory witness
// (rw_memory_witness.hip) and the time counters (ts_range_witness.hip); the scan of the tile histograms and the host helpers at the
// end also serve the Lasso lookup witness (lasso_witness.hip).  A pass over D digit values is
//   rank     rp_rank_tile: one workgroup per tile, a u16 table of D counters in LDS.  The tile goes in chunks of RP_CHUNK positions:
//            wave 0 walks a chunk's digits, staged in LDS, 64 at a time in position order (lw_walk_step) -> u16 in-tile rank per
//            position, while the other three waves stage the next chunk's digits; the table leaves as the tile's histogram.  The
//            digit of a position is the caller's: its callable gathers through the previous pass's order, decodes and checks the key.
//   scan     rp_scan_tiles: per digit value, exclusive scan of the tile histograms over the tiles -> u32 tile bases; returns the total
//   offsets  rp_offsets: one workgroup, exclusive scan of the totals over the digit values, in place
// and a scatter to offset[digit] + base[tile][digit] + rank, which is the caller's own.  The __global__ entry points stay in the
// callers' files (k_rw_*, k_ts_*, k_lasso_scan): thin wrappers that pick the column and the key.  The compiler sees through the digit
// callable: k_rw_rank and k_ts_rank keep the registers, LDS and occupancy they had as two hand-written copies.
#pragma once
#include "common.hpp"
#include "lasso_walk.hip.hpp"

static constexpr int RP_TILE = COZK_LASSO_TILE;  // positions per tile: in-tile ranks (< 32768) and counts (<= 32768) fit 16 bits
static constexpr int RP_PT = 256;
static constexpr int RP_CHUNK = 4096;            // digits staged in LDS at a time (two buffers: one walked, one being staged)
static constexpr int RP_SCAN_PT = 1024;          // the one-workgroup scans
static constexpr int RP_SCAN_ROWS = 65536 / RP_SCAN_PT;
static_assert(RP_SCAN_ROWS * (RP_SCAN_PT / 64) == RP_SCAN_PT, "rp_offsets scans one (row, wave) total per thread");
static_assert(RP_TILE <= 32768 && RP_TILE % RP_CHUNK == 0 && RP_CHUNK % 64 == 0, "in-tile counts must fit 16 bits");

// The walk of tile `tile` of a column of n positions, by a workgroup of RP_PT threads: rank[p] = the number of earlier positions of
// the tile with the digit of p, hist_row[0..Dp) = the tile's count of every digit value.  digit(p) -> uint16_t, below 2^key_bits.
template <class Digit>
__device__ __forceinline__ void rp_rank_tile(size_t tile, size_t n, Digit digit, uint32_t Dp, int key_bits, uint16_t* __restrict__ rank,
                                             uint16_t* __restrict__ hist_row) {
    __shared__ uint16_t tab[65536];
    __shared__ uint16_t keys[2][RP_CHUNK];
    uint32_t* tab32 = reinterpret_cast<uint32_t*>(tab);
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < Dp / 2; i += RP_PT) tab32[i] = 0;
    const size_t begin = tile * (size_t)RP_TILE, end = begin + RP_TILE < n ? begin + RP_TILE : n;
    // the digits of the chunk at c0, by the threads first, first + stride, ...
    auto stage = [&](size_t c0, uint16_t* dst, unsigned first, unsigned stride) {
#pragma unroll 4
        for (uint32_t e = first; e < (uint32_t)RP_CHUNK; e += stride) {
            const size_t p = c0 + e;
            if (p < end) dst[e] = digit(p);
        }
    };
    stage(begin, keys[0], threadIdx.x, RP_PT);
    __syncthreads();  // the first chunk's digits are staged and the table is clear
    int cur = 0;
    for (size_t c0 = begin; c0 < end; c0 += RP_CHUNK, cur ^= 1) {  // every bound of this loop is uniform over the workgroup
        if (wave == 0) {
            const uint32_t cnt = end - c0 < (size_t)RP_CHUNK ? (uint32_t)(end - c0) : (uint32_t)RP_CHUNK;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
                const bool valid = k0 + lane < cnt;
                const uint32_t r = lw_walk_step(tab, valid, valid ? keys[cur][k0 + lane] : 0, key_bits, lane);
                if (valid) rank[c0 + k0 + lane] = (uint16_t)r;
            }
        } else if (c0 + RP_CHUNK < end) {  // the other waves stage the next chunk beside the walk
            stage(c0 + RP_CHUNK, keys[cur ^ 1], threadIdx.x - 64, RP_PT - 64);
        }
        __syncthreads();  // the walk has left keys[cur], which the chunk after the next one rewrites; keys[cur ^ 1] is staged
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(hist_row);
    for (uint32_t i = threadIdx.x; i < Dp / 2; i += RP_PT) out[i] = tab32[i];
}

// One digit value's exclusive scan over the tiles: hist and bases point at the value's entry of tile 0, the rows are Dp apart
__device__ __forceinline__ uint32_t rp_scan_tiles(size_t tiles, uint32_t Dp, const uint16_t* __restrict__ hist, uint32_t* __restrict__ bases) {
    uint32_t run = 0;
    for (size_t t = 0; t < tiles; t++) {
        bases[t * Dp] = run;
        run += hist[t * Dp];
    }
    return run;
}

// inclusive scan (sum, or max) over the RP_SCAN_PT threads of the workgroup; returns the exclusive value, *total = the whole
template <bool MAX>
__device__ __forceinline__ uint32_t rw_block_scan(uint32_t x, uint32_t* sh, uint32_t* total) {
    const unsigned t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (unsigned off = 1; off < RP_SCAN_PT; off <<= 1) {
        const uint32_t y = t >= off ? sh[t - off] : 0;
        __syncthreads();
        x = MAX ? (x > y ? x : y) : x + y;
        sh[t] = x;
        __syncthreads();
    }
    *total = sh[RP_SCAN_PT - 1];
    const uint32_t excl = t ? sh[t - 1] : 0;
    __syncthreads();
    return excl;
}

// count[0..D) -> its exclusive prefix sums, in place, D <= 65536, by a workgroup of RP_SCAN_PT threads: up to RP_SCAN_ROWS rows of
// RP_SCAN_PT values, a value per thread and row (coalesced).  A wave scan per row leaves each value's prefix inside its wave in
// place; one workgroup scan over the (row, wave) totals, which are in the order of the values; then every value takes the prefix of
// its wave.
__device__ __forceinline__ void rp_offsets(uint32_t D, uint32_t* __restrict__ count) {
    __shared__ uint32_t sh[RP_SCAN_PT], pre[RP_SCAN_PT];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = (int)((D + RP_SCAN_PT - 1) / RP_SCAN_PT);  // uniform over the workgroup
    pre[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < rows; r++) {
        const uint32_t d = (uint32_t)r * RP_SCAN_PT + threadIdx.x;
        const uint32_t x = d < D ? count[d] : 0;
        uint32_t v = x;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(v, off);
            if ((int)lane >= off) v += y;
        }
        if (d < D) count[d] = v - x;
        if (lane == 63) pre[r * (RP_SCAN_PT / 64) + wave] = v;
    }
    __syncthreads();
    uint32_t total;
    const uint32_t before = rw_block_scan<false>(pre[threadIdx.x], sh, &total);
    pre[threadIdx.x] = before;  // every thread has read its total before rw_block_scan's first barrier
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < rows; r++) {
        const uint32_t d = (uint32_t)r * RP_SCAN_PT + threadIdx.x;
        if (d < D) count[d] += pre[r * (RP_SCAN_PT / 64) + wave];
    }
}

// The passes over `positions` keys below M: one for M <= 65536, two above, the second over the high digit's actual range
struct RadixPlan {
    int passes;
    uint32_t D[2];  // digit values of each pass (D[1] = 0 for one pass)
    uint32_t Dmax;  // the larger, rounded up to even: what a histogram row is allocated for
    size_t tiles;
    RadixPlan(size_t positions, size_t M) : passes(M > 65536 ? 2 : 1), tiles((positions + RP_TILE - 1) / RP_TILE) {
        D[0] = M < 65536 ? (uint32_t)M : 65536u;
        D[1] = passes == 2 ? (((uint32_t)M - 1) >> 16) + 1 : 0u;
        Dmax = ((D[0] > D[1] ? D[0] : D[1]) + 1) & ~1u;
    }
    uint32_t Dp(int k) const { return (D[k] + 1) & ~1u; }  // row stride of the histograms: whole 32-bit words
    int key_bits(int k) const {
        int b = 0;
        while (((uint32_t)1 << b) < D[k]) b++;
        return b;
    }
};

// The columns go in batches whose tile histograms (u16) and bases (u32) stay under `cap` bytes; one column is the least
static inline size_t radix_batch(size_t cap, size_t tiles, uint32_t D, size_t cols) {
    const size_t batch = cap / (tiles * D * (sizeof(uint16_t) + sizeof(uint32_t)));
    return batch < 1 ? 1 : (batch > cols ? cols : batch);
}

// The device word through which kernels report the smallest violation (atomicMin): viol_begin allocates it into *d (the caller
// frees it with ctx_dev_free) and sets it to all ones on the stream; viol_read, after the launches, returns it (~0: no violation).
static inline unsigned long long* viol_begin(cozk_ctx* ctx, void** d) {
    *d = ctx_dev_alloc(ctx, sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(*d, 0xff, sizeof(unsigned long long), ctx->stream));
    return (unsigned long long*)*d;
}
static inline unsigned long long viol_read(cozk_ctx* ctx, const unsigned long long* d) {
    unsigned long long* pin = (unsigned long long*)ctx_pinned(ctx, sizeof(unsigned long long));
    HIP_TRY(hipMemcpyAsync(pin, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return *pin;
}
