// The dealer's Lasso lookup witness on the device: read_cts / final_cts / E of every memory of the instruction lookups
// (co-jolt/src/jolt/vm/instruction_lookups/witness.rs:85-150, one sequential walk per memory over the whole trace) as three
// batched launches over (tile, memory).  For one memory with addresses addr[0..n), 0/1 flags and a subtable of M entries:
//
//   read_cts[j]  = #{ j' < j : flag[j'] = 1, addr[j'] = addr[j] }   if flag[j] = 1, else 0
//   final_cts[a] = #{ j : flag[j] = 1, addr[j] = a }
//   E[j]         = subtable[addr[j]]                                 if flag[j] = 1, else 0
//
// The counters follow TIME order (the reference's polynomial, and the only deterministic one), so nothing here ranks by the
// return order of an atomic: the flagged steps of a tile of LW_TILE consecutive steps are walked by ONE wave, 64 at a time in
// step order, and what the other waves do for it (loading, compacting) keeps that order by construction.
//
//   k_lasso_rank    one workgroup per (tile, memory), a u16 table of M counters in LDS (128 KiB at M = 2^16).  The tile goes in
//                   chunks of LW_CHUNK steps: all 256 threads load the chunk's flags and flagged addresses and compact the
//                   flagged steps, in step order (wave ballots + the four waves' counts), into an LDS list -- a memory is live
//                   at ~6 % of a Jolt trace's steps, and the walk should not pay for the rest.  Wave 0 then walks the list: the
//                   lanes with equal addresses find each other with one ballot per key bit; the lowest lane of a group reads and
//                   bumps the table (distinct leaders have distinct addresses: no atomic), the group takes the old value by
//                   shuffle and adds the number of its lower lanes.  read_cts <- the in-tile rank of the flagged steps; the table
//                   leaves as the tile's histogram.
//   k_lasso_scan    per (memory, address): exclusive scan of the tile histograms over the tiles -> u32 tile bases; total -> final_cts
//                   (rp_scan_tiles of radix_pass.hip.hpp, the scan of the read-write and timestamp witnesses' sort)
//   k_lasso_finish  per (step, memory): read_cts += base[tile][addr], E <- subtable[addr]; both 0 where the flag is off
//
// A flagged address >= M is skipped by every kernel (no load or store leaves its buffer) and reported through one device word,
// the smallest (memory, step) of a violation (an atomicMin: its result does not depend on the order of arrival).
#include "common.hpp"
#include "radix_pass.hip.hpp"  // the wave step of the walk (lw_walk_step), the scan over the tiles, the pass plan, the violation word

static constexpr int LW_TILE = RP_TILE;  // steps per tile: in-tile ranks and counts (<= 32768) fit 16 bits
static constexpr uint32_t LW_MAX_M = 65536;
static constexpr int LW_PT = 256;
static constexpr int LW_WAVES = LW_PT / 64;
static constexpr int LW_CHUNK = 4096;                          // steps compacted at a time: list entries = address | index in the chunk << 16
static constexpr int LW_PER = LW_CHUNK / LW_PT;                // ... per thread
static constexpr size_t LW_TRANSIENT_CAP = (size_t)256 << 20;  // tile histograms + tile bases of one batch of memories
static_assert(LW_TILE <= 32768 && LW_TILE % LW_CHUNK == 0 && LW_CHUNK <= 65536, "in-tile counts and chunk indices must fit 16 bits");

struct LwMem {
    const uint32_t* addr;
    const uint8_t* flag;  // null: used at every step
    const uint32_t* sub;
    uint32_t *rc, *E, *fc;
};

__global__ void __launch_bounds__(LW_PT) k_lasso_rank(const LwMem* __restrict__ mems, size_t n, uint32_t M, uint32_t Mp, int key_bits, uint32_t mem0,
                                                      uint16_t* __restrict__ hist, unsigned long long* __restrict__ viol) {
    __shared__ uint16_t tab[LW_MAX_M];
    __shared__ uint32_t list[LW_CHUNK];
    __shared__ uint32_t wcnt[2][LW_WAVES];
    uint32_t* tab32 = reinterpret_cast<uint32_t*>(tab);
    const LwMem mm = mems[blockIdx.y];
    const size_t tile = blockIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t i = threadIdx.x; i < Mp / 2; i += LW_PT) tab32[i] = 0;
    const size_t begin = tile * (size_t)LW_TILE, end = begin + LW_TILE < n ? begin + LW_TILE : n;
    for (size_t c0 = begin; c0 < end; c0 += LW_CHUNK) {  // every bound of these loops is uniform over the workgroup
        uint32_t a[LW_PER];
        bool on[LW_PER];
#pragma unroll
        for (int it = 0; it < LW_PER; it++) {
            const size_t j = c0 + (size_t)(it * LW_PT) + threadIdx.x;
            on[it] = j < end && (mm.flag ? mm.flag[j] != 0 : true);
            a[it] = on[it] ? mm.addr[j] : 0;
        }
        uint32_t cnt = 0;  // flagged steps of the chunk so far: the same value in every thread
#pragma unroll
        for (int it = 0; it < LW_PER; it++) {
            const uint32_t e = (uint32_t)(it * LW_PT) + threadIdx.x;
            const bool bad = on[it] && a[it] >= M;
            if (bad) atomicMin(viol, ((unsigned long long)(mem0 + blockIdx.y) << 32) | (unsigned long long)(c0 + e));
            const bool valid = on[it] && !bad;
            const unsigned long long b = __ballot(valid);
            if (lane == 0) wcnt[it & 1][wave] = (uint32_t)__popcll(b);
            __syncthreads();  // one barrier per pass: pass it + 2 rewrites wcnt[it & 1] only after every thread has left pass it + 1's
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < LW_WAVES; w++) {
                const uint32_t c = wcnt[it & 1][w];
                total += c;
                before += w < (int)wave ? c : 0;
            }
            if (valid) list[cnt + before + (uint32_t)__popcll(b & below)] = a[it] | (e << 16);
            cnt += total;
        }
        __syncthreads();  // the list is complete (and, in the first chunk, the table is clear)
        if (wave == 0) {
            for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
                const bool valid = k0 + lane < cnt;
                const uint32_t x = valid ? list[k0 + lane] : 0;
                const uint32_t rank = lw_walk_step(tab, valid, x & 0xffff, key_bits, lane);
                if (valid) mm.rc[c0 + (x >> 16)] = rank;
            }
        }
        __syncthreads();  // the next chunk rewrites the list
    }
    __syncthreads();
    uint32_t* out = reinterpret_cast<uint32_t*>(hist + ((size_t)blockIdx.y * gridDim.x + tile) * Mp);
    for (uint32_t i = threadIdx.x; i < Mp / 2; i += LW_PT) out[i] = tab32[i];
}

__global__ void __launch_bounds__(LW_PT) k_lasso_scan(const LwMem* __restrict__ mems, uint32_t M, uint32_t Mp, size_t tiles, const uint16_t* __restrict__ hist,
                                                      uint32_t* __restrict__ bases) {
    const uint32_t a = blockIdx.x * LW_PT + threadIdx.x;
    if (a >= M) return;
    const size_t row = (size_t)blockIdx.y * tiles * Mp + a;
    mems[blockIdx.y].fc[a] = rp_scan_tiles(tiles, Mp, hist + row, bases + row);
}

// the rank kernel wrote read_cts at the flagged steps only: this one writes every step
__global__ void __launch_bounds__(LW_PT) k_lasso_finish(const LwMem* __restrict__ mems, size_t n, uint32_t M, uint32_t Mp, size_t tiles,
                                                        const uint32_t* __restrict__ bases) {
    const size_t j = (size_t)blockIdx.x * LW_PT + threadIdx.x;
    if (j >= n) return;
    const LwMem mm = mems[blockIdx.y];
    uint32_t rc = 0, e = 0;
    if (mm.flag ? mm.flag[j] != 0 : true) {  // an unflagged step's address is never used as an index
        const uint32_t a = mm.addr[j];
        if (a < M) {
            rc = mm.rc[j] + bases[((size_t)blockIdx.y * tiles + j / LW_TILE) * Mp + a];
            e = mm.sub[a];
        }
    }
    mm.rc[j] = rc;
    mm.E[j] = e;
}

extern "C" {

int cozk_lasso_witness(cozk_ctx* ctx, const cozk_vec* const* dims, size_t n_dims, const cozk_vec* const* subtables, size_t n_subtables, const cozk_vec* const* flags,
                       const int* mem_dim, const int* mem_subtable, size_t n_mem, cozk_vec** read_cts, cozk_vec** E, cozk_vec** final_cts) {
    if (!read_cts || !E || !final_cts) return COZK_ERR_INVALID_ARG;
    size_t n = 0, M = 0;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && dims && subtables && flags && mem_dim && mem_subtable && n_dims >= 1 && n_subtables >= 1 && n_mem >= 1 && n_mem <= 65535,
                     "lasso_witness: dims, subtables, flags, mem_dim, mem_subtable; 1 <= n_mem <= 65535");
        for (size_t m = 0; m < n_mem; m++) read_cts[m] = E[m] = final_cts[m] = nullptr;
        for (size_t d = 0; d < n_dims; d++)
            COZK_REQUIRE(dims[d] && dims[d]->kind == COZK_SCALAR_U32 && dims[d]->n == dims[0]->n, "lasso_witness: dims[d] (U32, one length n)");
        n = dims[0]->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), "lasso_witness: 1 <= n < 2^32");
        for (size_t s = 0; s < n_subtables; s++)
            COZK_REQUIRE(subtables[s] && subtables[s]->kind == COZK_SCALAR_U32 && subtables[s]->n == subtables[0]->n, "lasso_witness: subtables[s] (U32, one length M)");
        M = subtables[0]->n;
        COZK_REQUIRE(M >= 1 && M <= LW_MAX_M, "lasso_witness: 1 <= M <= 65536");
        for (size_t m = 0; m < n_mem; m++) {
            COZK_REQUIRE(!flags[m] || (flags[m]->kind == COZK_SCALAR_U8 && flags[m]->n == n), "lasso_witness: flags[m] (U8, n entries, or NULL)");
            COZK_REQUIRE(mem_dim[m] >= 0 && (size_t)mem_dim[m] < n_dims, "lasso_witness: mem_dim[m] in 0..n_dims");
            COZK_REQUIRE(mem_subtable[m] >= 0 && (size_t)mem_subtable[m] < n_subtables, "lasso_witness: mem_subtable[m] in 0..n_subtables");
        }
    });
    if (rc != COZK_OK) return rc;
    for (size_t m = 0; m < n_mem && rc == COZK_OK; m++) {
        rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, &read_cts[m]);
        if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, &E[m]);
        if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, M, COZK_SCALAR_U32, &final_cts[m]);
    }
    void *d_mems = nullptr, *d_hist = nullptr, *d_bases = nullptr, *d_viol = nullptr;
    if (rc == COZK_OK) rc = cozk_guard(ctx, [&] {
        std::vector<LwMem> hm(n_mem);
        for (size_t m = 0; m < n_mem; m++)
            hm[m] = LwMem{(const uint32_t*)dims[mem_dim[m]]->d, flags[m] ? (const uint8_t*)flags[m]->d : nullptr, (const uint32_t*)subtables[mem_subtable[m]]->d,
                          (uint32_t*)read_cts[m]->d, (uint32_t*)E[m]->d, (uint32_t*)final_cts[m]->d};
        const RadixPlan plan(n, M);  // one pass: M <= 65536
        const size_t tiles = plan.tiles;
        const uint32_t Mp = plan.Dp(0);
        const int key_bits = plan.key_bits(0);
        const size_t batch = radix_batch(LW_TRANSIENT_CAP, tiles, Mp, n_mem);
        d_mems = ctx_dev_alloc(ctx, n_mem * sizeof(LwMem));
        d_hist = ctx_dev_alloc(ctx, batch * tiles * Mp * sizeof(uint16_t));
        d_bases = ctx_dev_alloc(ctx, batch * tiles * Mp * sizeof(uint32_t));
        unsigned long long* viol = viol_begin(ctx, &d_viol);
        HIP_TRY(hipMemcpyAsync(d_mems, hm.data(), n_mem * sizeof(LwMem), hipMemcpyHostToDevice, ctx->stream));
        for (size_t m0 = 0; m0 < n_mem; m0 += batch) {
            const unsigned nb = (unsigned)(n_mem - m0 < batch ? n_mem - m0 : batch);
            const LwMem* dm = (const LwMem*)d_mems + m0;
            k_lasso_rank<<<dim3((unsigned)tiles, nb), LW_PT, 0, ctx->stream>>>(dm, n, (uint32_t)M, Mp, key_bits, (uint32_t)m0, (uint16_t*)d_hist, viol);
            HIP_TRY(hipGetLastError());
            k_lasso_scan<<<dim3((unsigned)((M + LW_PT - 1) / LW_PT), nb), LW_PT, 0, ctx->stream>>>(dm, (uint32_t)M, Mp, tiles, (const uint16_t*)d_hist, (uint32_t*)d_bases);
            HIP_TRY(hipGetLastError());
            k_lasso_finish<<<dim3((unsigned)((n + LW_PT - 1) / LW_PT), nb), LW_PT, 0, ctx->stream>>>(dm, n, (uint32_t)M, Mp, tiles, (const uint32_t*)d_bases);
            HIP_TRY(hipGetLastError());
        }
        const unsigned long long bad = viol_read(ctx, viol);
        if (bad != ~0ull) {
            char buf[160];
            snprintf(buf, sizeof buf, "lasso_witness: memory %llu, step %llu: a flagged address is >= M = %zu", bad >> 32, bad & 0xffffffffull, M);
            throw CozkError(COZK_ERR_INVALID_ARG, buf);
        }
    });
    for (void* p : {d_mems, d_hist, d_bases, d_viol}) ctx_dev_free(ctx, p);
    if (rc != COZK_OK)
        for (size_t m = 0; m < n_mem; m++) {
            for (cozk_vec** v : {&read_cts[m], &E[m], &final_cts[m]}) {
                cozk_vec_free(*v);
                *v = nullptr;
            }
        }
    return rc;
}

size_t cozk_lasso_tile(void) { return (size_t)LW_TILE; }

}  // extern "C"
