// Lasso counters over an identity table of any length (cozk_time_counters), and on top of them the dealer's timestamp range-check
// witness (cozk_timestamp_range_witness; jolt-core's TimestampRangeCheckPolynomials::generate_witness, whose four families
// co-jolt/src/jolt/vm/jolt/witness.rs:384-409 shares as public vectors).  jolt-core is not in the reference tree: the recurrence is
// restated from upstream knowledge (parity unpinned); the field names and the multiset identity of the memory checking pin it.
// cozk_bytecode_witness is the same counters over one column, the bytecode trace over a table of B rows, plus one gather (k_bc_gather).
// cozk_timestamp_range_leaves, at the end of this file, turns those families and t_read into the leaves of the range check's
// grand-product circuits in one launch (k_ts_range_leaves).
// For one column of keys key[0..n) over a table of M entries:
//
//   read_cts[j]  = #{ j' < j : key[j'] = key[j] }      (TIME order)
//   final_cts[a] = #{ j : key[j] = a }
//
// and the witness is these counters for two columns per slot, key = t_read[s][j] and key = j - t_read[s][j], derived where a kernel
// needs them and never stored.  cozk_lasso_witness keeps one u16 counter per table entry in LDS, which ends at M = 65536; here the
// steps of a column are sorted by key with the stable 16-bit radix passes of radix_pass.hip.hpp (the tile walk, the scan over the
// tiles, the offsets scan: shared with rw_memory_witness.hip), one pass for M <= 65536 and two above, the second over the high
// digit's actual range.  The column is a grid dimension of every launch.  The pass's entry points and what is this file's own, per
// pass, over tiles of RP_TILE positions and D digit values:
//   k_ts_rank       rp_rank_tile per (tile, column) with the digit of a position: the key of the step there (in the second pass a
//                   gather through the first pass's order), a column of the batch chosen by blockIdx.y.  The first pass also checks
//                   every key.
//   k_ts_scan       rp_scan_tiles per (digit value, column); total -> count
//   one pass:  count IS final_cts (the scan writes it there), and
//   k_ts_finish     per (step, column): read_cts = base[tile][key] + in-tile rank
//   two passes, per pass:
//   k_ts_offsets    rp_offsets per column over count[]
//   k_ts_scatter    per (position, column): order_out[offset[digit] + base[tile][digit] + rank] = the step at the position; the
//                   second pass also leaves the key there, so the sweep below reads its neighbours' keys in place
//   and a sweep over the sorted positions q of a column, final_cts starting as zeros:
//   k_ts_seg_start  a position whose predecessor has another key: final_cts[key] = q, the segment's start (distinct keys, distinct
//                   words: no atomic)
//   k_ts_seg_rank   read_cts[step at q] = q - start[key]
//   k_ts_seg_count  the last position of a segment: final_cts[key] = q - start[key] + 1 (the one thread that reads the word writes it)
//
// Nothing ranks by the return order of an atomic and no workgroup waits for another, so the outputs are bit-for-bit deterministic.
// A key that breaks its bound (key >= M; t_read[s][j] > j for the witness) is used as 0 by every kernel (no load or store leaves its
// buffer) and reported through one device word, the smallest (column, step) / (step, slot) of a violation (an atomicMin: its result
// does not depend on the order of arrival); the call then returns no vector.
//
// Transient device memory for a batch of B columns, with tiles = ceil(n / RP_TILE), D1 = min(M, 65536), D2 = ceil(M / 65536)
// (0 for one pass), D = max(D1, D2) rounded up to even:
//   B (6 tiles D histograms and bases + 2 n ranks), and for two passes B (4 D counts + 8 n sorted steps + 4 n sorted keys) more.
// B is the largest count that keeps 6 tiles D B under 256 MiB (one column at least):
//   96 MiB + 16 MiB + 98 MiB at n = 2^20, 8 columns (4 slots) and M = 2^20.
#include "common.hpp"
#include "radix_pass.hip.hpp"

static constexpr size_t TS_MAX_COLS = COZK_TIME_COUNTERS_MAX_COLS;
static constexpr size_t TS_TRANSIENT_CAP = (size_t)256 << 20;  // tile histograms + tile bases of one batch of columns
static_assert(2 * COZK_RW_MEMORY_MAX_SLOTS <= COZK_TIME_COUNTERS_MAX_COLS, "the witness is two columns per slot");

struct TsCol {
    const uint32_t* src;  // the keys, or t_read of the slot
    uint32_t *rc, *fc;
    uint32_t gmr;         // the key is j - src[j] (global minus read)
};

// the key of step j; one that breaks its bound is used as 0 everywhere (and reported by k_ts_rank).  ts: src is a t_read column,
// bound by src[j] <= j, which keeps both of its keys below n <= M; otherwise src is the key, bound by M
__device__ __forceinline__ uint32_t ts_key(const TsCol& col, uint32_t j, uint32_t M, int ts, bool* bad) {
    const uint32_t x = col.src[j];
    *bad = ts ? x > j : x >= M;
    return *bad ? 0 : (col.gmr ? j - x : x);
}

// order: the steps of every column of the batch in the order of the previous pass; null = step p at position p
__global__ void __launch_bounds__(RP_PT) k_ts_rank(const TsCol* __restrict__ cols, size_t n, uint32_t M, int ts, uint32_t col0, const uint32_t* __restrict__ order,
                                                   int shift, uint32_t Dp, int key_bits, uint16_t* __restrict__ rank, uint16_t* __restrict__ hist,
                                                   unsigned long long* __restrict__ viol) {
    const TsCol col = cols[blockIdx.y];
    const size_t tile = blockIdx.x, at = (size_t)blockIdx.y * n;
    auto digit = [&](size_t p) {
        const uint32_t j = order ? order[at + p] : (uint32_t)p;
        bool bad;
        const uint32_t key = ts_key(col, j, M, ts, &bad);
        if (!order && bad) {
            const unsigned long long c = col0 + blockIdx.y;
            atomicMin(viol, ts ? ((unsigned long long)j << 32) | (c >> 1) : (c << 32) | j);
        }
        return (uint16_t)(key >> shift);
    };
    rp_rank_tile(tile, n, digit, Dp, key_bits, rank + at, hist + ((size_t)blockIdx.y * gridDim.x + tile) * Dp);
}

// count: the batch's counts, `stride` words per column; null = the column's final_cts (one pass: D = M)
__global__ void __launch_bounds__(RP_PT) k_ts_scan(const TsCol* __restrict__ cols, uint32_t D, uint32_t Dp, size_t tiles, const uint16_t* __restrict__ hist,
                                                   uint32_t* __restrict__ bases, uint32_t* __restrict__ count, uint32_t stride) {
    const uint32_t d = blockIdx.x * RP_PT + threadIdx.x;
    if (d >= D) return;
    const size_t row = (size_t)blockIdx.y * tiles * Dp + d;
    const uint32_t run = rp_scan_tiles(tiles, Dp, hist + row, bases + row);
    if (count)
        count[(size_t)blockIdx.y * stride + d] = run;
    else
        cols[blockIdx.y].fc[d] = run;
}

__global__ void __launch_bounds__(RP_PT) k_ts_finish(const TsCol* __restrict__ cols, size_t n, uint32_t M, int ts, uint32_t Dp, size_t tiles,
                                                     const uint16_t* __restrict__ rank, const uint32_t* __restrict__ bases) {
    const size_t j = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (j >= n) return;
    const TsCol col = cols[blockIdx.y];
    bool bad;
    const uint32_t key = ts_key(col, (uint32_t)j, M, ts, &bad);
    col.rc[j] = bases[((size_t)blockIdx.y * tiles + j / RP_TILE) * Dp + key] + rank[(size_t)blockIdx.y * n + j];
}

// count: the batch's counts, `stride` words per column
__global__ void __launch_bounds__(RP_SCAN_PT) k_ts_offsets(uint32_t D, uint32_t* __restrict__ count, uint32_t stride) {
    rp_offsets(D, count + (size_t)blockIdx.x * stride);
}

// key_out: null, or where the keys go in the new order
__global__ void __launch_bounds__(RP_PT) k_ts_scatter(const TsCol* __restrict__ cols, size_t n, uint32_t M, int ts, const uint32_t* __restrict__ order, int shift,
                                                      uint32_t Dp, size_t tiles, const uint16_t* __restrict__ rank, const uint32_t* __restrict__ bases,
                                                      const uint32_t* __restrict__ offset, uint32_t stride, uint32_t* __restrict__ order_out,
                                                      uint32_t* __restrict__ key_out) {
    const size_t p = (size_t)blockIdx.x * RP_PT + threadIdx.x, at = (size_t)blockIdx.y * n;
    if (p >= n) return;
    const uint32_t j = order ? order[at + p] : (uint32_t)p;
    bool bad;
    const uint32_t key = ts_key(cols[blockIdx.y], j, M, ts, &bad);
    const uint32_t d = (key >> shift) & 0xffff;
    // a permutation of 0..n: the counts are of these same digits
    const size_t pos = at + offset[(size_t)blockIdx.y * stride + d] + bases[((size_t)blockIdx.y * tiles + p / RP_TILE) * Dp + d] + rank[at + p];
    order_out[pos] = j;
    if (key_out) key_out[pos] = key;
}

__global__ void __launch_bounds__(RP_PT) k_ts_seg_start(const TsCol* __restrict__ cols, size_t n, const uint32_t* __restrict__ skey) {
    const size_t q = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (q >= n) return;
    skey += (size_t)blockIdx.y * n;
    const uint32_t key = skey[q];
    if (q == 0 || skey[q - 1] != key) cols[blockIdx.y].fc[key] = (uint32_t)q;
}

__global__ void __launch_bounds__(RP_PT) k_ts_seg_rank(const TsCol* __restrict__ cols, size_t n, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ order) {
    const size_t q = (size_t)blockIdx.x * RP_PT + threadIdx.x, at = (size_t)blockIdx.y * n;
    if (q >= n) return;
    const TsCol col = cols[blockIdx.y];
    col.rc[order[at + q]] = (uint32_t)q - col.fc[skey[at + q]];
}

__global__ void __launch_bounds__(RP_PT) k_ts_seg_count(const TsCol* __restrict__ cols, size_t n, const uint32_t* __restrict__ skey) {
    const size_t q = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (q >= n) return;
    skey += (size_t)blockIdx.y * n;
    const uint32_t key = skey[q];
    if (q + 1 == n || skey[q + 1] != key) {
        uint32_t* fc = cols[blockIdx.y].fc;
        fc[key] = (uint32_t)q - fc[key] + 1;
    }
}

// The counters of the columns src[c] (gmr[c]: the key is j - src[c][j]) into NEW vectors at *rc[c] (U32[n]) and *fc[c] (U32[M]); on
// any failure all of them are null.  who names the caller: it words a violation, and TS_RANGE says that the columns are t_read columns,
// two per slot (see ts_key).
enum TsCaller { TS_TIME_COUNTERS, TS_RANGE, TS_BYTECODE };
static int ts_counters(cozk_ctx* ctx, TsCaller who, const std::vector<const cozk_vec*>& src, const std::vector<uint32_t>& gmr, size_t n, size_t M,
                       const std::vector<cozk_vec**>& rc_out, const std::vector<cozk_vec**>& fc_out) {
    const int ts = who == TS_RANGE;
    const size_t nc = src.size();
    int rc = COZK_OK;
    for (size_t c = 0; c < nc && rc == COZK_OK; c++) {
        rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_U32, rc_out[c]);
        if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, M, COZK_SCALAR_U32, fc_out[c]);
    }
    void *d_cols = nullptr, *d_ord[2] = {nullptr, nullptr}, *d_skey = nullptr, *d_rank = nullptr, *d_hist = nullptr, *d_bases = nullptr, *d_count = nullptr,
         *d_viol = nullptr;
    if (rc == COZK_OK) rc = cozk_guard(ctx, [&] {
        TsCol hc[TS_MAX_COLS];
        for (size_t c = 0; c < nc; c++) hc[c] = TsCol{(const uint32_t*)src[c]->d, (uint32_t*)(*rc_out[c])->d, (uint32_t*)(*fc_out[c])->d, gmr[c]};
        const uint32_t m = (uint32_t)M;
        const RadixPlan plan(n, M);
        const size_t tiles = plan.tiles;
        const int passes = plan.passes;
        const uint32_t Dmax = plan.Dmax;
        const size_t batch = radix_batch(TS_TRANSIENT_CAP, tiles, Dmax, nc);
        d_cols = ctx_dev_alloc(ctx, nc * sizeof(TsCol));
        d_rank = ctx_dev_alloc(ctx, batch * n * sizeof(uint16_t));
        d_hist = ctx_dev_alloc(ctx, batch * tiles * Dmax * sizeof(uint16_t));
        d_bases = ctx_dev_alloc(ctx, batch * tiles * Dmax * sizeof(uint32_t));
        if (passes == 2) {
            for (int k = 0; k < 2; k++) d_ord[k] = ctx_dev_alloc(ctx, batch * n * sizeof(uint32_t));
            d_skey = ctx_dev_alloc(ctx, batch * n * sizeof(uint32_t));
            d_count = ctx_dev_alloc(ctx, batch * Dmax * sizeof(uint32_t));
        }
        unsigned long long* viol = viol_begin(ctx, &d_viol);
        hipStream_t st = ctx->stream;
        HIP_TRY(hipMemcpyAsync(d_cols, hc, nc * sizeof(TsCol), hipMemcpyHostToDevice, st));
        const unsigned pos_grid = (unsigned)((n + RP_PT - 1) / RP_PT);
        uint16_t *rank = (uint16_t*)d_rank, *hist = (uint16_t*)d_hist;
        uint32_t *bases = (uint32_t*)d_bases, *count = (uint32_t*)d_count, *skey = (uint32_t*)d_skey;
        for (size_t c0 = 0; c0 < nc; c0 += batch) {
            const unsigned nb = (unsigned)(nc - c0 < batch ? nc - c0 : batch);
            const TsCol* dc = (const TsCol*)d_cols + c0;
            for (int k = 0; k < passes; k++) {
                const uint32_t D = plan.D[k], Dp = plan.Dp(k);
                const uint32_t* in = k ? (const uint32_t*)d_ord[0] : nullptr;
                k_ts_rank<<<dim3((unsigned)tiles, nb), RP_PT, 0, st>>>(dc, n, m, ts, (uint32_t)c0, in, 16 * k, Dp, plan.key_bits(k), rank, hist, viol);
                HIP_TRY(hipGetLastError());
                k_ts_scan<<<dim3((D + RP_PT - 1) / RP_PT, nb), RP_PT, 0, st>>>(dc, D, Dp, tiles, hist, bases, count, Dmax);
                HIP_TRY(hipGetLastError());
                if (passes == 1) {
                    k_ts_finish<<<dim3(pos_grid, nb), RP_PT, 0, st>>>(dc, n, m, ts, Dp, tiles, rank, bases);
                    HIP_TRY(hipGetLastError());
                    break;
                }
                k_ts_offsets<<<nb, RP_SCAN_PT, 0, st>>>(D, count, Dmax);
                HIP_TRY(hipGetLastError());
                k_ts_scatter<<<dim3(pos_grid, nb), RP_PT, 0, st>>>(dc, n, m, ts, in, 16 * k, Dp, tiles, rank, bases, count, Dmax, (uint32_t*)d_ord[k], k ? skey : nullptr);
                HIP_TRY(hipGetLastError());
            }
            if (passes == 2) {
                for (unsigned c = 0; c < nb; c++) HIP_TRY(hipMemsetAsync(hc[c0 + c].fc, 0, M * sizeof(uint32_t), st));
                k_ts_seg_start<<<dim3(pos_grid, nb), RP_PT, 0, st>>>(dc, n, skey);
                HIP_TRY(hipGetLastError());
                k_ts_seg_rank<<<dim3(pos_grid, nb), RP_PT, 0, st>>>(dc, n, skey, (const uint32_t*)d_ord[1]);
                HIP_TRY(hipGetLastError());
                k_ts_seg_count<<<dim3(pos_grid, nb), RP_PT, 0, st>>>(dc, n, skey);
                HIP_TRY(hipGetLastError());
            }
        }
        const unsigned long long bad = viol_read(ctx, viol);
        if (bad != ~0ull) {
            char buf[160];
            if (ts)
                snprintf(buf, sizeof buf, "timestamp_range_witness: step %llu, slot %llu: t_read is greater than the step", bad >> 32, bad & 0xffffffffull);
            else if (who == TS_BYTECODE)
                snprintf(buf, sizeof buf, "bytecode_witness: step %llu: a[step] is >= B = %zu", bad & 0xffffffffull, M);
            else
                snprintf(buf, sizeof buf, "time_counters: column %llu, step %llu: the key is >= M = %zu", bad >> 32, bad & 0xffffffffull, M);
            throw CozkError(COZK_ERR_INVALID_ARG, buf);
        }
    });
    for (void* p : {d_cols, d_ord[0], d_ord[1], d_skey, d_rank, d_hist, d_bases, d_count, d_viol}) ctx_dev_free(ctx, p);
    if (rc != COZK_OK)
        for (size_t c = 0; c < nc; c++)
            for (cozk_vec** v : {rc_out[c], fc_out[c]}) {
                cozk_vec_free(*v);
                *v = nullptr;
            }
    return rc;
}

// The gather of cozk_bytecode_witness: a thread per step reads row a[j] of the six table columns (address U32 or U64, bitflags U64, rd,
// rs1, rs2 U8, imm I64) into v_read[0..4], each in its column's kind, and v_imm[j] = from_i64(imm), the Montgomery word of the signed
// value (|v| lifted by one product, negated where v < 0).  It runs after the counters have checked every a[j] < B.
struct BcGather {
    const void* address;
    const uint64_t* bitflags;
    const uint8_t* reg[3];
    const int64_t* imm;
    void* v_address;
    uint64_t* v_bitflags;
    uint8_t* v_reg[3];
    fe* v_imm;
    int address_u64;
};
__global__ void __launch_bounds__(RP_PT) k_bc_gather(const uint32_t* __restrict__ a, size_t n, uint32_t B, BcGather g) {
    const size_t j = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (j >= n) return;
    uint32_t x = a[j];
    if (x >= B) x = 0;  // refused by the counters before this launch; no load leaves its buffer
    if (g.address_u64)
        ((uint64_t*)g.v_address)[j] = ((const uint64_t*)g.address)[x];
    else
        ((uint32_t*)g.v_address)[j] = ((const uint32_t*)g.address)[x];
    g.v_bitflags[j] = g.bitflags[x];
#pragma unroll
    for (int k = 0; k < 3; k++) g.v_reg[k][j] = g.reg[k][x];
    const int64_t v = g.imm[x];
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    fe m = Fr::zero();
    m.l[0] = (uint32_t)mag;
    m.l[1] = (uint32_t)(mag >> 32);
    m = Fr::to_mont(m);
    fe_store(g.v_imm + j, v < 0 ? Fr::neg(m) : m);
}

// The leaves of the range check's 6 n_slots + 1 grand-product circuits (cozk_timestamp_range_leaves; the layout is in cozk.h).  A
// thread makes the six leaves of one (slot, step) and, for slot 0, the init leaf: six products of a 32-bit integer with a constant
// (g1r = (gamma + 1) R and g2r = gamma^2 R, Montgomery forms lifted once more, so that the product with a plain integer is a
// Montgomery form), the rest additions.  The keys t_read and j - t_read and the step number j exist only in registers.
struct TsLeafCols {
    const uint32_t *t_read[COZK_RW_MEMORY_MAX_SLOTS], *rc_rt[COZK_RW_MEMORY_MAX_SLOTS], *rc_gmr[COZK_RW_MEMORY_MAX_SLOTS], *fc_rt[COZK_RW_MEMORY_MAX_SLOTS],
        *fc_gmr[COZK_RW_MEMORY_MAX_SLOTS];
};
__device__ __forceinline__ fe ts_small(uint32_t v) {
    fe x = Fr::zero();
    x.l[0] = v;
    return x;
}
__global__ void __launch_bounds__(RP_PT) k_ts_range_leaves(TsLeafCols a, uint32_t n_slots, size_t n, fe g1r, fe g2r, fe g2, fe tau, fe* __restrict__ out,
                                                           unsigned long long* __restrict__ viol) {
    const size_t j = (size_t)blockIdx.x * RP_PT + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = blockIdx.y;
    uint32_t x = a.t_read[s][j];
    if (x > (uint32_t)j) {
        atomicMin(viol, ((unsigned long long)j << 32) | s);
        x = 0;
    }
    const fe init = Fr::sub(Fr::mul(g1r, ts_small((uint32_t)j)), tau);  // h(j, 0)
    const fe xg = Fr::mul(g1r, ts_small(x));
    const fe rt = Fr::add(Fr::sub(xg, tau), Fr::mul(g2r, ts_small(a.rc_rt[s][j])));
    const fe gmr = Fr::add(Fr::sub(init, xg), Fr::mul(g2r, ts_small(a.rc_gmr[s][j])));  // (j - x)(gamma + 1) = j (gamma + 1) - x (gamma + 1)
    fe* o = out + j;
    fe_store(o + (size_t)(4 * s) * n, rt);
    fe_store(o + (size_t)(4 * s + 1) * n, Fr::add(rt, g2));
    fe_store(o + (size_t)(4 * s + 2) * n, gmr);
    fe_store(o + (size_t)(4 * s + 3) * n, Fr::add(gmr, g2));
    if (s == 0) fe_store(o + (size_t)(4 * n_slots) * n, init);
    fe_store(o + (size_t)(4 * n_slots + 1 + 2 * s) * n, Fr::add(init, Fr::mul(g2r, ts_small(a.fc_rt[s][j]))));
    fe_store(o + (size_t)(4 * n_slots + 2 + 2 * s) * n, Fr::add(init, Fr::mul(g2r, ts_small(a.fc_gmr[s][j]))));
}

extern "C" {

int cozk_timestamp_range_leaves(cozk_ctx* ctx, const cozk_vec* const* t_read, const cozk_vec* const* rc_rt, const cozk_vec* const* rc_gmr,
                                const cozk_vec* const* fc_rt, const cozk_vec* const* fc_gmr, size_t n_slots, const uint64_t gamma[4],
                                const uint64_t tau[4], cozk_vec* out, size_t offset) {
    void* d_viol = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t_read && rc_rt && rc_gmr && fc_rt && fc_gmr && gamma && tau && out, "timestamp_range_leaves: bad argument");
        COZK_REQUIRE(n_slots >= 1 && n_slots <= COZK_RW_MEMORY_MAX_SLOTS, "timestamp_range_leaves: 1 <= n_slots <= 8");
        TsLeafCols h{};
        const cozk_vec* const* fam[5] = {t_read, rc_rt, rc_gmr, fc_rt, fc_gmr};
        const uint32_t** dst[5] = {h.t_read, h.rc_rt, h.rc_gmr, h.fc_rt, h.fc_gmr};
        for (int f = 0; f < 5; f++)
            for (size_t s = 0; s < n_slots; s++) {
                const cozk_vec* v = fam[f][s];
                COZK_REQUIRE(v && v->kind == COZK_SCALAR_U32, "timestamp_range_leaves: every column is a U32 vector");
                COZK_REQUIRE(v->n == t_read[0]->n, "timestamp_range_leaves: every column has n entries (the table is as long as the trace: M == n)");
                dst[f][s] = (const uint32_t*)v->d;
            }
        const size_t n = t_read[0]->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), "timestamp_range_leaves: 1 <= n < 2^32");
        COZK_REQUIRE(out->kind == COZK_SCALAR_FR && offset <= out->n && (out->n - offset) / (6 * n_slots + 1) >= n,
                     "timestamp_range_leaves: out is an FR vector with room for (6 n_slots + 1) n entries from offset");
        fe g, t;
        for (int i = 0; i < 4; i++) {
            g.l[2 * i] = (uint32_t)gamma[i], g.l[2 * i + 1] = (uint32_t)(gamma[i] >> 32);
            t.l[2 * i] = (uint32_t)tau[i], t.l[2 * i + 1] = (uint32_t)(tau[i] >> 32);
        }
        const fe g2 = Fr::mul(g, g);
        unsigned long long* viol = viol_begin(ctx, &d_viol);
        hipStream_t st = ctx->stream;
        k_ts_range_leaves<<<dim3((unsigned)((n + RP_PT - 1) / RP_PT), (unsigned)n_slots), RP_PT, 0, st>>>(
            h, (uint32_t)n_slots, n, Fr::to_mont(Fr::add(g, Fr::one())), Fr::to_mont(g2), g2, t, (fe*)out->d + offset, viol);
        HIP_TRY(hipGetLastError());
        const unsigned long long bad = viol_read(ctx, viol);
        if (bad != ~0ull) {
            char buf[160];
            snprintf(buf, sizeof buf, "timestamp_range_leaves: step %llu, slot %llu: t_read is greater than the step", bad >> 32, bad & 0xffffffffull);
            throw CozkError(COZK_ERR_INVALID_ARG, buf);
        }
    });
    ctx_dev_free(ctx, d_viol);
    return rc;
}

int cozk_time_counters(cozk_ctx* ctx, const cozk_vec* const* keys, size_t n_cols, size_t M, cozk_vec** read_cts, cozk_vec** final_cts) {
    if (!read_cts || !final_cts) return COZK_ERR_INVALID_ARG;
    if (n_cols <= TS_MAX_COLS)
        for (size_t c = 0; c < n_cols; c++) read_cts[c] = final_cts[c] = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && keys && n_cols >= 1 && n_cols <= TS_MAX_COLS, "time_counters: ctx, keys; 1 <= n_cols <= 16");
        for (size_t c = 0; c < n_cols; c++) {
            COZK_REQUIRE(keys[c] && keys[c]->kind == COZK_SCALAR_U32, "time_counters: keys[c] is a U32 vector");
            COZK_REQUIRE(keys[c]->n == keys[0]->n, "time_counters: keys[c] has n entries (one length for every column)");
        }
        COZK_REQUIRE(keys[0]->n >= 1 && keys[0]->n < ((size_t)1 << 32), "time_counters: 1 <= n < 2^32");
        COZK_REQUIRE(M >= 1 && M < ((size_t)1 << 32), "time_counters: 1 <= M < 2^32");
    });
    if (rc != COZK_OK) return rc;
    std::vector<const cozk_vec*> src(keys, keys + n_cols);
    std::vector<cozk_vec**> rc_out(n_cols), fc_out(n_cols);
    for (size_t c = 0; c < n_cols; c++) rc_out[c] = &read_cts[c], fc_out[c] = &final_cts[c];
    return ts_counters(ctx, TS_TIME_COUNTERS, src, std::vector<uint32_t>(n_cols, 0), keys[0]->n, M, rc_out, fc_out);
}

int cozk_bytecode_witness(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* const* table, cozk_vec** v_read, cozk_vec** v_imm, cozk_vec** t_read,
                          cozk_vec** t_final) {
    if (!v_read || !v_imm || !t_read || !t_final) return COZK_ERR_INVALID_ARG;
    cozk_vec** outs[8] = {&v_read[0], &v_read[1], &v_read[2], &v_read[3], &v_read[4], v_imm, t_read, t_final};
    for (cozk_vec** o : outs) *o = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && a && table, "bytecode_witness: bad argument");
        COZK_REQUIRE(a->kind == COZK_SCALAR_U32, "bytecode_witness: a is a U32 vector");
        COZK_REQUIRE(a->n >= 1 && a->n < ((size_t)1 << 32), "bytecode_witness: 1 <= n < 2^32");
        for (int k = 0; k < 6; k++) COZK_REQUIRE(table[k], "bytecode_witness: six table columns");
        COZK_REQUIRE(table[0]->kind == COZK_SCALAR_U32 || table[0]->kind == COZK_SCALAR_U64, "bytecode_witness: table[0] (address) is a U32 or U64 vector");
        COZK_REQUIRE(table[1]->kind == COZK_SCALAR_U64, "bytecode_witness: table[1] (bitflags) is a U64 vector");
        for (int k = 2; k < 5; k++) COZK_REQUIRE(table[k]->kind == COZK_SCALAR_U8, "bytecode_witness: table[2..4] (rd, rs1, rs2) are U8 vectors");
        COZK_REQUIRE(table[5]->kind == COZK_SCALAR_I64, "bytecode_witness: table[5] (imm) is an I64 vector");
        for (int k = 1; k < 6; k++) COZK_REQUIRE(table[k]->n == table[0]->n, "bytecode_witness: every table column has B entries");
        COZK_REQUIRE(table[0]->n >= 1 && table[0]->n < ((size_t)1 << 32), "bytecode_witness: 1 <= B < 2^32");
    });
    if (rc != COZK_OK) return rc;
    const size_t n = a->n, B = table[0]->n;
    rc = ts_counters(ctx, TS_BYTECODE, {a}, {0}, n, B, {t_read}, {t_final});
    for (int k = 0; k < 5 && rc == COZK_OK; k++) rc = cozk_vec_alloc(ctx, n, table[k]->kind, &v_read[k]);
    if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_FR, v_imm);
    if (rc == COZK_OK) rc = cozk_guard(ctx, [&] {
        BcGather g{};
        g.address = table[0]->d, g.bitflags = (const uint64_t*)table[1]->d, g.imm = (const int64_t*)table[5]->d;
        g.v_address = v_read[0]->d, g.v_bitflags = (uint64_t*)v_read[1]->d, g.v_imm = (fe*)(*v_imm)->d;
        for (int k = 0; k < 3; k++) g.reg[k] = (const uint8_t*)table[2 + k]->d, g.v_reg[k] = (uint8_t*)v_read[2 + k]->d;
        g.address_u64 = table[0]->kind == COZK_SCALAR_U64;
        k_bc_gather<<<(unsigned)((n + RP_PT - 1) / RP_PT), RP_PT, 0, ctx->stream>>>((const uint32_t*)a->d, n, (uint32_t)B, g);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    });
    if (rc != COZK_OK)
        for (cozk_vec** o : outs) {
            cozk_vec_free(*o);
            *o = nullptr;
        }
    return rc;
}

int cozk_timestamp_range_witness(cozk_ctx* ctx, const cozk_vec* const* t_read, size_t n_slots, size_t M, cozk_vec** read_cts_read_timestamp,
                                 cozk_vec** read_cts_global_minus_read, cozk_vec** final_cts_read_timestamp, cozk_vec** final_cts_global_minus_read) {
    if (!read_cts_read_timestamp || !read_cts_global_minus_read || !final_cts_read_timestamp || !final_cts_global_minus_read) return COZK_ERR_INVALID_ARG;
    if (n_slots <= COZK_RW_MEMORY_MAX_SLOTS)
        for (size_t s = 0; s < n_slots; s++)
            read_cts_read_timestamp[s] = read_cts_global_minus_read[s] = final_cts_read_timestamp[s] = final_cts_global_minus_read[s] = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t_read && n_slots >= 1 && n_slots <= COZK_RW_MEMORY_MAX_SLOTS, "timestamp_range_witness: ctx, t_read; 1 <= n_slots <= 8");
        for (size_t s = 0; s < n_slots; s++) {
            COZK_REQUIRE(t_read[s] && t_read[s]->kind == COZK_SCALAR_U32, "timestamp_range_witness: t_read[s] is a U32 vector");
            COZK_REQUIRE(t_read[s]->n == t_read[0]->n, "timestamp_range_witness: t_read[s] has n entries (one length for every slot)");
        }
        COZK_REQUIRE(t_read[0]->n >= 1 && M < ((size_t)1 << 32), "timestamp_range_witness: 1 <= n and M < 2^32");
        COZK_REQUIRE(M >= t_read[0]->n, "timestamp_range_witness: M >= n (the table is as long as the padded trace)");
    });
    if (rc != COZK_OK) return rc;
    // column 2 s is slot s's read timestamp, column 2 s + 1 its global time minus the read timestamp (k_ts_rank names the slot so)
    std::vector<const cozk_vec*> src(2 * n_slots);
    std::vector<uint32_t> gmr(2 * n_slots);
    std::vector<cozk_vec**> rc_out(2 * n_slots), fc_out(2 * n_slots);
    for (size_t s = 0; s < n_slots; s++) {
        src[2 * s] = src[2 * s + 1] = t_read[s];
        gmr[2 * s] = 0, gmr[2 * s + 1] = 1;
        rc_out[2 * s] = &read_cts_read_timestamp[s], rc_out[2 * s + 1] = &read_cts_global_minus_read[s];
        fc_out[2 * s] = &final_cts_read_timestamp[s], fc_out[2 * s + 1] = &final_cts_global_minus_read[s];
    }
    return ts_counters(ctx, TS_RANGE, src, gmr, t_read[0]->n, M, rc_out, fc_out);
}

}  // extern "C"
