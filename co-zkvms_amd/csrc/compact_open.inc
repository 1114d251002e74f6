// Openings of compact public columns (U8 / U16 / U32 / U64 vectors) without an Fr copy of them -- part of poly.hip's translation unit.
//
//   cozk_compact_batch_evaluate_at_chi   out[c] = sum_i chi[i] * cols[c][i]        (cozk_poly_batch_evaluate_at_chi on PLAIN copies)
//   cozk_compact_linear_combination      out[i] = sum_c coeffs[c] * cols[c][i]     (cozk_poly_linear_combination, PLAIN)
//
// The Fr operand (chi[i], coeffs[c]) is in Montgomery form, x R mod r, and the column entry v is a plain integer, so the integer
// product (x R) * v is already the Montgomery form of x * v: no Montgomery reduction per term, and the sum of the integer products
// is reduced mod r ONCE.  A term is < 2^256 * 2^64 = 2^320.  The accumulator is the exact integer sum in CO_LIMBS = 11 limbs
// (352 bits), every carry propagated with its term (8 multiply-adds of 32 x 32 + 64 bits per 32-bit limb of v, which cannot
// overflow: (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1): nothing is left lazy but the reduction, and the bound is 2^32 terms per
// accumulator.  Both calls refuse n >= 2^32, so a lane, a wave and a workgroup (whose raw sums are added before the one reduction)
// all stay below it.  co_reduce: S = T0 + 2^256 T1 with T1 < 2^96, S mod r = to_mont(from_mont(T0)) + to_mont(T1), canonical --
// the same field element, hence the same bytes, as the sum of the reduced Montgomery products of the Fr calls.
//
// Evaluation: a workgroup row (blockIdx.y) carries CO_CB = 8 columns and reads chi[i] once for all of them: 88 accumulator registers
// per lane, 194 VGPRs, two waves per SIMD.  More columns per row read chi fewer times but lose more than that: 12, 16 and 24 columns
// per row (24 = one row for a whole call, 256 VGPRs + 255 AGPRs at one wave per SIMD, no scratch) all measured 1.5-1.8 times as
// long at 2^20 and 2^22 entries of 20 columns (DESIGN 4) -- the kernel is bound by its multiply-add chains, not by HBM, and chi's
// second and third reading comes from the caches.  The four waves' raw sums meet in LDS and the first lanes of the workgroup reduce
// one column each, so a workgroup pays the reduction's instructions once, not once per column and wave.  A lane carries at least
// CO_LANE_TERMS terms where n allows and the grid ends at CO_EVAL_GRID_MAX workgroups per row: 256 workgroups were the fastest
// at 2^20 entries and 512 at 2^22.

static constexpr int CO_MAX_COLS = COZK_COMPACT_MAX_COLS;
static constexpr int CO_LIMBS = 11;
static constexpr int CO_CB = 8;
static constexpr size_t CO_LANE_TERMS = 16;
static constexpr unsigned CO_EVAL_GRID_MAX = 512;

struct CompactCols {
    const void* p[CO_MAX_COLS];
    uint8_t kind[CO_MAX_COLS];
};
struct CompactLin {
    CompactCols cols;
    fe cf[CO_MAX_COLS];
};

// acc += a * v * 2^(32 OFF), exact
template <int OFF>
static __device__ __forceinline__ void co_mac(uint32_t (&acc)[CO_LIMBS], const fe& a, uint32_t v) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)a.l[k] * v + acc[OFF + k] + carry;  // <= 2^64 - 1
        acc[OFF + k] = (uint32_t)t;
        carry = t >> 32;
    }
#pragma unroll
    for (int k = OFF + 8; k < CO_LIMBS; k++) {
        const uint64_t t = (uint64_t)acc[k] + carry;
        acc[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
static __device__ __forceinline__ void co_mac_entry(uint32_t (&acc)[CO_LIMBS], const fe& a, uint64_t v, int kind) {
    co_mac<0>(acc, a, (uint32_t)v);
    if (kind == COZK_SCALAR_U64) co_mac<1>(acc, a, (uint32_t)(v >> 32));  // uniform per column
}
static __device__ __forceinline__ void co_add(uint32_t (&acc)[CO_LIMBS], const uint32_t (&o)[CO_LIMBS]) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < CO_LIMBS; k++) {
        const uint64_t t = (uint64_t)acc[k] + o[k] + carry;
        acc[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
static __device__ __forceinline__ fe co_reduce(const uint32_t (&s)[CO_LIMBS]) {
    fe t0, t1 = Fr::zero();
#pragma unroll
    for (int k = 0; k < 8; k++) t0.l[k] = s[k];
#pragma unroll
    for (int k = 8; k < CO_LIMBS; k++) t1.l[k - 8] = s[k];
    return Fr::add(Fr::to_mont(Fr::from_mont(t0)), Fr::to_mont(t1));
}

// partial[c * gridDim.x + blockIdx.x] = sum over this workgroup's stride of chi[i] * cols[c][i], for the CO_CB columns of row blockIdx.y
__global__ void __launch_bounds__(PT) k_compact_eval_chi(CompactCols cols, int k, size_t n, const fe* __restrict__ chi, fe* __restrict__ partial) {
    constexpr int CB = CO_CB;
    __shared__ uint32_t raw[PT / 64][CB][CO_LIMBS];
    const int c0 = blockIdx.y * CB;
    const int kb = k - c0 < CB ? k - c0 : CB;  // uniform over the workgroup
    uint32_t acc[CB][CO_LIMBS];
#pragma unroll
    for (int q = 0; q < CB; q++)
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) acc[q][l] = 0;
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < n; i += (size_t)gridDim.x * PT) {
        const fe c = fe_load(chi + i);
#pragma unroll
        for (int q = 0; q < CB; q++)
            if (q < kb) {
                const int kind = cols.kind[c0 + q];
                co_mac_entry(acc[q], c, small_load(SmallCol{cols.p[c0 + q], kind}, i), kind);
            }
    }
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the wave's raw sum of each column: 6 shuffle steps x 11 limbs = 66 shuffles and 6 carry chains of 11 additions per column, 528
    // shuffles per wave at 8 columns.  Paid once per workgroup, beside lanes of >= 16 terms x 8 columns x ~30 instructions; with the
    // grid's cap of 512 workgroups it is part of why the kernel stays far from its byte floor (DESIGN 4).  kb is uniform over the
    // workgroup, so every lane of a wave takes part in each shuffle.
#pragma unroll
    for (int q = 0; q < CB; q++)
        if (q < kb) {
            for (int off = 32; off > 0; off >>= 1) {
                uint32_t o[CO_LIMBS];
#pragma unroll
                for (int l = 0; l < CO_LIMBS; l++) o[l] = __shfl_down(acc[q][l], off);
                co_add(acc[q], o);
            }
            if (lane == 0) {
#pragma unroll
                for (int l = 0; l < CO_LIMBS; l++) raw[wave][q][l] = acc[q][l];
            }
        }
    __syncthreads();
    if ((int)threadIdx.x < kb) {
        uint32_t s[CO_LIMBS], o[CO_LIMBS];
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) s[l] = raw[0][threadIdx.x][l];
#pragma unroll
        for (int w = 1; w < PT / 64; w++) {
#pragma unroll
            for (int l = 0; l < CO_LIMBS; l++) o[l] = raw[w][threadIdx.x][l];
            co_add(s, o);
        }
        fe_store(partial + (size_t)(c0 + threadIdx.x) * gridDim.x + blockIdx.x, co_reduce(s));
    }
}

// out[i] = sum_c cf[c] * cols[c][i]: the coefficients travel in the kernel arguments, one accumulator and one reduction per entry
__global__ void __launch_bounds__(PT) k_compact_lincomb(CompactLin a, int k, size_t n, fe* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    uint32_t acc[CO_LIMBS];
#pragma unroll
    for (int l = 0; l < CO_LIMBS; l++) acc[l] = 0;
    for (int c = 0; c < k; c++) {
        const int kind = a.cols.kind[c];
        co_mac_entry(acc, a.cf[c], small_load(SmallCol{a.cols.p[c], kind}, i), kind);
    }
    fe_store(out + i, co_reduce(acc));
}

// the checks both calls share; the columns' one length comes back in n
static void compact_cols(const char* what, const cozk_vec* const* cols, size_t k, CompactCols& h, size_t& n) {
    const std::string w(what);
    COZK_REQUIRE(k >= 1 && k <= (size_t)CO_MAX_COLS, w + ": 1 <= k <= 24 columns");
    for (size_t c = 0; c < k; c++) {
        const cozk_vec* v = cols[c];
        COZK_REQUIRE(v && (v->kind == COZK_SCALAR_U8 || v->kind == COZK_SCALAR_U16 || v->kind == COZK_SCALAR_U32 || v->kind == COZK_SCALAR_U64),
                     w + ": the columns are U8 / U16 / U32 / U64 vectors");
        COZK_REQUIRE(v->n == cols[0]->n, w + ": every column has one length");
        h.p[c] = v->d;
        h.kind[c] = (uint8_t)v->kind;
    }
    n = cols[0]->n;
    COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), w + ": 1 <= n < 2^32");
}

extern "C" {

int cozk_compact_batch_evaluate_at_chi(cozk_ctx* ctx, const cozk_vec* const* cols, size_t k, const cozk_vec* chi, uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && cols && chi && out, "compact_batch_evaluate: bad argument");
        CompactCols h{};
        size_t n = 0;
        compact_cols("compact_batch_evaluate", cols, k, h, n);
        COZK_REQUIRE(chi->kind == COZK_SCALAR_FR, "compact_batch_evaluate: chi is an FR vector");
        COZK_REQUIRE(n <= chi->n, "compact_batch_evaluate: chi shorter than the columns");
        const unsigned gx = grid_capped((n + CO_LANE_TERMS - 1) / CO_LANE_TERMS, CO_EVAL_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, (unsigned)k, gx, k);
        k_compact_eval_chi<<<dim3(gx, (unsigned)((k + CO_CB - 1) / CO_CB)), PT, 0, ctx->stream>>>(h, (int)k, n, (const fe*)chi->d, sl.partial);
        HIP_TRY(hipGetLastError());
        std::vector<fe> r(k);
        finish_sums(ctx, sl, (unsigned)k, gx, Fr::one(), 0, r.data());
        for (size_t c = 0; c < k; c++) fe_to_u64x4(r[c], out + 4 * c);
    });
}

int cozk_compact_linear_combination(cozk_ctx* ctx, const cozk_vec* const* cols, const uint64_t* coeffs, size_t k, cozk_vec** out_vec) {
    if (out_vec) *out_vec = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && cols && coeffs && out_vec, "compact_linear_combination: bad argument");
        CompactLin h{};
        size_t n = 0;
        compact_cols("compact_linear_combination", cols, k, h.cols, n);
        for (size_t c = 0; c < k; c++) h.cf[c] = fe_from_u64x4(coeffs + 4 * c);
        fe* d = dev_alloc_fe(n);
        k_compact_lincomb<<<grid_for(n), PT, 0, ctx->stream>>>(h, (int)k, n, d);
        if (hipGetLastError() != hipSuccess) {
            ctx_dev_free(ctx, d);
            throw CozkError(COZK_ERR_HIP, "compact_linear_combination: launch failed");
        }
        *out_vec = new cozk_vec{ctx, n, COZK_SCALAR_FR, d, n * sizeof(fe), true};
    });
}

}  // extern "C"
