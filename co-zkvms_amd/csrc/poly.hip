// Polynomial seam: device-resident multilinear polynomials over shares.
//
//   cozk_poly     <-> Rep3DensePolynomial (co-jolt/src/poly/dense_mlpoly.rs:23-32) / plain DensePolynomial
//   cozk_layer    <-> Rep3DenseInterleavedPolynomial (co-jolt/src/poly/dense_interleaved_poly.rs:35-48)
//   cozk_spliteq  <-> SplitEqPolynomial (jolt-core; used dense_interleaved_poly.rs:218-303)
//
// All kernels are streaming kernels on 32-byte Montgomery elements (16-byte vector loads per lane);
// round results (3-4 field elements) are reduced in-kernel (wave shuffle tree + LDS), finished by a
// one-block kernel, and returned through pinned host memory.
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <string.h>
#include "poly.hip.hpp"
#include "prf.hip.hpp"
#include "fr9.hip.hpp"
#include "shamir_deal.hip.hpp"
#include "host/layer_tail.hpp"

static constexpr int PT = 256;      // threads per block
static constexpr int MAXBLK = 2048; // grid cap for reducing kernels (>= 8 blocks per CU)
static constexpr unsigned ROUND_GRID_MAX = 1024;       // workgroups of a round-sum launch that is not sized by resident_grid
static constexpr unsigned BATCH_GRID_MAX = 512;        // ... of the batched reductions (dot product, opening, product and Spartan rounds)
static constexpr unsigned EVAL_GRID_MAX = 192;         // ... of the evaluate / batched dot-product kernels (few, long lanes)
static constexpr size_t LAYER_F9_MIN_CHUNKS = 1024;    // layers of this many 4-element chunks are throughput-bound: the 9 x 29 kernels
static constexpr size_t LAYER_GROUPED_MIN_E1H = 512;   // E1_len / 2 from which the split-eq inner sums (NESTED = 2) pay

struct cozk_poly {
    cozk_ctx* ctx;
    int mode;            // 1 plain, 2 rep3
    fe* a0; fe* b0;      // unbound coefficients (`coeffs`, immutable; possibly a borrowed chunk view)
    bool own0;
    fe* buf[2][2];       // ping-pong bound buffers [which][component]
    size_t cap[2];
    int cur;             // -1: unbound, else index of the live bound buffer
    size_t len;
    size_t orig_len;
};

struct cozk_layer {
    cozk_ctx* ctx;
    int mode;
    fe* buf[2][2];       // ping-pong [which][component]; component 1 of a PLAIN layer is null (the launch sites pass it as it is)
    size_t cap[2];
    int cur;
    size_t len;
};

struct cozk_spliteq {
    cozk_ctx* ctx;
    fe* E1[2]; fe* E2[2];   // ping-pong
    int c1, c2;
    size_t E1_len, E2_len, E1_cap, E2_cap;
    int num_vars;
};

static inline unsigned grid_for(size_t n) { return (unsigned)((n + PT - 1) / PT); }
static inline unsigned grid_capped(size_t n, unsigned cap = MAXBLK) {
    size_t g = (n + PT - 1) / PT;
    return (unsigned)(g > cap ? cap : (g ? g : 1));
}
// COZK_SUM_GRID_MAX=n (n > 0): at most n workgroups for the grid-stride round-sum launches (layer cubic sums, fused bind + sums,
// toggle and outer rounds), so that each lane adds thousands of terms -- what the lazy 9 x 29 sums are tested at.  Read on every
// call: a test may set it for one proof.  Unset or 0: the grids are unchanged.
static inline unsigned sum_grid(unsigned gx) {
    const char* e = getenv("COZK_SUM_GRID_MAX");
    const long n = e ? atol(e) : 0;
    return n > 0 && (unsigned long)n < gx ? (unsigned)n : gx;
}

// Few, long lanes for the evaluate kernel: a lane ends with one wide reduction per accumulator (8 products) + the block sums, which
// would outweigh its multiply-add chains if it only had a handful of elements.  COZK_EVAL_GX=n: another cap, for A/B runs.
static unsigned eval_grid_max() {
    static const unsigned cap = getenv("COZK_EVAL_GX") ? (unsigned)atoi(getenv("COZK_EVAL_GX")) : EVAL_GRID_MAX;
    return cap;
}

// Grid of a grid-stride kernel whose waves are long (thousands of instructions per element): exactly the workgroups the chip
// holds at once (occupancy query x CUs), so that every wave is resident from the start and the last residency round is not a
// partial one.  Measured on the 2^24-element probe with the LDS-staged 9 x 29 kernels (compute-bound): 0.311 vs 0.334 ms plain,
// 0.486 vs 0.505 ms Rep3 against the former fixed cap of 1024 workgroups (COZK_RESIDENT_GRID=0 restores it for A/B runs).
static unsigned resident_grid(const void* kernel, size_t nblocks_needed, int device) {
    static const int legacy = getenv("COZK_RESIDENT_GRID") && atoi(getenv("COZK_RESIDENT_GRID")) == 0;  // A/B switch: the old cap
    if (legacy) return (unsigned)(nblocks_needed < 1024 ? (nblocks_needed ? nblocks_needed : 1) : 1024);
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, unsigned> cache;
    unsigned cap;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find({kernel, device});
        if (it == cache.end()) {
            int per_cu = 0, cus = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PT, 0));
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
            unsigned v = (unsigned)(per_cu > 0 ? per_cu : 1) * (unsigned)(cus > 0 ? cus : 1);
            if (v > MAXBLK) v = MAXBLK;
            it = cache.emplace(std::make_pair(kernel, device), v).first;
        }
        cap = it->second;
    }
    return (unsigned)(nblocks_needed < cap ? (nblocks_needed ? nblocks_needed : 1) : cap);
}

static const fe* poly_a(const cozk_poly* p) { return p->cur < 0 ? p->a0 : p->buf[p->cur][0]; }
static const fe* poly_b(const cozk_poly* p) { return p->cur < 0 ? p->b0 : p->buf[p->cur][1]; }

// ------------------------------------------------------------------ kernels: dense polynomial
// bind: out[i] = lo + r (hi - lo); LowToHigh pairs (2i, 2i+1), HighToLow pairs (i, i + n)
// (dense_mlpoly.rs:310-378).  Algorithmic traffic: read n shares, write n/2 = 96 n bytes (REP3).
template <int NC, int ORDER>
__global__ void __launch_bounds__(PT) k_poly_bind(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* oa, fe* ob,
                                               size_t n_out, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    size_t lo_i = ORDER == COZK_LOW_TO_HIGH ? 2 * i : i;
    size_t hi_i = ORDER == COZK_LOW_TO_HIGH ? 2 * i + 1 : i + n_out;
    Sh<NC> lo = sh_load<NC>(ia, ib, lo_i), hi = sh_load<NC>(ia, ib, hi_i);
    sh_store<NC>(oa, ob, i, sh_lerp<NC>(lo, hi, r));
}

// partial[blockIdx.y * gridDim.x + blockIdx.x] = sum over this block's stride of (a+b) * chi
// (evaluate_at_chi, dense_mlpoly.rs:160-181; TWO_INV folded in by the finishing kernel)
template <int NC>
__global__ void __launch_bounds__(PT) k_poly_eval_chi(const fe* const* __restrict__ pa, const fe* const* __restrict__ pb,
                                                   const size_t* __restrict__ lens, const fe* __restrict__ chi, int k,
                                                   fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    // a workgroup row serves TWO polynomials, so chi[i] is fetched once per pair (chi is 32 MiB at 2^20: it does not stay in
    // L2 between the polynomials' passes); each product goes into its polynomial's wide accumulator (poly.hip.hpp: lazy dot
    // products, one reduction per lane at the end)
    const int p0 = 2 * blockIdx.y, p1 = p0 + 1;
    const bool two = p1 < k;
    const fe* a0 = pa[p0];
    const fe* b0 = NC == 2 ? pb[p0] : nullptr;
    const fe* a1 = two ? pa[p1] : nullptr;
    const fe* b1 = (two && NC == 2) ? pb[p1] : nullptr;
    const size_t n0 = lens[p0], n1 = two ? lens[p1] : 0;
    const size_t n = n0 > n1 ? n0 : n1;
    FrWide w0, w1;
    fr_wide_zero(w0);
    fr_wide_zero(w1);
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < n; i += (size_t)gridDim.x * PT) {
        fe c = fe_load(chi + i);
        if (i < n0) fr_wide_mac(w0, sh_ab_sum<NC>(sh_load<NC>(a0, b0, i)), c);
        if (i < n1) fr_wide_mac(w1, sh_ab_sum<NC>(sh_load<NC>(a1, b1, i)), c);
    }
    fe acc = fr_block_sum(fr_wide_reduce(w0), sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)p0 * gridDim.x + blockIdx.x, acc);
    if (two) {  // uniform per workgroup
        acc = fr_block_sum(fr_wide_reduce(w1), sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)p1 * gridDim.x + blockIdx.x, acc);
    }
}

// out[y] = scale * sum_x partial[y * nper + x]
// ... and, when `pub` is armed, the LAST of its (few) workgroups publishes the round's sequence number into the pinned word the host
// spins on: no stream memory write behind the kernel (~560 per chained proof, 3.5 us of GPU time + a launch gap each).
struct RoundPublish {
    unsigned* ticket;  // device counter, zero between launches; nullptr: nothing to publish
    uint32_t* flag;    // pinned word
    uint32_t seq;
};
__global__ void __launch_bounds__(PT) k_finish_sums(const fe* __restrict__ partial, unsigned nper, fe scale, int apply_scale,
                                                 fe* __restrict__ out, RoundPublish pub) {
    __shared__ fe sh4[4];
    fe acc = Fr::zero();
    for (unsigned x = threadIdx.x; x < nper; x += PT) acc = Fr::add(acc, fe_load(partial + (size_t)blockIdx.x * nper + x));
    acc = fr_block_sum(acc, sh4);
    if (threadIdx.x == 0) {
        fe_store(out + blockIdx.x, apply_scale ? Fr::mul(acc, scale) : acc);
        if (pub.ticket) {
            __threadfence_system();  // this workgroup's result is in host memory before its ticket
            if (atomicAdd(pub.ticket, 1u) == gridDim.x - 1) {
                *pub.ticket = 0;
                __threadfence_system();
                __hip_atomic_store(pub.flag, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// per-component dot product with a public vector (dot_product_with_public, dense_mlpoly.rs:228-234)
template <int NC>
__global__ void __launch_bounds__(PT) k_poly_dot_public(const fe* __restrict__ a, const fe* __restrict__ b,
                                                     const fe* __restrict__ pub, size_t n, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    FrWide w[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) fr_wide_zero(w[k]);
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < n; i += (size_t)gridDim.x * PT) {
        Sh<NC> s = sh_load<NC>(a, b, i);
        fe p = fe_load(pub + i);
#pragma unroll
        for (int k = 0; k < NC; k++) fr_wide_mac(w[k], s.c[k], p);
    }
#pragma unroll
    for (int k = 0; k < NC; k++) {
        fe v = fr_block_sum(fr_wide_reduce(w[k]), sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)k * gridDim.x + blockIdx.x, v);
    }
}

// out[i] = sum_k coeff[k] * poly_k[i] (i < len_k)   (linear_combination, dense_mlpoly.rs:195-226;
// public polynomials enter through their trivial share, multilinear_polynomial.rs:196-296)
template <int NC>
__global__ void __launch_bounds__(PT) k_poly_lincomb(const fe* const* __restrict__ pa, const fe* const* __restrict__ pb,
                                                  const size_t* __restrict__ lens, const fe* __restrict__ coeffs, int k,
                                                  fe* oa, fe* ob, size_t n) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    Sh<NC> acc;
    if (k >= 8) {
        // long combinations (the rho-RLC of all committed polynomials): one reduction per output element instead of k
        FrWide w[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) fr_wide_zero(w[c]);
        for (int j = 0; j < k; j++) {
            if (i < lens[j]) {
                fe cf = fe_load(coeffs + j);
                if (pa[j]) fr_wide_mac(w[0], fe_load(pa[j] + i), cf);
                if (NC == 2 && pb[j]) fr_wide_mac(w[NC - 1], fe_load(pb[j] + i), cf);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) acc.c[c] = fr_wide_reduce(w[c]);
        sh_store<NC>(oa, ob, i, acc);
        return;
    }
    for (int c = 0; c < NC; c++) acc.c[c] = Fr::zero();
    for (int j = 0; j < k; j++) {
        if (i < lens[j]) {
            fe cf = fe_load(coeffs + j);
            if (pa[j]) acc.c[0] = Fr::add(acc.c[0], Fr::mul(fe_load(pa[j] + i), cf));
            if (NC == 2 && pb[j]) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], Fr::mul(fe_load(pb[j] + i), cf));
        }
    }
    sh_store<NC>(oa, ob, i, acc);
}

// the same with the (<= 16) operand pointers passed by value in the kernel arguments: the opening-reduction
// sumcheck calls this once per round, and four metadata uploads + a drain per round cost more than the kernel
struct OpenQuadArgs {
    const fe* a[16];
    const fe* b[16];
    const fe* eq[16];
    size_t half[16];
};
template <int NC>
__global__ void __launch_bounds__(PT) k_open_quadratic_args(OpenQuadArgs args, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const fe* a = args.a[blockIdx.y];
    const fe* b = NC == 2 ? args.b[blockIdx.y] : nullptr;
    const fe* eq = args.eq[blockIdx.y];
    size_t h = args.half[blockIdx.y];
    fe e0 = Fr::zero(), e2 = Fr::zero();
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < h; i += (size_t)gridDim.x * PT) {
        fe q0 = fe_load(eq + i), q1 = fe_load(eq + i + h);
        fe p0 = sh_ab_sum<NC>(sh_load<NC>(a, b, i)), p1 = sh_ab_sum<NC>(sh_load<NC>(a, b, i + h));
        e0 = Fr::add(e0, Fr::mul(p0, q0));
        fe pb2 = Fr::sub(Fr::dbl(p1), p0), qb2 = Fr::sub(Fr::dbl(q1), q0);
        e2 = Fr::add(e2, Fr::mul(pb2, qb2));
    }
    e0 = fr_block_sum(e0, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)(2 * blockIdx.y) * gridDim.x + blockIdx.x, e0);
    e2 = fr_block_sum(e2, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)(2 * blockIdx.y + 1) * gridDim.x + blockIdx.x, e2);
}

// K11 leaf fingerprints (compute_leaves of the three memory-checking instances, e.g.
// co-jolt/src/jolt/vm/bytecode/worker.rs:57-100, read_write_memory/worker.rs:207-260):
//   leaf[i] = sum_k c_k * col_k[i]  (compact public columns, CompactPolynomial::field_mul)
//           + sum_j d_j * poly_j[i]  (shared or plain Fr polynomials, mul_public)
//           + constant               (e.g. -tau, or gamma^7 - tau for the write leaves)
// The public part enters a Rep3 leaf through add_public: party 0's a, party 1's b.  `cs` holds c_k * R (the
// Montgomery form of the Montgomery form), so that one product with the plain small integer gives c_k * v in
// Montgomery form.
struct SmallCol {
    const void* p;
    int kind;
};
static __device__ __forceinline__ uint64_t small_load(const SmallCol& c, size_t i) {
    switch (c.kind) {
        case COZK_SCALAR_U8: return reinterpret_cast<const uint8_t*>(c.p)[i];
        case COZK_SCALAR_U16: return reinterpret_cast<const uint16_t*>(c.p)[i];
        case COZK_SCALAR_U32: return reinterpret_cast<const uint32_t*>(c.p)[i];
        default: return reinterpret_cast<const uint64_t*>(c.p)[i];
    }
}
template <int NC>
__global__ void __launch_bounds__(PT) k_fingerprint_leaves(const SmallCol* __restrict__ cols, const fe* __restrict__ cs, int ks,
                                                        const fe* const* __restrict__ pa, const fe* const* __restrict__ pb,
                                                        const fe* __restrict__ ds, int kp, fe constant, int pub_a, int pub_b, fe* oa, fe* ob,
                                                        size_t n) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe pub = constant;
    for (int k = 0; k < ks; k++) {
        uint64_t v = small_load(cols[k], i);
        fe x = Fr::zero();
        x.l[0] = (uint32_t)v;
        x.l[1] = (uint32_t)(v >> 32);
        pub = Fr::add(pub, Fr::mul(fe_load(cs + k), x));
    }
    Sh<NC> acc;
    for (int c = 0; c < NC; c++) acc.c[c] = Fr::zero();
    for (int j = 0; j < kp; j++) {
        fe d = fe_load(ds + j);
        if (pa[j]) acc.c[0] = Fr::add(acc.c[0], Fr::mul(fe_load(pa[j] + i), d));
        if (NC == 2 && pb[j]) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], Fr::mul(fe_load(pb[j] + i), d));
    }
    if (pub_a) acc.c[0] = Fr::add(acc.c[0], pub);
    if (NC == 2 && pub_b) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], pub);
    sh_store<NC>(oa, ob, i, acc);
}

// the usual shapes (<= 16 columns, <= 8 polynomials) travel by value in the kernel arguments: no staging, no drain
struct FingerprintArgs {
    SmallCol cols[16];
    fe cs[16];
    const fe* pa[8];
    const fe* pb[8];
    fe ds[8];
};
template <int NC>
__global__ void __launch_bounds__(PT) k_fingerprint_leaves_args(FingerprintArgs a, int ks, int kp, fe constant, int pub_a, int pub_b, fe* oa, fe* ob,
                                                             size_t n) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe pub = constant;
    for (int k = 0; k < ks; k++) {
        uint64_t v = small_load(a.cols[k], i);
        fe x = Fr::zero();
        x.l[0] = (uint32_t)v;
        x.l[1] = (uint32_t)(v >> 32);
        pub = Fr::add(pub, Fr::mul(a.cs[k], x));
    }
    Sh<NC> acc;
    for (int c = 0; c < NC; c++) acc.c[c] = Fr::zero();
    for (int j = 0; j < kp; j++) {
        if (a.pa[j]) acc.c[0] = Fr::add(acc.c[0], Fr::mul(fe_load(a.pa[j] + i), a.ds[j]));
        if (NC == 2 && a.pb[j]) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], Fr::mul(fe_load(a.pb[j] + i), a.ds[j]));
    }
    if (pub_a) acc.c[0] = Fr::add(acc.c[0], pub);
    if (NC == 2 && pub_b) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], pub);
    sh_store<NC>(oa, ob, i, acc);
}

// quadratic opening-reduction round (compute_quadratic, opening_proof.rs:374-414): per opening
// eval_0 = sum_i poly[i]*eq[i], eval_2 = sum_i (2 poly[i+h] - poly[i]) * (2 eq[i+h] - eq[i]);
// partial[(2*y + e) * gridDim.x + x]; the (a+b)*TWO_INV conversion is folded into the finisher.
template <int NC>
__global__ void __launch_bounds__(PT) k_open_quadratic(const fe* const* __restrict__ pa, const fe* const* __restrict__ pb,
                                                    const fe* const* __restrict__ peq, const size_t* __restrict__ halves,
                                                    fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const fe* a = pa[blockIdx.y];
    const fe* b = NC == 2 ? pb[blockIdx.y] : nullptr;
    const fe* eq = peq[blockIdx.y];
    size_t h = halves[blockIdx.y];
    fe e0 = Fr::zero(), e2 = Fr::zero();
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < h; i += (size_t)gridDim.x * PT) {
        fe q0 = fe_load(eq + i), q1 = fe_load(eq + i + h);
        fe p0 = sh_ab_sum<NC>(sh_load<NC>(a, b, i)), p1 = sh_ab_sum<NC>(sh_load<NC>(a, b, i + h));
        e0 = Fr::add(e0, Fr::mul(p0, q0));
        fe pb2 = Fr::sub(Fr::dbl(p1), p0), qb2 = Fr::sub(Fr::dbl(q1), q0);
        e2 = Fr::add(e2, Fr::mul(pb2, qb2));
    }
    e0 = fr_block_sum(e0, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)(2 * blockIdx.y) * gridDim.x + blockIdx.x, e0);
    e2 = fr_block_sum(e2, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)(2 * blockIdx.y + 1) * gridDim.x + blockIdx.x, e2);
}

// PST13 `open` fold (pst13.rs:445-459): q[b] = r[2b+1] - r[2b]; r'[b] = r[2b](1-p) + r[2b+1] p
__global__ void __launch_bounds__(PT) k_pst_fold(const fe* __restrict__ r, fe* __restrict__ q, fe* __restrict__ rn, size_t half, fe p) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= half) return;
    fe lo = fe_load(r + 2 * i), hi = fe_load(r + 2 * i + 1);
    fe d = Fr::sub(hi, lo);
    fe_store(q + i, d);
    fe_store(rn + i, Fr::add(lo, Fr::mul(d, p)));
}

// ------------------------------------------------------------------ kernels: interleaved GKR layer
// The steps every Fr layer kernel below is made of (the 9 x 29 kernels have their own: layer9_terms .. layer9_finish): those that
// the host tail shares are in host/layer_tail.hpp (layer_bind_chunk, eq3, layer_chunk_count, split_eq_at, layer_eq_at, layer_terms,
// fold_pair), the reductions of a workgroup are here.
// items a round over split-eq tables sums: zip() stops at the shorter side of the layer and the eq table
template <int NESTED>
static __device__ __forceinline__ size_t split_eq_limit(size_t E2_len, int log_E1_half) {
    return NESTED ? ((size_t)E2_len << log_E1_half) : E2_len / 2;
}
// the workgroup's sum of v through `sh` (fr_block_sum) to row `row` of the partial sums, gridDim.x entries per row
static __device__ __forceinline__ void partial_row_sum(fe v, fe* sh, fe* __restrict__ partial, size_t row) {
    v = fr_block_sum(v, sh);
    if (threadIdx.x == 0) fe_store(partial + row * gridDim.x + blockIdx.x, v);
}

// the workgroup's three sums, one after the other through `sh` (fr_block_sum); sum k = 0, 1, 2 goes to out(k), which is evaluated
// behind the sum's barriers, where the kernels had their address arithmetic
template <class Out>
static __device__ __forceinline__ void layer_finish(fe s0, fe s2, fe s3, fe* sh, Out out) {
    s0 = fr_block_sum(s0, sh);
    if (threadIdx.x == 0) fe_store(out(0), s0);
    s2 = fr_block_sum(s2, sh);
    if (threadIdx.x == 0) fe_store(out(1), s2);
    s3 = fr_block_sum(s3, sh);
    if (threadIdx.x == 0) fe_store(out(2), s3);
}

template <int NC>
__global__ void __launch_bounds__(PT) k_layer_bind(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* oa, fe* ob,
                                                size_t len, fe r) {
    size_t c = (size_t)blockIdx.x * PT + threadIdx.x;
    size_t nch = (len + 3) / 4;
    if (c >= nch) return;
    Sh<NC> lo, hi;
    layer_bind_chunk<NC>(ia, ib, len, c, r, oa, ob, lo, hi);
}

// cubic round evaluations g(0), g(2), g(3) of sum eq * L * R  (compute_cubic,
// dense_interleaved_poly.rs:210-356).  NESTED: which form of the eq pair (layer_eq_at).
template <int NC, int NESTED>
__global__ void __launch_bounds__(PT) k_layer_cubic(const fe* __restrict__ a, const fe* __restrict__ b, size_t len,
                                                 const fe* __restrict__ E1, size_t E1_half, const fe* __restrict__ E2,
                                                 size_t E2_len, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const size_t nch = layer_chunk_count(len, NESTED, E1_half, E2_len);
    fe s0 = Fr::zero(), s2 = Fr::zero(), s3 = Fr::zero();
    for (size_t c = (size_t)blockIdx.x * PT + threadIdx.x; c < nch; c += (size_t)gridDim.x * PT) {
        fe e[3];
        fe scale;
        layer_eq_at(NESTED, E1, E1_half, E2, c, e, scale);
        Sh<NC> l0 = sh_load_or_zero<NC>(a, b, 4 * c, len), r0 = sh_load_or_zero<NC>(a, b, 4 * c + 1, len);
        Sh<NC> l1 = sh_load_or_zero<NC>(a, b, 4 * c + 2, len), r1 = sh_load_or_zero<NC>(a, b, 4 * c + 3, len);
        fe t0, t2, t3;
        layer_terms<NC>(l0, r0, l1, r1, e, NESTED, scale, t0, t2, t3);
        s0 = Fr::add(s0, t0);
        s2 = Fr::add(s2, t2);
        s3 = Fr::add(s3, t3);
    }
    layer_finish(s0, s2, s3, sh4, [&](unsigned k) { return partial + k * gridDim.x + blockIdx.x; });
}

// bind + the next round's cubic sums in ONE pass over a large layer: a lane reads 8 unbound elements, writes the 4
// bound ones and adds their chunk's three terms (eq tables already folded by the caller).  The separate kernels
// read the layer twice and write it once per round (80 B per element, plain); this reads once and writes once (48).
template <int NC, int NESTED>
__global__ void __launch_bounds__(PT) k_layer_bind_cubic(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* oa, fe* ob, size_t len_in, fe r,
                                                      const fe* __restrict__ E1, size_t E1_half, const fe* __restrict__ E2, size_t E2_len,
                                                      fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const size_t nch_in = (len_in + 3) / 4;      // input chunks of 4 -> 2 bound elements each
    const size_t len_out = 2 * nch_in;
    const size_t nch_out = (len_out + 3) / 4;    // output chunks of 4 bound elements = 2 input chunks
    const size_t nsum = layer_chunk_count(len_out, NESTED, E1_half, E2_len);
    fe s0 = Fr::zero(), s2 = Fr::zero(), s3 = Fr::zero();
    for (size_t c = (size_t)blockIdx.x * PT + threadIdx.x; c < nch_out; c += (size_t)gridDim.x * PT) {
        Sh<NC> v[4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            size_t ci = 2 * c + h;
            if (ci < nch_in) {
                layer_bind_chunk<NC>(ia, ib, len_in, ci, r, oa, ob, v[2 * h], v[2 * h + 1]);
            } else {
                for (int k = 0; k < NC; k++) v[2 * h].c[k] = v[2 * h + 1].c[k] = Fr::zero();
            }
        }
        if (c < nsum) {  // every output chunk is bound and stored; only those on the shorter side are summed
            fe e[3];
            fe scale;
            layer_eq_at(NESTED, E1, E1_half, E2, c, e, scale);
            fe t0, t2, t3;
            layer_terms<NC>(v[0], v[1], v[2], v[3], e, NESTED, scale, t0, t2, t3);
            s0 = Fr::add(s0, t0);
            s2 = Fr::add(s2, t2);
            s3 = Fr::add(s3, t3);
        }
    }
    layer_finish(s0, s2, s3, sh4, [&](unsigned k) { return partial + k * gridDim.x + blockIdx.x; });
}

// ---- the layer kernels on the 9 x 29 multiplier (round 3, fr9.hip.hpp): same thread mapping and tails as k_layer_cubic /
// k_layer_bind_cubic, every product on the fused 29-bit chains, additions lazy, one lambda-removing product per lane at the end.
// terms of one output chunk: s_k += (l_k x r_k) e_k at X = 0, 2, 3.  NESTED = 1: the E2 factor is folded into the eq pair first (two
// products per chunk).  NESTED = 2 (E1 tables of >= 512 pairs; the launcher walks the chunks block-contiguously): the inner sums of
// the split-eq form -- the terms of the chunks that share one E2 entry are summed with the raw E1 pair (lambda^2) in `grp` and
// multiplied by E2[x2] once per group (three products per E1_half / 256 chunks instead of two per chunk), as the reference's
// nested loops do (dense_interleaved_poly.rs:230-300).
struct Layer9Group {
    f9 g0, g2, g3;
    size_t x2;
};
static __device__ __forceinline__ void layer9_group_flush(Layer9Group& grp, const fe* __restrict__ E2, f9& s0, f9& s2, f9& s3) {
    if (grp.x2 == (size_t)-1) return;
    const f9 sc = f9_from_fe(fe_load(E2 + grp.x2));
    s0 = f9_norm(fr9_add(s0, fr9_mul(grp.g0, sc)));
    s2 = f9_norm(fr9_add(s2, fr9_mul(grp.g2, sc)));
    s3 = f9_norm(fr9_add(s3, fr9_mul(grp.g3, sc)));
}
// the periodic fold of the lazy sums (fr9.hip.hpp): once per FR9_FOLD_PERIOD iterations of the wave-uniform chunk walk, each of
// which adds at most one term to every sum (NESTED = 2: one to each group sum, at most one flush to each s)
template <int NESTED>
static __device__ __forceinline__ void layer9_fold(size_t it, f9& s0, f9& s2, f9& s3, Layer9Group& grp) {
    if (it == 0 || (it & (FR9_FOLD_PERIOD - 1)) != 0) return;
    fr9_fold(s0);
    fr9_fold(s2);
    fr9_fold(s3);
    if (NESTED == 2) {
        fr9_fold(grp.g0);
        fr9_fold(grp.g2);
        fr9_fold(grp.g3);
    }
}
template <int NC, int NESTED>
static __device__ __forceinline__ void layer9_terms(const Sh9<NC>& l0, const Sh9<NC>& r0, const Sh9<NC>& l1, const Sh9<NC>& r1, const fe* __restrict__ E1,
                                                    size_t E1_half, int e1_shift, const fe* __restrict__ E2, size_t c, f9& s0, f9& s2, f9& s3,
                                                    Layer9Group& grp) {
    f9 e0, e1;
    if (NESTED == 2) {
        const size_t x2 = c >> e1_shift, x1 = c & (E1_half - 1);
        if (x2 != grp.x2) {
            layer9_group_flush(grp, E2, s0, s2, s3);
            grp.g0 = grp.g2 = grp.g3 = fr9_zero();
            grp.x2 = x2;
        }
        e0 = f9_from_fe(fe_load(E1 + 2 * x1));
        e1 = f9_from_fe(fe_load(E1 + 2 * x1 + 1));
    } else if (NESTED) {
        const size_t x2 = c >> e1_shift, x1 = c & (E1_half - 1);
        const f9 sc = f9_from_fe(fe_load(E2 + x2));
        e0 = fr9_mul(f9_from_fe(fe_load(E1 + 2 * x1)), sc);
        e1 = fr9_mul(f9_from_fe(fe_load(E1 + 2 * x1 + 1)), sc);
    } else {
        e0 = f9_from_fe(fe_load(E2 + 2 * c));
        e1 = f9_from_fe(fe_load(E2 + 2 * c + 1));
    }
    const f9 me = f9_norm(f9_sub(e1, FR9_C2, e0));  // e0, e1 < 1.01 r normalised: me < 3.01 r
    const f9 e2 = fr9_add(e1, me), e3 = fr9_add(e2, me);  // limbs < 2^30, 1.5 * 2^30
    const Sh9<NC> ml = sh9_diff<NC>(l1, l0), mr = sh9_diff<NC>(r1, r0);
    const Sh9<NC> l2 = sh9_add_norm<NC>(l1, ml), r2 = sh9_add_norm<NC>(r1, mr);
    const Sh9<NC> l3 = sh9_add_norm<NC>(l2, ml), r3 = sh9_add_norm<NC>(r2, mr);
    f9& a0 = NESTED == 2 ? grp.g0 : s0;
    f9& a2 = NESTED == 2 ? grp.g2 : s2;
    f9& a3 = NESTED == 2 ? grp.g3 : s3;
    a0 = f9_norm(fr9_add(a0, fr9_mul(e0, sh9_local_mul<NC>(l0, r0))));
    a2 = f9_norm(fr9_add(a2, fr9_mul(e2, sh9_local_mul<NC>(l2, r2))));
    a3 = f9_norm(fr9_add(a3, fr9_mul(e3, sh9_local_mul<NC>(l3, r3))));
}
// the chunk walk of a workgroup: grid-stride, or (NESTED = 2) one contiguous range per workgroup so that a lane stays inside an E2
// group for E1_half / 256 iterations; `first` is the wave's first chunk of the first iteration
static __device__ __forceinline__ void layer9_walk(int nested, size_t nch, size_t& first, size_t& end, size_t& step) {
    if (nested == 2) {
        const size_t per = ((nch + gridDim.x - 1) / gridDim.x + PT - 1) / PT * PT;
        first = (size_t)blockIdx.x * per + (threadIdx.x & ~63u);
        end = (size_t)(blockIdx.x + 1) * per < nch ? (size_t)(blockIdx.x + 1) * per : nch;
        step = PT;
    } else {
        first = (size_t)blockIdx.x * PT + (threadIdx.x & ~63u);
        end = nch;
        step = (size_t)gridDim.x * PT;
    }
}
// lane sums -> canonical R-form block sums in partial[k * gridDim.x + blockIdx.x]
template <int NESTED>
static __device__ __forceinline__ void layer9_finish(const f9& s0, const f9& s2, const f9& s3, fe* __restrict__ partial, fe* sh4) {
    const f9 K = f9_const(NESTED ? FR9_K3 : FR9_K2);
    fe v = fr_block_sum(fr9_to_canonical(fr9_mul(s0, K)), sh4);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, v);
    v = fr_block_sum(fr9_to_canonical(fr9_mul(s2, K)), sh4);
    if (threadIdx.x == 0) fe_store(partial + gridDim.x + blockIdx.x, v);
    v = fr_block_sum(fr9_to_canonical(fr9_mul(s3, K)), sh4);
    if (threadIdx.x == 0) fe_store(partial + 2 * gridDim.x + blockIdx.x, v);
}


// ---- wave-private LDS staging of layer data (round 3).  A lane owns 128 consecutive bytes (4 field elements) of a row; read or
// written straight from the lane, a wave's dwordx4 instruction touches 64 different 128-byte lines 16 bytes at a time and every line
// is re-referenced by eight instructions (nontemporal accesses, which forbid that re-use, slowed the unstaged round 1.5-2 x).  Staged,
// instruction k moves rows 8k .. 8k+7 as eight WHOLE lines (lane l: row 8k + l / 8, 16-byte piece l % 8) and the lanes trade pieces
// through a wave-private LDS window of 64 rows x 144 bytes (128 + 16: a b128 access of 16 lanes then covers 16 distinct bank quads).
// A wave's LDS instructions execute in order; the fences keep the compiler from reordering them across the exchange.
static constexpr int ST_ROW = 144;
static constexpr int ST_WAVE_BYTES = 64 * ST_ROW;
static __device__ __forceinline__ void stage_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// out[0..3] <- the 4 elements at g + lane * row_stride (bytes); the wave's 64 rows are all in range
static __device__ __forceinline__ void stage_in_rows(const char* __restrict__ g, size_t row_stride, char* st, fe out[4]) {
    const int lane = threadIdx.x & 63, piece = lane & 7, sub = lane >> 3;
    uint4 t[8];
#pragma unroll
    for (int k = 0; k < 8; k++) t[k] = *reinterpret_cast<const uint4*>(g + (size_t)(8 * k + sub) * row_stride + 16 * piece);
#pragma unroll
    for (int k = 0; k < 8; k++) *reinterpret_cast<uint4*>(st + (8 * k + sub) * ST_ROW + 16 * piece) = t[k];
    stage_fence();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 lo = *reinterpret_cast<const uint4*>(st + lane * ST_ROW + 32 * j);
        const uint4 hi = *reinterpret_cast<const uint4*>(st + lane * ST_ROW + 32 * j + 16);
        out[j].l[0] = lo.x; out[j].l[1] = lo.y; out[j].l[2] = lo.z; out[j].l[3] = lo.w;
        out[j].l[4] = hi.x; out[j].l[5] = hi.y; out[j].l[6] = hi.z; out[j].l[7] = hi.w;
    }
    stage_fence();  // the window is free again once every lane has its row
}
// the 4 elements of this lane -> g + lane * row_stride (bytes)
static __device__ __forceinline__ void stage_out_rows(char* __restrict__ g, char* st, const fe in[4], size_t row_stride = 128) {
    const int lane = threadIdx.x & 63, piece = lane & 7, sub = lane >> 3;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        *reinterpret_cast<uint4*>(st + lane * ST_ROW + 32 * j) = make_uint4(in[j].l[0], in[j].l[1], in[j].l[2], in[j].l[3]);
        *reinterpret_cast<uint4*>(st + lane * ST_ROW + 32 * j + 16) = make_uint4(in[j].l[4], in[j].l[5], in[j].l[6], in[j].l[7]);
    }
    stage_fence();
#pragma unroll
    for (int k = 0; k < 8; k++)
        *reinterpret_cast<uint4*>(g + (size_t)(8 * k + sub) * row_stride + 16 * piece) = *reinterpret_cast<const uint4*>(st + (8 * k + sub) * ST_ROW + 16 * piece);
    stage_fence();
}

template <int NC, int NESTED>
__global__ void __launch_bounds__(PT) k_layer_cubic9(const fe* __restrict__ a, const fe* __restrict__ b, size_t len, const fe* __restrict__ E1, size_t E1_half,
                                                  const fe* __restrict__ E2, size_t E2_len, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ __attribute__((aligned(16))) char stage[PT / 64][ST_WAVE_BYTES];
    char* st = stage[threadIdx.x >> 6];
    size_t nch = (len + 3) / 4;
    const size_t limit = NESTED ? E1_half * E2_len : E2_len / 2;
    if (nch > limit) nch = limit;  // zip() stops at the shorter side
    const int e1_shift = NESTED ? __ffsll((long long)E1_half) - 1 : 0;
    f9 s0 = fr9_zero(), s2 = fr9_zero(), s3 = fr9_zero();
    Layer9Group grp;
    grp.g0 = grp.g2 = grp.g3 = fr9_zero();
    grp.x2 = (size_t)-1;
    size_t c_first, c_end, c_step;
    layer9_walk(NESTED, nch, c_first, c_end, c_step);
    // the trip count is per WAVE (c0 = the wave's first chunk): a wave whose 64 chunks are all inside the layer takes the staged path
    size_t it = 0;
    for (size_t c0 = c_first; c0 < c_end; c0 += c_step, it++) {
        layer9_fold<NESTED>(it, s0, s2, s3, grp);
        const size_t c = c0 + (threadIdx.x & 63);
        if (c0 + 64 <= nch && 4 * (c0 + 64) <= len) {
            Sh9<NC> q[4];
            const fe* comp[2] = {a, b};
#pragma unroll
            for (int k = 0; k < NC; k++) {
                fe raw[4];
                stage_in_rows(reinterpret_cast<const char*>(comp[k] + 4 * c0), 128, st, raw);
#pragma unroll
                for (int j = 0; j < 4; j++) q[j].c[k] = f9_from_fe(raw[j]);
            }
            layer9_terms<NC, NESTED>(q[0], q[1], q[2], q[3], E1, E1_half, e1_shift, E2, c, s0, s2, s3, grp);
        } else if (c < nch) {
            const Sh9<NC> l0 = sh9_load_or_zero<NC>(a, b, 4 * c, len), r0 = sh9_load_or_zero<NC>(a, b, 4 * c + 1, len);
            const Sh9<NC> l1 = sh9_load_or_zero<NC>(a, b, 4 * c + 2, len), r1 = sh9_load_or_zero<NC>(a, b, 4 * c + 3, len);
            layer9_terms<NC, NESTED>(l0, r0, l1, r1, E1, E1_half, e1_shift, E2, c, s0, s2, s3, grp);
        }
    }
    if (NESTED == 2) layer9_group_flush(grp, E2, s0, s2, s3);
    layer9_finish<NESTED>(s0, s2, s3, partial, sh4);
}

template <int NC, int NESTED>
__global__ void __launch_bounds__(PT) k_layer_bind_cubic9(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* oa, fe* ob, size_t len_in, fe r5,
                                                       const fe* __restrict__ E1, size_t E1_half, const fe* __restrict__ E2, size_t E2_len,
                                                       fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const size_t nch_in = (len_in + 3) / 4;
    const size_t len_out = 2 * nch_in;
    const size_t nch_out = (len_out + 3) / 4;
    const size_t limit = NESTED ? E1_half * E2_len : E2_len / 2;
    const int e1_shift = NESTED ? __ffsll((long long)E1_half) - 1 : 0;
    const f9 r9 = f9_from_fe(r5);
    f9 s0 = fr9_zero(), s2 = fr9_zero(), s3 = fr9_zero();
    __shared__ __attribute__((aligned(16))) char stage[PT / 64][ST_WAVE_BYTES];
    char* st = stage[threadIdx.x >> 6];
    Layer9Group grp;
    grp.g0 = grp.g2 = grp.g3 = fr9_zero();
    grp.x2 = (size_t)-1;
    size_t c_first, c_end, c_step;
    layer9_walk(NESTED, nch_out, c_first, c_end, c_step);
    size_t it = 0;
    for (size_t c0 = c_first; c0 < c_end; c0 += c_step, it++) {
        layer9_fold<NESTED>(it, s0, s2, s3, grp);
        const size_t c = c0 + (threadIdx.x & 63);
        Sh9<NC> v[4];
        if (c0 + 64 <= nch_out && 8 * (c0 + 64) <= len_in) {
            // staged: the wave's 64 x 8 inputs come in as whole lines (two halves of 4 elements per lane and component), its
            // 64 x 4 outputs leave as whole lines
            const fe* icomp[2] = {ia, ib};
            fe* ocomp[2] = {oa, ob};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                Sh9<NC> u[4];
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    fe raw[4];
                    stage_in_rows(reinterpret_cast<const char*>(icomp[k] + 8 * c0 + 4 * h), 256, st, raw);
#pragma unroll
                    for (int j = 0; j < 4; j++) u[j].c[k] = f9_from_fe(raw[j]);
                }
                v[2 * h] = sh9_lerp<NC>(u[0], u[2], r9);
                v[2 * h + 1] = sh9_lerp<NC>(u[1], u[3], r9);
            }
#pragma unroll
            for (int k = 0; k < NC; k++) {
                fe outv[4];
#pragma unroll
                for (int j = 0; j < 4; j++) outv[j] = fr9_to_canonical(v[j].c[k]);
                stage_out_rows(reinterpret_cast<char*>(ocomp[k] + 4 * c0), st, outv);
            }
            if (c < limit) layer9_terms<NC, NESTED>(v[0], v[1], v[2], v[3], E1, E1_half, e1_shift, E2, c, s0, s2, s3, grp);
            continue;
        }
        if (c >= nch_out) continue;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const size_t ci = 2 * c + h;
            if (ci < nch_in) {
                const Sh9<NC> u0 = sh9_load_or_zero<NC>(ia, ib, 4 * ci, len_in), u1 = sh9_load_or_zero<NC>(ia, ib, 4 * ci + 1, len_in);
                const Sh9<NC> u2 = sh9_load_or_zero<NC>(ia, ib, 4 * ci + 2, len_in), u3 = sh9_load_or_zero<NC>(ia, ib, 4 * ci + 3, len_in);
                v[2 * h] = sh9_lerp<NC>(u0, u2, r9);
                v[2 * h + 1] = sh9_lerp<NC>(u1, u3, r9);
                sh9_store<NC>(oa, ob, 2 * ci, v[2 * h]);
                sh9_store<NC>(oa, ob, 2 * ci + 1, v[2 * h + 1]);
            } else {
                for (int k = 0; k < NC; k++) v[2 * h].c[k] = v[2 * h + 1].c[k] = fr9_zero();
            }
        }
        if (c < limit) layer9_terms<NC, NESTED>(v[0], v[1], v[2], v[3], E1, E1_half, e1_shift, E2, c, s0, s2, s3, grp);
    }
    if (NESTED == 2) layer9_group_flush(grp, E2, s0, s2, s3);
    layer9_finish<NESTED>(s0, s2, s3, partial, sh4);
}

// One whole sumcheck round of a SMALL layer in a single one-workgroup launch: bind the layer and the split-eq
// tables with the previous challenge (k_layer_bind + SplitEqPolynomial::bind), then the cubic sums of the new
// round (k_layer_cubic) and their block reduction straight into the pinned result slot.  The GKR proof is ~270
// rounds deep and ~200 of them touch <= 8192 elements: as five separate launches each costs more in launch
// gaps than in work.
static constexpr int RT = 1024;
static constexpr size_t ROUND_SMALL_MAX = 2048;  // layer length before the bind (measured: a single workgroup loses above 2^11)
template <int NC>
__global__ void __launch_bounds__(RT) k_layer_round_small(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* oa, fe* ob, size_t len_in,
                                                       int do_bind, fe r, const fe* fold_in, fe* fold_out, size_t fold_n, fe* scale_vec,
                                                       size_t scale_n, const fe* ca, const fe* cb, size_t len, const fe* E1, size_t E1_half,
                                                       const fe* E2, size_t E2_len, int nested, fe* __restrict__ res) {
    __shared__ fe sh16[16];
    if (do_bind) {
        size_t nch_in = (len_in + 3) / 4;
        for (size_t c = threadIdx.x; c < nch_in; c += RT) {
            Sh<NC> lo, hi;
            layer_bind_chunk<NC>(ia, ib, len_in, c, r, oa, ob, lo, hi);
        }
        for (size_t i = threadIdx.x; i < fold_n; i += RT) fe_store(fold_out + i, fold_pair(fold_in, i, r));
        __syncthreads();
        if (scale_n) {  // E1 just collapsed to one value: it multiplies E2 from now on
            fe s = fe_load(fold_out);
            for (size_t i = threadIdx.x; i < scale_n; i += RT) fe_store(scale_vec + i, Fr::mul(fe_load(scale_vec + i), s));
            __syncthreads();
        }
    }
    // This kernel spills (232 / 760 bytes per lane) and its spill size moves with layer_chunk_count and layer_eq_at in place of
    // the next lines, so the clamp and the eq pair stay written out here until the kernel is out of scratch.
    size_t nch = (len + 3) / 4;
    size_t limit = nested ? E1_half * E2_len : E2_len / 2;
    if (nch > limit) nch = limit;
    fe s0 = Fr::zero(), s2 = Fr::zero(), s3 = Fr::zero();
    for (size_t c = threadIdx.x; c < nch; c += RT) {
        fe e[3];
        fe scale = Fr::zero();
        if (nested) {
            size_t x2 = c >> (__ffsll((long long)E1_half) - 1), x1 = c & (E1_half - 1);  // E1_half is a power of two
            eq3(fe_load(E1 + 2 * x1), fe_load(E1 + 2 * x1 + 1), e);
            scale = fe_load(E2 + x2);
        } else {
            eq3(fe_load(E2 + 2 * c), fe_load(E2 + 2 * c + 1), e);
        }
        Sh<NC> l0 = sh_load_or_zero<NC>(ca, cb, 4 * c, len), r0 = sh_load_or_zero<NC>(ca, cb, 4 * c + 1, len);
        Sh<NC> l1 = sh_load_or_zero<NC>(ca, cb, 4 * c + 2, len), r1 = sh_load_or_zero<NC>(ca, cb, 4 * c + 3, len);
        fe t0, t2, t3;
        layer_terms<NC>(l0, r0, l1, r1, e, nested, scale, t0, t2, t3);
        s0 = Fr::add(s0, t0);
        s2 = Fr::add(s2, t2);
        s3 = Fr::add(s3, t3);
    }
    layer_finish(s0, s2, s3, sh16, [&](unsigned k) { return res + k; });
}

// ------------------------------------------------------------------ layer groups (cozk_layer_group_*)
// The same round for k SMALL layers of one length that share the public eq tables, the challenge and the claim (the senders of a
// Shamir prover): ONE launch of k workgroups, workgroup m serving member m.  The members' pointers travel in the kernel arguments,
// four tables of COZK_LAYER_GROUP_MAX pointers (1 KiB) indexed by the wave-uniform blockIdx.x as ShamirExtractArgs' are: scalar
// loads, nothing staged.  Bind, barrier, sums and tails (sh_load_or_zero, the shorter side of layer and eq) are those of
// k_layer_round_small; member m's sums go to res[3 m .. 3 m + 2] of the pinned result slot.  The eq fold is NOT in here: workgroups
// cannot wait for each other, and a fold that all of them wrote would race with the ones that read it.  The caller folds the tables
// once per round with the cozk_spliteq_bind launches in front of this one on the same stream (no host wait in between).
struct LayerGroupArgs {
    const fe* ia[COZK_LAYER_GROUP_MAX];
    const fe* ib[COZK_LAYER_GROUP_MAX];
    fe* oa[COZK_LAYER_GROUP_MAX];
    fe* ob[COZK_LAYER_GROUP_MAX];
};
template <int NC>
__global__ void __launch_bounds__(RT) k_layer_group_round_small(LayerGroupArgs a, size_t len_in, int do_bind, fe r, size_t len, const fe* E1, size_t E1_half,
                                                             const fe* E2, size_t E2_len, int nested, fe* __restrict__ res) {
    // len_in <= ROUND_SMALL_MAX = 2 RT: at most RT / 2 chunks, so a lane owns at most ONE chunk of the bind and ONE of the sums: no
    // grid-stride loop, no accumulator.  With 1024 lanes a wave has 128 registers and k_layer_round_small's unrolled body spills
    // (232 / 760 bytes per lane); here the two halves of the bind and the three points of the sums are ROLLED loops, so that one
    // lerp or one point's products are in the register file at a time, each sum is reduced as soon as its term exists, and nothing
    // but pointers lives across a barrier -- a point reloads its chunk and its eq pair, a few cache-resident kilobytes.
    __shared__ fe sh16[16];
    const unsigned m = blockIdx.x;
    const size_t c = threadIdx.x;
    const fe *ca = a.ia[m], *cb = a.ib[m];  // without a bind the sums read the member as it is
    if (do_bind) {
        const fe *ia = a.ia[m], *ib = a.ib[m];
        fe *oa = a.oa[m], *ob = a.ob[m];
        if (c < (len_in + 3) / 4) {
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                const Sh<NC> lo = sh_load_or_zero<NC>(ia, ib, 4 * c + h, len_in), hi = sh_load_or_zero<NC>(ia, ib, 4 * c + 2 + h, len_in);
                sh_store<NC>(oa, ob, 2 * c + h, sh_lerp<NC>(lo, hi, r));
            }
        }
        __syncthreads();
        ca = oa;
        cb = ob;
    }
    const bool on = c < layer_chunk_count(len, nested, E1_half, E2_len);
    // The terms of k_layer_round_small, (L(X) x R(X)) eq(X) [E2[x2]] at X = 0, 2, 3, with the E2 factor multiplied into eq(X) first:
    // the same field elements, and every stored result is canonical, so the bytes are the same.  The lane's eq pair, and (nested)
    // the E2 entry that multiplies it:
    const fe* ep = E2 + 2 * c;
    const fe* sp = nullptr;
    if (nested) {
        ep = E1 + 2 * (c & (E1_half - 1));               // E1_half is a power of two
        sp = E2 + (c >> (__ffsll((long long)E1_half) - 1));
    }
    // side(s, X): L (s = 0) or R (s = 1) of the lane's chunk at X, from its two elements
    auto side = [&](int s, int X) {
        const Sh<NC> v0 = sh_load_or_zero<NC>(ca, cb, 4 * c + s, len), v1 = sh_load_or_zero<NC>(ca, cb, 4 * c + 2 + s, len);
        if (X == 0) return v0;
        const Sh<NC> d = sh_sub<NC>(v1, v0);
        Sh<NC> v = sh_add<NC>(v1, d);
        if (X == 3) v = sh_add<NC>(v, d);
        return v;
    };
#pragma unroll 1
    for (int p = 0; p < 3; p++) {  // X = 0, 2, 3; rolled: one point's products at a time in the register file
        const int X = p ? p + 1 : 0;
        fe t = Fr::zero();
        if (on) {
            fe e = fe_load(ep);
            if (X) {
                const fe e1 = fe_load(ep + 1), d = Fr::sub(e1, e);
                e = Fr::add(e1, d);
                if (X == 3) e = Fr::add(e, d);
            }
            if (nested) e = Fr::mul(e, fe_load(sp));
            t = Fr::mul(sh_local_mul<NC>(side(0, X), side(1, X)), e);
        }
        t = fr_block_sum(t, sh16);
        if (threadIdx.x == 0) fe_store(res + 3 * m + p, t);
    }
}

// The last bind and the final claims of the first gridDim.x members in one launch: workgroup m (one wave, lanes 0 and 1 at work)
// binds member m's <= 4 elements to its two claims L, R (k_layer_bind on one chunk), stores them as the member's bound layer and
// writes them to res[(2 m + side) NC + component] of the pinned slot.  do_bind = 0: the member is already down to (L, R).
static constexpr int GFT = 64;
template <int NC>
__global__ void __launch_bounds__(GFT) k_layer_group_final(LayerGroupArgs a, size_t len_in, int do_bind, fe r, fe* __restrict__ res) {
    const unsigned m = blockIdx.x, j = threadIdx.x;
    if (j >= 2) return;
    const fe *ia = a.ia[m], *ib = a.ib[m];
    Sh<NC> v;
    if (do_bind) {
        v = sh_lerp<NC>(sh_load_or_zero<NC>(ia, ib, j, len_in), sh_load_or_zero<NC>(ia, ib, j + 2, len_in), r);
        sh_store<NC>(a.oa[m], a.ob[m], j, v);
    } else {
        v = sh_load<NC>(ia, ib, j);
    }
    for (int c = 0; c < NC; c++) fe_store(res + (size_t)(2 * m + j) * NC + c, v.c[c]);
}

// ------------------------------------------------------------------ persistent round kernel (host mailbox)
// A launch-and-drain costs ~38 us on this platform however small the kernel (measured per round, 2^3 .. 2^19
// elements alike), and a grand product has ~170 rounds on layers of <= 2048 elements.  For those tails ONE
// single-workgroup kernel stays resident for all remaining rounds of the layer's sumcheck and talks to the host
// through a mailbox in fine-grained pinned memory: it publishes the three cubic sums of a round, spins (wave 0
// only; the other waves sit at the barrier) until the host has posted the challenge, binds layer + eq tables,
// and goes on -- a PCIe round trip (~3 us) per round instead of a launch.  After the last challenge it binds once
// more and publishes the final claims.  Every wait is bounded by the wall clock (resident_timeout_s() seconds of the
// 100 MHz counter): a host that never answers makes the kernel raise `status` and return, so the grid always drains.
static constexpr size_t HOST_TAIL_CAP = 2048;                 // longest layer a host tail starts from (COZK_HOST_TAIL_MAX is capped here)
static constexpr size_t HOST_TAIL_AREA = 3 * HOST_TAIL_CAP;  // entries of the mailbox's tail area
struct alignas(64) RoundMailbox {
    // host -> device, ONE 64-byte line read by one load instruction (four lanes x 16 B = one PCIe read instead of a poll of the
    // sequence number followed by a read of the challenge): pieces 0..2 = three limbs of the challenge + the challenge's number
    // as a tag in their last word (a 16-byte piece is read whole, the host writes its tag last, so a piece whose tag matches
    // carries its payload), piece 3 = the abort word
    uint32_t cmd[16];
    uint32_t pad0[16];
    uint32_t res_seq;  // device -> host: result number k is ready
    uint32_t status;   // device -> host: 0 ok, 1 timed out waiting for the host, 2 aborted
    uint32_t tail_n[3];  // device -> host, with a handed-over tail: its layer length, E1_len, E2_len (the host checks its own count)
    uint32_t pad2[11];
    fe res[4];         // device -> host: cubic sums g(0), g(2), g(3); final: left.a, left.b, right.a, right.b
    unsigned long long dbg[8];  // device -> host: 100 MHz ticks spent waiting / binding / in the cubic sums / publishing
    // device -> host: the tail handed over to the host (layout of LayerTailView: layer a, layer b, E1, E2), from the resident
    // kernel's last stage or from k_layer_tail_out; the host binds it in place.  A layer of HOST_TAIL_CAP elements in both
    // components and as many eq entries.
    fe tail[HOST_TAIL_AREA];
};
static constexpr long long MB_TICKS_PER_S = 100000000ll;  // wall_clock64() runs at 100 MHz
// watchdog of the resident kernel, seconds (COZK_RESIDENT_TIMEOUT_S, default 10, 1..600): raise it when the round
// callback can legitimately take longer (a coordinator across a slow link)
static int resident_timeout_s() {
    const char* e = getenv("COZK_RESIDENT_TIMEOUT_S");  // read per call (a handful of times per layer): hosts and tests may change it
    int t = e ? atoi(e) : 10;
    return t < 1 ? 1 : (t > 600 ? 600 : t);
}
static constexpr size_t ROUND_PERSIST_MAX = 2048;

// A layer and its live eq tables, copied by one workgroup of nt threads into a host area in the layout of LayerTailView
// (host/layer_tail.hpp): what the host tail of cozk_layer_prove_rounds starts from.  The caller has checked that they fit.
template <int NC>
static __device__ __forceinline__ void layer_tail_out(const fe* la, const fe* lb, size_t len, const fe* E1, size_t E1_len, const fe* E2, size_t E2_len,
                                                      fe* area, int nt) {
    for (size_t i = threadIdx.x; i < len; i += nt) {
        fe_store(area + i, fe_load(la + i));
        if (NC == 2) fe_store(area + len + i, fe_load(lb + i));
    }
    fe* eq = area + NC * len;
    for (size_t i = threadIdx.x; i < E1_len; i += nt) fe_store(eq + i, fe_load(E1 + i));
    for (size_t i = threadIdx.x; i < E2_len; i += nt) fe_store(eq + E1_len + i, fe_load(E2 + i));
}
// the same for a layer that no resident kernel holds (per-round launches, or a layer that starts at the tail's length)
template <int NC>
__global__ void __launch_bounds__(RT) k_layer_tail_out(const fe* la, const fe* lb, size_t len, const fe* E1, size_t E1_len, const fe* E2, size_t E2_len,
                                                    fe* area) {
    layer_tail_out<NC>(la, lb, len, E1, E1_len, E2, E2_len, area, RT);
}
// what a host tail leaves behind, back on the device: the bound layer (2 elements per component) and the live eq entries, at most
// TAIL_BACK_MAX values that travel in the kernel arguments -- no source buffer has to outlive the launch
static constexpr int TAIL_BACK_MAX = 8;
struct TailBackArgs {
    fe v[TAIL_BACK_MAX];
    fe* dst[TAIL_BACK_MAX];
};
__global__ void __launch_bounds__(64) k_layer_tail_back(TailBackArgs a, int n) {
    if ((int)threadIdx.x < n) fe_store(a.dst[threadIdx.x], a.v[threadIdx.x]);
}

template <int NC, int TRACE>
__global__ void __launch_bounds__(RT) k_layer_rounds_persistent(fe* la0, fe* lb0, fe* la1, fe* lb1, int lcur, size_t len, fe* e1_0, fe* e1_1,
                                                             int c1, size_t E1_len, fe* e2_0, fe* e2_1, int c2, size_t E2_len, int nrounds,
                                                             int bind_first, fe r_first, RoundMailbox* mb, long long timeout_ticks, int tail_out) {
    __shared__ fe sh16[16];
    __shared__ fe sh_r;
    __shared__ int sh_ok;
    fe* la[2] = {la0, la1};
    fe* lb[2] = {lb0, lb1};
    fe* e1[2] = {e1_0, e1_1};
    fe* e2[2] = {e2_0, e2_1};
    uint32_t seq = 0;
    long long tk0 = TRACE ? wall_clock64() : 0, tk_wait = 0, tk_bind = 0, tk_cubic = 0, tk_pub = 0;  // TRACE: per-phase device times (COZK_TRACE_ROUNDS)
    // rounds 0 .. nrounds-1 publish cubic sums; "round" nrounds only binds and publishes the final claims, or, with tail_out, the
    // bound layer and the live eq tables, whose remaining rounds the host runs itself (the host has checked that they fit mb->tail)
    for (int round = 0; round <= nrounds; round++) {
        bool do_bind = round > 0 || bind_first;
        fe r = r_first;
        if (TRACE) tk0 = wall_clock64();
        if (round > 0) {
            if (threadIdx.x < 64) {  // wave 0 polls: lanes 0..3 read one 16-byte piece of the command line each
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                const int lane = threadIdx.x;
                const long long t0 = wall_clock64();
                int ok = 1;
                v4u v = {0u, 0u, 0u, 0u};
                for (;;) {
                    if (lane < 4) v = *reinterpret_cast<volatile v4u*>(&mb->cmd[4 * lane]);
                    const unsigned long long ready = __ballot(lane < 3 && v.w == (uint32_t)round);
                    const unsigned long long aborted = __ballot(lane == 3 && v.x != 0u);
                    if ((ready & 7ull) == 7ull) break;
                    if (aborted) {
                        ok = 0;
                        if (lane == 0) __hip_atomic_store(&mb->status, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                    if (__shfl((int)(wall_clock64() - t0 > timeout_ticks), 0)) {  // lane 0's clock decides for the wave
                        ok = 0;
                        if (lane == 0) __hip_atomic_store(&mb->status, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                fe rr;
                rr.l[0] = __shfl(v.x, 0); rr.l[1] = __shfl(v.y, 0); rr.l[2] = __shfl(v.z, 0);
                rr.l[3] = __shfl(v.x, 1); rr.l[4] = __shfl(v.y, 1); rr.l[5] = __shfl(v.z, 1);
                rr.l[6] = __shfl(v.x, 2); rr.l[7] = __shfl(v.y, 2);
                if (lane == 0) {
                    if (ok) sh_r = rr;
                    sh_ok = ok;
                }
            }
            __syncthreads();
            if (!sh_ok) return;  // uniform: every wave reads the same shared word after the barrier
            r = sh_r;
        }
        if (TRACE) {
            long long t = wall_clock64();
            tk_wait += t - tk0;
            tk0 = t;
        }
        if (do_bind) {
            const fe *ia = la[lcur], *ib = lb[lcur];
            fe *oa = la[1 - lcur], *ob = lb[1 - lcur];
            size_t nch_in = (len + 3) / 4;
            for (size_t c = threadIdx.x; c < nch_in; c += RT) {
                Sh<NC> lo, hi;
                layer_bind_chunk<NC>(ia, ib, len, c, r, oa, ob, lo, hi);
            }
            lcur = 1 - lcur;
            len = 2 * nch_in;
            // SplitEqPolynomial::bind
            if (E1_len == 1) {
                size_t n = E2_len / 2;
                const fe* in = e2[c2];
                fe* out = e2[1 - c2];
                // from the LAST thread down: the fold runs on other waves than the layer's bind instead of behind it in the same
                // lanes (a tiny round's bind phase was two dependent load -> product -> store chains back to back: 4.9 us)
                for (size_t i = RT - 1 - threadIdx.x; i < n; i += RT) fe_store(out + i, fold_pair(in, i, r));
                c2 = 1 - c2;
                E2_len = n;
                __syncthreads();
            } else {
                size_t n = E1_len / 2;
                const fe* in = e1[c1];
                fe* out = e1[1 - c1];
                for (size_t i = RT - 1 - threadIdx.x; i < n; i += RT) fe_store(out + i, fold_pair(in, i, r));
                c1 = 1 - c1;
                E1_len = n;
                __syncthreads();
                if (n == 1) {
                    fe sc = fe_load(e1[c1]);
                    fe* v = e2[c2];
                    for (size_t i = threadIdx.x; i < E2_len; i += RT) fe_store(v + i, Fr::mul(fe_load(v + i), sc));
                    __syncthreads();
                }
            }
        }
        seq++;
        if (TRACE) {
            long long t = wall_clock64();
            tk_bind += t - tk0;
            tk0 = t;
        }
        if (round == nrounds) {  // final claims: coeffs[0], coeffs[1] of the fully bound layer
            if (tail_out) {  // all threads, plain vector stores; the binds above are behind a barrier
                layer_tail_out<NC>(la[lcur], lb[lcur], len, e1[c1], E1_len, e2[c2], E2_len, mb->tail, RT);
                __threadfence_system();
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                mb->dbg[0] = (unsigned long long)tk_wait;
                mb->dbg[1] = (unsigned long long)tk_bind;
                mb->dbg[2] = (unsigned long long)tk_cubic;
                mb->dbg[3] = (unsigned long long)tk_pub;
                if (tail_out) {
                    mb->tail_n[0] = (uint32_t)len;
                    mb->tail_n[1] = (uint32_t)E1_len;
                    mb->tail_n[2] = (uint32_t)E2_len;
                } else {
                    fe z = Fr::zero();
                    fe v[4] = {fe_load(la[lcur]), NC == 2 ? fe_load(lb[lcur]) : z, fe_load(la[lcur] + 1), NC == 2 ? fe_load(lb[lcur] + 1) : z};
                    for (int k = 0; k < 4; k++) fe_store(&mb->res[k], v[k]);
                }
                __threadfence_system();
                __hip_atomic_store(&mb->res_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
        // cubic sums of this round.  The serial chain is what a tiny round costs (one dependent Fr product is
        // ~1.3 us on a lone wave), so the three evaluation points go to three groups of five waves: a lane does
        // ONE (chunk, point) term -- l x r and e x scale side by side, then their product -- and the three sums
        // come out of one reduction pass.
        const fe *ca = la[lcur], *cb = lb[lcur];
        const fe *E1 = e1[c1], *E2 = e2[c2];
        const bool nested = E1_len != 1;
        const size_t E1_half = E1_len / 2;
        const size_t nch = layer_chunk_count(len, nested, E1_half, E2_len);
        const int wave = threadIdx.x >> 6;
        const int pt = wave / 5;  // 0, 1, 2 = evaluation at 0, 2, 3; wave 15 idles
        fe acc = Fr::zero();
        if (pt < 3) {
            for (size_t c = threadIdx.x - 320 * pt; c < nch; c += 320) {
                fe e0, e1v, ek;
                if (nested) {
                    size_t x2 = c >> (__ffsll((long long)E1_half) - 1), x1 = c & (E1_half - 1);  // E1_half is a power of two
                    e0 = fe_load(E1 + 2 * x1);
                    e1v = fe_load(E1 + 2 * x1 + 1);
                } else {
                    e0 = fe_load(E2 + 2 * c);
                    e1v = fe_load(E2 + 2 * c + 1);
                }
                Sh<NC> l0 = sh_load_or_zero<NC>(ca, cb, 4 * c, len), r0 = sh_load_or_zero<NC>(ca, cb, 4 * c + 1, len);
                Sh<NC> lk = l0, rk = r0;
                ek = e0;
                if (pt > 0) {
                    Sh<NC> l1 = sh_load_or_zero<NC>(ca, cb, 4 * c + 2, len), r1 = sh_load_or_zero<NC>(ca, cb, 4 * c + 3, len);
                    Sh<NC> ml = sh_sub<NC>(l1, l0), mr = sh_sub<NC>(r1, r0);
                    fe me = Fr::sub(e1v, e0);
                    lk = sh_add<NC>(l1, ml);
                    rk = sh_add<NC>(r1, mr);
                    ek = Fr::add(e1v, me);
                    if (pt == 2) {
                        lk = sh_add<NC>(lk, ml);
                        rk = sh_add<NC>(rk, mr);
                        ek = Fr::add(ek, me);
                    }
                }
                fe lr = sh_local_mul<NC>(lk, rk);
                // same association as k_layer_cubic ((l x r) e) scale: field products are exact, any order agrees
                fe es = nested ? Fr::mul(ek, fe_load(E2 + (c >> (__ffsll((long long)E1_half) - 1)))) : ek;
                acc = Fr::add(acc, Fr::mul(lr, es));
            }
        }
        acc = fr_wave_sum(acc);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh16[wave] = acc;
        __syncthreads();
        if (TRACE) {
            long long t = wall_clock64();
            tk_cubic += t - tk0;
            tk0 = t;
        }
        if (threadIdx.x < 3) {
            fe v = sh16[5 * threadIdx.x];
            for (int i = 1; i < 5; i++) v = Fr::add(v, sh16[5 * threadIdx.x + i]);
            fe_store(&mb->res[threadIdx.x], v);
            __threadfence_system();
        }
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&mb->res_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (TRACE) {
            long long t = wall_clock64();
            tk_pub += t - tk0;
            tk0 = t;
        }
    }
}

// out[j] = L[j] x R[j] (+ mask_j): local half of `mul_vec` (layer_output,
// dense_interleaved_poly.rs:122-141; local product ops.rs:71-78; zero-sharing mask
// mask_j = PRF(key_self, ctr+j) - PRF(key_prev, ctr+j), the keyed ChaCha12 PRF of prf.hip.hpp)
template <int NC>
__global__ void __launch_bounds__(PT) k_layer_output(const fe* __restrict__ a, const fe* __restrict__ b, size_t len,
                                                  fe* __restrict__ out, size_t n_out, int masked, prf_key key_self,
                                                  prf_key key_prev, uint64_t ctr) {
    size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_out) return;
    Sh<NC> l = sh_load_or_zero<NC>(a, b, 2 * j, len), r = sh_load_or_zero<NC>(a, b, 2 * j + 1, len);
    fe v = sh_local_mul<NC>(l, r);
    if (masked) v = Fr::add(v, Fr::sub(prf_fr(key_self, ctr + j), prf_fr(key_prev, ctr + j)));
    fe_store(out + j, v);
}

// element-wise Rep3 mul_vec local part on two share vectors (rep3::arithmetic::mul_vec)
template <int NC>
__global__ void __launch_bounds__(PT) k_mul_vec_local(const fe* __restrict__ xa, const fe* __restrict__ xb,
                                                   const fe* __restrict__ ya, const fe* __restrict__ yb, size_t n,
                                                   fe* __restrict__ out, int masked, prf_key key_self, prf_key key_prev,
                                                   uint64_t ctr) {
    size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n) return;
    fe v = sh_local_mul<NC>(sh_load<NC>(xa, xb, j), sh_load<NC>(ya, yb, j));
    if (masked) v = Fr::add(v, Fr::sub(prf_fr(key_self, ctr + j), prf_fr(key_prev, ctr + j)));
    fe_store(out + j, v);
}

// ------------------------------------------------------------------ kernels: generic product rounds
// One round of `prove_arbitrary_worker` (co-jolt/src/subprotocols/sumcheck.rs:168-246) for the
// comb_funcs the reference uses -- a product of m polynomials of which at most one is shared
// (Spartan inner / shift sumchecks r1cs/spartan/worker.rs:162-235, output check
// read_write_memory/worker.rs:149-164): evaluations at x = 0, 2, .., degree of
// sum_i prod_j P_j(x; i) with HighToLow pairs (i, i + half) (sumcheck_evals, dense_mlpoly.rs:113-147).
// partial[e * gridDim.x + block]; shared factor enters as (a + b), TWO_INV applied by the finisher.
struct ProdRoundPtrs {  // <= 4 factors: the pointer table travels in the kernel arguments (no upload + stream sync per round)
    const fe* a[4];
    const fe* b[4];
};
template <int NC, int M>
__global__ void __launch_bounds__(PT) k_prod_round(ProdRoundPtrs tab, int shared_idx, size_t half, int degree, fe* __restrict__ partial) {
    const fe* const* pa = tab.a;
    const fe* const* pb = tab.b;
    __shared__ fe sh4[4];
    fe acc[4];
    for (int e = 0; e < 4; e++) acc[e] = Fr::zero();
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < half; i += (size_t)gridDim.x * PT) {
        fe cur[M], step[M];
        for (int j = 0; j < M; j++) {
            fe lo, hi;
            if (NC == 2 && j == shared_idx) {
                lo = Fr::add(fe_load(pa[j] + i), fe_load(pb[j] + i));
                hi = Fr::add(fe_load(pa[j] + i + half), fe_load(pb[j] + i + half));
            } else {
                lo = fe_load(pa[j] + i);
                hi = fe_load(pa[j] + i + half);
            }
            step[j] = Fr::sub(hi, lo);
            cur[j] = lo;
        }
        for (int e = 0; e < degree; e++) {
            // points 0, 2, 3, ...: after the first evaluation jump to x = 2
            if (e == 1)
                for (int j = 0; j < M; j++) cur[j] = Fr::add(Fr::add(cur[j], step[j]), step[j]);
            else if (e > 1)
                for (int j = 0; j < M; j++) cur[j] = Fr::add(cur[j], step[j]);
            fe prod = cur[0];
            for (int j = 1; j < M; j++) prod = Fr::mul(prod, cur[j]);
            acc[e] = Fr::add(acc[e], prod);
        }
    }
    for (int e = 0; e < degree; e++) {
        fe v = fr_block_sum(acc[e], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)e * gridDim.x + blockIdx.x, v);
    }
}

// co-spartan sumcheck #1 round (co-noir-spartan/co-spartan/src/sumcheck.rs:171-280): evaluations at
// X = 0..3 of sum_b [ (A x B)(X) * pub(X) - into_additive(C(X) * pub(X)) ], LowToHigh pairs (2b, 2b+1).
// The -C term is accumulated as (c.a + c.b) * pub separately so that TWO_INV is applied once per sum.
template <int NC>
__global__ void __launch_bounds__(PT) k_spartan_first(const fe* __restrict__ aa, const fe* __restrict__ ab, const fe* __restrict__ ba,
                                                   const fe* __restrict__ bb, const fe* __restrict__ ca, const fe* __restrict__ cb,
                                                   const fe* __restrict__ pub, size_t half, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe accp[4], accc[4];
    for (int e = 0; e < 4; e++) {
        accp[e] = Fr::zero();
        accc[e] = Fr::zero();
    }
    for (size_t b = (size_t)blockIdx.x * PT + threadIdx.x; b < half; b += (size_t)gridDim.x * PT) {
        Sh<NC> A = sh_load<NC>(aa, ab, 2 * b), B = sh_load<NC>(ba, bb, 2 * b), C = sh_load<NC>(ca, cb, 2 * b);
        Sh<NC> sA = sh_sub<NC>(sh_load<NC>(aa, ab, 2 * b + 1), A), sB = sh_sub<NC>(sh_load<NC>(ba, bb, 2 * b + 1), B),
               sC = sh_sub<NC>(sh_load<NC>(ca, cb, 2 * b + 1), C);
        fe P = fe_load(pub + 2 * b);
        fe sP = Fr::sub(fe_load(pub + 2 * b + 1), P);
        for (int e = 0; e < 4; e++) {
            accp[e] = Fr::add(accp[e], Fr::mul(sh_local_mul<NC>(A, B), P));
            accc[e] = Fr::add(accc[e], Fr::mul(sh_ab_sum<NC>(C), P));
            A = sh_add<NC>(A, sA);
            B = sh_add<NC>(B, sB);
            C = sh_add<NC>(C, sC);
            P = Fr::add(P, sP);
        }
    }
    for (int e = 0; e < 4; e++) {
        fe v = fr_block_sum(accp[e], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)e * gridDim.x + blockIdx.x, v);
        fe w = fr_block_sum(accc[e], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)(4 + e) * gridDim.x + blockIdx.x, w);
    }
}

// co-spartan sumcheck #2 round (sumcheck.rs:282-395): Rep3 evaluations at X = 0..2 of
// sum_b z(X) * (alpha a(X) + beta b(X) + gamma c(X)); component k of the share lands in partial rows 3k..3k+2
template <int NC>
__global__ void __launch_bounds__(PT) k_spartan_second(const fe* __restrict__ za, const fe* __restrict__ zb, const fe* __restrict__ pa,
                                                    const fe* __restrict__ pbv, const fe* __restrict__ pc, fe c0, fe c1, fe c2,
                                                    size_t half, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe acc[NC][3];
    for (int k = 0; k < NC; k++)
        for (int e = 0; e < 3; e++) acc[k][e] = Fr::zero();
    for (size_t b = (size_t)blockIdx.x * PT + threadIdx.x; b < half; b += (size_t)gridDim.x * PT) {
        Sh<NC> Z = sh_load<NC>(za, zb, 2 * b);
        Sh<NC> sZ = sh_sub<NC>(sh_load<NC>(za, zb, 2 * b + 1), Z);
        fe A = fe_load(pa + 2 * b), B = fe_load(pbv + 2 * b), C = fe_load(pc + 2 * b);
        fe sA = Fr::sub(fe_load(pa + 2 * b + 1), A), sB = Fr::sub(fe_load(pbv + 2 * b + 1), B), sC = Fr::sub(fe_load(pc + 2 * b + 1), C);
        for (int e = 0; e < 3; e++) {
            fe lin = Fr::add(Fr::add(Fr::mul(A, c0), Fr::mul(B, c1)), Fr::mul(C, c2));
            for (int k = 0; k < NC; k++) acc[k][e] = Fr::add(acc[k][e], Fr::mul(Z.c[k], lin));
            Z = sh_add<NC>(Z, sZ);
            A = Fr::add(A, sA);
            B = Fr::add(B, sB);
            C = Fr::add(C, sC);
        }
    }
    for (int k = 0; k < NC; k++)
        for (int e = 0; e < 3; e++) {
            fe v = fr_block_sum(acc[k][e], sh4);
            if (threadIdx.x == 0) fe_store(partial + (size_t)(3 * k + e) * gridDim.x + blockIdx.x, v);
        }
}

// zero_round (co-noir-spartan/co-spartan/src/worker.rs:153-182): za[row] = sum_nnz val_a * z[col] (same for
// b, c) on shares, CSR rows (field sums are order-independent, so COO vs CSR order cannot change a bit)
// Rows up to SPMV_LONG entries: one lane per row.  Longer rows (R1CS has them: the constant-1 column of the
// transposed matrices that `third_round` walks, worker.rs:241-249, holds an entry of almost every constraint)
// are cut into SPMV_CHUNK-entry work items queued on the device: one workgroup reduces one item
// (k_sparse_matvec3_items), then one workgroup per long row adds up its items' partial sums
// (k_sparse_matvec3_rows).  A dense column of 2^18 entries costs two short launches instead of a 2^18-step
// serial loop.  Queue layout in `q`: [0] number of long rows, [1] number of items, then rows[] = (row, first item,
// item count) and items[] = (row, chunk index).
static constexpr uint32_t SPMV_LONG = 64;
static constexpr uint32_t SPMV_CHUNK = 2048;
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_matvec3(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                                                    const fe* __restrict__ va, const fe* __restrict__ vb, const fe* __restrict__ vc,
                                                    const fe* __restrict__ za, const fe* __restrict__ zb, size_t nrows,
                                                    fe* oa0, fe* oa1, fe* ob0, fe* ob1, fe* oc0, fe* oc1,
                                                    uint32_t* __restrict__ q, uint32_t* __restrict__ q_rows, uint32_t* __restrict__ q_items) {
    size_t r = (size_t)blockIdx.x * PT + threadIdx.x;
    if (r >= nrows) return;
    uint32_t e0 = row_ptr[r], e1 = row_ptr[r + 1];
    if (e1 - e0 > SPMV_LONG) {
        uint32_t nchunks = (e1 - e0 + SPMV_CHUNK - 1) / SPMV_CHUNK;
        uint32_t ri = atomicAdd(&q[0], 1u);
        uint32_t first = atomicAdd(&q[1], nchunks);
        q_rows[3 * ri] = (uint32_t)r;
        q_rows[3 * ri + 1] = first;
        q_rows[3 * ri + 2] = nchunks;
        for (uint32_t j = 0; j < nchunks; j++) {
            q_items[2 * (first + j)] = (uint32_t)r;
            q_items[2 * (first + j) + 1] = j;
        }
        return;
    }
    Sh<NC> A, B, C;
    for (int k = 0; k < NC; k++) A.c[k] = B.c[k] = C.c[k] = Fr::zero();
    for (uint32_t e = e0; e < e1; e++) {
        Sh<NC> z = sh_load<NC>(za, zb, col[e]);
        A = sh_add<NC>(A, sh_mul_public<NC>(z, fe_load(va + e)));
        B = sh_add<NC>(B, sh_mul_public<NC>(z, fe_load(vb + e)));
        C = sh_add<NC>(C, sh_mul_public<NC>(z, fe_load(vc + e)));
    }
    sh_store<NC>(oa0, oa1, r, A);
    sh_store<NC>(ob0, ob1, r, B);
    sh_store<NC>(oc0, oc1, r, C);
}
// partial[item][3][NC]: the sums of one SPMV_CHUNK-entry slice of a long row
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_matvec3_items(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                                                          const fe* __restrict__ va, const fe* __restrict__ vb, const fe* __restrict__ vc,
                                                          const fe* __restrict__ za, const fe* __restrict__ zb, const uint32_t* __restrict__ q,
                                                          const uint32_t* __restrict__ q_items, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    uint32_t nitems = q[1];
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {  // every workgroup reaches the end of the queue
        uint32_t r = q_items[2 * it], j = q_items[2 * it + 1];
        uint32_t lo = row_ptr[r] + j * SPMV_CHUNK;
        uint32_t hi = min(lo + SPMV_CHUNK, row_ptr[r + 1]);
        Sh<NC> A, B, C;
        for (int k = 0; k < NC; k++) A.c[k] = B.c[k] = C.c[k] = Fr::zero();
        for (uint32_t e = lo + threadIdx.x; e < hi; e += PT) {
            Sh<NC> z = sh_load<NC>(za, zb, col[e]);
            A = sh_add<NC>(A, sh_mul_public<NC>(z, fe_load(va + e)));
            B = sh_add<NC>(B, sh_mul_public<NC>(z, fe_load(vb + e)));
            C = sh_add<NC>(C, sh_mul_public<NC>(z, fe_load(vc + e)));
        }
        fe* out = partial + (size_t)it * 3 * NC;
        for (int k = 0; k < NC; k++) {
            fe a = fr_block_sum(A.c[k], sh4), b = fr_block_sum(B.c[k], sh4), c = fr_block_sum(C.c[k], sh4);
            if (threadIdx.x == 0) {
                fe_store(out + k, a);
                fe_store(out + NC + k, b);
                fe_store(out + 2 * NC + k, c);
            }
        }
    }
}
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_matvec3_rows(const uint32_t* __restrict__ q, const uint32_t* __restrict__ q_rows,
                                                         const fe* __restrict__ partial, fe* oa0, fe* oa1, fe* ob0, fe* ob1, fe* oc0, fe* oc1) {
    __shared__ fe sh4[4];
    uint32_t nlong = q[0];
    for (uint32_t ri = blockIdx.x; ri < nlong; ri += gridDim.x) {
        uint32_t r = q_rows[3 * ri], first = q_rows[3 * ri + 1], n = q_rows[3 * ri + 2];
        fe acc[3 * NC];
        for (int k = 0; k < 3 * NC; k++) acc[k] = Fr::zero();
        for (uint32_t j = threadIdx.x; j < n; j += PT)
            for (int k = 0; k < 3 * NC; k++) acc[k] = Fr::add(acc[k], fe_load(partial + (size_t)(first + j) * 3 * NC + k));
        fe tot[3 * NC];
        for (int k = 0; k < 3 * NC; k++) tot[k] = fr_block_sum(acc[k], sh4);
        if (threadIdx.x == 0) {
            Sh<NC> A, B, C;
            for (int k = 0; k < NC; k++) {
                A.c[k] = tot[k];
                B.c[k] = tot[NC + k];
                C.c[k] = tot[2 * NC + k];
            }
            sh_store<NC>(oa0, oa1, r, A);
            sh_store<NC>(ob0, ob1, r, B);
            sh_store<NC>(oc0, oc1, r, C);
        }
    }
}

// ------------------------------------------------------------------ kernels: split-eq tables
__global__ void __launch_bounds__(PT) k_fold_pairs(const fe* __restrict__ in, fe* __restrict__ out, size_t n_out, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    fe_store(out + i, fold_pair(in, i, r));
}
__global__ void __launch_bounds__(PT) k_fold_halves(fe* __restrict__ v, size_t n_out, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    fe lo = fe_load(v + i), hi = fe_load(v + i + n_out);
    fe_store(v + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
}
__global__ void __launch_bounds__(PT) k_scale_by_first(fe* __restrict__ v, size_t n, const fe* __restrict__ s) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe_store(v + i, Fr::mul(fe_load(v + i), fe_load(s)));
}
// EqPolynomial::evals(r) on device, big-endian (r[0] <-> MSB): level j doubles the table
__global__ void __launch_bounds__(PT) k_eq_expand(const fe* __restrict__ in, fe* __restrict__ out, size_t n_in, fe rj) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_in) return;
    fe e = fe_load(in + i);
    fe hi = Fr::mul(e, rj);
    fe_store(out + 2 * i, Fr::sub(e, hi));
    fe_store(out + 2 * i + 1, hi);
}

// a table above 2^13 entries as the outer product of two small ones: out[i] = hi[i >> m] x lo[i & (2^m - 1)], hi over the first
// variables (r[0] stays in the most significant index bit), lo over the last m.  Each workgroup takes one contiguous range, 256
// consecutive entries per step, so that a wave reads ONE hi entry (2^m >= 128); both factors and the product are canonical
// (Fr::mul reduces fully), so the bytes are those of the level-by-level table.
__global__ void __launch_bounds__(PT) k_eq_outer(const fe* __restrict__ hi, const fe* __restrict__ lo, int m, size_t n, fe* __restrict__ out) {
    const size_t per = ((n / PT + gridDim.x - 1) / gridDim.x) * PT;  // n is a multiple of PT
    const size_t first = (size_t)blockIdx.x * per, end = first + per < n ? first + per : n;
    const size_t mask = ((size_t)1 << m) - 1;
    for (size_t i = first + threadIdx.x; i < end; i += PT) fe_store(out + i, Fr::mul(fe_load(hi + (i >> m)), fe_load(lo + (i & mask))));
}

// whole EqPolynomial::evals table in one launch (one workgroup; tables here are <= 2^13 entries:
// the two halves of a split-eq): level j doubles the table in place from the top index down
__global__ void k_store_fe(fe* out, fe v) { fe_store(out, v); }
__global__ void k_store_u32s(uint32_t* out, const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, int n0, size_t stride0) {
    // out[i] = in0[i * stride0] for i < n0, then out[n0] = *in1 (small gathers into a pinned slot instead of strided device-to-host copies)
    int i = threadIdx.x;
    if (i < n0) out[i] = in0[(size_t)i * stride0];
    if (i == n0 && in1) out[n0] = *in1;
}
// The point travels in the kernel arguments (<= 13 x 32 B): a grand product builds ~220 of these tables per chained proof, and a
// host-to-device copy of the point plus the stream synchronisation that protects the caller's buffer cost more than the kernel.
struct EqBuildPoint {
    fe r[13];
};
__global__ void __launch_bounds__(1024) k_eq_build(EqBuildPoint pt, int nv, fe* __restrict__ out) {
    if (threadIdx.x == 0) fe_store(out, Fr::one());
    __syncthreads();
    size_t n = 1;
    for (int j = 0; j < nv; j++) {
        fe rj = pt.r[j];
        // read phase, then write phase: entry i expands to (2i, 2i+1)
        fe e[8];
        int cnt = 0;
        for (size_t i = threadIdx.x; i < n; i += 1024) e[cnt++] = fe_load(out + i);
        __syncthreads();
        cnt = 0;
        for (size_t i = threadIdx.x; i < n; i += 1024) {
            fe hi = Fr::mul(e[cnt], rj);
            fe_store(out + 2 * i, Fr::sub(e[cnt], hi));
            fe_store(out + 2 * i + 1, hi);
            cnt++;
        }
        __syncthreads();
        n *= 2;
    }
}

// ------------------------------------------------------------------ host helpers
// from the pool of the context whose ABI call is running on this thread (cozk_guard)
static fe* dev_alloc_fe(size_t n) { return (fe*)ctx_dev_alloc(t_cur_ctx, (n ? n : 1) * sizeof(fe)); }

// COZK_SYNC_ROUNDS (set to anything): wait for round results with hipStreamSynchronize; nothing publishes or spins on the pinned word
static bool sync_rounds() {
    static const bool on = getenv("COZK_SYNC_ROUNDS") != nullptr;
    return on;
}
// COZK_TRACE_ROUNDS (set to anything): the resident round kernel times its phases (it reads the 100 MHz clock four times per round)
// and cozk_layer_prove_rounds prints them
static bool trace_rounds() {
    static const bool on = getenv("COZK_TRACE_ROUNDS") != nullptr;
    return on;
}

// copy k small results from device scratch to host (sync)
// the stream's work up to here has finished: a stream memory write of a sequence number + a host spin on that pinned word replaces
// hipStreamSynchronize's event / interrupt path (tens of microseconds) with a cache-line hand-off (COZK_SYNC_ROUNDS: the blocking wait)
static void stream_drain_by_flag(cozk_ctx* ctx) {
    if (sync_rounds()) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return;
    }
    if (!ctx->round_flag) HIP_TRY(hipHostMalloc((void**)&ctx->round_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    uint32_t seq = ++ctx->round_seq;
    HIP_TRY(hipStreamWriteValue32(ctx->stream, (void*)ctx->round_flag, seq, 0));
    volatile uint32_t* f = ctx->round_flag;
    uint64_t spins = 0;
    while (*f != seq) {
        __builtin_ia32_pause();
        if (++spins > (1ull << 22)) {  // ~10 ms without news: fall back to the blocking wait (also surfaces errors)
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            break;
        }
    }
}
// arm the finishing kernel's own publication of the round (COZK_FLAG_IN_FINISH=0 / COZK_SYNC_ROUNDS: not armed, fetch_fe drains the stream)
static RoundPublish arm_round_publish(cozk_ctx* ctx) {
    static const bool on = !(getenv("COZK_FLAG_IN_FINISH") && atoi(getenv("COZK_FLAG_IN_FINISH")) == 0);
    if (!on || sync_rounds()) return RoundPublish{nullptr, nullptr, 0};
    if (!ctx->round_flag) HIP_TRY(hipHostMalloc((void**)&ctx->round_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    if (!ctx->finish_ticket) {
        HIP_TRY(hipMalloc((void**)&ctx->finish_ticket, 64));
        HIP_TRY(hipMemsetAsync(ctx->finish_ticket, 0, 64, ctx->stream));
    }
    ctx->armed_seq = ++ctx->round_seq;
    return RoundPublish{ctx->finish_ticket, ctx->round_flag, ctx->armed_seq};
}
// copy k small results to the host.  Round results are written by the finishing kernel straight into pinned (device-visible) host
// memory (d == the pinned slot): nothing to copy, only the stream to drain, ~270 times per grand product; anything else is copied
// into the pinned slot first.
static void fetch_fe(cozk_ctx* ctx, const fe* d, size_t k, fe* h) {
    fe* pin = (fe*)ctx_pinned(ctx, k * sizeof(fe));
    const uint32_t armed = ctx->armed_seq;
    ctx->armed_seq = 0;
    if (d == pin && armed) {  // the finishing kernel publishes the sequence number itself
        volatile uint32_t* f = ctx->round_flag;
        uint64_t spins = 0;
        while (*f != armed) {
            __builtin_ia32_pause();
            if (++spins > (1ull << 22)) {  // ~10 ms without news: the blocking wait also surfaces launch errors
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        if (d != pin) HIP_TRY(hipMemcpyAsync(pin, d, k * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        stream_drain_by_flag(ctx);
    }
    for (size_t i = 0; i < k; i++) h[i] = pin[i];
}
// where a finishing kernel should put k round results (pinned host memory, mapped into the device)
static fe* result_slot(cozk_ctx* ctx, size_t k) { return (fe*)ctx_pinned(ctx, k * sizeof(fe)); }

// The two-stage round sums: a kernel writes `rows` rows of gx block partials, k_finish_sums adds each row up into the pinned result
// slot and publishes the round, the host fetches the results.  sum_launch makes the ONE scratch reservation of such a call: `meta_bytes`
// for the caller's pointer tables (at `meta`), then, 32-byte aligned, rows * gx_max + rows partials; gx_max is the LARGEST grid the
// caller may still pick.  `res` is the pinned slot for n_res results (a caller may have kernels of its own write results behind the
// finished rows before it calls finish_sums).
struct SumLaunch {
    fe* partial;
    fe* res;
    char* meta;
    size_t cap;    // partials reserved
    size_t n_res;  // results fetched
};
static SumLaunch sum_launch(cozk_ctx* ctx, unsigned rows, unsigned gx_max, size_t n_res, size_t meta_bytes = 0) {
    const size_t meta = (meta_bytes + 31) & ~(size_t)31, cap = (size_t)rows * gx_max;
    ctx->scratch.reserve(meta + (cap + rows) * sizeof(fe));
    char* base = (char*)ctx->scratch.p;
    return SumLaunch{(fe*)(base + meta), result_slot(ctx, n_res), base, cap, n_res};
}
// k_finish_sums over `rows` rows of `gx` partials with the round's publication armed, the launch check, and the n_res results to
// `out`.  ctx->armed_seq is 0 on every way out, so a failure here cannot make a later fetch_fe wait for a stale sequence number.
static void finish_sums(cozk_ctx* ctx, const SumLaunch& sl, unsigned rows, unsigned gx, fe scale, int apply_scale, fe* out) {
    COZK_REQUIRE((size_t)rows * gx <= sl.cap && rows <= sl.n_res, "finish_sums: more block partials than sum_launch reserved");
    struct Disarm {
        cozk_ctx* ctx;
        ~Disarm() { ctx->armed_seq = 0; }
    } disarm{ctx};
    k_finish_sums<<<rows, PT, 0, ctx->stream>>>(sl.partial, gx, scale, apply_scale, sl.res, arm_round_publish(ctx));
    HIP_TRY(hipGetLastError());
    fetch_fe(ctx, sl.res, sl.n_res, out);
}

// ------------------------------------------------------------------ what the group families share (host only)
// A group (layer, toggle, spartan, outer, shift, primary) drives k members, each its owner's, with launches on the DRIVER's stream.

// The stream-ordering rule of every group: what a member's own stream still does to it precedes the driver's launches (the rule of
// cozk_shamir_scatter: the producer's stream is drained before another stream reads what it wrote).  Each distinct context of `owners`
// is drained once, in the order given; `skip`: a context that is not waited for.
static void drain_streams(const std::vector<cozk_ctx*>& owners, const cozk_ctx* skip = nullptr) {
    for (size_t i = 0; i < owners.size(); i++) {
        cozk_ctx* c = owners[i];
        if (c == skip || std::find(owners.begin(), owners.end(), c) != owners.begin() + (long)i) continue;  // not its first mention
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
}

// The checks on member i that the families share: there with a context, PLAIN (where the family asks for it), on the driver's device,
// not given twice.  The refusal texts name the member with the family's nouns.
struct MemberNouns {
    const char *one, *on_device, *dup;  // "null <one>", "every <one> must be PLAIN", "every <on_device> must live ..", "duplicate <dup>"
};
static constexpr MemberNouns MEMBER{"member", "member", "member"};
template <bool PLAIN, class T>
static void group_member_check(const std::string& what, const MemberNouns& w, const cozk_ctx* driver, T* const* members, int i) {
    const T* m = members[i];
    COZK_REQUIRE(m && m->ctx, what + ": null " + w.one);
    if constexpr (PLAIN) COZK_REQUIRE(m->mode == COZK_MODE_PLAIN, what + ": every " + w.one + " must be PLAIN");
    COZK_REQUIRE(m->ctx->device == driver->device, what + ": every " + w.on_device + " must live on the driver's device");
    for (int j = 0; j < i; j++) COZK_REQUIRE(members[j] != m, what + ": duplicate " + w.dup);
}

// A group's own copy of the public polynomial that its members are summed against, ping-pong, from the driver's pool: a binding round
// reads in(), writes out() (half as long) and advances.
struct GroupPub {
    fe* buf[2] = {nullptr, nullptr};
    int cur = 0;
    size_t len = 0;  // current length = that of every member
    // on a failure the caller frees what was allocated (free)
    void create(cozk_ctx* driver, const cozk_poly* pub) {
        len = pub->len;
        buf[0] = (fe*)ctx_dev_alloc(driver, len * sizeof(fe));
        buf[1] = (fe*)ctx_dev_alloc(driver, (len / 2) * sizeof(fe));
        HIP_TRY(hipMemcpyAsync(buf[0], poly_a(pub), len * sizeof(fe), hipMemcpyDeviceToDevice, driver->stream));
        HIP_TRY(hipStreamSynchronize(driver->stream));
    }
    void free(cozk_ctx* driver) {
        for (int i = 0; i < 2; i++) ctx_dev_free(driver, buf[i]);
    }
    const fe* in() const { return buf[cur]; }
    fe* out() const { return buf[1 - cur]; }
    void advance(size_t new_len) {
        cur = 1 - cur;
        len = new_len;
    }
    void download(cozk_ctx* ctx, uint64_t* out) const {
        std::vector<fe> h(len);
        HIP_TRY(hipMemcpyAsync(h.data(), buf[cur], len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < len; i++) fe_to_u64x4(h[i], out + 4 * i);
    }
};

// The sum step of a round group: `rows` sums (a few per member) over `items` work items per member, blockIdx.y the member.  Small
// members: ONE launch of one workgroup per member that writes its sums straight to the pinned slot.  Otherwise gx <= grid_cap
// workgroups per member write block partials and k_finish_sums adds the rows up.  The caller launches into `partial` with grid.x = gx,
// then fetches.
static constexpr unsigned GROUP_GRID_MAX = 2048;  // workgroups of ONE group round launch over all its members (MAXBLK, shared: a member
                                                  // gets GROUP_GRID_MAX / k of them, and never fewer than 64)
struct GroupSums {
    cozk_ctx* ctx;
    unsigned rows, gx;
    bool small;
    SumLaunch sl;
    fe* partial;
    void fetch(fe* out) const {
        if (small) fetch_fe(ctx, partial, rows, out);
        else finish_sums(ctx, sl, rows, gx, Fr::one(), 0, out);
    }
};
static GroupSums group_sums(cozk_ctx* ctx, unsigned rows, size_t items, bool small, unsigned grid_cap) {
    GroupSums s{ctx, rows, 1u, small, SumLaunch{}, nullptr};
    if (small) s.partial = result_slot(ctx, rows);
    else {
        s.gx = sum_grid(grid_capped(items, grid_cap));
        s.sl = sum_launch(ctx, rows, s.gx, rows);
        s.partial = s.sl.partial;
    }
    return s;
}

// the tail of a group's final call: n <= 4 COZK_LAYER_GROUP_MAX values from the result slot `res` to the caller, 4 words each
static void fetch_u64x4(cozk_ctx* ctx, const fe* res, size_t n, uint64_t* out) {
    fe h[4 * COZK_LAYER_GROUP_MAX];
    COZK_REQUIRE(n <= sizeof h / sizeof h[0], "fetch_u64x4: more values than a group's final call returns");
    fetch_fe(ctx, res, n, h);
    for (size_t i = 0; i < n; i++) fe_to_u64x4(h[i], out + 4 * i);
}

// make ping-pong side `which` of a polynomial or layer hold n elements (both components of a Rep3 object), from and to the pool of
// the object's own context, whichever context's call is running
template <class P>
static void pingpong_ensure(P* p, int which, size_t n) {
    if (p->cap[which] >= n) return;
    for (int c = 0; c < 2; c++) {
        if (p->buf[which][c]) ctx_dev_free(p->ctx, p->buf[which][c]);
        p->buf[which][c] = nullptr;
    }
    const size_t bytes = (n ? n : 1) * sizeof(fe);
    p->buf[which][0] = (fe*)ctx_dev_alloc(p->ctx, bytes);
    if (p->mode == COZK_MODE_REP3) p->buf[which][1] = (fe*)ctx_dev_alloc(p->ctx, bytes);
    p->cap[which] = n;
}

// One bind of a layer, everything but the kernel: the other ping-pong side is made to hold the bound layer, the layer moves on to it,
// and the launcher gets what it reads and writes (component b null for PLAIN).
struct LayerStep {
    const fe *ia, *ib;
    fe *oa, *ob;
    size_t len_in, len_out;
};
static LayerStep layer_advance(cozk_layer* l) {
    const int dst = 1 - l->cur;
    const size_t len_out = 2 * ((l->len + 3) / 4);
    pingpong_ensure(l, dst, len_out);
    const LayerStep s{l->buf[l->cur][0], l->buf[l->cur][1], l->buf[dst][0], l->buf[dst][1], l->len, len_out};
    l->cur = dst;
    l->len = len_out;
    return s;
}

// the round polynomial of compute_cubic through the evaluations [g0, claim - g0, g2, g3] (dense_interleaved_poly.rs:349-365): its four
// additive coefficient shares, low to high
static void cubic_coeffs_out(const fe s[3], const uint64_t prev_claim[4], uint64_t out_coeffs[16]) {
    fe ev[4] = {s[0], Fr::sub(fe_from_u64x4(prev_claim), s[0]), s[1], s[2]};
    fe cf[4];
    unipoly_from_evals(ev, 4, cf);
    for (int i = 0; i < 4; i++) fe_to_u64x4(cf[i], out_coeffs + 4 * i);
}

// build an eq table on device: out (len 2^nv) from point r (host), big-endian.  Up to 2^13 entries: one launch.  Up to 2^26: three
// launches, the tables of the first nv - m and of the last m = ceil(nv / 2) variables, then their outer product (k_eq_outer); `tmp`
// holds the two small tables (eq_tmp_entries).  Above that, or with COZK_EQ_LEVELS set (read per call: the A/B switch and the
// tests' second opinion): level by level through `tmp` as a second table of 2^nv entries.
static constexpr int EQ_BUILD_MAX_NV = 13, EQ_OUTER_MAX_NV = 2 * EQ_BUILD_MAX_NV;
static bool eq_by_levels(int nv) { return nv > EQ_OUTER_MAX_NV || getenv("COZK_EQ_LEVELS") != nullptr; }
// entries of `tmp` that eq_evals_device needs for a table of nv variables
static size_t eq_tmp_entries(int nv) {
    if (nv <= EQ_BUILD_MAX_NV) return 0;
    if (eq_by_levels(nv)) return (size_t)1 << nv;
    const int m = (nv + 1) / 2;
    return ((size_t)1 << m) + ((size_t)1 << (nv - m));
}
static void eq_build_launch(cozk_ctx* ctx, const fe* r, int nv, fe* out) {
    // the point in the kernel arguments
    EqBuildPoint pt;
    for (int j = 0; j < nv; j++) pt.r[j] = r[j];
    for (int j = nv; j < EQ_BUILD_MAX_NV; j++) pt.r[j] = Fr::zero();
    k_eq_build<<<1, 1024, 0, ctx->stream>>>(pt, nv, out);
}
static void eq_evals_device(cozk_ctx* ctx, const fe* r, int nv, fe* out, fe* tmp) {
    if (nv <= EQ_BUILD_MAX_NV) {
        (void)tmp;
        eq_build_launch(ctx, r, nv, out);
        HIP_TRY(hipGetLastError());
        return;
    }
    if (!eq_by_levels(nv)) {
        const int m = (nv + 1) / 2;
        const size_t n = (size_t)1 << nv;
        fe *lo = tmp, *hi = tmp + ((size_t)1 << m);
        eq_build_launch(ctx, r + (nv - m), m, lo);
        eq_build_launch(ctx, r, nv - m, hi);
        k_eq_outer<<<grid_capped(n), PT, 0, ctx->stream>>>(hi, lo, m, n, out);
        HIP_TRY(hipGetLastError());
        return;
    }
    fe* cur = (nv % 2 == 0) ? out : tmp;  // ping-pong so that the last level lands in `out`
    fe* nxt = (nv % 2 == 0) ? tmp : out;
    k_store_fe<<<1, 1, 0, ctx->stream>>>(cur, Fr::one());  // the value travels in the kernel arguments: no copy, no sync
    size_t n = 1;
    for (int j = 0; j < nv; j++) {
        k_eq_expand<<<grid_for(n), PT, 0, ctx->stream>>>(cur, nxt, n, r[j]);
        std::swap(cur, nxt);
        n *= 2;
    }
    HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ C ABI: dense polynomial
extern "C" {

int cozk_poly_create(cozk_ctx* ctx, int mode, const cozk_vec* a, const cozk_vec* b, cozk_poly** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && out && a && a->kind == COZK_SCALAR_FR && (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3),
                     "poly_create: bad argument");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || (b && b->kind == COZK_SCALAR_FR && b->n == a->n), "poly_create: share b missing");
        cozk_poly* p = new cozk_poly();
        p->ctx = ctx;
        p->mode = mode;
        p->len = p->orig_len = a->n;
        p->cur = -1;
        p->own0 = true;
        p->a0 = dev_alloc_fe(a->n);
        p->b0 = nullptr;
        HIP_TRY(hipMemcpyAsync(p->a0, a->d, a->n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
        if (mode == COZK_MODE_REP3) {
            p->b0 = dev_alloc_fe(a->n);
            HIP_TRY(hipMemcpyAsync(p->b0, b->d, a->n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
        }
        *out = p;
    });
}

// zero-copy chunk view over the high variables (`split_poly`, dense_mlpoly.rs:275-301)
int cozk_poly_chunk(cozk_ctx* ctx, const cozk_poly* src, size_t offset, size_t len, cozk_poly** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && src && out && src->cur < 0 && offset + len <= src->orig_len, "poly_chunk: bad argument (source must be unbound)");
        cozk_poly* p = new cozk_poly();
        p->ctx = ctx;
        p->mode = src->mode;
        p->len = p->orig_len = len;
        p->cur = -1;
        p->own0 = false;
        p->a0 = src->a0 + offset;
        p->b0 = src->b0 ? src->b0 + offset : nullptr;
        *out = p;
    });
}

int cozk_poly_free(cozk_poly* p) {
    if (!p) return COZK_OK;
    if (p->own0) {
        if (p->a0) ctx_dev_free(p->ctx, p->a0);
        if (p->b0) ctx_dev_free(p->ctx, p->b0);
    }
    for (int w = 0; w < 2; w++)
        for (int c = 0; c < 2; c++)
            if (p->buf[w][c]) ctx_dev_free(p->ctx, p->buf[w][c]);
    delete p;
    return COZK_OK;
}

size_t cozk_poly_len(const cozk_poly* p) { return p ? p->len : 0; }
int cozk_poly_mode(const cozk_poly* p) { return p ? p->mode : 0; }

// current coefficients -> host (a: len x 4 u64; b likewise or NULL)
int cozk_poly_download(cozk_ctx* ctx, const cozk_poly* p, uint64_t* a, uint64_t* b) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && a, "poly_download: bad argument");
        HIP_TRY(hipMemcpyAsync(a, poly_a(p), p->len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        if (p->mode == COZK_MODE_REP3 && b)
            HIP_TRY(hipMemcpyAsync(b, poly_b(p), p->len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    });
}

// `copy_share_a` (dense_mlpoly.rs:103-110) as a zero-copy view of the current coefficients
int cozk_poly_share_view(cozk_ctx* ctx, const cozk_poly* p, int component, cozk_vec** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && out && (component == 0 || (component == 1 && p->mode == COZK_MODE_REP3)), "poly_share_view: bad argument");
        const fe* d = component == 0 ? poly_a(p) : poly_b(p);
        *out = new cozk_vec{ctx, p->len, COZK_SCALAR_FR, (void*)d, p->len * sizeof(fe), false};
    });
}

// PolynomialBinding::bind / bind_parallel (dense_mlpoly.rs:310-459; the correct `left +` formula
// is used for every case -- see SURVEY 9 on the reference's bind_parallel quirk)
int cozk_poly_bind(cozk_ctx* ctx, cozk_poly* p, const uint64_t r[4], int order) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && r && p->len >= 2 && (order == COZK_LOW_TO_HIGH || order == COZK_HIGH_TO_LOW), "poly_bind: bad argument");
        size_t n = p->len / 2;
        fe rr = fe_from_u64x4(r);
        const fe* ia = poly_a(p);
        const fe* ib = poly_b(p);
        int dst;
        if (p->cur >= 0 && order == COZK_HIGH_TO_LOW) {
            dst = p->cur;  // in place: lane i reads (i, i+n) and writes i
        } else {
            dst = p->cur < 0 ? 0 : 1 - p->cur;
            pingpong_ensure(p, dst, n);
        }
        fe* oa = p->buf[dst][0];
        fe* ob = p->buf[dst][1];
        if (p->mode == COZK_MODE_REP3) {
            if (order == COZK_LOW_TO_HIGH) k_poly_bind<2, COZK_LOW_TO_HIGH><<<grid_for(n), PT, 0, ctx->stream>>>(ia, ib, oa, ob, n, rr);
            else k_poly_bind<2, COZK_HIGH_TO_LOW><<<grid_for(n), PT, 0, ctx->stream>>>(ia, ib, oa, ob, n, rr);
        } else {
            if (order == COZK_LOW_TO_HIGH) k_poly_bind<1, COZK_LOW_TO_HIGH><<<grid_for(n), PT, 0, ctx->stream>>>(ia, ib, oa, ob, n, rr);
            else k_poly_bind<1, COZK_HIGH_TO_LOW><<<grid_for(n), PT, 0, ctx->stream>>>(ia, ib, oa, ob, n, rr);
        }
        HIP_TRY(hipGetLastError());
        p->cur = dst;
        p->len = n;
    });
}

// get_bound_coeff / final_sumcheck_claim (dense_mlpoly.rs:251-257,461-465)
int cozk_poly_get_coeff(cozk_ctx* ctx, const cozk_poly* p, size_t index, uint64_t a[4], uint64_t b[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && a && index < p->len, "poly_get_coeff: bad argument");
        fe h[2];
        fetch_fe(ctx, poly_a(p) + index, 1, &h[0]);
        fe_to_u64x4(h[0], a);
        if (p->mode == COZK_MODE_REP3 && b) {
            fetch_fe(ctx, poly_b(p) + index, 1, &h[1]);
            fe_to_u64x4(h[1], b);
        }
    });
}

// build EqPolynomial::evals(r) on device (big-endian) -> cozk_vec of 2^nv elements
int cozk_eq_evals(cozk_ctx* ctx, const uint64_t* r, int nv, cozk_vec** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && out && nv >= 0 && nv < 40 && (r || nv == 0), "eq_evals: bad argument");
        size_t n = (size_t)1 << nv;
        std::vector<fe> rr(nv);
        for (int j = 0; j < nv; j++) rr[j] = fe_from_u64x4(r + 4 * j);
        fe* d = dev_alloc_fe(n);
        ctx->scratch2.reserve(eq_tmp_entries(nv) * sizeof(fe));  // two half tables, not a second table (512 MiB at nv = 24)
        eq_evals_device(ctx, rr.data(), nv, d, ctx->scratch2.as<fe>());
        *out = new cozk_vec{ctx, n, COZK_SCALAR_FR, d, n * sizeof(fe), true};
    });
}

// Rep3DensePolynomial::batch_evaluate (dense_mlpoly.rs:183-192): out[k] = additive share of poly_k(r)
// = TWO_INV * sum_i (a_i + b_i) chi_i (REP3) or sum_i a_i chi_i (PLAIN).  chi: FR vec, len >= max len.
int cozk_poly_batch_evaluate_at_chi(cozk_ctx* ctx, const cozk_poly* const* polys, size_t k, const cozk_vec* chi,
                                    uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && k > 0 && chi && out && chi->kind == COZK_SCALAR_FR, "batch_evaluate: bad argument");
        int mode = polys[0]->mode;
        size_t maxlen = 0;
        std::vector<const fe*> ha(k), hb(k);
        std::vector<size_t> hl(k);
        for (size_t i = 0; i < k; i++) {
            COZK_REQUIRE(polys[i] && polys[i]->mode == mode, "batch_evaluate: mixed share modes");
            COZK_REQUIRE(polys[i]->len <= chi->n, "batch_evaluate: chi shorter than polynomial");
            ha[i] = poly_a(polys[i]);
            hb[i] = poly_b(polys[i]);
            hl[i] = polys[i]->len;
            if (hl[i] > maxlen) maxlen = hl[i];
        }
        const unsigned gx = grid_capped(maxlen, eval_grid_max());
        const SumLaunch sl = sum_launch(ctx, (unsigned)k, gx, k, k * (2 * sizeof(void*) + sizeof(size_t)));
        const fe** da = (const fe**)sl.meta;
        const fe** db = da + k;
        size_t* dl = (size_t*)(db + k);
        HIP_TRY(hipMemcpyAsync(da, ha.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(db, hb.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dl, hl.data(), k * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
        dim3 grid(gx, (unsigned)((k + 1) / 2));
        {
            // algorithmic bytes: chi read once for the batch, every polynomial once (96 n, then 64 n per extra polynomial: SURVEY 8d K6)
            uint64_t alg = (uint64_t)chi->n * 32;
            for (size_t i = 0; i < k; i++) alg += (uint64_t)hl[i] * (mode == COZK_MODE_REP3 ? 64 : 32);
            ProfScope prof(ctx, COZK_PROF_EVAL_CHI, alg);
            if (mode == COZK_MODE_REP3) k_poly_eval_chi<2><<<grid, PT, 0, ctx->stream>>>(da, db, dl, (const fe*)chi->d, (int)k, sl.partial);
            else k_poly_eval_chi<1><<<grid, PT, 0, ctx->stream>>>(da, db, dl, (const fe*)chi->d, (int)k, sl.partial);
        }
        std::vector<fe> h(k);
        finish_sums(ctx, sl, (unsigned)k, gx, fr_two_inv(), mode == COZK_MODE_REP3 ? 1 : 0, h.data());
        for (size_t i = 0; i < k; i++) fe_to_u64x4(h[i], out + 4 * i);
    });
}

// dot_product_with_public (dense_mlpoly.rs:228-234) -> share (a[4], b[4])
int cozk_poly_dot_product_with_public(cozk_ctx* ctx, const cozk_poly* p, const cozk_vec* pub, uint64_t a[4], uint64_t b[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && pub && a && pub->kind == COZK_SCALAR_FR && pub->n == p->len, "dot_product: length mismatch (zip_eq)");
        const unsigned gx = grid_capped(p->len, BATCH_GRID_MAX);
        const int nc = p->mode == COZK_MODE_REP3 ? 2 : 1;
        const SumLaunch sl = sum_launch(ctx, nc, gx, nc);
        if (nc == 2) k_poly_dot_public<2><<<gx, PT, 0, ctx->stream>>>(poly_a(p), poly_b(p), (const fe*)pub->d, p->len, sl.partial);
        else k_poly_dot_public<1><<<gx, PT, 0, ctx->stream>>>(poly_a(p), poly_b(p), (const fe*)pub->d, p->len, sl.partial);
        fe h[2];
        finish_sums(ctx, sl, nc, gx, Fr::one(), 0, h);
        fe_to_u64x4(h[0], a);
        if (nc == 2 && b) fe_to_u64x4(h[1], b);
    });
}

// Rep3DensePolynomial::linear_combination / Rep3MultilinearPolynomial::linear_combination
// (dense_mlpoly.rs:195-226; multilinear_polynomial.rs:196-296).  A PLAIN polynomial inside a REP3
// combination is a public polynomial entering through its trivial share (P0: a = v, P1: b = v,
// P2: nothing; types.rs:90-96) -- `party_id` selects which.
int cozk_poly_linear_combination(cozk_ctx* ctx, const cozk_poly* const* polys, const uint64_t* coeffs, size_t k,
                                 int out_mode, int party_id, cozk_poly** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && coeffs && k > 0 && out && (out_mode == COZK_MODE_PLAIN || out_mode == COZK_MODE_REP3) &&
                         party_id >= 0 && party_id < 3,
                     "linear_combination: bad argument");
        size_t maxlen = 0;
        std::vector<const fe*> ha(k), hb(k);
        std::vector<size_t> hl(k);
        std::vector<fe> hc(k);
        for (size_t i = 0; i < k; i++) {
            const cozk_poly* p = polys[i];
            COZK_REQUIRE(p, "linear_combination: null polynomial");
            hl[i] = p->len;
            hc[i] = fe_from_u64x4(coeffs + 4 * i);
            if (p->len > maxlen) maxlen = p->len;
            if (p->mode == COZK_MODE_REP3) {
                COZK_REQUIRE(out_mode == COZK_MODE_REP3, "linear_combination: shared input needs a shared output");
                ha[i] = poly_a(p);
                hb[i] = poly_b(p);
            } else if (out_mode == COZK_MODE_REP3) {
                // public polynomial: `add_public` puts it on P0's a / P1's b / nowhere on P2
                // (SharedOrPublic::add_public_assign, co-jolt/src/utils/shared_or_public.rs:150-152)
                ha[i] = party_id == 0 ? poly_a(p) : nullptr;
                hb[i] = party_id == 1 ? poly_a(p) : nullptr;
            } else {
                ha[i] = poly_a(p);
                hb[i] = nullptr;
            }
        }
        cozk_poly* o = new cozk_poly();
        o->ctx = ctx;
        o->mode = out_mode;
        o->len = o->orig_len = maxlen;
        o->cur = -1;
        o->own0 = true;
        o->a0 = dev_alloc_fe(maxlen);
        o->b0 = out_mode == COZK_MODE_REP3 ? dev_alloc_fe(maxlen) : nullptr;
        size_t meta = k * (2 * sizeof(void*) + sizeof(size_t)) + 64 + k * sizeof(fe);
        ctx->scratch.reserve(meta + 64);
        char* base = (char*)ctx->scratch.p;
        const fe** da = (const fe**)base;
        const fe** db = da + k;
        size_t* dl = (size_t*)(db + k);
        fe* dc = (fe*)(((uintptr_t)(dl + k) + 31) & ~(uintptr_t)31);
        HIP_TRY(hipMemcpyAsync(da, ha.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(db, hb.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dl, hl.data(), k * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dc, hc.data(), k * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        {
            // algorithmic bytes: every operand component read once + the result written once ((m + 1) n S)
            uint64_t alg = (uint64_t)maxlen * (out_mode == COZK_MODE_REP3 ? 64 : 32);
            for (size_t i = 0; i < k; i++) alg += (uint64_t)hl[i] * ((ha[i] ? 32 : 0) + (out_mode == COZK_MODE_REP3 && hb[i] ? 32 : 0));
            ProfScope prof(ctx, COZK_PROF_LINCOMB, alg);
            if (out_mode == COZK_MODE_REP3) k_poly_lincomb<2><<<grid_for(maxlen), PT, 0, ctx->stream>>>(da, db, dl, dc, (int)k, o->a0, o->b0, maxlen);
            else k_poly_lincomb<1><<<grid_for(maxlen), PT, 0, ctx->stream>>>(da, db, dl, dc, (int)k, o->a0, o->b0, maxlen);
        }
        HIP_TRY(hipGetLastError());
        *out = o;
    });
}

// compute_leaves (K11): see k_fingerprint_leaves.  Writes n leaves at out_a/out_b[offset ..]; public polynomials
// (MODE_PLAIN) among `polys` count as part of the public term when the output is REP3.
int cozk_fingerprint_leaves(cozk_ctx* ctx, const cozk_vec* const* cols, const uint64_t* col_coeffs, size_t ks, const cozk_poly* const* polys,
                            const uint64_t* poly_coeffs, size_t kp, const uint64_t constant[4], int mode, int party_id, cozk_vec* out_a,
                            cozk_vec* out_b, size_t offset, size_t n) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && constant && out_a && out_a->kind == COZK_SCALAR_FR && (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3) &&
                         party_id >= 0 && party_id < 3 && n > 0 && offset + n <= out_a->n && (ks == 0 || (cols && col_coeffs)) &&
                         (kp == 0 || (polys && poly_coeffs)) && ks <= 32 && kp <= 32,
                     "fingerprint_leaves: bad argument");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || (out_b && out_b->kind == COZK_SCALAR_FR && out_b->n == out_a->n), "fingerprint_leaves: share b output missing");
        std::vector<SmallCol> hcols(ks);
        std::vector<fe> hcs(ks), hds(kp);
        std::vector<const fe*> ha(kp), hb(kp);
        for (size_t k = 0; k < ks; k++) {
            const cozk_vec* v = cols[k];
            COZK_REQUIRE(v && v->n >= n && (v->kind == COZK_SCALAR_U8 || v->kind == COZK_SCALAR_U16 || v->kind == COZK_SCALAR_U32 || v->kind == COZK_SCALAR_U64),
                         "fingerprint_leaves: compact columns are U8 / U16 / U32 / U64 vectors of >= n entries");
            hcols[k] = SmallCol{v->d, v->kind};
            hcs[k] = Fr::to_mont(fe_from_u64x4(col_coeffs + 4 * k));  // c * R^2: one product with a plain integer -> Montgomery c * v
        }
        for (size_t j = 0; j < kp; j++) {
            const cozk_poly* p = polys[j];
            COZK_REQUIRE(p && p->len >= n, "fingerprint_leaves: polynomial shorter than n");
            hds[j] = fe_from_u64x4(poly_coeffs + 4 * j);
            if (p->mode == COZK_MODE_REP3) {
                COZK_REQUIRE(mode == COZK_MODE_REP3, "fingerprint_leaves: shared input needs a shared output");
                ha[j] = poly_a(p);
                hb[j] = poly_b(p);
            } else if (mode == COZK_MODE_REP3) {
                ha[j] = party_id == 0 ? poly_a(p) : nullptr;  // add_public: P0's a, P1's b
                hb[j] = party_id == 1 ? poly_a(p) : nullptr;
            } else {
                ha[j] = poly_a(p);
                hb[j] = nullptr;
            }
        }
        fe cst0 = fe_from_u64x4(constant);
        if (ks <= 16 && kp <= 8) {
            FingerprintArgs fa;
            memset(&fa, 0, sizeof fa);
            for (size_t k = 0; k < ks; k++) {
                fa.cols[k] = hcols[k];
                fa.cs[k] = hcs[k];
            }
            for (size_t j = 0; j < kp; j++) {
                fa.pa[j] = ha[j];
                fa.pb[j] = hb[j];
                fa.ds[j] = hds[j];
            }
            fe* oa0 = (fe*)out_a->d + offset;
            if (mode == COZK_MODE_REP3)
                k_fingerprint_leaves_args<2><<<grid_for(n), PT, 0, ctx->stream>>>(fa, (int)ks, (int)kp, cst0, party_id == 0, party_id == 1, oa0,
                                                                                 (fe*)out_b->d + offset, n);
            else
                k_fingerprint_leaves_args<1><<<grid_for(n), PT, 0, ctx->stream>>>(fa, (int)ks, (int)kp, cst0, 1, 0, oa0, nullptr, n);
            HIP_TRY(hipGetLastError());
            return;
        }
        size_t meta = ks * sizeof(SmallCol) + 64 + (ks + kp) * sizeof(fe) + 64 + 2 * kp * sizeof(void*) + 64;
        ctx->scratch.reserve(meta);
        char* base = (char*)ctx->scratch.p;
        SmallCol* dcols = (SmallCol*)base;
        fe* dcs = (fe*)(((uintptr_t)(dcols + ks) + 31) & ~(uintptr_t)31);
        fe* dds = dcs + ks;
        const fe** da = (const fe**)(((uintptr_t)(dds + kp) + 15) & ~(uintptr_t)15);
        const fe** db = da + kp;
        if (ks) {
            HIP_TRY(hipMemcpyAsync(dcols, hcols.data(), ks * sizeof(SmallCol), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(dcs, hcs.data(), ks * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        }
        if (kp) {
            HIP_TRY(hipMemcpyAsync(dds, hds.data(), kp * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(da, ha.data(), kp * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(db, hb.data(), kp * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the staging vectors live on this stack frame
        fe cst = fe_from_u64x4(constant);
        fe* oa = (fe*)out_a->d + offset;
        if (mode == COZK_MODE_REP3)
            k_fingerprint_leaves<2><<<grid_for(n), PT, 0, ctx->stream>>>(dcols, dcs, (int)ks, da, db, dds, (int)kp, cst, party_id == 0, party_id == 1, oa,
                                                                        (fe*)out_b->d + offset, n);
        else
            k_fingerprint_leaves<1><<<grid_for(n), PT, 0, ctx->stream>>>(dcols, dcs, (int)ks, da, db, dds, (int)kp, cst, 1, 0, oa, nullptr, n);
        HIP_TRY(hipGetLastError());
    });
}

// one round of the batched opening-reduction sumcheck for the openings that are "live" this round
// (compute_quadratic, opening_proof.rs:374-414): out[2*i] = eval_0, out[2*i+1] = eval_2 as additive
// shares (REP3: TWO_INV * (a+b) already applied; PLAIN: the value).
int cozk_open_quadratic_evals(cozk_ctx* ctx, const cozk_poly* const* polys, const cozk_poly* const* eqs, size_t k,
                              uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && eqs && k > 0 && out, "open_quadratic: bad argument");
        COZK_REQUIRE(polys[0], "open_quadratic: null polynomial");
        int mode = polys[0]->mode;
        std::vector<const fe*> ha(k), hb(k), he(k);
        std::vector<size_t> hh(k);
        size_t maxh = 0;
        for (size_t i = 0; i < k; i++) {
            COZK_REQUIRE(polys[i] && eqs[i] && polys[i]->mode == mode && eqs[i]->mode == COZK_MODE_PLAIN &&
                             eqs[i]->len == polys[i]->len && polys[i]->len >= 2,
                         "open_quadratic: polynomial / eq mismatch");
            ha[i] = poly_a(polys[i]);
            hb[i] = poly_b(polys[i]);
            he[i] = poly_a(eqs[i]);
            hh[i] = polys[i]->len / 2;
            if (hh[i] > maxh) maxh = hh[i];
        }
        const unsigned gx = grid_capped(maxh, BATCH_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, (unsigned)(2 * k), gx, 2 * k, k * (3 * sizeof(void*) + sizeof(size_t)));
        fe* partial = sl.partial;
        const fe** da = (const fe**)sl.meta;
        const fe** db = da + k;
        const fe** de = db + k;
        size_t* dh = (size_t*)(de + k);
        dim3 grid(gx, (unsigned)k);
        if (k <= 16) {
            OpenQuadArgs args;
            for (size_t i = 0; i < 16; i++) {
                args.a[i] = i < k ? ha[i] : nullptr;
                args.b[i] = i < k ? hb[i] : nullptr;
                args.eq[i] = i < k ? he[i] : nullptr;
                args.half[i] = i < k ? hh[i] : 0;
            }
            if (mode == COZK_MODE_REP3) k_open_quadratic_args<2><<<grid, PT, 0, ctx->stream>>>(args, partial);
            else k_open_quadratic_args<1><<<grid, PT, 0, ctx->stream>>>(args, partial);
        } else {
            HIP_TRY(hipMemcpyAsync(da, ha.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(db, hb.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(de, he.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(dh, hh.data(), k * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (mode == COZK_MODE_REP3) k_open_quadratic<2><<<grid, PT, 0, ctx->stream>>>(da, db, de, dh, partial);
            else k_open_quadratic<1><<<grid, PT, 0, ctx->stream>>>(da, db, de, dh, partial);
        }
        std::vector<fe> h(2 * k);
        finish_sums(ctx, sl, (unsigned)(2 * k), gx, fr_two_inv(), mode == COZK_MODE_REP3 ? 1 : 0, h.data());
        for (size_t i = 0; i < 2 * k; i++) fe_to_u64x4(h[i], out + 4 * i);
    });
}

// one round of prove_arbitrary_worker's evaluation loop (sumcheck.rs:189-215) for a product of m
// polynomials (<= 4), at most one of them REP3: out[e] = additive evaluation at x = 0, 2, .., degree
// (e = 0..degree-1).  All polynomials must have the same (current) length; HighToLow.
int cozk_prod_sumcheck_evals(cozk_ctx* ctx, const cozk_poly* const* polys, size_t m, int degree, uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && out && m >= 1 && m <= 4 && degree >= 1 && degree <= 4, "prod_sumcheck: bad argument");
        COZK_REQUIRE(polys[0], "prod_sumcheck: null polynomial");
        size_t len = polys[0]->len;
        int shared = -1;
        const fe* ha[4] = {nullptr, nullptr, nullptr, nullptr};
        const fe* hb[4] = {nullptr, nullptr, nullptr, nullptr};
        for (size_t j = 0; j < m; j++) {
            COZK_REQUIRE(polys[j] && polys[j]->len == len && len >= 2, "prod_sumcheck: length mismatch");
            ha[j] = poly_a(polys[j]);
            hb[j] = poly_b(polys[j]);
            if (polys[j]->mode == COZK_MODE_REP3) {
                COZK_REQUIRE(shared < 0, "prod_sumcheck: at most one shared factor (a shared x shared product needs a reshare)");
                shared = (int)j;
            }
        }
        size_t half = len / 2;
        const unsigned gx = grid_capped(half, BATCH_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, 4, gx, (size_t)degree);
        ProdRoundPtrs tab;
        for (int j = 0; j < 4; j++) {
            tab.a[j] = ha[j];
            tab.b[j] = hb[j];
        }
        using ProdRoundKernel = void (*)(ProdRoundPtrs, int, size_t, int, fe*);
        static const ProdRoundKernel kernels[2][4] = {{k_prod_round<1, 1>, k_prod_round<1, 2>, k_prod_round<1, 3>, k_prod_round<1, 4>},
                                                      {k_prod_round<2, 1>, k_prod_round<2, 2>, k_prod_round<2, 3>, k_prod_round<2, 4>}};  // [shared][m - 1]
        kernels[shared >= 0][m - 1]<<<gx, PT, 0, ctx->stream>>>(tab, shared, half, degree, sl.partial);
        fe h[4];
        finish_sums(ctx, sl, (unsigned)degree, gx, fr_two_inv(), shared >= 0 ? 1 : 0, h);
        for (int e = 0; e < degree; e++) fe_to_u64x4(h[e], out + 4 * e);
    });
}

// Rep3Sumcheck::first_sumcheck_prove_round evaluations (co-spartan/src/sumcheck.rs:171-280), before the
// additive zero-mask: out[t] for X = t = 0..3.  za, zb, zc share polys (same mode), pub a PLAIN poly.
int cozk_spartan_first_round(cozk_ctx* ctx, const cozk_poly* za, const cozk_poly* zb, const cozk_poly* zc, const cozk_poly* pub,
                             uint64_t out[16]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && za && zb && zc && pub && out && pub->mode == COZK_MODE_PLAIN && za->mode == zb->mode && za->mode == zc->mode &&
                         za->len == zb->len && za->len == zc->len && za->len == pub->len && za->len >= 2,
                     "spartan_first_round: bad argument");
        size_t half = za->len / 2;
        const unsigned gx = grid_capped(half, BATCH_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, 8, gx, 8);
        fe* partial = sl.partial;
        if (za->mode == COZK_MODE_REP3)
            k_spartan_first<2><<<gx, PT, 0, ctx->stream>>>(poly_a(za), poly_b(za), poly_a(zb), poly_b(zb), poly_a(zc), poly_b(zc), poly_a(pub), half, partial);
        else
            k_spartan_first<1><<<gx, PT, 0, ctx->stream>>>(poly_a(za), nullptr, poly_a(zb), nullptr, poly_a(zc), nullptr, poly_a(pub), half, partial);
        fe h[8];
        finish_sums(ctx, sl, 8, gx, Fr::one(), 0, h);
        for (int e = 0; e < 4; e++) {
            fe c = za->mode == COZK_MODE_REP3 ? Fr::mul(h[4 + e], fr_two_inv()) : h[4 + e];
            fe_to_u64x4(Fr::sub(h[e], c), out + 4 * e);
        }
    });
}

// Rep3Sumcheck::second_sumcheck_prove_round evaluations (sumcheck.rs:282-395), before the Rep3 mask:
// out_a[t], out_b[t] for X = t = 0..2 (out_b = 0 for PLAIN).  coef = (alpha, beta, gamma), 12 u64.
int cozk_spartan_second_round(cozk_ctx* ctx, const cozk_poly* z, const cozk_poly* a, const cozk_poly* b, const cozk_poly* c,
                              const uint64_t coef[12], uint64_t out_a[12], uint64_t out_b[12]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && z && a && b && c && coef && out_a && out_b && a->mode == COZK_MODE_PLAIN && b->mode == COZK_MODE_PLAIN &&
                         c->mode == COZK_MODE_PLAIN && z->len == a->len && z->len == b->len && z->len == c->len && z->len >= 2,
                     "spartan_second_round: bad argument");
        size_t half = z->len / 2;
        const unsigned gx = grid_capped(half, BATCH_GRID_MAX);
        const int nc = z->mode == COZK_MODE_REP3 ? 2 : 1;
        const SumLaunch sl = sum_launch(ctx, 3 * nc, gx, (size_t)(3 * nc));
        fe* partial = sl.partial;
        fe c0 = fe_from_u64x4(coef), c1 = fe_from_u64x4(coef + 4), c2 = fe_from_u64x4(coef + 8);
        if (nc == 2) k_spartan_second<2><<<gx, PT, 0, ctx->stream>>>(poly_a(z), poly_b(z), poly_a(a), poly_a(b), poly_a(c), c0, c1, c2, half, partial);
        else k_spartan_second<1><<<gx, PT, 0, ctx->stream>>>(poly_a(z), nullptr, poly_a(a), poly_a(b), poly_a(c), c0, c1, c2, half, partial);
        fe h[6];
        finish_sums(ctx, sl, 3 * nc, gx, Fr::one(), 0, h);
        for (int e = 0; e < 3; e++) {
            fe_to_u64x4(h[e], out_a + 4 * e);
            if (nc == 2) fe_to_u64x4(h[3 + e], out_b + 4 * e);
            else for (int k = 0; k < 4; k++) out_b[4 * e + k] = 0;
        }
    });
}

// SpartanProverWorker::zero_round (co-spartan/src/worker.rs:153-182): (za, zb, zc) = (A, B, C) . z on shares.
// CSR: row_ptr (U32, nrows + 1), col (U32, nnz), val_a/b/c (FR, nnz).
int cozk_sparse_matvec3(cozk_ctx* ctx, const cozk_vec* row_ptr, const cozk_vec* col, const cozk_vec* val_a, const cozk_vec* val_b,
                        const cozk_vec* val_c, const cozk_poly* z, cozk_poly** out_za, cozk_poly** out_zb, cozk_poly** out_zc) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && row_ptr && col && val_a && val_b && val_c && z && out_za && out_zb && out_zc &&
                         row_ptr->kind == COZK_SCALAR_U32 && col->kind == COZK_SCALAR_U32 && val_a->kind == COZK_SCALAR_FR &&
                         val_b->kind == COZK_SCALAR_FR && val_c->kind == COZK_SCALAR_FR && row_ptr->n >= 2 &&
                         val_a->n == col->n && val_b->n == col->n && val_c->n == col->n,
                     "sparse_matvec3: bad argument");
        size_t nrows = row_ptr->n - 1;
        cozk_poly* o[3];
        for (int i = 0; i < 3; i++) {
            o[i] = new cozk_poly();
            o[i]->ctx = ctx;
            o[i]->mode = z->mode;
            o[i]->len = o[i]->orig_len = nrows;
            o[i]->cur = -1;
            o[i]->own0 = true;
            o[i]->a0 = dev_alloc_fe(nrows);
            o[i]->b0 = z->mode == COZK_MODE_REP3 ? dev_alloc_fe(nrows) : nullptr;
        }
        // device-side queues of the long rows and of their SPMV_CHUNK-entry work items, and the items' partial sums
        const size_t nnz = col->n;
        const size_t max_rows = nnz / SPMV_LONG + 1, max_items = nnz / SPMV_CHUNK + max_rows;
        const int nc = z->mode == COZK_MODE_REP3 ? 2 : 1;
        const size_t q_words = 16 + 3 * max_rows + 2 * max_items;
        const size_t q_bytes = (q_words * sizeof(uint32_t) + 63) & ~(size_t)63;
        ctx->scratch.reserve(q_bytes + max_items * 3 * nc * sizeof(fe));
        uint32_t* q = ctx->scratch.as<uint32_t>();
        uint32_t* q_rows = q + 16;
        uint32_t* q_items = q_rows + 3 * max_rows;
        fe* partial = reinterpret_cast<fe*>(reinterpret_cast<char*>(ctx->scratch.p) + q_bytes);
        HIP_TRY(hipMemsetAsync(q, 0, 2 * sizeof(uint32_t), ctx->stream));
        const uint32_t* rp = (const uint32_t*)row_ptr->d;
        const uint32_t* ci = (const uint32_t*)col->d;
        const fe *pa = (const fe*)val_a->d, *pb = (const fe*)val_b->d, *pc = (const fe*)val_c->d;
        unsigned g_items = (unsigned)std::min<size_t>(max_items, 4096), g_rows = (unsigned)std::min<size_t>(max_rows, 1024);
        if (z->mode == COZK_MODE_REP3) {
            k_sparse_matvec3<2><<<grid_for(nrows), PT, 0, ctx->stream>>>(rp, ci, pa, pb, pc, poly_a(z), poly_b(z), nrows, o[0]->a0, o[0]->b0, o[1]->a0,
                                                                        o[1]->b0, o[2]->a0, o[2]->b0, q, q_rows, q_items);
            k_sparse_matvec3_items<2><<<g_items, PT, 0, ctx->stream>>>(rp, ci, pa, pb, pc, poly_a(z), poly_b(z), q, q_items, partial);
            k_sparse_matvec3_rows<2><<<g_rows, PT, 0, ctx->stream>>>(q, q_rows, partial, o[0]->a0, o[0]->b0, o[1]->a0, o[1]->b0, o[2]->a0, o[2]->b0);
        } else {
            k_sparse_matvec3<1><<<grid_for(nrows), PT, 0, ctx->stream>>>(rp, ci, pa, pb, pc, poly_a(z), nullptr, nrows, o[0]->a0, nullptr, o[1]->a0, nullptr,
                                                                        o[2]->a0, nullptr, q, q_rows, q_items);
            k_sparse_matvec3_items<1><<<g_items, PT, 0, ctx->stream>>>(rp, ci, pa, pb, pc, poly_a(z), nullptr, q, q_items, partial);
            k_sparse_matvec3_rows<1><<<g_rows, PT, 0, ctx->stream>>>(q, q_rows, partial, o[0]->a0, nullptr, o[1]->a0, nullptr, o[2]->a0, nullptr);
        }
        HIP_TRY(hipGetLastError());
        *out_za = o[0];
        *out_zb = o[1];
        *out_zc = o[2];
    });
}

// PST13 `open` fold step (pst13.rs:445-459): r (len 2h) -> q (len h), r' (len h)
int cozk_pst_fold(cozk_ctx* ctx, const cozk_vec* r, const uint64_t p[4], cozk_vec* q, cozk_vec* r_next) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && r && p && q && r_next && r->kind == COZK_SCALAR_FR && r->n >= 2 && r->n % 2 == 0 &&
                         q->n >= r->n / 2 && r_next->n >= r->n / 2,
                     "pst_fold: bad argument");
        // the kernel stores r->n / 2 field elements into each: an element count alone would let a U8 vector of that many BYTES through
        COZK_REQUIRE(q->kind == COZK_SCALAR_FR && r_next->kind == COZK_SCALAR_FR, "pst_fold: q and r_next must be FR vectors");
        size_t h = r->n / 2;
        k_pst_fold<<<grid_for(h), PT, 0, ctx->stream>>>((const fe*)r->d, (fe*)q->d, (fe*)r_next->d, h, fe_from_u64x4(p));
        HIP_TRY(hipGetLastError());
    });
}

// ------------------------------------------------------------------ C ABI: interleaved GKR layer
int cozk_layer_create(cozk_ctx* ctx, int mode, const cozk_vec* a, const cozk_vec* b, int take_ownership, cozk_layer** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && out && a && a->kind == COZK_SCALAR_FR && a->n % 2 == 0 && (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3),
                     "layer_create: bad argument (coeffs.len() % 2 == 0, dense_interleaved_poly.rs:62)");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || (b && b->kind == COZK_SCALAR_FR && b->n == a->n), "layer_create: share b missing");
        cozk_layer* l = new cozk_layer();
        l->ctx = ctx;
        l->mode = mode;
        l->len = a->n;
        l->cur = 0;
        l->cap[0] = a->n;
        if (take_ownership) {
            COZK_REQUIRE(a->owned && (mode == COZK_MODE_PLAIN || b->owned), "layer_create: cannot take ownership of a view");
            l->buf[0][0] = (fe*)a->d;
            const_cast<cozk_vec*>(a)->owned = false;
            if (mode == COZK_MODE_REP3) {
                l->buf[0][1] = (fe*)b->d;
                const_cast<cozk_vec*>(b)->owned = false;
            }
        } else {
            l->buf[0][0] = dev_alloc_fe(a->n);
            HIP_TRY(hipMemcpyAsync(l->buf[0][0], a->d, a->n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            if (mode == COZK_MODE_REP3) {
                l->buf[0][1] = dev_alloc_fe(a->n);
                HIP_TRY(hipMemcpyAsync(l->buf[0][1], b->d, a->n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        *out = l;
    });
}

int cozk_layer_free(cozk_layer* l) {
    if (!l) return COZK_OK;
    for (int w = 0; w < 2; w++)
        for (int c = 0; c < 2; c++)
            if (l->buf[w][c]) ctx_dev_free(l->ctx, l->buf[w][c]);
    delete l;
    return COZK_OK;
}

size_t cozk_layer_len(const cozk_layer* l) { return l ? l->len : 0; }

int cozk_layer_download(cozk_ctx* ctx, const cozk_layer* l, uint64_t* a, uint64_t* b) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && a, "layer_download: bad argument");
        HIP_TRY(hipMemcpyAsync(a, l->buf[l->cur][0], l->len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        if (l->mode == COZK_MODE_REP3 && b)
            HIP_TRY(hipMemcpyAsync(b, l->buf[l->cur][1], l->len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    });
}

// deep copy (the GKR prover binds layers destructively; tests and the harness keep the originals)
int cozk_layer_clone(cozk_ctx* ctx, const cozk_layer* src, cozk_layer** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && src && out, "layer_clone: bad argument");
        cozk_layer* l = new cozk_layer();
        l->ctx = ctx;
        l->mode = src->mode;
        l->len = src->len;
        l->cur = 0;
        l->cap[0] = src->len;
        for (int c = 0; c < (src->mode == COZK_MODE_REP3 ? 2 : 1); c++) {
            l->buf[0][c] = dev_alloc_fe(src->len);
            HIP_TRY(hipMemcpyAsync(l->buf[0][c], src->buf[src->cur][c], src->len * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
        }
        *out = l;
    });
}

int cozk_layer_as_poly(cozk_ctx* ctx, const cozk_layer* l, cozk_poly** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && out, "layer_as_poly: bad argument");
        cozk_poly* p = new cozk_poly();
        p->ctx = ctx;
        p->mode = l->mode;
        p->len = p->orig_len = l->len;
        p->cur = -1;
        p->own0 = false;
        p->a0 = l->buf[l->cur][0];
        p->b0 = l->buf[l->cur][1];
        *out = p;
    });
}

// Rep3Bindable::bind (dense_interleaved_poly.rs:155-195)
int cozk_layer_bind(cozk_ctx* ctx, cozk_layer* l, const uint64_t r[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && r && l->len >= 2, "layer_bind: bad argument");
        const LayerStep b = layer_advance(l);
        auto* const kernel = l->mode == COZK_MODE_REP3 ? k_layer_bind<2> : k_layer_bind<1>;
        kernel<<<grid_for(b.len_out / 2), PT, 0, ctx->stream>>>(b.ia, b.ib, b.oa, b.ob, b.len_in, fe_from_u64x4(r));
        HIP_TRY(hipGetLastError());
    });
}

// SplitEqPolynomial::new(w) (jolt-core; m = len/2, E2 = evals(w[..m]), E1 = evals(w[m..]))
int cozk_spliteq_new(cozk_ctx* ctx, const uint64_t* w, int nv, cozk_spliteq** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && out && nv >= 0 && nv < 60 && (w || nv == 0), "spliteq_new: bad argument");
        int m = nv / 2;
        cozk_spliteq* e = new cozk_spliteq();
        e->ctx = ctx;
        e->num_vars = nv;
        e->E2_len = e->E2_cap = (size_t)1 << m;
        e->E1_len = e->E1_cap = (size_t)1 << (nv - m);
        for (int k = 0; k < 2; k++) {
            e->E1[k] = dev_alloc_fe(e->E1_cap);
            e->E2[k] = dev_alloc_fe(e->E2_cap);
        }
        std::vector<fe> rr(nv);
        for (int j = 0; j < nv; j++) rr[j] = fe_from_u64x4(w + 4 * j);
        eq_evals_device(ctx, rr.data(), m, e->E2[0], e->E2[1]);
        eq_evals_device(ctx, rr.data() + m, nv - m, e->E1[0], e->E1[1]);
        e->c1 = e->c2 = 0;
        *out = e;
    });
}

int cozk_spliteq_free(cozk_spliteq* e) {
    if (!e) return COZK_OK;
    for (int k = 0; k < 2; k++) {
        if (e->E1[k]) ctx_dev_free(e->ctx, e->E1[k]);
        if (e->E2[k]) ctx_dev_free(e->ctx, e->E2[k]);
    }
    delete e;
    return COZK_OK;
}

int cozk_spliteq_lens(const cozk_spliteq* e, size_t* e1_len, size_t* e2_len) {
    if (!e) return COZK_ERR_INVALID_ARG;
    if (e1_len) *e1_len = e->E1_len;
    if (e2_len) *e2_len = e->E2_len;
    return COZK_OK;
}

// current tables -> host (tests): E1_len x 4 u64 and E2_len x 4 u64; either pointer may be null
int cozk_spliteq_download(cozk_ctx* ctx, const cozk_spliteq* e, uint64_t* e1, uint64_t* e2) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && e, "spliteq_download: bad argument");
        COZK_REQUIRE(e->ctx == ctx, "spliteq_download: the eq polynomial belongs to another context");
        if (e1) HIP_TRY(hipMemcpyAsync(e1, e->E1[e->c1], e->E1_len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        if (e2) HIP_TRY(hipMemcpyAsync(e2, e->E2[e->c2], e->E2_len * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    });
}

// SplitEqPolynomial::bind(r)
static bool spliteq_bound(const cozk_spliteq* e) { return e->E1_len == 1 && e->E2_len < 2; }
// one variable left: the next bind leaves the polynomial fully bound (the table lengths are powers of two)
static bool spliteq_last_bind(const cozk_spliteq* e) { return !spliteq_bound(e) && e->E1_len * e->E2_len == 2; }
// One bind, everything but the kernels, and the ONE place that does it: E1 folds until it is a single value, then E2; the folded
// table flips its ping-pong side and halves.  The launcher gets the fold, and, when E1 has just collapsed, the vector that its last
// value fold_out[0] multiplies from now on (E2).  The resident kernel does the same steps on the device; the host follows it with
// this function.  The caller has checked !spliteq_bound(e).
struct SpliteqStep {
    const fe* fold_in;
    fe* fold_out;
    size_t fold_n;
    fe* scale_vec;  // null unless E1 has just collapsed
    size_t scale_n;
};
static SpliteqStep spliteq_advance(cozk_spliteq* e) {
    SpliteqStep s{};
    if (e->E1_len == 1) {
        s.fold_in = e->E2[e->c2];
        s.fold_out = e->E2[1 - e->c2];
        s.fold_n = e->E2_len / 2;
        e->c2 = 1 - e->c2;
        e->E2_len = s.fold_n;
    } else {
        s.fold_in = e->E1[e->c1];
        s.fold_out = e->E1[1 - e->c1];
        s.fold_n = e->E1_len / 2;
        e->c1 = 1 - e->c1;
        e->E1_len = s.fold_n;
        if (s.fold_n == 1) {
            s.scale_vec = e->E2[e->c2];
            s.scale_n = e->E2_len;
        }
    }
    return s;
}
// the fold launches of one bind on ctx's stream (one, or two when E1 collapses)
static void spliteq_bind_launch(cozk_ctx* ctx, cozk_spliteq* e, const fe& rr) {
    const SpliteqStep s = spliteq_advance(e);
    k_fold_pairs<<<grid_for(s.fold_n), PT, 0, ctx->stream>>>(s.fold_in, s.fold_out, s.fold_n, rr);
    if (s.scale_n) k_scale_by_first<<<grid_for(s.scale_n), PT, 0, ctx->stream>>>(s.scale_vec, s.scale_n, s.fold_out);
    HIP_TRY(hipGetLastError());
}
int cozk_spliteq_bind(cozk_ctx* ctx, cozk_spliteq* e, const uint64_t r[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && e && r, "spliteq_bind: bad argument");
        COZK_REQUIRE(!spliteq_bound(e), "spliteq_bind: polynomial already fully bound");
        spliteq_bind_launch(ctx, e, fe_from_u64x4(r));
    });
}

// Which kernel a layer of `chunks` 4-element chunks takes, for the sums alone (layer_cubic_kernel) and for bind + sums in one pass
// (layer_bind_cubic_kernel).  F9: the 9 x 29 multiplier kernels (fr9.hip.hpp) for layers large enough to be throughput-bound;
// COZK_LAYER_F9=0: the saturated kernels everywhere.  NESTED: 0 the eq table is E2 alone, 1 E1 x E2, 2 E1 x E2 with the split-eq
// inner sums (layer9_terms) -- 9 x 29 plain kernels only, from E1_len / 2 >= LAYER_GROUPED_MIN_E1H (the Rep3 kernels lose with the
// three group accumulators: 0.58 vs 0.52 ms, register pressure); COZK_LAYER_GROUPED=0 switches it off.
struct LayerVariant {
    bool f9;
    int nested;
};
static LayerVariant layer_variant(const cozk_layer* l, const cozk_spliteq* e, size_t chunks) {
    static const bool f9_env = (getenv("COZK_LAYER_F9") ? atoi(getenv("COZK_LAYER_F9")) : 1) != 0;
    static const bool group_env = !(getenv("COZK_LAYER_GROUPED") && atoi(getenv("COZK_LAYER_GROUPED")) == 0);
    const bool f9 = f9_env && chunks >= LAYER_F9_MIN_CHUNKS, nested = e->E1_len != 1;
    const bool grouped = f9 && nested && group_env && l->mode == COZK_MODE_PLAIN && e->E1_len / 2 >= LAYER_GROUPED_MIN_E1H;
    return LayerVariant{f9, grouped ? 2 : (nested ? 1 : 0)};
}
using LayerCubicKernel = void (*)(const fe*, const fe*, size_t, const fe*, size_t, const fe*, size_t, fe*);
static LayerCubicKernel layer_cubic_kernel(int mode, LayerVariant v) {
    if (mode == COZK_MODE_REP3) {
        if (v.f9) return v.nested ? k_layer_cubic9<2, 1> : k_layer_cubic9<2, 0>;
        return v.nested ? k_layer_cubic<2, 1> : k_layer_cubic<2, 0>;
    }
    if (v.f9) return v.nested == 2 ? k_layer_cubic9<1, 2> : (v.nested ? k_layer_cubic9<1, 1> : k_layer_cubic9<1, 0>);
    return v.nested ? k_layer_cubic<1, 1> : k_layer_cubic<1, 0>;
}
using LayerBindCubicKernel = void (*)(const fe*, const fe*, fe*, fe*, size_t, fe, const fe*, size_t, const fe*, size_t, fe*);
static LayerBindCubicKernel layer_bind_cubic_kernel(int mode, LayerVariant v) {
    if (mode == COZK_MODE_REP3) {
        if (v.f9) return v.nested ? k_layer_bind_cubic9<2, 1> : k_layer_bind_cubic9<2, 0>;
        return v.nested ? k_layer_bind_cubic<2, 1> : k_layer_bind_cubic<2, 0>;
    }
    if (v.f9) return v.nested == 2 ? k_layer_bind_cubic9<1, 2> : (v.nested ? k_layer_bind_cubic9<1, 1> : k_layer_bind_cubic9<1, 0>);
    return v.nested ? k_layer_bind_cubic<1, 1> : k_layer_bind_cubic<1, 0>;
}
// workgroups of a layer round-sum launch over `chunks` chunks: the 9 x 29 kernels fill the chip exactly (resident_grid)
static unsigned layer_sum_grid(cozk_ctx* ctx, const void* kernel, bool f9, size_t chunks) {
    return sum_grid(f9 ? resident_grid(kernel, (chunks + PT - 1) / PT, ctx->device) : grid_capped(chunks, ROUND_GRID_MAX));
}

// Rep3BatchedCubicSumcheckWorker::compute_cubic (dense_interleaved_poly.rs:210-365): returns the 4
// additive coefficient shares of the round polynomial through evals [g0, claim - g0, g2, g3]
// The launch half of a large layer's round sums, on ctx's stream (the layer's own context, or the driver of a layer group): the
// kernel and its grid are chosen first (they depend on the mode, the length and the eq tables only, so the members of a group
// share them), the caller reserves gx block partials for each of the three rows, and the launch writes the rows at `partial`,
// `partial + gx`, `partial + 2 gx`.  The finish half is finish_sums over all the rows of the reservation.
struct LayerCubicPlan {
    LayerVariant v;
    LayerCubicKernel kernel;
    unsigned gx;
};
static LayerCubicPlan layer_cubic_plan(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq) {
    const size_t nch = (l->len + 3) / 4;
    const LayerVariant v = layer_variant(l, eq, nch);
    const LayerCubicKernel kernel = layer_cubic_kernel(l->mode, v);
    return LayerCubicPlan{v, kernel, layer_sum_grid(ctx, (const void*)kernel, v.f9, nch)};
}
static void layer_cubic_launch(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq, const LayerCubicPlan& p, fe* partial) {
    p.kernel<<<p.gx, PT, 0, ctx->stream>>>(l->buf[l->cur][0], l->buf[l->cur][1], l->len, eq->E1[eq->c1], p.v.nested ? eq->E1_len / 2 : 0, eq->E2[eq->c2],
                                           eq->E2_len, partial);
}
static void layer_cubic_sums(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq, fe s[3]) {
    const LayerCubicPlan p = layer_cubic_plan(ctx, l, eq);
    const SumLaunch sl = sum_launch(ctx, 3, p.gx, 3);
    layer_cubic_launch(ctx, l, eq, p, sl.partial);
    finish_sums(ctx, sl, 3, p.gx, Fr::one(), 0, s);
}

// The same two halves for bind + sums in one pass (eq tables already folded by the caller).  The launch makes the other ping-pong
// side hold the bound layer -- from the pool of the LAYER's context, whichever context drives the launch -- and moves the layer on.
struct LayerBindCubicPlan {
    LayerVariant v;
    LayerBindCubicKernel kernel;
    unsigned gx;
};
static LayerBindCubicPlan layer_bind_cubic_plan(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* e) {
    const size_t nout = 2 * ((l->len + 3) / 4), nch_out = (nout + 3) / 4;
    const LayerVariant v = layer_variant(l, e, nch_out);
    const LayerBindCubicKernel kernel = layer_bind_cubic_kernel(l->mode, v);
    return LayerBindCubicPlan{v, kernel, layer_sum_grid(ctx, (const void*)kernel, v.f9, nch_out)};
}
static void layer_bind_cubic_launch(cozk_ctx* ctx, cozk_layer* l, const cozk_spliteq* e, const LayerBindCubicPlan& p, const uint64_t r[4], fe* partial) {
    const LayerStep b = layer_advance(l);
    fe rr = fe_from_u64x4(r);
    if (p.v.f9)
        for (int d = 0; d < 5; d++) rr = Fr::dbl(rr);  // the 9 x 29 kernels take the challenge times 2^5 = 1 / lambda (fr9.hip.hpp)
    const bool rep3 = l->mode == COZK_MODE_REP3;
    {
        // algorithmic bytes: the layer read once and its bound half written once (SURVEY 8d K3 + K4 fused), + the eq tables
        const uint64_t S = rep3 ? 64 : 32;
        ProfScope prof(ctx, COZK_PROF_BIND_CUBIC, (uint64_t)b.len_in * S + (uint64_t)b.len_out * S + (uint64_t)(e->E1_len + e->E2_len) * 32);
        p.kernel<<<p.gx, PT, 0, ctx->stream>>>(b.ia, b.ib, b.oa, b.ob, b.len_in, rr, e->E1[e->c1], p.v.nested ? e->E1_len / 2 : 0, e->E2[e->c2], e->E2_len,
                                               partial);
    }
}

int cozk_layer_compute_cubic(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq, const uint64_t prev_claim[4],
                             uint64_t out_coeffs[16]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && eq && prev_claim && out_coeffs, "compute_cubic: bad argument");
        fe s[3];
        layer_cubic_sums(ctx, l, eq, s);
        cubic_coeffs_out(s, prev_claim, out_coeffs);
    });
}

// One round of prove_sumcheck (co-jolt/src/subprotocols/sumcheck.rs:107-122) per call: bind the layer and the
// split-eq polynomial with the previous round's challenge `r` (NULL in the first round), then compute_cubic.
// Layers of <= ROUND_SMALL_MAX elements take the single-launch kernel; larger ones the separate kernels.
int cozk_layer_round(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* e, const uint64_t* r, const uint64_t prev_claim[4],
                     uint64_t out_coeffs[16]) {
    if (!ctx || !l || !e || !prev_claim || !out_coeffs) return COZK_ERR_INVALID_ARG;
    if (l->len > ROUND_SMALL_MAX) {
        if (!r) return cozk_layer_compute_cubic(ctx, l, e, prev_claim, out_coeffs);
        // large layer: fold the eq tables, then bind and take the next round's sums in one pass (k_layer_bind_cubic)
        int rc = cozk_spliteq_bind(ctx, e, r);
        if (rc != COZK_OK) return rc;
        return cozk_guard(ctx, [&] {
            const LayerBindCubicPlan p = layer_bind_cubic_plan(ctx, l, e);
            const SumLaunch sl = sum_launch(ctx, 3, p.gx, 3);
            layer_bind_cubic_launch(ctx, l, e, p, r, sl.partial);
            fe sres[3];
            finish_sums(ctx, sl, 3, p.gx, Fr::one(), 0, sres);
            cubic_coeffs_out(sres, prev_claim, out_coeffs);
        });
    }
    return cozk_guard(ctx, [&] {
        // every refusal comes before the first change to the layer or the eq polynomial
        if (r) {
            COZK_REQUIRE(l->len >= 2, "layer_round: layer already fully bound");
            COZK_REQUIRE(!spliteq_bound(e), "layer_round: eq polynomial already fully bound");
        }
        LayerStep b{};
        SpliteqStep f{};
        fe rr = Fr::zero();
        if (r) {
            rr = fe_from_u64x4(r);
            b = layer_advance(l);
            f = spliteq_advance(e);
        }
        fe* res = result_slot(ctx, 3);
        auto* const kernel = l->mode == COZK_MODE_REP3 ? k_layer_round_small<2> : k_layer_round_small<1>;
        kernel<<<1, RT, 0, ctx->stream>>>(b.ia, b.ib, b.oa, b.ob, b.len_in, r != nullptr, rr, f.fold_in, f.fold_out, f.fold_n, f.scale_vec, f.scale_n,
                                          l->buf[l->cur][0], l->buf[l->cur][1], l->len, e->E1[e->c1], e->E1_len / 2, e->E2[e->c2], e->E2_len, e->E1_len != 1,
                                          res);
        HIP_TRY(hipGetLastError());
        fe sres[3];
        fetch_fe(ctx, res, 3, sres);
        cubic_coeffs_out(sres, prev_claim, out_coeffs);
    });
}

// The whole round loop of Rep3BatchedCubicSumcheckWorker::prove_sumcheck (co-jolt/src/subprotocols/sumcheck.rs:
// 96-131) for one layer: per round compute_cubic -> `cb` (the host sends the coefficients, receives the challenge
// and the next claim) -> bind, then final_claims.  While the layer is large each round is its own launch
// (cozk_layer_round); once it is down to ROUND_PERSIST_MAX elements the remaining rounds, the last bind and the
// final claims run inside ONE resident kernel that exchanges sums and challenges with this thread through a
// pinned mailbox (k_layer_rounds_persistent).  cb returns 0 on success; `next_claim` must already be this party's
// additive share.  out_r = num_rounds x 4; final_claims = left.a, left.b, right.a, right.b.
//
// The host tail.  Once the layer is at most host_tail_max() elements long, the remaining rounds, the last bind and the final claims
// run on this thread (layer_tail_rounds, host/layer_tail.hpp) on a copy of the layer and the live eq tables in the mailbox's tail
// area: the resident kernel is asked for only as many rounds as it takes to get there and publishes the bound tail in its last
// stage; a layer that no resident kernel holds is gathered by one launch (k_layer_tail_out).  Afterwards the layer and the eq
// polynomial are left as the device rounds leave them: sides and lengths through layer_advance / spliteq_advance, the values by
// one small launch (k_layer_tail_back).
// COZK_HOST_TAIL_MAX=n, read on every call: the longest layer the host takes over, for calls that may use the resident kernel and
// for calls that may not alike (0: no host tail; capped at HOST_TAIL_CAP).  The defaults are measured ("Host tails"): a
// resident round costs ~19 us and a launched one ~38 us whatever the length, a host round the callback and its field products.
extern "C++" {
static constexpr size_t HOST_TAIL_RESIDENT = 256, HOST_TAIL_LAUNCHED = 512;
static size_t host_tail_max(bool resident) {
    const char* s = getenv("COZK_HOST_TAIL_MAX");
    const long n = s ? atol(s) : (long)(resident ? HOST_TAIL_RESIDENT : HOST_TAIL_LAUNCHED);
    return n <= 0 ? 0 : ((size_t)n > HOST_TAIL_CAP ? HOST_TAIL_CAP : (size_t)n);
}
static RoundMailbox* ctx_mailbox(cozk_ctx* ctx) {
    if (!ctx->mailbox) HIP_TRY(hipHostMalloc(&ctx->mailbox, sizeof(RoundMailbox), hipHostMallocMapped | hipHostMallocCoherent));
    return (RoundMailbox*)ctx->mailbox;
}
// binds the eq polynomial can still take (its tables are powers of two long)
static int spliteq_binds_left(size_t E1_len, size_t E2_len) {
    int n = 0;
    for (size_t v = E1_len; v > 1; v >>= 1) n++;
    for (size_t v = E2_len; v > 1; v >>= 1) n++;
    return n;
}
// may the host take over a layer of this shape with `binds` binds to go?  (A call that would bind an exhausted eq polynomial is
// refused by the device path's own checks: it stays there.)
static bool host_tail_takes(LayerTailShape s, int nc, size_t tail_max, int binds) {
    return s.len >= 2 && s.len <= tail_max && layer_tail_entries(nc, s.len, s.E1_len, s.E2_len) <= HOST_TAIL_AREA &&
           spliteq_binds_left(s.E1_len, s.E2_len) >= binds;
}
// The rounds `round` .. num_rounds - 1 of the call on the tail in `area` (the layer and the eq polynomial stand at its shape), and
// the state they leave behind.
template <int NC>
static void layer_host_tail(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* e, fe* area, bool have_r, uint64_t rr[4], uint64_t pc[4], int round, int num_rounds,
                            cozk_round_cb cb, void* user, uint64_t* out_r, uint64_t final_claims[16]) {
    using clk = std::chrono::steady_clock;
    const bool trace = trace_rounds();
    LayerTailView t = layer_tail_view(area, NC, l->len, e->E1_len, e->E2_len);
    double us_cb = 0;
    const clk::time_point t_start = trace ? clk::now() : clk::time_point();
    fe fin[4];
    const int binds = layer_tail_rounds<NC>(
        t, have_r, have_r ? fe_from_u64x4(rr) : Fr::zero(), num_rounds - round,
        [&](int j, const fe s[3]) {
            uint64_t coeffs[16], nc[4];
            cubic_coeffs_out(s, pc, coeffs);
            const clk::time_point t0 = trace ? clk::now() : clk::time_point();
            if (cb(user, round + j, coeffs, rr, nc) != 0) throw CozkError(COZK_ERR_INTERNAL, "layer_prove_rounds: round callback failed");
            if (trace) us_cb += std::chrono::duration<double, std::micro>(clk::now() - t0).count();
            memcpy(out_r + 4 * (round + j), rr, 4 * sizeof(uint64_t));
            memcpy(pc, nc, 4 * sizeof(uint64_t));
            return fe_from_u64x4(rr);
        },
        fin);
    COZK_REQUIRE(t.len == 2, "final_claims: layer must be fully bound (len == 2)");
    for (int k = 0; k < 4; k++) fe_to_u64x4(fin[k], final_claims + 4 * k);
    if (trace && num_rounds > round) {
        const double us = std::chrono::duration<double, std::micro>(clk::now() - t_start).count();
        fprintf(stderr, "[host tail] %d rounds from %zu elements: host us/round: callback %.1f compute %.1f\n", num_rounds - round, (size_t)l->len,
                us_cb / (num_rounds - round), (us - us_cb) / (num_rounds - round));
    }
    // the device state: sides and lengths as the launchers move them, then the values
    for (int b = 0; b < binds; b++) {
        (void)layer_advance(l);
        (void)spliteq_advance(e);
    }
    COZK_REQUIRE(l->len == t.len && e->E1_len == t.E1_len && e->E2_len == t.E2_len, "layer_prove_rounds: host tail out of step with the layer");
    if (!binds) return;
    const size_t nback = layer_tail_entries(NC, t.len, t.E1_len, t.E2_len);
    if (nback <= (size_t)TAIL_BACK_MAX) {
        TailBackArgs a{};
        int n = 0;
        auto put = [&](fe* dst, const fe* src, size_t cnt) {
            for (size_t i = 0; i < cnt; i++, n++) {
                a.v[n] = src[i];
                a.dst[n] = dst + i;
            }
        };
        put(l->buf[l->cur][0], t.la, t.len);
        if (NC == 2) put(l->buf[l->cur][1], t.lb, t.len);
        put(e->E1[e->c1], t.E1, t.E1_len);
        put(e->E2[e->c2], t.E2, t.E2_len);
        k_layer_tail_back<<<1, 64, 0, ctx->stream>>>(a, n);
        HIP_TRY(hipGetLastError());
    } else {  // an eq polynomial of more variables than the layer binds: copies from the tail area, which the next call reuses
        HIP_TRY(hipMemcpyAsync(l->buf[l->cur][0], t.la, t.len * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        if (NC == 2) HIP_TRY(hipMemcpyAsync(l->buf[l->cur][1], t.lb, t.len * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(e->E1[e->c1], t.E1, t.E1_len * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        if (t.E2_len) HIP_TRY(hipMemcpyAsync(e->E2[e->c2], t.E2, t.E2_len * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
}
// the same for a layer that is on the device alone: one launch gathers it into the tail area, one drain
static void layer_host_tail_gathered(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* e, bool have_r, uint64_t rr[4], uint64_t pc[4], int round, int num_rounds,
                                     cozk_round_cb cb, void* user, uint64_t* out_r, uint64_t final_claims[16]) {
    RoundMailbox* mb = ctx_mailbox(ctx);
    const bool rep3 = l->mode == COZK_MODE_REP3;
    auto* const kernel = rep3 ? k_layer_tail_out<2> : k_layer_tail_out<1>;
    kernel<<<1, RT, 0, ctx->stream>>>(l->buf[l->cur][0], l->buf[l->cur][1], l->len, e->E1[e->c1], e->E1_len, e->E2[e->c2], e->E2_len, mb->tail);
    HIP_TRY(hipGetLastError());
    stream_drain_by_flag(ctx);
    std::atomic_thread_fence(std::memory_order_acquire);
    if (rep3) layer_host_tail<2>(ctx, l, e, mb->tail, have_r, rr, pc, round, num_rounds, cb, user, out_r, final_claims);
    else layer_host_tail<1>(ctx, l, e, mb->tail, have_r, rr, pc, round, num_rounds, cb, user, out_r, final_claims);
}
}  // extern "C++"

int cozk_layer_prove_rounds(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* e, const uint64_t claim[4], int num_rounds, cozk_round_cb cb,
                            void* user, uint64_t* out_r, uint64_t final_claims[16]) {
    if (!ctx || !l || !e || !claim || !cb || !final_claims || num_rounds < 0 || (num_rounds > 0 && !out_r)) return COZK_ERR_INVALID_ARG;
    // What the rounds, the last bind and the final claims below would refuse half-way, asked before the first round: a refused call
    // leaves the layer and the eq polynomial as they were, and the callback is not called.  The call binds num_rounds times.
    int rc0 = cozk_guard(ctx, [&] {
        COZK_REQUIRE(spliteq_binds_left(e->E1_len, e->E2_len) >= num_rounds, "layer_prove_rounds: the eq polynomial has fewer unbound variables than the call has rounds");
        size_t len = l->len;
        for (int j = 0; j < num_rounds && len > 2; j++) len = 2 * ((len + 3) / 4);  // as layer_advance
        COZK_REQUIRE(l->len >= 2 && len == 2, "layer_prove_rounds: num_rounds binds must leave the layer fully bound (len == 2)");
    });
    if (rc0 != COZK_OK) return rc0;
    static const bool no_persist = getenv("COZK_NO_PERSIST") != nullptr;  // set to anything: every round is its own launch
    uint64_t pc[4], rr[4], coeffs[16], nc[4];
    memcpy(pc, claim, sizeof pc);
    bool have_r = false;
    int round = 0;
    const int nc_layer = l->mode == COZK_MODE_REP3 ? 2 : 1;
    // the resident kernel is used when the context allows it (cozk_ctx_set_resident_rounds; by default only while this
    // is the one live context on its device in the process) and is abandoned for the rest of the call once its watchdog
    // has fired (a round callback that took longer than COZK_RESIDENT_TIMEOUT_S): the loop then goes on with one launch
    // per round, from exactly the state the kernel left
    bool allow_resident = !no_persist && ctx_resident_rounds_enabled(ctx);
    for (;;) {
        bool host_tail = false;
        for (; round < num_rounds; round++) {
            host_tail = host_tail_takes(LayerTailShape{l->len, e->E1_len, e->E2_len}, nc_layer, host_tail_max(allow_resident),
                                        num_rounds - round + (have_r ? 1 : 0));
            if (host_tail) break;
            if (allow_resident && l->len <= ROUND_PERSIST_MAX && l->len >= 2) break;
            int rc = cozk_layer_round(ctx, l, e, have_r ? rr : nullptr, pc, coeffs);
            if (rc != COZK_OK) return rc;
            if (cb(user, round, coeffs, rr, nc) != 0) {
                ctx->last_error = "layer_prove_rounds: round callback failed";
                return COZK_ERR_INTERNAL;
            }
            memcpy(out_r + 4 * round, rr, sizeof rr);
            memcpy(pc, nc, sizeof pc);
            have_r = true;
        }
        if (round == num_rounds) {  // every remaining round ran as its own launch
            if (have_r) {
                int rc = cozk_layer_bind(ctx, l, rr);
                if (rc != COZK_OK) return rc;
                rc = cozk_spliteq_bind(ctx, e, rr);
                if (rc != COZK_OK) return rc;
            }
            return cozk_layer_final_claims(ctx, l, final_claims);
        }
        if (host_tail)  // the layer is short enough already: no resident kernel in between
            return cozk_guard(ctx, [&] { layer_host_tail_gathered(ctx, l, e, have_r, rr, pc, round, num_rounds, cb, user, out_r, final_claims); });
        int rounds_done = -1;  // >= 0: the resident kernel timed out after that many of its rounds; fall back
        int rc = cozk_guard(ctx, [&] {
            const int nrem = num_rounds - round;
            // both ping-pong buffers of the layer must hold the current length
            pingpong_ensure(l, 1 - l->cur, l->len);
            RoundMailbox* mb = ctx_mailbox(ctx);
            memset(mb, 0, offsetof(RoundMailbox, tail));
            std::atomic_thread_fence(std::memory_order_seq_cst);
            const int bind_first = have_r ? 1 : 0;
            // rounds the kernel keeps: all of them, or, with a host tail, as many as it takes until the layer it has bound is short
            // enough (at least one: a layer that is short enough before its first round never gets here)
            int nker = nrem;
            {
                const size_t tail_max = host_tail_max(true);
                LayerTailShape sh{l->len, e->E1_len, e->E2_len};
                if (bind_first) sh = layer_tail_shape_bound(sh);
                for (int k = 1; k < nrem && tail_max; k++) {
                    sh = layer_tail_shape_bound(sh);
                    if (host_tail_takes(sh, nc_layer, tail_max, nrem - k)) {
                        nker = k;
                        break;
                    }
                }
            }
            const bool tail_out = nker < nrem;
            fe r_first = have_r ? fe_from_u64x4(rr) : Fr::zero();
            const long long ticks = (long long)resident_timeout_s() * MB_TICKS_PER_S;
            const bool rep3 = l->mode == COZK_MODE_REP3;
            auto* const kernel = rep3 ? (trace_rounds() ? k_layer_rounds_persistent<2, 1> : k_layer_rounds_persistent<2, 0>)
                                      : (trace_rounds() ? k_layer_rounds_persistent<1, 1> : k_layer_rounds_persistent<1, 0>);
            kernel<<<1, RT, 0, ctx->stream>>>(l->buf[0][0], l->buf[0][1], l->buf[1][0], l->buf[1][1], l->cur, l->len, e->E1[0], e->E1[1], e->c1, e->E1_len,
                                              e->E2[0], e->E2[1], e->c2, e->E2_len, nker, bind_first, r_first, mb, ticks, tail_out ? 1 : 0);
            HIP_TRY(hipGetLastError());
            volatile uint32_t* res_seq = &mb->res_seq;
            volatile uint32_t* status = &mb->status;
            auto give_up = [&](const char* why) {
                *(volatile uint32_t*)&mb->cmd[12] = 1;
                std::atomic_thread_fence(std::memory_order_seq_cst);
                (void)hipStreamSynchronize(ctx->stream);
                throw CozkError(COZK_ERR_INTERNAL, why);
            };
            // false: the kernel's watchdog fired (it waited resident_timeout_s() for the host's challenge and left)
            auto wait_result = [&](uint32_t want) -> bool {
                auto t0 = std::chrono::steady_clock::now();
                uint64_t spins = 0;
                while (*res_seq != want) {
                    if (*status == 1) return false;
                    if (*status) give_up("layer_prove_rounds: the resident kernel stopped");
                    __builtin_ia32_pause();
                    if ((++spins & 0xfffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(resident_timeout_s() + 5))
                        give_up("layer_prove_rounds: no result from the resident kernel");
                }
                std::atomic_thread_fence(std::memory_order_acquire);
                return true;
            };
            // mirror the kernel's bookkeeping: one bind per completed round (+ the pending one it started with), by the steps the
            // launchers take (both ping-pong sides hold the layer already, so nothing is allocated)
            auto mirror_binds = [&](int binds) {
                for (int b = 0; b < binds; b++) {
                    (void)layer_advance(l);
                    (void)spliteq_advance(e);
                }
            };
            int j = 0;
            bool alive = true;
            for (; j < nker; j++) {
                if (!(alive = wait_result((uint32_t)j + 1))) break;
                const fe sres[3] = {mb->res[0], mb->res[1], mb->res[2]};
                cubic_coeffs_out(sres, pc, coeffs);
                if (cb(user, round + j, coeffs, rr, nc) != 0) give_up("layer_prove_rounds: round callback failed");
                memcpy(out_r + 4 * (round + j), rr, sizeof rr);
                memcpy(pc, nc, sizeof pc);
                have_r = true;
                {
                    // three self-validating pieces: payload first, then the half that carries the tag (x86 stores stay in order)
                    const fe rv = fe_from_u64x4(rr);
                    const uint32_t tag = (uint32_t)j + 1;
                    const uint32_t pay[9] = {rv.l[0], rv.l[1], rv.l[2], rv.l[3], rv.l[4], rv.l[5], rv.l[6], rv.l[7], 0u};
                    for (int k = 0; k < 3; k++) {
                        volatile uint64_t* piece = reinterpret_cast<volatile uint64_t*>(&mb->cmd[4 * k]);
                        piece[0] = (uint64_t)pay[3 * k] | ((uint64_t)pay[3 * k + 1] << 32);
                        std::atomic_thread_fence(std::memory_order_release);
                        piece[1] = (uint64_t)pay[3 * k + 2] | ((uint64_t)tag << 32);
                    }
                }
            }
            if (alive) alive = wait_result((uint32_t)nker + 1);
            if (!alive) {
                // the kernel left while the host was inside the callback of round j - 1 (or before the first result):
                // it published j results and bound j - 1 (+ bind_first) times; the challenge of round j - 1 is pending
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                mirror_binds(j > 0 ? j - 1 + bind_first : 0);
                rounds_done = j;
                return;
            }
            if (trace_rounds())
                fprintf(stderr, "[mailbox] %d rounds: device us/round: wait %.1f bind %.1f cubic %.1f publish %.1f\n", nker,
                        mb->dbg[0] / 100.0 / (nker + 1), mb->dbg[1] / 100.0 / (nker + 1), mb->dbg[2] / 100.0 / nker, mb->dbg[3] / 100.0 / nker);
            mirror_binds(nker + bind_first);
            if (!tail_out) {
                for (int k = 0; k < 4; k++) fe_to_u64x4(mb->res[k], final_claims + 4 * k);
                return;
            }
            // the kernel has left the bound tail in the mailbox: the remaining rounds run here
            COZK_REQUIRE(mb->tail_n[0] == l->len && mb->tail_n[1] == e->E1_len && mb->tail_n[2] == e->E2_len,
                         "layer_prove_rounds: the resident kernel handed over another tail than expected");
            if (rep3) layer_host_tail<2>(ctx, l, e, mb->tail, false, rr, pc, round + nker, num_rounds, cb, user, out_r, final_claims);
            else layer_host_tail<1>(ctx, l, e, mb->tail, false, rr, pc, round + nker, num_rounds, cb, user, out_r, final_claims);
        });
        if (rc != COZK_OK || rounds_done < 0) return rc;
        round += rounds_done;
        allow_resident = false;
    }
}

// cozk_layer_prove_rounds for a worker sub-net, which cannot derive g(1) from the (global) previous claim and sends
// the raw sums g(0), g(2), g(3) instead (as cozk_layer_compute_cubic_evals).  Same machinery: the round polynomial
// through (g0, -g0, g2, g3) -- i.e. previous claim 0 -- is evaluated back at 0, 2, 3 for the callback.
namespace {
struct EvalsShim {
    cozk_round_evals_cb cb;
    void* user;
};
int evals_shim_cb(void* user, int round, const uint64_t coeffs[16], uint64_t r_out[4], uint64_t next_claim_out[4]) {
    EvalsShim* sh = static_cast<EvalsShim*>(user);
    std::vector<fe> cf(4);
    for (int i = 0; i < 4; i++) cf[i] = fe_from_u64x4(coeffs + 4 * i);
    uint64_t ev[12];
    fe_to_u64x4(cf[0], ev);
    auto horner = [&](const fe& x) { return Fr::add(cf[0], Fr::mul(x, Fr::add(cf[1], Fr::mul(x, Fr::add(cf[2], Fr::mul(x, cf[3])))))); };
    fe_to_u64x4(horner(Fr::from_u64(2)), ev + 4);
    fe_to_u64x4(horner(Fr::from_u64(3)), ev + 8);
    for (int i = 0; i < 4; i++) next_claim_out[i] = 0;
    return sh->cb(sh->user, round, ev, r_out);
}
}  // namespace
int cozk_layer_prove_rounds_evals(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* e, int num_rounds, cozk_round_evals_cb cb, void* user,
                                  uint64_t* out_r, uint64_t final_claims[16]) {
    if (!cb) return COZK_ERR_INVALID_ARG;
    EvalsShim sh{cb, user};
    const uint64_t zero[4] = {0, 0, 0, 0};
    return cozk_layer_prove_rounds(ctx, l, e, zero, num_rounds, evals_shim_cb, &sh, out_r, final_claims);
}

// the raw additive sums g(0), g(2), g(3) of compute_cubic, for a worker sub-net that cannot derive g(1) from
// the (global) previous claim: the coordinator inserts claim - g(0), as the reference does for the primary
// sumcheck (jolt/vm/instruction_lookups/worker.rs:593-597, coordinator.rs:131-132)
int cozk_layer_compute_cubic_evals(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq, uint64_t out_evals[12]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && eq && out_evals, "compute_cubic_evals: bad argument");
        fe s[3];
        layer_cubic_sums(ctx, l, eq, s);
        for (int i = 0; i < 3; i++) fe_to_u64x4(s[i], out_evals + 4 * i);
    });
}

// final_claims (dense_interleaved_poly.rs:367-372): coeffs[0], coeffs[1]; out = L.a, L.b, R.a, R.b
int cozk_layer_final_claims(cozk_ctx* ctx, const cozk_layer* l, uint64_t out[16]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && out && l->len == 2, "final_claims: layer must be fully bound (len == 2)");
        fe h[2];
        fetch_fe(ctx, l->buf[l->cur][0], 2, h);
        fe_to_u64x4(h[0], out);
        fe_to_u64x4(h[1], out + 8);
        if (l->mode == COZK_MODE_REP3) {
            fetch_fe(ctx, l->buf[l->cur][1], 2, h);
            fe_to_u64x4(h[0], out + 4);
            fe_to_u64x4(h[1], out + 12);
        } else {
            for (int i = 0; i < 4; i++) out[4 + i] = out[12 + i] = 0;
        }
    });
}

// ------------------------------------------------------------------ C ABI: layer groups
// k layers of one mode and one length that share the public eq polynomial, the challenge and the claim, driven as one unit of work
// on the DRIVER's stream: one sumcheck round of all of them is 2 to 3 launches and one fetch instead of k launches and k fetches.
// The members stay their owners' (their buffers come from and return to their own contexts' pools); the group only refers to them.
struct cozk_layer_group {
    cozk_ctx* driver;
    int mode;
    std::vector<cozk_layer*> m;
};

// the one current length of members 0..k - 1
static size_t layer_group_len(const cozk_layer_group* g, size_t k, const char* what) {
    for (size_t i = 1; i < k; i++) COZK_REQUIRE(g->m[i]->len == g->m[0]->len, std::string(what) + ": the members must have one length");
    return k ? g->m[0]->len : 0;
}

int cozk_layer_group_create(cozk_ctx* driver, cozk_layer* const* layers, int k, cozk_layer_group** out) {
    if (out) *out = nullptr;
    return cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && layers && out, "layer_group_create: null argument");
        COZK_REQUIRE(k >= 1 && k <= COZK_LAYER_GROUP_MAX, "layer_group_create: 1 <= k <= COZK_LAYER_GROUP_MAX");
        std::vector<cozk_ctx*> owners;
        for (int i = 0; i < k; i++) {
            const cozk_layer* l = layers[i];
            group_member_check<false>("layer_group_create", MEMBER, driver, layers, i);
            COZK_REQUIRE(l->mode == layers[0]->mode, "layer_group_create: the members must have one mode");
            COZK_REQUIRE(l->len == layers[0]->len && l->len >= 2, "layer_group_create: the members must have one length >= 2");
            owners.push_back(l->ctx);
        }
        drain_streams(owners);
        for (int i = 0; i < k; i++) {  // the other ping-pong side, once: later rounds allocate nothing
            cozk_layer* l = layers[i];
            pingpong_ensure(l, 1 - l->cur, 2 * ((l->len + 3) / 4));
        }
        cozk_layer_group* g = new cozk_layer_group();
        g->driver = driver;
        g->mode = layers[0]->mode;
        g->m.assign(layers, layers + k);
        *out = g;
    });
}

int cozk_layer_group_free(cozk_layer_group* g) {
    delete g;
    return COZK_OK;
}

// the pointer tables of one launch over members 0 .. k - 1; bind: every member moves on to its other ping-pong side (layer_advance)
static LayerGroupArgs layer_group_args(const cozk_layer_group* g, size_t k, bool bind) {
    LayerGroupArgs a;
    memset(&a, 0, sizeof a);
    for (size_t m = 0; m < k; m++) {
        cozk_layer* l = g->m[m];
        if (bind) {
            const LayerStep b = layer_advance(l);
            a.ia[m] = b.ia;
            a.ib[m] = b.ib;
            a.oa[m] = b.oa;
            a.ob[m] = b.ob;
        } else {
            a.ia[m] = l->buf[l->cur][0];
            a.ib[m] = l->buf[l->cur][1];
        }
    }
    return a;
}

int cozk_layer_group_round(cozk_layer_group* g, cozk_spliteq* e, const uint64_t* r, const uint64_t prev_claim[4], uint64_t* out_coeffs) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(e && prev_claim && out_coeffs, "layer_group_round: null argument");
        COZK_REQUIRE(e->ctx == ctx, "layer_group_round: the eq polynomial must be the driver's");
        const unsigned k = (unsigned)g->m.size();
        const size_t len = layer_group_len(g, k, "layer_group_round");
        if (r) {
            COZK_REQUIRE(len > 2, "layer_group_round: the members are already fully bound");
            COZK_REQUIRE(!spliteq_bound(e), "layer_group_round: eq polynomial already fully bound");
        }
        const bool rep3 = g->mode == COZK_MODE_REP3;
        fe s[3 * COZK_LAYER_GROUP_MAX];
        if (len > ROUND_SMALL_MAX) {
            // large members: the launches of cozk_layer_round back to back, member m on its own three rows of ONE reservation
            // (all take the same grid: one length, one mode, one eq), ONE finishing kernel over the 3 k rows and ONE fetch
            if (!r) {
                const LayerCubicPlan p = layer_cubic_plan(ctx, g->m[0], e);
                const SumLaunch sl = sum_launch(ctx, 3 * k, p.gx, 3 * k);
                for (unsigned m = 0; m < k; m++) layer_cubic_launch(ctx, g->m[m], e, p, sl.partial + (size_t)3 * m * p.gx);
                finish_sums(ctx, sl, 3 * k, p.gx, Fr::one(), 0, s);
            } else {
                spliteq_bind_launch(ctx, e, fe_from_u64x4(r));
                const LayerBindCubicPlan p = layer_bind_cubic_plan(ctx, g->m[0], e);
                const SumLaunch sl = sum_launch(ctx, 3 * k, p.gx, 3 * k);
                for (unsigned m = 0; m < k; m++) layer_bind_cubic_launch(ctx, g->m[m], e, p, r, sl.partial + (size_t)3 * m * p.gx);
                finish_sums(ctx, sl, 3 * k, p.gx, Fr::one(), 0, s);
            }
        } else {
            const LayerGroupArgs a = layer_group_args(g, k, r != nullptr);
            fe rr = Fr::zero();
            if (r) {
                rr = fe_from_u64x4(r);
                spliteq_bind_launch(ctx, e, rr);  // once for all members, in front of their launch on the same stream
            }
            const size_t len_now = g->m[0]->len;
            const int nested = e->E1_len != 1;
            fe* res = result_slot(ctx, (size_t)3 * k);
            auto* const kernel = rep3 ? k_layer_group_round_small<2> : k_layer_group_round_small<1>;
            kernel<<<k, RT, 0, ctx->stream>>>(a, len, r != nullptr, rr, len_now, e->E1[e->c1], e->E1_len / 2, e->E2[e->c2], e->E2_len, nested, res);
            HIP_TRY(hipGetLastError());
            fetch_fe(ctx, res, (size_t)3 * k, s);
        }
        for (unsigned m = 0; m < k; m++) cubic_coeffs_out(s + 3 * m, prev_claim, out_coeffs + 16 * m);
    });
}

int cozk_layer_group_final(cozk_layer_group* g, cozk_spliteq* e, const uint64_t* r, int k_final, uint64_t* out_claims) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(e && out_claims, "layer_group_final: null argument");
        COZK_REQUIRE(e->ctx == ctx, "layer_group_final: the eq polynomial must be the driver's");
        COZK_REQUIRE(k_final >= 0 && k_final <= (int)g->m.size(), "layer_group_final: 0 <= k_final <= k");
        const size_t len = layer_group_len(g, (size_t)k_final, "layer_group_final");
        COZK_REQUIRE(k_final == 0 || (r ? len <= 4 : len == 2), "layer_group_final: the members must be fully bound (len == 2) after the bind");
        if (r) COZK_REQUIRE(!spliteq_bound(e), "layer_group_final: eq polynomial already fully bound");
        const bool rep3 = g->mode == COZK_MODE_REP3;
        const int nc = rep3 ? 2 : 1;
        const LayerGroupArgs a = layer_group_args(g, (size_t)k_final, r != nullptr);  // len <= 4 binds to 2 elements
        fe rr = Fr::zero();
        if (r) {
            rr = fe_from_u64x4(r);
            spliteq_bind_launch(ctx, e, rr);  // as cozk_layer_prove_rounds does behind its last round
        }
        if (k_final == 0) {
            if (r) stream_drain_by_flag(ctx);
            return;
        }
        const size_t n_res = (size_t)2 * nc * (size_t)k_final;
        fe* res = result_slot(ctx, n_res);
        auto* const kernel = rep3 ? k_layer_group_final<2> : k_layer_group_final<1>;
        kernel<<<k_final, GFT, 0, ctx->stream>>>(a, len, r != nullptr, rr, res);
        HIP_TRY(hipGetLastError());
        fe h[4 * COZK_LAYER_GROUP_MAX];
        fetch_fe(ctx, res, n_res, h);
        for (int m = 0; m < k_final; m++) {  // the layout of cozk_layer_final_claims: L.a, L.b, R.a, R.b (b = 0 for PLAIN)
            uint64_t* out = out_claims + 16 * m;
            for (int i = 0; i < 16; i++) out[i] = 0;
            for (int side = 0; side < 2; side++)
                for (int c = 0; c < nc; c++) fe_to_u64x4(h[(2 * m + side) * nc + c], out + 8 * side + 4 * c);
        }
    });
}

// local half of layer_output / mul_vec: out[j] = L[j] x R[j] + mask_j (additive share c.a);
// masked = 0 for the plain prover (then out IS the next layer).  The ring reshare that turns c.a
// into (c.a, c.b = prev's c.a) is the network seam (cozk_layer_create on the two buffers).
int cozk_layer_output_local(cozk_ctx* ctx, const cozk_layer* l, int masked, const uint8_t* key_self_b, const uint8_t* key_prev_b,
                            uint64_t counter, cozk_vec** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && out && l->len >= 2 && (!masked || (key_self_b && key_prev_b)), "layer_output_local: bad argument");
        prf_key seed_self{}, seed_prev{};
        if (masked) {
            seed_self = prf_key_from_bytes(key_self_b);
            seed_prev = prf_key_from_bytes(key_prev_b);
        }
        size_t n = (l->len + 1) / 2;
        fe* d = dev_alloc_fe(n);
        const fe* a = l->buf[l->cur][0];
        const fe* b = l->buf[l->cur][1];
        {
            // algorithmic bytes: 2 n shares read, n additive shares written (192 n for Rep3)
            ProfScope prof(ctx, COZK_PROF_LAYER_OUTPUT, (uint64_t)l->len * (l->mode == COZK_MODE_REP3 ? 64 : 32) + (uint64_t)n * 32);
            if (l->mode == COZK_MODE_REP3) k_layer_output<2><<<grid_for(n), PT, 0, ctx->stream>>>(a, b, l->len, d, n, masked, seed_self, seed_prev, counter);
            else k_layer_output<1><<<grid_for(n), PT, 0, ctx->stream>>>(a, b, l->len, d, n, masked, seed_self, seed_prev, counter);
        }
        HIP_TRY(hipGetLastError());
        *out = new cozk_vec{ctx, n, COZK_SCALAR_FR, d, n * sizeof(fe), true};
    });
}

// rep3::arithmetic::mul_vec local half on two share vectors (x, y given as SoA component vectors)
int cozk_rep3_mul_vec_local(cozk_ctx* ctx, int mode, const cozk_vec* xa, const cozk_vec* xb, const cozk_vec* ya,
                            const cozk_vec* yb, int masked, const uint8_t* key_self_b, const uint8_t* key_prev_b, uint64_t counter,
                            cozk_vec** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && xa && ya && out && xa->n == ya->n && (mode == COZK_MODE_PLAIN || (xb && yb && xb->n == xa->n && yb->n == xa->n)) &&
                         (!masked || (key_self_b && key_prev_b)),
                     "mul_vec_local: bad argument");
        // the kernel reads xa->n field elements from each: a narrow vector of that many entries is shorter than that
        COZK_REQUIRE(xa->kind == COZK_SCALAR_FR && ya->kind == COZK_SCALAR_FR &&
                         (mode == COZK_MODE_PLAIN || (xb->kind == COZK_SCALAR_FR && yb->kind == COZK_SCALAR_FR)),
                     "mul_vec_local: the share components must be FR vectors");
        prf_key seed_self{}, seed_prev{};
        if (masked) {
            seed_self = prf_key_from_bytes(key_self_b);
            seed_prev = prf_key_from_bytes(key_prev_b);
        }
        size_t n = xa->n;
        fe* d = dev_alloc_fe(n);
        if (mode == COZK_MODE_REP3)
            k_mul_vec_local<2><<<grid_for(n), PT, 0, ctx->stream>>>((const fe*)xa->d, (const fe*)xb->d, (const fe*)ya->d, (const fe*)yb->d, n, d, masked, seed_self, seed_prev, counter);
        else
            k_mul_vec_local<1><<<grid_for(n), PT, 0, ctx->stream>>>((const fe*)xa->d, nullptr, (const fe*)ya->d, nullptr, n, d, masked, seed_self, seed_prev, counter);
        HIP_TRY(hipGetLastError());
        *out = new cozk_vec{ctx, n, COZK_SCALAR_FR, d, n * sizeof(fe), true};
    });
}

// claimed_outputs (grand_product.rs:266-272): last layer chunks(2) -> L x R, additive; out: n/2 x 4 u64
int cozk_layer_claimed_outputs(cozk_ctx* ctx, const cozk_layer* l, uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && l && out && l->len >= 2 && l->len % 2 == 0, "claimed_outputs: bad argument");
        size_t n = l->len / 2;
        ctx->scratch.reserve(n * sizeof(fe));
        fe* d = ctx->scratch.as<fe>();
        const fe* a = l->buf[l->cur][0];
        const fe* b = l->buf[l->cur][1];
        if (l->mode == COZK_MODE_REP3) k_layer_output<2><<<grid_for(n), PT, 0, ctx->stream>>>(a, b, l->len, d, n, 0, prf_key{}, prf_key{}, 0);
        else k_layer_output<1><<<grid_for(n), PT, 0, ctx->stream>>>(a, b, l->len, d, n, 0, prf_key{}, prf_key{}, 0);
        HIP_TRY(hipGetLastError());
        std::vector<fe> h(n);
        fetch_fe(ctx, d, n, h.data());
        for (size_t i = 0; i < n; i++) fe_to_u64x4(h[i], out + 4 * i);
    });
}

}  // extern "C"

#include "toggle_layer.inc"
#include "spartan_group.inc"
#include "sparse_layer.inc"
#include "primary_sumcheck.inc"
#include "primary_group.inc"
#include "spartan_outer.inc"
#include "outer_group.inc"
#include "spartan_inner.inc"
#include "logup.inc"
#include "compact_open.inc"
#include "output_check.inc"
