// Shamir secret sharing on the device: deal a vector to n parties, open vectors and commitments with Lagrange coefficients
// (mpc-types/src/protocols/shamir.rs).  A ShamirPrimeFieldShare is repr(transparent) over F (shamir/arithmetic/types.rs:
// 10-30), so a party's share vector is a plain FR cozk_vec and the local operators are the existing element-wise kernels.
#include "poly.hip.hpp"
#include "prf.hip.hpp"
#include "shamir_deal.hip.hpp"

#include <string.h>

#include <vector>

// ------------------------------------------------------------------ share / eval: all parties in one pass
// shares[p][i] = f_i(p + 1), f_i(x) = v[i] + sum_{c = 1..degree} coef_c[i] x^c (shamir.rs:190-207 `share`, :166-175
// `evaluate_poly`).  A lane owns element i: it obtains its `degree` coefficients once (PRF blocks, or loads), keeps them
// in registers, runs one Horner chain per party and stores n field elements: 32 B read and n * 32 B written per element
// (64 B read where the secret is the product of two share vectors, ShamirMulPrfSrc: the re-deal of a multiplication; the
// same 64 B, contiguous per lane, where the two factors are the interleaved halves L[i] = v[2 i], R[i] = v[2 i + 1] of one GKR
// layer, ShamirPairsPrfSrc: the re-deal of a tree level of the grand product).
// fr_mul_small_add (the Horner step) and shamir_prf_fr (the coefficients) live in shamir_deal.hip.hpp, shared with the fused re-deal of
// primary_group.inc.
struct ShamirOut {
    fe* p[COZK_SHAMIR_MAX_PARTIES];
};
struct ShamirPrfCoefs {  // coef_c[i] = PRF(keys[c - 1], counter + i)
    uint64_t counter;
    prf_key keys[COZK_SHAMIR_MAX_DEGREE];
    __device__ __forceinline__ fe coef(int c, size_t i) const {
        prf_key key;  // a copy in scalar registers: no address of the kernel argument is taken
#pragma unroll
        for (int w = 0; w < 8; w++) key.k[w] = keys[c].k[w];
        return shamir_prf_fr(key, counter + i);
    }
};
struct ShamirPrfSrc : ShamirPrfCoefs {  // a secret vector, PRF coefficients
    const fe* v;
    __device__ __forceinline__ fe value(size_t i) const { return fe_load(v + i); }
};
struct ShamirMulPrfSrc : ShamirPrfCoefs {  // the secret is the product a[i] b[i] of two share vectors, never stored (GRR re-deal)
    const fe *a, *b;
    __device__ __forceinline__ fe value(size_t i) const { return Fr::mul(fe_load(a + i), fe_load(b + i)); }
};
struct ShamirPairsPrfSrc : ShamirPrfCoefs {  // the secret is the product v[2 i] v[2 i + 1] of one interleaved GKR layer, never stored (a tree level)
    const fe* v;
    __device__ __forceinline__ fe value(size_t i) const { return Fr::mul(fe_load(v + 2 * i), fe_load(v + 2 * i + 1)); }
};
struct ShamirRandPrfSrc : ShamirPrfCoefs {  // the secret is itself a PRF element, never stored (double-random pairs, offline)
    prf_key key0;
    __device__ __forceinline__ fe value(size_t i) const {
        prf_key key;
#pragma unroll
        for (int w = 0; w < 8; w++) key.k[w] = key0.k[w];
        return shamir_prf_fr(key, counter + i);
    }
};
struct ShamirVecSrc {  // the caller's coefficient vectors
    const fe* v;
    const fe* c[COZK_SHAMIR_MAX_DEGREE];
    __device__ __forceinline__ fe coef(int k, size_t i) const { return fe_load(c[k] + i); }
    __device__ __forceinline__ fe value(size_t i) const { return fe_load(v + i); }
};

// DEG = 1..7: the degree at compile time, c[k] = coefficient k + 1.  DEG = 0: degree 8..15 at run time; the coefficients are
// then produced by ONE rolled loop (one copy of the ChaCha block, the key or pointer picked by a wave-uniform index) and pushed
// into c[] as a shift register, so that c[] is only ever indexed with constants and stays in registers: after the loop
// c[j] = coefficient deg - j, the leading one first, which is the order Horner consumes them in.
template <int DEG, class Src>
__global__ void __launch_bounds__(256) k_shamir_share(Src src, ShamirOut out, size_t n, int degree, int num_parties) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int MAXD = DEG ? DEG : COZK_SHAMIR_MAX_DEGREE;
    const int deg = DEG ? DEG : degree;
    fe c[MAXD];
    if (DEG) {
#pragma unroll
        for (int k = 0; k < MAXD; k++) c[MAXD - 1 - k] = src.coef(k, i);
    } else {
#pragma unroll
        for (int k = 0; k < MAXD; k++) c[k] = Fr::zero();
#pragma unroll 1
        for (int k = 0; k < deg; k++) {
            const fe next = src.coef(k, i);
#pragma unroll
            for (int m = MAXD - 1; m > 0; m--) c[m] = c[m - 1];
            c[0] = next;
        }
    }
    const fe v = src.value(i);
#pragma unroll 1  // one Horner chain at a time: the coefficients, not several parties' accumulators, own the registers
    for (int p = 1; p <= num_parties; p++) {
        fe acc = c[0];
#pragma unroll
        for (int m = 1; m < MAXD; m++)
            if (m < deg) acc = fr_mul_small_add(acc, (uint32_t)p, c[m]);
        fe_store(out.p[p - 1] + i, fr_mul_small_add(acc, (uint32_t)p, v));
    }
}

template <class Src>
static void launch_share(hipStream_t st, const Src& src, const ShamirOut& out, size_t n, int degree, int num_parties) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    switch (degree) {
#define SHAMIR_CASE_(D) case D: k_shamir_share<D, Src><<<grid, 256, 0, st>>>(src, out, n, degree, num_parties); break
        SHAMIR_CASE_(1);
        SHAMIR_CASE_(2);
        SHAMIR_CASE_(3);
        SHAMIR_CASE_(4);
        SHAMIR_CASE_(5);
        SHAMIR_CASE_(6);
        SHAMIR_CASE_(7);
#undef SHAMIR_CASE_
        default: k_shamir_share<0, Src><<<grid, 256, 0, st>>>(src, out, n, degree, num_parties); break;
    }
    HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ combine: out[i] = sum_j lambda_j s_j[i]
// (shamir.rs:314-322 `reconstruct` per element).  lambda travels in the kernel arguments (uniform across the wave); the
// products go into one wide accumulator and are reduced once per element (poly.hip.hpp FrWide, as k_poly_eval_chi and
// k_poly_lincomb do).  k_poly_lincomb itself takes device-side pointer and coefficient tables over polynomial handles,
// so it is not reused here.
struct ShamirCombineArgs {
    const fe* s[COZK_SHAMIR_MAX_PARTIES];
    fe lambda[COZK_SHAMIR_MAX_PARTIES];
};
__global__ void __launch_bounds__(256) k_shamir_combine(ShamirCombineArgs a, int k, fe* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    FrWide w;
    fr_wide_zero(w);
    for (int j = 0; j < k; j++) fr_wide_mac(w, fe_load(a.s[j] + i), a.lambda[j]);
    fe_store(out + i, fr_wide_reduce(w));
}

__global__ void __launch_bounds__(256) k_fe_add_scalar(fe* __restrict__ v, size_t n, fe s) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fe_store(v + i, Fr::add(fe_load(v + i), s));
}

// ------------------------------------------------------------------ extract: out_k[i] = sum_j (j + 1)^k s_j[i]
// The Vandermonde step of the double-random preprocessing (Damgard-Nielsen): count <= n - 1 <= 31 outputs from n <= 32
// inputs.  k_shamir_combine would re-read every input once per output; here a lane owns element i, the rolled loop over j loads
// s_j[i] ONCE per tile of SHAMIR_EXTRACT_TILE outputs into a running value w = s_j (j + 1)^k, and per output of the tile adds w to
// that output's accumulator and steps w with fr_mul_small_add(w, j + 1, 0) (j + 1 <= 32: inside its proven input bound; the
// result is canonical, so is every Fr::add of canonical values, so is every store).  A tile that does not begin at k = 0 starts
// from w = s_j (j + 1)^k0 by ONE Montgomery product with a constant from the kernel arguments (the 8 k0 small steps it replaces
// cost as much at k0 = 8 and more after).  Pointers and constants travel in the kernel arguments, indexed by the wave-uniform j.
// The tile is 8 accumulators (64 VGPRs); the kernel compiles to 164 VGPRs (160 for the SCALED variant), 3 waves per SIMD, no
// scratch.  A tile of 4 compiles to 116 (4 waves) and doubles the re-reads, 12 to 220 (2 waves), 16 to 256 (1 wave).
#define SHAMIR_EXTRACT_TILE 8
struct ShamirExtractArgs {
    const fe* s[COZK_SHAMIR_MAX_PARTIES];
    fe* out[SHAMIR_EXTRACT_TILE];
    fe start[COZK_SHAMIR_MAX_PARTIES];  // (j + 1)^k0, Montgomery; read only by the SCALED variant
};
template <bool SCALED>  // a tile that begins at k0 > 0
__global__ void __launch_bounds__(256) k_shamir_extract(ShamirExtractArgs a, int num_in, int cnt, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe acc[SHAMIR_EXTRACT_TILE];
#pragma unroll
    for (int k = 0; k < SHAMIR_EXTRACT_TILE; k++) acc[k] = Fr::zero();
#pragma unroll 1
    for (int j = 0; j < num_in; j++) {
        fe w = fe_load(a.s[j] + i);
        if (SCALED) w = Fr::mul(w, a.start[j]);
#pragma unroll
        for (int k = 0; k < SHAMIR_EXTRACT_TILE; k++)
            if (k < cnt) {
                acc[k] = Fr::add(acc[k], w);
                if (k + 1 < cnt) w = fr_mul_small_add(w, (uint32_t)j + 1, Fr::zero());
                __builtin_amdgcn_sched_barrier(0);  // keeps the scheduler from running the tile's powers of w ahead of their additions (176 VGPRs, 2 waves)
            }
    }
#pragma unroll
    for (int k = 0; k < SHAMIR_EXTRACT_TILE; k++)
        if (k < cnt) fe_store(a.out[k] + i, acc[k]);
}

// out[i] = a[i] b[i] + c[i]: the mask of the king multiplication (96 B read, 32 B written; the product is never stored)
__global__ void __launch_bounds__(256) k_fe_mul_add(const fe* __restrict__ a, const fe* __restrict__ b, const fe* __restrict__ c, fe* __restrict__ out,
                                                    size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fe_store(out + i, Fr::add(Fr::mul(fe_load(a + i), fe_load(b + i)), fe_load(c + i)));
}

// out[j] = v[2 j] v[2 j + 1] + r2t[j]: k_fe_mul_add for one interleaved GKR layer, the mask of a tree level of the king construct.
// A lane owns product j and reads its 64 contiguous bytes of the layer: 96 B read, 32 B written, the product never stored.  The
// caller passes r2t already advanced by its element offset into the half of the pair: no slice is copied.
__global__ void __launch_bounds__(256) k_shamir_mask_pairs(const fe* __restrict__ v, const fe* __restrict__ r2t, fe* __restrict__ out, size_t m) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) fe_store(out + j, Fr::add(Fr::mul(fe_load(v + 2 * j), fe_load(v + 2 * j + 1)), fe_load(r2t + j)));
}

// ------------------------------------------------------------------ king finish: z = sum_p lambda_p m_p, c_q = z - rt_q for every q
// The king's open and the unmask of every party of its device in ONE launch.  A lane owns element i: z as in k_shamir_combine
// (lambda in the kernel arguments, one FrWide accumulator reduced once: canonical), then a ROLLED loop over the `count` recipients
// whose pointers travel in the kernel arguments, indexed by the wave-uniform q as ShamirExtractArgs' are: one load, one Fr::sub
// (canonical in, canonical out) and one store per recipient; z itself is stored only where the caller wants it (parties on other
// devices).  rt[q] arrives advanced by the element offset into the half of the pair.  (k + count) x 32 B read and count x 32 B
// (+ 32 B) written per element.
struct ShamirKingFinishArgs {
    const fe* m[COZK_SHAMIR_MAX_PARTIES];
    fe lambda[COZK_SHAMIR_MAX_PARTIES];
    const fe* rt[COZK_SHAMIR_MAX_PARTIES];
    fe* out[COZK_SHAMIR_MAX_PARTIES];
};
__global__ void __launch_bounds__(256) k_shamir_king_finish(ShamirKingFinishArgs a, int k, int count, fe* __restrict__ z_out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    FrWide w;
    fr_wide_zero(w);
    for (int j = 0; j < k; j++) fr_wide_mac(w, fe_load(a.m[j] + i), a.lambda[j]);
    const fe z = fr_wide_reduce(w);
    if (z_out) fe_store(z_out + i, z);
#pragma unroll 1
    for (int q = 0; q < count; q++) fe_store(a.out[q] + i, Fr::sub(z, fe_load(a.rt[q] + i)));
}

// ------------------------------------------------------------------ host
static fe fe_from_abi(const uint64_t s[4]) {
    fe r;
    for (int i = 0; i < 4; i++) {
        r.l[2 * i] = (uint32_t)s[i];
        r.l[2 * i + 1] = (uint32_t)(s[i] >> 32);
    }
    return r;
}
static void fe_to_abi(const fe& a, uint64_t s[4]) {
    for (int i = 0; i < 4; i++) s[i] = (uint64_t)a.l[2 * i] | ((uint64_t)a.l[2 * i + 1] << 32);
}

static void require_points(const uint32_t* points, size_t k, const char* who) {
    const std::string w(who);
    COZK_REQUIRE(points, w + ": null points");
    COZK_REQUIRE(k >= 1 && k <= COZK_SHAMIR_MAX_PARTIES, w + ": 1 <= k <= COZK_SHAMIR_MAX_PARTIES points");
    uint64_t seen = 0;
    for (size_t i = 0; i < k; i++) {
        COZK_REQUIRE(points[i] >= 1 && points[i] <= COZK_SHAMIR_MAX_PARTIES, w + ": points must lie in 1..COZK_SHAMIR_MAX_PARTIES");
        COZK_REQUIRE(!((seen >> points[i]) & 1), w + ": points must be distinct");
        seen |= (uint64_t)1 << points[i];
    }
}

static void require_share_args(const char* who, int degree, int num_parties) {
    const std::string w(who);
    COZK_REQUIRE(degree >= 1 && degree <= COZK_SHAMIR_MAX_DEGREE, w + ": 1 <= degree <= COZK_SHAMIR_MAX_DEGREE");
    COZK_REQUIRE(num_parties > degree && num_parties <= COZK_SHAMIR_MAX_PARTIES, w + ": degree < num_parties <= COZK_SHAMIR_MAX_PARTIES");
}

static void require_mul_args(const char* who, int degree, int num_parties) {
    require_share_args(who, degree, num_parties);
    COZK_REQUIRE(2 * degree + 1 <= num_parties, std::string(who) + ": 2 * degree + 1 <= num_parties (that many parties re-deal the product)");
}

static void require_factors(const char* who, const cozk_vec* a, const cozk_vec* b) {
    const std::string w(who);
    COZK_REQUIRE(a->kind == COZK_SCALAR_FR && b->kind == COZK_SCALAR_FR, w + ": the factors must be FR vectors");
    COZK_REQUIRE(a->n == b->n, w + ": the factors must have one length");
}

static void require_pairs(const char* who, const cozk_vec* v) {
    const std::string w(who);
    COZK_REQUIRE(v->kind == COZK_SCALAR_FR, w + ": the layer must be an FR vector");
    COZK_REQUIRE(v->n % 2 == 0, w + ": the layer must have an even length (L[j] = v[2 j], R[j] = v[2 j + 1])");
}

static void free_all(cozk_vec** out, int n) {
    for (int p = 0; p < n; p++) {
        cozk_vec_free(out[p]);
        out[p] = nullptr;
    }
}

// the num_parties outputs, from ctxs[p]'s allocator (or from `one`'s for all of them); on failure none is left
static int alloc_outputs(cozk_ctx* one, cozk_ctx* const* ctxs, size_t n, int num_parties, cozk_vec** out) {
    for (int p = 0; p < num_parties; p++) {
        int rc = cozk_vec_alloc(ctxs ? ctxs[p] : one, n, COZK_SCALAR_FR, &out[p]);
        if (rc != COZK_OK) {
            out[p] = nullptr;
            free_all(out, num_parties);
            return rc;
        }
    }
    return COZK_OK;
}

static void clear_outputs(cozk_vec** out, int num_parties) {
    if (num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES)
        for (int p = 0; p < num_parties; p++) out[p] = nullptr;
}

template <class Src>
static void fill_prf_coefs(Src& src, const uint8_t* keys, int degree, uint64_t counter) {
    memset(&src, 0, sizeof src);
    src.counter = counter;
    for (int c = 0; c < degree; c++) src.keys[c] = prf_key_from_bytes(keys + (size_t)COZK_PRF_KEY_BYTES * c);
}
static ShamirPrfSrc prf_src(const cozk_vec* v, const uint8_t* keys, int degree, uint64_t counter) {
    ShamirPrfSrc src;
    fill_prf_coefs(src, keys, degree, counter);
    src.v = (const fe*)v->d;
    return src;
}
static ShamirMulPrfSrc mul_prf_src(const cozk_vec* a, const cozk_vec* b, const uint8_t* keys, int degree, uint64_t counter) {
    ShamirMulPrfSrc src;
    fill_prf_coefs(src, keys, degree, counter);
    src.a = (const fe*)a->d;
    src.b = (const fe*)b->d;
    return src;
}

static ShamirPairsPrfSrc pairs_prf_src(const cozk_vec* v, const uint8_t* keys, int degree, uint64_t counter) {
    ShamirPairsPrfSrc src;
    fill_prf_coefs(src, keys, degree, counter);
    src.v = (const fe*)v->d;
    return src;
}

// a null output pointer is reported through cozk_last_error like every other bad argument
static int require_out(cozk_ctx* ctx, const void* out, const char* msg) {
    return cozk_guard(ctx, [&] { COZK_REQUIRE(out, msg); });
}

static ShamirOut out_table(cozk_vec* const* out, int num_parties) {
    ShamirOut o;
    memset(&o, 0, sizeof o);
    for (int p = 0; p < num_parties; p++) o.p[p] = (fe*)out[p]->d;
    return o;
}

// ------------------------------------------------------------------ the skeleton of an entry point of ONE context
// An output table of such an entry point: `len` handles from ctx's pool (from owners[p]'s where the parties own them:
// cozk_shamir_scatter); an optional table may be absent (the z of cozk_shamir_king_finish).
struct OutTable {
    cozk_vec** v;
    int len;
    bool optional = false;
    cozk_ctx* const* owners = nullptr;
};

// Every table that is there is cleared (where its length is a count at all: slots of an unknown number stay untouched) and a
// missing one is refused with `null_out`; check() throws on a bad argument and returns the element count n of every output; the
// tables are allocated; launch(n) enqueues on ctx's stream, unless n = 0.  Whatever fails, no table is left holding a handle.
template <class Check, class Launch>
static int entry_point(cozk_ctx* ctx, const char* null_out, std::initializer_list<OutTable> tables, Check check, Launch launch) {
    bool missing = false;
    for (const OutTable& t : tables) {
        if (t.v) clear_outputs(t.v, t.len);
        else missing |= !t.optional;
    }
    size_t n = 0;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(!missing, null_out);
        n = check();
    });
    if (rc != COZK_OK) return rc;
    auto drop = [&] {
        for (const OutTable& t : tables)
            if (t.v) free_all(t.v, t.len);
    };
    for (const OutTable& t : tables)
        if (t.v && (rc = alloc_outputs(ctx, t.owners, n, t.len, t.v)) != COZK_OK) {
            drop();
            return rc;
        }
    rc = cozk_guard(ctx, [&] {
        if (n) launch(n);
    });
    if (rc != COZK_OK) drop();
    return rc;
}

// ------------------------------------------------------------------ one party's vector among the arguments of an in-process call
// there, FR, (of an even length,) of n elements, a block of that party's context -- in this order.  The texts are the entry
// point's own, behind its name
struct OwnVecTexts {
    std::string null, kind, even /* empty: either parity */, len, own;
};
static void require_own_vec(const char* who, const cozk_vec* v, const cozk_ctx* ctx, size_t n, const OwnVecTexts& t) {
    const std::string w = std::string(who) + ": ";
    COZK_REQUIRE(v, w + t.null);
    COZK_REQUIRE(v->kind == COZK_SCALAR_FR, w + t.kind);
    COZK_REQUIRE(t.even.empty() || v->n % 2 == 0, w + t.even);
    COZK_REQUIRE(v->n == n, w + t.len);
    COZK_REQUIRE(v->ctx == ctx, w + t.own);
}
// a factor or a half of the pair of the king multiplication
static void require_own_vec(const char* who, const cozk_vec* v, const cozk_ctx* ctx, size_t n, const char* what) {
    const std::string s(what);
    require_own_vec(who, v, ctx, n, {"null " + s, s + " must be an FR vector", "", "the factors and the pair must have one length", s + " must be a vector of its party's context"});
}
// party p's interleaved GKR layer (require_pairs' texts)
static const OwnVecTexts LAYER_TEXTS = {"parties 0..2 * degree need their layer", "the layer must be an FR vector",
                                        "the layer must have an even length (L[j] = v[2 j], R[j] = v[2 j + 1])", "the layers must have one length",
                                        "party p's layer must be a vector of party_ctxs[p]"};

// ------------------------------------------------------------------ the in-process drivers: one thread, one context per party
// Who may touch a block, and when.  A context's pool orders its blocks by that context's stream only (common.hpp): a block a
// party has just freed may still be read by a kernel in flight on that party's stream, and a block handed out is assumed to be
// used on that stream.  The drivers below let one context's stream write into another context's block, so they keep three rules:
//   1. before any stream writes into a block of another context, the OWNER's stream has drained (every driver drains every
//      party's stream once, after it has allocated and before the first launch);
//   2. the owner's stream reads such a block only after the WRITER's stream has drained (the drain step after the launches,
//      which also gives the writers' staging blocks back);
//   3. a block returns to its pool only behind its last reader on the owner's stream, or after a drain.
//
// The staged fan-out: dealer's stream writes one vector of n elements for each of `count` recipients -- launch(table) is the
// caller's dealing kernel -- into dst[q] in place where recipient q lives on the dealer's device, else into a slice of ONE
// staging block of the dealer's followed by one peer copy.  The caller has seen to rule 1, drains the dealer's stream before
// anybody reads (rule 2) and then frees *stage, also where this throws.
template <class Launch>
static void fan_out(cozk_ctx* dealer, cozk_ctx* const* rcp, fe* const* dst, int count, size_t n, fe** stage, Launch launch) {
    size_t remote = 0;
    for (int q = 0; q < count; q++) remote += rcp[q]->device != dealer->device;
    if (remote) *stage = (fe*)ctx_dev_alloc(dealer, remote * n * sizeof(fe));
    ShamirOut o;
    memset(&o, 0, sizeof o);
    size_t r = 0;
    for (int q = 0; q < count; q++) o.p[q] = rcp[q]->device != dealer->device ? *stage + n * r++ : dst[q];
    launch(o);
    for (int q = 0; q < count; q++)
        if (rcp[q]->device != dealer->device)
            HIP_TRY(hipMemcpyPeerAsync(dst[q], rcp[q]->device, o.p[q], dealer->device, n * sizeof(fe), dealer->stream));
}

static int drain_all(cozk_ctx* const* pcs, int parties) {
    return cozk_guard(pcs[0], [&] {
        for (int q = 0; q < parties; q++) HIP_TRY(hipStreamSynchronize(pcs[q]->stream));
    });
}

// the writers' streams drain (rule 2) and their staging blocks go back
static int drain_writers(cozk_ctx* const* pcs, int writers, fe** stage, int* failed) {
    for (int p = 0; p < writers; p++) {
        int rc = cozk_guard(pcs[p], [&] {
            HIP_TRY(hipStreamSynchronize(pcs[p]->stream));
            ctx_dev_free(pcs[p], stage[p]);
            stage[p] = nullptr;
        });
        if (rc != COZK_OK) {
            *failed = p;
            return rc;
        }
    }
    return COZK_OK;
}

// The all-to-all deal: parties 0..dealers - 1 each deal n elements with `degree` coefficients to parties 0..rcp - 1 (one launch of
// the dealing kernel with the source src_of(p) and one fan_out per dealer), then finish(q, row) enqueues recipient q's step on
// its own stream -- row[p] = what dealer p dealt to q, a block of q -- and produces q's outputs; q's pool takes the row back
// behind it (rule 3).  A failure of party p's step leaves its text with party 0 and nothing of the driver's own allocated; what
// finish has produced by then is the caller's to free.
template <class SrcOf, class Finish>
static int deal_all_to_all(cozk_ctx* const* pcs, size_t n, int dealers, int rcp, int degree, SrcOf src_of, Finish finish) {
    cozk_ctx* const c0 = pcs[0];
    const int parties = dealers > rcp ? dealers : rcp;
    int rc = COZK_OK;
    std::vector<cozk_vec*> recv((size_t)rcp * dealers, nullptr);  // recv[q * dealers + p]
    std::vector<fe*> stage(dealers, nullptr);
    auto fail = [&](int code, int p) {
        if (pcs[p] != c0) c0->last_error = pcs[p]->last_error;
        for (int q = 0; q < parties; q++) (void)hipStreamSynchronize(pcs[q]->stream);
        for (int d = 0; d < dealers; d++) ctx_dev_free(pcs[d], stage[d]);
        for (cozk_vec* v : recv) cozk_vec_free(v);
        return code;
    };
    for (int q = 0; q < rcp; q++)
        for (int p = 0; p < dealers; p++)
            if ((rc = cozk_vec_alloc(pcs[q], n, COZK_SCALAR_FR, &recv[(size_t)q * dealers + p])) != COZK_OK) return fail(rc, q);
    if (n) {
        if ((rc = drain_all(pcs, parties)) != COZK_OK) return fail(rc, 0);
        for (int p = 0; p < dealers; p++) {
            rc = cozk_guard(pcs[p], [&] {
                fe* dst[COZK_SHAMIR_MAX_PARTIES];
                for (int q = 0; q < rcp; q++) dst[q] = (fe*)recv[(size_t)q * dealers + p]->d;
                fan_out(pcs[p], pcs, dst, rcp, n, &stage[p], [&](const ShamirOut& o) { launch_share(pcs[p]->stream, src_of(p), o, n, degree, rcp); });
            });
            if (rc != COZK_OK) return fail(rc, p);
        }
        int failed = 0;
        if ((rc = drain_writers(pcs, dealers, stage.data(), &failed)) != COZK_OK) return fail(rc, failed);
    }
    for (int q = 0; q < rcp; q++) {
        cozk_vec** row = &recv[(size_t)q * dealers];
        if ((rc = finish(q, row)) != COZK_OK) return fail(rc, q);
        free_all(row, dealers);
    }
    return COZK_OK;
}

extern "C" {

int cozk_shamir_share_vec(cozk_ctx* ctx, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties, uint64_t counter,
                          cozk_vec** out) {
    return entry_point(
        ctx, "shamir_share_vec: null output", {{out, num_parties}},
        [&] {
            COZK_REQUIRE(ctx && v && keys, "shamir_share_vec: null argument");
            COZK_REQUIRE(v->kind == COZK_SCALAR_FR, "shamir_share_vec: the secret must be an FR vector");
            require_share_args("shamir_share_vec", degree, num_parties);
            return v->n;
        },
        [&](size_t n) { launch_share(ctx->stream, prf_src(v, keys, degree, counter), out_table(out, num_parties), n, degree, num_parties); });
}

int cozk_shamir_eval_vec(cozk_ctx* ctx, const cozk_vec* const* coeffs, int degree, int num_parties, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_eval_vec: null output", {{out, num_parties}},
        [&] {
            COZK_REQUIRE(ctx && coeffs, "shamir_eval_vec: null argument");
            require_share_args("shamir_eval_vec", degree, num_parties);
            for (int c = 0; c <= degree; c++) {
                COZK_REQUIRE(coeffs[c] && coeffs[c]->kind == COZK_SCALAR_FR, "shamir_eval_vec: degree + 1 FR coefficient vectors");
                COZK_REQUIRE(coeffs[c]->n == coeffs[0]->n, "shamir_eval_vec: coefficient vectors must have equal length");
            }
            return coeffs[0]->n;
        },
        [&](size_t n) {
            ShamirVecSrc src;
            memset(&src, 0, sizeof src);
            src.v = (const fe*)coeffs[0]->d;
            for (int c = 1; c <= degree; c++) src.c[c - 1] = (const fe*)coeffs[c]->d;
            launch_share(ctx->stream, src, out_table(out, num_parties), n, degree, num_parties);
        });
}

// cozk_rep3_scatter for Shamir: party p's vector is a block of party_ctxs[p]'s allocator, written by the dealer's stream (fan_out)
int cozk_shamir_scatter(cozk_ctx* dealer, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties, uint64_t counter,
                        cozk_ctx* const* party_ctxs, cozk_vec** out) {
    fe* stage = nullptr;
    int rc = entry_point(
        dealer, "shamir_scatter: null output", {{out, num_parties, false, party_ctxs}},
        [&] {
            COZK_REQUIRE(dealer && v && keys && party_ctxs, "shamir_scatter: null argument");
            COZK_REQUIRE(v->kind == COZK_SCALAR_FR, "shamir_scatter: the secret must be an FR vector");
            require_share_args("shamir_scatter", degree, num_parties);
            for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_scatter: null party context");
            return v->n;
        },
        [&](size_t n) {
            for (int p = 0; p < num_parties; p++) HIP_TRY(hipStreamSynchronize(party_ctxs[p]->stream));  // rule 1
            fan_out(dealer, party_ctxs, out_table(out, num_parties).p, num_parties, n, &stage,
                    [&](const ShamirOut& o) { launch_share(dealer->stream, prf_src(v, keys, degree, counter), o, n, degree, num_parties); });
            HIP_TRY(hipStreamSynchronize(dealer->stream));  // rule 2: the parties' streams may use the shares as soon as this returns
        });
    ctx_dev_free(dealer, stage);
    return rc;
}

int cozk_shamir_lagrange(const uint32_t* points, size_t k, uint64_t* out) {
    return cozk_guard(nullptr, [&] {
        COZK_REQUIRE(out, "shamir_lagrange: null output");
        require_points(points, k, "shamir_lagrange");
        fe l[COZK_SHAMIR_MAX_PARTIES];
        lagrange_host(points, k, l);
        for (size_t i = 0; i < k; i++) fe_to_abi(l[i], out + 4 * i);
    });
}

int cozk_shamir_combine_vec(cozk_ctx* ctx, const cozk_vec* const* shares, const uint32_t* points, size_t k, int degree,
                            cozk_vec** out) {
    return entry_point(
        ctx, "shamir_combine_vec: null output", {{out, 1}},
        [&] {
            COZK_REQUIRE(ctx && shares, "shamir_combine_vec: null argument");
            require_points(points, k, "shamir_combine_vec");
            COZK_REQUIRE(degree >= 0 && (size_t)degree < k, "shamir_combine_vec: 0 <= degree < k (degree + 1 shares are needed)");
            for (size_t j = 0; j < k; j++) {
                COZK_REQUIRE(shares[j] && shares[j]->kind == COZK_SCALAR_FR, "shamir_combine_vec: k FR share vectors");
                COZK_REQUIRE(shares[j]->n == shares[0]->n, "shamir_combine_vec: share vectors must have equal length");
            }
            return shares[0]->n;
        },
        [&](size_t n) {
            ShamirCombineArgs a;
            memset(&a, 0, sizeof a);
            lagrange_host(points, (size_t)degree + 1, a.lambda);  // of points[..=degree]: only those shares are used
            for (int j = 0; j <= degree; j++) a.s[j] = (const fe*)shares[j]->d;
            k_shamir_combine<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(a, degree + 1, (fe*)(*out)->d, n);
            HIP_TRY(hipGetLastError());
        });
}

int cozk_shamir_combine_points(cozk_ctx* ctx, const uint64_t* xy, const int* infinity, const uint32_t* points, size_t k, int degree,
                               uint64_t out_xy[8], int* out_infinity) {
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(xy && out_xy && out_infinity, "shamir_combine_points: null argument");
        require_points(points, k, "shamir_combine_points");
        COZK_REQUIRE(degree >= 0 && (size_t)degree < k, "shamir_combine_points: 0 <= degree < k (degree + 1 shares are needed)");
    });
    if (rc != COZK_OK) return rc;
    fe l[COZK_SHAMIR_MAX_PARTIES];
    lagrange_host(points, (size_t)degree + 1, l);
    uint64_t scaled[COZK_SHAMIR_MAX_PARTIES * 8];
    int scaled_inf[COZK_SHAMIR_MAX_PARTIES];
    for (int j = 0; j <= degree; j++) {  // reconstruct_point (shamir.rs:432-440): sum_j lambda_j P_j
        uint64_t s[4];
        fe_to_abi(l[j], s);
        rc = cozk_g1_mul(ctx, xy + 8 * j, infinity ? infinity[j] : 0, s, scaled + 8 * j, &scaled_inf[j]);
        if (rc != COZK_OK) return rc;
    }
    return cozk_g1_sum(ctx, scaled, scaled_inf, (size_t)degree + 1, out_xy, out_infinity);
}

// ------------------------------------------------------------------ multiplication with degree reduction (GRR / BGW resharing)
// c = a b as a degree-t sharing again: the dealers, parties 0..2t, each re-deal their local product a_p b_p with degree t
// (one k_shamir_share<.., ShamirMulPrfSrc> launch), every party receives one vector from every dealer, and party q's result is
// sum_p lambda_p h_{p -> q}, lambda = lagrange(1..2t + 1) -- which is cozk_shamir_combine_vec of the received vectors with
// degree 2t.  The reference has no such step (no Shamir network at all); tests/shamir_mul_ref.py restates it.
int cozk_shamir_mul_deal(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const uint8_t* keys, int degree, int num_parties,
                         uint64_t counter, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_mul_deal: null output", {{out, num_parties}},
        [&] {
            COZK_REQUIRE(ctx && a && b && keys, "shamir_mul_deal: null argument");
            require_factors("shamir_mul_deal", a, b);
            require_mul_args("shamir_mul_deal", degree, num_parties);
            return a->n;
        },
        [&](size_t n) { launch_share(ctx->stream, mul_prf_src(a, b, keys, degree, counter), out_table(out, num_parties), n, degree, num_parties); });
}

}  // extern "C"

// what cozk_shamir_mul_inproc and cozk_shamir_mul_pairs_inproc share, behind their argument checks: n elements per party,
// src_of(p) = dealer p's source for the dealing kernel, the finish = the degree-2t combine
template <class SrcOf>
static int mul_all_to_all(cozk_ctx* const* party_ctxs, size_t n, int degree, int num_parties, cozk_vec** out, SrcOf src_of) {
    const int dealers = 2 * degree + 1;
    uint32_t points[COZK_SHAMIR_MAX_PARTIES];
    for (int p = 0; p < dealers; p++) points[p] = (uint32_t)p + 1;
    int rc = deal_all_to_all(party_ctxs, n, dealers, num_parties, degree, src_of, [&](int q, cozk_vec* const* row) {
        return cozk_shamir_combine_vec(party_ctxs[q], row, points, (size_t)dealers, 2 * degree, &out[q]);
    });
    if (rc != COZK_OK) free_all(out, num_parties);
    return rc;
}

extern "C" {

int cozk_shamir_mul_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* a, const cozk_vec* const* b, const uint8_t* const* keys,
                           int degree, int num_parties, uint64_t counter, cozk_vec** out) {
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 ? party_ctxs[0] : nullptr;  // receives the error message
    if (int rc0 = require_out(c0, out, "shamir_mul_inproc: null output")) return rc0;
    clear_outputs(out, num_parties);
    const int dealers = 2 * degree + 1;
    int rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && a && b && keys, "shamir_mul_inproc: null argument");
        require_mul_args("shamir_mul_inproc", degree, num_parties);
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_mul_inproc: null party context");
        for (int p = 0; p < dealers; p++) {
            COZK_REQUIRE(a[p] && b[p], "shamir_mul_inproc: parties 0..2 * degree need both factors");
            require_factors("shamir_mul_inproc", a[p], b[p]);
            COZK_REQUIRE(a[p]->n == a[0]->n, "shamir_mul_inproc: the factors must have one length");
            COZK_REQUIRE(a[p]->ctx == party_ctxs[p] && b[p]->ctx == party_ctxs[p], "shamir_mul_inproc: party p's factors must be vectors of party_ctxs[p]");
            COZK_REQUIRE(keys[p], "shamir_mul_inproc: parties 0..2 * degree need their key block");
        }
    });
    if (rc != COZK_OK) return rc;
    return mul_all_to_all(party_ctxs, a[0]->n, degree, num_parties, out, [&](int p) { return mul_prf_src(a[p], b[p], keys[p], degree, counter); });
}

int cozk_shamir_mul_deal_pairs(cozk_ctx* ctx, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties, uint64_t counter, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_mul_deal_pairs: null output", {{out, num_parties}},
        [&] {
            COZK_REQUIRE(ctx && v && keys, "shamir_mul_deal_pairs: null argument");
            require_pairs("shamir_mul_deal_pairs", v);
            require_mul_args("shamir_mul_deal_pairs", degree, num_parties);
            return v->n / 2;
        },
        [&](size_t m) { launch_share(ctx->stream, pairs_prf_src(v, keys, degree, counter), out_table(out, num_parties), m, degree, num_parties); });
}

int cozk_shamir_mul_pairs_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* v, const uint8_t* const* keys, int degree, int num_parties,
                                 uint64_t counter, cozk_vec** out) {
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 ? party_ctxs[0] : nullptr;  // receives the error message
    if (int rc0 = require_out(c0, out, "shamir_mul_pairs_inproc: null output")) return rc0;
    clear_outputs(out, num_parties);
    int rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && v && keys, "shamir_mul_pairs_inproc: null argument");
        require_mul_args("shamir_mul_pairs_inproc", degree, num_parties);
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_mul_pairs_inproc: null party context");
        COZK_REQUIRE(v[0], "shamir_mul_pairs_inproc: parties 0..2 * degree need their layer");
        for (int p = 0; p < 2 * degree + 1; p++) {
            require_own_vec("shamir_mul_pairs_inproc", v[p], party_ctxs[p], v[0]->n, LAYER_TEXTS);
            COZK_REQUIRE(keys[p], "shamir_mul_pairs_inproc: parties 0..2 * degree need their key block");
        }
    });
    if (rc != COZK_OK) return rc;
    return mul_all_to_all(party_ctxs, v[0]->n / 2, degree, num_parties, out, [&](int p) { return pairs_prf_src(v[p], keys[p], degree, counter); });
}

int cozk_shamir_mul_vec(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const uint8_t* keys, int degree, uint64_t counter, cozk_vec** out) {
    if (int rc0 = require_out(ctx, out, "shamir_mul_vec: null output")) return rc0;
    *out = nullptr;
    bool dealer = false;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && a, "shamir_mul_vec: null argument");
        COZK_REQUIRE(a->kind == COZK_SCALAR_FR, "shamir_mul_vec: the factors must be FR vectors");
        COZK_REQUIRE(ctx->ring_comm, "shamir_mul_vec: cozk_ring_init has not been called on this context");
        require_mul_args("shamir_mul_vec (num_parties = ranks of the ring)", degree, ctx->ring_n);
        dealer = ctx->ring_rank <= 2 * degree;
        if (dealer) {
            COZK_REQUIRE(b && keys, "shamir_mul_vec: null argument");
            require_factors("shamir_mul_vec", a, b);
        }
    });
    if (rc != COZK_OK) return rc;
    const int num_parties = ctx->ring_n, dealers = 2 * degree + 1, self = ctx->ring_rank;
    cozk_vec *dealt[COZK_SHAMIR_MAX_PARTIES] = {}, *recv[COZK_SHAMIR_MAX_PARTIES] = {};
    const cozk_vec *send[COZK_SHAMIR_MAX_PARTIES] = {}, *shares[COZK_SHAMIR_MAX_PARTIES] = {};
    uint32_t points[COZK_SHAMIR_MAX_PARTIES];
    if (dealer) rc = cozk_shamir_mul_deal(ctx, a, b, keys, degree, num_parties, counter, dealt);
    for (int p = 0; p < dealers && rc == COZK_OK; p++)
        if (p != self) rc = cozk_vec_alloc(ctx, a->n, COZK_SCALAR_FR, &recv[p]);
    if (rc == COZK_OK) {
        for (int q = 0; q < num_parties; q++) send[q] = dealer && q != self ? dealt[q] : nullptr;  // the own slot stays local
        rc = cozk_ring_all_to_all(ctx, send, recv);
    }
    if (rc == COZK_OK) {
        for (int p = 0; p < dealers; p++) {
            shares[p] = p == self ? dealt[p] : recv[p];
            points[p] = (uint32_t)p + 1;
        }
        rc = cozk_shamir_combine_vec(ctx, shares, points, (size_t)dealers, 2 * degree, out);
    }
    // everything above is enqueued on the context's stream, and so is whatever reuses these blocks
    free_all(dealt, num_parties);
    free_all(recv, num_parties);
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ multiplication with a king and double-random pairs
// (Damgard-Nielsen; semi-honest).  Offline, every party deals one random secret twice -- degree t and degree 2t, two launches of
// the dealing kernel with the ShamirRandPrfSrc source, which recomputes the secret and never stores it -- everyone receives one
// vector of each kind from everyone, and the (n - t) x n Vandermonde matrix on the points 1..n (k_shamir_extract) turns the n
// received vectors into n - t pairs ([r]_t, [r]_2t) no t parties know.  Online, parties 0..2t send a b + r_2t to the king, who
// opens z = a b + r with the degree-2t combine and sends it to everyone; party q keeps z - r_t.  The reference has none of it;
// tests/shamir_dn_ref.py restates it.
static void require_rand_args(const char* who, int degree, int num_parties) {
    const std::string w(who);
    COZK_REQUIRE(degree >= 1 && 2 * degree <= COZK_SHAMIR_MAX_DEGREE, w + ": 1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE (the degree-2t sharing is dealt too)");
    COZK_REQUIRE(2 * degree + 1 <= num_parties && num_parties <= COZK_SHAMIR_MAX_PARTIES, w + ": 2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES");
}

// keys[0] = the secret stream; `degree` coefficient keys from keys[first]
static ShamirRandPrfSrc rand_prf_src(const uint8_t* keys, int first, int degree, uint64_t counter) {
    ShamirRandPrfSrc src;
    fill_prf_coefs(src, keys + (size_t)COZK_PRF_KEY_BYTES * first, degree, counter);
    src.key0 = prf_key_from_bytes(keys);
    return src;
}

static void launch_extract(hipStream_t st, const fe* const* in, int num_in, int count, fe* const* out, size_t n) {
    for (int k0 = 0; k0 < count; k0 += SHAMIR_EXTRACT_TILE) {
        ShamirExtractArgs a;
        memset(&a, 0, sizeof a);
        const int cnt = count - k0 < SHAMIR_EXTRACT_TILE ? count - k0 : SHAMIR_EXTRACT_TILE;
        for (int k = 0; k < cnt; k++) a.out[k] = out[k0 + k];
        for (int j = 0; j < num_in; j++) {
            a.s[j] = in[j];
            if (!k0) continue;
            const fe x = Fr::from_u64((uint64_t)j + 1);
            fe pw = Fr::one();
            for (int e = 0; e < k0; e++) pw = Fr::mul(pw, x);
            a.start[j] = pw;
        }
        const unsigned grid = (unsigned)((n + 255) / 256);
        if (k0) k_shamir_extract<true><<<grid, 256, 0, st>>>(a, num_in, cnt, n);
        else k_shamir_extract<false><<<grid, 256, 0, st>>>(a, num_in, cnt, n);
        HIP_TRY(hipGetLastError());
    }
}

// both output tables are required; where only one is given it is still cleared
static int require_out2(cozk_ctx* ctx, cozk_vec** x, cozk_vec** y, int len, const char* msg) {
    int rc = cozk_guard(ctx, [&] { COZK_REQUIRE(x && y, msg); });
    if (rc != COZK_OK) {
        if (x) clear_outputs(x, len);
        if (y) clear_outputs(y, len);
    }
    return rc;
}

static void launch_mul_add(hipStream_t st, const cozk_vec* a, const cozk_vec* b, const cozk_vec* c, fe* out) {
    if (a->n == 0) return;
    k_fe_mul_add<<<(unsigned)((a->n + 255) / 256), 256, 0, st>>>((const fe*)a->d, (const fe*)b->d, (const fe*)c->d, out, a->n);
    HIP_TRY(hipGetLastError());
}

// one degree of the preprocessing: every party deals with `deg` coefficient keys from keys[p][first] to parties 0..rcp - 1, each
// of which extracts `count` vectors into r[q * count + k] (cozk_shamir_rand_inproc: rcp = np, count = np - t).  The caller frees r.
static int rand_pass(cozk_ctx* const* pcs, const uint8_t* const* keys, size_t n, int first, int deg, int np, int rcp, int count, uint64_t counter,
                     cozk_vec** r) {
    return deal_all_to_all(
        pcs, n, np, rcp, deg, [&](int p) { return rand_prf_src(keys[p], first, deg, counter); },
        [&](int q, cozk_vec* const* row) { return cozk_shamir_rand_extract(pcs[q], row, np, count, &r[(size_t)q * count]); });
}

// the preprocessing of the king grand product (csrc/host/shamir_gp.hpp), which extracts only what it uses: `count` <= np - t pairs,
// the degree-t halves for parties 0..rcp_t - 1 into r_t[q * count + k], the degree-2t halves for the senders 0..2t into
// r_2t[p * count + k].  The values are those of cozk_shamir_rand_inproc at the same keys and counter (a party that is dealt
// nothing changes no other party's vectors).  Arguments are the caller's to check; on failure both tables are NULL.
int shamir_rand_pairs_inproc(cozk_ctx* const* pcs, const uint8_t* const* keys, size_t n_elems, int t, int np, uint64_t counter, int count, int rcp_t,
                             cozk_vec** r_t, cozk_vec** r_2t) {
    const int senders = 2 * t + 1;
    for (int i = 0; i < rcp_t * count; i++) r_t[i] = nullptr;
    for (int i = 0; i < senders * count; i++) r_2t[i] = nullptr;
    int rc = rand_pass(pcs, keys, n_elems, 1, t, np, rcp_t, count, counter, r_t);
    if (rc == COZK_OK) rc = rand_pass(pcs, keys, n_elems, 1 + t, 2 * t, np, senders, count, counter, r_2t);
    if (rc != COZK_OK) {
        free_all(r_t, rcp_t * count);
        free_all(r_2t, senders * count);
    }
    return rc;
}

extern "C" {

int cozk_shamir_rand_deal(cozk_ctx* ctx, size_t n_elems, const uint8_t* keys, int degree, int num_parties, uint64_t counter, cozk_vec** out_t,
                          cozk_vec** out_2t) {
    return entry_point(
        ctx, "shamir_rand_deal: null output", {{out_t, num_parties}, {out_2t, num_parties}},
        [&] {
            COZK_REQUIRE(ctx && keys, "shamir_rand_deal: null argument");
            require_rand_args("shamir_rand_deal", degree, num_parties);
            return n_elems;
        },
        [&](size_t n) {
            launch_share(ctx->stream, rand_prf_src(keys, 1, degree, counter), out_table(out_t, num_parties), n, degree, num_parties);
            launch_share(ctx->stream, rand_prf_src(keys, 1 + degree, 2 * degree, counter), out_table(out_2t, num_parties), n, 2 * degree, num_parties);
        });
}

int cozk_shamir_rand_extract(cozk_ctx* ctx, const cozk_vec* const* recv, int num_parties, int count, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_rand_extract: null output", {{out, count}},
        [&] {
            COZK_REQUIRE(ctx && recv, "shamir_rand_extract: null argument");
            COZK_REQUIRE(num_parties >= 2 && num_parties <= COZK_SHAMIR_MAX_PARTIES, "shamir_rand_extract: 2 <= num_parties <= COZK_SHAMIR_MAX_PARTIES");
            COZK_REQUIRE(count >= 1 && count <= num_parties - 1, "shamir_rand_extract: 1 <= count <= num_parties - 1");
            for (int j = 0; j < num_parties; j++) {
                COZK_REQUIRE(recv[j] && recv[j]->kind == COZK_SCALAR_FR, "shamir_rand_extract: num_parties FR vectors");
                COZK_REQUIRE(recv[j]->n == recv[0]->n, "shamir_rand_extract: the vectors must have one length");
            }
            return recv[0]->n;
        },
        [&](size_t n) {
            const fe* in[COZK_SHAMIR_MAX_PARTIES];
            fe* o[COZK_SHAMIR_MAX_PARTIES];
            for (int j = 0; j < num_parties; j++) in[j] = (const fe*)recv[j]->d;
            for (int k = 0; k < count; k++) o[k] = (fe*)out[k]->d;
            launch_extract(ctx->stream, in, num_parties, count, o, n);
        });
}

int cozk_shamir_rand_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* keys, size_t n_elems, int degree, int num_parties, uint64_t counter,
                            cozk_vec** r_t, cozk_vec** r_2t) {
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 ? party_ctxs[0] : nullptr;  // receives the error message
    // n (n - t) handles per table: that length is known once 1 <= degree < num_parties <= COZK_SHAMIR_MAX_PARTIES
    const bool known = num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES && degree >= 1 && degree < num_parties;
    const size_t len = known ? (size_t)num_parties * (num_parties - degree) : 0;
    auto clear = [&](cozk_vec** t) {
        for (size_t i = 0; t && i < len; i++) t[i] = nullptr;
    };
    clear(r_t), clear(r_2t);
    int rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(r_t && r_2t, "shamir_rand_inproc: null output");
        COZK_REQUIRE(party_ctxs && keys, "shamir_rand_inproc: null argument");
        require_rand_args("shamir_rand_inproc", degree, num_parties);
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_rand_inproc: null party context");
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(keys[p], "shamir_rand_inproc: every party needs its key block");
    });
    if (rc != COZK_OK) return rc;
    // one degree after the other: n^2 receive vectors are alive at a time, not 2 n^2
    rc = rand_pass(party_ctxs, keys, n_elems, 1, degree, num_parties, num_parties, num_parties - degree, counter, r_t);
    if (rc == COZK_OK) rc = rand_pass(party_ctxs, keys, n_elems, 1 + degree, 2 * degree, num_parties, num_parties, num_parties - degree, counter, r_2t);
    if (rc != COZK_OK)
        for (size_t i = 0; i < len; i++) {
            cozk_vec_free(r_t[i]);
            cozk_vec_free(r_2t[i]);
            r_t[i] = r_2t[i] = nullptr;
        }
    return rc;
}

int cozk_shamir_rand_vec(cozk_ctx* ctx, size_t n_elems, const uint8_t* keys, int degree, uint64_t counter, cozk_vec** r_t, cozk_vec** r_2t) {
    // ring ranks - degree handles per table: known once there is a ring and 1 <= degree < its ranks
    const int count = ctx && ctx->ring_comm && degree >= 1 && degree < ctx->ring_n && ctx->ring_n <= COZK_SHAMIR_MAX_PARTIES ? ctx->ring_n - degree : 0;
    if (int rc0 = require_out2(ctx, r_t, r_2t, count, "shamir_rand_vec: null output")) return rc0;
    clear_outputs(r_t, count);
    clear_outputs(r_2t, count);
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && keys, "shamir_rand_vec: null argument");
        COZK_REQUIRE(ctx->ring_comm, "shamir_rand_vec: cozk_ring_init has not been called on this context");
        require_rand_args("shamir_rand_vec (num_parties = ranks of the ring)", degree, ctx->ring_n);
    });
    if (rc != COZK_OK) return rc;
    const int np = ctx->ring_n, self = ctx->ring_rank;
    cozk_vec *dealt[2][COZK_SHAMIR_MAX_PARTIES] = {}, *recv[2][COZK_SHAMIR_MAX_PARTIES] = {};
    rc = cozk_shamir_rand_deal(ctx, n_elems, keys, degree, np, counter, dealt[0], dealt[1]);
    for (int h = 0; h < 2 && rc == COZK_OK; h++) {
        for (int p = 0; p < np && rc == COZK_OK; p++)
            if (p != self) rc = cozk_vec_alloc(ctx, n_elems, COZK_SCALAR_FR, &recv[h][p]);
        if (rc != COZK_OK) break;
        const cozk_vec *send[COZK_SHAMIR_MAX_PARTIES] = {}, *got[COZK_SHAMIR_MAX_PARTIES] = {};
        for (int q = 0; q < np; q++) send[q] = q != self ? dealt[h][q] : nullptr;  // the own slot stays local
        rc = cozk_ring_all_to_all(ctx, send, recv[h]);
        if (rc != COZK_OK) break;
        for (int p = 0; p < np; p++) got[p] = p == self ? dealt[h][p] : recv[h][p];
        rc = cozk_shamir_rand_extract(ctx, got, np, count, h ? r_2t : r_t);
    }
    // everything above is enqueued on the context's stream, and so is whatever reuses these blocks
    for (int h = 0; h < 2; h++) {
        free_all(dealt[h], np);
        free_all(recv[h], np);
    }
    if (rc != COZK_OK) {
        free_all(r_t, count);
        free_all(r_2t, count);
    }
    return rc;
}

int cozk_shamir_mul_mask(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const cozk_vec* r_2t, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_mul_mask: null output", {{out, 1}},
        [&] {
            COZK_REQUIRE(ctx && a && b && r_2t, "shamir_mul_mask: null argument");
            COZK_REQUIRE(a->kind == COZK_SCALAR_FR && b->kind == COZK_SCALAR_FR && r_2t->kind == COZK_SCALAR_FR, "shamir_mul_mask: the factors and the mask must be FR vectors");
            COZK_REQUIRE(a->n == b->n && a->n == r_2t->n, "shamir_mul_mask: the factors and the mask must have one length");
            return a->n;
        },
        [&](size_t) { launch_mul_add(ctx->stream, a, b, r_2t, (fe*)(*out)->d); });
}

}  // extern "C"

// ------------------------------------------------------------------ the online step with a king, in process
// The halves of a pair are addressed by an element offset, so that one preprocessed pair serves many tree levels of the king
// grand product; the king's open and the unmasks of its device are one launch (k_shamir_king_finish).
static void launch_mask_pairs(hipStream_t st, const cozk_vec* v, const cozk_vec* r_2t, size_t off, fe* out) {
    const size_t m = v->n / 2;
    if (m == 0) return;
    k_shamir_mask_pairs<<<(unsigned)((m + 255) / 256), 256, 0, st>>>((const fe*)v->d, (const fe*)r_2t->d + off, out, m);
    HIP_TRY(hipGetLastError());
}

// z = sum_{j < k} lambda_j m[j], lambda = lagrange(1..k); out[q] = z - (rt[q] + off) for q < count; z_out may be null
static void launch_king_finish(hipStream_t st, const fe* const* m, int k, const fe* const* rt, size_t off, int count, fe* const* out, fe* z_out, size_t n) {
    if (n == 0) return;
    ShamirKingFinishArgs a;
    memset(&a, 0, sizeof a);
    uint32_t points[COZK_SHAMIR_MAX_PARTIES];
    for (int j = 0; j < k; j++) points[j] = (uint32_t)j + 1;
    lagrange_host(points, (size_t)k, a.lambda);
    for (int j = 0; j < k; j++) a.m[j] = m[j];
    for (int q = 0; q < count; q++) {
        a.rt[q] = rt[q] + off;
        a.out[q] = out[q];
    }
    k_shamir_king_finish<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(a, k, count, z_out, n);
    HIP_TRY(hipGetLastError());
}

// the same launch for poly.hip's translation unit (cozk_primary_group_level_king, primary_group.inc): m = rows of its staging block, out =
// the members' level buffers
void shamir_launch_king_finish(hipStream_t st, const fe* const* m, int k, const fe* const* rt, size_t off, int count, fe* const* out, size_t n) {
    launch_king_finish(st, m, k, rt, off, count, out, nullptr, n);
}

// off + len <= have without overflow
static bool slice_fits(size_t off, size_t len, size_t have) { return off <= have && len <= have - off; }

// The king driver behind cozk_shamir_mul_king_inproc and cozk_shamir_mul_king_pairs_inproc: n products per party, the pair read from
// element r_offset.  mask(p, dst) enqueues sender p's masked products m_p on p's stream into dst.  The fan-in mirrors fan_out:
// dst is the king's block where sender p lives on the king's device, else a staging block of p's followed by one peer copy.  Then
// ONE launch on the king's stream opens z = sum_p lambda_p m_p and writes c_q = z - rt_q for every party q of the king's device;
// z itself is stored only where some party lives on another device, peer-copied there by the king's stream, and subtracted on
// that party's own stream (the same kernel, k = 1).  The three rules above fan_out hold: rule 1 by the one drain of every stream
// (the senders write into the king's blocks, the king into every recipient's), rule 2 by the senders' drain and the king's.
template <class Mask>
static int king_drive(cozk_ctx* const* party_ctxs, const cozk_vec* const* r_t, size_t n, size_t r_offset, int degree, int num_parties, int king,
                      cozk_vec** out, Mask mask) {
    cozk_ctx *const c0 = party_ctxs[0], *const kc = party_ctxs[king];
    const int senders = 2 * degree + 1;
    int rc = COZK_OK;
    cozk_vec* m[COZK_SHAMIR_MAX_PARTIES] = {};   // m[p], a block of the king
    fe* stage[COZK_SHAMIR_MAX_PARTIES] = {};     // the same on a sender's other device
    cozk_vec* zq[COZK_SHAMIR_MAX_PARTIES] = {};  // z on a party's other device, a block of that party
    cozk_vec* z = nullptr;                       // z on the king's device: only where some party lives on another
    // a failure of party p's step leaves its text with party 0 and nothing allocated
    auto fail = [&](int code, int p) {
        if (party_ctxs[p] != c0) c0->last_error = party_ctxs[p]->last_error;
        for (int q = 0; q < num_parties; q++) (void)hipStreamSynchronize(party_ctxs[q]->stream);
        for (int s = 0; s < senders; s++) ctx_dev_free(party_ctxs[s], stage[s]);
        free_all(m, senders);
        free_all(zq, num_parties);
        cozk_vec_free(z);
        free_all(out, num_parties);
        return code;
    };
    bool any_remote = false;
    for (int p = 0; p < senders; p++)
        if ((rc = cozk_vec_alloc(kc, n, COZK_SCALAR_FR, &m[p])) != COZK_OK) return fail(rc, king);
    for (int q = 0; q < num_parties; q++) {
        if (party_ctxs[q]->device != kc->device) {
            any_remote = true;
            if ((rc = cozk_vec_alloc(party_ctxs[q], n, COZK_SCALAR_FR, &zq[q])) != COZK_OK) return fail(rc, q);
        }
        if ((rc = cozk_vec_alloc(party_ctxs[q], n, COZK_SCALAR_FR, &out[q])) != COZK_OK) {
            out[q] = nullptr;
            return fail(rc, q);
        }
    }
    if (any_remote && (rc = cozk_vec_alloc(kc, n, COZK_SCALAR_FR, &z)) != COZK_OK) return fail(rc, king);
    if (n == 0) {
        free_all(m, senders);
        free_all(zq, num_parties);
        cozk_vec_free(z);
        return COZK_OK;
    }
    if ((rc = drain_all(party_ctxs, num_parties)) != COZK_OK) return fail(rc, 0);
    for (int p = 0; p < senders; p++) {  // the fan-in: the mask on each sender's own stream, into the king's memory
        cozk_ctx* sc = party_ctxs[p];
        rc = cozk_guard(sc, [&] {
            const bool remote = sc->device != kc->device;
            if (remote) stage[p] = (fe*)ctx_dev_alloc(sc, n * sizeof(fe));
            mask(p, remote ? stage[p] : (fe*)m[p]->d);
            if (remote) HIP_TRY(hipMemcpyPeerAsync(m[p]->d, kc->device, stage[p], sc->device, n * sizeof(fe), sc->stream));
        });
        if (rc != COZK_OK) return fail(rc, p);
    }
    int failed = 0;
    if ((rc = drain_writers(party_ctxs, senders, stage, &failed)) != COZK_OK) return fail(rc, failed);
    rc = cozk_guard(kc, [&] {
        const fe *mp[COZK_SHAMIR_MAX_PARTIES], *rt[COZK_SHAMIR_MAX_PARTIES];
        fe* o[COZK_SHAMIR_MAX_PARTIES];
        int count = 0;
        for (int p = 0; p < senders; p++) mp[p] = (const fe*)m[p]->d;
        for (int q = 0; q < num_parties; q++)
            if (!zq[q]) {
                rt[count] = (const fe*)r_t[q]->d;
                o[count++] = (fe*)out[q]->d;
            }
        launch_king_finish(kc->stream, mp, senders, rt, r_offset, count, o, z ? (fe*)z->d : nullptr, n);
        for (int q = 0; q < num_parties; q++)  // z to the other devices by the king's stream
            if (zq[q]) HIP_TRY(hipMemcpyPeerAsync(zq[q]->d, party_ctxs[q]->device, z->d, kc->device, n * sizeof(fe), kc->stream));
        HIP_TRY(hipStreamSynchronize(kc->stream));  // the recipients' streams may use their blocks as soon as this returns
    });
    if (rc != COZK_OK) return fail(rc, king);
    free_all(m, senders);
    cozk_vec_free(z);
    z = nullptr;
    for (int q = 0; q < num_parties; q++) {
        if (!zq[q]) continue;
        rc = cozk_guard(party_ctxs[q], [&] {
            const fe *mp[1] = {(const fe*)zq[q]->d}, *rt[1] = {(const fe*)r_t[q]->d};
            fe* o[1] = {(fe*)out[q]->d};
            launch_king_finish(party_ctxs[q]->stream, mp, 1, rt, r_offset, 1, o, nullptr, n);  // lagrange(1) = 1
        });
        if (rc != COZK_OK) return fail(rc, q);
    }
    free_all(zq, num_parties);  // each behind its reader on its owner's stream
    return COZK_OK;
}

extern "C" {

int cozk_shamir_mul_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* a, const cozk_vec* const* b, const cozk_vec* const* r_t,
                                const cozk_vec* const* r_2t, int degree, int num_parties, int king, cozk_vec** out) {
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 ? party_ctxs[0] : nullptr;  // receives the error message
    if (int rc0 = require_out(c0, out, "shamir_mul_king_inproc: null output")) return rc0;
    clear_outputs(out, num_parties);
    const char* who = "shamir_mul_king_inproc";
    int rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && a && b && r_t && r_2t, "shamir_mul_king_inproc: null argument");
        require_rand_args(who, degree, num_parties);
        COZK_REQUIRE(king >= 0 && king < num_parties, "shamir_mul_king_inproc: 0 <= king < num_parties");
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_mul_king_inproc: null party context");
        COZK_REQUIRE(r_t[0], "shamir_mul_king_inproc: null first half of the pair");
        for (int p = 0; p < num_parties; p++) require_own_vec(who, r_t[p], party_ctxs[p], r_t[0]->n, "the first half of the pair");
        for (int p = 0; p < 2 * degree + 1; p++) {
            require_own_vec(who, a[p], party_ctxs[p], r_t[0]->n, "a factor of parties 0..2 * degree");
            require_own_vec(who, b[p], party_ctxs[p], r_t[0]->n, "a factor of parties 0..2 * degree");
            require_own_vec(who, r_2t[p], party_ctxs[p], r_t[0]->n, "the second half of the pair of parties 0..2 * degree");
        }
    });
    if (rc != COZK_OK) return rc;
    return king_drive(party_ctxs, r_t, r_t[0]->n, 0, degree, num_parties, king, out,
                      [&](int p, fe* dst) { launch_mul_add(party_ctxs[p]->stream, a[p], b[p], r_2t[p], dst); });
}

int cozk_shamir_mul_king_vec(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const cozk_vec* r_t, const cozk_vec* r_2t, int degree, int king,
                             cozk_vec** out) {
    if (int rc0 = require_out(ctx, out, "shamir_mul_king_vec: null output")) return rc0;
    *out = nullptr;
    const char* who = "shamir_mul_king_vec";
    bool sender = false;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && r_t, "shamir_mul_king_vec: null argument");
        COZK_REQUIRE(ctx->ring_comm, "shamir_mul_king_vec: cozk_ring_init has not been called on this context");
        require_rand_args("shamir_mul_king_vec (num_parties = ranks of the ring)", degree, ctx->ring_n);
        COZK_REQUIRE(king >= 0 && king < ctx->ring_n, "shamir_mul_king_vec: 0 <= king < ranks of the ring");
        require_own_vec(who, r_t, ctx, r_t->n, "the first half of the pair");
        sender = ctx->ring_rank <= 2 * degree;
        if (sender) {
            require_own_vec(who, a, ctx, r_t->n, "a factor of parties 0..2 * degree");
            require_own_vec(who, b, ctx, r_t->n, "a factor of parties 0..2 * degree");
            require_own_vec(who, r_2t, ctx, r_t->n, "the second half of the pair of parties 0..2 * degree");
        }
    });
    if (rc != COZK_OK) return rc;
    const int np = ctx->ring_n, senders = 2 * degree + 1, self = ctx->ring_rank;
    const size_t n = r_t->n;
    cozk_vec *m = nullptr, *z = nullptr, *recv[COZK_SHAMIR_MAX_PARTIES] = {};
    const cozk_vec *send[COZK_SHAMIR_MAX_PARTIES] = {}, *shares[COZK_SHAMIR_MAX_PARTIES] = {};
    if (sender) rc = cozk_shamir_mul_mask(ctx, a, b, r_2t, &m);
    if (self == king)
        for (int p = 0; p < senders && rc == COZK_OK; p++)
            if (p != self) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_FR, &recv[p]);
    if (rc == COZK_OK) {  // round 1: the gather to the king (its own slot stays local)
        if (sender && self != king) send[king] = m;
        rc = cozk_ring_all_to_all(ctx, send, recv);
    }
    if (rc == COZK_OK && self == king) {
        uint32_t points[COZK_SHAMIR_MAX_PARTIES];
        for (int p = 0; p < senders; p++) {
            shares[p] = p == self ? m : recv[p];
            points[p] = (uint32_t)p + 1;
        }
        rc = cozk_shamir_combine_vec(ctx, shares, points, (size_t)senders, 2 * degree, &z);
    }
    free_all(recv, np);
    cozk_vec_free(m);
    if (rc == COZK_OK && self != king) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_FR, &z);
    if (rc == COZK_OK) {  // round 2: the king's fan-out
        for (int q = 0; q < np; q++) send[q] = self == king && q != self ? z : nullptr;
        if (self != king) recv[king] = z;
        rc = cozk_ring_all_to_all(ctx, send, recv);
    }
    if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, n, COZK_SCALAR_FR, out);
    if (rc == COZK_OK) rc = cozk_vec_binop(ctx, COZK_OP_SUB, 0, z, r_t, *out);
    // everything above is enqueued on the context's stream, and so is whatever reuses these blocks
    cozk_vec_free(z);
    if (rc != COZK_OK) {
        cozk_vec_free(*out);
        *out = nullptr;
    }
    return rc;
}

int cozk_shamir_mul_mask_pairs(cozk_ctx* ctx, const cozk_vec* v, const cozk_vec* r_2t, size_t r_offset, cozk_vec** out) {
    return entry_point(
        ctx, "shamir_mul_mask_pairs: null output", {{out, 1}},
        [&] {
            COZK_REQUIRE(ctx && v && r_2t, "shamir_mul_mask_pairs: null argument");
            require_pairs("shamir_mul_mask_pairs", v);
            COZK_REQUIRE(r_2t->kind == COZK_SCALAR_FR, "shamir_mul_mask_pairs: the mask must be an FR vector");
            COZK_REQUIRE(slice_fits(r_offset, v->n / 2, r_2t->n), "shamir_mul_mask_pairs: r_offset + len(v) / 2 <= len(r_2t)");
            return v->n / 2;
        },
        [&](size_t) { launch_mask_pairs(ctx->stream, v, r_2t, r_offset, (fe*)(*out)->d); });
}

int cozk_shamir_king_finish(cozk_ctx* ctx, const cozk_vec* const* masked, int degree, const cozk_vec* const* r_t, size_t r_offset, int count,
                            cozk_vec** out, cozk_vec** z_out) {
    const int k = 2 * degree + 1;
    return entry_point(
        ctx, "shamir_king_finish: null output", {{out, count}, {z_out, 1, true}},
        [&] {
            COZK_REQUIRE(ctx && masked && r_t, "shamir_king_finish: null argument");
            COZK_REQUIRE(degree >= 1 && degree <= COZK_SHAMIR_MAX_DEGREE, "shamir_king_finish: 1 <= degree <= COZK_SHAMIR_MAX_DEGREE (2 * degree + 1 masked vectors)");
            COZK_REQUIRE(count >= 1 && count <= COZK_SHAMIR_MAX_PARTIES, "shamir_king_finish: 1 <= count <= COZK_SHAMIR_MAX_PARTIES");
            for (int j = 0; j < k; j++) {
                COZK_REQUIRE(masked[j] && masked[j]->kind == COZK_SCALAR_FR, "shamir_king_finish: 2 * degree + 1 masked FR vectors");
                COZK_REQUIRE(masked[j]->n == masked[0]->n, "shamir_king_finish: the masked vectors must have one length");
            }
            for (int q = 0; q < count; q++) {
                COZK_REQUIRE(r_t[q] && r_t[q]->kind == COZK_SCALAR_FR, "shamir_king_finish: count FR first halves of the pair");
                COZK_REQUIRE(slice_fits(r_offset, masked[0]->n, r_t[q]->n), "shamir_king_finish: r_offset + len(masked) <= len(r_t)");
            }
            return masked[0]->n;
        },
        [&](size_t n) {
            const fe *m[COZK_SHAMIR_MAX_PARTIES], *rt[COZK_SHAMIR_MAX_PARTIES];
            fe* o[COZK_SHAMIR_MAX_PARTIES];
            for (int j = 0; j < k; j++) m[j] = (const fe*)masked[j]->d;
            for (int q = 0; q < count; q++) {
                rt[q] = (const fe*)r_t[q]->d;
                o[q] = (fe*)out[q]->d;
            }
            launch_king_finish(ctx->stream, m, k, rt, r_offset, count, o, z_out ? (fe*)(*z_out)->d : nullptr, n);
        });
}

int cozk_shamir_mul_king_pairs_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* v, const cozk_vec* const* r_t, const cozk_vec* const* r_2t,
                                      size_t r_offset, int degree, int num_parties, int king, cozk_vec** out) {
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 ? party_ctxs[0] : nullptr;  // receives the error message
    if (int rc0 = require_out(c0, out, "shamir_mul_king_pairs_inproc: null output")) return rc0;
    clear_outputs(out, num_parties);
    const char* who = "shamir_mul_king_pairs_inproc";
    int rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && v && r_t && r_2t, "shamir_mul_king_pairs_inproc: null argument");
        require_rand_args(who, degree, num_parties);
        COZK_REQUIRE(king >= 0 && king < num_parties, "shamir_mul_king_pairs_inproc: 0 <= king < num_parties");
        for (int p = 0; p < num_parties; p++) COZK_REQUIRE(party_ctxs[p], "shamir_mul_king_pairs_inproc: null party context");
        COZK_REQUIRE(v[0], "shamir_mul_king_pairs_inproc: parties 0..2 * degree need their layer");
        COZK_REQUIRE(r_t[0], "shamir_mul_king_pairs_inproc: null first half of the pair");
        OwnVecTexts half = {"null first half of the pair", "the halves of the pair must be FR vectors", "", "the halves of the pair must have one length",
                            "party p's halves of the pair must be vectors of party_ctxs[p]"};
        for (int p = 0; p < num_parties; p++) require_own_vec(who, r_t[p], party_ctxs[p], r_t[0]->n, half);
        half.null = "parties 0..2 * degree need the second half of the pair";
        for (int p = 0; p < 2 * degree + 1; p++) {
            require_own_vec(who, v[p], party_ctxs[p], v[0]->n, LAYER_TEXTS);
            require_own_vec(who, r_2t[p], party_ctxs[p], r_t[0]->n, half);
        }
        COZK_REQUIRE(slice_fits(r_offset, v[0]->n / 2, r_t[0]->n), "shamir_mul_king_pairs_inproc: r_offset + len(v) / 2 <= len of the halves of the pair");
    });
    if (rc != COZK_OK) return rc;
    return king_drive(party_ctxs, r_t, v[0]->n / 2, r_offset, degree, num_parties, king, out,
                      [&](int p, fe* dst) { launch_mask_pairs(party_ctxs[p]->stream, v[p], r_2t[p], r_offset, dst); });
}

int cozk_vec_add_scalar(cozk_ctx* ctx, cozk_vec* v, const uint64_t s[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && v && s && v->kind == COZK_SCALAR_FR, "vec_add_scalar: bad argument");
        if (v->n == 0) return;
        k_fe_add_scalar<<<(unsigned)((v->n + 255) / 256), 256, 0, ctx->stream>>>((fe*)v->d, v->n, fe_from_abi(s));
        HIP_TRY(hipGetLastError());
    });
}

}  // extern "C"
