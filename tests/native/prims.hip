// Test-only harness over the product's arithmetic headers: element-wise kernels for the 8 x 32 Montgomery fields (canonical and
// lazy operations), the XYZZ G1 formulas and the 9 x 29 layers, plus host wrappers for the host paths of the same headers (the
// two host Montgomery products, SHA-256, the transcript), and the wide dot-product accumulator FrWide of poly.hip.hpp.  The headers are included, never copied: what is tested is the code
// the kernels inline.  Each device wrapper uploads host arrays of u32 limbs, launches, synchronises, downloads and returns the
// HIP status.  Built by co-zkvms_amd/build.py (build_prims) into tests/native/libcozk_prims.so; driven by tests/test_gpu_prims.py
// and tests/test_host_prims.py.
#include <stdlib.h>

#include "../../co-zkvms_amd/csrc/fr9.hip.hpp"
#include "../../co-zkvms_amd/csrc/host/wire.hpp"
#include "../../co-zkvms_amd/csrc/poly.hip.hpp"

#define PRIMS_NAME_(n) #n ","

// ------------------------------------------------------------------------------------------------ 8 x 32 fields
// op names in enum order: the Python side maps names to numbers through prims_ff_ops()
#define FF_OPS(X)                                                                                                         \
    X(add) X(sub) X(neg) X(dbl) X(mul) X(sqr) X(mul2) X(mul_add2) X(mul_sub2) X(to_mont) X(from_mont) X(from_u64) X(pow)    \
    X(inv) X(mul_nr) X(mul_add2_nr) X(lmul) X(lmul2) X(ladd) X(lsub) X(ldbl) X(lneg) X(lmul_sub2) X(lis_zero) X(lcanon)   \
    X(mul_host) X(mul_host32)
#define FF_ENUM_(n) FF_##n,
enum { FF_OPS(FF_ENUM_) FF_NOPS };
static const char* const FF_NAMES = FF_OPS(PRIMS_NAME_);

// o1 (and o2 for the paired products) = op(a, b, c, d); false for an op this side does not have.  The exponent of pow is b's
// limbs; from_u64 reads a's two low limbs; lis_zero answers in o1.l[0].
template <class F>
static __host__ __device__ bool ff_apply(int op, const fe& a, const fe& b, const fe& c, const fe& d, fe& o1, fe& o2) {
    o1 = F::zero();
    o2 = F::zero();
    switch (op) {
        case FF_add: o1 = F::add(a, b); return true;
        case FF_sub: o1 = F::sub(a, b); return true;
        case FF_neg: o1 = F::neg(a); return true;
        case FF_dbl: o1 = F::dbl(a); return true;
        case FF_mul: o1 = F::mul(a, b); return true;
        case FF_sqr: o1 = F::sqr(a); return true;
        case FF_mul2: F::mul2(a, b, c, d, o1, o2); return true;
        case FF_mul_add2: o1 = F::mul_add2(a, b, c, d); return true;
        case FF_mul_sub2: o1 = F::mul_sub2(a, b, c, d); return true;
        case FF_to_mont: o1 = F::to_mont(a); return true;
        case FF_from_mont: o1 = F::from_mont(a); return true;
        case FF_from_u64: o1 = F::from_u64((uint64_t)a.l[0] | ((uint64_t)a.l[1] << 32)); return true;
        case FF_pow: o1 = F::pow(a, b.l); return true;
        case FF_inv: o1 = F::inv(a); return true;
        case FF_lmul: o1 = F::lmul(a, b); return true;
        case FF_lmul2: F::lmul2(a, b, c, d, o1, o2); return true;
        case FF_ladd: o1 = F::ladd(a, b); return true;
        case FF_lsub: o1 = F::lsub(a, b); return true;
        case FF_ldbl: o1 = F::ldbl(a); return true;
        case FF_lneg: o1 = F::lneg(a); return true;
        case FF_lmul_sub2: o1 = F::lmul_sub2(a, b, c, d); return true;
        case FF_lis_zero: o1.l[0] = F::lis_zero(a) ? 1u : 0u; return true;
        case FF_lcanon: o1 = F::lcanon(a); return true;
#if defined(__HIP_DEVICE_COMPILE__)
        case FF_mul_nr: o1 = F::mul_nr(a, b); return true;
        case FF_mul_add2_nr: o1 = F::mul_add2_nr(a, b, c, d); return true;
#else
        case FF_mul_host: o1 = F::mul_host(a, b); return true;
        case FF_mul_host32: o1 = F::mul_host32(a, b); return true;
#endif
        default: return false;
    }
}

template <class F>
__global__ void k_ff(int op, const fe* a, const fe* b, const fe* c, const fe* d, fe* out, uint32_t* ok, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe o1, o2;
    ok[i] = ff_apply<F>(op, a[i], b[i], c[i], d[i], o1, o2) ? 1u : 0u;
    out[2 * i] = o1;
    out[2 * i + 1] = o2;
}

// ------------------------------------------------------------------------------------------------ G1 (XYZZ, lazy range)
// p is an XYZZ point; q's (x, y) an affine point (q itself for add).  Affine results land in out's (x, y), on_curve in out.x.l[0].
#define G1_OPS(X) X(add_mixed) X(add) X(dbl) X(dbl_affine) X(to_affine) X(neg_affine) X(neg_xyzz) X(on_curve)
#define G1_ENUM_(n) G1_##n,
enum { G1_OPS(G1_ENUM_) G1_NOPS };
static const char* const G1_NAMES = G1_OPS(PRIMS_NAME_);

__global__ void k_g1(int op, const g1_xyzz* p, const g1_xyzz* q, g1_xyzz* out, uint32_t* ok, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const g1_xyzz P = p[i], Qx = q[i];
    g1_affine Q;
    Q.x = Qx.x;
    Q.y = Qx.y;
    g1_xyzz r = G1::identity();
    bool done = true;
    switch (op) {
        case G1_add_mixed: r = G1::add_mixed(P, Q); break;
        case G1_add: r = G1::add(P, Qx); break;
        case G1_dbl: r = G1::dbl(P); break;
        case G1_dbl_affine: r = G1::dbl_affine(Q); break;
        case G1_to_affine: {
            const g1_affine a = G1::to_affine(P);
            r.x = a.x;
            r.y = a.y;
            break;
        }
        case G1_neg_affine: {
            const g1_affine a = G1::neg(Q);
            r.x = a.x;
            r.y = a.y;
            break;
        }
        case G1_neg_xyzz: r = G1::neg(P); break;
        case G1_on_curve: r.x.l[0] = G1::on_curve(Q) ? 1u : 0u; break;
        default: done = false;
    }
    ok[i] = done ? 1u : 0u;
    out[i] = r;
}

// ------------------------------------------------------------------------------------------------ 9 x 29 layers
// a, b, c, d: 9 limbs per lane (the 8 x 32 operand of from_fe in the first 8); out: two 9-limb results per lane (the 8 x 32
// results of to_fe / fr9_to_canonical in the first 8).  fr9_chain runs `terms` accumulations acc = f9_norm(fr9_add(acc,
// fr9_mul(a, b))), folded every FR9_FOLD_PERIOD terms as the round-sum kernels fold.
#define F9_OPS(X)                                                                                                         \
    X(from_fe) X(to_fe) X(norm) X(fr9_mul) X(fr9_mul_add2) X(fr9_mul_sc_rp) X(fr9_mul_sc_k1) X(fr9_mul_sc_k2)                  \
    X(fr9_mul_sc_k3) X(fr9_add) X(fr9_sub_c2) X(fr9_sub_c3) X(fr9_sub_c5) X(fr9_to_canonical) X(fr9_fold) X(fr9_chain)        \
    X(fq9_mul) X(fq9_sqr) X(fq9_mul_x2) X(fq9_sqr_x2) X(fq9_mul_add2) X(fq9_sub_c2) X(fq9_sub_c3) X(fq9_sub_c7)               \
    X(fq9_is_zero_mod_p)
#define F9_ENUM_(n) F9OP_##n,
enum { F9_OPS(F9_ENUM_) F9_NOPS };
static const char* const F9_NAMES = F9_OPS(PRIMS_NAME_);

static __device__ __forceinline__ f9 f9_ld(const uint32_t* p) {
    f9 r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.l[k] = p[k];
    return r;
}
static __device__ __forceinline__ void f9_st(uint32_t* p, const f9& v) {
#pragma unroll
    for (int k = 0; k < 9; k++) p[k] = v.l[k];
}
static __device__ __forceinline__ f9 fe_as_f9(const fe& v) {  // 8 x 32 limbs in the first 8 slots of a 9-limb record
    f9 r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = v.l[k];
    r.l[8] = 0;
    return r;
}

__global__ void k_f9(int op, const uint32_t* pa, const uint32_t* pb, const uint32_t* pc, const uint32_t* pd, uint32_t* out,
                     uint32_t* ok, int terms, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f9 a = f9_ld(pa + 9 * i), b = f9_ld(pb + 9 * i), c = f9_ld(pc + 9 * i), d = f9_ld(pd + 9 * i);
    f9 r = fr9_zero(), r2 = fr9_zero();
    bool done = true;
    switch (op) {
        case F9OP_from_fe: {
            fe x;
#pragma unroll
            for (int k = 0; k < 8; k++) x.l[k] = a.l[k];
            r = f9_from_fe(x);
            break;
        }
        case F9OP_to_fe: r = fe_as_f9(f9_to_fe(a)); break;
        case F9OP_norm: r = f9_norm(a); break;
        case F9OP_fr9_mul: r = fr9_mul(a, b); break;
        case F9OP_fr9_mul_add2: r = fr9_mul_add2(a, b, c, d); break;
        case F9OP_fr9_mul_sc_rp: r = fr9_mul_sc(a, f9_const(FR9_RP)); break;
        case F9OP_fr9_mul_sc_k1: r = fr9_mul_sc(a, f9_const(FR9_K1)); break;
        case F9OP_fr9_mul_sc_k2: r = fr9_mul_sc(a, f9_const(FR9_K2)); break;
        case F9OP_fr9_mul_sc_k3: r = fr9_mul_sc(a, f9_const(FR9_K3)); break;
        case F9OP_fr9_add: r = fr9_add(a, b); break;
        case F9OP_fr9_sub_c2: r = f9_sub(a, FR9_C2, b); break;
        case F9OP_fr9_sub_c3: r = f9_sub(a, FR9_C3, b); break;
        case F9OP_fr9_sub_c5: r = f9_sub(a, FR9_C5, b); break;
        case F9OP_fr9_to_canonical: r = fe_as_f9(fr9_to_canonical(a)); break;
        case F9OP_fr9_fold: r = a; fr9_fold(r); break;
        case F9OP_fr9_chain:
            for (int it = 0; it < terms; it++) {
                if (it != 0 && (it & (FR9_FOLD_PERIOD - 1)) == 0) fr9_fold(r);
                r = f9_norm(fr9_add(r, fr9_mul(a, b)));
            }
            break;
        case F9OP_fq9_mul: r = f9_mul(a, b); break;
        case F9OP_fq9_sqr: r = f9_sqr(a); break;
        case F9OP_fq9_mul_x2: f9_mul_x2(a, b, c, d, r, r2); break;
        case F9OP_fq9_sqr_x2: f9_sqr_x2(a, c, r, r2); break;
        case F9OP_fq9_mul_add2: r = f9_mul_add2(a, b, c, d); break;
        case F9OP_fq9_sub_c2: r = f9_sub(a, F9_C2, b); break;
        case F9OP_fq9_sub_c3: r = f9_sub(a, F9_C3, b); break;
        case F9OP_fq9_sub_c7: r = f9_sub(a, F9_C7, b); break;
        case F9OP_fq9_is_zero_mod_p: r.l[0] = f9_is_zero_mod_p(a) ? 1u : 0u; break;
        default: done = false;
    }
    ok[i] = done ? 1u : 0u;
    f9_st(out + 18 * i, r);
    f9_st(out + 18 * i + 9, r2);
}

// One madd9 chain per lane: k affine points of 18 limbs each (qx then qy, 9 x 29, R-form); the first starts the accumulator
// (xyzz9_from_affine), the rest are added.  Per lane out: the 36 limbs of the accumulator, the 32 limbs of xyzz9_to_xyzz, and
// the index of the first addition madd9 refused (k when none did; the accumulator is the one before it).
static constexpr int MADD9_OUT = 36 + 32 + 1;
__global__ void k_madd9_chain(const uint32_t* pts, int k, uint32_t* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* q = pts + (size_t)18 * k * i;
    xyzz9 acc = xyzz9_from_affine(f9_ld(q), f9_ld(q + 9));
    int fail = k;
    for (int j = 1; j < k; j++)
        if (!madd9(acc, f9_ld(q + 18 * j), f9_ld(q + 18 * j + 9))) {
            fail = j;
            break;
        }
    uint32_t* o = out + (size_t)MADD9_OUT * i;
    f9_st(o, acc.x);
    f9_st(o + 9, acc.y);
    f9_st(o + 18, acc.zz);
    f9_st(o + 27, acc.zzz);
    const g1_xyzz s = xyzz9_to_xyzz(acc);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        o[36 + j] = s.x.l[j];
        o[44 + j] = s.y.l[j];
        o[52 + j] = s.zz.l[j];
        o[60 + j] = s.zzz.l[j];
    }
    o[68] = (uint32_t)fail;
}

// ------------------------------------------------------------------------------------------------ FrWide (poly.hip.hpp)
// Per lane 61 words: the 15 columns as (low word of lo, high word of lo, hi), then a and b.  wide_reduce = fr_wide_reduce of the
// columns as given; wide_mac adds ONE term a * b with fr_wide_mac first.  The caller keeps every column, with the carry that
// reaches it, below 2^96: the range fr_wide_reduce is written for.
#define WIDE_OPS(X) X(wide_reduce) X(wide_mac)
#define WIDE_ENUM_(n) WIDE_##n,
enum { WIDE_OPS(WIDE_ENUM_) WIDE_NOPS };
static const char* const WIDE_NAMES = WIDE_OPS(PRIMS_NAME_);
static constexpr int WIDE_IN = 15 * 3 + 8 + 8;

__global__ void k_wide(int op, const uint32_t* in, uint32_t* out, uint32_t* ok, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + (size_t)WIDE_IN * i;
    FrWide w;
#pragma unroll
    for (int k = 0; k < 15; k++) {
        w.lo[k] = (uint64_t)p[3 * k] | ((uint64_t)p[3 * k + 1] << 32);
        w.hi[k] = p[3 * k + 2];
    }
    fe a, b;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        a.l[k] = p[45 + k];
        b.l[k] = p[53 + k];
    }
    if (op == WIDE_wide_mac) fr_wide_mac(w, a, b);
    ok[i] = op == WIDE_wide_reduce || op == WIDE_wide_mac ? 1u : 0u;
    const fe r = fr_wide_reduce(w);
#pragma unroll
    for (int k = 0; k < 8; k++) out[8 * i + k] = r.l[k];
}

// ------------------------------------------------------------------------------------------------ host side of the wrappers
namespace {
struct Dev {
    void* p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    ~Dev() {
        if (p) (void)hipFree(p);
    }
};
#define PRIMS_TRY(x)                     \
    do {                                 \
        hipError_t e_ = (x);             \
        if (e_ != hipSuccess) return e_; \
    } while (0)
constexpr unsigned BLOCK = 256;
unsigned grid(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// upload nin inputs of n x in_words u32, launch, synchronise, download n x out_words u32 (and n flags when ok is given)
template <class Launch>
int run(size_t n, size_t in_words, const uint32_t* const* in, int nin, size_t out_words, uint32_t* out, uint32_t* ok,
        Launch launch) {
    Dev din[4], dout, dok;
    for (int k = 0; k < 4; k++) {
        PRIMS_TRY(din[k].alloc(k < nin ? n * in_words * 4 : 0));
        if (k < nin && n) PRIMS_TRY(hipMemcpy(din[k].p, in[k], n * in_words * 4, hipMemcpyHostToDevice));
    }
    PRIMS_TRY(dout.alloc(n * out_words * 4));
    PRIMS_TRY(dok.alloc(n * 4));
    if (n == 0) return hipSuccess;
    launch((const uint32_t*)din[0].p, (const uint32_t*)din[1].p, (const uint32_t*)din[2].p, (const uint32_t*)din[3].p,
           (uint32_t*)dout.p, (uint32_t*)dok.p);
    PRIMS_TRY(hipGetLastError());
    PRIMS_TRY(hipDeviceSynchronize());
    PRIMS_TRY(hipMemcpy(out, dout.p, n * out_words * 4, hipMemcpyDeviceToHost));
    if (ok) PRIMS_TRY(hipMemcpy(ok, dok.p, n * 4, hipMemcpyDeviceToHost));
    return hipSuccess;
}
}  // namespace

extern "C" {

const char* prims_ff_ops() { return FF_NAMES; }
const char* prims_g1_ops() { return G1_NAMES; }
const char* prims_f9_ops() { return F9_NAMES; }
const char* prims_wide_ops() { return WIDE_NAMES; }

// field 0 = Fr, 1 = Fq; a..d: n x 8 limbs; out: n x 16 limbs (o1, o2); ok: n flags (0 = op not on the device)
int prims_ff(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out,
             uint32_t* ok, size_t n) {
    const uint32_t* in[4] = {a, b, c, d};
    return run(n, 8, in, 4, 16, out, ok,
               [&](const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D, uint32_t* O, uint32_t* K) {
                   if (field == 0)
                       k_ff<Fr><<<grid(n), BLOCK>>>(op, (const fe*)A, (const fe*)B, (const fe*)C, (const fe*)D, (fe*)O, K, n);
                   else
                       k_ff<Fq><<<grid(n), BLOCK>>>(op, (const fe*)A, (const fe*)B, (const fe*)C, (const fe*)D, (fe*)O, K, n);
               });
}

// the same operations through the host path of the headers; -1 for an op the host does not have
int prims_ff_host(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out,
                  size_t n) {
    for (size_t i = 0; i < n; i++) {
        fe A, B, C, D, o1, o2;
        memcpy(A.l, a + 8 * i, 32);
        memcpy(B.l, b + 8 * i, 32);
        memcpy(C.l, c + 8 * i, 32);
        memcpy(D.l, d + 8 * i, 32);
        const bool done = field == 0 ? ff_apply<Fr>(op, A, B, C, D, o1, o2) : ff_apply<Fq>(op, A, B, C, D, o1, o2);
        if (!done) return -1;
        memcpy(out + 16 * i, o1.l, 32);
        memcpy(out + 16 * i + 8, o2.l, 32);
    }
    return 0;
}

// p, q, out: n x 32 limbs (g1_xyzz)
int prims_g1(int op, const uint32_t* p, const uint32_t* q, uint32_t* out, uint32_t* ok, size_t n) {
    const uint32_t* in[4] = {p, q, nullptr, nullptr};
    return run(n, 32, in, 2, 32, out, ok,
               [&](const uint32_t* A, const uint32_t* B, const uint32_t*, const uint32_t*, uint32_t* O, uint32_t* K) {
                   k_g1<<<grid(n), BLOCK>>>(op, (const g1_xyzz*)A, (const g1_xyzz*)B, (g1_xyzz*)O, K, n);
               });
}

// a..d: n x 9 limbs; out: n x 18 limbs
int prims_f9(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t* ok,
             int terms, size_t n) {
    const uint32_t* in[4] = {a, b, c, d};
    return run(n, 9, in, 4, 18, out, ok,
               [&](const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D, uint32_t* O, uint32_t* K) {
                   k_f9<<<grid(n), BLOCK>>>(op, A, B, C, D, O, K, terms, n);
               });
}

// pts: n x k x 18 limbs; out: n x 69 limbs
int prims_madd9_chain(const uint32_t* pts, int k, uint32_t* out, size_t n) {
    if (k < 1) return -1;
    const uint32_t* in[4] = {pts, nullptr, nullptr, nullptr};
    return run(n, (size_t)18 * k, in, 1, MADD9_OUT, out, nullptr,
               [&](const uint32_t* A, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t* O, uint32_t*) {
                   k_madd9_chain<<<grid(n), BLOCK>>>(A, k, O, n);
               });
}

// in: n x 61 words (k_wide); out: n x 8 limbs
int prims_wide(int op, const uint32_t* in, uint32_t* out, uint32_t* ok, size_t n) {
    const uint32_t* ins[4] = {in, nullptr, nullptr, nullptr};
    return run(n, WIDE_IN, ins, 1, 8, out, ok,
               [&](const uint32_t* A, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t* O, uint32_t* K) {
                   k_wide<<<grid(n), BLOCK>>>(op, A, O, K, n);
               });
}

// 1 when this process's Sha256 compresses with the SHA extensions: the condition Sha256::block evaluates once per process
int prims_sha_uses_shani() {
#if COZK_HAVE_SHANI
    return __builtin_cpu_supports("sha") && getenv("COZK_NO_SHANI") == nullptr;
#else
    return 0;
#endif
}

// SHA-256 of msg fed to update() in the given chunk sizes (which sum to the message length)
void prims_sha256(const uint8_t* msg, const size_t* chunks, size_t nchunks, uint8_t out[32]) {
    cozk::Sha256 s;
    for (size_t k = 0; k < nchunks; k++) {
        s.update(msg, chunks[k]);
        msg += chunks[k];
    }
    s.final(out);
}

// a Transcript("cozk") driven by a script of records: 'S' + 32 B (one Montgomery Fr: append_scalar), 'V' + u32 count + 32 B each
// (append_scalars), 'P' + u8 infinity + 64 B (Montgomery Fq x, y: append_point), 'C' (challenge_scalar: 8 limbs to out, in
// Montgomery form).  Returns the number of challenges written, or -1 on a malformed script.
int prims_transcript(const uint8_t* script, size_t len, uint32_t* out, size_t max_out) {
    cozk::Transcript t;
    size_t pos = 0;
    int nout = 0;
    auto get_fe = [&](fe& x) {
        memcpy(x.l, script + pos, 32);
        pos += 32;
    };
    while (pos < len) {
        const uint8_t op = script[pos++];
        if (op == 'S') {
            if (len - pos < 32) return -1;
            fe x;
            get_fe(x);
            t.append_scalar(x);
        } else if (op == 'V') {
            if (len - pos < 4) return -1;
            uint32_t k;
            memcpy(&k, script + pos, 4);
            pos += 4;
            if ((len - pos) / 32 < k) return -1;
            std::vector<fe> v(k);
            for (auto& x : v) get_fe(x);
            t.append_scalars(v);
        } else if (op == 'P') {
            if (len - pos < 65) return -1;
            const bool inf = script[pos++] != 0;
            g1_affine p;
            get_fe(p.x);
            get_fe(p.y);
            if (inf) p.x = p.y = Fq::zero();
            t.append_point(p);
        } else if (op == 'C') {
            if ((size_t)nout >= max_out) return -1;
            const fe c = t.challenge_scalar();
            memcpy(out + 8 * nout, c.l, 32);
            nout++;
        } else {
            return -1;
        }
    }
    return nout;
}

// verify_sumcheck_rounds on a fresh Transcript("cozk"): n_polys compressed polys, poly k holding lens[k] Montgomery Fr coefficients,
// concatenated in `coeffs`; `claim` in and out; the challenges drawn go to rs_out (room for n_polys of them) and one more challenge,
// drawn after the replay, to next_out (the transcript's state).  Returns 1 when the replay accepts the shape, 0 when not.
int prims_verify_sumcheck_rounds(const uint32_t* coeffs, const size_t* lens, size_t n_polys, size_t rounds, size_t degree, uint32_t claim[8],
                                 uint32_t* rs_out, uint32_t next_out[8]) {
    std::vector<std::vector<fe>> polys(n_polys);
    for (size_t k = 0; k < n_polys; k++) {
        polys[k].resize(lens[k]);
        for (auto& x : polys[k]) {
            memcpy(x.l, coeffs, 32);
            coeffs += 8;
        }
    }
    cozk::Transcript t;
    fe c;
    memcpy(c.l, claim, 32);
    std::vector<fe> rs;
    const bool ok = cozk::verify_sumcheck_rounds(polys, rounds, degree, c, t, rs);
    memcpy(claim, c.l, 32);
    for (size_t j = 0; j < rs.size(); j++) memcpy(rs_out + 8 * j, rs[j].l, 32);
    const fe nx = t.challenge_scalar();
    memcpy(next_out, nx.l, 32);
    return ok ? 1 : 0;
}

// eq_eval(a, b) (rev == 0) or eq_eval_rev(a, b) of n Montgomery Fr values each
void prims_eq_eval(const uint32_t* a, const uint32_t* b, size_t n, int rev, uint32_t out[8]) {
    std::vector<fe> va(n), vb(n);
    for (size_t i = 0; i < n; i++) {
        memcpy(va[i].l, a + 8 * i, 32);
        memcpy(vb[i].l, b + 8 * i, 32);
    }
    const fe e = rev ? cozk::eq_eval_rev(va, vb) : cozk::eq_eval(va, vb);
    memcpy(out, e.l, 32);
}

// mle_claim_padded of n Montgomery Fr outputs on a fresh Transcript("cozk"): the claim to claim_out, the point drawn to r_out.
// Returns the point's length, or -1 when it exceeds max_r.
int prims_mle_claim_padded(const uint32_t* outputs, size_t n, uint32_t claim_out[8], uint32_t* r_out, size_t max_r) {
    std::vector<fe> v(n), r;
    for (size_t i = 0; i < n; i++) memcpy(v[i].l, outputs + 8 * i, 32);
    cozk::Transcript t;
    const fe claim = cozk::mle_claim_padded(v, t, r);
    if (r.size() > max_r) return -1;
    memcpy(claim_out, claim.l, 32);
    for (size_t j = 0; j < r.size(); j++) memcpy(r_out + 8 * j, r[j].l, 32);
    return (int)r.size();
}

}  // extern "C"
