// The leaves of the read-write memory check's grand-product circuits from the compact columns of cozk_rw_memory_witness
// (cozk_rw_memory_leaves, cozk_rw_memory_init_final_leaves; the layout is in cozk.h), with h(a, v, t) = a + v gamma + t gamma^2 - tau:
//
//   k_rw_leaves     a thread per (slot, step): the read leaf h(addr, v_read, t_read) and the write leaf h(addr, w, j)
//   k_rw_if_leaves  a thread per address: the init leaf h(a, v_init, 0) and the final leaf h(a, v_final, t_final)
//
// and the same circuits with the values as polynomials, plain or Rep3 shares (cozk_rw_memory_shared_leaves,
// cozk_rw_memory_shared_init_final_leaves; Rep3ReadWriteMemoryProver::compute_leaves, co-jolt/src/jolt/vm/read_write_memory/worker.rs:196-344:
// every leaf is add_public(mul_public(v_share, gamma), t gamma^2 + a - tau, party_id)):
//
//   k_rws_leaves<NC>     a thread per (slot, step), NC components per leaf
//   k_rws_if_leaves<NC>  a thread per address
//
// The step number j and the address a exist only in registers.  Every leaf is the canonical Montgomery word of its value, so it
// equals bit for bit what cozk_fingerprint_leaves gives for the same columns.
//
// The arithmetic: every column entry is below 2^32 and ONE = R mod r, G1 = gamma R mod r, G2 = gamma^2 R mod r, C = (r - tau) R mod r
// are Montgomery forms, so the leaf is the residue of the exact integer
//     S = a ONE + v G1 + t G2 + C  <=  3 (2^32 - 1)(r - 1) + (r - 1)  <  3 * 2^32 r  <  2^288      (r < 2^254)
// in RL_LIMBS = 9 limbs: 8 multiply-adds of 32 x 32 + 64 bits per term (no overflow: (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1), every
// carry walked into limb 8.  rl_reduce takes S mod r by a short Barrett quotient: with S1 = floor(S / 2^253) < 2^35 and
// MU = floor(2^288 / r) < 2^35,
//     qh = floor(S1 MU / 2^35)   has   q - 2 <= qh <= q = floor(S / r) < 3 * 2^32
// (S1 > S / 2^253 - 1, MU > 2^288 / r - 1, S < 2^288, r >= 2^253: qh > S / r - 3), so T = S - qh r lies in [0, 3 r), below 2^256: it
// is computed on the low 8 limbs alone (qh r mod 2^256 by 8 + 7 multiply-adds, qh = qh_hi 2^32 + qh_lo with qh_hi < 8) and two
// conditional subtractions of r leave the canonical word.  tests/rw_proof_ref.py (leaf_word_model) restates these words with the
// bounds as asserts.
//
// The shared kernels keep the value term apart: the public part a ONE + t G2 + C is the same exact sum with two terms (S < 2 * 2^32 r),
// reduced once per leaf, and each share component is one Fr::mul by gamma and one Fr::add of the public part where the component
// carries it (party 0's a, party 1's b; a plain prover's only component).  Party 2 computes no public part, and a public polynomial
// in a REP3 call is read only by the party whose component carries it: both branches are uniform over the launch.  A slot that only
// reads uses one v gamma product per component for both of its leaves.  Every word is canonical, so the leaves equal bit for bit what
// the composition of cozk_fingerprint_leaves calls gives (rw_memory_leaves_composed with polynomial terms).
//
// Measured and not kept: a full Fr::mul per term, as k_ts_range_leaves has it (five products per (slot, step), 128
// multiply-adds each) took 2.5 times as long at 2^20 steps with 4 slots; a thread per step over all slots, which makes j gamma^2
// once per step, 9 % longer (82 VGPRs against 60, a quarter of the threads).
#include "common.hpp"

static constexpr int RL_PT = 256;
static constexpr int RL_LIMBS = 9;
static constexpr uint64_t RL_MU = 0x54a474626ull;  // floor(2^288 / r), 35 bits
static constexpr size_t RL_MAX_SLOTS = COZK_RW_MEMORY_MAX_SLOTS;
#define RL_STR_(x) #x
#define RL_STR(x) RL_STR_(x)

struct RwLeafCols {
    const void* addr[RL_MAX_SLOTS];
    const uint32_t *v_read[RL_MAX_SLOTS], *t_read[RL_MAX_SLOTS], *v_written[RL_MAX_SLOTS];  // v_written null: w = v_read
    uint8_t addr_u8[RL_MAX_SLOTS];
};
// the coefficients of the address, value and time terms and the constant: ONE, G1, G2, C
struct RwLeafCoeffs {
    fe a, v, t, c;
};
struct RlAcc {
    uint32_t s[RL_LIMBS];
};

static __device__ __forceinline__ RlAcc rl_start(const fe& c) {
    RlAcc r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.s[k] = c.l[k];
    r.s[8] = 0;
    return r;
}

// acc += coeff * v
static __device__ __forceinline__ void rl_term(RlAcc& acc, const fe& coeff, uint32_t v) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)coeff.l[k] * v + acc.s[k] + carry;  // <= 2^64 - 1
        acc.s[k] = (uint32_t)t;
        carry = t >> 32;
    }
    acc.s[8] += (uint32_t)carry;  // the sum stays below 2^288
}

static __device__ __forceinline__ fe rl_reduce(const RlAcc& acc) {
    const uint32_t* s = acc.s;
    const uint64_t s1 = ((uint64_t)s[8] << 3) | (s[7] >> 29);                          // floor(S / 2^253) < 2^35
    const uint64_t q = (__umul64hi(s1, RL_MU) << 29) | ((s1 * RL_MU) >> 35);           // floor(S1 MU / 2^35), the product < 2^70
    const uint32_t q_lo = (uint32_t)q, q_hi = (uint32_t)(q >> 32);                     // q_hi < 8
    uint32_t p[8];                                                                     // q r mod 2^256
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)FrParams::MOD[k] * q_lo + carry;
        p[k] = (uint32_t)t;
        carry = t >> 32;
    }
    carry = 0;
#pragma unroll
    for (int k = 1; k < 8; k++) {
        const uint64_t t = (uint64_t)FrParams::MOD[k - 1] * q_hi + p[k] + carry;
        p[k] = (uint32_t)t;
        carry = t >> 32;
    }
    fe d;  // T = S - q r in [0, 3 r): below 2^256, so the low 8 limbs are all of it
    uint64_t borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)s[k] - p[k] - borrow;
        d.l[k] = (uint32_t)t;
        borrow = (t >> 63) & 1;
    }
    return Fr::reduce_once(Fr::reduce_once(d));
}

static __device__ __forceinline__ uint32_t rl_addr(const RwLeafCols& a, uint32_t s, size_t j) {
    return a.addr_u8[s] ? (uint32_t)((const uint8_t*)a.addr[s])[j] : ((const uint32_t*)a.addr[s])[j];
}

// out[(2 s) n + j] = h(addr, v_read, t_read), out[(2 s + 1) n + j] = h(addr, w, j); blockIdx.y is the slot
__global__ void __launch_bounds__(RL_PT) k_rw_leaves(RwLeafCols a, size_t n, RwLeafCoeffs cf, fe* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * RL_PT + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = blockIdx.y;
    const uint32_t v = a.v_read[s][j];
    const uint32_t w = a.v_written[s] ? a.v_written[s][j] : v;  // uniform over the workgroup
    RlAcc base = rl_start(cf.c);
    rl_term(base, cf.a, rl_addr(a, s, j));
    RlAcc rd = base;
    rl_term(rd, cf.v, v);
    rl_term(rd, cf.t, a.t_read[s][j]);
    fe_store(out + (size_t)(2 * s) * n + j, rl_reduce(rd));
    rl_term(base, cf.v, w);
    rl_term(base, cf.t, (uint32_t)j);
    fe_store(out + (size_t)(2 * s + 1) * n + j, rl_reduce(base));
}

// out[a] = h(a, v_init[a], 0), out[MEM + a] = h(a, v_final[a], t_final[a])
__global__ void __launch_bounds__(RL_PT) k_rw_if_leaves(const uint32_t* __restrict__ v_init, const uint32_t* __restrict__ v_final, const uint32_t* __restrict__ t_final,
                                                        size_t MEM, RwLeafCoeffs cf, fe* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RL_PT + threadIdx.x;
    if (i >= MEM) return;
    RlAcc base = rl_start(cf.c);
    rl_term(base, cf.a, (uint32_t)i);
    RlAcc in = base;
    rl_term(in, cf.v, v_init[i]);
    fe_store(out + i, rl_reduce(in));
    rl_term(base, cf.v, v_final[i]);
    rl_term(base, cf.t, t_final[i]);
    fe_store(out + MEM + i, rl_reduce(base));
}

// ---- the values as polynomials: component pointers, null where the component takes nothing from the polynomial
struct RwSharedCols {
    const void* addr[RL_MAX_SLOTS];
    const uint32_t* t_read[RL_MAX_SLOTS];
    const fe* v_read[2][RL_MAX_SLOTS];     // [component][slot]
    const fe* v_written[2][RL_MAX_SLOTS];  // read only where writes[s]
    uint8_t addr_u8[RL_MAX_SLOTS], writes[RL_MAX_SLOTS];
};
struct RwSharedIfCols {
    const fe *v_init[2], *v_final[2];
    const uint32_t* t_final;
};
static __device__ __forceinline__ uint32_t rl_addr(const RwSharedCols& a, uint32_t s, size_t j) {
    return a.addr_u8[s] ? (uint32_t)((const uint8_t*)a.addr[s])[j] : ((const uint32_t*)a.addr[s])[j];
}
// gamma v, zero where the component takes nothing
static __device__ __forceinline__ fe rl_share_term(const fe* p, size_t j, const fe& gamma) { return p ? Fr::mul(fe_load(p + j), gamma) : Fr::zero(); }

// o[c][(2 s) n + j] = gamma v_read_c + [pub[c]] (addr + t_read gamma^2 - tau), o[c][(2 s + 1) n + j] = gamma w_c + [pub[c]] (addr + j gamma^2 - tau);
// blockIdx.y is the slot.  cf.v is gamma itself (the share term is a field product), cf.a, cf.t, cf.c as in k_rw_leaves.
template <int NC>
__global__ void __launch_bounds__(RL_PT) k_rws_leaves(RwSharedCols a, size_t n, RwLeafCoeffs cf, int pub_a, int pub_b, fe* __restrict__ oa, fe* __restrict__ ob) {
    const size_t j = (size_t)blockIdx.x * RL_PT + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = blockIdx.y;
    fe pub_r = Fr::zero(), pub_w = Fr::zero();
    if (pub_a || pub_b) {  // uniform over the launch
        RlAcc base = rl_start(cf.c);
        rl_term(base, cf.a, rl_addr(a, s, j));
        RlAcc rd = base;
        rl_term(rd, cf.t, a.t_read[s][j]);
        pub_r = rl_reduce(rd);
        rl_term(base, cf.t, (uint32_t)j);
        pub_w = rl_reduce(base);
    }
    const size_t ir = (size_t)(2 * s) * n + j, iw = ir + n;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int pub = c == 0 ? pub_a : pub_b;
        fe* o = c == 0 ? oa : ob;
        const fe x = rl_share_term(a.v_read[c][s], j, cf.v);
        const fe y = a.writes[s] ? rl_share_term(a.v_written[c][s], j, cf.v) : x;  // uniform over the workgroup
        fe_store(o + ir, pub ? Fr::add(x, pub_r) : x);
        fe_store(o + iw, pub ? Fr::add(y, pub_w) : y);
    }
}

// o[c][i] = gamma v_init_c + [pub[c]] (i - tau), o[c][MEM + i] = gamma v_final_c + [pub[c]] (i + t_final gamma^2 - tau)
template <int NC>
__global__ void __launch_bounds__(RL_PT) k_rws_if_leaves(RwSharedIfCols a, size_t MEM, RwLeafCoeffs cf, int pub_a, int pub_b, fe* __restrict__ oa, fe* __restrict__ ob) {
    const size_t i = (size_t)blockIdx.x * RL_PT + threadIdx.x;
    if (i >= MEM) return;
    fe pub_i = Fr::zero(), pub_f = Fr::zero();
    if (pub_a || pub_b) {  // uniform over the launch
        RlAcc base = rl_start(cf.c);
        rl_term(base, cf.a, (uint32_t)i);
        pub_i = rl_reduce(base);
        rl_term(base, cf.t, a.t_final[i]);
        pub_f = rl_reduce(base);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int pub = c == 0 ? pub_a : pub_b;
        fe* o = c == 0 ? oa : ob;
        const fe x = rl_share_term(a.v_init[c], i, cf.v), y = rl_share_term(a.v_final[c], i, cf.v);
        fe_store(o + i, pub ? Fr::add(x, pub_i) : x);
        fe_store(o + MEM + i, pub ? Fr::add(y, pub_f) : y);
    }
}

namespace {

fe rl_fe(const uint64_t w[4]) {
    fe x;
    for (int i = 0; i < 4; i++) x.l[2 * i] = (uint32_t)w[i], x.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
    return x;
}
RwLeafCoeffs rl_coeffs(const uint64_t gamma[4], const uint64_t tau[4]) {
    const fe g = rl_fe(gamma);
    return RwLeafCoeffs{Fr::one(), g, Fr::mul(g, g), Fr::neg(rl_fe(tau))};
}

// ---- the shared calls' argument checks
void rl_shared_outputs(const std::string& w, int mode, int party_id, const cozk_vec* out_a, const cozk_vec* out_b, size_t offset, size_t circuits, size_t len,
                       const std::string& room) {
    COZK_REQUIRE(mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, w + ": mode is COZK_MODE_PLAIN or COZK_MODE_REP3");
    COZK_REQUIRE(party_id >= 0 && party_id < 3, w + ": 0 <= party_id < 3");
    COZK_REQUIRE(out_a && out_a->kind == COZK_SCALAR_FR && offset <= out_a->n && (out_a->n - offset) / circuits >= len,
                 w + ": out_a is an FR vector with room for " + room + " entries from offset");
    if (mode == COZK_MODE_REP3)
        COZK_REQUIRE(out_b && out_b != out_a && out_b->d != out_a->d && out_b->kind == COZK_SCALAR_FR && offset <= out_b->n && (out_b->n - offset) / circuits >= len,
                     w + ": REP3 needs out_b, another FR vector with room for " + room + " entries from offset");
    else
        COZK_REQUIRE(!out_b, w + ": out_b is NULL for PLAIN");
}
// The component pointers of one value polynomial (what cozk_fingerprint_leaves does with a polynomial term): a shared one gives both
// components; a public one in a REP3 call enters through add_public, party 0's a and party 1's b; a plain call reads component a.
// The views go into `views`, which the caller frees: the polynomial keeps its buffers.
struct RlViews {
    std::vector<cozk_vec*> v;
    ~RlViews() {
        for (cozk_vec* w : v) cozk_vec_free(w);
    }
};
void rl_poly_components(cozk_ctx* ctx, const std::string& w, const cozk_poly* p, int mode, int party_id, RlViews& views, const fe*& a, const fe*& b) {
    const fe* c[2] = {nullptr, nullptr};
    const int pm = cozk_poly_mode(p);
    for (int k = 0; k < (pm == COZK_MODE_REP3 ? 2 : 1); k++) {
        cozk_vec* view = nullptr;
        if (cozk_poly_share_view(ctx, p, k, &view) != COZK_OK) throw CozkError(COZK_ERR_INVALID_ARG, w + ": " + ctx->last_error);
        views.v.push_back(view);
        c[k] = (const fe*)view->d;
    }
    if (pm == COZK_MODE_REP3 || mode == COZK_MODE_PLAIN) {
        a = c[0], b = c[1];
    } else {
        a = party_id == 0 ? c[0] : nullptr;
        b = party_id == 1 ? c[0] : nullptr;
    }
}

}  // namespace

extern "C" {

int cozk_rw_memory_leaves(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_vec* const* v_read, const cozk_vec* const* t_read,
                          const cozk_vec* const* v_written, size_t n_slots, const uint64_t gamma[4], const uint64_t tau[4], cozk_vec* out, size_t offset) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && addr && v_read && t_read && gamma && tau && out, "rw_memory_leaves: bad argument");
        COZK_REQUIRE(n_slots >= 1 && n_slots <= RL_MAX_SLOTS, "rw_memory_leaves: 1 <= n_slots <= " RL_STR(COZK_RW_MEMORY_MAX_SLOTS));
        RwLeafCols h{};
        for (size_t s = 0; s < n_slots; s++) {
            const cozk_vec *a = addr[s], *vr = v_read[s], *tr = t_read[s], *vw = v_written ? v_written[s] : nullptr;
            COZK_REQUIRE(a && (a->kind == COZK_SCALAR_U8 || a->kind == COZK_SCALAR_U32), "rw_memory_leaves: addr[s] is a U8 or U32 vector");
            COZK_REQUIRE(vr && tr && vr->kind == COZK_SCALAR_U32 && tr->kind == COZK_SCALAR_U32 && (!vw || vw->kind == COZK_SCALAR_U32),
                         "rw_memory_leaves: v_read[s], t_read[s] and v_written[s] are U32 vectors");
            COZK_REQUIRE(a->n == addr[0]->n && vr->n == a->n && tr->n == a->n && (!vw || vw->n == a->n), "rw_memory_leaves: every column has n entries");
            h.addr[s] = a->d;
            h.addr_u8[s] = a->kind == COZK_SCALAR_U8;
            h.v_read[s] = (const uint32_t*)vr->d;
            h.t_read[s] = (const uint32_t*)tr->d;
            h.v_written[s] = vw ? (const uint32_t*)vw->d : nullptr;
        }
        const size_t n = addr[0]->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), "rw_memory_leaves: 1 <= n < 2^32");
        COZK_REQUIRE(out->kind == COZK_SCALAR_FR && offset <= out->n && (out->n - offset) / (2 * n_slots) >= n,
                     "rw_memory_leaves: out is an FR vector with room for 2 n_slots n entries from offset");
        const dim3 grid((unsigned)((n + RL_PT - 1) / RL_PT), (unsigned)n_slots);
        k_rw_leaves<<<grid, RL_PT, 0, ctx->stream>>>(h, n, rl_coeffs(gamma, tau), (fe*)out->d + offset);
        HIP_TRY(hipGetLastError());
    });
}

int cozk_rw_memory_init_final_leaves(cozk_ctx* ctx, const cozk_vec* v_init, const cozk_vec* v_final, const cozk_vec* t_final, const uint64_t gamma[4],
                                     const uint64_t tau[4], cozk_vec* out, size_t offset) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && v_init && v_final && t_final && gamma && tau && out, "rw_memory_init_final_leaves: bad argument");
        COZK_REQUIRE(v_init->kind == COZK_SCALAR_U32 && v_final->kind == COZK_SCALAR_U32 && t_final->kind == COZK_SCALAR_U32,
                     "rw_memory_init_final_leaves: v_init, v_final and t_final are U32 vectors");
        const size_t MEM = v_init->n;
        COZK_REQUIRE(v_final->n == MEM && t_final->n == MEM, "rw_memory_init_final_leaves: every column has MEM entries");
        COZK_REQUIRE(MEM >= 1 && MEM < ((size_t)1 << 32), "rw_memory_init_final_leaves: 1 <= MEM < 2^32");
        COZK_REQUIRE(out->kind == COZK_SCALAR_FR && offset <= out->n && (out->n - offset) / 2 >= MEM,
                     "rw_memory_init_final_leaves: out is an FR vector with room for 2 MEM entries from offset");
        k_rw_if_leaves<<<(unsigned)((MEM + RL_PT - 1) / RL_PT), RL_PT, 0, ctx->stream>>>((const uint32_t*)v_init->d, (const uint32_t*)v_final->d,
                                                                                         (const uint32_t*)t_final->d, MEM, rl_coeffs(gamma, tau), (fe*)out->d + offset);
        HIP_TRY(hipGetLastError());
    });
}

int cozk_rw_memory_shared_leaves(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_poly* const* v_read, const cozk_vec* const* t_read,
                                 const cozk_poly* const* v_written, size_t n_slots, const uint64_t gamma[4], const uint64_t tau[4], int mode, int party_id,
                                 cozk_vec* out_a, cozk_vec* out_b, size_t offset) {
    return cozk_guard(ctx, [&] {
        const std::string w = "rw_memory_shared_leaves";
        COZK_REQUIRE(ctx && addr && v_read && t_read && gamma && tau, w + ": bad argument");
        COZK_REQUIRE(n_slots >= 1 && n_slots <= RL_MAX_SLOTS, w + ": 1 <= n_slots <= " RL_STR(COZK_RW_MEMORY_MAX_SLOTS));
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, w + ": mode is COZK_MODE_PLAIN or COZK_MODE_REP3");
        for (size_t s = 0; s < n_slots; s++) {
            const cozk_vec *a = addr[s], *tr = t_read[s];
            const cozk_poly *vr = v_read[s], *vw = v_written ? v_written[s] : nullptr;
            COZK_REQUIRE(a && (a->kind == COZK_SCALAR_U8 || a->kind == COZK_SCALAR_U32), w + ": addr[s] is a U8 or U32 vector");
            COZK_REQUIRE(tr && tr->kind == COZK_SCALAR_U32, w + ": t_read[s] is a U32 vector");
            COZK_REQUIRE(addr[0] && a->n == addr[0]->n && tr->n == a->n, w + ": every column has n entries");
            COZK_REQUIRE(vr, w + ": v_read[s] is a polynomial");
            COZK_REQUIRE(cozk_poly_len(vr) >= a->n && (!vw || cozk_poly_len(vw) >= a->n), w + ": a value polynomial is shorter than n");
            COZK_REQUIRE(mode == COZK_MODE_REP3 || (cozk_poly_mode(vr) == COZK_MODE_PLAIN && (!vw || cozk_poly_mode(vw) == COZK_MODE_PLAIN)),
                         w + ": a shared value polynomial needs mode COZK_MODE_REP3");
        }
        const size_t n = addr[0]->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), w + ": 1 <= n < 2^32");
        rl_shared_outputs(w, mode, party_id, out_a, out_b, offset, 2 * n_slots, n, "2 n_slots n");
        RwSharedCols h{};
        RlViews views;
        for (size_t s = 0; s < n_slots; s++) {
            h.addr[s] = addr[s]->d;
            h.addr_u8[s] = addr[s]->kind == COZK_SCALAR_U8;
            h.t_read[s] = (const uint32_t*)t_read[s]->d;
            rl_poly_components(ctx, w, v_read[s], mode, party_id, views, h.v_read[0][s], h.v_read[1][s]);
            if (v_written && v_written[s]) {
                h.writes[s] = 1;
                rl_poly_components(ctx, w, v_written[s], mode, party_id, views, h.v_written[0][s], h.v_written[1][s]);
            }
        }
        const dim3 grid((unsigned)((n + RL_PT - 1) / RL_PT), (unsigned)n_slots);
        const RwLeafCoeffs cf = rl_coeffs(gamma, tau);  // cf.v = gamma in Montgomery form: the factor of the share products
        fe* oa = (fe*)out_a->d + offset;
        if (mode == COZK_MODE_REP3) k_rws_leaves<2><<<grid, RL_PT, 0, ctx->stream>>>(h, n, cf, party_id == 0, party_id == 1, oa, (fe*)out_b->d + offset);
        else k_rws_leaves<1><<<grid, RL_PT, 0, ctx->stream>>>(h, n, cf, 1, 0, oa, nullptr);
        HIP_TRY(hipGetLastError());
    });
}

int cozk_rw_memory_shared_init_final_leaves(cozk_ctx* ctx, const cozk_poly* v_init, const cozk_poly* v_final, const cozk_vec* t_final, const uint64_t gamma[4],
                                            const uint64_t tau[4], int mode, int party_id, cozk_vec* out_a, cozk_vec* out_b, size_t offset) {
    return cozk_guard(ctx, [&] {
        const std::string w = "rw_memory_shared_init_final_leaves";
        COZK_REQUIRE(ctx && v_init && v_final && t_final && gamma && tau, w + ": bad argument");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, w + ": mode is COZK_MODE_PLAIN or COZK_MODE_REP3");
        COZK_REQUIRE(t_final->kind == COZK_SCALAR_U32, w + ": t_final is a U32 vector");
        const size_t MEM = t_final->n;
        COZK_REQUIRE(MEM >= 1 && MEM < ((size_t)1 << 32), w + ": 1 <= MEM < 2^32");
        COZK_REQUIRE(cozk_poly_len(v_init) >= MEM && cozk_poly_len(v_final) >= MEM, w + ": a value polynomial is shorter than MEM");
        COZK_REQUIRE(mode == COZK_MODE_REP3 || (cozk_poly_mode(v_init) == COZK_MODE_PLAIN && cozk_poly_mode(v_final) == COZK_MODE_PLAIN),
                     w + ": a shared value polynomial needs mode COZK_MODE_REP3");
        rl_shared_outputs(w, mode, party_id, out_a, out_b, offset, 2, MEM, "2 MEM");
        RwSharedIfCols h{};
        RlViews views;
        h.t_final = (const uint32_t*)t_final->d;
        rl_poly_components(ctx, w, v_init, mode, party_id, views, h.v_init[0], h.v_init[1]);
        rl_poly_components(ctx, w, v_final, mode, party_id, views, h.v_final[0], h.v_final[1]);
        const unsigned grid = (unsigned)((MEM + RL_PT - 1) / RL_PT);
        const RwLeafCoeffs cf = rl_coeffs(gamma, tau);  // cf.v = gamma in Montgomery form: the factor of the share products
        fe* oa = (fe*)out_a->d + offset;
        if (mode == COZK_MODE_REP3) k_rws_if_leaves<2><<<grid, RL_PT, 0, ctx->stream>>>(h, MEM, cf, party_id == 0, party_id == 1, oa, (fe*)out_b->d + offset);
        else k_rws_if_leaves<1><<<grid, RL_PT, 0, ctx->stream>>>(h, MEM, cf, 1, 0, oa, nullptr);
        HIP_TRY(hipGetLastError());
    });
}

}  // extern "C"
