// The leaves of the read-write memory check's grand-product circuits from the compact columns of cozk_rw_memory_witness
// (cozk_rw_memory_leaves, cozk_rw_memory_init_final_leaves; the layout is in cozk.h), with h(a, v, t) = a + v gamma + t gamma^2 - tau:
//
//   k_rw_leaves     a thread per (slot, step): the read leaf h(addr, v_read, t_read) and the write leaf h(addr, w, j)
//   k_rw_if_leaves  a thread per address: the init leaf h(a, v_init, 0) and the final leaf h(a, v_final, t_final)
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

}  // extern "C"
