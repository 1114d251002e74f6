// The dealing step of Shamir secret sharing -- the ONE copy of the small-multiplier Horner step and of the PRF coefficients behind
// cozk_shamir_share_vec and every fused re-deal (shamir.hip's k_shamir_share over its sources; primary_group.inc's
// k_primary_group_deal, whose secret is a slot value of a collation program):
//   share of party p (1-based evaluation point) = v + sum_{c = 1..degree} coef_c p^c,   coef_c = PRF(keys[c - 1], counter + position)
// (mpc-types/src/protocols/shamir.rs:190-207 `share`, :166-175 `evaluate_poly`), and the Lagrange coefficients that open it.
#pragma once
#include "ff.hip.hpp"
#include "prf.hip.hpp"

// ------------------------------------------------------------------ the small-multiplier Horner step
// a * p + c mod r for canonical Montgomery residues a, c and a PLAIN integer p <= 32 (the evaluation point of party p):
// the Montgomery residue of x * p is (x R) * p, so no Montgomery product is needed -- 8 multiply-adds give the 9-word value
//   t = a p + c <= 32 (r - 1) + (r - 1) < 33 r < 2^260            (r < 2^254)
// and one quotient estimate brings it back below r.  With T = floor(t / 2^228) (< 2^32) and D = floor(r / 2^228) + 1:
//   q = floor(T / D) <= (t / 2^228) / (r / 2^228) = t / r, so q <= Q = floor(t / r) and t - q r >= 0;
//   T > t / 2^228 - 1 and D <= r / 2^228 + 1 give t / r - T / D < (t / r + 1) / (r / 2^228) < 34 / (5 * 10^7) < 10^-6, so
//   q > t / r - 1 - 10^-6, i.e. q >= Q - 1 and t - q r < 2 r < 2^255: it fits 8 words,
// and ONE conditional subtraction (reduce_once) makes it canonical.  16 multiply-adds and 2 borrow chains instead of the
// 128 multiply-adds of a Montgomery product.  Input bound: a, c < r and 0 <= p <= 32; output < r.
static __device__ __forceinline__ fe fr_mul_small_add(const fe& a, uint32_t p, const fe& c) {
    uint32_t t[9];
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t m = (uint64_t)a.l[i] * p + c.l[i] + carry;  // < 2^32 * 32 + 2^32 + 2^38
        t[i] = (uint32_t)m;
        carry = m >> 32;
    }
    t[8] = (uint32_t)carry;
    const uint32_t T = (t[8] << 28) | (t[7] >> 4);          // t >> 228 (t[7] holds bits 224..255); t < 2^260, so t[8] < 16
    const uint32_t q = T / ((FrParams::MOD[7] >> 4) + 1u);  // <= 33
    fe s;
    uint64_t mc = 0, borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t m = (uint64_t)q * FrParams::MOD[i] + mc;
        mc = m >> 32;
        uint64_t d = (uint64_t)t[i] - (uint32_t)m - borrow;
        s.l[i] = (uint32_t)d;
        borrow = (d >> 63) & 1;
    }
    return Fr::reduce_once(s);  // word 8 of t - q r is zero (t - q r < 2^255)
}

// prf_fr (prf.hip.hpp) with the two halves of the block read through constant indices: the same value, and fifteen inlined
// copies of it keep their block words in registers
static __device__ __forceinline__ fe shamir_prf_fr(const prf_key key, uint64_t j) {
    for (uint32_t attempt = 0;; attempt++) {
        uint32_t w[16];
        chacha12_block(key, j, attempt, w);
        fe lo, hi;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            lo.l[i] = w[i];
            hi.l[i] = w[8 + i];
        }
        lo.l[7] &= 0x3fffffffu;
        hi.l[7] &= 0x3fffffffu;
        const bool ok_lo = !Fr::geq_mod(lo), ok_hi = !Fr::geq_mod(hi);
        fe v;
#pragma unroll
        for (int i = 0; i < 8; i++) v.l[i] = ok_lo ? lo.l[i] : hi.l[i];
        if (ok_lo || ok_hi) return Fr::to_mont(v);
    }
}

// The coefficients of one element, leading one first -- the order Horner consumes them in -- and the chain itself, as functions, for
// kernels that deal a value they compute themselves (k_shamir_share spells the same steps out over its sources).  DEG = 1..: the degree
// at compile time, MAXD == DEG, c[DEG - 1 - k] = coefficient k + 1.  DEG = 0: the degree (<= MAXD) at run time; the coefficients are
// then produced by ONE rolled loop (one copy of the ChaCha block, the key picked by a wave-uniform index) and pushed into c[] as a
// shift register, so that c[] is only ever indexed with constants and stays in registers: after the loop c[j] = coefficient deg - j.
// coef(k) = coefficient k + 1 of this element.
template <int DEG, int MAXD, class Coef>
static __device__ __forceinline__ void shamir_deal_coefs(fe (&c)[MAXD], int deg, Coef coef) {
    if (DEG) {
#pragma unroll
        for (int k = 0; k < MAXD; k++) c[MAXD - 1 - k] = coef(k);
    } else {
#pragma unroll
        for (int k = 0; k < MAXD; k++) c[k] = Fr::zero();
#pragma unroll 1
        for (int k = 0; k < deg; k++) {
            const fe next = coef(k);
#pragma unroll
            for (int m = MAXD - 1; m > 0; m--) c[m] = c[m - 1];
            c[0] = next;
        }
    }
}

// the share of the party at evaluation point p (1..32) of the secret v under the coefficients of shamir_deal_coefs: canonical
template <int MAXD>
static __device__ __forceinline__ fe shamir_deal_eval(const fe (&c)[MAXD], int deg, uint32_t p, const fe& v) {
    fe acc = c[0];
#pragma unroll
    for (int m = 1; m < MAXD; m++)
        if (m < deg) acc = fr_mul_small_add(acc, p, c[m]);
    return fr_mul_small_add(acc, p, v);
}

// lagrange_from_coeff (shamir.rs:273-291): lambda_i = prod_{j != i} x_j / (x_j - x_i), Montgomery form
static inline void lagrange_host(const uint32_t* points, size_t k, fe* out) {
    for (size_t i = 0; i < k; i++) {
        fe num = Fr::one(), den = Fr::one();
        const fe xi = Fr::from_u64(points[i]);
        for (size_t j = 0; j < k; j++) {
            if (j == i) continue;
            const fe xj = Fr::from_u64(points[j]);
            num = Fr::mul(num, xj);
            den = Fr::mul(den, Fr::sub(xj, xi));
        }
        out[i] = Fr::mul(num, Fr::inv(den));
    }
}
