// The word arithmetic of the bytecode leaf kernels (bytecode_leaves.hip has the bounds): the exact 11-limb sum of 64 x 256-bit products
// and its reduction by a 69-bit Barrett quotient, and on top of them the public part of a read leaf and the init / final pair of a table
// row.  Host and device: the kernels call bc_read_public and bc_init_final per entry, and the stand-alone host program
// tests/native/bytecode_leaf_check.hip runs the same functions on a CPU.
#pragma once
#include "ff.hip.hpp"

static constexpr int BC_LIMBS = 11;
struct BcParams {
    static constexpr uint32_t MU[3] = {0x8e8129eau, 0x291d1898u, 0x15u};  // floor(2^322 / r), 69 bits
};

// G_1 .. G_7, ONE, NEG_ONE and C
struct BcCoeffs {
    fe g[7], one, neg_one, c;
};
struct BcAcc {
    uint32_t s[BC_LIMBS];
};

static FF_HD BcAcc bc_start(const fe& c) {
    BcAcc r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.s[k] = c.l[k];
#pragma unroll
    for (int k = 8; k < BC_LIMBS; k++) r.s[k] = 0;
    return r;
}

// acc += coeff * v * 2^(32 OFF), exact
template <int OFF>
static FF_HD void bc_mac(BcAcc& acc, const fe& coeff, uint32_t v) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)coeff.l[k] * v + acc.s[OFF + k] + carry;  // <= 2^64 - 1
        acc.s[OFF + k] = (uint32_t)t;
        carry = t >> 32;
    }
#pragma unroll
    for (int k = OFF + 8; k < BC_LIMBS; k++) {
        const uint64_t t = (uint64_t)acc.s[k] + carry;
        acc.s[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
// wide: the entry has a high half (a U64 / I64 column; uniform over the launch)
static FF_HD void bc_term(BcAcc& acc, const fe& coeff, uint64_t v, bool wide) {
    bc_mac<0>(acc, coeff, (uint32_t)v);
    if (wide) bc_mac<1>(acc, coeff, (uint32_t)(v >> 32));
}

static FF_HD fe bc_reduce(const BcAcc& acc) {
    const uint32_t* s = acc.s;
    // S1 = floor(S / 2^253) < 2^69: bit 253 is bit 29 of limb 7, and limb 10 is below 4
    const uint32_t x[3] = {(s[7] >> 29) | (s[8] << 3), (s[8] >> 29) | (s[9] << 3), (s[9] >> 29) | (s[10] << 3)};
    uint32_t p[6] = {0, 0, 0, 0, 0, 0};  // S1 MU < 2^138
#pragma unroll
    for (int i = 0; i < 3; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint64_t t = (uint64_t)x[i] * BcParams::MU[k] + p[i + k] + carry;
            p[i + k] = (uint32_t)t;
            carry = t >> 32;
        }
        p[i + 3] = (uint32_t)carry;
    }
    const uint32_t q[3] = {(p[2] >> 5) | (p[3] << 27), (p[3] >> 5) | (p[4] << 27), p[4] >> 5};  // floor(S1 MU / 2^69), q[2] < 2^5
    uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                                    // qh r mod 2^256
#pragma unroll
    for (int i = 0; i < 3; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int k = 0; k + i < 8; k++) {
            const uint64_t t = (uint64_t)FrParams::MOD[k] * q[i] + m[i + k] + carry;
            m[i + k] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    fe d;  // T = S - qh r in [0, 3 r): below 2^256, so the low 8 limbs are all of it
    uint64_t borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)s[k] - m[k] - borrow;
        d.l[k] = (uint32_t)t;
        borrow = (t >> 63) & 1;
    }
    return Fr::reduce_once(Fr::reduce_once(d));
}


// one entry of a column: wide = it has a high half (a U64 / I64 column; uniform over a launch)
struct BcEntry {
    uint64_t v;
    bool wide;
};

// S mod r for S = C + sum_k G_(k+1) entry(k).v: the public part of a read leaf.  entry(k), k = 0..6: a, v[0..4], t_read, each read where its
// term is made
template <class Entry>
static FF_HD fe bc_read_public(const BcCoeffs& cf, Entry entry) {
    BcAcc acc = bc_start(cf.c);
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const BcEntry e = entry(k);
        bc_term(acc, cf.g[k], e.v, e.wide);
    }
    return bc_reduce(acc);
}

// init = i G_1 + sum_k G_(k+2) entry(k).v + imm + C and fin = init + entry(6).v G_7 for row i.  entry(k), k = 0..6: table[0..4], the imm word,
// t_final.  imm_signed: entry(5).v holds the bits of an I64, which enters as |v| (2^63 for the smallest) times ONE or NEG_ONE
template <class Entry>
static FF_HD void bc_init_final(const BcCoeffs& cf, uint32_t i, Entry entry, bool imm_signed, fe& init, fe& fin) {
    BcAcc acc = bc_start(cf.c);
    bc_mac<0>(acc, cf.g[0], i);
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const BcEntry e = entry(k);
        bc_term(acc, cf.g[k + 1], e.v, e.wide);
    }
    const BcEntry imm = entry(5);
    const bool neg = imm_signed && (int64_t)imm.v < 0;
    fe ci;
#pragma unroll
    for (int l = 0; l < 8; l++) ci.l[l] = neg ? cf.neg_one.l[l] : cf.one.l[l];
    bc_term(acc, ci, neg ? 0 - imm.v : imm.v, imm.wide || imm_signed);
    init = bc_reduce(acc);
    const BcEntry t = entry(6);
    bc_term(acc, cf.g[6], t.v, t.wide);
    fin = bc_reduce(acc);
}

// the coefficients from gamma and tau as the ABI carries them (4 x u64, Montgomery)
static inline BcCoeffs bc_coeffs(const uint64_t gamma[4], const uint64_t tau[4]) {
    BcCoeffs cf;
    fe t;
    for (int i = 0; i < 4; i++) {
        cf.g[0].l[2 * i] = (uint32_t)gamma[i], cf.g[0].l[2 * i + 1] = (uint32_t)(gamma[i] >> 32);
        t.l[2 * i] = (uint32_t)tau[i], t.l[2 * i + 1] = (uint32_t)(tau[i] >> 32);
    }
    for (int k = 1; k < 7; k++) cf.g[k] = Fr::mul(cf.g[k - 1], cf.g[0]);
    cf.one = Fr::one();
    cf.neg_one = Fr::neg(cf.one);
    cf.c = Fr::neg(t);
    return cf;
}
