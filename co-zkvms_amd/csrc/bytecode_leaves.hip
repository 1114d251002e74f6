// The leaves of the bytecode memory check's grand-product circuits (cozk_bytecode_leaves, cozk_bytecode_init_final_leaves; the layout
// is in cozk.h; Rep3BytecodeProver::compute_leaves, co-jolt/src/jolt/vm/bytecode/worker.rs:43-142), with g^k the powers of gamma:
//
//   k_bc_leaves     a thread per step:  read = a g + v[0] g^2 + .. + v[4] g^6 + t_read g^7 + imm - tau  and  write = read + g^7,
//                   from seven compact public columns and the one field column imm (plain, or a Rep3 share)
//   k_bc_if_leaves  a thread per table row:  init = i g + table[0] g^2 + .. + table[4] g^6 + from_i64(table[5]) - tau  and
//                   final = init + t_final g^7; the row number i exists only in registers
//
// Every leaf is the canonical Montgomery word of its value, so it equals bit for bit what the composition of cozk_fingerprint_leaves
// calls gives.  In REP3 the public part enters through add_public as there: party 0's a, party 1's b.
//
// The arithmetic (compact_open.inc and rw_memory_leaves.hip, widened): every coefficient G_k = g^k R mod r, ONE = R mod r,
// NEG_ONE = (r - 1) R mod r and C = (r - tau) R mod r is a Montgomery form below r, and every column entry a plain integer below 2^64
// (an I64 imm is |v| <= 2^63 times ONE or NEG_ONE), so the public part of a leaf is the residue of the exact integer
//     S = C + sum of at most 8 terms coeff * entry  <  r + 8 (2^64 - 1) r  <  2^68 r  <  2^322                    (r < 2^254)
// (k_bc_leaves has 7 terms; k_bc_if_leaves 8, the row number among them below 2^32), held in BC_LIMBS = 11 limbs: per 32-bit half of
// an entry 8 multiply-adds of 32 x 32 + 64 bits (no overflow: (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1), every carry walked to limb 10.
// bc_reduce takes S mod r by a Barrett quotient: with S1 = floor(S / 2^253) < 2^69 and MU = floor(2^322 / r) < 2^69,
//     qh = floor(S1 MU / 2^69)   has   q - 2 <= qh <= q = floor(S / r) < 2^68
// (S1 > S / 2^253 - 1, MU > 2^322 / r - 1, S < 2^322, r >= 2^253: qh > S / r - 3), so T = S - qh r lies in [0, 3 r), below 2^256: it is
// computed on the low 8 limbs alone (S1 MU by 3 x 3 and qh r mod 2^256 by 8 + 7 + 6 multiply-adds) and two conditional subtractions
// of r leave the canonical word.  The rw kernel's 9 limbs and 35-bit constant do not carry over: its entries are below 2^32.
// The field column joins by one Fr::add on the reduced word (it is a share in REP3, and must stay apart from the public part), and the
// write leaf is one more Fr::add of G_7; the final leaf is a second reduction of the sum with its eighth term.
// The arithmetic itself is in bytecode_arith.hip.hpp, host and device; tests/bytecode_ref.py (leaf_word_model, init_final_word_model)
// restates these words with the bounds as asserts.
#include "common.hpp"
#include "bytecode_arith.hip.hpp"

static constexpr int BC_PT = 256;
struct BcCols {
    const void* p[7];
    uint8_t kind[7];
};
static __device__ __forceinline__ uint64_t bc_load(const void* p, int kind, size_t i) {
    switch (kind) {  // uniform over the launch
        case COZK_SCALAR_U8: return ((const uint8_t*)p)[i];
        case COZK_SCALAR_U16: return ((const uint16_t*)p)[i];
        case COZK_SCALAR_U32: return ((const uint32_t*)p)[i];
        default: return ((const uint64_t*)p)[i];  // U64, and the bits of an I64
    }
}

// cols: a, v[0..4], t_read.  ia / ib: the imm column's a and b components, null where the party adds nothing (add_public)
template <int NC>
__global__ void __launch_bounds__(BC_PT) k_bc_leaves(BcCols cols, size_t n, BcCoeffs cf, const fe* __restrict__ ia, const fe* __restrict__ ib, int pub_a, int pub_b,
                                                     fe* __restrict__ oa, fe* __restrict__ ob) {
    const size_t j = (size_t)blockIdx.x * BC_PT + threadIdx.x;
    if (j >= n) return;
    const fe pub = bc_read_public(cf, [&](int k) { return BcEntry{bc_load(cols.p[k], cols.kind[k], j), cols.kind[k] == COZK_SCALAR_U64}; });
    fe a = ia ? fe_load(ia + j) : Fr::zero();
    if (pub_a) a = Fr::add(a, pub);
    fe_store(oa + j, a);
    fe_store(oa + n + j, pub_a ? Fr::add(a, cf.g[6]) : a);
    if (NC == 2) {
        fe b = ib ? fe_load(ib + j) : Fr::zero();
        if (pub_b) b = Fr::add(b, pub);
        fe_store(ob + j, b);
        fe_store(ob + n + j, pub_b ? Fr::add(b, cf.g[6]) : b);
    }
}

// cols: table[0..4], table[5] (imm; imm_signed: an I64 column), t_final.  A party that adds no public part stores zeros.
template <int NC>
__global__ void __launch_bounds__(BC_PT) k_bc_if_leaves(BcCols cols, int imm_signed, size_t B, BcCoeffs cf, int pub_a, int pub_b, fe* __restrict__ oa,
                                                        fe* __restrict__ ob) {
    const size_t i = (size_t)blockIdx.x * BC_PT + threadIdx.x;
    if (i >= B) return;
    fe init = Fr::zero(), fin = Fr::zero();
    if (pub_a || pub_b) {  // uniform over the launch
        bc_init_final(cf, (uint32_t)i, [&](int k) { return BcEntry{bc_load(cols.p[k], cols.kind[k], i), cols.kind[k] == COZK_SCALAR_U64}; }, imm_signed != 0, init, fin);
    }
    const fe zero = Fr::zero();
    fe_store(oa + i, pub_a ? init : zero);
    fe_store(oa + B + i, pub_a ? fin : zero);
    if (NC == 2) {
        fe_store(ob + i, pub_b ? init : zero);
        fe_store(ob + B + i, pub_b ? fin : zero);
    }
}

namespace {

bool bc_compact(const cozk_vec* v) {
    return v && (v->kind == COZK_SCALAR_U8 || v->kind == COZK_SCALAR_U16 || v->kind == COZK_SCALAR_U32 || v->kind == COZK_SCALAR_U64);
}
// the checks on mode, party and outputs that both calls share; len = 2 n or 2 B
void bc_outputs(const std::string& w, int mode, int party_id, const cozk_vec* out_a, const cozk_vec* out_b, size_t offset, size_t len) {
    COZK_REQUIRE(mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, w + ": mode is COZK_MODE_PLAIN or COZK_MODE_REP3");
    COZK_REQUIRE(party_id >= 0 && party_id < 3, w + ": 0 <= party_id < 3");
    COZK_REQUIRE(out_a && out_a->kind == COZK_SCALAR_FR && offset <= out_a->n && out_a->n - offset >= len,
                 w + ": out_a is an FR vector with room for two circuits from offset");
    if (mode == COZK_MODE_REP3)
        COZK_REQUIRE(out_b && out_b != out_a && out_b->kind == COZK_SCALAR_FR && offset <= out_b->n && out_b->n - offset >= len,
                     w + ": REP3 needs out_b, an FR vector with room for two circuits from offset");
    else
        COZK_REQUIRE(!out_b, w + ": out_b is NULL for PLAIN");
}

}  // namespace

extern "C" {

int cozk_bytecode_leaves(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* const* v, const cozk_vec* t_read, const cozk_poly* imm, const uint64_t gamma[4],
                         const uint64_t tau[4], int mode, int party_id, cozk_vec* out_a, cozk_vec* out_b, size_t offset) {
    cozk_vec* view[2] = {nullptr, nullptr};
    const int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && a && v && t_read && imm && gamma && tau, "bytecode_leaves: bad argument");
        const cozk_vec* col[7] = {a, v[0], v[1], v[2], v[3], v[4], t_read};
        BcCols h{};
        for (int k = 0; k < 7; k++) {
            COZK_REQUIRE(bc_compact(col[k]), "bytecode_leaves: a, v[0..4] and t_read are U8 / U16 / U32 / U64 vectors");
            COZK_REQUIRE(col[k]->n == a->n, "bytecode_leaves: every column has n entries");
            h.p[k] = col[k]->d;
            h.kind[k] = (uint8_t)col[k]->kind;
        }
        const size_t n = a->n;
        COZK_REQUIRE(n >= 1 && n < ((size_t)1 << 32), "bytecode_leaves: 1 <= n < 2^32");
        COZK_REQUIRE(cozk_poly_len(imm) >= n, "bytecode_leaves: imm is shorter than n");
        bc_outputs("bytecode_leaves", mode, party_id, out_a, out_b, offset, 2 * n);
        const int imm_mode = cozk_poly_mode(imm);
        COZK_REQUIRE(imm_mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, "bytecode_leaves: a shared imm needs mode COZK_MODE_REP3");
        for (int c = 0; c < (imm_mode == COZK_MODE_REP3 ? 2 : 1); c++)
            if (cozk_poly_share_view(ctx, imm, c, &view[c]) != COZK_OK) throw CozkError(COZK_ERR_INVALID_ARG, "bytecode_leaves: " + ctx->last_error);
        const fe *ia = (const fe*)view[0]->d, *ib = view[1] ? (const fe*)view[1]->d : nullptr;
        const BcCoeffs cf = bc_coeffs(gamma, tau);
        const unsigned grid = (unsigned)((n + BC_PT - 1) / BC_PT);
        fe* oa = (fe*)out_a->d + offset;
        if (mode == COZK_MODE_REP3) {
            if (imm_mode == COZK_MODE_PLAIN) {  // a public imm enters through add_public too: party 0's a, party 1's b
                ib = party_id == 1 ? ia : nullptr;
                ia = party_id == 0 ? ia : nullptr;
            }
            k_bc_leaves<2><<<grid, BC_PT, 0, ctx->stream>>>(h, n, cf, ia, ib, party_id == 0, party_id == 1, oa, (fe*)out_b->d + offset);
        } else {
            k_bc_leaves<1><<<grid, BC_PT, 0, ctx->stream>>>(h, n, cf, ia, nullptr, 1, 0, oa, nullptr);
        }
        HIP_TRY(hipGetLastError());
    });
    for (cozk_vec* w : view) cozk_vec_free(w);  // views: the polynomial keeps its buffers
    return rc;
}

int cozk_bytecode_init_final_leaves(cozk_ctx* ctx, const cozk_vec* const* table, const cozk_vec* t_final, const uint64_t gamma[4], const uint64_t tau[4], int mode,
                                    int party_id, cozk_vec* out_a, cozk_vec* out_b, size_t offset) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && table && t_final && gamma && tau, "bytecode_init_final_leaves: bad argument");
        const cozk_vec* col[7] = {table[0], table[1], table[2], table[3], table[4], table[5], t_final};
        BcCols h{};
        for (int k = 0; k < 7; k++) {
            if (k == 5)
                COZK_REQUIRE(bc_compact(col[k]) || (col[k] && col[k]->kind == COZK_SCALAR_I64), "bytecode_init_final_leaves: table[5] is a U8 / U16 / U32 / U64 / I64 vector");
            else
                COZK_REQUIRE(bc_compact(col[k]), "bytecode_init_final_leaves: table[0..4] and t_final are U8 / U16 / U32 / U64 vectors");
            COZK_REQUIRE(col[k]->n == col[0]->n, "bytecode_init_final_leaves: every column has B entries");
            h.p[k] = col[k]->d;
            h.kind[k] = (uint8_t)col[k]->kind;
        }
        const size_t B = col[0]->n;
        COZK_REQUIRE(B >= 1 && B < ((size_t)1 << 32), "bytecode_init_final_leaves: 1 <= B < 2^32");
        bc_outputs("bytecode_init_final_leaves", mode, party_id, out_a, out_b, offset, 2 * B);
        const BcCoeffs cf = bc_coeffs(gamma, tau);
        const unsigned grid = (unsigned)((B + BC_PT - 1) / BC_PT);
        const int imm_signed = h.kind[5] == COZK_SCALAR_I64;
        fe* oa = (fe*)out_a->d + offset;
        if (mode == COZK_MODE_REP3)
            k_bc_if_leaves<2><<<grid, BC_PT, 0, ctx->stream>>>(h, imm_signed, B, cf, party_id == 0, party_id == 1, oa, (fe*)out_b->d + offset);
        else
            k_bc_if_leaves<1><<<grid, BC_PT, 0, ctx->stream>>>(h, imm_signed, B, cf, 1, 0, oa, nullptr);
        HIP_TRY(hipGetLastError());
    });
}

}  // extern "C"
