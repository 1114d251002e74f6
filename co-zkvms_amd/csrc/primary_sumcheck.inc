// Lasso's primary sumcheck of the instruction lookups (SURVEY 8(f)1b) -- part of poly.hip's translation unit.
//
//   sum_x eq(r, x) * ( sum_i flag_i(x) * g_i(E_1(x), .., E_alpha(x)) - lookup_output(x) ) = 0
//
//   cozk_primary  <->  the state of prove_primary_sumcheck_inner (co-jolt/src/jolt/vm/instruction_lookups/worker.rs:375-452):
//   eq (public), the instruction flags (public 0/1 columns), the E polynomials and lookup_outputs (shared), all bound
//   LowToHigh once per round; one round = primary_sumcheck_prover_message (:454-598): `degree` additive evaluations at
//   X = 0, 2, 3, .., degree (the coordinator inserts claim - e(0), instruction_lookups/coordinator.rs:131-132).
//
// The instruction collations g_i (combine_lookups_rep3_batched, co-jolt/src/jolt/instruction/*.rs) come as a TABLE of
// forms (include/cozk.h COZK_G_*: all 27 RV32I instructions of jolt/vm/rv32i_vm.rs:41-70 are one of them).  CONCAT,
// NOT_FIRST and ZERO are linear and local.  Every other form is compiled (prim_compile) into a small straight-line
// PROGRAM over the instruction's memories:
//     slot   = sum_p X_p (x) Y_p [+ into_additive(A)]      a value that is reshared: one batched mul_vec /
//                                                          reshare_additive_many of its LEVEL (slt.rs:262-283)
//     result = sum_p X_p (x) Y_p + into_additive(A)        the last, local step: stays additive (worker.rs:553)
// where X, Y, A are public affine forms (c0 + sum of +-1, +-2 multiples) of memories and earlier slots -- c0 enters by
// add_public (party 0's a, party 1's b: mpc-types rep3/arithmetic/ops.rs).  All items of a level go through ONE exchange:
// local products + zero-sharing masks on the device, then the ring reshare (the host runs it between cozk_primary_level
// and the next call; utils/future.rs:48-69 is the reference's batching of the same thing).  The final reshare of
// sltu.rs:163-169 / the last mul_vec of slt.rs:289-296 is not performed: into_additive follows it (worker.rs:553), which
// restores the same total, so the coordinator's sums -- and the proof -- are unchanged and one ring round is saved.
//
// MI355X formulation: flags are public, so WHICH (index, instruction) pairs are active is public too: one 0/1 array in
// (instruction, index) order + one exclusive scan give every party the same item list, grouped by instruction (hence the
// same buffer positions and mask counters).  Linear instructions are summed in one streaming pass that skips an
// instruction as soon as both of its flags at the index are zero (after round 0 at most 2^round instructions are live per
// index); the multiplicative ones touch only their items.

#include <hipcub/hipcub.hpp>

static constexpr int PRIM_MAX_MEMS = COZK_PRIMARY_MAX_MEMS;
static constexpr int PRIM_MAX_DEG = 8;
static constexpr int PRIM_MAX_LEVELS = COZK_PRIMARY_MAX_LEVELS;
static constexpr int PRIM_MAX_SLOTS = 12;
static constexpr int PRIM_MAX_PROD = 4;
static constexpr int PRIM_MAX_FINAL = 8;
static constexpr int PRIM_MAX_MUL = 32;
static constexpr int PRIM_SLOT = 32;  // PrimLC::src >= PRIM_SLOT: slot number src - PRIM_SLOT; below: position in the instruction's mems

struct PrimLC {  // c0 + sum_t coef[t] * value(src[t])
    int8_t n, c0;
    int8_t coef[3];
    uint8_t src[3];
};
struct PrimProd {
    PrimLC x, y;
};
struct PrimSlot {
    int8_t level, n_prod, q, has_add;  // q: position among the slots of its level
    PrimLC add;
    PrimProd prod[PRIM_MAX_PROD];
};
struct PrimInstrDev {
    int form, n_mems, bits, n_levels, n_slots, n_final, g_degree, linear;
    int mems[PRIM_MAX_MEMS];
    fe coef[PRIM_MAX_MEMS];  // linear forms: weights (CONCAT 2^(bits (C-1-j)), NOT_FIRST -1) in Montgomery form
    fe lin_c0;               // linear forms: the public constant as THIS party adds it to its (a + b) sums
    int nq[PRIM_MAX_LEVELS];  // slots per level
    PrimSlot slots[PRIM_MAX_SLOTS];
    PrimProd fin[PRIM_MAX_FINAL];
    PrimLC fin_add;
};

struct cozk_primary {
    cozk_ctx* ctx;
    int mode, party;
    int n_instr, n_mem, degree, max_levels;
    size_t n0, n;               // original / current length of every polynomial
    int T;                      // polynomials per set: flags | E.a | E.b | out.a | out.b | eq
    fe* store[2];               // ping-pong sets: polynomial p lives at store[w] + p * cap[w]
    size_t cap[2];
    int cur;
    std::vector<PrimInstrDev> instrs;
    std::vector<int> lin, mul;  // indices of the linear / multiplicative instructions
    PrimInstrDev* d_instrs;
    int* d_lin;
    int* d_mul;
    // item list of the current round, grouped by instruction: items of mul[s] are [first[s], first[s + 1])
    uint64_t* d_live;           // per index: bit i = instruction i live (a flag of the pair non-zero)
    uint32_t* d_act;            // [n_mul][idx_cap]: 1 = instruction mul[s] active at the index; then its exclusive scan
    uint32_t* d_item_idx;       // per item: index
    uint32_t* d_item_slot;      // per item: position in `mul`
    uint32_t* d_bases;          // [PRIM_MAX_LEVELS][PRIM_MAX_MUL] element offsets of the instruction groups in the level buffers, then first[PRIM_MAX_MUL]
    size_t items_cap, idx_cap;
    size_t n_items;
    size_t level_elems[PRIM_MAX_LEVELS];
    fe* P[PRIM_MAX_LEVELS][2];  // reshared values of level t (1-based: P[t-1]), [component]
    size_t P_cap[PRIM_MAX_LEVELS];
    DevBuf scan_tmp;
    fe lin_sums[PRIM_MAX_DEG];  // the linear pass of this round: sums of (a + b) terms
};

// ---------------------------------------------------------------- form -> program
namespace {
struct PrimBuild {
    PrimInstrDev& d;
    explicit PrimBuild(PrimInstrDev& dd) : d(dd) {}
    static PrimLC konst(int c0) {
        PrimLC l{};
        l.c0 = (int8_t)c0;
        return l;
    }
    static PrimLC mem(int pos, int c = 1) {
        PrimLC l{};
        l.n = 1;
        l.coef[0] = (int8_t)c;
        l.src[0] = (uint8_t)pos;
        return l;
    }
    static PrimLC slot(int s, int c = 1) { return mem(PRIM_SLOT + s, c); }
    static PrimLC neg(PrimLC l) {
        for (int t = 0; t < l.n; t++) l.coef[t] = (int8_t)-l.coef[t];
        l.c0 = (int8_t)-l.c0;
        return l;
    }
    static PrimLC one_minus(PrimLC l) {
        l = neg(l);
        l.c0 = (int8_t)(l.c0 + 1);
        return l;
    }
    static PrimLC plus(PrimLC a, const PrimLC& b) {
        COZK_REQUIRE(a.n + b.n <= 3, "primary: affine form too long");
        for (int t = 0; t < b.n; t++) {
            a.coef[a.n] = b.coef[t];
            a.src[a.n] = b.src[t];
            a.n++;
        }
        a.c0 = (int8_t)(a.c0 + b.c0);
        return a;
    }
    int add_slot(int level, const std::vector<PrimProd>& prods, const PrimLC* add = nullptr) {
        COZK_REQUIRE(d.n_slots < PRIM_MAX_SLOTS && level >= 1 && level <= PRIM_MAX_LEVELS && prods.size() <= (size_t)PRIM_MAX_PROD,
                     "primary: collation program too large (chunk count C too high for this form)");
        PrimSlot& s = d.slots[d.n_slots];
        s.level = (int8_t)level;
        s.n_prod = (int8_t)prods.size();
        s.q = (int8_t)d.nq[level - 1]++;
        for (size_t p = 0; p < prods.size(); p++) s.prod[p] = prods[p];
        s.has_add = add ? 1 : 0;
        if (add) s.add = *add;
        if (level > d.n_levels) d.n_levels = level;
        return d.n_slots++;
    }
    void add_final(const PrimLC& x, const PrimLC& y) {
        COZK_REQUIRE(d.n_final < PRIM_MAX_FINAL, "primary: collation program too large");
        d.fin[d.n_final++] = PrimProd{x, y};
    }
    // prefix products P_0 = m_0, P_t = P_{t-1} (x) m_t (level t) of the memories at `pos`: returns P_0 .. P_{count-1}
    std::vector<PrimLC> prefix(const std::vector<int>& pos, int count) {
        std::vector<PrimLC> P;
        if (count <= 0) return P;
        P.push_back(mem(pos[0]));
        for (int t = 1; t < count; t++) P.push_back(slot(add_slot(t, {PrimProd{P[t - 1], mem(pos[t])}})));
        return P;
    }
    void negate_result() {  // g -> 1 - g
        for (int f = 0; f < d.n_final; f++) d.fin[f].x = neg(d.fin[f].x);
        d.fin_add = one_minus(d.fin_add);
    }
    // sum_i ltu_i prod_{j<i} eq_j  (sltu.rs:139-170): ltu at positions l0 .., eq at e0 ..; n_eq eq memories are chained
    std::vector<PrimLC> ltu_part(int C, int l0, int e0, int n_eq) {
        d.fin_add = plus(d.fin_add, mem(l0));
        std::vector<int> eqpos;
        for (int t = 0; t < n_eq; t++) eqpos.push_back(e0 + t);
        std::vector<PrimLC> P = prefix(eqpos, std::min(n_eq, C - 1));
        for (int i = 1; i < C; i++) add_final(mem(l0 + i), P[i - 1]);
        return P;
    }
    void product_part(int p0, int n, bool negated) {  // prod_{t<n} mems[p0 + t] added to (subtracted from) the result
        if (n == 1) {
            d.fin_add = plus(d.fin_add, mem(p0, negated ? -1 : 1));
            return;
        }
        std::vector<int> pos;
        for (int t = 0; t < n; t++) pos.push_back(p0 + t);
        std::vector<PrimLC> P = prefix(pos, n - 1);
        add_final(negated ? neg(P[n - 2]) : P[n - 2], mem(p0 + n - 1));
    }
};

static int prim_lc_degree(const PrimInstrDev& d, const PrimLC& l, const int* slot_deg) {
    int g = 0;
    for (int t = 0; t < l.n; t++) g = std::max(g, l.src[t] < PRIM_SLOT ? 1 : slot_deg[l.src[t] - PRIM_SLOT]);
    (void)d;
    return g;
}

// the chunk count C of a form from its memory count; 0 = the count does not fit the form
static int prim_chunks(int form, int n) {
    switch (form) {
        case COZK_G_LTU:
        case COZK_G_NOT_LTU: return n % 2 == 1 ? (n + 1) / 2 : 0;
        case COZK_G_SLT:
        case COZK_G_NOT_SLT: return n % 2 == 1 && n >= 5 ? (n - 1) / 2 : 0;
        case COZK_G_LTE:
        case COZK_G_DIV0: return n % 2 == 0 ? n / 2 : 0;
        case COZK_G_UNSIGNED_REM: return (n + 1) % 3 == 0 ? (n + 1) / 3 : 0;
        case COZK_G_SIGNED_REM: return n >= 10 && (n - 2) % 4 == 0 ? (n - 2) / 4 : 0;
        default: return n;
    }
}

static void prim_compile(const cozk_primary_instr& s, int party, bool rep3, PrimInstrDev& d) {
    d = PrimInstrDev{};
    d.form = s.form;
    d.n_mems = s.n_mems;
    d.bits = s.bits;
    for (int t = 0; t < s.n_mems; t++) {
        d.mems[t] = s.mems[t];
        d.coef[t] = Fr::zero();
    }
    d.lin_c0 = Fr::zero();
    const int n = s.n_mems;
    const int C = prim_chunks(s.form, n);
    COZK_REQUIRE(C >= 1, "primary_create: the memory count does not fit the instruction form");
    PrimBuild b(d);
    const fe one_here = (!rep3 || party < 2) ? Fr::one() : Fr::zero();  // add_public of 1 as seen in this party's a + b
    switch (s.form) {
        case COZK_G_CONCAT: {
            COZK_REQUIRE(s.bits >= 0 && s.bits * (n - 1) < 200, "primary_create: CONCAT shift");
            d.linear = 1;
            fe shift = Fr::from_u64(1), two = Fr::from_u64(2);
            for (int k = 0; k < s.bits; k++) shift = Fr::mul(shift, two);
            fe w = Fr::one();
            for (int t = n - 1; t >= 0; t--) {
                d.coef[t] = w;
                w = Fr::mul(w, shift);
            }
            d.g_degree = 1;
            return;
        }
        case COZK_G_NOT_FIRST:
            d.linear = 1;
            d.coef[0] = Fr::neg(Fr::one());
            d.lin_c0 = one_here;
            d.g_degree = 1;
            return;
        case COZK_G_ZERO:
            d.linear = 1;
            d.g_degree = 1;  // virtual_pow2.rs:24-26 declares 1
            return;
        case COZK_G_PRODUCT:
        case COZK_G_NOT_PRODUCT:
            b.product_part(0, n, false);
            break;
        case COZK_G_LTU:
        case COZK_G_NOT_LTU:
            (void)b.ltu_part(C, 0, C, C - 1);
            break;
        case COZK_G_LTE: {  // ltu_sum over all C chunks + prod of all C eq (virtual_assert_lte.rs:33-50)
            if (C == 1) {
                d.fin_add = b.plus(b.mem(0), b.mem(1));
                break;
            }
            std::vector<PrimLC> P = b.ltu_part(C, 0, C, C);  // chains eq_0 .. eq_{C-2}: P_0 .. P_{C-2}
            b.add_final(P[C - 2], b.mem(2 * C - 1));
            break;
        }
        case COZK_G_UNSIGNED_REM:
            (void)b.ltu_part(C, 0, C, C - 1);
            b.product_part(2 * C - 1, C, false);
            break;
        case COZK_G_DIV0:
            d.fin_add = b.konst(1);
            b.product_part(0, C, true);
            b.product_part(C, C, false);
            break;
        case COZK_G_SLT:
        case COZK_G_NOT_SLT: {
            // mems: l, r, ltu[C-1], eq[C-2], lt_abs, eq_abs (slt.rs:65-74)
            const int l = 0, r = 1, ltu0 = 2, eq0 = C + 1, lt_abs = 2 * C - 1, eq_abs = 2 * C;
            std::vector<int> chain{eq_abs};
            for (int t = 0; t < C - 2; t++) chain.push_back(eq0 + t);
            std::vector<PrimLC> P = b.prefix(chain, C - 1);  // eq_abs prod_{j<i} eq_j, i = 0 .. C-2
            const int Lr = std::max(1, C - 1);  // the reshare_additive_many level (slt.rs:262-283): after the chain
            const int lnr = b.add_slot(Lr, {PrimProd{b.mem(l), b.one_minus(b.mem(r))}});
            const int lr = b.add_slot(Lr, {PrimProd{b.mem(l), b.mem(r)}});
            const int nlnr = b.add_slot(Lr, {PrimProd{b.one_minus(b.mem(l)), b.one_minus(b.mem(r))}});
            std::vector<PrimProd> sp;
            for (int i = 0; i <= C - 2; i++) sp.push_back(PrimProd{b.mem(ltu0 + i), P[i]});
            PrimLC la = b.mem(lt_abs);
            const int S = b.add_slot(Lr, sp, &la);
            d.fin_add = b.slot(lnr);
            b.add_final(b.plus(b.slot(lr), b.slot(nlnr)), b.slot(S));
            break;
        }
        case COZK_G_SIGNED_REM: {
            // mems: l, r, eq[C-1], ltu[C-1], eq_abs, lt_abs, left_is_zero[C], right_is_zero[C]
            // (virtual_assert_valid_signed_remainder.rs:76-95; formula :40-67)
            const int l = 0, r = 1, eq0 = 2, ltu0 = C + 1, eq_abs = 2 * C, lt_abs = 2 * C + 1, lz0 = 2 * C + 2, rz0 = 3 * C + 2;
            std::vector<int> chain{eq_abs}, lz, rz;
            for (int t = 0; t < C - 1; t++) chain.push_back(eq0 + t);
            for (int t = 0; t < C; t++) {
                lz.push_back(lz0 + t);
                rz.push_back(rz0 + t);
            }
            std::vector<PrimLC> P = b.prefix(chain, C);  // P_i = eq_abs prod_{j<i} eq_j; P_{C-1} = EQ(x_{<s}, y_{<s})
            std::vector<PrimLC> LZ = b.prefix(lz, C);    // remainder_is_zero as a share: it is multiplied again
            const int lr = b.add_slot(1, {PrimProd{b.mem(l), b.mem(r)}});
            const int nlr = b.add_slot(1, {PrimProd{b.one_minus(b.mem(l)), b.mem(r)}});
            std::vector<PrimProd> sp;
            for (int i = 0; i <= C - 2; i++) sp.push_back(PrimProd{b.mem(ltu0 + i), P[i]});
            PrimLC la = b.mem(lt_abs);
            const int S = b.add_slot(std::max(1, C - 1), sp, &la);
            b.add_final(b.plus(b.one_minus(b.mem(l)), b.mem(r, -1)), b.slot(S));
            b.add_final(b.slot(lr), b.one_minus(P[C - 1]));
            b.add_final(b.slot(nlr), LZ[C - 1]);
            b.product_part(rz0, C, false);
            break;
        }
        default: throw CozkError(COZK_ERR_INVALID_ARG, "primary_create: unknown instruction form");
    }
    if (s.form == COZK_G_NOT_PRODUCT || s.form == COZK_G_NOT_LTU || s.form == COZK_G_NOT_SLT) b.negate_result();
    // degree of g in the sumcheck variable
    int slot_deg[PRIM_MAX_SLOTS];
    for (int q = 0; q < d.n_slots; q++) {
        const PrimSlot& sl = d.slots[q];
        int g = sl.has_add ? prim_lc_degree(d, sl.add, slot_deg) : 0;
        for (int p = 0; p < sl.n_prod; p++) g = std::max(g, prim_lc_degree(d, sl.prod[p].x, slot_deg) + prim_lc_degree(d, sl.prod[p].y, slot_deg));
        slot_deg[q] = g;
    }
    int g = prim_lc_degree(d, d.fin_add, slot_deg);
    for (int f = 0; f < d.n_final; f++) g = std::max(g, prim_lc_degree(d, d.fin[f].x, slot_deg) + prim_lc_degree(d, d.fin[f].y, slot_deg));
    d.g_degree = std::max(1, g);
}
}  // namespace

// polynomial slots inside a set
static __host__ __device__ inline int prim_slot_flag(int i) { return i; }
static __host__ __device__ inline int prim_slot_E(int n_instr, int n_mem, int m, int comp) { return n_instr + comp * n_mem + m; }
static __host__ __device__ inline int prim_slot_out(int n_instr, int n_mem, int NC, int comp) { return n_instr + NC * n_mem + comp; }
static __host__ __device__ inline int prim_slot_eq(int n_instr, int n_mem, int NC) { return n_instr + NC * n_mem + NC; }

// value at evaluation point number k (X = 0, 2, 3, ..): v0 + X (v1 - v0), walked incrementally by the callers

// bind every polynomial of the set with r, LowToHigh (worker.rs:413-425)
__global__ void __launch_bounds__(PT) k_primary_bind(const fe* __restrict__ src, size_t cap_src, fe* __restrict__ dst, size_t cap_dst, size_t n_out, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    const fe* in = src + (size_t)blockIdx.y * cap_src;
    fe lo = fe_load(in + 2 * i), hi = fe_load(in + 2 * i + 1);
    fe_store(dst + (size_t)blockIdx.y * cap_dst + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
}

__global__ void __launch_bounds__(PT) k_primary_flags_expand(const uint8_t* const* __restrict__ cols, size_t n, size_t cap, int n_instr, fe* __restrict__ store) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    int c = blockIdx.y;
    fe_store(store + (size_t)prim_slot_flag(c) * cap + i, cols[c][i] ? Fr::one() : Fr::zero());
}

// which instructions are live at index i (either flag of the pair non-zero): one bit per instruction.  The loads of the
// n_instr flag pairs are independent, so they are all in flight at once; the passes below test bits instead of re-reading flags.
__global__ void __launch_bounds__(PT) k_primary_mask(const fe* __restrict__ st, size_t cap, size_t half, int n_instr, uint64_t* __restrict__ mask) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= half) return;
    uint64_t m = 0;
    for (int q = 0; q < n_instr; q++) {
        const fe* fp = st + (size_t)prim_slot_flag(q) * cap;
        fe f0 = fe_load(fp + 2 * i), f1 = fe_load(fp + 2 * i + 1);
        uint32_t nz = 0;
#pragma unroll
        for (int l = 0; l < 8; l++) nz |= f0.l[l] | f1.l[l];
        m |= (uint64_t)(nz != 0) << q;
    }
    mask[i] = m;
}

// the streaming pass over the LINEAR instructions, lookup_outputs and eq:
//   partial[k] += eq(k) * ( sum_{linear i} f_i(k) * (G_i.a + G_i.b)(k) - (out.a + out.b)(k) )      k = 0 .. D-1 <-> X = 0, 2, .., D
// (the (a + b) sums become additive shares by the TWO_INV the host applies once: into_additive, worker.rs:553,576)
template <int NC>
__global__ void __launch_bounds__(PT) k_primary_linear(const fe* __restrict__ st, size_t cap, size_t half, int n_instr, int n_mem, int D,
                                                    const PrimInstrDev* __restrict__ instrs, uint64_t lin_bits,
                                                    const uint64_t* __restrict__ mask, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    // per index the contribution  eq(X) (sum_i f_i(X) G_i(X) - out(X))  is a CUBIC in X (f, G, out, eq are linear in X): the
    // kernel sums its four coefficients, the host evaluates the sum at X = 0, 2, .., D -- the same field elements as
    // summing the D evaluations, with 4 accumulators instead of 2 D and ~3 products per live instruction instead of D
    fe c0 = Fr::zero(), c1 = Fr::zero(), c2 = Fr::zero(), c3 = Fr::zero();
    const fe* eqp = st + (size_t)prim_slot_eq(n_instr, n_mem, NC) * cap;
    const fe* oa = st + (size_t)prim_slot_out(n_instr, n_mem, NC, 0) * cap;
    const fe* ob = NC == 2 ? st + (size_t)prim_slot_out(n_instr, n_mem, NC, 1) * cap : nullptr;
    (void)D;
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < half; i += (size_t)gridDim.x * PT) {
        // inner(X) = sum_i f_i(X) G_i(X) = q0 + q1 X + q2 X^2
        fe q0 = Fr::zero(), q2 = Fr::zero(), q11 = Fr::zero();  // q11 = sum f_i(1) G_i(1)
        // every lane walks ITS OWN live linear instructions (one or two per index pair: the flags are one-hot per cycle) instead of
        // the wave walking the union of its lanes' -- with the uniform 27-instruction mix that union was ~20 instructions with a
        // quarter of the lanes active in each (rocprofv3 --pmc: 0.24 lane utilisation)
        uint64_t todo = mask[i] & lin_bits;
        while (todo) {
            const int iq = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const PrimInstrDev& in = instrs[iq];
            const fe* fp = st + (size_t)prim_slot_flag(iq) * cap;
            fe f0 = fe_load(fp + 2 * i), f1 = fe_load(fp + 2 * i + 1);
            fe g0 = in.lin_c0, g1 = in.lin_c0;
            const int nt = in.form == COZK_G_ZERO ? 0 : (in.form == COZK_G_NOT_FIRST ? 1 : in.n_mems);
            for (int t = 0; t < nt; t++) {
                const fe* ea = st + (size_t)prim_slot_E(n_instr, n_mem, in.mems[t], 0) * cap;
                fe v0 = fe_load(ea + 2 * i), v1 = fe_load(ea + 2 * i + 1);
                if (NC == 2) {
                    const fe* eb = st + (size_t)prim_slot_E(n_instr, n_mem, in.mems[t], 1) * cap;
                    v0 = Fr::add(v0, fe_load(eb + 2 * i));
                    v1 = Fr::add(v1, fe_load(eb + 2 * i + 1));
                }
                g0 = Fr::add(g0, Fr::mul(v0, in.coef[t]));
                g1 = Fr::add(g1, Fr::mul(v1, in.coef[t]));
            }
            q0 = Fr::add(q0, Fr::mul(f0, g0));
            q11 = Fr::add(q11, Fr::mul(f1, g1));
            q2 = Fr::add(q2, Fr::mul(Fr::sub(f1, f0), Fr::sub(g1, g0)));
        }
        fe q1 = Fr::sub(Fr::sub(q11, q0), q2);
        fe e0 = fe_load(eqp + 2 * i), e1 = fe_load(eqp + 2 * i + 1);
        fe o0 = fe_load(oa + 2 * i), o1 = fe_load(oa + 2 * i + 1);
        if (NC == 2) {
            o0 = Fr::add(o0, fe_load(ob + 2 * i));
            o1 = Fr::add(o1, fe_load(ob + 2 * i + 1));
        }
        fe de = Fr::sub(e1, e0);
        q0 = Fr::sub(q0, o0);
        q1 = Fr::sub(q1, Fr::sub(o1, o0));
        // (q0 + q1 X + q2 X^2)(e0 + de X)
        c0 = Fr::add(c0, Fr::mul(q0, e0));
        c1 = Fr::add(c1, Fr::add(Fr::mul(q0, de), Fr::mul(q1, e0)));
        c2 = Fr::add(c2, Fr::add(Fr::mul(q1, de), Fr::mul(q2, e0)));
        c3 = Fr::add(c3, Fr::mul(q2, de));
    }
    fe v = fr_block_sum(c0, sh4);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, v);
    v = fr_block_sum(c1, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)gridDim.x + blockIdx.x, v);
    v = fr_block_sum(c2, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)2 * gridDim.x + blockIdx.x, v);
    v = fr_block_sum(c3, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)3 * gridDim.x + blockIdx.x, v);
}

// columns into their slots of the store: 16-byte pieces, one column per blockIdx.y
static constexpr int PRIM_GATHER_MAX = 160;
struct PrimGatherTab {
    const fe* src[PRIM_GATHER_MAX];
    uint32_t slot[PRIM_GATHER_MAX];
};
__global__ void __launch_bounds__(PT) k_primary_gather(PrimGatherTab tab, size_t n, fe* __restrict__ store) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;  // 16-byte piece of the column
    if (i >= 2 * n) return;
    const uint4* s = reinterpret_cast<const uint4*>(tab.src[blockIdx.y]);
    uint4* d = reinterpret_cast<uint4*>(store + (size_t)tab.slot[blockIdx.y] * n);
    d[i] = s[i];
}

struct PrimBasesTab {
    uint32_t v[(PRIM_MAX_LEVELS + 1) * PRIM_MAX_MUL];
};
__global__ void k_primary_store_bases(PrimBasesTab tab, uint32_t* __restrict__ out) {
    for (int i = threadIdx.x; i < (PRIM_MAX_LEVELS + 1) * PRIM_MAX_MUL; i += blockDim.x) out[i] = tab.v[i];
}

// which multiplicative instructions are active where: act[s][i] from the live mask, grid (indices, n_mul)
__global__ void __launch_bounds__(PT) k_primary_active(const uint64_t* __restrict__ mask, size_t half, const int* __restrict__ mul, uint32_t* __restrict__ act) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= half) return;
    const int s = blockIdx.y;
    act[(size_t)s * half + i] = (uint32_t)((mask[i] >> mul[s]) & 1);
}
__global__ void __launch_bounds__(PT) k_primary_items(const uint32_t* __restrict__ act, const uint32_t* __restrict__ off, size_t half,
                                                   uint32_t* __restrict__ item_idx, uint32_t* __restrict__ item_slot) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= half) return;
    const size_t t = (size_t)blockIdx.y * half + i;
    if (!act[t]) return;
    const uint32_t o = off[t];
    item_idx[o] = (uint32_t)i;
    item_slot[o] = blockIdx.y;
}

template <int NC>
static __device__ __forceinline__ void prim_E_pair(const fe* st, size_t cap, int n_instr, int n_mem, int m, size_t i, Sh<NC>& v0, Sh<NC>& v1) {
    const fe* ea = st + (size_t)prim_slot_E(n_instr, n_mem, m, 0) * cap;
    const fe* eb = NC == 2 ? st + (size_t)prim_slot_E(n_instr, n_mem, m, 1) * cap : nullptr;
    v0 = sh_load<NC>(ea, eb, 2 * i);
    v1 = sh_load<NC>(ea, eb, 2 * i + 1);
}

struct PrimLevelPtrs {
    const fe* a[PRIM_MAX_LEVELS];
    const fe* b[PRIM_MAX_LEVELS];
};

// one (item, evaluation point) of a collation program
template <int NC>
struct PrimCtx {
    const fe* st;
    size_t cap, i;
    int n_instr, n_mem, party, D, s, k, X;
    uint32_t jrel;  // item number inside its instruction group
    const PrimInstrDev* in;
    const uint32_t* bases;
    PrimLevelPtrs P;
};
template <int NC>
static __device__ __forceinline__ size_t prim_slot_pos(const PrimCtx<NC>& c, int level0, int q) {
    return (size_t)c.bases[level0 * PRIM_MAX_MUL + c.s] + ((size_t)c.jrel * c.in->nq[level0] + q) * c.D + c.k;
}
template <int NC>
static __device__ __forceinline__ Sh<NC> prim_value(const PrimCtx<NC>& c, int src) {
    if (src < PRIM_SLOT) {  // E_mems[src](X) = v0 + X (v1 - v0)
        Sh<NC> v0, v1;
        prim_E_pair<NC>(c.st, c.cap, c.n_instr, c.n_mem, c.in->mems[src], c.i, v0, v1);
        Sh<NC> d = sh_sub<NC>(v1, v0), v = v0;
        for (int x = 0; x < c.X; x++) v = sh_add<NC>(v, d);  // X <= 8
        return v;
    }
    const PrimSlot& sl = c.in->slots[src - PRIM_SLOT];
    return sh_load<NC>(c.P.a[sl.level - 1], c.P.b[sl.level - 1], prim_slot_pos<NC>(c, sl.level - 1, sl.q));
}
template <int NC>
static __device__ __forceinline__ Sh<NC> prim_lc(const PrimCtx<NC>& c, const PrimLC& lc) {
    Sh<NC> acc;
    for (int t = 0; t < NC; t++) acc.c[t] = Fr::zero();
    for (int t = 0; t < lc.n; t++) {
        Sh<NC> v = prim_value<NC>(c, lc.src[t]);
        const int w = lc.coef[t];
        if (w == 2 || w == -2) v = sh_add<NC>(v, v);
        acc = w > 0 ? sh_add<NC>(acc, v) : sh_sub<NC>(acc, v);
    }
    if (lc.c0) {  // add_public: party 0's a and party 1's b carry the constant; the plain prover's value does
        const int comp = NC == 1 ? 0 : (c.party == 0 ? 0 : (c.party == 1 ? NC - 1 : -1));
        if (comp >= 0) acc.c[comp] = lc.c0 > 0 ? Fr::add(acc.c[comp], Fr::one()) : Fr::sub(acc.c[comp], Fr::one());
    }
    return acc;
}
template <int NC>
static __device__ __forceinline__ fe prim_products(const PrimCtx<NC>& c, const PrimProd* prods, int n) {
    fe z = Fr::zero();
    for (int p = 0; p < n; p++) z = Fr::add(z, sh_local_mul<NC>(prim_lc<NC>(c, prods[p].x), prim_lc<NC>(c, prods[p].y)));
    return z;
}

// level `level` (1-based) of the collation programs: every slot of that level of every item, at every evaluation point:
//   za[pos] = sum_p X_p (x) Y_p + into_additive(A) + mask          (mul_vec local half: mpc-types/src/protocols/rep3/
//   arithmetic/ops.rs:71-78; into_additive: types.rs:76-81; zero-sharing mask: prf.hip.hpp)
template <int NC>
__global__ void __launch_bounds__(PT) k_primary_level(const fe* __restrict__ st, size_t cap, int n_instr, int n_mem, int D, int party,
                                                   const PrimInstrDev* __restrict__ instrs, const int* __restrict__ mul,
                                                   const uint32_t* __restrict__ item_idx, const uint32_t* __restrict__ item_slot, size_t n_items, int level,
                                                   const uint32_t* __restrict__ bases, PrimLevelPtrs P, fe* __restrict__ za, int masked, prf_key key_self,
                                                   prf_key key_prev, uint64_t ctr) {
    size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_items) return;
    PrimCtx<NC> c;
    c.st = st;
    c.cap = cap;
    c.n_instr = n_instr;
    c.n_mem = n_mem;
    c.party = party;
    c.D = D;
    c.s = (int)item_slot[j];
    c.in = instrs + mul[c.s];
    if (level > c.in->n_levels || c.in->nq[level - 1] == 0) return;  // this instruction has nothing at this level
    c.i = item_idx[j];
    c.jrel = (uint32_t)j - bases[PRIM_MAX_LEVELS * PRIM_MAX_MUL + c.s];
    c.bases = bases;
    c.P = P;
    c.k = blockIdx.y;  // one evaluation point per grid row: n_items x D threads keep the chip busy, the item loop does not
    c.X = c.k == 0 ? 0 : c.k + 1;
    for (int q = 0; q < c.in->n_slots; q++) {
        const PrimSlot& sl = c.in->slots[q];
        if (sl.level != level) continue;
        fe z = prim_products<NC>(c, sl.prod, sl.n_prod);
        if (sl.has_add) {
            fe v = sh_ab_sum<NC>(prim_lc<NC>(c, sl.add));
            z = Fr::add(z, NC == 2 ? Fr::mul(v, fr_two_inv()) : v);
        }
        const size_t pos = prim_slot_pos<NC>(c, level - 1, sl.q);
        if (masked) z = Fr::add(z, Fr::sub(prf_fr(key_self, ctr + pos), prf_fr(key_prev, ctr + pos)));
        fe_store(za + pos, z);
    }
}

// the last, local step of every multiplicative item and its contribution to the round sums:
// partial[k] (ab sums of the affine part, TWO_INV pending) and partial[D + k] (additive sums of the products)
//   += eq(k) f(k) g(k)
template <int NC>
__global__ void __launch_bounds__(PT) k_primary_final(const fe* __restrict__ st, size_t cap, int n_instr, int n_mem, int D, int party,
                                                   const PrimInstrDev* __restrict__ instrs, const int* __restrict__ mul,
                                                   const uint32_t* __restrict__ item_idx, const uint32_t* __restrict__ item_slot, size_t n_items,
                                                   const uint32_t* __restrict__ bases, PrimLevelPtrs P, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe acc_ab = Fr::zero(), acc_ad = Fr::zero();
    const int k = blockIdx.y, X = k == 0 ? 0 : k + 1;
    const fe* eqp = st + (size_t)prim_slot_eq(n_instr, n_mem, NC) * cap;
    for (size_t j = (size_t)blockIdx.x * PT + threadIdx.x; j < n_items; j += (size_t)gridDim.x * PT) {
        PrimCtx<NC> c;
        c.st = st;
        c.cap = cap;
        c.n_instr = n_instr;
        c.n_mem = n_mem;
        c.party = party;
        c.D = D;
        c.s = (int)item_slot[j];
        const int ii = mul[c.s];
        c.in = instrs + ii;
        c.i = item_idx[j];
        c.jrel = (uint32_t)j - bases[PRIM_MAX_LEVELS * PRIM_MAX_MUL + c.s];
        c.bases = bases;
        c.P = P;
        c.k = k;
        c.X = X;
        const fe* fp = st + (size_t)prim_slot_flag(ii) * cap;
        fe f0 = fe_load(fp + 2 * c.i), f1 = fe_load(fp + 2 * c.i + 1);
        fe e0 = fe_load(eqp + 2 * c.i), e1 = fe_load(eqp + 2 * c.i + 1);
        fe df = Fr::sub(f1, f0), de = Fr::sub(e1, e0);
        fe fk = f0, ek = e0;
        for (int x = 0; x < X; x++) {
            fk = Fr::add(fk, df);
            ek = Fr::add(ek, de);
        }
        fe w = Fr::mul(fk, ek);
        if (c.in->fin_add.n || c.in->fin_add.c0) acc_ab = Fr::add(acc_ab, Fr::mul(sh_ab_sum<NC>(prim_lc<NC>(c, c.in->fin_add)), w));
        if (c.in->n_final) acc_ad = Fr::add(acc_ad, Fr::mul(prim_products<NC>(c, c.in->fin, c.in->n_final), w));
    }
    fe v = fr_block_sum(acc_ab, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)k * gridDim.x + blockIdx.x, v);
    v = fr_block_sum(acc_ad, sh4);
    if (threadIdx.x == 0) fe_store(partial + (size_t)(D + k) * gridDim.x + blockIdx.x, v);
}

// The instruction table compiled: the programs, which instructions are linear / multiplicative, the sumcheck degree and the deepest
// program.  The one copy behind cozk_primary_create and cozk_primary_plan (n_mem == 0: the plan has no memories to check against).
struct PrimTable {
    std::vector<PrimInstrDev> instrs;
    std::vector<int> lin, mul;
    int degree = 0, max_levels = 0;
};
static PrimTable prim_compile_table(const cozk_primary_instr* instrs, size_t n_instr, size_t n_mem, int party_id, bool rep3, const std::string& who) {
    PrimTable tb;
    int gdeg = 1;
    for (size_t i = 0; i < n_instr; i++) {
        const cozk_primary_instr& si = instrs[i];
        COZK_REQUIRE(si.form >= 0 && si.form <= COZK_G_ZERO && si.n_mems >= 1 && si.n_mems <= PRIM_MAX_MEMS, who + ": instruction form / memory count");
        for (int t = 0; t < si.n_mems; t++) COZK_REQUIRE(si.mems[t] >= 0 && (!n_mem || (size_t)si.mems[t] < n_mem), who + ": memory index out of range");
        PrimInstrDev d;
        prim_compile(si, party_id, rep3, d);
        if (d.linear) tb.lin.push_back((int)i);
        else tb.mul.push_back((int)i);
        if (d.g_degree > gdeg) gdeg = d.g_degree;
        if (d.n_levels > tb.max_levels) tb.max_levels = d.n_levels;
        tb.instrs.push_back(d);
    }
    COZK_REQUIRE(tb.mul.size() <= (size_t)PRIM_MAX_MUL, who + ": at most 32 multiplicative instructions");
    tb.degree = gdeg + 2;  // sumcheck_poly_degree (worker.rs:701-708)
    COZK_REQUIRE(tb.degree <= PRIM_MAX_DEG, who + ": degree too high");
    return tb;
}

// Item counts -> level sizes: first[q] .. first[n_mul] are the first items of the instruction groups and the total; level t holds, group
// after group, items x nq[t] x D elements.  hb (may be NULL) receives the groups' element offsets [t * PRIM_MAX_MUL + q].  The one copy
// behind cozk_primary_round_begin and cozk_primary_plan.
static void prim_level_layout(const std::vector<PrimInstrDev>& instrs, const std::vector<int>& mul, int max_levels, int D, const uint32_t* first,
                              uint32_t* hb, size_t level_elems[PRIM_MAX_LEVELS], const std::string& who) {
    for (int t = 0; t < PRIM_MAX_LEVELS; t++) level_elems[t] = 0;
    for (int t = 0; t < max_levels; t++) {
        uint64_t run = 0;
        for (size_t q = 0; q < mul.size(); q++) {
            if (hb) hb[t * PRIM_MAX_MUL + q] = (uint32_t)run;
            run += (uint64_t)(first[q + 1] - first[q]) * (uint64_t)instrs[(size_t)mul[q]].nq[t] * (uint64_t)D;
        }
        COZK_REQUIRE(run < (1ull << 32), who + ": level buffer exceeds 2^32 elements");
        level_elems[t] = (size_t)run;
    }
}

extern "C" {

int cozk_primary_create(cozk_ctx* ctx, int mode, int party_id, const cozk_primary_instr* instrs, size_t n_instr, const cozk_vec* const* flags,
                        const cozk_poly* const* E, size_t n_mem, const cozk_poly* lookup_outputs, const cozk_vec* eq, cozk_primary** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && instrs && n_instr > 0 && n_instr <= 64 && flags && E && n_mem > 0 && lookup_outputs && eq && out &&
                         (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3) && party_id >= 0 && party_id < 3,
                     "primary_create: bad argument");
        const size_t n = eq->n;
        COZK_REQUIRE(eq->kind == COZK_SCALAR_FR && n >= 2 && (n & (n - 1)) == 0, "primary_create: eq must be an FR vector of power-of-two length");
        COZK_REQUIRE(lookup_outputs->mode == mode && lookup_outputs->len == n && lookup_outputs->cur < 0, "primary_create: lookup_outputs shape / mode");
        // everything below may throw (argument checks of the instruction table, allocations): the guard frees what exists
        struct Guard {
            cozk_primary* p;
            ~Guard() { cozk_primary_free(p); }
        } guard{new cozk_primary()};
        cozk_primary* p = guard.p;
        p->ctx = ctx;
        p->d_instrs = nullptr;
        p->d_lin = p->d_mul = nullptr;
        p->d_act = p->d_item_idx = p->d_item_slot = p->d_bases = nullptr;
        p->d_live = nullptr;
        p->store[0] = p->store[1] = nullptr;
        for (int t = 0; t < PRIM_MAX_LEVELS; t++) p->P[t][0] = p->P[t][1] = nullptr;
        p->mode = mode;
        p->party = party_id;
        p->n_instr = (int)n_instr;
        p->n_mem = (int)n_mem;
        p->n0 = p->n = n;
        const int NC = mode == COZK_MODE_REP3 ? 2 : 1;
        p->T = (int)n_instr + NC * (int)n_mem + NC + 1;
        {
            PrimTable tb = prim_compile_table(instrs, n_instr, n_mem, party_id, mode == COZK_MODE_REP3, "primary_create");
            p->instrs = std::move(tb.instrs);
            p->lin = std::move(tb.lin);
            p->mul = std::move(tb.mul);
            p->degree = tb.degree;
            p->max_levels = tb.max_levels;
        }
        for (int w = 0; w < 2; w++) {
            p->cap[w] = w == 0 ? n : n / 2;
            p->store[w] = dev_alloc_fe((size_t)p->T * p->cap[w]);
        }
        p->cur = 0;
        // flags: 0/1 U8 columns (unbound) or FR vectors (already bound: the remaining rounds of a worker sub-net split)
        const bool flags_fr = flags[0] && flags[0]->kind == COZK_SCALAR_FR;
        if (flags_fr) {
            for (size_t i = 0; i < n_instr; i++) {
                COZK_REQUIRE(flags[i] && flags[i]->kind == COZK_SCALAR_FR && flags[i]->n == n, "primary_create: every flag vector has n entries of one kind");
                HIP_TRY(hipMemcpyAsync(p->store[0] + (size_t)prim_slot_flag((int)i) * n, flags[i]->d, n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            }
        } else {
            std::vector<const uint8_t*> cols(n_instr);
            for (size_t i = 0; i < n_instr; i++) {
                COZK_REQUIRE(flags[i] && flags[i]->kind == COZK_SCALAR_U8 && flags[i]->n == n, "primary_create: every flag column is a U8 vector of n entries");
                cols[i] = (const uint8_t*)flags[i]->d;
            }
            ctx->scratch2.reserve(n_instr * sizeof(void*));
            HIP_TRY(hipMemcpyAsync(ctx->scratch2.p, cols.data(), n_instr * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            dim3 gf(grid_for(n), (unsigned)n_instr);
            k_primary_flags_expand<<<gf, PT, 0, ctx->stream>>>((const uint8_t* const*)ctx->scratch2.p, n, p->cap[0], (int)n_instr, p->store[0]);
            HIP_TRY(hipGetLastError());
        }
        // E, lookup_outputs, eq: copies (the committed polynomials stay untouched for the openings) -- ONE gather launch over the
        // pointer table in its arguments instead of 2 x 54 + 3 device-to-device copies (108 blit kernels of 32 MiB at 1.6 TB/s each
        // cost 4.2 ms per 2^20-cycle proof)
        {
            PrimGatherTab tab;
            int nc = 0;
            auto add = [&](const fe* src, int slot) {
                COZK_REQUIRE(nc < PRIM_GATHER_MAX, "primary_create: too many columns for the gather table");
                tab.src[nc] = src;
                tab.slot[nc] = (uint32_t)slot;
                nc++;
            };
            for (size_t m = 0; m < n_mem; m++) {
                COZK_REQUIRE(E[m] && E[m]->mode == mode && E[m]->len == n && E[m]->cur < 0, "primary_create: E polynomial shape / mode");
                add(E[m]->a0, prim_slot_E((int)n_instr, (int)n_mem, (int)m, 0));
                if (NC == 2) add(E[m]->b0, prim_slot_E((int)n_instr, (int)n_mem, (int)m, 1));
            }
            add(lookup_outputs->a0, prim_slot_out((int)n_instr, (int)n_mem, NC, 0));
            if (NC == 2) add(lookup_outputs->b0, prim_slot_out((int)n_instr, (int)n_mem, NC, 1));
            add((const fe*)eq->d, prim_slot_eq((int)n_instr, (int)n_mem, NC));
            dim3 gg(grid_for(2 * n), (unsigned)nc);
            k_primary_gather<<<gg, PT, 0, ctx->stream>>>(tab, n, p->store[0]);
            HIP_TRY(hipGetLastError());
        }
        // tables
        p->d_instrs = (PrimInstrDev*)ctx_dev_alloc(ctx, p->instrs.size() * sizeof(PrimInstrDev));
        p->d_lin = (int*)ctx_dev_alloc(ctx, (p->lin.size() + 1) * sizeof(int));
        p->d_mul = (int*)ctx_dev_alloc(ctx, (p->mul.size() + 1) * sizeof(int));
        HIP_TRY(hipMemcpyAsync(p->d_instrs, p->instrs.data(), p->instrs.size() * sizeof(PrimInstrDev), hipMemcpyHostToDevice, ctx->stream));
        if (!p->lin.empty()) HIP_TRY(hipMemcpyAsync(p->d_lin, p->lin.data(), p->lin.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (!p->mul.empty()) HIP_TRY(hipMemcpyAsync(p->d_mul, p->mul.data(), p->mul.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        p->idx_cap = n / 2;
        p->d_act = (uint32_t*)ctx_dev_alloc(ctx, (p->mul.size() * p->idx_cap + 1) * sizeof(uint32_t) * 2);
        p->d_bases = (uint32_t*)ctx_dev_alloc(ctx, (size_t)(PRIM_MAX_LEVELS + 1) * PRIM_MAX_MUL * sizeof(uint32_t));
        p->d_live = (uint64_t*)ctx_dev_alloc(ctx, (p->idx_cap + 1) * sizeof(uint64_t));
        p->d_item_idx = p->d_item_slot = nullptr;
        p->items_cap = 0;
        p->n_items = 0;
        for (int t = 0; t < PRIM_MAX_LEVELS; t++) {
            p->P[t][0] = p->P[t][1] = nullptr;
            p->P_cap[t] = 0;
            p->level_elems[t] = 0;
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        guard.p = nullptr;
        *out = p;
    });
}

int cozk_primary_free(cozk_primary* p) {
    if (!p) return COZK_OK;
    cozk_ctx* ctx = p->ctx;
    for (int w = 0; w < 2; w++) ctx_dev_free(ctx, p->store[w]);
    ctx_dev_free(ctx, p->d_instrs);
    ctx_dev_free(ctx, p->d_lin);
    ctx_dev_free(ctx, p->d_mul);
    ctx_dev_free(ctx, p->d_act);
    ctx_dev_free(ctx, p->d_live);
    ctx_dev_free(ctx, p->d_bases);
    ctx_dev_free(ctx, p->d_item_idx);
    ctx_dev_free(ctx, p->d_item_slot);
    for (int t = 0; t < PRIM_MAX_LEVELS; t++)
        for (int c = 0; c < 2; c++) ctx_dev_free(ctx, p->P[t][c]);
    p->scan_tmp.release();
    delete p;
    return COZK_OK;
}

int cozk_primary_degree(const cozk_primary* p) { return p ? p->degree : 0; }
size_t cozk_primary_len(const cozk_primary* p) { return p ? p->n : 0; }
size_t cozk_primary_level_elems(const cozk_primary* p, int level) {
    return p && level >= 1 && level <= p->max_levels && p->n_items ? p->level_elems[level - 1] : 0;
}

// The public exchange plan: n_elems[PRIM_MAX_LEVELS * r + level - 1] of every round from the flag columns alone.  Instruction i is live
// at index j of round r iff one of the 2^(r + 1) cycles below j carries its flag (a bound flag is non-zero iff one of its pair was,
// up to a negligible probability): an OR pyramid over round 0's live masks, on the host -- the plan is made once, offline, over
// n_instr bytes per cycle.
int cozk_primary_plan(cozk_ctx* ctx, const cozk_primary_instr* instrs, size_t n_instr, const cozk_vec* const* flags, int log_n, uint64_t* n_elems_out,
                      uint64_t* total_out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && instrs && n_instr > 0 && n_instr <= 64 && flags && n_elems_out && total_out, "primary_plan: bad argument");
        COZK_REQUIRE(log_n >= 1 && log_n <= 30, "primary_plan: log_n out of range (1..30)");
        const size_t n = (size_t)1 << log_n;
        for (size_t i = 0; i < n_instr; i++)
            COZK_REQUIRE(flags[i] && flags[i]->kind == COZK_SCALAR_U8 && flags[i]->n == n, "primary_plan: every flag column is a U8 vector of 2^log_n entries");
        const PrimTable tb = prim_compile_table(instrs, n_instr, 0, 0, false, "primary_plan");
        std::vector<uint64_t> live(n / 2, 0);
        {
            std::vector<uint8_t> col(n);
            for (size_t i = 0; i < n_instr; i++) {
                HIP_TRY(hipMemcpyAsync(col.data(), flags[i]->d, n, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                for (size_t j = 0; j < n / 2; j++) live[j] |= (uint64_t)((col[2 * j] | col[2 * j + 1]) != 0) << i;
            }
        }
        uint64_t total = 0;
        size_t half = n / 2;
        for (int r = 0; r < log_n; r++) {
            if (r) {
                half /= 2;
                for (size_t j = 0; j < half; j++) live[j] = live[2 * j] | live[2 * j + 1];
            }
            uint32_t cnt[64] = {0}, first[PRIM_MAX_MUL + 1] = {0};
            for (size_t j = 0; j < half; j++)
                for (uint64_t m = live[j]; m; m &= m - 1) cnt[__builtin_ctzll(m)]++;
            for (size_t s = 0; s < tb.mul.size(); s++) first[s + 1] = first[s] + cnt[tb.mul[s]];
            size_t le[PRIM_MAX_LEVELS];
            prim_level_layout(tb.instrs, tb.mul, tb.max_levels, tb.degree, first, nullptr, le, "primary_plan");
            for (int t = 0; t < PRIM_MAX_LEVELS; t++) {
                n_elems_out[(size_t)PRIM_MAX_LEVELS * r + t] = le[t];
                total += le[t];
            }
        }
        *total_out = total;
    });
}

// first half of a round: bind everything with the previous challenge (NULL in the first round), the streaming pass over the
// linear instructions, and the item list of the multiplicative ones.  n_items x degree products per level follow.
int cozk_primary_round_begin(cozk_ctx* ctx, cozk_primary* p, const uint64_t* r, size_t* n_items, int* n_levels) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && n_items && n_levels, "primary_round_begin: bad argument");
        const int NC = p->mode == COZK_MODE_REP3 ? 2 : 1;
        // every check before the bind: a refused call leaves the primary as it was.  With two entries left the last
        // challenge belongs to cozk_primary_final_evals, a bind here would leave nothing to sum
        if (r) {
            COZK_REQUIRE(p->n >= 2, "primary_round_begin: fully bound");
            COZK_REQUIRE(p->n >= 4, "primary_round_begin: nothing left to sum");
        }
        COZK_REQUIRE(p->n >= 2, "primary_round_begin: nothing left to sum");
        COZK_REQUIRE(p->mul.size() * ((r ? p->n / 2 : p->n) / 2) < ((size_t)1 << 31), "primary sumcheck: activity array too long for the 32-bit item scan");
        if (r) {
            const int dst = 1 - p->cur;
            const size_t n_out = p->n / 2;
            dim3 g(grid_for(n_out), (unsigned)p->T);
            k_primary_bind<<<g, PT, 0, ctx->stream>>>(p->store[p->cur], p->cap[p->cur], p->store[dst], p->cap[dst], n_out, fe_from_u64x4(r));
            HIP_TRY(hipGetLastError());
            p->cur = dst;
            p->n = n_out;
        }
        const size_t half = p->n / 2;
        const fe* st = p->store[p->cur];
        const size_t cap = p->cap[p->cur];
        const int D = p->degree;
        // linear pass
        const unsigned gx = grid_capped(half, ROUND_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, 4, gx, 4);
        fe* partial = sl.partial;
        k_primary_mask<<<grid_for(half), PT, 0, ctx->stream>>>(st, cap, half, p->n_instr, p->d_live);
        uint64_t lin_bits = 0;  // the linear instructions as a bit set over the instruction indices (< 64: the live mask is one u64)
        for (int q : p->lin) lin_bits |= 1ull << q;
        if (NC == 2) k_primary_linear<2><<<gx, PT, 0, ctx->stream>>>(st, cap, half, p->n_instr, p->n_mem, D, p->d_instrs, lin_bits, p->d_live, partial);
        else k_primary_linear<1><<<gx, PT, 0, ctx->stream>>>(st, cap, half, p->n_instr, p->n_mem, D, p->d_instrs, lin_bits, p->d_live, partial);
        fe cf[4];
        finish_sums(ctx, sl, 4, gx, Fr::one(), 0, cf);
        for (int k = 0; k < D; k++) {  // the cubic at X = 0, 2, 3, .., D (Horner; X as a field element)
            const fe X = Fr::from_u64(k == 0 ? 0 : (uint64_t)k + 1);
            p->lin_sums[k] = Fr::add(cf[0], Fr::mul(X, Fr::add(cf[1], Fr::mul(X, Fr::add(cf[2], Fr::mul(X, cf[3]))))));
        }
        // item list of the multiplicative instructions, grouped by instruction
        p->n_items = 0;
        for (int t = 0; t < PRIM_MAX_LEVELS; t++) p->level_elems[t] = 0;
        const size_t n_mul = p->mul.size();
        if (n_mul) {
            dim3 ga(grid_for(half), (unsigned)n_mul);
            k_primary_active<<<ga, PT, 0, ctx->stream>>>(p->d_live, half, p->d_mul, p->d_act);
            const size_t n_act = n_mul * half;  // < 2^31: checked above
            uint32_t* off = p->d_act + n_mul * p->idx_cap + 1;
            size_t tmp_bytes = 0;
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, p->d_act, off, (int)n_act, ctx->stream));
            p->scan_tmp.reserve(tmp_bytes + 16);
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(p->scan_tmp.p, tmp_bytes, p->d_act, off, (int)n_act, ctx->stream));
            // first item of every instruction group + the total
            // ... gathered by one small kernel into the pinned slot (three strided device-to-host copies + a blocking sync before)
            uint32_t first[PRIM_MAX_MUL + 1], last_act = 0;
            {
                uint32_t* pin = (uint32_t*)ctx_pinned(ctx, (PRIM_MAX_MUL + 2) * sizeof(uint32_t));
                k_store_u32s<<<1, 64, 0, ctx->stream>>>(pin, off, off + n_act - 1, (int)n_mul, half);
                k_store_u32s<<<1, 64, 0, ctx->stream>>>(pin + n_mul + 1, p->d_act + n_act - 1, nullptr, 1, 1);
                HIP_TRY(hipGetLastError());
                stream_drain_by_flag(ctx);
                for (size_t q = 0; q <= n_mul; q++) first[q] = pin[q];
                last_act = pin[n_mul + 1];
            }
            first[n_mul] += last_act;
            p->n_items = first[n_mul];
            if (p->n_items > p->items_cap) {
                ctx_dev_free(ctx, p->d_item_idx);
                ctx_dev_free(ctx, p->d_item_slot);
                p->d_item_idx = (uint32_t*)ctx_dev_alloc(ctx, p->n_items * sizeof(uint32_t));
                p->d_item_slot = (uint32_t*)ctx_dev_alloc(ctx, p->n_items * sizeof(uint32_t));
                p->items_cap = p->n_items;
            }
            if (p->n_items) {
                k_primary_items<<<ga, PT, 0, ctx->stream>>>(p->d_act, off, half, p->d_item_idx, p->d_item_slot);
                HIP_TRY(hipGetLastError());
                // where every instruction group's reshared values live in the level buffers
                uint32_t hb[(PRIM_MAX_LEVELS + 1) * PRIM_MAX_MUL] = {0};
                prim_level_layout(p->instrs, p->mul, p->max_levels, D, first, hb, p->level_elems, "primary_round_begin");
                for (int t = 0; t < p->max_levels; t++) {
                    if (p->level_elems[t] > p->P_cap[t]) {
                        for (int c = 0; c < NC; c++) {
                            ctx_dev_free(ctx, p->P[t][c]);
                            p->P[t][c] = dev_alloc_fe(p->level_elems[t]);
                        }
                        p->P_cap[t] = p->level_elems[t];
                    }
                }
                for (size_t q = 0; q < n_mul; q++) hb[PRIM_MAX_LEVELS * PRIM_MAX_MUL + q] = first[q];
                PrimBasesTab tab;  // the table travels in the kernel arguments: no upload, no sync
                memcpy(tab.v, hb, sizeof(hb));
                k_primary_store_bases<<<1, 256, 0, ctx->stream>>>(tab, p->d_bases);
                HIP_TRY(hipGetLastError());
            }
        }
        *n_items = p->n_items;
        *n_levels = p->n_items ? p->max_levels : 0;
    });
}

// multiplication level `level` (1 .. n_levels): the local half of the batched mul_vec of all items.  Returns the device
// buffers of the exchange: *send = this party's new additive shares (n = n_items * degree elements), *recv = where the
// previous party's must land (Rep3; the host runs the ring reshare between this call and the next).  PLAIN: no exchange.
int cozk_primary_level(cozk_ctx* ctx, cozk_primary* p, int level, const uint8_t* key_self, const uint8_t* key_prev, uint64_t counter, const void** send,
                       void** recv, size_t* n_elems) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && level >= 1 && level <= p->max_levels && p->n_items, "primary_level: bad level / no items");
        const bool rep3 = p->mode == COZK_MODE_REP3;
        COZK_REQUIRE(!rep3 || (key_self && key_prev), "primary_level: PRF keys required");
        prf_key ks{}, kp{};
        if (rep3) {
            ks = prf_key_from_bytes(key_self);
            kp = prf_key_from_bytes(key_prev);
        }
        const fe* st = p->store[p->cur];
        const size_t cap = p->cap[p->cur];
        const size_t n_el = p->level_elems[level - 1];
        if (n_el) {
            PrimLevelPtrs P{};
            for (int t = 0; t < PRIM_MAX_LEVELS; t++) {
                P.a[t] = p->P[t][0];
                P.b[t] = p->P[t][1];
            }
            if (rep3)
                k_primary_level<2><<<dim3(grid_for(p->n_items), (unsigned)p->degree), PT, 0, ctx->stream>>>(st, cap, p->n_instr, p->n_mem, p->degree, p->party, p->d_instrs, p->d_mul,
                                                                                  p->d_item_idx, p->d_item_slot, p->n_items, level, p->d_bases, P,
                                                                                  p->P[level - 1][0], 1, ks, kp, counter);
            else
                k_primary_level<1><<<dim3(grid_for(p->n_items), (unsigned)p->degree), PT, 0, ctx->stream>>>(st, cap, p->n_instr, p->n_mem, p->degree, p->party, p->d_instrs, p->d_mul,
                                                                                  p->d_item_idx, p->d_item_slot, p->n_items, level, p->d_bases, P,
                                                                                  p->P[level - 1][0], 0, ks, kp, 0);
            HIP_TRY(hipGetLastError());
        }
        if (send) *send = p->P[level - 1][0];
        if (recv) *recv = rep3 ? p->P[level - 1][1] : nullptr;
        if (n_elems) *n_elems = n_el;
    });
}

// second half of a round: the local last step of the multiplicative items; out = degree x 4 u64: this party's additive
// evaluations at X = 0, 2, 3, .., degree
int cozk_primary_round_finish(cozk_ctx* ctx, cozk_primary* p, uint64_t* out_evals) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && out_evals, "primary_round_finish: bad argument");
        const int D = p->degree;
        const bool rep3 = p->mode == COZK_MODE_REP3;
        fe ab[PRIM_MAX_DEG], ad[PRIM_MAX_DEG];
        for (int k = 0; k < D; k++) {
            ab[k] = p->lin_sums[k];
            ad[k] = Fr::zero();
        }
        if (p->n_items) {
            const fe* st = p->store[p->cur];
            const size_t cap = p->cap[p->cur];
            const unsigned gx = grid_capped(p->n_items, ROUND_GRID_MAX);
            const SumLaunch sl = sum_launch(ctx, 2 * D, gx, 2 * D);
            fe* partial = sl.partial;
            PrimLevelPtrs P{};
            for (int t = 0; t < PRIM_MAX_LEVELS; t++) {
                P.a[t] = p->P[t][0];
                P.b[t] = p->P[t][1];
            }
            if (rep3)
                k_primary_final<2><<<dim3(gx, (unsigned)D), PT, 0, ctx->stream>>>(st, cap, p->n_instr, p->n_mem, D, p->party, p->d_instrs, p->d_mul, p->d_item_idx, p->d_item_slot, p->n_items,
                                                                p->d_bases, P, partial);
            else
                k_primary_final<1><<<dim3(gx, (unsigned)D), PT, 0, ctx->stream>>>(st, cap, p->n_instr, p->n_mem, D, p->party, p->d_instrs, p->d_mul, p->d_item_idx, p->d_item_slot, p->n_items,
                                                                p->d_bases, P, partial);
            fe s[2 * PRIM_MAX_DEG];
            finish_sums(ctx, sl, 2 * D, gx, Fr::one(), 0, s);
            for (int k = 0; k < D; k++) {
                ab[k] = Fr::add(ab[k], s[k]);
                ad[k] = s[D + k];
            }
        }
        for (int k = 0; k < D; k++) {
            fe v = rep3 ? Fr::mul(ab[k], fr_two_inv()) : ab[k];  // into_additive of the (a + b) sums
            fe_to_u64x4(Fr::add(v, ad[k]), out_evals + 4 * k);
        }
    });
}

// after the last round: bind with the last challenge and read the final claims (worker.rs:427-452): E(r) as shares
// (n_mem x (a[4], b[4])), the flags (n_instr x 4, public), lookup_outputs(r) (a[4], b[4]) and eq(r)
int cozk_primary_final_evals(cozk_ctx* ctx, cozk_primary* p, const uint64_t r[4], uint64_t* E_evals, uint64_t* flag_evals, uint64_t out_eval[8],
                             uint64_t eq_eval[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && p && r && E_evals && flag_evals && out_eval && p->n == 2, "primary_final_evals: one unbound variable must be left");
        const int NC = p->mode == COZK_MODE_REP3 ? 2 : 1;
        const int dst = 1 - p->cur;
        dim3 g(1, (unsigned)p->T);
        k_primary_bind<<<g, PT, 0, ctx->stream>>>(p->store[p->cur], p->cap[p->cur], p->store[dst], p->cap[dst], 1, fe_from_u64x4(r));
        HIP_TRY(hipGetLastError());
        p->cur = dst;
        p->n = 1;
        std::vector<fe> h((size_t)p->T);
        HIP_TRY(hipMemcpy2DAsync(h.data(), sizeof(fe), p->store[dst], p->cap[dst] * sizeof(fe), sizeof(fe), (size_t)p->T, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < p->n_instr; i++) fe_to_u64x4(h[prim_slot_flag(i)], flag_evals + 4 * i);
        for (int m = 0; m < p->n_mem; m++) {
            fe_to_u64x4(h[prim_slot_E(p->n_instr, p->n_mem, m, 0)], E_evals + 8 * m);
            fe_to_u64x4(NC == 2 ? h[prim_slot_E(p->n_instr, p->n_mem, m, 1)] : Fr::zero(), E_evals + 8 * m + 4);
        }
        fe_to_u64x4(h[prim_slot_out(p->n_instr, p->n_mem, NC, 0)], out_eval);
        fe_to_u64x4(NC == 2 ? h[prim_slot_out(p->n_instr, p->n_mem, NC, 1)] : Fr::zero(), out_eval + 4);
        if (eq_eval) fe_to_u64x4(h[prim_slot_eq(p->n_instr, p->n_mem, NC)], eq_eval);
    });
}

}  // extern "C"
