// The output check of the read-write memory proof (prove_outputs, co-jolt/src/jolt/vm/read_write_memory/worker.rs:110-175) from the
// compact columns -- part of poly.hip's translation unit (co_mac / co_add / co_reduce of compact_open.inc, k_prod_round, k_fold_halves).
//
//   sum_x eq(r_eq, x) * io_range(x) * (v_final(x) - v_io(x)) = 0,   degree 3, HighToLow
//
// as cozk_output_check_create / _round / _final: every round's evaluations at X = 0, 2, 3 and the three final values, byte for byte
// what cozk_prod_sumcheck_evals / cozk_poly_bind / cozk_poly_get_coeff give on Fr copies of the three MEM-entry vectors, without
// those copies.  MEM = 2^m, the io window is [lo, hi) of W words, W' = 2^lw the power of two at or above W, variable i is index bit
// m-1-i, round k binds variable k, n_k = 2^(m-k), h = n_k / 2.  d[x] = v_final[x] - v_io[x - lo] inside the window, v_final[x] outside.
//
// Sparse rounds (h >= W', rounds 0 .. m-lw-1): no two window words are partners, the window holds at most one multiple c of W' and so
// has at most two sides [lo, c), [c, hi) whose words share their index bits above lw.  On side s the bound range is ONE scalar
// rho[s] = prod_{i<k} (bit_i(s) ? r_i : 1 - r_i), the upper eq bits ONE scalar H[s] = prod_{i=k+1}^{m-lw-1} eq1(r_eq[i], bit_i(s)), the
// low eq bits the table Llow = eq_evals(r_eq[m-lw..m)) of W' entries, and with c_k = prod_{i<k} eq1(r_eq[i], r_i),
// l_k(t) = (1 - r_eq[k])(1 - t) + r_eq[k] t, w_s(t) = bit_k(s) ? t : 1 - t,
//     s_k(t) = c_k l_k(t) sum_s H[s] rho[s] w_s(t) (A_s + t (B_s - A_s)),
//     A_s = sum_{x in side s} Llow[x mod W'] D_k[x mod h],   B_s the same at (x mod h) + h.
// The device makes the dots, the host the scalars.  eq is never a table of MEM entries and is never bound; the range is never a vector.
// Only d is folded whole (v_final(r) depends on every word): the first fold D_1[y] = (1 - r_0) d[y] + r_0 d[y + h] comes straight from
// the U32 columns, later folds are k_fold_halves in place.  After round m-lw-1 the length is W': E = c Llow, R = rho[s] on side s's
// positions mod W', D as folded, and the remaining lw rounds are the dense product sumcheck on W'-entry vectors (k_prod_round,
// k_oc_bind3).  W' = MEM: no sparse round, d is materialised once and everything is the dense tail.
//
// Kernels and their algorithmic bytes (W the window, h the half length, 32-byte Fr):
//   k_oc_dots_u32     round 0: per side sum Llow v_final[y], sum Llow v_final[y + h], sum Llow v_io       reads W (32 + 12) B
//   k_oc_first_fold   D_1 from the columns                                               reads MEM 4 B (+ W 4 B), writes MEM / 2 * 32 B
//   k_oc_dots_fr      rounds 1 .. m-lw-1: per side A_s, B_s on the Fr fold                                  reads W 96 B
//   k_fold_halves     the later folds, in place                                                   reads n_k 32 B, writes n_k / 2 * 32 B
//   k_oc_tail_init    E = c Llow in place, R from rho                                                      reads W' 32 B, writes W' 64 B
//   k_oc_materialise  W' = MEM: d and the range as Fr                                               reads MEM 4 B (+ W 4 B), writes MEM 64 B
//   k_oc_bind3        the dense tail's bind of E, R, D in place (one launch)                  reads 3 n_k 32 B, writes 3 n_k / 2 * 32 B
// Launch shape: a round is its fold (one launch), its dots (one launch) and k_finish_sums; the fold is NOT fused with the next round's
// dots: the dots read W scattered entries of the folded array and end in a grid-wide sum, the fold writes n_k / 2 entries with no
// reduction, and a fused kernel would need the fold's whole grid to finish before the dots' W entries exist -- a grid barrier for one
// saved launch.  Grids come from the element count: the fold and the elementwise kernels one lane per entry, the dots grid_capped over
// the window (CO_LANE_TERMS terms per lane for the exact sums, as k_compact_eval_chi; BATCH_GRID_MAX workgroups at most).
//
// Exact sums: Llow[.] and the fold's (1 - r), r are Montgomery forms, a column word is a plain integer below 2^32, so their integer
// product is the Montgomery form of the field product and a sum of such products is reduced ONCE (co_reduce).  The v_io terms go to a
// second non-negative accumulator and the two are subtracted in the field.  k_oc_first_fold adds at most two terms below 2^288 each
// per accumulator: a sum below 2^289, limb 9 <= 1 and limb 10 = 0 of CO_LIMBS = 11 (tests/output_check_ref.py first_fold_words asserts
// it); k_oc_dots_u32 adds at most W < 2^32 terms per accumulator over a lane, a wave and a workgroup: below 2^320 < 2^352.
//
// Device memory of a handle (from the context's pool, allocated in create, nothing later): lw < m: MEM / 2 Fr entries for the folds
// plus two W'-entry Fr vectors (Llow, which becomes E, and R); lw == m: three MEM-entry Fr vectors (the dense composition's).  No Fr
// vector of MEM entries exists unless W' = MEM.  v_final and v_io are only read and must outlive the handle.
//
// The shared form (cozk_output_check_shared_create): v_final is a polynomial, PLAIN (one Fr component a) or a party's REP3 share (a, b).
// Everything the check sends is linear in the share and a party's message is the additive share (a + b) 2^-1 (into_additive; k_prod_round<2, M>
// with finish_sums' TWO_INV), so the party needs ONE Fr vector
//     T[x] = a[x] + b[x] (REP3), a[x] (PLAIN);   d[x] = T[x] - sub v_io[x - lo] inside the window, T[x] outside,
// sub = 1 for PLAIN and REP3 parties 0 and 1, 0 for REP3 party 2: cozk_poly_linear_combination puts a public term into party 0's a and
// party 1's b, so a + b loses v_io once for parties 0 and 1 and never for party 2; over the three parties the sum is 2 (v_final - v_io).
// On d everything above applies unchanged; for REP3 the host multiplies the three round values and d's final value by 2^-1.  Every value
// is canonical, so a party's bytes are those of cozk_prod_sumcheck_evals / cozk_poly_bind / into_additive on the dense polynomials.
//   k_ocs_dots0<NC>        round 0: per side sum Llow T[y], sum Llow T[y + h] (Fr::mul), sum Llow v_io (exact)   reads W (32 + NC 64 + 4) B
//   k_ocs_first_fold<NC>   D_1 from the components                              reads MEM NC 32 B (+ W 4 B), writes MEM / 2 * 32 B
//   k_ocs_materialise<NC>  W' = MEM: d and the range as Fr                              reads MEM NC 32 B (+ W 4 B), writes MEM 64 B
// NC the components; every later round runs the kernels above on the Fr fold.  With sub = 0 no v_io entry is read and the kernels get a
// null v_io: the branch is uniform over the launch (as pub_a / pub_b of k_bc_if_leaves).  The exact v_io row of k_ocs_dots0 adds fewer
// than 2^32 terms below 2^288 each: below 2^320 in CO_LIMBS = 11 limbs; k_ocs_first_fold's at most two terms stay below 2^289.

struct OcSides {
    size_t lo[2], hi[2];  // side s = [lo[s], hi[s]); an unused side is empty
};

struct cozk_output_check {
    cozk_ctx* ctx = nullptr;
    const uint32_t *vf = nullptr, *vio = nullptr;  // borrowed
    const fe *ta = nullptr, *tb = nullptr;         // the shared form: v_final's components, borrowed (tb null: one component); vf is null
    bool sub = true;                               // the shared form: this party's d loses v_io inside the window
    bool rep3 = false;                             // REP3: the round values and d's final value are times 2^-1
    int m = 0, lw = 0, k = 0;                      // k variables are bound
    bool started = false;                          // round 0 has been asked for
    size_t lo = 0, hi = 0, len = 0;                // len = 2^(m - k)
    int nside = 0;
    OcSides sides{};
    std::vector<fe> r_eq;
    fe c, rho[2];
    fe *D = nullptr, *E = nullptr, *Rg = nullptr;
    bool d_is_cols = true;  // no fold yet: d is the two columns
};

// raw[wave][q] += this wave's sum of acc[q], then the first NQ lanes of the workgroup reduce one sum each (k_compact_eval_chi's ending)
template <int NQ>
static __device__ __forceinline__ void oc_exact_block_sums(uint32_t (&acc)[NQ][CO_LIMBS], uint32_t (&raw)[PT / 64][NQ][CO_LIMBS], fe* __restrict__ partial,
                                                           size_t row0) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
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
    if ((int)threadIdx.x < NQ) {
        uint32_t s[CO_LIMBS], o[CO_LIMBS];
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) s[l] = raw[0][threadIdx.x][l];
#pragma unroll
        for (int w = 1; w < PT / 64; w++) {
#pragma unroll
            for (int l = 0; l < CO_LIMBS; l++) o[l] = raw[w][threadIdx.x][l];
            co_add(s, o);
        }
        fe_store(partial + (row0 + threadIdx.x) * gridDim.x + blockIdx.x, co_reduce(s));
    }
}

// round 0.  Side s = blockIdx.y: partial rows 3 s + {0, 1, 2} = sum Llow[x mod W'] {v_final[x mod h], v_final[(x mod h) + h], v_io[x - lo]}
// over the side's words x.  x < MEM = 2 h, so (x mod h) + h < MEM; x - lo < W; x mod W' < W'.
__global__ void __launch_bounds__(PT) k_oc_dots_u32(const uint32_t* __restrict__ vf, const uint32_t* __restrict__ vio, const fe* __restrict__ Llow, size_t lo,
                                                    OcSides sides, size_t h, size_t wmask, fe* __restrict__ partial) {
    __shared__ uint32_t raw[PT / 64][3][CO_LIMBS];
    uint32_t acc[3][CO_LIMBS];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) acc[q][l] = 0;
    const size_t end = sides.hi[blockIdx.y];
    for (size_t x = sides.lo[blockIdx.y] + (size_t)blockIdx.x * PT + threadIdx.x; x < end; x += (size_t)gridDim.x * PT) {
        const fe L = fe_load(Llow + (x & wmask));
        const size_t y = x & (h - 1);
        co_mac<0>(acc[0], L, vf[y]);
        co_mac<0>(acc[1], L, vf[y + h]);
        co_mac<0>(acc[2], L, vio[x - lo]);
    }
    oc_exact_block_sums<3>(acc, raw, partial, 3 * (size_t)blockIdx.y);
}

// D_1[y] = (1 - r) d[y] + r d[y + h], y < h = MEM / 2, from the columns: a = 1 - r, b = r (Montgomery).  At most two terms per accumulator.
__global__ void __launch_bounds__(PT) k_oc_first_fold(const uint32_t* __restrict__ vf, const uint32_t* __restrict__ vio, size_t lo, size_t hi, size_t h, fe a, fe b,
                                                      fe* __restrict__ D) {
    const size_t y = (size_t)blockIdx.x * PT + threadIdx.x;
    if (y >= h) return;
    uint32_t pos[CO_LIMBS];
#pragma unroll
    for (int l = 0; l < CO_LIMBS; l++) pos[l] = 0;
    co_mac<0>(pos, a, vf[y]);
    co_mac<0>(pos, b, vf[y + h]);
    fe v = co_reduce(pos);
    const bool in_lo = y >= lo && y < hi, in_hi = y + h >= lo && y + h < hi;
    if (in_lo || in_hi) {
        uint32_t neg[CO_LIMBS];
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) neg[l] = 0;
        if (in_lo) co_mac<0>(neg, a, vio[y - lo]);
        if (in_hi) co_mac<0>(neg, b, vio[y + h - lo]);
        v = Fr::sub(v, co_reduce(neg));
    }
    fe_store(D + y, v);
}

// rounds 1 .. m-lw-1.  Side s = blockIdx.y: partial rows 2 s + {0, 1} = A_s, B_s over the Fr fold D of 2 h entries
__global__ void __launch_bounds__(PT) k_oc_dots_fr(const fe* __restrict__ D, const fe* __restrict__ Llow, OcSides sides, size_t h, size_t wmask,
                                                   fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe A = Fr::zero(), B = Fr::zero();
    const size_t end = sides.hi[blockIdx.y];
    for (size_t x = sides.lo[blockIdx.y] + (size_t)blockIdx.x * PT + threadIdx.x; x < end; x += (size_t)gridDim.x * PT) {
        const fe L = fe_load(Llow + (x & wmask));
        const size_t y = x & (h - 1);
        A = Fr::add(A, Fr::mul(L, fe_load(D + y)));
        B = Fr::add(B, Fr::mul(L, fe_load(D + y + h)));
    }
    const fe sa = fr_block_sum(A, sh4);
    if (threadIdx.x == 0) fe_store(partial + (2 * (size_t)blockIdx.y) * gridDim.x + blockIdx.x, sa);
    const fe sb = fr_block_sum(B, sh4);
    if (threadIdx.x == 0) fe_store(partial + (2 * (size_t)blockIdx.y + 1) * gridDim.x + blockIdx.x, sb);
}

// ---- the shared form: v_final as NC Fr components, T = a (+ b)
template <int NC>
static __device__ __forceinline__ fe ocs_T(const fe* __restrict__ ta, const fe* __restrict__ tb, size_t x) {
    const fe a = fe_load(ta + x);
    if (NC == 1) return a;
    return Fr::add(a, fe_load(tb + x));
}

// round 0.  Side s = blockIdx.y: partial rows 3 s + {0, 1, 2} = sum Llow[x mod W'] {T[x mod h], T[(x mod h) + h], v_io[x - lo]} over the
// side's words x; the T rows as k_oc_dots_fr, the v_io row exact as k_oc_dots_u32 (0 with sub = 0: vio is null and is not read).
// x < MEM = 2 h, so (x mod h) + h < MEM; x - lo < W; x mod W' < W'.
template <int NC>
__global__ void __launch_bounds__(PT) k_ocs_dots0(const fe* __restrict__ ta, const fe* __restrict__ tb, const uint32_t* __restrict__ vio, int sub,
                                                  const fe* __restrict__ Llow, size_t lo, OcSides sides, size_t h, size_t wmask, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ uint32_t raw[PT / 64][1][CO_LIMBS];
    fe A = Fr::zero(), B = Fr::zero();
    uint32_t acc[1][CO_LIMBS];
#pragma unroll
    for (int l = 0; l < CO_LIMBS; l++) acc[0][l] = 0;
    const size_t end = sides.hi[blockIdx.y];
    for (size_t x = sides.lo[blockIdx.y] + (size_t)blockIdx.x * PT + threadIdx.x; x < end; x += (size_t)gridDim.x * PT) {
        const fe L = fe_load(Llow + (x & wmask));
        const size_t y = x & (h - 1);
        A = Fr::add(A, Fr::mul(L, ocs_T<NC>(ta, tb, y)));
        B = Fr::add(B, Fr::mul(L, ocs_T<NC>(ta, tb, y + h)));
        if (sub) co_mac<0>(acc[0], L, vio[x - lo]);
    }
    const fe sa = fr_block_sum(A, sh4);
    if (threadIdx.x == 0) fe_store(partial + (3 * (size_t)blockIdx.y) * gridDim.x + blockIdx.x, sa);
    const fe sb = fr_block_sum(B, sh4);
    if (threadIdx.x == 0) fe_store(partial + (3 * (size_t)blockIdx.y + 1) * gridDim.x + blockIdx.x, sb);
    oc_exact_block_sums<1>(acc, raw, partial, 3 * (size_t)blockIdx.y + 2);
}

// D_1[y] = T[y] + r (T[y + h] - T[y]) minus the window terms (1 - r) v_io[y - lo] where y is in the window and r v_io[y + h - lo] where
// y + h is, y < h = MEM / 2: a = 1 - r, b = r (Montgomery).  One lane per entry; y + h < 2 h = MEM, and an index into v_io is taken only
// inside [lo, hi), so it is below W.  sub = 0: no window term (vio is null and is not read).
template <int NC>
__global__ void __launch_bounds__(PT) k_ocs_first_fold(const fe* __restrict__ ta, const fe* __restrict__ tb, const uint32_t* __restrict__ vio, int sub, size_t lo,
                                                       size_t hi, size_t h, fe a, fe b, fe* __restrict__ D) {
    const size_t y = (size_t)blockIdx.x * PT + threadIdx.x;
    if (y >= h) return;
    const fe t0 = ocs_T<NC>(ta, tb, y), t1 = ocs_T<NC>(ta, tb, y + h);
    fe v = Fr::add(t0, Fr::mul(Fr::sub(t1, t0), b));
    const bool in_lo = y >= lo && y < hi, in_hi = y + h >= lo && y + h < hi;
    if (sub && (in_lo || in_hi)) {
        uint32_t neg[CO_LIMBS];
#pragma unroll
        for (int l = 0; l < CO_LIMBS; l++) neg[l] = 0;
        if (in_lo) co_mac<0>(neg, a, vio[y - lo]);
        if (in_hi) co_mac<0>(neg, b, vio[y + h - lo]);
        v = Fr::sub(v, co_reduce(neg));
    }
    fe_store(D + y, v);
}

// W' = MEM: D[x] = d[x], R[x] = io_range(x) as Fr; x < n = MEM, and x - lo < W inside the window
template <int NC>
__global__ void __launch_bounds__(PT) k_ocs_materialise(const fe* __restrict__ ta, const fe* __restrict__ tb, const uint32_t* __restrict__ vio, int sub, size_t lo,
                                                        size_t hi, size_t n, fe* __restrict__ D, fe* __restrict__ Rg) {
    const size_t x = (size_t)blockIdx.x * PT + threadIdx.x;
    if (x >= n) return;
    const bool in = x >= lo && x < hi;
    fe v = ocs_T<NC>(ta, tb, x);
    if (sub && in) v = Fr::sub(v, Fr::from_u64(vio[x - lo]));
    fe_store(D + x, v);
    fe_store(Rg + x, in ? Fr::one() : Fr::zero());
}

// a side lies inside one W'-aligned block: its positions mod W' are [lo mod W', lo mod W' + (hi - lo))
static __device__ __forceinline__ int oc_side_at(const OcSides& sides, size_t i, size_t wmask) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const size_t p = sides.lo[s] & wmask;
        if (i >= p && i - p < sides.hi[s] - sides.lo[s]) return s;
    }
    return -1;
}

// the dense tail begins (length n = W'): E = c Llow in place, R[i] = rho[s] on side s's positions, 0 elsewhere
__global__ void __launch_bounds__(PT) k_oc_tail_init(fe* __restrict__ E, fe* __restrict__ Rg, fe c, fe rho0, fe rho1, OcSides sides, size_t n) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe_store(E + i, Fr::mul(c, fe_load(E + i)));
    const int s = oc_side_at(sides, i, n - 1);
    fe_store(Rg + i, s < 0 ? Fr::zero() : (s ? rho1 : rho0));
}

// W' = MEM: D[x] = d[x], R[x] = io_range(x) as Fr
__global__ void __launch_bounds__(PT) k_oc_materialise(const uint32_t* __restrict__ vf, const uint32_t* __restrict__ vio, size_t lo, size_t hi, size_t n,
                                                       fe* __restrict__ D, fe* __restrict__ Rg) {
    const size_t x = (size_t)blockIdx.x * PT + threadIdx.x;
    if (x >= n) return;
    const bool in = x >= lo && x < hi;
    fe v = Fr::from_u64(vf[x]);
    if (in) v = Fr::sub(v, Fr::from_u64(vio[x - lo]));
    fe_store(D + x, v);
    fe_store(Rg + x, in ? Fr::one() : Fr::zero());
}

// the dense tail's bind, HighToLow in place: lane i reads (i, i + n_out) and writes i, of array blockIdx.y
struct OcTriple {
    fe* p[3];
};
__global__ void __launch_bounds__(PT) k_oc_bind3(OcTriple t, size_t n_out, fe r) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    fe* v = t.p[blockIdx.y];
    const fe lo = fe_load(v + i), hi = fe_load(v + i + n_out);
    fe_store(v + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
}

__global__ void k_oc_final(const fe* __restrict__ E, const fe* __restrict__ Rg, const fe* __restrict__ D, fe* __restrict__ res) {
    fe_store(res, fe_load(E));
    fe_store(res + 1, fe_load(Rg));
    fe_store(res + 2, fe_load(D));
}

static inline int oc_bit(const cozk_output_check* oc, int s, int i) { return (int)((oc->sides.lo[s] >> (oc->m - 1 - i)) & 1); }
static inline bool oc_sparse(const cozk_output_check* oc) { return oc->k < oc->m - oc->lw; }
static inline fe oc_eq1(const fe& a, const fe& b) {  // a b + (1 - a)(1 - b)
    const fe one = Fr::one();
    return Fr::add(Fr::mul(a, b), Fr::mul(Fr::sub(one, a), Fr::sub(one, b)));
}
static inline unsigned oc_longest_side(const cozk_output_check* oc, size_t per_lane) {
    size_t w = 0;
    for (int s = 0; s < oc->nside; s++) w = std::max(w, oc->sides.hi[s] - oc->sides.lo[s]);
    return grid_capped((w + per_lane - 1) / per_lane, BATCH_GRID_MAX);
}

static void oc_release(cozk_output_check* oc) {
    for (fe* p : {oc->D, oc->E, oc->Rg}) ctx_dev_free(oc->ctx, p);
    oc->D = oc->E = oc->Rg = nullptr;
}

// the round polynomial at X = 0, 2, 3 in the handle's state
static void oc_round_evals(cozk_output_check* oc, uint64_t out[12]) {
    cozk_ctx* ctx = oc->ctx;
    const size_t h = oc->len / 2;
    fe ev[3];
    if (!oc_sparse(oc)) {
        const unsigned gx = grid_capped(h, BATCH_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, 4, gx, 3);
        ProdRoundPtrs tab{};
        tab.a[0] = oc->E, tab.a[1] = oc->Rg, tab.a[2] = oc->D;
        k_prod_round<1, 3><<<gx, PT, 0, ctx->stream>>>(tab, -1, h, 3, sl.partial);
        HIP_TRY(hipGetLastError());
        finish_sums(ctx, sl, 3, gx, oc->rep3 ? fr_two_inv() : Fr::one(), oc->rep3 ? 1 : 0, ev);
    } else {
        const int k = oc->k;
        const size_t wmask = ((size_t)1 << oc->lw) - 1;
        fe A[2] = {Fr::zero(), Fr::zero()}, B[2] = {Fr::zero(), Fr::zero()};
        if (oc->d_is_cols) {
            const unsigned gx = oc_longest_side(oc, oc->ta ? 1 : CO_LANE_TERMS);  // the shared form's T rows are k_oc_dots_fr's
            const SumLaunch sl = sum_launch(ctx, 6, gx, 6);
            const uint32_t* vio = oc->sub ? oc->vio : nullptr;
            if (oc->tb) k_ocs_dots0<2><<<dim3(gx, 2), PT, 0, ctx->stream>>>(oc->ta, oc->tb, vio, oc->sub, oc->E, oc->lo, oc->sides, h, wmask, sl.partial);
            else if (oc->ta) k_ocs_dots0<1><<<dim3(gx, 2), PT, 0, ctx->stream>>>(oc->ta, nullptr, vio, oc->sub, oc->E, oc->lo, oc->sides, h, wmask, sl.partial);
            else k_oc_dots_u32<<<dim3(gx, 2), PT, 0, ctx->stream>>>(oc->vf, oc->vio, oc->E, oc->lo, oc->sides, h, wmask, sl.partial);
            HIP_TRY(hipGetLastError());
            fe s[6];
            finish_sums(ctx, sl, 6, gx, Fr::one(), 0, s);
            for (int sd = 0; sd < oc->nside; sd++) {  // the window's own half loses the v_io sum (0 in the shared form with sub = 0)
                const bool up = oc_bit(oc, sd, 0) != 0;
                A[sd] = up ? s[3 * sd] : Fr::sub(s[3 * sd], s[3 * sd + 2]);
                B[sd] = up ? Fr::sub(s[3 * sd + 1], s[3 * sd + 2]) : s[3 * sd + 1];
            }
        } else {
            const unsigned gx = oc_longest_side(oc, 1);
            const SumLaunch sl = sum_launch(ctx, 4, gx, 4);
            k_oc_dots_fr<<<dim3(gx, 2), PT, 0, ctx->stream>>>(oc->D, oc->E, oc->sides, h, wmask, sl.partial);
            HIP_TRY(hipGetLastError());
            fe s[4];
            finish_sums(ctx, sl, 4, gx, Fr::one(), 0, s);
            for (int sd = 0; sd < oc->nside; sd++) A[sd] = s[2 * sd], B[sd] = s[2 * sd + 1];
        }
        const fe one = Fr::one();
        fe HR[2];
        for (int sd = 0; sd < oc->nside; sd++) {
            fe H = one;
            for (int i = k + 1; i < oc->m - oc->lw; i++) H = Fr::mul(H, oc_bit(oc, sd, i) ? oc->r_eq[(size_t)i] : Fr::sub(one, oc->r_eq[(size_t)i]));
            HR[sd] = Fr::mul(H, oc->rho[sd]);
        }
        const uint64_t ts[3] = {0, 2, 3};
        for (int e = 0; e < 3; e++) {
            const fe t = Fr::from_u64(ts[e]), omt = Fr::sub(one, t);
            const fe l = Fr::add(Fr::mul(Fr::sub(one, oc->r_eq[(size_t)k]), omt), Fr::mul(oc->r_eq[(size_t)k], t));
            fe acc = Fr::zero();
            for (int sd = 0; sd < oc->nside; sd++) {
                const fe line = Fr::add(A[sd], Fr::mul(t, Fr::sub(B[sd], A[sd])));
                acc = Fr::add(acc, Fr::mul(Fr::mul(HR[sd], oc_bit(oc, sd, k) ? t : omt), line));
            }
            ev[e] = Fr::mul(Fr::mul(oc->c, l), acc);
            if (oc->rep3) ev[e] = Fr::mul(ev[e], fr_two_inv());
        }
    }
    for (int e = 0; e < 3; e++) fe_to_u64x4(ev[e], out + 4 * e);
}

// bind variable k with r
static void oc_bind(cozk_output_check* oc, const fe& r) {
    cozk_ctx* ctx = oc->ctx;
    const size_t h = oc->len / 2;
    const fe one = Fr::one();
    if (oc_sparse(oc)) {
        const int k = oc->k;
        const fe omr = Fr::sub(one, r);
        const uint32_t* vio = oc->sub ? oc->vio : nullptr;
        if (oc->d_is_cols && oc->tb) k_ocs_first_fold<2><<<grid_for(h), PT, 0, ctx->stream>>>(oc->ta, oc->tb, vio, oc->sub, oc->lo, oc->hi, h, omr, r, oc->D);
        else if (oc->d_is_cols && oc->ta) k_ocs_first_fold<1><<<grid_for(h), PT, 0, ctx->stream>>>(oc->ta, nullptr, vio, oc->sub, oc->lo, oc->hi, h, omr, r, oc->D);
        else if (oc->d_is_cols) k_oc_first_fold<<<grid_for(h), PT, 0, ctx->stream>>>(oc->vf, oc->vio, oc->lo, oc->hi, h, omr, r, oc->D);
        else k_fold_halves<<<grid_for(h), PT, 0, ctx->stream>>>(oc->D, h, r);
        HIP_TRY(hipGetLastError());
        oc->d_is_cols = false;
        oc->c = Fr::mul(oc->c, oc_eq1(oc->r_eq[(size_t)k], r));
        for (int sd = 0; sd < oc->nside; sd++) oc->rho[sd] = Fr::mul(oc->rho[sd], oc_bit(oc, sd, k) ? r : omr);
        oc->k++;
        oc->len = h;
        if (!oc_sparse(oc)) {  // the length is W': the dense tail's vectors
            k_oc_tail_init<<<grid_for(h), PT, 0, ctx->stream>>>(oc->E, oc->Rg, oc->c, oc->rho[0], oc->rho[1], oc->sides, h);
            HIP_TRY(hipGetLastError());
        }
    } else {
        OcTriple t{{oc->E, oc->Rg, oc->D}};
        k_oc_bind3<<<dim3(grid_for(h), 3), PT, 0, ctx->stream>>>(t, h, r);
        HIP_TRY(hipGetLastError());
        oc->k++;
        oc->len = h;
    }
}

// What both creates do once their arguments stand: the window's geometry, the handle's device memory, Llow, and with W' = MEM the dense
// vectors.  `src` carries the borrowed sources (vf and vio, or ta, tb and vio with sub and rep3) and nothing else.
static cozk_output_check* oc_build(cozk_ctx* ctx, const cozk_output_check& src, size_t MEM, size_t W, size_t io_start, const uint64_t* r_eq) {
    cozk_output_check* oc = new cozk_output_check(src);
    oc->ctx = ctx;
    oc->m = __builtin_ctzll(MEM);
    while (((size_t)1 << oc->lw) < W) oc->lw++;
    oc->lo = io_start, oc->hi = io_start + W, oc->len = MEM;
    const size_t Wp = (size_t)1 << oc->lw;
    const size_t c = (io_start / Wp + 1) * Wp;  // the one multiple of W' the window can hold inside
    oc->nside = c < oc->hi ? 2 : 1;
    oc->sides.lo[0] = io_start, oc->sides.hi[0] = c < oc->hi ? c : oc->hi;
    oc->sides.lo[1] = oc->sides.hi[1] = oc->hi;
    if (oc->nside == 2) oc->sides.lo[1] = c;
    oc->r_eq.resize((size_t)oc->m);
    for (int i = 0; i < oc->m; i++) oc->r_eq[(size_t)i] = fe_from_u64x4(r_eq + 4 * i);
    oc->c = oc->rho[0] = oc->rho[1] = Fr::one();
    try {
        const bool dense = oc->lw == oc->m;
        oc->D = dev_alloc_fe(dense ? MEM : MEM / 2);
        oc->E = dev_alloc_fe(Wp);
        oc->Rg = dev_alloc_fe(Wp);
        if (oc->lw > 13) ctx->scratch2.reserve(Wp * sizeof(fe));
        eq_evals_device(ctx, oc->r_eq.data() + (oc->m - oc->lw), oc->lw, oc->E, ctx->scratch2.as<fe>());  // Llow; with lw == m it is E
        if (dense) {
            const uint32_t* vio = oc->sub ? oc->vio : nullptr;
            if (oc->tb) k_ocs_materialise<2><<<grid_for(MEM), PT, 0, ctx->stream>>>(oc->ta, oc->tb, vio, oc->sub, oc->lo, oc->hi, MEM, oc->D, oc->Rg);
            else if (oc->ta) k_ocs_materialise<1><<<grid_for(MEM), PT, 0, ctx->stream>>>(oc->ta, nullptr, vio, oc->sub, oc->lo, oc->hi, MEM, oc->D, oc->Rg);
            else k_oc_materialise<<<grid_for(MEM), PT, 0, ctx->stream>>>(oc->vf, oc->vio, oc->lo, oc->hi, MEM, oc->D, oc->Rg);
            HIP_TRY(hipGetLastError());
            oc->d_is_cols = false;
        }
    } catch (...) {
        oc_release(oc);
        delete oc;
        throw;
    }
    return oc;
}

extern "C" {

int cozk_output_check_create(cozk_ctx* ctx, const cozk_vec* v_final, const cozk_vec* v_io, size_t io_start, const uint64_t* r_eq, cozk_output_check** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && v_final && v_io && r_eq && out, "output_check_create: null argument");
        COZK_REQUIRE(v_final->kind == COZK_SCALAR_U32, "output_check_create: v_final is a U32 vector");
        const size_t MEM = v_final->n;
        COZK_REQUIRE(MEM >= 2 && (MEM & (MEM - 1)) == 0 && MEM < ((size_t)1 << 32), "output_check_create: v_final has 2^m entries, 1 <= m < 32");
        COZK_REQUIRE(v_io->kind == COZK_SCALAR_U32, "output_check_create: v_io is a U32 vector");
        const size_t W = v_io->n;
        COZK_REQUIRE(W >= 1, "output_check_create: io_len is 0");
        COZK_REQUIRE(io_start <= MEM && W <= MEM - io_start, "output_check_create: io_start + io_len > MEM");
        COZK_REQUIRE(v_final->ctx && v_io->ctx && v_final->ctx->device == ctx->device && v_io->ctx->device == ctx->device,
                     "output_check_create: v_final and v_io live on the context's device");
        cozk_output_check src;
        src.vf = (const uint32_t*)v_final->d, src.vio = (const uint32_t*)v_io->d;
        *out = oc_build(ctx, src, MEM, W, io_start, r_eq);
    });
}

int cozk_output_check_shared_create(cozk_ctx* ctx, const cozk_poly* v_final, const cozk_vec* v_io, size_t io_start, const uint64_t* r_eq, int party,
                                    cozk_output_check** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && v_final && v_io && r_eq && out, "output_check_shared_create: null argument");
        const size_t MEM = v_final->len;
        COZK_REQUIRE(MEM >= 2 && (MEM & (MEM - 1)) == 0 && MEM < ((size_t)1 << 32), "output_check_shared_create: v_final has 2^m entries, 1 <= m < 32");
        COZK_REQUIRE(v_final->cur < 0, "output_check_shared_create: v_final is bound");
        const bool rep3 = v_final->mode == COZK_MODE_REP3;
        COZK_REQUIRE(party >= 0 && party <= (rep3 ? 2 : 0), "output_check_shared_create: party is 0..2 for a REP3 v_final and 0 for a PLAIN one");
        COZK_REQUIRE(v_io->kind == COZK_SCALAR_U32, "output_check_shared_create: v_io is a U32 vector");
        const size_t W = v_io->n;
        COZK_REQUIRE(W >= 1, "output_check_shared_create: io_len is 0");
        COZK_REQUIRE(io_start <= MEM && W <= MEM - io_start, "output_check_shared_create: io_start + io_len > MEM");
        COZK_REQUIRE(v_final->ctx && v_io->ctx && v_final->ctx->device == ctx->device && v_io->ctx->device == ctx->device,
                     "output_check_shared_create: v_final and v_io live on the context's device");
        cozk_output_check src;
        src.ta = v_final->a0, src.tb = rep3 ? v_final->b0 : nullptr, src.vio = (const uint32_t*)v_io->d;
        src.rep3 = rep3, src.sub = !(rep3 && party == 2);
        *out = oc_build(ctx, src, MEM, W, io_start, r_eq);
    });
}

int cozk_output_check_round(cozk_output_check* oc, const uint64_t* r, uint64_t out[12]) {
    if (!oc) return COZK_ERR_INVALID_ARG;
    return cozk_guard(oc->ctx, [&] {
        COZK_REQUIRE(out, "output_check_round: null argument");
        COZK_REQUIRE(oc->started || !r, "output_check_round: round 0 takes no challenge (r is NULL)");
        COZK_REQUIRE(!oc->started || r, "output_check_round: a round after round 0 binds the previous variable (r is not NULL)");
        COZK_REQUIRE(!oc->started || oc->len > 2, "output_check_round: one variable is left: call cozk_output_check_final");
        if (r) oc_bind(oc, fe_from_u64x4(r));
        oc->started = true;
        oc_round_evals(oc, out);
    });
}

int cozk_output_check_final(cozk_output_check* oc, const uint64_t r[4], uint64_t out[12]) {
    if (!oc) return COZK_ERR_INVALID_ARG;
    return cozk_guard(oc->ctx, [&] {
        COZK_REQUIRE(r && out, "output_check_final: null argument");
        COZK_REQUIRE(oc->len == 2, "output_check_final: more than one variable is left");
        oc_bind(oc, fe_from_u64x4(r));
        fe* res = result_slot(oc->ctx, 3);
        k_oc_final<<<1, 1, 0, oc->ctx->stream>>>(oc->E, oc->Rg, oc->D, res);
        HIP_TRY(hipGetLastError());
        fe h[3];
        fetch_fe(oc->ctx, res, 3, h);
        if (oc->rep3) h[2] = Fr::mul(h[2], fr_two_inv());  // the additive share of (v_final - v_io)(r)
        for (int e = 0; e < 3; e++) fe_to_u64x4(h[e], out + 4 * e);
    });
}

size_t cozk_output_check_len(const cozk_output_check* oc) { return oc ? oc->len : 0; }

int cozk_output_check_free(cozk_output_check* oc) {
    if (!oc) return COZK_OK;
    oc_release(oc);
    delete oc;
    return COZK_OK;
}

}  // extern "C"
