// co-jolt's Spartan OUTER sumcheck over Az / Bz / Cz (SURVEY 8(f)2) -- part of poly.hip's translation unit.
//
//   sum_x eq(tau, x) * (Az(x) * Bz(x) - Cz(x)) = 0
//
//   cozk_outer  <->  Rep3SpartanInterleavedPolynomial + GruenSplitEqPolynomial as driven by prove_spartan_cubic_sumcheck
//   (co-jolt/src/poly/spartan_interleaved_poly.rs:22-664, co-jolt/src/r1cs/spartan/worker.rs:277-300,
//   co-jolt/src/subprotocols/sumcheck_spartan.rs:44-79).
//
// The reference keeps Az, Bz, Cz as ONE sparse interleaved list of (index, SharedOrPublic) entries (row r of the three
// sits at 3 r, 3 r + 1, 3 r + 2) and walks blocks of 6 with a dozen public / shared / additive cases
// (utils/shared_or_public.rs).  Here they are three share arrays over rows = step * padded_constraints + constraint (stored compactly:
// only the real constraint rows of a step, see cozk_outer::act_rows),
// every value a share (a public value is its trivial share: party 0's a, party 1's b): k_r1cs_rows evaluates the
// constraint rows straight from the witness columns, a round streams row pairs (2k, 2k + 1) once, binding is a pairwise
// fold.  Per party the sums differ from the reference's only by sharings of zero; what the coordinator adds up -- and the
// proof -- is identical (oracle/pyspartan_outer.py restates the SPARSE algorithm and the tests compare proofs).
// The round polynomial comes from the two quadratic evaluations t(0), t(infinity) and the Gruen linear factor exactly as
// process_eq_sumcheck_round_worker forms it; in the first round t(0) is not computed (it is zero for a satisfied system,
// spartan_interleaved_poly.rs:203-205).

struct OuterLC {
    int first, n, offset;  // terms [first, first + n); offset != 0: evaluated at the NEXT step (cross-step constraints)
};
struct OuterRow {
    OuterLC a, b, c;  // uniform: Az = a, Bz = b, Cz = c;  cross-step: Az = a - b, Bz = c (the condition), Cz = 0
    int cross;
};

struct cozk_outer {
    cozk_ctx* ctx;
    int mode, party;
    size_t L;             // current number of rows (power of two)
    fe* buf[2][3][2];     // ping-pong [which][az | bz | cz][component]
    size_t cap[2];
    int cur;
    // Gruen split-eq: tables for every prefix of w_out / w_in (table k has 2^k entries at offset 2^k - 1)
    std::vector<fe> w;
    size_t n_out, n_in;   // variables in the current tables
    fe* E_out;
    fe* E_in;
    int current_index;
    fe current_scalar;
    int round;
    // rows [act_rows, per_step) of every step are zero by construction (the constraints are padded to a power of two; binding the
    // row variables halves both: per_step -> per_step / 2, act_rows -> ceil(act_rows / 2)) and are NOT STORED: while a step spans
    // several rows the arrays are compact, element (step, row) at step * act_rows + row; L stays the dense-equivalent length
    size_t per_step, act_rows;
};

// constraint rows -> dense Az, Bz, Cz shares (Rep3SpartanInterleavedPolynomial::new, spartan_interleaved_poly.rs:40-172;
// LC::evaluate_row_rep3_mixed, r1cs/ops.rs:18-37; eval_offset_lc_rep3_mixed, spartan_interleaved_poly.rs:666-684)
template <int NC>
static __device__ __forceinline__ Sh<NC> outer_eval_lc(const OuterLC& lc, const int* __restrict__ tvar, const fe* __restrict__ tcoef,
                                                       const fe* const* __restrict__ va, const fe* const* __restrict__ vb, size_t step, size_t num_steps,
                                                       int pub_comp) {
    Sh<NC> acc;
    for (int k = 0; k < NC; k++) acc.c[k] = Fr::zero();
    fe pub = Fr::zero();
    size_t row = step;
    bool const_only = false;
    if (lc.offset) {
        if (step + 1 < num_steps) row = step + 1;
        else const_only = true;  // last step: only the constant term (:679-683)
    }
    for (int t = 0; t < lc.n; t++) {
        int v = tvar[lc.first + t];
        fe c = tcoef[lc.first + t];
        if (v < 0) {
            pub = Fr::add(pub, c);
        } else if (!const_only) {
            if (vb[v] || NC == 1) {
                acc.c[0] = Fr::add(acc.c[0], Fr::mul(fe_load(va[v] + row), c));
                if (NC == 2) acc.c[NC - 1] = Fr::add(acc.c[NC - 1], Fr::mul(fe_load(vb[v] + row), c));
            } else {
                pub = Fr::add(pub, Fr::mul(fe_load(va[v] + row), c));  // a public column
            }
        }
    }
    if (pub_comp >= 0) acc.c[pub_comp] = Fr::add(acc.c[pub_comp], pub);  // add_public: party 0's a, party 1's b
    return acc;
}

template <int NC>
__global__ void __launch_bounds__(PT) k_r1cs_rows(const OuterRow* __restrict__ rows, int n_rows, size_t padded, size_t num_steps, const int* __restrict__ tvar,
                                               const fe* __restrict__ tcoef, const fe* const* __restrict__ va, const fe* const* __restrict__ vb, int pub_comp,
                                               fe* aza, fe* azb, fe* bza, fe* bzb, fe* cza, fe* czb) {
    (void)padded;
    size_t idx = (size_t)blockIdx.x * PT + threadIdx.x;  // compact storage: step * n_rows + constraint
    if (idx >= num_steps * (size_t)n_rows) return;
    size_t step = idx / (size_t)n_rows;
    int ci = (int)(idx - step * (size_t)n_rows);
    Sh<NC> az, bz, cz;
    for (int k = 0; k < NC; k++) az.c[k] = bz.c[k] = cz.c[k] = Fr::zero();
    {
        const OuterRow& r = rows[ci];
        az = outer_eval_lc<NC>(r.a, tvar, tcoef, va, vb, step, num_steps, pub_comp);
        if (r.cross) {
            az = sh_sub<NC>(az, outer_eval_lc<NC>(r.b, tvar, tcoef, va, vb, step, num_steps, pub_comp));
            bz = outer_eval_lc<NC>(r.c, tvar, tcoef, va, vb, step, num_steps, pub_comp);
        } else {
            bz = outer_eval_lc<NC>(r.b, tvar, tcoef, va, vb, step, num_steps, pub_comp);
            cz = outer_eval_lc<NC>(r.c, tvar, tcoef, va, vb, step, num_steps, pub_comp);
        }
    }
    sh_store<NC>(aza, azb, idx, az);
    sh_store<NC>(bza, bzb, idx, bz);
    sh_store<NC>(cza, czb, idx, cz);
}

// The same rows with ONE THREAD PER STEP and a uniform loop over the constraints (round 3): every lane of a wave evaluates the same
// linear combination, so there is no divergence (thread-per-row: a wave ran as long as its longest LC -- the 39-term pack_be row --
// while 56 of 128 rows are padding), the column reads are coalesced (lane = step) and the table entries are wave-uniform scalar
// loads; coefficients +-1 (most terms) add / subtract instead of multiplying.  Rows [n_rows, padded) are left unwritten (cozk_outer::act_rows).
template <int NC>
static __device__ __forceinline__ Sh<NC> outer_eval_lc_step(const OuterLC lc, const int* __restrict__ tvar, const int* __restrict__ tkind,
                                                            const fe* __restrict__ tcoef, const fe* const* __restrict__ va, const fe* const* __restrict__ vb,
                                                            size_t step, size_t num_steps, int pub_comp) {
    Sh<NC> acc;
    for (int k = 0; k < NC; k++) acc.c[k] = Fr::zero();
    fe pub = Fr::zero();
    size_t row = step;
    bool const_only = false;
    if (lc.offset) {
        if (step + 1 < num_steps) row = step + 1;
        else const_only = true;  // last step: only the constant term (:679-683)
    }
    for (int t = 0; t < lc.n; t++) {
        const int v = tvar[lc.first + t];
        const int kind = tkind[lc.first + t];  // 0: +1, 1: -1, 2: general coefficient
        if (v < 0) {
            pub = Fr::add(pub, tcoef[lc.first + t]);
            continue;
        }
        if (const_only) continue;
        const bool shared = vb[v] || NC == 1;
        fe xa = fe_load(va[v] + row), xb;
        if (NC == 2 && vb[v]) xb = fe_load(vb[v] + row);
        if (kind == 2) {
            const fe c = tcoef[lc.first + t];
            xa = Fr::mul(xa, c);
            if (NC == 2 && vb[v]) xb = Fr::mul(xb, c);
        }
        if (shared) {
            acc.c[0] = kind == 1 ? Fr::sub(acc.c[0], xa) : Fr::add(acc.c[0], xa);
            if (NC == 2) acc.c[NC - 1] = kind == 1 ? Fr::sub(acc.c[NC - 1], xb) : Fr::add(acc.c[NC - 1], xb);
        } else {
            pub = kind == 1 ? Fr::sub(pub, xa) : Fr::add(pub, xa);  // a public column
        }
    }
    if (pub_comp >= 0) acc.c[pub_comp] = Fr::add(acc.c[pub_comp], pub);  // add_public: party 0's a, party 1's b
    return acc;
}

// value q (0: Az, 1: Bz, 2: Cz) of constraint row r at `step`
template <int NC>
static __device__ __forceinline__ Sh<NC> outer_row_value(const OuterRow& r, int q, const int* __restrict__ tvar, const int* __restrict__ tkind,
                                                         const fe* __restrict__ tcoef, const fe* const* __restrict__ va, const fe* const* __restrict__ vb,
                                                         size_t step, size_t num_steps, int pub_comp) {
    Sh<NC> z;
    for (int k = 0; k < NC; k++) z.c[k] = Fr::zero();
    if (r.cross) {  // (a - b) * c = 0 across two steps
        if (q == 0)
            return sh_sub<NC>(outer_eval_lc_step<NC>(r.a, tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp),
                              outer_eval_lc_step<NC>(r.b, tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp));
        if (q == 1) return outer_eval_lc_step<NC>(r.c, tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp);
        return z;
    }
    return outer_eval_lc_step<NC>(q == 0 ? r.a : (q == 1 ? r.b : r.c), tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp);
}

// A lane's rows of one step lie 32 B apart, the steps of a wave padded * 32 B apart: stored straight from the lane, every store
// instruction hits 64 different lines 16 bytes at a time (7.2 GB at 2^20 steps went out at ~1 TB/s).  Four consecutive rows of a
// step are one 128-byte line: a wave computes them for its 64 steps and hands them out as whole lines through its LDS window
// (stage_out_rows, poly.hip); the last n_rows % 4 rows and partial waves take the direct path.
template <int NC>
__global__ void __launch_bounds__(PT) k_r1cs_rows_step(const OuterRow* __restrict__ rows, int n_rows, size_t padded, size_t num_steps, const int* __restrict__ tvar,
                                                    const int* __restrict__ tkind, const fe* __restrict__ tcoef, const fe* const* __restrict__ va,
                                                    const fe* const* __restrict__ vb, int pub_comp, fe* aza, fe* azb, fe* bza, fe* bzb, fe* cza, fe* czb) {
    __shared__ __attribute__((aligned(16))) char stage[PT / 64][ST_WAVE_BYTES];
    char* st = stage[threadIdx.x >> 6];
    const size_t step0 = (size_t)blockIdx.x * PT + (threadIdx.x & ~63u);
    const size_t step = step0 + (threadIdx.x & 63);
    fe* outa[3] = {aza, bza, cza};
    fe* outb[3] = {azb, bzb, czb};
    int ci = 0;
    (void)padded;
    const size_t stride = (size_t)n_rows;  // compact storage: the padding rows of a step are not stored
    if (step0 + 64 <= num_steps && (stride & 3) == 0) {
        for (; ci + 4 <= n_rows; ci += 4) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                fe va4[4], vb4[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const OuterRow r = rows[ci + j];
                    const Sh<NC> z = outer_row_value<NC>(r, q, tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp);
                    va4[j] = z.c[0];
                    if (NC == 2) vb4[j] = z.c[NC - 1];
                }
                stage_out_rows(reinterpret_cast<char*>(outa[q] + step0 * stride + (size_t)ci), st, va4, stride * sizeof(fe));
                if (NC == 2) stage_out_rows(reinterpret_cast<char*>(outb[q] + step0 * stride + (size_t)ci), st, vb4, stride * sizeof(fe));
            }
        }
    }
    if (step >= num_steps) return;
    for (; ci < n_rows; ci++) {
        const OuterRow r = rows[ci];
        const size_t idx = step * stride + (size_t)ci;
        for (int q = 0; q < 3; q++) {
            const Sh<NC> z = outer_row_value<NC>(r, q, tvar, tkind, tcoef, va, vb, step, num_steps, pub_comp);
            sh_store<NC>(outa[q], outb[q], idx, z);
        }
    }
}
// rows [n_rows, padded) of every step of the (up to 6) arrays are zero: 16-byte pieces, coalesced within a step's tail
// quadratic evaluations of a round (spartan_interleaved_poly.rs:410-505): over row pairs (2k, 2k + 1),
//   partial[0] += e_k (Az_0 (x) Bz_0)        partial[1] += e_k (Cz_0.a + Cz_0.b)        partial[2] += e_k (dAz (x) dBz)
// with e_k = E_out[k >> in_bits] * E_in[k & in_mask]; the host forms t(0) = [0] - TWO_INV [1], t(infinity) = [2]
template <int NC>
__global__ void __launch_bounds__(PT) k_outer_round(const fe* __restrict__ aza, const fe* __restrict__ azb, const fe* __restrict__ bza, const fe* __restrict__ bzb,
                                                 const fe* __restrict__ cza, const fe* __restrict__ czb, size_t npairs, const fe* __restrict__ E_in, int in_bits,
                                                 const fe* __restrict__ E_out, int want_t0, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe s0 = Fr::zero(), s1 = Fr::zero(), s2 = Fr::zero();
    const size_t in_mask = ((size_t)1 << in_bits) - 1;
    for (size_t k = (size_t)blockIdx.x * PT + threadIdx.x; k < npairs; k += (size_t)gridDim.x * PT) {
        fe e = Fr::mul(fe_load(E_out + (k >> in_bits)), fe_load(E_in + (k & in_mask)));
        Sh<NC> a0 = sh_load<NC>(aza, azb, 2 * k), a1 = sh_load<NC>(aza, azb, 2 * k + 1);
        Sh<NC> b0 = sh_load<NC>(bza, bzb, 2 * k), b1 = sh_load<NC>(bza, bzb, 2 * k + 1);
        s2 = Fr::add(s2, Fr::mul(sh_local_mul<NC>(sh_sub<NC>(a1, a0), sh_sub<NC>(b1, b0)), e));
        if (want_t0) {
            s0 = Fr::add(s0, Fr::mul(sh_local_mul<NC>(a0, b0), e));
            s1 = Fr::add(s1, Fr::mul(sh_ab_sum<NC>(sh_load<NC>(cza, czb, 2 * k)), e));
        }
    }
    s0 = fr_block_sum(s0, sh4);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, s0);
    s1 = fr_block_sum(s1, sh4);
    if (threadIdx.x == 0) fe_store(partial + gridDim.x + blockIdx.x, s1);
    s2 = fr_block_sum(s2, sh4);
    if (threadIdx.x == 0) fe_store(partial + 2 * gridDim.x + blockIdx.x, s2);
}

struct OuterBindArgs {
    const fe* in[6];
    fe* out[6];
};
__global__ void __launch_bounds__(PT) k_outer_bind(OuterBindArgs a, size_t n_out, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    const fe* in = a.in[blockIdx.y];
    fe lo = fe_load(in + 2 * i), hi = fe_load(in + 2 * i + 1);
    fe_store(a.out[blockIdx.y] + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
}

// The same two kernels over the ACTIVE rows only, while a step still spans several rows (the first log2(padded) rounds carry ~94 %
// of the traffic; Jolt's 72 constraints in 128 slots leave 44 % of every step zero -- the reference never materialises those rows
// either, its SpartanInterleavedPolynomial is sparse).  act = active rows per step before the bind / in this round.
template <int NC>
__global__ void __launch_bounds__(PT) k_outer_round_act(const fe* __restrict__ aza, const fe* __restrict__ azb, const fe* __restrict__ bza, const fe* __restrict__ bzb,
                                                     const fe* __restrict__ cza, const fe* __restrict__ czb, uint32_t num_steps, uint32_t per_step, uint32_t act,
                                                     const fe* __restrict__ E_in, int in_bits, const fe* __restrict__ E_out, int want_t0,
                                                     fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe s0 = Fr::zero(), s1 = Fr::zero(), s2 = Fr::zero();
    const size_t in_mask = ((size_t)1 << in_bits) - 1;
    const uint32_t act_pairs = (act + 1) / 2, pairs_per_step = per_step / 2;
    const size_t total = (size_t)num_steps * act_pairs;
    for (size_t q = (size_t)blockIdx.x * PT + threadIdx.x; q < total; q += (size_t)gridDim.x * PT) {
        const uint32_t step = (uint32_t)(q / act_pairs), pr = (uint32_t)(q - (size_t)step * act_pairs);
        const size_t k = (size_t)step * pairs_per_step + pr;  // the pair's index in the padded (dense-equivalent) order: eq tables
        const size_t si = (size_t)step * act + 2 * pr;        // ... and in the compact storage
        const bool has_hi = 2 * pr + 1 < act;
        fe e = Fr::mul(fe_load(E_out + (k >> in_bits)), fe_load(E_in + (k & in_mask)));
        Sh<NC> a0 = sh_load<NC>(aza, azb, si), b0 = sh_load<NC>(bza, bzb, si);
        Sh<NC> a1, b1;
        if (has_hi) {
            a1 = sh_load<NC>(aza, azb, si + 1);
            b1 = sh_load<NC>(bza, bzb, si + 1);
        } else {
            for (int c = 0; c < NC; c++) a1.c[c] = b1.c[c] = Fr::zero();
        }
        s2 = Fr::add(s2, Fr::mul(sh_local_mul<NC>(sh_sub<NC>(a1, a0), sh_sub<NC>(b1, b0)), e));
        if (want_t0) {
            s0 = Fr::add(s0, Fr::mul(sh_local_mul<NC>(a0, b0), e));
            s1 = Fr::add(s1, Fr::mul(sh_ab_sum<NC>(sh_load<NC>(cza, czb, si)), e));
        }
    }
    s0 = fr_block_sum(s0, sh4);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, s0);
    s1 = fr_block_sum(s1, sh4);
    if (threadIdx.x == 0) fe_store(partial + gridDim.x + blockIdx.x, s1);
    s2 = fr_block_sum(s2, sh4);
    if (threadIdx.x == 0) fe_store(partial + 2 * gridDim.x + blockIdx.x, s2);
}
// k_outer_round_act on the 9 x 29 multiplier (fr9.hip.hpp) for the rounds that are large enough to be throughput-bound: six products
// per pair at ~208 instructions instead of ~600.  e = E_out x E_in carries lambda, a local product carries lambda, their product
// lambda^3; the Cz term is (c.a + c.b) x e: lambda^2 -- one product with the matching constant per lane at the end.
template <int NC>
__global__ void __launch_bounds__(PT) k_outer_round_act9(const fe* __restrict__ aza, const fe* __restrict__ azb, const fe* __restrict__ bza, const fe* __restrict__ bzb,
                                                      const fe* __restrict__ cza, const fe* __restrict__ czb, uint32_t num_steps, uint32_t per_step, uint32_t act,
                                                      const fe* __restrict__ E_in, int in_bits, const fe* __restrict__ E_out, int want_t0,
                                                      fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    f9 s0 = fr9_zero(), s1 = fr9_zero(), s2 = fr9_zero();
    const size_t in_mask = ((size_t)1 << in_bits) - 1;
    const uint32_t act_pairs = (act + 1) / 2, pairs_per_step = per_step / 2;
    const size_t total = (size_t)num_steps * act_pairs;
    unsigned it = 0;  // the periodic fold of the lazy sums (fr9.hip.hpp): one term per sum and iteration
    for (size_t q = (size_t)blockIdx.x * PT + threadIdx.x; q < total; q += (size_t)gridDim.x * PT, it++) {
        if (it != 0 && (it & (FR9_FOLD_PERIOD - 1)) == 0) {
            fr9_fold(s0);
            fr9_fold(s1);
            fr9_fold(s2);
        }
        const uint32_t step = (uint32_t)(q / act_pairs), pr = (uint32_t)(q - (size_t)step * act_pairs);
        const size_t k = (size_t)step * pairs_per_step + pr;
        const size_t si = (size_t)step * act + 2 * pr;
        const bool has_hi = 2 * pr + 1 < act;
        const f9 e = fr9_mul(f9_from_fe(fe_load(E_out + (k >> in_bits))), f9_from_fe(fe_load(E_in + (k & in_mask))));
        const Sh9<NC> a0 = sh9_load_or_zero<NC>(aza, azb, si, (size_t)-1), b0 = sh9_load_or_zero<NC>(bza, bzb, si, (size_t)-1);
        const Sh9<NC> a1 = sh9_load_or_zero<NC>(aza, azb, si + 1, has_hi ? (size_t)-1 : 0), b1 = sh9_load_or_zero<NC>(bza, bzb, si + 1, has_hi ? (size_t)-1 : 0);
        Sh9<NC> da, db;
        for (int c = 0; c < NC; c++) {
            da.c[c] = f9_sub(a1.c[c], FR9_C2, a0.c[c]);  // canonical inputs: limbs < 1.5 * 2^30, fine as a product's first operand
            db.c[c] = f9_sub(b1.c[c], FR9_C2, b0.c[c]);
        }
        s2 = f9_norm(fr9_add(s2, fr9_mul(e, sh9_local_mul<NC>(da, db))));
        if (want_t0) {
            s0 = f9_norm(fr9_add(s0, fr9_mul(e, sh9_local_mul<NC>(a0, b0))));
            const Sh9<NC> c0 = sh9_load_or_zero<NC>(cza, czb, si, (size_t)-1);
            s1 = f9_norm(fr9_add(s1, fr9_mul(NC == 2 ? fr9_add(c0.c[0], c0.c[NC - 1]) : c0.c[0], e)));
        }
    }
    fe v = fr_block_sum(fr9_to_canonical(fr9_mul(s0, f9_const(FR9_K3))), sh4);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, v);
    v = fr_block_sum(fr9_to_canonical(fr9_mul(s1, f9_const(FR9_K2))), sh4);
    if (threadIdx.x == 0) fe_store(partial + gridDim.x + blockIdx.x, v);
    v = fr_block_sum(fr9_to_canonical(fr9_mul(s2, f9_const(FR9_K3))), sh4);
    if (threadIdx.x == 0) fe_store(partial + 2 * gridDim.x + blockIdx.x, v);
}
__global__ void __launch_bounds__(PT) k_outer_bind_act(OuterBindArgs a, uint32_t num_steps, uint32_t per_step_in, uint32_t act_in, fe r) {
    (void)per_step_in;
    const uint32_t act_out = (act_in + 1) / 2;
    const size_t q = (size_t)blockIdx.x * PT + threadIdx.x;  // = the compact output index step * act_out + row
    if (q >= (size_t)num_steps * act_out) return;
    const uint32_t step = (uint32_t)(q / act_out), row = (uint32_t)(q - (size_t)step * act_out);
    const fe* in = a.in[blockIdx.y] + (size_t)step * act_in + 2 * row;
    fe lo = fe_load(in);
    fe hi = 2 * row + 1 < act_in ? fe_load(in + 1) : Fr::zero();
    fe_store(a.out[blockIdx.y] + q, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
}

// every prefix table of eq(w[..k], .), big-endian: table k from table k - 1 (k_eq_expand)
static void outer_build_tables(cozk_ctx* ctx, const std::vector<fe>& w, fe* tab) {
    fe one = Fr::one();
    HIP_TRY(hipMemcpyAsync(tab, &one, sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < w.size(); k++) {
        size_t n = (size_t)1 << k;
        k_eq_expand<<<grid_for(n), PT, 0, ctx->stream>>>(tab + (n - 1), tab + (2 * n - 1), n, w[k]);
    }
    HIP_TRY(hipGetLastError());
}

extern "C" {

int cozk_outer_create(cozk_ctx* ctx, int mode, int party_id, const cozk_r1cs* sys, const cozk_poly* const* vars, size_t n_vars, const uint64_t* tau,
                      size_t n_tau, cozk_outer** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && sys && vars && n_vars > 0 && tau && out && (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3) && party_id >= 0 && party_id < 3,
                     "outer_create: bad argument");
        const size_t num_steps = vars[0]->len;
        COZK_REQUIRE(num_steps >= 1 && (num_steps & (num_steps - 1)) == 0, "outer_create: the number of steps must be a power of two");
        const size_t padded = sys->padded_num_constraints;
        const size_t n_rows = sys->n_uniform + sys->n_cross;
        COZK_REQUIRE(padded >= n_rows && padded >= 1 && (padded & (padded - 1)) == 0, "outer_create: padded_num_constraints must be a power of two >= the constraints");
        const size_t L = num_steps * padded;
        COZK_REQUIRE(L >= 2 && ((size_t)1 << n_tau) == L, "outer_create: tau needs log2(steps * padded constraints) entries");
        const int NC = mode == COZK_MODE_REP3 ? 2 : 1;
        std::vector<const fe*> va(n_vars), vb(n_vars);
        for (size_t v = 0; v < n_vars; v++) {
            COZK_REQUIRE(vars[v] && vars[v]->len == num_steps && vars[v]->cur < 0, "outer_create: every witness column has one (unbound) entry per step");
            COZK_REQUIRE(vars[v]->mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, "outer_create: a shared column needs the Rep3 mode");
            va[v] = vars[v]->a0;
            vb[v] = vars[v]->mode == COZK_MODE_REP3 ? vars[v]->b0 : nullptr;
        }
        // the constraint table
        std::vector<int> tvar(sys->term_var, sys->term_var + sys->n_terms);
        std::vector<fe> tcoef(sys->n_terms);
        for (size_t t = 0; t < sys->n_terms; t++) {
            COZK_REQUIRE(tvar[t] < (int)n_vars, "outer_create: term variable out of range");
            int64_t c = sys->term_coeff[t];
            fe m = Fr::from_u64((uint64_t)(c < 0 ? -c : c));
            tcoef[t] = c < 0 ? Fr::neg(m) : m;
        }
        auto lc = [&](const cozk_lc& s) {
            COZK_REQUIRE(s.first_term >= 0 && s.n_terms >= 0 && (size_t)(s.first_term + s.n_terms) <= sys->n_terms, "outer_create: LC range");
            return OuterLC{s.first_term, s.n_terms, s.offset};
        };
        std::vector<OuterRow> rows;
        for (size_t i = 0; i < sys->n_uniform; i++) rows.push_back(OuterRow{lc(sys->uniform[3 * i]), lc(sys->uniform[3 * i + 1]), lc(sys->uniform[3 * i + 2]), 0});
        for (size_t i = 0; i < sys->n_cross; i++) rows.push_back(OuterRow{lc(sys->cross[3 * i]), lc(sys->cross[3 * i + 1]), lc(sys->cross[3 * i + 2]), 1});
        cozk_outer* st = new cozk_outer();
        st->ctx = ctx;
        st->mode = mode;
        st->party = party_id;
        st->L = L;
        st->cur = 0;
        st->round = 0;
        st->per_step = padded;
        st->act_rows = n_rows;
        for (int w = 0; w < 2; w++) {
            st->cap[w] = w == 0 ? num_steps * n_rows : num_steps * ((n_rows + 1) / 2);  // compact: 72 of 128 rows of a Jolt step
            for (int q = 0; q < 3; q++)
                for (int c = 0; c < 2; c++) st->buf[w][q][c] = c < NC ? dev_alloc_fe(st->cap[w]) : nullptr;
        }
        // upload tables (scratch for the duration of the row kernel)
        std::vector<int> tkind(tvar.size());
        for (size_t t = 0; t < tvar.size(); t++) tkind[t] = sys->term_coeff[t] == 1 ? 0 : (sys->term_coeff[t] == -1 ? 1 : 2);
        size_t bytes = rows.size() * sizeof(OuterRow) + 2 * tvar.size() * sizeof(int) + 64 + tcoef.size() * sizeof(fe) + 2 * n_vars * sizeof(void*) + 64;
        char* d = (char*)ctx_dev_alloc(ctx, bytes);
        OuterRow* d_rows = (OuterRow*)d;
        fe* d_coef = (fe*)(((uintptr_t)(d_rows + rows.size()) + 31) & ~(uintptr_t)31);
        const fe** d_va = (const fe**)(d_coef + tcoef.size());
        const fe** d_vb = d_va + n_vars;
        int* d_var = (int*)(d_vb + n_vars);
        int* d_kind = d_var + tvar.size();
        if (!rows.empty()) HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(OuterRow), hipMemcpyHostToDevice, ctx->stream));
        if (!tcoef.empty()) HIP_TRY(hipMemcpyAsync(d_coef, tcoef.data(), tcoef.size() * sizeof(fe), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_va, va.data(), n_vars * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_vb, vb.data(), n_vars * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        if (!tvar.empty()) {
            HIP_TRY(hipMemcpyAsync(d_var, tvar.data(), tvar.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(d_kind, tkind.data(), tkind.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        }
        const int pub_comp = mode == COZK_MODE_PLAIN ? 0 : (party_id == 0 ? 0 : (party_id == 1 ? 1 : -1));
        // one thread per step once there are enough steps to fill the chip; thread per row below that (COZK_R1CS_BY_ROW=1 forces it)
        static const bool by_row_env = getenv("COZK_R1CS_BY_ROW") != nullptr;  // set to anything
        if (num_steps >= 32 && !by_row_env) {
            if (NC == 2)
                k_r1cs_rows_step<2><<<grid_for(num_steps), PT, 0, ctx->stream>>>(d_rows, (int)rows.size(), padded, num_steps, d_var, d_kind, d_coef, d_va, d_vb, pub_comp,
                                                                                 st->buf[0][0][0], st->buf[0][0][1], st->buf[0][1][0], st->buf[0][1][1], st->buf[0][2][0],
                                                                                 st->buf[0][2][1]);
            else
                k_r1cs_rows_step<1><<<grid_for(num_steps), PT, 0, ctx->stream>>>(d_rows, (int)rows.size(), padded, num_steps, d_var, d_kind, d_coef, d_va, d_vb, pub_comp,
                                                                                 st->buf[0][0][0], nullptr, st->buf[0][1][0], nullptr, st->buf[0][2][0], nullptr);
        } else if (NC == 2)
            k_r1cs_rows<2><<<grid_for(num_steps * n_rows), PT, 0, ctx->stream>>>(d_rows, (int)rows.size(), padded, num_steps, d_var, d_coef, d_va, d_vb, pub_comp, st->buf[0][0][0],
                                                                st->buf[0][0][1], st->buf[0][1][0], st->buf[0][1][1], st->buf[0][2][0], st->buf[0][2][1]);
        else
            k_r1cs_rows<1><<<grid_for(num_steps * n_rows), PT, 0, ctx->stream>>>(d_rows, (int)rows.size(), padded, num_steps, d_var, d_coef, d_va, d_vb, pub_comp, st->buf[0][0][0],
                                                                nullptr, st->buf[0][1][0], nullptr, st->buf[0][2][0], nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx_dev_free(ctx, d);
        // GruenSplitEqPolynomial::new(tau): w = [w_out (n / 2) | w_in | w_last]
        st->w.resize(n_tau);
        for (size_t i = 0; i < n_tau; i++) st->w[i] = fe_from_u64x4(tau + 4 * i);
        const size_t m = n_tau / 2;
        st->n_out = m;
        st->n_in = n_tau - 1 - m;
        st->E_out = dev_alloc_fe(((size_t)2 << st->n_out));
        st->E_in = dev_alloc_fe(((size_t)2 << st->n_in));
        outer_build_tables(ctx, std::vector<fe>(st->w.begin(), st->w.begin() + m), st->E_out);
        outer_build_tables(ctx, std::vector<fe>(st->w.begin() + m, st->w.begin() + (n_tau - 1)), st->E_in);
        st->current_index = (int)n_tau;
        st->current_scalar = Fr::one();
        *out = st;
    });
}

int cozk_outer_free(cozk_outer* st) {
    if (!st) return COZK_OK;
    for (int w = 0; w < 2; w++)
        for (int q = 0; q < 3; q++)
            for (int c = 0; c < 2; c++) ctx_dev_free(st->ctx, st->buf[w][q][c]);
    ctx_dev_free(st->ctx, st->E_out);
    ctx_dev_free(st->ctx, st->E_in);
    delete st;
    return COZK_OK;
}

size_t cozk_outer_len(const cozk_outer* st) { return st ? st->L : 0; }

// current Az, Bz, Cz -> host (tests): each L x 4 u64 per component; b pointers may be NULL
int cozk_outer_download(cozk_ctx* ctx, const cozk_outer* st, uint64_t* az_a, uint64_t* az_b, uint64_t* bz_a, uint64_t* bz_b, uint64_t* cz_a, uint64_t* cz_b) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && st, "outer_download: bad argument");
        uint64_t* dst[3][2] = {{az_a, az_b}, {bz_a, bz_b}, {cz_a, cz_b}};
        const size_t num_steps = st->L / st->per_step, stored = num_steps * st->act_rows;
        std::vector<fe> tmp(st->act_rows < st->per_step ? stored : 0);
        for (int q = 0; q < 3; q++)
            for (int c = 0; c < 2; c++) {
                if (!dst[q][c] || !st->buf[st->cur][q][c]) continue;
                if (st->act_rows == st->per_step) {
                    HIP_TRY(hipMemcpyAsync(dst[q][c], st->buf[st->cur][q][c], st->L * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
                    HIP_TRY(hipStreamSynchronize(ctx->stream));
                    continue;
                }
                // compact storage -> the dense-equivalent rows the caller asked for (the rows that are not stored are zero)
                HIP_TRY(hipMemcpyAsync(tmp.data(), st->buf[st->cur][q][c], stored * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                memset(dst[q][c], 0, st->L * sizeof(fe));
                for (size_t step = 0; step < num_steps; step++)
                    memcpy(dst[q][c] + 4 * step * st->per_step, tmp.data() + step * st->act_rows, st->act_rows * sizeof(fe));
            }
    });
}

// everything of one bind but the kernel: the layer moves on to its other ping-pong side and halves, and GruenSplitEqPolynomial::bind
// folds eq(w_i, r) into the scalar and drops the last variable of E_in (then of E_out)
static void outer_bind_state(cozk_outer* st, const fe& r) {
    if (st->per_step > 1) {
        st->per_step /= 2;
        st->act_rows = (st->act_rows + 1) / 2;
    }
    st->cur = 1 - st->cur;
    st->L /= 2;
    const fe& w = st->w[st->current_index - 1];
    fe wr = Fr::mul(w, r);
    st->current_scalar = Fr::mul(st->current_scalar, Fr::add(Fr::sub(Fr::sub(Fr::one(), w), r), Fr::dbl(wr)));
    st->current_index -= 1;
    if ((int)(st->w.size() / 2) < st->current_index) st->n_in -= 1;
    else if (0 < st->current_index) st->n_out -= 1;
}

// Would the split-eq tables cover the row pairs of the round that follows -- after one more bind, if `bind` -- exactly?  Asked BEFORE
// that bind (the counts move as outer_bind_state moves them), so a refusal finds the handle as it was.  An internal invariant: create
// sets L = 2^n_tau, current_index = n_tau and n_in + n_out = n_tau - 1, and every bind with current_index >= 2 halves L and takes one
// variable off n_in or n_out, so no sequence of calls through the API makes it false.  Needs current_index >= (bind ? 2 : 1).
static bool outer_eq_in_step(const cozk_outer* st, bool bind) {
    size_t n_in = st->n_in, n_out = st->n_out;
    if (bind) {
        if ((int)(st->w.size() / 2) < st->current_index - 1) n_in -= 1;
        else n_out -= 1;
    }
    return (bind ? st->L / 4 : st->L / 2) == ((size_t)1 << (n_in + n_out));
}

static void outer_bind(cozk_ctx* ctx, cozk_outer* st, const fe& r) {
    const int NC = st->mode == COZK_MODE_REP3 ? 2 : 1;
    const int dst = 1 - st->cur;
    const size_t n_out = st->L / 2;
    OuterBindArgs a{};
    int k = 0;
    for (int q = 0; q < 3; q++)
        for (int c = 0; c < NC; c++) {
            a.in[k] = st->buf[st->cur][q][c];
            a.out[k] = st->buf[dst][q][c];
            k++;
        }
    if (st->per_step > 1) {
        const size_t num_steps = st->L / st->per_step, act_out = (st->act_rows + 1) / 2;
        dim3 g(grid_for(num_steps * act_out), (unsigned)k);
        k_outer_bind_act<<<g, PT, 0, ctx->stream>>>(a, (uint32_t)num_steps, (uint32_t)st->per_step, (uint32_t)st->act_rows, r);
    } else {
        dim3 g(grid_for(n_out), (unsigned)k);
        k_outer_bind<<<g, PT, 0, ctx->stream>>>(a, n_out, r);
    }
    HIP_TRY(hipGetLastError());
    outer_bind_state(st, r);
}

// The 9 x 29 kernel takes the rounds over compact (active-row) storage that are throughput-bound: OUTER_F9_MIN_PAIRS row pairs or
// more.  COZK_OUTER_F9=0: the saturated kernel everywhere.
static constexpr size_t OUTER_F9_MIN_PAIRS = 1024;
static bool outer_use_f9(size_t act_pairs) {
    static const bool f9_env = !(getenv("COZK_OUTER_F9") && atoi(getenv("COZK_OUTER_F9")) == 0);
    return f9_env && act_pairs >= OUTER_F9_MIN_PAIRS;
}

// one round of prove_spartan_cubic_sumcheck: bind with the previous challenge (NULL in the first round), the quadratic
// evaluations, and the cubic round polynomial as process_eq_sumcheck_round_worker forms it (sumcheck_spartan.rs:44-79).
// claim = this party's additive share of the running claim; out_coeffs = 4 additive coefficient shares (low -> high).
int cozk_outer_round(cozk_ctx* ctx, cozk_outer* st, const uint64_t* r, const uint64_t claim[4], uint64_t out_coeffs[16]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && st && claim && out_coeffs, "outer_round: bad argument");
        // every check before the bind: a refused call leaves the handle as it was, and launches nothing
        COZK_REQUIRE(st->L >= 2 && st->current_index >= 1, "outer_round: fully bound");
        COZK_REQUIRE(!r || (st->L >= 4 && st->current_index >= 2),
                     "outer_round: nothing left to sum after this bind (the last challenge goes to cozk_outer_final_evals)");
        COZK_REQUIRE(outer_eq_in_step(st, r != nullptr), "outer_round: split-eq tables out of step with the layer");
        if (r) outer_bind(ctx, st, fe_from_u64x4(r));
        const size_t npairs = st->L / 2;
        const bool act = st->per_step > 1;
        const size_t num_steps = st->L / st->per_step;
        const size_t act_pairs = num_steps * ((st->act_rows + 1) / 2);
        const unsigned gx = sum_grid(grid_capped(act ? act_pairs : npairs, ROUND_GRID_MAX));
        const SumLaunch sl = sum_launch(ctx, 3, gx, 3);
        const fe* E_in = st->E_in + (((size_t)1 << st->n_in) - 1);
        const fe* E_out = st->E_out + (((size_t)1 << st->n_out) - 1);
        const int want_t0 = st->round > 0 ? 1 : 0;
        const bool rep3 = st->mode == COZK_MODE_REP3;
        auto& b = st->buf[st->cur];
        const fe *az_b = rep3 ? b[0][1] : nullptr, *bz_b = rep3 ? b[1][1] : nullptr, *cz_b = rep3 ? b[2][1] : nullptr;
        if (act) {
            auto* const kernel = outer_use_f9(act_pairs) ? (rep3 ? k_outer_round_act9<2> : k_outer_round_act9<1>) : (rep3 ? k_outer_round_act<2> : k_outer_round_act<1>);
            kernel<<<gx, PT, 0, ctx->stream>>>(b[0][0], az_b, b[1][0], bz_b, b[2][0], cz_b, (uint32_t)num_steps, (uint32_t)st->per_step, (uint32_t)st->act_rows, E_in,
                                               (int)st->n_in, E_out, want_t0, sl.partial);
        } else {
            auto* const kernel = rep3 ? k_outer_round<2> : k_outer_round<1>;
            kernel<<<gx, PT, 0, ctx->stream>>>(b[0][0], az_b, b[1][0], bz_b, b[2][0], cz_b, npairs, E_in, (int)st->n_in, E_out, want_t0, sl.partial);
        }
        fe s[3];
        finish_sums(ctx, sl, 3, gx, Fr::one(), 0, s);
        fe t0 = Fr::zero();
        if (want_t0) t0 = Fr::sub(s[0], st->mode == COZK_MODE_REP3 ? Fr::mul(s[1], fr_two_inv()) : s[1]);
        fe tinf = s[2];
        // UniPoly::from_linear_times_quadratic_with_hint([scalar - scalar w, 2 scalar w - scalar], t0, tinf, claim)
        fe sw = Fr::mul(st->current_scalar, st->w[st->current_index - 1]);
        fe l0 = Fr::sub(st->current_scalar, sw), l1 = Fr::sub(Fr::dbl(sw), st->current_scalar);
        fe hint = fe_from_u64x4(claim);
        fe c0 = Fr::mul(l0, t0);
        fe t1 = Fr::sub(Fr::sub(Fr::mul(Fr::sub(hint, c0), Fr::inv(Fr::add(l0, l1))), t0), tinf);
        fe cf[4] = {c0, Fr::add(Fr::mul(l0, t1), Fr::mul(l1, t0)), Fr::add(Fr::mul(l0, tinf), Fr::mul(l1, t1)), Fr::mul(l1, tinf)};
        for (int i = 0; i < 4; i++) fe_to_u64x4(cf[i], out_coeffs + 4 * i);
        st->round++;
    });
}

// final_sumcheck_evals (spartan_interleaved_poly.rs:648-664) after binding with the last challenge: this party's additive
// Az(r), Bz(r), Cz(r)
int cozk_outer_final_evals(cozk_ctx* ctx, cozk_outer* st, const uint64_t r[4], uint64_t out[12]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && st && r && out && st->L == 2, "outer_final_evals: one unbound variable must be left");
        outer_bind(ctx, st, fe_from_u64x4(r));
        const int NC = st->mode == COZK_MODE_REP3 ? 2 : 1;
        fe h[6];
        ctx->scratch.reserve(6 * sizeof(fe));
        fe* d = ctx->scratch.as<fe>();
        for (int q = 0; q < 3; q++)
            for (int c = 0; c < NC; c++) HIP_TRY(hipMemcpyAsync(d + 2 * q + c, st->buf[st->cur][q][c], sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h, d, 6 * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int q = 0; q < 3; q++) {
            fe v = NC == 2 ? Fr::mul(Fr::add(h[2 * q], h[2 * q + 1]), fr_two_inv()) : h[2 * q];  // into_additive
            fe_to_u64x4(v, out + 4 * q);
        }
    });
}

}  // extern "C"
