// co-noir-spartan's PUBLIC lookup round (SURVEY 8(f)4; co-noir-spartan/co-spartan/src/worker.rs:400-575 fourth_round,
// :694-724 distributed_sumcheck_worker; co-noir-spartan/spartan/src/logup.rs:31-80 LogLookupProof::prove;
// co-noir-spartan/co-spartan/src/sumcheck.rs:459-500 append_sumcheck_polys) -- part of poly.hip's translation unit.
// Everything here works on plain Fr data (no shares): the sparse-matrix memory check of Spartan is public.
//
//   cozk_hash_tuple        hash_tuple (worker.rs:836-846): out[j] = idx[j] + v * eq[idx[j]], padded with out[0]
//   cozk_logup_h           LogLookupProof::prove's field work: phi = x + values; h = m / phi (or 1 / phi) -- one pass, the
//                          inversion per element by Fermat (a batch-inversion tree saves multiplications on a CPU; on this
//                          machine 2^18 independent 380-product chains are ~1 ms and need no second pass over the data)
//   cozk_vec_boost_degree  boost_degree (spartan/src/utils.rs:11-27): scale by 2^-(new - old), repeat 2^(new - old) times
//   cozk_prodlist_*        IPForMLSumcheck::{prover_init, prove_round} of ark-linear-sumcheck (out of tree, fork e0500b8)
//                          over a ListOfProductsOfPolynomials: per round the evaluations at t = 0 .. max_multiplicands of
//                          sum_b sum_products coef * prod_j (P_j[2b] + t (P_j[2b+1] - P_j[2b])), then fix_variables (the
//                          FIRST variable = index bit 0: LowToHigh) with the verifier's randomness

static constexpr int PL_MAX_POLYS = 48;
static constexpr int PL_MAX_TERMS = 32;
static constexpr int PL_MAX_FACTORS = 4;
static constexpr int PL_MAX_DEG = 4;

struct ProdListDev {
    int n_polys, n_terms, degree;
    const fe* poly[PL_MAX_POLYS];
    fe coef[PL_MAX_TERMS];
    int n_factors[PL_MAX_TERMS];
    int factor[PL_MAX_TERMS][PL_MAX_FACTORS];
};

struct cozk_prodlist {
    cozk_ctx* ctx;
    int num_vars;
    size_t n;                 // current length of every polynomial
    int n_polys;
    fe* store[2];             // ping-pong: polynomial p at store[w] + p * cap[w]
    size_t cap[2];
    int cur;
    ProdListDev desc;
    ProdListDev* d_desc;
};

__global__ void __launch_bounds__(PT) k_hash_tuple(const uint32_t* __restrict__ idx, size_t n_real, const fe* __restrict__ eq, fe v, fe* __restrict__ out,
                                                size_t n_out) {
    size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_out) return;
    uint32_t i = idx[j < n_real ? j : 0];  // the tail repeats entry 0 (worker.rs:842-844)
    fe x = Fr::zero();
    x.l[0] = i;
    fe_store(out + j, Fr::add(Fr::to_mont(x), Fr::mul(v, fe_load(eq + i))));
}

// out[j] = src[idx[j]] for j < n_real (0xffffffff = usize::MAX: no entry), 0 on the padding: eq_tilde_{rx,ry}(_chunk) of
// third_round (worker.rs:296-343, 376-391)
__global__ void __launch_bounds__(PT) k_vec_gather(const uint32_t* __restrict__ idx, size_t n_real, const fe* __restrict__ src, size_t n_src, fe* __restrict__ out,
                                                size_t n_out) {
    size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_out) return;
    fe v = Fr::zero();
    if (j < n_real) {
        uint32_t i = idx[j];
        if (i != 0xffffffffu && i < n_src) v = fe_load(src + i);
    }
    fe_store(out + j, v);
}

__global__ void __launch_bounds__(PT) k_logup_h(const fe* __restrict__ vals, const fe* __restrict__ m, size_t n, fe x, fe* __restrict__ phi,
                                             fe* __restrict__ h) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe p = Fr::add(x, fe_load(vals + i));
    fe_store(phi + i, p);
    fe inv = Fr::inv(p);
    fe_store(h + i, m ? Fr::mul(fe_load(m + i), inv) : inv);
}

__global__ void __launch_bounds__(PT) k_boost_degree(const fe* __restrict__ in, size_t n_in, fe factor, fe* __restrict__ out, size_t n_out) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n_out) return;
    fe_store(out + i, Fr::mul(fe_load(in + (i & (n_in - 1))), factor));
}

__global__ void __launch_bounds__(PT) k_prodlist_round(const ProdListDev* __restrict__ dp, size_t half, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ ProdListDev d;
    for (size_t k = threadIdx.x; k < sizeof(ProdListDev) / 4; k += PT) ((uint32_t*)&d)[k] = ((const uint32_t*)dp)[k];
    __syncthreads();
    fe acc[PL_MAX_DEG + 1];
    for (int t = 0; t <= PL_MAX_DEG; t++) acc[t] = Fr::zero();
    const int D = d.degree;
    for (size_t b = (size_t)blockIdx.x * PT + threadIdx.x; b < half; b += (size_t)gridDim.x * PT) {
        for (int q = 0; q < d.n_terms; q++) {
            fe prod[PL_MAX_DEG + 1];
            for (int t = 0; t <= D; t++) prod[t] = d.coef[q];
            for (int j = 0; j < d.n_factors[q]; j++) {
                const fe* tab = d.poly[d.factor[q][j]];
                fe start = fe_load(tab + 2 * b), step = Fr::sub(fe_load(tab + 2 * b + 1), start);
                for (int t = 0; t <= D; t++) {
                    prod[t] = Fr::mul(prod[t], start);
                    start = Fr::add(start, step);
                }
            }
            for (int t = 0; t <= D; t++) acc[t] = Fr::add(acc[t], prod[t]);
        }
    }
    for (int t = 0; t <= D; t++) {
        fe v = fr_block_sum(acc[t], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)t * gridDim.x + blockIdx.x, v);
    }
}

extern "C" {

int cozk_hash_tuple(cozk_ctx* ctx, const cozk_vec* idx, const cozk_vec* eq, const uint64_t v_msg[4], size_t n_out, cozk_vec** out) {
    if (!out) return COZK_ERR_INVALID_ARG;
    *out = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && idx && eq && v_msg && idx->kind == COZK_SCALAR_U32 && eq->kind == COZK_SCALAR_FR && idx->n >= 1 && n_out >= idx->n,
                     "hash_tuple: idx (U32, non-empty), eq (FR), n_out >= idx.len()");
    });
    if (rc != COZK_OK) return rc;
    rc = cozk_vec_alloc(ctx, n_out, COZK_SCALAR_FR, out);
    if (rc != COZK_OK) return rc;
    return cozk_guard(ctx, [&] {
        k_hash_tuple<<<grid_for(n_out), PT, 0, ctx->stream>>>((const uint32_t*)idx->d, idx->n, (const fe*)eq->d, fe_from_u64x4(v_msg), (fe*)(*out)->d, n_out);
        HIP_TRY(hipGetLastError());
    });
}

int cozk_vec_gather(cozk_ctx* ctx, const cozk_vec* idx, const cozk_vec* src, size_t n_out, cozk_vec** out) {
    if (!out) return COZK_ERR_INVALID_ARG;
    *out = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && idx && src && idx->kind == COZK_SCALAR_U32 && src->kind == COZK_SCALAR_FR && n_out >= idx->n && n_out >= 1,
                     "vec_gather: idx (U32), src (FR), n_out >= idx.len()");
    });
    if (rc != COZK_OK) return rc;
    rc = cozk_vec_alloc(ctx, n_out, COZK_SCALAR_FR, out);
    if (rc != COZK_OK) return rc;
    return cozk_guard(ctx, [&] {
        k_vec_gather<<<grid_for(n_out), PT, 0, ctx->stream>>>((const uint32_t*)idx->d, idx->n, (const fe*)src->d, src->n, (fe*)(*out)->d, n_out);
        HIP_TRY(hipGetLastError());
    });
}

// phi = x + values, h = m / phi (m = NULL: 1 / phi): LogLookupProof::prove (logup.rs:45-70)
int cozk_logup_h(cozk_ctx* ctx, const cozk_vec* values, const cozk_vec* m, const uint64_t x[4], cozk_vec** out_phi, cozk_vec** out_h) {
    if (!out_phi || !out_h) return COZK_ERR_INVALID_ARG;
    *out_phi = *out_h = nullptr;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && values && x && values->kind == COZK_SCALAR_FR && (!m || (m->kind == COZK_SCALAR_FR && m->n == values->n)), "logup_h: bad argument");
    });
    if (rc != COZK_OK) return rc;
    rc = cozk_vec_alloc(ctx, values->n, COZK_SCALAR_FR, out_phi);
    if (rc == COZK_OK) rc = cozk_vec_alloc(ctx, values->n, COZK_SCALAR_FR, out_h);
    if (rc != COZK_OK) return rc;
    return cozk_guard(ctx, [&] {
        if (values->n == 0) return;
        k_logup_h<<<grid_for(values->n), PT, 0, ctx->stream>>>((const fe*)values->d, m ? (const fe*)m->d : nullptr, values->n, fe_from_u64x4(x), (fe*)(*out_phi)->d,
                                                              (fe*)(*out_h)->d);
        HIP_TRY(hipGetLastError());
    });
}

int cozk_vec_boost_degree(cozk_ctx* ctx, const cozk_vec* v, int new_num_vars, cozk_vec** out) {
    if (!out) return COZK_ERR_INVALID_ARG;
    *out = nullptr;
    size_t n_out = 0;
    int dd = 0;
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && v && v->kind == COZK_SCALAR_FR && v->n >= 1 && (v->n & (v->n - 1)) == 0 && new_num_vars >= 0 && new_num_vars <= 40, "boost_degree: bad argument");
        int nv = 0;
        while (((size_t)1 << nv) < v->n) nv++;
        COZK_REQUIRE(new_num_vars >= nv, "boost_degree: new_dim >= num_vars");
        dd = new_num_vars - nv;
        n_out = (size_t)1 << new_num_vars;
    });
    if (rc != COZK_OK) return rc;
    rc = cozk_vec_alloc(ctx, n_out, COZK_SCALAR_FR, out);
    if (rc != COZK_OK) return rc;
    return cozk_guard(ctx, [&] {
        fe two = Fr::from_u64(2), p = Fr::one();
        for (int i = 0; i < dd; i++) p = Fr::mul(p, two);
        k_boost_degree<<<grid_for(n_out), PT, 0, ctx->stream>>>((const fe*)v->d, v->n, Fr::inv(p), (fe*)(*out)->d, n_out);
        HIP_TRY(hipGetLastError());
    });
}

// IPForMLSumcheck::prover_init over ListOfProductsOfPolynomials: polys = the flattened multilinear extensions (copied),
// product q = coefs[q] * prod_{j < counts[q]} polys[factor_idx[first + j]]
int cozk_prodlist_create(cozk_ctx* ctx, const cozk_vec* const* polys, size_t n_polys, const uint64_t* coefs, const int* counts, const int* factor_idx,
                         size_t n_terms, cozk_prodlist** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && n_polys >= 1 && n_polys <= PL_MAX_POLYS && coefs && counts && factor_idx && n_terms >= 1 && n_terms <= PL_MAX_TERMS && out,
                     "prodlist_create: bad argument");
        COZK_REQUIRE(polys[0], "prodlist_create: null polynomial");
        const size_t n = polys[0]->n;
        COZK_REQUIRE(n >= 1 && (n & (n - 1)) == 0, "prodlist_create: power-of-two polynomials");
        struct Guard {  // argument checks follow the allocations: free what exists if one of them throws
            cozk_prodlist* p;
            ~Guard() { cozk_prodlist_free(p); }
        } guard{new cozk_prodlist()};
        cozk_prodlist* pl = guard.p;
        pl->ctx = ctx;
        pl->store[0] = pl->store[1] = nullptr;
        pl->d_desc = nullptr;
        pl->n = n;
        pl->num_vars = 0;
        while (((size_t)1 << pl->num_vars) < n) pl->num_vars++;
        pl->n_polys = (int)n_polys;
        pl->cap[0] = n;
        pl->cap[1] = n > 1 ? n / 2 : 1;
        for (int w = 0; w < 2; w++) pl->store[w] = dev_alloc_fe(n_polys * pl->cap[w]);
        pl->cur = 0;
        for (size_t p = 0; p < n_polys; p++) {
            COZK_REQUIRE(polys[p] && polys[p]->kind == COZK_SCALAR_FR && polys[p]->n == n, "prodlist_create: every polynomial has the same length");
            HIP_TRY(hipMemcpyAsync(pl->store[0] + p * n, polys[p]->d, n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
        }
        ProdListDev& d = pl->desc;
        memset(&d, 0, sizeof d);
        d.n_polys = (int)n_polys;
        d.n_terms = (int)n_terms;
        d.degree = 0;
        size_t first = 0;
        for (size_t q = 0; q < n_terms; q++) {
            COZK_REQUIRE(counts[q] >= 1 && counts[q] <= PL_MAX_FACTORS, "prodlist_create: 1..4 factors per product");
            d.coef[q] = fe_from_u64x4(coefs + 4 * q);
            d.n_factors[q] = counts[q];
            for (int j = 0; j < counts[q]; j++) {
                int f = factor_idx[first + j];
                COZK_REQUIRE(f >= 0 && (size_t)f < n_polys, "prodlist_create: factor index out of range");
                d.factor[q][j] = f;
            }
            first += counts[q];
            if (counts[q] > d.degree) d.degree = counts[q];  // max_multiplicands
        }
        pl->d_desc = (ProdListDev*)ctx_dev_alloc(ctx, sizeof(ProdListDev));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        guard.p = nullptr;
        *out = pl;
    });
}

int cozk_prodlist_free(cozk_prodlist* pl) {
    if (!pl) return COZK_OK;
    for (int w = 0; w < 2; w++) ctx_dev_free(pl->ctx, pl->store[w]);
    ctx_dev_free(pl->ctx, pl->d_desc);
    delete pl;
    return COZK_OK;
}

int cozk_prodlist_degree(const cozk_prodlist* pl) { return pl ? pl->desc.degree : 0; }

static void prodlist_fix(cozk_ctx* ctx, cozk_prodlist* pl, const fe& r) {
    const int dst = 1 - pl->cur;
    const size_t n_out = pl->n / 2;
    dim3 g(grid_for(n_out), (unsigned)pl->n_polys);
    k_primary_bind<<<g, PT, 0, ctx->stream>>>(pl->store[pl->cur], pl->cap[pl->cur], pl->store[dst], pl->cap[dst], n_out, r);
    HIP_TRY(hipGetLastError());
    pl->cur = dst;
    pl->n = n_out;
}

// IPForMLSumcheck::prove_round: fix_variables with the previous randomness (NULL in the first round), then the
// (max_multiplicands + 1) evaluations at t = 0 .. max_multiplicands
int cozk_prodlist_round(cozk_ctx* ctx, cozk_prodlist* pl, const uint64_t* r, uint64_t* out_evals) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && pl && out_evals, "prodlist_round: bad argument");
        // every check before the fix: a refused call leaves the list as it was, and launches nothing
        COZK_REQUIRE(!r || pl->n >= 2, "prodlist_round: fully fixed");
        COZK_REQUIRE(pl->n >= 2, "prodlist_round: no variable left");
        COZK_REQUIRE(!r || pl->n >= 4, "prodlist_round: nothing left to sum after this fix (the last randomness goes to cozk_prodlist_final)");
        if (r) prodlist_fix(ctx, pl, fe_from_u64x4(r));
        for (int p = 0; p < pl->n_polys; p++) pl->desc.poly[p] = pl->store[pl->cur] + (size_t)p * pl->cap[pl->cur];
        HIP_TRY(hipMemcpyAsync(pl->d_desc, &pl->desc, sizeof(ProdListDev), hipMemcpyHostToDevice, ctx->stream));
        const size_t half = pl->n / 2;
        const int D = pl->desc.degree;
        const unsigned gx = grid_capped(half, ROUND_GRID_MAX);
        const SumLaunch sl = sum_launch(ctx, D + 1, gx, D + 1);
        k_prodlist_round<<<gx, PT, 0, ctx->stream>>>(pl->d_desc, half, sl.partial);
        fe s[PL_MAX_DEG + 1];
        finish_sums(ctx, sl, D + 1, gx, Fr::one(), 0, s);
        for (int t = 0; t <= D; t++) fe_to_u64x4(s[t], out_evals + 4 * t);
    });
}

// the last fix_variables + obtain_distrbuted_sumcheck_prover_state (co-spartan/src/sumcheck.rs:434-452): every flattened
// polynomial's single remaining evaluation (n_polys x 4 u64)
int cozk_prodlist_final(cozk_ctx* ctx, cozk_prodlist* pl, const uint64_t r[4], uint64_t* out_vals) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && pl && r && out_vals && pl->n == 2, "prodlist_final: one variable must be left");
        prodlist_fix(ctx, pl, fe_from_u64x4(r));
        std::vector<fe> h((size_t)pl->n_polys);
        HIP_TRY(hipMemcpy2DAsync(h.data(), sizeof(fe), pl->store[pl->cur], pl->cap[pl->cur] * sizeof(fe), sizeof(fe), (size_t)pl->n_polys, hipMemcpyDeviceToHost,
                                 ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int p = 0; p < pl->n_polys; p++) fe_to_u64x4(h[p], out_vals + 4 * p);
    });
}

}  // extern "C"
