// co-jolt's Spartan INNER and SHIFT sumchecks (SURVEY 8(f)2, r1cs/spartan/worker.rs:100-275) -- the device operators they
// need beyond the polynomial seam; part of poly.hip's translation unit.
//
//   cozk_eq_plus_one_evals        EqPlusOnePolynomial::evals(rx_step, None) (jolt-core, out of tree; worker.rs:116): the table
//                                 eq_plus_one(r, y) over y (big-endian), eq_plus_one(x, y) = [y = x + 1], x < 2^l - 1
//   cozk_poly_batch_dot_public    bind_z / bind_shift_z (worker.rs:139-152): dot_product_with_public of every flattened
//                                 witness polynomial with ONE or TWO public vectors in one pass over the polynomials
//
// The inner sumcheck itself runs over MixedPolynomials of 4 * num_vars_padded = 512 entries (host, prover.hpp); the shift
// sumcheck is prove_arbitrary_worker over (sum_i eq_ry[i] poly_i, eq_plus_one) = cozk_poly_linear_combination +
// cozk_prod_sumcheck_evals + cozk_poly_bind.

struct EqP1Args {
    fe r[30];
    int l;
};
// y != 0 with k trailing zero bits: x = y - 1 has its low k bits set, bit k clear, the high bits of y:
// eq_plus_one(r, y) = prod_{j < k} r_low(j) * (1 - r_low(k)) * eq(r_high, y_high)         (r_low(j) = r[l - 1 - j])
__global__ void __launch_bounds__(PT) k_eq_plus_one(EqP1Args a, fe* __restrict__ out, size_t n) {
    size_t y = (size_t)blockIdx.x * PT + threadIdx.x;
    if (y >= n) return;
    if (y == 0) {
        fe_store(out, Fr::zero());
        return;
    }
    const int l = a.l;
    const int k = __ffsll((long long)y) - 1;
    fe v = Fr::sub(Fr::one(), a.r[l - 1 - k]);
    for (int j = 0; j < k; j++) v = Fr::mul(v, a.r[l - 1 - j]);
    const size_t hi = y >> (k + 1);
    const int m = l - k - 1;
    for (int j = 0; j < m; j++) {
        const fe& rj = a.r[j];
        v = Fr::mul(v, ((hi >> (m - 1 - j)) & 1) ? rj : Fr::sub(Fr::one(), rj));
    }
    fe_store(out + y, v);
}

// partial[((p * NP + q) * 2 + c) * gridDim.x + blockIdx.x] = sum over this block's stride of component c of poly p times pub q;
// a polynomial without a b component (public, or the plain prover) leaves its c = 1 slots zero
template <int NP>
__global__ void __launch_bounds__(PT) k_poly_batch_dot_public(const fe* const* __restrict__ pa, const fe* const* __restrict__ pb, size_t n,
                                                           const fe* __restrict__ pub0, const fe* __restrict__ pub1, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const int p = blockIdx.y;
    const fe* a = pa[p];
    const fe* b = pb[p];
    FrWide wa[NP], wb[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) {
        fr_wide_zero(wa[q]);
        fr_wide_zero(wb[q]);
    }
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < n; i += (size_t)gridDim.x * PT) {
        fe va = fe_load(a + i);
        fe c0 = fe_load(pub0 + i);
        fr_wide_mac(wa[0], va, c0);
        fe c1;
        if (NP == 2) {
            c1 = fe_load(pub1 + i);
            fr_wide_mac(wa[NP - 1], va, c1);
        }
        if (b) {  // uniform per workgroup row
            fe vb = fe_load(b + i);
            fr_wide_mac(wb[0], vb, c0);
            if (NP == 2) fr_wide_mac(wb[NP - 1], vb, c1);
        }
    }
#pragma unroll
    for (int q = 0; q < NP; q++) {
        fe v = fr_block_sum(fr_wide_reduce(wa[q]), sh4);
        if (threadIdx.x == 0) fe_store(partial + ((size_t)(p * NP + q) * 2 + 0) * gridDim.x + blockIdx.x, v);
        v = b ? fr_block_sum(fr_wide_reduce(wb[q]), sh4) : Fr::zero();
        if (threadIdx.x == 0) fe_store(partial + ((size_t)(p * NP + q) * 2 + 1) * gridDim.x + blockIdx.x, v);
    }
}

extern "C" {

int cozk_eq_plus_one_evals(cozk_ctx* ctx, const uint64_t* r, int nv, cozk_vec** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && out && nv >= 0 && nv <= 30 && (r || nv == 0), "eq_plus_one_evals: bad argument (nv <= 30)");
        const size_t n = (size_t)1 << nv;
        EqP1Args a{};
        a.l = nv;
        for (int j = 0; j < nv; j++) a.r[j] = fe_from_u64x4(r + 4 * j);
        fe* d = dev_alloc_fe(n);
        k_eq_plus_one<<<grid_for(n), PT, 0, ctx->stream>>>(a, d, n);
        HIP_TRY(hipGetLastError());
        *out = new cozk_vec{ctx, n, COZK_SCALAR_FR, d, n * sizeof(fe), true};
    });
}

// out[(p * n_pub + q) * 8 ..] = (a[4], b[4]) of dot_product_with_public(poly_p, pub_q) (dense_mlpoly.rs:228-234); b = 0 for a
// PLAIN polynomial (a public polynomial's dot product is a public value, multilinear_polynomial.rs)
int cozk_poly_batch_dot_public(cozk_ctx* ctx, const cozk_poly* const* polys, size_t k, const cozk_vec* const* pubs, size_t n_pub, uint64_t* out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && polys && k > 0 && pubs && (n_pub == 1 || n_pub == 2) && out, "batch_dot_public: bad argument (one or two public vectors)");
        COZK_REQUIRE(polys[0], "batch_dot_public: null polynomial");
        const size_t n = polys[0]->len;
        for (size_t q = 0; q < n_pub; q++) COZK_REQUIRE(pubs[q] && pubs[q]->kind == COZK_SCALAR_FR && pubs[q]->n == n, "batch_dot_public: length mismatch (zip_eq)");
        std::vector<const fe*> ha(k), hb(k);
        for (size_t i = 0; i < k; i++) {
            COZK_REQUIRE(polys[i] && polys[i]->len == n, "batch_dot_public: polynomials of one length");
            ha[i] = poly_a(polys[i]);
            hb[i] = polys[i]->mode == COZK_MODE_REP3 ? poly_b(polys[i]) : nullptr;
        }
        const unsigned gx = grid_capped(n, EVAL_GRID_MAX);  // few, long lanes: one wide reduction per accumulator per lane (as k_poly_eval_chi)
        const size_t n_out = k * n_pub * 2;
        const SumLaunch sl = sum_launch(ctx, (unsigned)n_out, gx, n_out, 2 * k * sizeof(void*));
        fe* partial = sl.partial;
        const fe** da = (const fe**)sl.meta;
        const fe** db = da + k;
        HIP_TRY(hipMemcpyAsync(da, ha.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(db, hb.data(), k * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
        dim3 grid(gx, (unsigned)k);
        if (n_pub == 2) k_poly_batch_dot_public<2><<<grid, PT, 0, ctx->stream>>>(da, db, n, (const fe*)pubs[0]->d, (const fe*)pubs[1]->d, partial);
        else k_poly_batch_dot_public<1><<<grid, PT, 0, ctx->stream>>>(da, db, n, (const fe*)pubs[0]->d, nullptr, partial);
        std::vector<fe> h(n_out);
        finish_sums(ctx, sl, (unsigned)n_out, gx, Fr::one(), 0, h.data());
        for (size_t i = 0; i < n_out; i++) fe_to_u64x4(h[i], out + 4 * i);
    });
}

}  // extern "C"
