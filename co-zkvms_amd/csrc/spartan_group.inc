// Spartan groups (cozk_spartan_group_*): one round of a co-noir-spartan sumcheck for k members against ONE public polynomial -- the
// senders of a Shamir prover (csrc/host/shamir_spartan.hpp), each a party with a context of its own on one device.  Part of poly.hip's
// translation unit (cozk_poly, the round-sum helpers).
//
//   FIRST   member = (za, zb, zc), public = eq:   g_m(X) = sum_b pub(X) (za_m(X) zb_m(X) - zc_m(X)),  X = 0..3   (k_spartan_first)
//   SECOND  member = (z),          public = lin:  g_m(X) = sum_b pub(X) z_m(X),                       X = 0..2   (k_spartan_second with
//           lin = alpha A + beta B + gamma C formed once in front of the rounds)
//
// LowToHigh pairs (2b, 2b + 1).  Field arithmetic is exact and every stored value canonical, so pub (za zb - zc) summed in one
// accumulator is byte for byte the accp - accc of the per-poly call, and z lin that of z (alpha a + beta b + gamma c).
//
// One launch per round whatever k is: blockIdx.y is the member, blockIdx.x strides over the pairs.  With a challenge the bind is FUSED
// with the sums, in the manner of k_layer_bind_cubic: a lane reads the four elements 4b .. 4b + 3 of every plane and of the public
// polynomial, binds them to the pair (2b, 2b + 1) of the next round, stores the pair and adds its terms -- the planes are read once per
// round instead of twice, and a round is 2 launches (this one and k_finish_sums) instead of 5 per member.  Every member row binds the
// public polynomial for itself (2 of its 14 / 6 lerps and products per pair); only row 0 stores it, into the OTHER ping-pong buffer
// of the group, so no workgroup reads what another one writes.
struct SpartanGroupArgs {
    const fe* in[3 * COZK_LAYER_GROUP_MAX];  // plane j of member m at [P m + j]: scalar loads indexed by the wave-uniform blockIdx.y
    fe* out[3 * COZK_LAYER_GROUP_MAX];       // the bound planes (BIND only)
};

template <int P, int BIND>
__global__ void __launch_bounds__(PT) k_spartan_group_round(SpartanGroupArgs a, const fe* __restrict__ pub_in, fe* pub_out, size_t pairs, fe r,
                                                         fe* __restrict__ partial) {
    constexpr int E = P == 3 ? 4 : 3;
    __shared__ fe sh4[4];
    const unsigned m = blockIdx.y;
    fe acc[E];
    for (int e = 0; e < E; e++) acc[e] = Fr::zero();
    for (size_t b = (size_t)blockIdx.x * PT + threadIdx.x; b < pairs; b += (size_t)gridDim.x * PT) {
        fe v[P + 1], s[P + 1];  // the pair's value at X and its step; [P] = the public polynomial
#pragma unroll
        for (int j = 0; j <= P; j++) {
            const fe* in = j < P ? a.in[P * m + j] : pub_in;
            fe lo, hi;
            if (BIND) {
                const fe x0 = fe_load(in + 4 * b), x1 = fe_load(in + 4 * b + 1), x2 = fe_load(in + 4 * b + 2), x3 = fe_load(in + 4 * b + 3);
                lo = Fr::add(x0, Fr::mul(Fr::sub(x1, x0), r));
                hi = Fr::add(x2, Fr::mul(Fr::sub(x3, x2), r));
                fe* out = j < P ? a.out[P * m + j] : pub_out;
                if (j < P || m == 0) {
                    fe_store(out + 2 * b, lo);
                    fe_store(out + 2 * b + 1, hi);
                }
            } else {
                lo = fe_load(in + 2 * b);
                hi = fe_load(in + 2 * b + 1);
            }
            v[j] = lo;
            s[j] = Fr::sub(hi, lo);
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const fe t = P == 3 ? Fr::sub(Fr::mul(v[0], v[1]), v[2]) : v[0];
            acc[e] = Fr::add(acc[e], Fr::mul(t, v[P]));
            if (e + 1 < E) {
#pragma unroll
                for (int j = 0; j <= P; j++) v[j] = Fr::add(v[j], s[j]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        const fe t = fr_block_sum(acc[e], sh4);
        if (threadIdx.x == 0) fe_store(partial + ((size_t)m * E + e) * gridDim.x + blockIdx.x, t);
    }
}

// The last bind and the final values in one launch: workgroup m (one wave) binds the <= 2 elements of member m's P planes to their
// final values, stores them as the bound polynomials and writes them to res[P m + j]; lane P of workgroup 0 does the same for the public
// polynomial, res[P k_final].  do_bind = 0: everything is already down to one element.
template <int P>
__global__ void __launch_bounds__(GFT) k_spartan_group_final(SpartanGroupArgs a, const fe* __restrict__ pub_in, fe* pub_out, int k_final, int do_bind,
                                                          fe r, fe* __restrict__ res) {
    const int m = (int)blockIdx.x, j = (int)threadIdx.x;
    const bool member = m < k_final && j < P, pub = m == 0 && j == P;
    if (!member && !pub) return;
    const fe* in = member ? a.in[P * m + j] : pub_in;
    fe v = fe_load(in);
    if (do_bind) {
        v = Fr::add(v, Fr::mul(Fr::sub(fe_load(in + 1), v), r));
        fe_store(member ? a.out[P * m + j] : pub_out, v);
    }
    fe_store(res + (member ? P * m + j : P * k_final), v);
}

// ------------------------------------------------------------------ C ABI: Spartan groups
struct cozk_spartan_group {
    cozk_ctx* driver;
    int kind, P, E, k;
    std::vector<cozk_poly*> planes;  // k x P, referred to
    GroupPub pub;                    // pub.len = the current length of every member plane
};

// the one current length of the planes of members 0 .. k - 1, which is the public polynomial's
static void spartan_group_check_len(const cozk_spartan_group* g, int k, const char* what) {
    for (int i = 0; i < k * g->P; i++)
        COZK_REQUIRE(g->planes[i]->len == g->pub.len, std::string(what) + ": every member plane must have the group's current length");
}

// the pointer tables of one launch over members 0 .. k - 1; bind: every plane moves on to its other ping-pong side, as cozk_poly_bind
// (LowToHigh) leaves it -- sized at create, so nothing is allocated here
static SpartanGroupArgs spartan_group_args(cozk_spartan_group* g, int k, bool bind) {
    SpartanGroupArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < k * g->P; i++) {
        cozk_poly* p = g->planes[i];
        a.in[i] = poly_a(p);
        if (bind) {
            const int dst = p->cur < 0 ? 0 : 1 - p->cur;
            pingpong_ensure(p, dst, p->len / 2);
            a.out[i] = p->buf[dst][0];
            p->cur = dst;
            p->len /= 2;
        }
    }
    return a;
}

extern "C" {

int cozk_spartan_group_create(cozk_ctx* driver, int kind, cozk_poly* const* planes, int k, const cozk_poly* pub, cozk_spartan_group** out) {
    if (out) *out = nullptr;
    return cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && planes && pub && out, "spartan_group_create: null argument");
        COZK_REQUIRE(kind == COZK_SPARTAN_GROUP_FIRST || kind == COZK_SPARTAN_GROUP_SECOND, "spartan_group_create: unknown kind");
        COZK_REQUIRE(k >= 1 && k <= COZK_LAYER_GROUP_MAX, "spartan_group_create: 1 <= k <= COZK_LAYER_GROUP_MAX");
        const int P = kind == COZK_SPARTAN_GROUP_FIRST ? 3 : 1;
        COZK_REQUIRE(pub->ctx && pub->mode == COZK_MODE_PLAIN, "spartan_group_create: the public polynomial must be PLAIN");
        COZK_REQUIRE(pub->ctx->device == driver->device, "spartan_group_create: the public polynomial must live on the driver's device");
        const size_t len = pub->len;
        COZK_REQUIRE(len >= 2 && (len & (len - 1)) == 0, "spartan_group_create: the length must be a power of two >= 2");
        std::vector<cozk_ctx*> owners{pub->ctx};
        for (int i = 0; i < k * P; i++) {
            const cozk_poly* p = planes[i];
            group_member_check<true>("spartan_group_create", MemberNouns{"member plane", "member", "plane"}, driver, planes, i);
            COZK_REQUIRE(p->len == len, "spartan_group_create: the member planes and the public polynomial must have one length");
            COZK_REQUIRE(p != pub, "spartan_group_create: a member plane is the public polynomial");
            owners.push_back(p->ctx);
        }
        drain_streams(owners);
        // both ping-pong sides of every plane for all rounds to come, once: the first bind writes len / 2, the second len / 4
        for (int i = 0; i < k * P; i++) {
            cozk_poly* p = planes[i];
            const int first = p->cur < 0 ? 0 : 1 - p->cur;
            pingpong_ensure(p, first, len / 2);
            if (p->cur < 0) pingpong_ensure(p, 1 - first, len / 4);
        }
        cozk_spartan_group* g = new cozk_spartan_group();
        g->driver = driver;
        g->kind = kind;
        g->P = P;
        g->E = P == 3 ? 4 : 3;
        g->k = k;
        g->planes.assign(planes, planes + (size_t)k * P);
        try {
            g->pub.create(driver, pub);
        } catch (...) {
            cozk_spartan_group_free(g);
            throw;
        }
        *out = g;
    });
}

int cozk_spartan_group_free(cozk_spartan_group* g) {
    if (!g) return COZK_OK;
    g->pub.free(g->driver);
    delete g;
    return COZK_OK;
}

int cozk_spartan_group_round(cozk_spartan_group* g, const uint64_t* r, uint64_t* out_evals) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out_evals, "spartan_group_round: null argument");
        spartan_group_check_len(g, g->k, "spartan_group_round");
        COZK_REQUIRE(g->pub.len >= 2, "spartan_group_round: the members are fully bound");
        if (r) COZK_REQUIRE(g->pub.len >= 4, "spartan_group_round: a binding round on members that the bind leaves fully bound");
        const size_t len_in = g->pub.len, pairs = r ? len_in / 4 : len_in / 2;
        const unsigned k = (unsigned)g->k, rows = k * (unsigned)g->E;
        const fe rr = r ? fe_from_u64x4(r) : Fr::zero();
        const fe* pin = g->pub.in();
        fe* pout = g->pub.out();
        const GroupSums gs = group_sums(ctx, rows, pairs, len_in <= ROUND_SMALL_MAX, std::max(64u, GROUP_GRID_MAX / k));
        fe* const partial = gs.partial;
        const SpartanGroupArgs a = spartan_group_args(g, g->k, r != nullptr);
        if (r) g->pub.advance(len_in / 2);
        const dim3 grid(gs.gx, k);
        if (g->P == 3) {
            if (r) k_spartan_group_round<3, 1><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, pairs, rr, partial);
            else k_spartan_group_round<3, 0><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, pairs, rr, partial);
        } else {
            if (r) k_spartan_group_round<1, 1><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, pairs, rr, partial);
            else k_spartan_group_round<1, 0><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, pairs, rr, partial);
        }
        HIP_TRY(hipGetLastError());
        fe s[4 * COZK_LAYER_GROUP_MAX];
        gs.fetch(s);
        for (unsigned i = 0; i < rows; i++) fe_to_u64x4(s[i], out_evals + 4 * i);
    });
}

int cozk_spartan_group_final(cozk_spartan_group* g, const uint64_t* r, int k_final, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out, "spartan_group_final: null argument");
        COZK_REQUIRE(k_final >= 0 && k_final <= g->k, "spartan_group_final: 0 <= k_final <= k");
        spartan_group_check_len(g, k_final, "spartan_group_final");
        COZK_REQUIRE(r ? g->pub.len == 2 : g->pub.len == 1, "spartan_group_final: the bind must leave one element (len == 2 with r, len == 1 without)");
        const fe rr = r ? fe_from_u64x4(r) : Fr::zero();
        const fe* pin = g->pub.in();
        fe* pout = g->pub.out();
        const size_t n_res = (size_t)k_final * g->P + 1;
        fe* res = result_slot(ctx, n_res);
        const SpartanGroupArgs a = spartan_group_args(g, k_final, r != nullptr);
        if (r) g->pub.advance(1);
        const unsigned gx = (unsigned)(k_final ? k_final : 1);
        if (g->P == 3) k_spartan_group_final<3><<<gx, GFT, 0, ctx->stream>>>(a, pin, pout, k_final, r != nullptr, rr, res);
        else k_spartan_group_final<1><<<gx, GFT, 0, ctx->stream>>>(a, pin, pout, k_final, r != nullptr, rr, res);
        HIP_TRY(hipGetLastError());
        fetch_u64x4(ctx, res, n_res, out);
    });
}

size_t cozk_spartan_group_len(const cozk_spartan_group* g) { return g ? g->pub.len : 0; }

int cozk_spartan_group_pub_download(cozk_spartan_group* g, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out, "spartan_group_pub_download: null argument");
        g->pub.download(ctx, out);
    });
}

}  // extern "C"
