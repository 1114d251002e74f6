// Outer groups (cozk_outer_group_*) and shift groups (cozk_shift_group_*): the two sumchecks of co-jolt's Spartan worker
// (Rep3UniformSpartanProver::prove, restated in csrc/host/spartan_jolt.hpp) whose rounds the Spartan groups cannot carry, for k members
// with ONE challenge -- the senders of a Shamir prover, each a party with a context of its own on one device.  Part of poly.hip's
// translation unit, behind spartan_outer.inc (cozk_outer, outer_bind_state).
//
//   OUTER  member = a PLAIN cozk_outer (Az, Bz, Cz over compact active-row storage), public = the Gruen split-eq tables, which every
//          member built from the same tau: the group reads member 0's.  Per member and round
//              t(0) = sum_k e_k (Az_0 Bz_0 - Cz_0),   t(inf) = sum_k e_k (Az_1 - Az_0) (Bz_1 - Bz_0)
//          over the row pairs k of the round; the cubic is formed on the host per member exactly as cozk_outer_round forms it.  Field
//          arithmetic is exact and every stored value canonical, so e (a b - c) summed in one accumulator is byte for byte the
//          s0 - s1 of k_outer_round_act.
//   SHIFT  member = ONE PLAIN polynomial z_m, public = ONE polynomial (eq_plus_one), HighToLow pairs (i, i + len / 2):
//              g_m(X) = sum_i pub(X; i) z_m(X; i)  at X = 0, 2  --  cozk_prod_sumcheck_evals({z_m, pub}, degree 2)
//
// One launch per round whatever k is: blockIdx.y is the member, blockIdx.x strides over the row pairs.  With a challenge the bind is
// FUSED with the sums in ALL storage regimes of the outer sumcheck: a lane reads the (up to) four rows that become one pair of the next
// round, binds them, stores the pair into the other ping-pong side and adds its terms with the tables of the round AFTER the bind.

// Where the rows of one launch lie.  A "unit" is a run of rows that is stored contiguously and whose row pairs do not reach into the
// next unit; pair pr of unit u has the eq index u * k_stride + pr.  Its two rows rho = 2 pr + j (j = 0, 1) are
//     BIND = 0:  read at  u * in_unit + rho                     (present while rho < act_out)
//     BIND = 1:  bound from the rows  u * in_unit + rho * rho_stride (+ 1: present while 2 rho + 1 < act_in), written to
//                u * act_out + rho                              (present, and written, while rho < act_out)
// Rows that are not present are zero and not stored (cozk_outer::act_rows).  The three regimes of outer_group_shape() fill this in.
struct OuterGroupShape {
    uint32_t units, pairs_unit, k_stride;
    uint32_t in_unit, rho_stride, act_in, act_out;
};

struct OuterGroupArgs {
    const fe* in[3 * COZK_LAYER_GROUP_MAX];  // plane q (Az, Bz, Cz) of member m at [3 m + q]: scalar loads indexed by the wave-uniform blockIdx.y
    fe* out[3 * COZK_LAYER_GROUP_MAX];       // the bound planes (BIND only)
};

// partial[(2 m + e) * gridDim.x + blockIdx.x]: e = 0 the t(0) sum (zero without BIND: the first round does not compute it), e = 1 t(inf)
template <int BIND>
__global__ void __launch_bounds__(PT) k_outer_group_round(OuterGroupArgs a, OuterGroupShape sh, const fe* __restrict__ E_in, int in_bits,
                                                       const fe* __restrict__ E_out, fe r, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const unsigned m = blockIdx.y;
    const size_t in_mask = ((size_t)1 << in_bits) - 1;
    const size_t total = (size_t)sh.units * sh.pairs_unit;
    fe s0 = Fr::zero(), s2 = Fr::zero();
    for (size_t q = (size_t)blockIdx.x * PT + threadIdx.x; q < total; q += (size_t)gridDim.x * PT) {
        const uint32_t u = (uint32_t)(q / sh.pairs_unit), pr = (uint32_t)(q - (size_t)u * sh.pairs_unit);
        const size_t k = (size_t)u * sh.k_stride + pr;
        const fe e = Fr::mul(fe_load(E_out + (k >> in_bits)), fe_load(E_in + (k & in_mask)));
        fe v[3][2];  // [Az | Bz | Cz][row 2 pr | row 2 pr + 1] of this round
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t rho = 2 * pr + j;
            const bool present = rho < sh.act_out;
#pragma unroll
            for (int p = 0; p < 3; p++) {
                fe x = Fr::zero();
                if (BIND) {
                    if (present) {
                        const fe* in = a.in[3 * m + p] + (size_t)u * sh.in_unit + (size_t)rho * sh.rho_stride;
                        const fe lo = fe_load(in);
                        const fe hi = 2 * rho + 1 < sh.act_in ? fe_load(in + 1) : Fr::zero();
                        x = Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r));
                        fe_store(a.out[3 * m + p] + (size_t)u * sh.act_out + rho, x);
                    }
                } else if (present && p < 2) {  // the first round does not compute t(0): Cz is not read
                    x = fe_load(a.in[3 * m + p] + (size_t)u * sh.in_unit + rho);
                }
                v[p][j] = x;
            }
        }
        s2 = Fr::add(s2, Fr::mul(Fr::mul(Fr::sub(v[0][1], v[0][0]), Fr::sub(v[1][1], v[1][0])), e));
        if (BIND) s0 = Fr::add(s0, Fr::mul(Fr::sub(Fr::mul(v[0][0], v[1][0]), v[2][0]), e));
    }
    s0 = fr_block_sum(s0, sh4);
    if (threadIdx.x == 0) fe_store(partial + ((size_t)m * 2) * gridDim.x + blockIdx.x, s0);
    s2 = fr_block_sum(s2, sh4);
    if (threadIdx.x == 0) fe_store(partial + ((size_t)m * 2 + 1) * gridDim.x + blockIdx.x, s2);
}

// The last bind and Az, Bz, Cz(r) in one launch: lane q < 3 of workgroup m (one wave) binds the one row pair that is left of plane q of
// member m (`stored` = 1: its upper row is a zero that is not stored), stores the value as the bound plane and writes it to res[3 m + q].
__global__ void __launch_bounds__(GFT) k_outer_group_final(OuterGroupArgs a, int stored, fe r, fe* __restrict__ res) {
    const int m = (int)blockIdx.x, q = (int)threadIdx.x;
    if (q >= 3) return;
    const fe* in = a.in[3 * m + q];
    const fe lo = fe_load(in);
    const fe hi = stored > 1 ? fe_load(in + 1) : Fr::zero();
    const fe v = Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r));
    fe_store(a.out[3 * m + q], v);
    fe_store(res + 3 * m + q, v);
}

// ------------------------------------------------------------------ C ABI: outer groups
struct cozk_outer_group {
    cozk_ctx* driver;
    int k;
    std::vector<cozk_outer*> members;  // referred to
};

// Every member PLAIN, on the driver's device, distinct, and in member 0's state.  Host only: nothing is launched and nothing changed.
static void outer_group_check(cozk_ctx* driver, cozk_outer* const* members, int k, const std::string& what) {
    const cozk_outer* m0 = members[0];
    for (int i = 0; i < k; i++) {
        group_member_check<true>(what, MEMBER, driver, members, i);
        const cozk_outer* m = members[i];
        if (i == 0) m0 = m;
        COZK_REQUIRE(m->L == m0->L && m->per_step == m0->per_step && m->act_rows == m0->act_rows && m->round == m0->round &&
                         m->current_index == m0->current_index && m->n_in == m0->n_in && m->n_out == m0->n_out,
                     what + ": every member must be in the same state (L, per_step, act_rows, round)");
        COZK_REQUIRE(m->w.size() == m0->w.size() && memcmp(m->w.data(), m0->w.data(), m0->w.size() * sizeof(fe)) == 0,
                     what + ": every member must have been made with the same tau");
    }
}

// the three storage regimes of a round over members in the state of `st` (before the bind, if there is one)
static OuterGroupShape outer_group_shape(const cozk_outer* st, bool bind) {
    const size_t P = st->per_step, A = st->act_rows, steps = st->L / P;
    OuterGroupShape s{};
    if (!bind) {
        if (P > 1) s = OuterGroupShape{(uint32_t)steps, (uint32_t)((A + 1) / 2), (uint32_t)(P / 2), (uint32_t)A, 1, 0, (uint32_t)A};
        else s = OuterGroupShape{(uint32_t)(st->L / 2), 1, 1, 2, 1, 0, 2};  // dense: every pair a unit of its own
    } else if (P >= 4) {
        // compact storage on both sides; the pair lies inside a step
        const size_t A2 = (A + 1) / 2;
        s = OuterGroupShape{(uint32_t)steps, (uint32_t)((A2 + 1) / 2), (uint32_t)(P / 4), (uint32_t)A, 2, (uint32_t)A, (uint32_t)A2};
    } else if (P == 2 && A == 1) {
        // the output rows are whole steps of ONE stored row each: two steps make a pair, nothing to read above a row
        s = OuterGroupShape{(uint32_t)(steps / 2), 1, 1, 2, 1, 0, 2};
    } else {
        // P == 2 (the output rows are whole steps, a pair straddles two of them) or dense storage: four consecutive rows make a pair
        s = OuterGroupShape{(uint32_t)(st->L / 4), 1, 1, 4, 2, 4, 2};
    }
    return s;
}

static OuterGroupArgs outer_group_args(const cozk_outer_group* g, int k) {
    OuterGroupArgs a;
    memset(&a, 0, sizeof a);
    for (int m = 0; m < k; m++) {
        const cozk_outer* st = g->members[(size_t)m];
        for (int q = 0; q < 3; q++) {
            a.in[3 * m + q] = st->buf[st->cur][q][0];
            a.out[3 * m + q] = st->buf[1 - st->cur][q][0];
        }
    }
    return a;
}

extern "C" {

int cozk_outer_group_free(cozk_outer_group* g) {
    delete g;
    return COZK_OK;
}

int cozk_outer_group_create(cozk_ctx* driver, cozk_outer* const* members, int k, cozk_outer_group** out) {
    if (out) *out = nullptr;
    return cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && members && out, "outer_group_create: null argument");
        COZK_REQUIRE(k >= 1 && k <= COZK_LAYER_GROUP_MAX, "outer_group_create: 1 <= k <= COZK_LAYER_GROUP_MAX");
        outer_group_check(driver, members, k, "outer_group_create");
        std::vector<cozk_ctx*> owners;
        for (int i = 0; i < k; i++) owners.push_back(members[i]->ctx);
        drain_streams(owners);
        cozk_outer_group* g = new cozk_outer_group();
        g->driver = driver;
        g->k = k;
        g->members.assign(members, members + k);
        *out = g;
    });
}

size_t cozk_outer_group_len(const cozk_outer_group* g) { return g ? g->members[0]->L : 0; }

int cozk_outer_group_round(cozk_outer_group* g, const uint64_t* r, const uint64_t* claims, uint64_t* out_coeffs) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(claims && out_coeffs, "outer_group_round: null argument");
        outer_group_check(ctx, g->members.data(), g->k, "outer_group_round");
        cozk_outer* const m0 = g->members[0];
        COZK_REQUIRE(m0->round > 0 || !r, "outer_group_round: the first round takes no challenge (r must be NULL)");
        COZK_REQUIRE(m0->round == 0 || r, "outer_group_round: every round after the first binds with the previous challenge (r is NULL)");
        COZK_REQUIRE(m0->L >= (r ? 4u : 2u) && m0->current_index >= (r ? 2 : 1), "outer_group_round: the members are fully bound");
        // the last check, still before the bind below (outer_group_check holds every member to m0's counts): a refused call leaves the members as they were
        COZK_REQUIRE(outer_eq_in_step(m0, r != nullptr), "outer_group_round: split-eq tables out of step with the members");
        const fe rr = r ? fe_from_u64x4(r) : Fr::zero();
        const OuterGroupShape shape = outer_group_shape(m0, r != nullptr);
        const OuterGroupArgs a = outer_group_args(g, g->k);
        const size_t total = (size_t)shape.units * shape.pairs_unit;
        const unsigned k = (unsigned)g->k, rows = 2 * k;
        // small: members of <= ROUND_SMALL_MAX (dense-equivalent) rows
        const GroupSums gs = group_sums(ctx, rows, total, m0->L <= ROUND_SMALL_MAX, std::max(64u, GROUP_GRID_MAX / k));
        fe* const partial = gs.partial;
        // the members move on to the state of this round: the tables and the linear factor below are those AFTER the bind
        if (r)
            for (cozk_outer* st : g->members) outer_bind_state(st, rr);
        const fe* E_in = m0->E_in + (((size_t)1 << m0->n_in) - 1);
        const fe* E_out = m0->E_out + (((size_t)1 << m0->n_out) - 1);
        const dim3 grid(gs.gx, k);
        if (r) k_outer_group_round<1><<<grid, PT, 0, ctx->stream>>>(a, shape, E_in, (int)m0->n_in, E_out, rr, partial);
        else k_outer_group_round<0><<<grid, PT, 0, ctx->stream>>>(a, shape, E_in, (int)m0->n_in, E_out, rr, partial);
        HIP_TRY(hipGetLastError());
        fe s[2 * COZK_LAYER_GROUP_MAX];
        gs.fetch(s);
        // UniPoly::from_linear_times_quadratic_with_hint([scalar - scalar w, 2 scalar w - scalar], t0, tinf, claim_m), as cozk_outer_round
        const fe sw = Fr::mul(m0->current_scalar, m0->w[m0->current_index - 1]);
        const fe l0 = Fr::sub(m0->current_scalar, sw), l1 = Fr::sub(Fr::dbl(sw), m0->current_scalar);
        const fe linv = Fr::inv(Fr::add(l0, l1));
        for (unsigned m = 0; m < k; m++) {
            const fe t0 = s[2 * m], tinf = s[2 * m + 1];
            const fe hint = fe_from_u64x4(claims + 4 * m);
            const fe c0 = Fr::mul(l0, t0);
            const fe t1 = Fr::sub(Fr::sub(Fr::mul(Fr::sub(hint, c0), linv), t0), tinf);
            const fe cf[4] = {c0, Fr::add(Fr::mul(l0, t1), Fr::mul(l1, t0)), Fr::add(Fr::mul(l0, tinf), Fr::mul(l1, t1)), Fr::mul(l1, tinf)};
            for (int i = 0; i < 4; i++) fe_to_u64x4(cf[i], out_coeffs + 16 * m + 4 * i);
            g->members[m]->round++;
        }
    });
}

int cozk_outer_group_final(cozk_outer_group* g, const uint64_t r[4], int k_final, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(r && out, "outer_group_final: null argument");
        COZK_REQUIRE(k_final >= 0 && k_final <= g->k, "outer_group_final: 0 <= k_final <= k");
        outer_group_check(ctx, g->members.data(), g->k, "outer_group_final");
        cozk_outer* const m0 = g->members[0];
        COZK_REQUIRE(m0->L == 2, "outer_group_final: one unbound variable must be left (L == 2)");
        if (k_final == 0) return;
        const fe rr = fe_from_u64x4(r);
        const int stored = m0->per_step > 1 ? (int)m0->act_rows : 2;
        const OuterGroupArgs a = outer_group_args(g, k_final);
        for (int m = 0; m < k_final; m++) outer_bind_state(g->members[(size_t)m], rr);
        const size_t n_res = 3 * (size_t)k_final;
        fe* res = result_slot(ctx, n_res);
        k_outer_group_final<<<(unsigned)k_final, GFT, 0, ctx->stream>>>(a, stored, rr, res);
        HIP_TRY(hipGetLastError());
        fetch_u64x4(ctx, res, n_res, out);
    });
}

}  // extern "C"

// ------------------------------------------------------------------ shift groups
struct ShiftGroupArgs {
    const fe* in[COZK_LAYER_GROUP_MAX];
    fe* out[COZK_LAYER_GROUP_MAX];  // BIND: the bound member; == in[m] once the member is bound in place, as cozk_poly_bind(HIGH_TO_LOW) does
};

// partial[(2 m + e) * gridDim.x + blockIdx.x], e = 0: X = 0, e = 1: X = 2.  `half` = pairs of this round (after the bind).  With BIND lane
// i reads i, i + half, i + 2 half, i + 3 half of the member and of the public polynomial and writes i and i + half: no lane reads what
// another one writes, so a member may be bound in place.  Every member row binds the public polynomial for itself; only row 0 stores it,
// into the OTHER ping-pong buffer of the group.
template <int BIND>
__global__ void __launch_bounds__(PT) k_shift_group_round(ShiftGroupArgs a, const fe* __restrict__ pub_in, fe* __restrict__ pub_out, size_t half, fe r,
                                                       fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const unsigned m = blockIdx.y;
    const fe* zin = a.in[m];
    fe* zout = a.out[m];
    fe e0 = Fr::zero(), e2 = Fr::zero();
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < half; i += (size_t)gridDim.x * PT) {
        fe lo[2], hi[2];  // [member | public]
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const fe* in = j == 0 ? zin : pub_in;
            if (BIND) {
                const fe x0 = fe_load(in + i), x1 = fe_load(in + i + half), x2 = fe_load(in + i + 2 * half), x3 = fe_load(in + i + 3 * half);
                lo[j] = Fr::add(x0, Fr::mul(Fr::sub(x2, x0), r));
                hi[j] = Fr::add(x1, Fr::mul(Fr::sub(x3, x1), r));
                if (j == 0 || m == 0) {
                    fe* out = j == 0 ? zout : pub_out;
                    fe_store(out + i, lo[j]);
                    fe_store(out + i + half, hi[j]);
                }
            } else {
                lo[j] = fe_load(in + i);
                hi[j] = fe_load(in + i + half);
            }
        }
        e0 = Fr::add(e0, Fr::mul(lo[0], lo[1]));
        const fe dz = Fr::sub(hi[0], lo[0]), dp = Fr::sub(hi[1], lo[1]);
        e2 = Fr::add(e2, Fr::mul(Fr::add(Fr::add(lo[0], dz), dz), Fr::add(Fr::add(lo[1], dp), dp)));
    }
    e0 = fr_block_sum(e0, sh4);
    if (threadIdx.x == 0) fe_store(partial + ((size_t)m * 2) * gridDim.x + blockIdx.x, e0);
    e2 = fr_block_sum(e2, sh4);
    if (threadIdx.x == 0) fe_store(partial + ((size_t)m * 2 + 1) * gridDim.x + blockIdx.x, e2);
}

// The last bind and the final values in one launch: lane m < k_final binds the two elements of member m, lane k_final those of the
// public polynomial; res[m], res[k_final].  do_bind = 0: everything is down to one element already.
__global__ void __launch_bounds__(GFT) k_shift_group_final(ShiftGroupArgs a, const fe* __restrict__ pub_in, fe* __restrict__ pub_out, int k_final,
                                                        int do_bind, fe r, fe* __restrict__ res) {
    const int m = (int)threadIdx.x;
    if (m > k_final) return;
    const fe* in = m < k_final ? a.in[m] : pub_in;
    fe v = fe_load(in);
    if (do_bind) {
        v = Fr::add(v, Fr::mul(Fr::sub(fe_load(in + 1), v), r));
        fe_store(m < k_final ? a.out[m] : pub_out, v);
    }
    fe_store(res + m, v);
}

struct cozk_shift_group {
    cozk_ctx* driver;
    int k;
    std::vector<cozk_poly*> members;  // referred to
    GroupPub pub;                     // pub.len = the current length of every member
};

static void shift_group_check_len(const cozk_shift_group* g, int k, const char* what) {
    for (int i = 0; i < k; i++) COZK_REQUIRE(g->members[(size_t)i]->len == g->pub.len, std::string(what) + ": every member must have the group's current length");
}

// the pointer tables of one launch over members 0 .. k - 1; bind: every member moves on as cozk_poly_bind(HIGH_TO_LOW) moves it -- to
// side 0 from its unbound coefficients (sized at create), in place afterwards
static ShiftGroupArgs shift_group_args(cozk_shift_group* g, int k, bool bind) {
    ShiftGroupArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < k; i++) {
        cozk_poly* p = g->members[(size_t)i];
        a.in[i] = poly_a(p);
        if (bind) {
            const int dst = p->cur < 0 ? 0 : p->cur;
            if (p->cur < 0) pingpong_ensure(p, dst, p->len / 2);
            a.out[i] = p->buf[dst][0];
            p->cur = dst;
            p->len /= 2;
        }
    }
    return a;
}

extern "C" {

int cozk_shift_group_free(cozk_shift_group* g) {
    if (!g) return COZK_OK;
    g->pub.free(g->driver);
    delete g;
    return COZK_OK;
}

int cozk_shift_group_create(cozk_ctx* driver, cozk_poly* const* members, int k, const cozk_poly* pub, cozk_shift_group** out) {
    if (out) *out = nullptr;
    return cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && members && pub && out, "shift_group_create: null argument");
        COZK_REQUIRE(k >= 1 && k <= COZK_LAYER_GROUP_MAX, "shift_group_create: 1 <= k <= COZK_LAYER_GROUP_MAX");
        COZK_REQUIRE(pub->ctx && pub->mode == COZK_MODE_PLAIN, "shift_group_create: the public polynomial must be PLAIN");
        COZK_REQUIRE(pub->ctx->device == driver->device, "shift_group_create: the public polynomial must live on the driver's device");
        const size_t len = pub->len;
        COZK_REQUIRE(len >= 2 && (len & (len - 1)) == 0, "shift_group_create: the length must be a power of two >= 2");
        std::vector<cozk_ctx*> owners{pub->ctx};
        for (int i = 0; i < k; i++) {
            const cozk_poly* p = members[i];
            group_member_check<true>("shift_group_create", MEMBER, driver, members, i);
            COZK_REQUIRE(p->len == len, "shift_group_create: the members and the public polynomial must have one length");
            COZK_REQUIRE(p != pub, "shift_group_create: a member is the public polynomial");
            owners.push_back(p->ctx);
        }
        drain_streams(owners);
        // an unbound member is bound into side 0, a bound one in place: nothing else is ever written
        for (int i = 0; i < k; i++)
            if (members[i]->cur < 0) pingpong_ensure(members[i], 0, len / 2);
        cozk_shift_group* g = new cozk_shift_group();
        g->driver = driver;
        g->k = k;
        g->members.assign(members, members + k);
        try {
            g->pub.create(driver, pub);
        } catch (...) {
            cozk_shift_group_free(g);
            throw;
        }
        *out = g;
    });
}

int cozk_shift_group_round(cozk_shift_group* g, const uint64_t* r, uint64_t* out_evals) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out_evals, "shift_group_round: null argument");
        shift_group_check_len(g, g->k, "shift_group_round");
        COZK_REQUIRE(g->pub.len >= 2, "shift_group_round: the members are fully bound");
        if (r) COZK_REQUIRE(g->pub.len >= 4, "shift_group_round: a binding round on members that the bind leaves fully bound");
        const size_t len_in = g->pub.len, half = r ? len_in / 4 : len_in / 2;
        const unsigned k = (unsigned)g->k, rows = 2 * k;
        const fe rr = r ? fe_from_u64x4(r) : Fr::zero();
        const fe* pin = g->pub.in();
        fe* pout = g->pub.out();
        const GroupSums gs = group_sums(ctx, rows, half, len_in <= ROUND_SMALL_MAX, std::max(64u, GROUP_GRID_MAX / k));
        fe* const partial = gs.partial;
        const ShiftGroupArgs a = shift_group_args(g, g->k, r != nullptr);
        if (r) g->pub.advance(len_in / 2);
        const dim3 grid(gs.gx, k);
        if (r) k_shift_group_round<1><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, half, rr, partial);
        else k_shift_group_round<0><<<grid, PT, 0, ctx->stream>>>(a, pin, pout, half, rr, partial);
        HIP_TRY(hipGetLastError());
        fe s[2 * COZK_LAYER_GROUP_MAX];
        gs.fetch(s);
        for (unsigned i = 0; i < rows; i++) fe_to_u64x4(s[i], out_evals + 4 * i);
    });
}

int cozk_shift_group_final(cozk_shift_group* g, const uint64_t* r, int k_final, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out, "shift_group_final: null argument");
        COZK_REQUIRE(k_final >= 0 && k_final <= g->k, "shift_group_final: 0 <= k_final <= k");
        shift_group_check_len(g, k_final, "shift_group_final");
        COZK_REQUIRE(r ? g->pub.len == 2 : g->pub.len == 1, "shift_group_final: the bind must leave one element (len == 2 with r, len == 1 without)");
        const fe rr = r ? fe_from_u64x4(r) : Fr::zero();
        const fe* pin = g->pub.in();
        fe* pout = g->pub.out();
        const size_t n_res = (size_t)k_final + 1;
        fe* res = result_slot(ctx, n_res);
        const ShiftGroupArgs a = shift_group_args(g, k_final, r != nullptr);
        if (r) g->pub.advance(1);
        k_shift_group_final<<<1, GFT, 0, ctx->stream>>>(a, pin, pout, k_final, r != nullptr, rr, res);
        HIP_TRY(hipGetLastError());
        fetch_u64x4(ctx, res, n_res, out);
    });
}

size_t cozk_shift_group_len(const cozk_shift_group* g) { return g ? g->pub.len : 0; }

int cozk_shift_group_pub_download(cozk_shift_group* g, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out, "shift_group_pub_download: null argument");
        g->pub.download(ctx, out);
    });
}

}  // extern "C"
