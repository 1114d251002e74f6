// Level groups of Lasso's primary sumcheck (cozk_primary_group_*): one multiplication level, and the last local step of a round, for
// the k = 2t + 1 senders of a Shamir prover at once.  Part of poly.hip's translation unit, behind primary_sumcheck.inc (cozk_primary,
// PrimCtx, prim_products, prim_lc, prim_slot_pos).
//
// primary_sumcheck.inc compiles every multiplicative collation into slots that are sums of products of TWO affine forms.  A party that
// holds degree-t Shamir shares of the memories (and of the earlier slots) therefore computes, with the PLAIN program, a point of a
// degree-2t polynomial whose constant term is the slot value.  Where Rep3 puts the ring reshare, Shamir puts the degree reduction
// (GRR; shamir.rs `degree_reduce`): sender m re-deals its local value z with a fresh degree-t polynomial,
//     h[m -> q][pos] = z + sum_{c = 1..t} PRF(keys_m[c - 1], counter + pos) (q + 1)^c           q = 0 .. 2t,
// and receiver q combines what it was dealt with lagrange(1 .. 2t + 1):
//     P_q[level - 1][pos] = sum_{m <= 2t} lambda_m h[m -> q][pos].
// Public constants enter every member's single component (COZK_MODE_PLAIN): the constant sharing.
//
//   k_primary_group_deal     grid (item blocks, D evaluation points, k members): member m's unmasked slot values of the level -- exactly
//                            k_primary_level<1>'s z -- are never stored; they are dealt with the rule of cozk_shamir_mul_deal
//                            (shamir_deal.hip.hpp: the one copy of the dealing and PRF code) into the staging block [m][q][level_elems].
//                            A workgroup reads ONE member's secrets.
//   k_primary_group_combine  grid (element blocks, k receivers): the receiver's step, written into member q's own level buffer.
//   k_primary_group_final    k_primary_final<1> with the member on a grid axis; one k_finish_sums over all members' rows.
// Two launches per level and two per finish whatever k is.  Receivers are the 2t + 1 senders only: a party above 2t holds no program
// state and would have no use for a slot value.
//
// The KING form of the level (cozk_primary_group_level_king) reduces the degree on a preprocessed double-random pair ([r]_t, [r]_2t)
// instead (Damgard-Nielsen; shamir.hip): sender m sends z + r_2t,m to the king, who opens zed = sum_m lambda_m (z_m + r_2t,m) = slot + r
// and sends it to everyone; receiver q keeps zed - r_t,q.  No PRF runs online and the staging block is [k][level_elems].
//   k_primary_group_mask     the deal kernel's grid and slot values; staging[m][pos] = z + r_2t[m][r_offset + pos].
//   the finish               k_shamir_king_finish (shamir.hip: the one copy of the open-and-unmask step) over the table of the
//                            members' level buffers, grid (element blocks): 2k x 32 B read, k x 32 B written per element.

static constexpr int PRIM_GROUP_MAX = COZK_PRIMARY_GROUP_MAX;  // 2t + 1 with 2t <= COZK_SHAMIR_MAX_DEGREE
static constexpr int PRIM_GROUP_MAX_T = (PRIM_GROUP_MAX - 1) / 2;

struct PrimGroupMember {
    const fe* st;  // the member's current polynomial set
    const PrimInstrDev* instrs;
    const int* mul;
    const uint32_t *item_idx, *item_slot, *bases;
    fe* P[PRIM_MAX_LEVELS];
};
struct PrimGroupArgs {
    PrimGroupMember m[PRIM_GROUP_MAX];  // indexed by the wave-uniform member number: scalar loads
};

// one (item, evaluation point) of member `mb`: the setup of k_primary_level / k_primary_final
static __device__ __forceinline__ PrimCtx<1> prim_group_ctx(const PrimGroupMember& mb, size_t cap, int n_instr, int n_mem, int D, size_t j, int k) {
    PrimCtx<1> c;
    c.st = mb.st;
    c.cap = cap;
    c.n_instr = n_instr;
    c.n_mem = n_mem;
    c.party = 0;
    c.D = D;
    c.s = (int)mb.item_slot[j];
    c.in = mb.instrs + mb.mul[c.s];
    c.i = mb.item_idx[j];
    c.jrel = (uint32_t)j - mb.bases[PRIM_MAX_LEVELS * PRIM_MAX_MUL + c.s];
    c.bases = mb.bases;
    for (int t = 0; t < PRIM_MAX_LEVELS; t++) {
        c.P.a[t] = mb.P[t];
        c.P.b[t] = nullptr;
    }
    c.k = k;
    c.X = k == 0 ? 0 : k + 1;
    return c;
}

// DEG = t at compile time (1..3), 0: t <= PRIM_GROUP_MAX_T at run time (the shift register of shamir_deal_coefs)
template <int DEG>
__global__ void __launch_bounds__(PT) k_primary_group_deal(PrimGroupArgs a, size_t cap, int n_instr, int n_mem, int D, size_t n_items, int level,
                                                        const prf_key* __restrict__ keys, int t, uint64_t ctr, fe* __restrict__ stage,
                                                        size_t level_elems) {
    const size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_items) return;
    const unsigned m = blockIdx.z, k = gridDim.z;
    const PrimCtx<1> c = prim_group_ctx(a.m[m], cap, n_instr, n_mem, D, j, (int)blockIdx.y);
    if (level > c.in->n_levels || c.in->nq[level - 1] == 0) return;  // this instruction has nothing at this level
    constexpr int MAXD = DEG ? DEG : PRIM_GROUP_MAX_T;
    const int deg = DEG ? DEG : t;
    const prf_key* km = keys + (size_t)m * t;
    fe* out = stage + (size_t)m * k * level_elems;
    for (int q = 0; q < c.in->n_slots; q++) {
        const PrimSlot& sl = c.in->slots[q];
        if (sl.level != level) continue;
        fe z = prim_products<1>(c, sl.prod, sl.n_prod);
        if (sl.has_add) z = Fr::add(z, sh_ab_sum<1>(prim_lc<1>(c, sl.add)));
        const size_t pos = prim_slot_pos<1>(c, level - 1, sl.q);
        fe cf[MAXD];
        shamir_deal_coefs<DEG, MAXD>(cf, deg, [&](int cc) {
            prf_key key;  // a copy in scalar registers of the wave-uniform table entry
#pragma unroll
            for (int w = 0; w < 8; w++) key.k[w] = km[cc].k[w];
            return shamir_prf_fr(key, ctr + pos);
        });
#pragma unroll 1  // one Horner chain at a time, as k_shamir_share
        for (unsigned p = 1; p <= k; p++) fe_store(out + (size_t)(p - 1) * level_elems + pos, shamir_deal_eval<MAXD>(cf, deg, p, z));
    }
}

struct PrimGroupMaskArgs {
    const fe* r2t[PRIM_GROUP_MAX];  // member m's degree-2t half, advanced by the element offset
};
// k_primary_group_deal's walk over the slots of one (item, evaluation point, member); the value is masked, not dealt
__global__ void __launch_bounds__(PT) k_primary_group_mask(PrimGroupArgs a, PrimGroupMaskArgs r, size_t cap, int n_instr, int n_mem, int D, size_t n_items,
                                                        int level, fe* __restrict__ stage, size_t level_elems) {
    const size_t j = (size_t)blockIdx.x * PT + threadIdx.x;
    if (j >= n_items) return;
    const unsigned m = blockIdx.z;
    const PrimCtx<1> c = prim_group_ctx(a.m[m], cap, n_instr, n_mem, D, j, (int)blockIdx.y);
    if (level > c.in->n_levels || c.in->nq[level - 1] == 0) return;  // this instruction has nothing at this level
    const fe* mask = r.r2t[m];
    fe* out = stage + (size_t)m * level_elems;
    for (int q = 0; q < c.in->n_slots; q++) {
        const PrimSlot& sl = c.in->slots[q];
        if (sl.level != level) continue;
        fe z = prim_products<1>(c, sl.prod, sl.n_prod);
        if (sl.has_add) z = Fr::add(z, sh_ab_sum<1>(prim_lc<1>(c, sl.add)));
        const size_t pos = prim_slot_pos<1>(c, level - 1, sl.q);
        fe_store(out + pos, Fr::add(z, fe_load(mask + pos)));
    }
}

struct PrimGroupCombineArgs {
    fe* out[PRIM_GROUP_MAX];  // receiver q's level buffer
    fe lambda[PRIM_GROUP_MAX];
};
__global__ void __launch_bounds__(PT) k_primary_group_combine(PrimGroupCombineArgs a, const fe* __restrict__ stage, size_t level_elems) {
    const size_t pos = (size_t)blockIdx.x * PT + threadIdx.x;
    if (pos >= level_elems) return;
    const unsigned q = blockIdx.y, k = gridDim.y;
    FrWide w;
    fr_wide_zero(w);
    for (unsigned m = 0; m < k; m++) fr_wide_mac(w, fe_load(stage + ((size_t)m * k + q) * level_elems + pos), a.lambda[m]);
    fe_store(a.out[q] + pos, fr_wide_reduce(w));  // canonical
}

// partial[(2 D m + kk) * gridDim.x + blockIdx.x] (the affine part) and [(2 D m + D + kk) * ..] (the products) of member m at point kk
__global__ void __launch_bounds__(PT) k_primary_group_final(PrimGroupArgs a, size_t cap, int n_instr, int n_mem, int D, size_t n_items,
                                                         fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    fe acc_ab = Fr::zero(), acc_ad = Fr::zero();
    const unsigned m = blockIdx.z;
    const int k = blockIdx.y;
    const PrimGroupMember& mb = a.m[m];
    const fe* eqp = mb.st + (size_t)prim_slot_eq(n_instr, n_mem, 1) * cap;
    for (size_t j = (size_t)blockIdx.x * PT + threadIdx.x; j < n_items; j += (size_t)gridDim.x * PT) {
        const PrimCtx<1> c = prim_group_ctx(mb, cap, n_instr, n_mem, D, j, k);
        const fe* fp = mb.st + (size_t)prim_slot_flag(mb.mul[c.s]) * cap;
        fe f0 = fe_load(fp + 2 * c.i), f1 = fe_load(fp + 2 * c.i + 1);
        fe e0 = fe_load(eqp + 2 * c.i), e1 = fe_load(eqp + 2 * c.i + 1);
        fe df = Fr::sub(f1, f0), de = Fr::sub(e1, e0);
        fe fk = f0, ek = e0;
        for (int x = 0; x < c.X; x++) {
            fk = Fr::add(fk, df);
            ek = Fr::add(ek, de);
        }
        fe w = Fr::mul(fk, ek);
        if (c.in->fin_add.n || c.in->fin_add.c0) acc_ab = Fr::add(acc_ab, Fr::mul(sh_ab_sum<1>(prim_lc<1>(c, c.in->fin_add)), w));
        if (c.in->n_final) acc_ad = Fr::add(acc_ad, Fr::mul(prim_products<1>(c, c.in->fin, c.in->n_final), w));
    }
    const size_t row = (size_t)2 * D * m;
    fe v = fr_block_sum(acc_ab, sh4);
    if (threadIdx.x == 0) fe_store(partial + (row + k) * gridDim.x + blockIdx.x, v);
    v = fr_block_sum(acc_ad, sh4);
    if (threadIdx.x == 0) fe_store(partial + (row + D + k) * gridDim.x + blockIdx.x, v);
}

// ------------------------------------------------------------------ C ABI
struct cozk_primary_group {
    cozk_ctx* driver;
    int k, t;
    std::vector<cozk_primary*> members;  // referred to
    bool keyless;                        // made by cozk_primary_group_create_king: king levels only
    prf_key* d_keys;                     // [k][t], from the driver's pool; NULL in a keyless group
    fe* stage;                           // [k][k][stage_cap / k^2 ...]: the dealt values of the level in flight ([k][..]: the masked values of a
                                         // king level), from the driver's pool
    size_t stage_cap;                    // elements
    fe lambda[PRIM_GROUP_MAX];
};

// Every member PLAIN, on the driver's device, distinct, of member 0's table and length; `round`: and with member 0's items and level
// sizes (every call; create cannot know which round_begin calls will follow).  Host only.
static void primary_group_check(cozk_ctx* driver, cozk_primary* const* members, int k, const std::string& what, bool round) {
    const cozk_primary* m0 = members[0];
    for (int i = 0; i < k; i++) {
        group_member_check<true>(what, MEMBER, driver, members, i);
        const cozk_primary* m = members[i];
        if (i == 0) m0 = m;
        COZK_REQUIRE(m->n_instr == m0->n_instr && m->n_mem == m0->n_mem && m->degree == m0->degree && m->mul == m0->mul && m->lin == m0->lin,
                     what + ": every member must have the same instruction table (n_instr, n_mem, degree)");
        for (int q = 0; q < m0->n_instr; q++) {
            const PrimInstrDev &x = m->instrs[(size_t)q], &y = m0->instrs[(size_t)q];
            COZK_REQUIRE(x.form == y.form && x.n_mems == y.n_mems && x.bits == y.bits && memcmp(x.mems, y.mems, sizeof x.mems) == 0,
                         what + ": every member must have the same instruction table (n_instr, n_mem, degree)");
        }
        COZK_REQUIRE(m->n0 == m0->n0 && m->n == m0->n && m->cur == m0->cur, what + ": every member must have the same length");
        if (!round) continue;
        COZK_REQUIRE(m->n_items == m0->n_items, what + ": every member must have the same item count (the same round_begin calls)");
        for (int l = 0; l < PRIM_MAX_LEVELS; l++)
            COZK_REQUIRE(m->level_elems[l] == m0->level_elems[l], what + ": every member must have the same level sizes (the same round_begin calls)");
    }
}

// round_begin and final_evals stay per member and run on the member's OWN stream; round_begin returns with its last launches (the item
// list, the bases) still enqueued there.  So every group call that launches waits, after its host checks and before its first launch,
// for every distinct member stream other than the driver's (drain_streams).  The way back is the calls' own drain of the driver's
// stream.
static void primary_group_wait_members(const cozk_primary_group* g) {
    std::vector<cozk_ctx*> owners;
    for (const cozk_primary* p : g->members) owners.push_back(p->ctx);
    drain_streams(owners, g->driver);
}

static PrimGroupArgs primary_group_args(const cozk_primary_group* g) {
    PrimGroupArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < g->k; i++) {
        const cozk_primary* p = g->members[(size_t)i];
        PrimGroupMember& mb = a.m[i];
        mb.st = p->store[p->cur];
        mb.instrs = p->d_instrs;
        mb.mul = p->d_mul;
        mb.item_idx = p->d_item_idx;
        mb.item_slot = p->d_item_slot;
        mb.bases = p->d_bases;
        for (int l = 0; l < PRIM_MAX_LEVELS; l++) mb.P[l] = p->P[l][0];
    }
    return a;
}

// the king's open and unmask (shamir.hip): z = sum_{j < k} lambda_j m[j], out[q] = z - (rt[q] + off) for q < count
void shamir_launch_king_finish(hipStream_t st, const fe* const* m, int k, const fe* const* rt, size_t off, int count, fe* const* out, size_t n);

// both creates: keys == NULL only in a keyless group
static int primary_group_make(cozk_ctx* driver, cozk_primary* const* members, int k, const uint8_t* keys, bool keyless, const std::string& who,
                              cozk_primary_group** out) {
    if (out) *out = nullptr;
    return cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && members && (keys || keyless) && out, who + ": null argument");
        COZK_REQUIRE(k >= 3 && k <= PRIM_GROUP_MAX && k % 2 == 1, who + ": k = 2t + 1 with 1 <= t, k <= COZK_PRIMARY_GROUP_MAX");
        primary_group_check(driver, members, k, who, false);
        std::vector<cozk_ctx*> owners;
        for (int i = 0; i < k; i++) owners.push_back(members[i]->ctx);
        drain_streams(owners);
        cozk_primary_group* g = new cozk_primary_group();
        g->driver = driver;
        g->k = k;
        g->t = (k - 1) / 2;
        g->members.assign(members, members + k);
        g->keyless = keyless;
        g->d_keys = nullptr;
        g->stage = nullptr;
        g->stage_cap = 0;
        uint32_t pts[PRIM_GROUP_MAX];
        for (int i = 0; i < k; i++) pts[i] = (uint32_t)i + 1;
        lagrange_host(pts, (size_t)k, g->lambda);
        try {
            std::vector<prf_key> hk(keyless ? 0 : (size_t)k * g->t);
            for (size_t i = 0; i < hk.size(); i++) hk[i] = prf_key_from_bytes(keys + (size_t)COZK_PRF_KEY_BYTES * i);
            if (!keyless) {
                g->d_keys = (prf_key*)ctx_dev_alloc(driver, hk.size() * sizeof(prf_key));
                HIP_TRY(hipMemcpyAsync(g->d_keys, hk.data(), hk.size() * sizeof(prf_key), hipMemcpyHostToDevice, driver->stream));
                HIP_TRY(hipStreamSynchronize(driver->stream));
            }
        } catch (...) {
            ctx_dev_free(driver, g->d_keys);
            delete g;
            throw;
        }
        *out = g;
    });
}

// the staging block of `need` elements, grown on demand
static void primary_group_stage(cozk_primary_group* g, size_t need) {
    if (need <= g->stage_cap) return;
    ctx_dev_free(g->driver, g->stage);
    g->stage = nullptr;
    g->stage_cap = 0;
    g->stage = (fe*)ctx_dev_alloc(g->driver, need * sizeof(fe));
    g->stage_cap = need;
}

extern "C" {

int cozk_primary_group_free(cozk_primary_group* g) {
    if (!g) return COZK_OK;
    ctx_dev_free(g->driver, g->d_keys);
    ctx_dev_free(g->driver, g->stage);
    delete g;
    return COZK_OK;
}

int cozk_primary_group_create(cozk_ctx* driver, cozk_primary* const* members, int k, const uint8_t* keys, cozk_primary_group** out) {
    return primary_group_make(driver, members, k, keys, false, "primary_group_create", out);
}

int cozk_primary_group_create_king(cozk_ctx* driver, cozk_primary* const* members, int k, cozk_primary_group** out) {
    return primary_group_make(driver, members, k, nullptr, true, "primary_group_create_king", out);
}

size_t cozk_primary_group_len(const cozk_primary_group* g) { return g ? g->members[0]->n : 0; }

int cozk_primary_group_level(cozk_primary_group* g, int level, uint64_t counter, size_t* n_elems) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(n_elems, "primary_group_level: null argument");
        COZK_REQUIRE(!g->keyless, "primary_group_level: the group has no PRF keys (cozk_primary_group_create_king): cozk_primary_group_level_king");
        primary_group_check(ctx, g->members.data(), g->k, "primary_group_level", true);
        const cozk_primary* m0 = g->members[0];
        COZK_REQUIRE(level >= 1 && level <= m0->max_levels && m0->n_items, "primary_group_level: bad level / no items");
        const size_t n_el = m0->level_elems[level - 1];
        *n_elems = n_el;
        if (!n_el) return;  // nothing at this level: no launch, and the caller's counter stays
        const size_t k = (size_t)g->k, need = k * k * n_el;
        for (cozk_primary* p : g->members) COZK_REQUIRE(p->P[level - 1][0] && p->P_cap[level - 1] >= n_el, "primary_group_level: a member has no level buffer");
        primary_group_stage(g, need);
        primary_group_wait_members(g);
        const PrimGroupArgs a = primary_group_args(g);
        const size_t cap = m0->cap[m0->cur];
        const dim3 gd(grid_for(m0->n_items), (unsigned)m0->degree, (unsigned)k);
#define PRIM_GROUP_DEAL_(DEG) \
    k_primary_group_deal<DEG><<<gd, PT, 0, ctx->stream>>>(a, cap, m0->n_instr, m0->n_mem, m0->degree, m0->n_items, level, g->d_keys, g->t, counter, g->stage, n_el)
        switch (g->t) {
            case 1: PRIM_GROUP_DEAL_(1); break;
            case 2: PRIM_GROUP_DEAL_(2); break;
            case 3: PRIM_GROUP_DEAL_(3); break;
            default: PRIM_GROUP_DEAL_(0); break;
        }
#undef PRIM_GROUP_DEAL_
        HIP_TRY(hipGetLastError());
        PrimGroupCombineArgs ca;
        memset(&ca, 0, sizeof ca);
        for (size_t q = 0; q < k; q++) {
            ca.out[q] = g->members[q]->P[level - 1][0];
            ca.lambda[q] = g->lambda[q];
        }
        k_primary_group_combine<<<dim3(grid_for(n_el), (unsigned)k), PT, 0, ctx->stream>>>(ca, g->stage, n_el);
        HIP_TRY(hipGetLastError());
        stream_drain_by_flag(ctx);  // the members' own streams may go on
    });
}

size_t cozk_primary_group_staging_bytes(const cozk_primary_group* g) { return g ? g->stage_cap * sizeof(fe) : 0; }

int cozk_primary_group_level_king(cozk_primary_group* g, int level, const cozk_vec* const* r_t, const cozk_vec* const* r_2t, size_t r_offset,
                                  size_t* n_elems) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(n_elems && r_t && r_2t, "primary_group_level_king: null argument");
        const size_t k = (size_t)g->k;
        for (size_t i = 0; i < k; i++)
            for (const cozk_vec* v : {r_t[i], r_2t[i]})
                COZK_REQUIRE(v && v->kind == COZK_SCALAR_FR && v->ctx && v->ctx->device == ctx->device,
                             "primary_group_level_king: 2 (2t + 1) FR halves of the pair on the driver's device");
        primary_group_check(ctx, g->members.data(), g->k, "primary_group_level_king", true);
        const cozk_primary* m0 = g->members[0];
        COZK_REQUIRE(level >= 1 && level <= m0->max_levels && m0->n_items, "primary_group_level_king: bad level / no items");
        const size_t n_el = m0->level_elems[level - 1];
        for (size_t i = 0; i < k; i++)
            for (const cozk_vec* v : {r_t[i], r_2t[i]})
                COZK_REQUIRE(r_offset <= v->n && n_el <= v->n - r_offset, "primary_group_level_king: r_offset + n_elems <= len of every half of the pair");
        *n_elems = n_el;
        if (!n_el) return;  // nothing at this level: no launch, and no element of the pair is used
        for (cozk_primary* p : g->members) COZK_REQUIRE(p->P[level - 1][0] && p->P_cap[level - 1] >= n_el, "primary_group_level_king: a member has no level buffer");
        primary_group_stage(g, k * n_el);
        primary_group_wait_members(g);
        const PrimGroupArgs a = primary_group_args(g);
        PrimGroupMaskArgs ra;
        memset(&ra, 0, sizeof ra);
        const fe *mp[PRIM_GROUP_MAX], *rt[PRIM_GROUP_MAX];
        fe* o[PRIM_GROUP_MAX];
        for (size_t i = 0; i < k; i++) {
            ra.r2t[i] = (const fe*)r_2t[i]->d + r_offset;
            mp[i] = g->stage + i * n_el;
            rt[i] = (const fe*)r_t[i]->d;
            o[i] = g->members[i]->P[level - 1][0];
        }
        const dim3 gd(grid_for(m0->n_items), (unsigned)m0->degree, (unsigned)k);
        k_primary_group_mask<<<gd, PT, 0, ctx->stream>>>(a, ra, m0->cap[m0->cur], m0->n_instr, m0->n_mem, m0->degree, m0->n_items, level, g->stage, n_el);
        HIP_TRY(hipGetLastError());
        shamir_launch_king_finish(ctx->stream, mp, (int)k, rt, r_offset, (int)k, o, n_el);
        stream_drain_by_flag(ctx);  // the members' own streams may go on
    });
}

int cozk_primary_group_round_finish(cozk_primary_group* g, uint64_t* out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(out, "primary_group_round_finish: null argument");
        primary_group_check(ctx, g->members.data(), g->k, "primary_group_round_finish", true);
        const cozk_primary* m0 = g->members[0];
        const int D = m0->degree;
        const unsigned k = (unsigned)g->k, rows = 2u * (unsigned)D * k;
        std::vector<fe> s((size_t)rows, Fr::zero());
        if (m0->n_items) {
            const GroupSums gs = group_sums(ctx, rows, m0->n_items, false, std::max(64u, ROUND_GRID_MAX / k));
            primary_group_wait_members(g);
            const PrimGroupArgs a = primary_group_args(g);
            k_primary_group_final<<<dim3(gs.gx, (unsigned)D, k), PT, 0, ctx->stream>>>(a, m0->cap[m0->cur], m0->n_instr, m0->n_mem, D, m0->n_items, gs.partial);
            HIP_TRY(hipGetLastError());
            gs.fetch(s.data());
        }
        for (unsigned m = 0; m < k; m++) {
            const cozk_primary* p = g->members[m];
            for (int kk = 0; kk < D; kk++) {
                const fe ab = Fr::add(p->lin_sums[kk], s[(size_t)2 * D * m + kk]);
                fe_to_u64x4(Fr::add(ab, s[(size_t)2 * D * m + D + kk]), out + 4 * ((size_t)m * D + kk));
            }
        }
    });
}

// where member `member`'s reshared values of `level` live (device address; NULL when the level holds nothing) and how many there are
int cozk_primary_group_level_buffer(const cozk_primary_group* g, int member, int level, const void** buf, size_t* n_elems) {
    if (!g) return COZK_ERR_INVALID_ARG;
    return cozk_guard(g->driver, [&] {
        COZK_REQUIRE(buf && n_elems && member >= 0 && member < g->k, "primary_group_level_buffer: bad argument");
        const cozk_primary* p = g->members[(size_t)member];
        COZK_REQUIRE(level >= 1 && level <= p->max_levels, "primary_group_level_buffer: bad level");
        *n_elems = p->n_items ? p->level_elems[level - 1] : 0;
        *buf = *n_elems ? p->P[level - 1][0] : nullptr;
    });
}

}  // extern "C"
