// Sparse pair layers of the toggled batched grand product -- part of poly.hip's translation unit.
//
//   cozk_sparse_layer  <->  Rep3SparseInterleavedPolynomial (co-jolt/src/poly/sparse_interleaved_poly.rs:28-737): an interleaved
//   layer whose missing entries are this party's trivial share of ONE.
//
// MI355X formulation: STORED PAIRS.  A dense interleaved layer of length n is n / 2 pairs (L_j, R_j) at entries 2j, 2j + 1; the
// object stores the pairs that are not (one, one): a sorted U32 array idx[cnt] of global pair indices and the values L, R
// interleaved in that order (one FR array of 2 cnt, two for Rep3).  The reference keeps single elements and walks 20 neighbour
// cases per bind (:210-380); with pairs both structural maps are ONE operation on the sorted list:
//   bind          stored pairs 2k, 2k + 1 -> pair k, L' = lerp(L_2k, L_2k+1, r), R' likewise     (missing sibling = (one, one))
//   layer_output  pair j -> entry j of the next layer = half j & 1 of that layer's pair j >> 1
// either way neighbours with equal idx >> 1 merge into one item at idx >> 1: a head flag (idx[i] >> 1 != idx[i-1] >> 1), an
// exclusive scan of the flags and one lane per merged group, which reads its own item and, if stored, the sibling (the next item).
// The pattern is public and the same for every party.  The values are, entry by entry, those of the dense formulation
// restricted to the stored pairs (a pair (a, one) is multiplied where the reference keeps it "ready": the same value).
//
// The scan: tiles of SP_TILE items, one workgroup each -- count the flags per tile (k_sparse_count), one workgroup scans the tile
// counts (k_sparse_scan_blocks), the consumer kernels recompute the flags and place every flagged item with ballots + a running
// tile offset (sp_tile_pos).  The flags are 0/1, so a wave's prefix is one popcount.
//
// The dense formulation pads a ragged tail with ZEROS (dense_interleaved_poly.rs:155-195) where a sparse layer would read a
// missing pair as ones, so bind, round and layer_output are defined for n % 4 == 0 only: every length the toggled tree has
// down to the reference's coalesce point (one pair per circuit, n = 2 * batch), where the prover hands over to a dense layer.

struct cozk_sparse_layer {
    cozk_ctx* ctx;
    int mode;
    size_t n;              // dense length (entries)
    size_t cnt;            // stored pairs
    uint32_t* idx[2];      // ping-pong: sorted pair indices
    fe* v[2][2];           // ping-pong [which][component]: L, R interleaved, 2 * cnt entries
    size_t cap[2];         // pairs each side holds
    int cur;
    bool planned;          // blk / next_cnt describe the current lists
    size_t next_cnt;       // merged groups = stored pairs after a bind = stored pairs of the output layer
    unsigned long long* blk;  // exclusive tile offsets of the head flags (+ the total)
    size_t blk_cap;
    uint64_t rounds_run;
    mutable int party;     // whose trivial share of one a missing entry is; -1: not known yet (a Rep3 layer from explicit lists)
};

static constexpr int SP_ITEMS = 8;  // items per lane of a scan tile
static constexpr size_t SP_TILE = (size_t)PT * SP_ITEMS;

// head of a merged group: the first stored pair of its quad
struct SpHeadFlag {
    const uint32_t* idx;
    __device__ __forceinline__ bool operator()(size_t i) const { return i == 0 || (idx[i] >> 1) != (idx[i - 1] >> 1); }
};
// pair p of the toggle layer's output is stored iff one of its two flags is set; the two 0/1 bytes are one aligned 16-bit load
// (N is a power of two >= 2, so a pair never straddles two circuits)
struct SpToggleFlag {
    const uint8_t* fl;
    int log_n;
    __device__ __forceinline__ uint16_t pair(size_t p) const {
        const size_t e = 2 * p, b = e >> log_n, i = e & (((size_t)1 << log_n) - 1);
        return *(const uint16_t*)(fl + (((b >> 1) << log_n) + i));
    }
    __device__ __forceinline__ bool operator()(size_t p) const { return pair(p) != 0; }
};

template <class F>
__global__ void __launch_bounds__(PT) k_sparse_count(F f, size_t n, unsigned long long* __restrict__ blk) {
    __shared__ unsigned wc[PT / 64];
    const size_t base = (size_t)blockIdx.x * SP_TILE;
    unsigned c = 0;  // wave-uniform
    for (int k = 0; k < SP_ITEMS; k++) {
        const size_t i = base + (size_t)k * PT + threadIdx.x;
        const bool on = i < n && f(i);
        c += (unsigned)__popcll(__ballot(on));
    }
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < PT / 64; w++) t += wc[w];
        blk[blockIdx.x] = t;
    }
}

// exclusive scan of nb tile counts in place, the total to blk[nb]: one workgroup, a contiguous run per lane
__global__ void __launch_bounds__(1024) k_sparse_scan_blocks(unsigned long long* __restrict__ blk, size_t nb) {
    __shared__ unsigned long long part[1024];
    const size_t per = (nb + 1023) / 1024;
    const size_t lo = (size_t)threadIdx.x * per < nb ? (size_t)threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    unsigned long long s = 0;
    for (size_t i = lo; i < hi; i++) s += blk[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; t++) {
            const unsigned long long c = part[t];
            part[t] = run;
            run += c;
        }
        blk[nb] = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (size_t i = lo; i < hi; i++) {
        const unsigned long long c = blk[i];
        blk[i] = run;
        run += c;
    }
}

// position of this lane's item among the flagged items of the whole list (meaningful where `on`); every lane of the workgroup
// calls it, `run` is the tile's running offset (workgroup-uniform)
static __device__ __forceinline__ unsigned long long sp_tile_pos(bool on, unsigned long long& run, unsigned* wc) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(on);
    if (lane == 0) wc[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < PT / 64; w++) {
        const unsigned c = wc[w];
        all += c;
        if (w < wv) before += c;
    }
    __syncthreads();
    const unsigned long long pos = run + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    run += all;
    return pos;
}

template <int NC>
static __device__ __forceinline__ Sh<NC> sp_one(const fe& one_a, const fe& one_b) {
    Sh<NC> o;
    o.c[0] = one_a;
    if (NC == 2) o.c[NC - 1] = one_b;
    return o;
}

// compaction of the toggle layer's output (sparse_grand_product.rs:76-97): the stored pairs, each entry flag ? fingerprint : one
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_from_toggle(const fe* __restrict__ pa, const fe* __restrict__ pb, SpToggleFlag f, size_t npairs, fe one_a,
                                                        fe one_b, const unsigned long long* __restrict__ blk, uint32_t* __restrict__ oidx,
                                                        fe* __restrict__ oa, fe* __restrict__ ob) {
    __shared__ unsigned wc[PT / 64];
    unsigned long long run = blk[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SP_TILE;
    const Sh<NC> one = sp_one<NC>(one_a, one_b);
    for (int k = 0; k < SP_ITEMS; k++) {
        const size_t p = base + (size_t)k * PT + threadIdx.x;
        const uint16_t v = p < npairs ? f.pair(p) : (uint16_t)0;
        const unsigned long long pos = sp_tile_pos(v != 0, run, wc);
        if (v != 0) {
            oidx[pos] = (uint32_t)p;
            sh_store<NC>(oa, ob, 2 * pos, (v & 0xff) ? sh_load<NC>(pa, pb, 2 * p) : one);
            sh_store<NC>(oa, ob, 2 * pos + 1, (v >> 8) ? sh_load<NC>(pa, pb, 2 * p + 1) : one);
        }
    }
}

// item i as a member of its merged group
struct SpGroup {
    bool head;     // the lane that owns the group
    bool has_sib;  // the next item is the other half of the group
    uint32_t q;    // idx >> 1: the group's index
    uint32_t half; // idx & 1
};
static __device__ __forceinline__ SpGroup sp_group(const uint32_t* __restrict__ idx, size_t i, size_t cnt) {
    SpGroup g{false, false, 0u, 0u};
    if (i >= cnt) return g;
    const uint32_t me = idx[i];
    g.q = me >> 1;
    g.half = me & 1u;
    g.head = i == 0 || (idx[i - 1] >> 1) != g.q;
    g.has_sib = i + 1 < cnt && (idx[i + 1] >> 1) == g.q;
    return g;
}
// the four entries of a head's group: pair 2q = (L0, R0), pair 2q + 1 = (L1, R1), a missing one = (one, one).  The list is strictly
// increasing, so a head with a sibling is the even half.  A lane reads 64 x NC contiguous bytes per stored pair in 16-byte loads.
template <int NC>
static __device__ __forceinline__ void sp_quad(const fe* __restrict__ va, const fe* __restrict__ vb, size_t i, const SpGroup& g, const Sh<NC>& one, Sh<NC>& L0,
                                               Sh<NC>& R0, Sh<NC>& L1, Sh<NC>& R1) {
    L0 = R0 = L1 = R1 = one;
    if (g.half == 0) {
        L0 = sh_load<NC>(va, vb, 2 * i);
        R0 = sh_load<NC>(va, vb, 2 * i + 1);
        if (g.has_sib) {
            L1 = sh_load<NC>(va, vb, 2 * i + 2);
            R1 = sh_load<NC>(va, vb, 2 * i + 3);
        }
    } else {
        L1 = sh_load<NC>(va, vb, 2 * i);
        R1 = sh_load<NC>(va, vb, 2 * i + 1);
    }
}

// merge-bind (sparse_interleaved_poly.rs:210-380 in pair form)
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_bind(const uint32_t* __restrict__ idx, const fe* __restrict__ va, const fe* __restrict__ vb, size_t cnt,
                                                 const unsigned long long* __restrict__ blk, fe one_a, fe one_b, fe r, uint32_t* __restrict__ oidx,
                                                 fe* __restrict__ oa, fe* __restrict__ ob) {
    __shared__ unsigned wc[PT / 64];
    unsigned long long run = blk[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SP_TILE;
    const Sh<NC> one = sp_one<NC>(one_a, one_b);
    for (int k = 0; k < SP_ITEMS; k++) {
        const size_t i = base + (size_t)k * PT + threadIdx.x;
        const SpGroup g = sp_group(idx, i, cnt);
        const unsigned long long pos = sp_tile_pos(g.head, run, wc);
        if (g.head) {
            Sh<NC> L0, R0, L1, R1;
            sp_quad<NC>(va, vb, i, g, one, L0, R0, L1, R1);
            oidx[pos] = g.q;
            sh_store<NC>(oa, ob, 2 * pos, sh_lerp<NC>(L0, L1, r));
            sh_store<NC>(oa, ob, 2 * pos + 1, sh_lerp<NC>(R0, R1, r));
        }
    }
}

// merge-output (layer_output, sparse_interleaved_poly.rs:135-196, local half): per merged group the two additive products of its
// pairs, a missing pair the additive trivial one `add_one`; + the zero-sharing mask at counter + position when masked
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_output(const uint32_t* __restrict__ idx, const fe* __restrict__ va, const fe* __restrict__ vb, size_t cnt,
                                                   const unsigned long long* __restrict__ blk, fe add_one, int masked, prf_key key_self, prf_key key_prev,
                                                   uint64_t ctr, fe* __restrict__ out) {
    __shared__ unsigned wc[PT / 64];
    unsigned long long run = blk[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SP_TILE;
    for (int k = 0; k < SP_ITEMS; k++) {
        const size_t i = base + (size_t)k * PT + threadIdx.x;
        const SpGroup g = sp_group(idx, i, cnt);
        const unsigned long long pos = sp_tile_pos(g.head, run, wc);
        if (g.head) {
            const fe mine = sh_local_mul<NC>(sh_load<NC>(va, vb, 2 * i), sh_load<NC>(va, vb, 2 * i + 1));
            fe p0 = g.half == 0 ? mine : add_one, p1 = g.half == 1 ? mine : add_one;
            if (g.has_sib) p1 = sh_local_mul<NC>(sh_load<NC>(va, vb, 2 * i + 2), sh_load<NC>(va, vb, 2 * i + 3));
            if (masked) {
                const uint64_t c = ctr + 2 * pos;
                p0 = Fr::add(p0, Fr::sub(prf_fr(key_self, c), prf_fr(key_prev, c)));
                p1 = Fr::add(p1, Fr::sub(prf_fr(key_self, c + 1), prf_fr(key_prev, c + 1)));
            }
            fe_store(out + 2 * pos, p0);
            fe_store(out + 2 * pos + 1, p1);
        }
    }
}

// the merged groups' indices alone: the idx of the layer that layer_output or a bind gives
__global__ void __launch_bounds__(PT) k_sparse_group_idx(const uint32_t* __restrict__ idx, size_t cnt, const unsigned long long* __restrict__ blk,
                                                      uint32_t* __restrict__ oidx) {
    __shared__ unsigned wc[PT / 64];
    unsigned long long run = blk[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SP_TILE;
    for (int k = 0; k < SP_ITEMS; k++) {
        const size_t i = base + (size_t)k * PT + threadIdx.x;
        const SpGroup g = sp_group(idx, i, cnt);
        const unsigned long long pos = sp_tile_pos(g.head, run, wc);
        if (g.head) oidx[pos] = g.q;
    }
}

// Round sums in delta form (compute_cubic, sparse_interleaved_poly.rs:415-715): over the merged groups (quads q = idx >> 1)
//     D(X) = sum eq_q(X) (L(X) R(X) - sub_one)           X = 0, 2, 3
// sub_one = 1 for the party that additive_sub_shared_by_public gives the public part to (party 0, the plain prover), 0 for the
// others; the host adds S_all(X) for the same party (additive_add_public).  The eq weights come from the flat or nested split-eq
// tables as k_toggle_cubic takes them.  One lane per stored item; the lanes that are not heads idle (at the densities the storage
// rule admits most items are heads).  Three accumulators and fully unrolled X loops: nothing is indexed dynamically.
template <int NC, int NESTED>
__global__ void __launch_bounds__(PT) k_sparse_cubic(const uint32_t* __restrict__ idx, const fe* __restrict__ va, const fe* __restrict__ vb, size_t cnt,
                                                  fe one_a, fe one_b, fe sub_one, size_t nquads, const fe* __restrict__ E1, int log_E1_half,
                                                  const fe* __restrict__ E2, size_t E2_len, fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    const size_t limit = split_eq_limit<NESTED>(E2_len, log_E1_half);
    if (nquads > limit) nquads = limit;
    const Sh<NC> one = sp_one<NC>(one_a, one_b);
    fe D0 = Fr::zero(), D2 = Fr::zero(), D3 = Fr::zero();
    const size_t stride = (size_t)gridDim.x * PT;
    for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < cnt; i += stride) {
        const SpGroup g = sp_group(idx, i, cnt);
        if (!g.head || g.q >= nquads) continue;
        const size_t j = g.q;
        Sh<NC> L0, R0, L1, R1;
        sp_quad<NC>(va, vb, i, g, one, L0, R0, L1, R1);
        // the products first, the eq weights after them: fewer values live at once
        fe t0 = Fr::sub(sh_local_mul<NC>(L0, R0), sub_one);
        const Sh<NC> ml = sh_sub<NC>(L1, L0), mr = sh_sub<NC>(R1, R0);
        L1 = sh_add<NC>(L1, ml);
        R1 = sh_add<NC>(R1, mr);
        fe t2 = Fr::sub(sh_local_mul<NC>(L1, R1), sub_one);
        L1 = sh_add<NC>(L1, ml);
        R1 = sh_add<NC>(R1, mr);
        fe t3 = Fr::sub(sh_local_mul<NC>(L1, R1), sub_one);
        fe e[3], sc;
        split_eq_at(NESTED, E1, log_E1_half, E2, j, e, sc);
        if (NESTED) {
            t0 = Fr::mul(t0, sc);
            t2 = Fr::mul(t2, sc);
            t3 = Fr::mul(t3, sc);
        }
        D0 = Fr::add(D0, Fr::mul(e[0], t0));
        D2 = Fr::add(D2, Fr::mul(e[1], t2));
        D3 = Fr::add(D3, Fr::mul(e[2], t3));
    }
    partial_row_sum(D0, sh4, partial, 0);
    partial_row_sum(D2, sh4, partial, 1);
    partial_row_sum(D3, sh4, partial, 2);
}

// scatter to dense: fill with trivial ones, then the stored pairs
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_fill(fe* __restrict__ oa, fe* __restrict__ ob, size_t n, fe one_a, fe one_b) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    fe_store(oa + i, one_a);
    if (NC == 2) fe_store(ob + i, one_b);
}
template <int NC>
__global__ void __launch_bounds__(PT) k_sparse_scatter(const uint32_t* __restrict__ idx, const fe* __restrict__ va, const fe* __restrict__ vb, size_t cnt,
                                                    size_t npairs, fe* __restrict__ oa, fe* __restrict__ ob) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= cnt) return;
    const size_t p = idx[i];
    if (p >= npairs) return;
    sh_store<NC>(oa, ob, 2 * p, sh_load<NC>(va, vb, 2 * i));
    sh_store<NC>(oa, ob, 2 * p + 1, sh_load<NC>(va, vb, 2 * i + 1));
}

// ------------------------------------------------------------------ host side
// promote_to_trivial_share(party_id, one): P0 (1, 0), P1 (0, 1), P2 (0, 0); the plain prover's one is 1
static void sparse_ones(int mode, int party_id, fe& one_a, fe& one_b) {
    one_a = (mode == COZK_MODE_PLAIN || party_id == 0) ? Fr::one() : Fr::zero();
    one_b = (mode == COZK_MODE_REP3 && party_id == 1) ? Fr::one() : Fr::zero();
}
static const fe* sp_v(const cozk_sparse_layer* s, int c) { return s->v[s->cur][c]; }
static size_t sparse_tiles(size_t items) { return (items + SP_TILE - 1) / SP_TILE; }

static cozk_sparse_layer* sparse_new(cozk_ctx* ctx, int mode, size_t n) {
    cozk_sparse_layer* s = new cozk_sparse_layer();
    s->ctx = ctx;
    s->mode = mode;
    s->n = n;
    s->cnt = 0;
    for (int w = 0; w < 2; w++) {
        s->idx[w] = nullptr;
        s->v[w][0] = s->v[w][1] = nullptr;
        s->cap[w] = 0;
    }
    s->cur = 0;
    s->planned = false;
    s->next_cnt = 0;
    s->blk = nullptr;
    s->blk_cap = 0;
    s->rounds_run = 0;
    s->party = mode == COZK_MODE_PLAIN ? 0 : -1;
    return s;
}
static void sparse_release_side(cozk_sparse_layer* s, int w) {
    if (s->idx[w]) ctx_dev_free(s->ctx, s->idx[w]);
    for (int c = 0; c < 2; c++)
        if (s->v[w][c]) ctx_dev_free(s->ctx, s->v[w][c]);
    s->idx[w] = nullptr;
    s->v[w][0] = s->v[w][1] = nullptr;
    s->cap[w] = 0;
}
// side w holds `pairs` stored pairs (from the pool of the layer's own context)
static void sparse_reserve(cozk_sparse_layer* s, int w, size_t pairs) {
    if (s->cap[w] >= pairs && s->idx[w]) return;
    sparse_release_side(s, w);
    const size_t p = pairs ? pairs : 1;
    s->idx[w] = (uint32_t*)ctx_dev_alloc(s->ctx, p * sizeof(uint32_t));
    s->v[w][0] = (fe*)ctx_dev_alloc(s->ctx, 2 * p * sizeof(fe));
    if (s->mode == COZK_MODE_REP3) s->v[w][1] = (fe*)ctx_dev_alloc(s->ctx, 2 * p * sizeof(fe));
    s->cap[w] = p;
}
static unsigned long long* sparse_blk(cozk_sparse_layer* s, size_t tiles) {
    if (s->blk_cap < tiles + 1) {
        if (s->blk) ctx_dev_free(s->ctx, s->blk);
        s->blk = (unsigned long long*)ctx_dev_alloc(s->ctx, (tiles + 1) * sizeof(unsigned long long));
        s->blk_cap = tiles + 1;
    }
    return s->blk;
}
// one 64-bit word from the device (the total of a scan)
static unsigned long long sparse_fetch_u64(cozk_ctx* ctx, const unsigned long long* d) {
    unsigned long long* pin = (unsigned long long*)ctx_pinned(ctx, sizeof(unsigned long long));
    HIP_TRY(hipMemcpyAsync(pin, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return *pin;
}
// count + scan of the flags F over `items` items: tile offsets and the total at blk[tiles]; items > 0
template <class F>
static unsigned long long sparse_scan(cozk_ctx* ctx, F f, size_t items, unsigned long long* blk) {
    const size_t tiles = sparse_tiles(items);
    k_sparse_count<F><<<(unsigned)tiles, PT, 0, ctx->stream>>>(f, items, blk);
    HIP_TRY(hipGetLastError());
    k_sparse_scan_blocks<<<1, 1024, 0, ctx->stream>>>(blk, tiles);
    HIP_TRY(hipGetLastError());
    return sparse_fetch_u64(ctx, blk + tiles);
}
// the merge plan of the current lists: the head flags' tile offsets and the number of merged groups
static void sparse_plan(cozk_ctx* ctx, cozk_sparse_layer* s) {
    if (s->planned) return;
    s->next_cnt = s->cnt ? (size_t)sparse_scan(ctx, SpHeadFlag{s->idx[s->cur]}, s->cnt, sparse_blk(s, sparse_tiles(s->cnt))) : 0;
    s->planned = true;
}
// the calls that name the party fix it; a layer keeps the one it has
static bool sparse_party_ok(const cozk_sparse_layer* s, int party_id) {
    if (party_id < 0 || party_id > 2) return false;
    if (s->mode == COZK_MODE_PLAIN) return true;
    if (s->party < 0) s->party = party_id;
    return s->party == party_id;
}
static size_t sparse_bytes(const cozk_sparse_layer* s) { return s->cnt * (size_t)(64 * (s->mode == COZK_MODE_REP3 ? 2 : 1) + 4); }

extern "C" {

int cozk_sparse_layer_free(cozk_sparse_layer* s) {
    if (!s) return COZK_OK;
    for (int w = 0; w < 2; w++) sparse_release_side(s, w);
    if (s->blk) ctx_dev_free(s->ctx, s->blk);
    delete s;
    return COZK_OK;
}
size_t cozk_sparse_layer_len(const cozk_sparse_layer* s) { return s ? s->n : 0; }
size_t cozk_sparse_layer_count(const cozk_sparse_layer* s) { return s ? s->cnt : 0; }
size_t cozk_sparse_layer_bytes(const cozk_sparse_layer* s) { return s ? sparse_bytes(s) : 0; }

int cozk_sparse_layer_next_count(cozk_ctx* ctx, cozk_sparse_layer* s, size_t* out) {
    if (out) *out = 0;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && out, "sparse_layer_next_count: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_next_count: the layer belongs to another context");
        sparse_plan(ctx, s);
        *out = s->next_cnt;
    });
}

// Rep3SparseInterleavedPolynomial::new (sparse_interleaved_poly.rs:40-75) from explicit lists
int cozk_sparse_layer_create(cozk_ctx* ctx, int mode, size_t n, cozk_vec* idx, cozk_vec* a, cozk_vec* b, int take_ownership, cozk_sparse_layer** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && idx && a && out, "sparse_layer_create: null argument");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3, "sparse_layer_create: mode must be COZK_MODE_PLAIN or COZK_MODE_REP3");
        COZK_REQUIRE(n >= 2 && n % 2 == 0, "sparse_layer_create: the dense length must be even and >= 2");
        COZK_REQUIRE(n / 2 <= ((size_t)1 << 32), "sparse_layer_create: more than 2^32 pairs");
        COZK_REQUIRE(idx->kind == COZK_SCALAR_U32, "sparse_layer_create: idx must be a U32 vector");
        const size_t cnt = idx->n;
        COZK_REQUIRE(cnt <= n / 2, "sparse_layer_create: more stored pairs than the layer has");
        COZK_REQUIRE(a->kind == COZK_SCALAR_FR && a->n == 2 * cnt, "sparse_layer_create: the values must be an FR vector of 2 * count entries");
        COZK_REQUIRE(mode == COZK_MODE_PLAIN || (b && b->kind == COZK_SCALAR_FR && b->n == 2 * cnt),
                     "sparse_layer_create: a Rep3 layer needs the b values, an FR vector of 2 * count entries");
        {  // the pattern, checked on the host
            std::vector<uint32_t> h(cnt);
            if (cnt) HIP_TRY(hipMemcpyAsync(h.data(), idx->d, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < cnt; i++) {
                COZK_REQUIRE((size_t)h[i] < n / 2, "sparse_layer_create: a pair index is >= n / 2");
                COZK_REQUIRE(i == 0 || h[i] > h[i - 1], "sparse_layer_create: idx must be strictly increasing");
            }
        }
        cozk_sparse_layer* s = sparse_new(ctx, mode, n);
        struct Guard {
            cozk_sparse_layer* s;
            ~Guard() { if (s) cozk_sparse_layer_free(s); }
        } guard{s};
        cozk_vec* src[2] = {a, mode == COZK_MODE_REP3 ? b : nullptr};
        const bool adopt = take_ownership && idx->owned && a->owned && (!src[1] || src[1]->owned) && idx->ctx == ctx && a->ctx == ctx && (!src[1] || src[1]->ctx == ctx);
        if (adopt) {
            s->idx[0] = (uint32_t*)vec_adopt(idx);
            s->v[0][0] = (fe*)vec_adopt(a);
            if (src[1]) s->v[0][1] = (fe*)vec_adopt(src[1]);
            s->cap[0] = cnt;
        } else {
            sparse_reserve(s, 0, cnt);
            if (cnt) {
                HIP_TRY(hipMemcpyAsync(s->idx[0], idx->d, cnt * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
                HIP_TRY(hipMemcpyAsync(s->v[0][0], a->d, 2 * cnt * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
                if (src[1]) HIP_TRY(hipMemcpyAsync(s->v[0][1], src[1]->d, 2 * cnt * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        s->cnt = cnt;
        guard.s = nullptr;
        *out = s;
    });
}

// layer_output of the toggle layer (sparse_grand_product.rs:76-97) as stored pairs: a count, a scan and a write
int cozk_toggle_sparse_output(cozk_ctx* ctx, const cozk_toggle* t, int party_id, cozk_sparse_layer** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t && out, "toggle_sparse_output: null argument");
        COZK_REQUIRE(t->s.cur < 0 && party_id >= 0 && party_id < 3, "toggle_sparse_output: needs an unbound toggle layer and a party 0..2");
        const size_t n = t->s.batch * t->s.n0, npairs = n / 2;
        COZK_REQUIRE(npairs <= ((size_t)1 << 32), "toggle_sparse_output: more than 2^32 pairs");
        cozk_sparse_layer* s = sparse_new(ctx, t->mode, n);
        if (t->mode == COZK_MODE_REP3) s->party = party_id;
        struct Guard {
            cozk_sparse_layer* s;
            ~Guard() { if (s) cozk_sparse_layer_free(s); }
        } guard{s};
        const SpToggleFlag f{t->fl0, log2_sz(t->s.n0)};
        const size_t tiles = sparse_tiles(npairs);
        unsigned long long* blk = (unsigned long long*)ctx_dev_alloc(ctx, (tiles + 1) * sizeof(unsigned long long));
        struct Blk {
            cozk_ctx* ctx;
            void* p;
            ~Blk() { ctx_dev_free(ctx, p); }
        } blk_guard{ctx, blk};
        const size_t cnt = (size_t)sparse_scan(ctx, f, npairs, blk);
        sparse_reserve(s, 0, cnt);
        if (cnt) {
            fe one_a, one_b;
            sparse_ones(t->mode, party_id, one_a, one_b);
            auto* const kernel = t->mode == COZK_MODE_REP3 ? k_sparse_from_toggle<2> : k_sparse_from_toggle<1>;
            kernel<<<(unsigned)tiles, PT, 0, ctx->stream>>>(t->fp0[0], t->fp0[1], f, npairs, one_a, one_b, blk, s->idx[0], s->v[0][0], s->v[0][1]);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ctx->stream));  // blk returns to the pool with this call
        }
        s->cnt = cnt;
        guard.s = nullptr;
        *out = s;
    });
}

// local half of layer_output (sparse_interleaved_poly.rs:135-196): the compact vector of 2 * G additive products
int cozk_sparse_layer_output_local(cozk_ctx* ctx, cozk_sparse_layer* s, int masked, const uint8_t* key_self_b, const uint8_t* key_prev_b, uint64_t counter,
                                   cozk_vec** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && out && (!masked || (key_self_b && key_prev_b)), "sparse_layer_output_local: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_output_local: the layer belongs to another context");
        COZK_REQUIRE(s->party >= 0, "sparse_layer_output_local: the party of a Rep3 layer from explicit lists is not known before its first round or to_dense");
        const int party_id = s->party;
        COZK_REQUIRE(s->n % 4 == 0, "sparse_layer_output_local: the dense length must be a multiple of 4");
        prf_key seed_self{}, seed_prev{};
        if (masked) {
            seed_self = prf_key_from_bytes(key_self_b);
            seed_prev = prf_key_from_bytes(key_prev_b);
        }
        sparse_plan(ctx, s);
        const size_t G = s->next_cnt;
        fe* d = dev_alloc_fe(2 * G);
        if (G) {
            // additive::promote_to_trivial_share(one): party 0 holds 1, the others 0
            const fe add_one = (s->mode == COZK_MODE_PLAIN || party_id == 0) ? Fr::one() : Fr::zero();
            const unsigned tiles = (unsigned)sparse_tiles(s->cnt);
            if (s->mode == COZK_MODE_REP3)
                k_sparse_output<2><<<tiles, PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), sp_v(s, 1), s->cnt, s->blk, add_one, masked, seed_self, seed_prev, counter, d);
            else
                k_sparse_output<1><<<tiles, PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), nullptr, s->cnt, s->blk, add_one, masked, seed_self, seed_prev, counter, d);
            HIP_TRY(hipGetLastError());
        }
        *out = new cozk_vec{ctx, 2 * G, COZK_SCALAR_FR, d, 2 * G * sizeof(fe), true};
    });
}

// the products of cozk_sparse_layer_output_local (and, for Rep3, what the ring reshare gave for them) as the next layer
int cozk_sparse_layer_from_output(cozk_ctx* ctx, cozk_sparse_layer* s, cozk_vec* va, cozk_vec* vb, int take_ownership, cozk_sparse_layer** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && va && out, "sparse_layer_from_output: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_from_output: the layer belongs to another context");
        COZK_REQUIRE(s->n % 4 == 0, "sparse_layer_from_output: the dense length must be a multiple of 4");
        sparse_plan(ctx, s);
        const size_t G = s->next_cnt;
        COZK_REQUIRE(va->kind == COZK_SCALAR_FR && va->n == 2 * G, "sparse_layer_from_output: the products must be an FR vector of 2 * next_count entries");
        COZK_REQUIRE(s->mode == COZK_MODE_PLAIN || (vb && vb->kind == COZK_SCALAR_FR && vb->n == 2 * G),
                     "sparse_layer_from_output: a Rep3 layer needs the b products, an FR vector of 2 * next_count entries");
        cozk_sparse_layer* nx = sparse_new(ctx, s->mode, s->n / 2);
        nx->party = s->party;
        struct Guard {
            cozk_sparse_layer* s;
            ~Guard() { if (s) cozk_sparse_layer_free(s); }
        } guard{nx};
        cozk_vec* src[2] = {va, s->mode == COZK_MODE_REP3 ? vb : nullptr};
        const bool adopt = take_ownership && va->owned && va->ctx == ctx && (!src[1] || (src[1]->owned && src[1]->ctx == ctx));
        nx->idx[0] = (uint32_t*)ctx_dev_alloc(ctx, (G ? G : 1) * sizeof(uint32_t));
        nx->cap[0] = G ? G : 1;
        for (int c = 0; c < 2; c++) {
            if (!src[c]) continue;
            if (adopt) {
                nx->v[0][c] = (fe*)vec_adopt(src[c]);
            } else {
                nx->v[0][c] = (fe*)ctx_dev_alloc(ctx, 2 * (G ? G : 1) * sizeof(fe));
                if (G) HIP_TRY(hipMemcpyAsync(nx->v[0][c], src[c]->d, 2 * G * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        if (G) {
            k_sparse_group_idx<<<(unsigned)sparse_tiles(s->cnt), PT, 0, ctx->stream>>>(s->idx[s->cur], s->cnt, s->blk, nx->idx[0]);
            HIP_TRY(hipGetLastError());
        }
        nx->cnt = G;
        guard.s = nullptr;
        *out = nx;
    });
}

// Rep3Bindable::bind (sparse_interleaved_poly.rs:210-380)
int cozk_sparse_layer_bind(cozk_ctx* ctx, cozk_sparse_layer* s, const uint64_t r[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && r, "sparse_layer_bind: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_bind: the layer belongs to another context");
        COZK_REQUIRE(s->party >= 0, "sparse_layer_bind: the party of a Rep3 layer from explicit lists is not known before its first round or to_dense");
        const int party_id = s->party;
        COZK_REQUIRE(s->n >= 4, "sparse_layer_bind: the bind would leave fewer than one pair");
        COZK_REQUIRE(s->n % 4 == 0, "sparse_layer_bind: the dense length must be a multiple of 4");
        sparse_plan(ctx, s);
        const int dst = 1 - s->cur;
        const size_t G = s->next_cnt;
        sparse_reserve(s, dst, G);
        if (G) {
            fe one_a, one_b;
            sparse_ones(s->mode, party_id, one_a, one_b);
            const fe rr = fe_from_u64x4(r);
            const unsigned tiles = (unsigned)sparse_tiles(s->cnt);
            if (s->mode == COZK_MODE_REP3)
                k_sparse_bind<2><<<tiles, PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), sp_v(s, 1), s->cnt, s->blk, one_a, one_b, rr, s->idx[dst], s->v[dst][0], s->v[dst][1]);
            else
                k_sparse_bind<1><<<tiles, PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), nullptr, s->cnt, s->blk, one_a, one_b, rr, s->idx[dst], s->v[dst][0], nullptr);
            HIP_TRY(hipGetLastError());
        }
        s->cur = dst;
        s->cnt = G;
        s->n /= 2;
        s->planned = false;
    });
}

// one round of prove_sumcheck over a sparse layer (compute_cubic, sparse_interleaved_poly.rs:415-715): the contract of cozk_toggle_round
int cozk_sparse_layer_round(cozk_ctx* ctx, cozk_sparse_layer* s, cozk_spliteq* e, const uint64_t* r, int party_id, uint64_t out_evals[12]) {
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && e && out_evals, "sparse_layer_round: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_round: the layer belongs to another context");
        COZK_REQUIRE(e->ctx == ctx, "sparse_layer_round: the eq polynomial belongs to another context");
        COZK_REQUIRE(!spliteq_bound(e), "sparse_layer_round: eq polynomial already fully bound");
        COZK_REQUIRE(!r || !spliteq_last_bind(e), "sparse_layer_round: the bind would leave no round to run (the eq polynomial has one variable left)");
        const size_t n_round = r ? s->n / 2 : s->n;
        COZK_REQUIRE(!r || s->n >= 4, "sparse_layer_round: the bind would leave fewer than one pair");
        COZK_REQUIRE(s->n % 4 == 0 && n_round % 4 == 0, "sparse_layer_round: the dense length must be a multiple of 4 (in a binding round, of 8)");
        // the last check: it gives a layer that has no party yet this one, and a refused call leaves the layer as it was
        COZK_REQUIRE(sparse_party_ok(s, party_id), "sparse_layer_round: the party must be 0..2 and the one the layer was built for");
    });
    if (rc != COZK_OK) return rc;
    if (r) {
        // neither bind can refuse from here: each of their checks (the context, a known party, n >= 4 and a multiple of 4; an eq
        // polynomial that is not fully bound) is among the ones above, and the eq polynomial keeps a variable for the round below
        rc = cozk_sparse_layer_bind(ctx, s, r);
        if (rc != COZK_OK) return rc;
        rc = cozk_spliteq_bind(ctx, e, r);
        if (rc != COZK_OK) return rc;
    }
    return cozk_guard(ctx, [&] {
        const size_t nquads = s->n / 4;
        const EqView v = eq_view(e);
        fe sums[6];  // D(0), D(2), D(3), S_all(0), S_all(2), S_all(3)
        // additive_sub_shared_by_public / additive_add_public: party 0 only (the plain prover is party 0)
        const bool pub = s->mode == COZK_MODE_PLAIN || party_id == 0;
        if (s->cnt) {
            const unsigned gx = sum_grid(grid_capped(s->cnt, ROUND_GRID_MAX));
            const SumLaunch sl = sum_launch(ctx, 3, gx, 6);
            fe one_a, one_b;
            sparse_ones(s->mode, party_id, one_a, one_b);
            const fe sub_one = pub ? Fr::one() : Fr::zero();
            const bool rep3 = s->mode == COZK_MODE_REP3;
            auto* const kernel = rep3 ? (v.nested ? k_sparse_cubic<2, 1> : k_sparse_cubic<2, 0>) : (v.nested ? k_sparse_cubic<1, 1> : k_sparse_cubic<1, 0>);
            kernel<<<gx, PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), sp_v(s, 1), s->cnt, one_a, one_b, sub_one, nquads, v.E1, v.lg1, v.E2, v.E2_len, sl.partial);
            HIP_TRY(hipGetLastError());
            eq_sums_launch(ctx, v, nquads, sl.res + 3);
            finish_sums(ctx, sl, 3, gx, Fr::one(), 0, sums);
        } else {  // nothing stored: the all-ones sums alone, no launch of an empty grid
            fe* res = result_slot(ctx, 6);
            eq_sums_launch(ctx, v, nquads, res + 3);
            fetch_fe(ctx, res, 6, sums);
            for (int k = 0; k < 3; k++) sums[k] = Fr::zero();
        }
        for (int k = 0; k < 3; k++) fe_to_u64x4(pub ? Fr::add(sums[k], sums[3 + k]) : sums[k], out_evals + 4 * k);
        if (s->rounds_run++ == 0) {
            ctx->sparse_stats.layers_sparse++;
            ctx->sparse_stats.bytes_sparse += sparse_bytes(s);
            ctx->sparse_stats.bytes_dense_equivalent += (uint64_t)s->n * 32 * (s->mode == COZK_MODE_REP3 ? 2 : 1);
        }
        ctx->sparse_stats.sparse_rounds++;
    });
}

// coalesce (sparse_interleaved_poly.rs:91-103): the dense interleaved layer, an ordinary cozk_layer
int cozk_sparse_layer_to_dense(cozk_ctx* ctx, const cozk_sparse_layer* s, int party_id, cozk_layer** out) {
    if (out) *out = nullptr;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s && out, "sparse_layer_to_dense: null argument");
        COZK_REQUIRE(s->ctx == ctx, "sparse_layer_to_dense: the layer belongs to another context");
        COZK_REQUIRE(sparse_party_ok(s, party_id), "sparse_layer_to_dense: the party must be 0..2 and the one the layer was built for");
        cozk_layer* l = new cozk_layer();
        l->ctx = ctx;
        l->mode = s->mode;
        l->cur = 0;
        l->len = s->n;
        for (int w = 0; w < 2; w++) {
            l->buf[w][0] = l->buf[w][1] = nullptr;
            l->cap[w] = 0;
        }
        struct Guard {
            cozk_layer* l;
            ~Guard() { if (l) cozk_layer_free(l); }
        } guard{l};
        l->buf[0][0] = dev_alloc_fe(s->n);
        if (s->mode == COZK_MODE_REP3) l->buf[0][1] = dev_alloc_fe(s->n);
        l->cap[0] = s->n;
        fe one_a, one_b;
        sparse_ones(s->mode, party_id, one_a, one_b);
        if (s->mode == COZK_MODE_REP3) k_sparse_fill<2><<<grid_for(s->n), PT, 0, ctx->stream>>>(l->buf[0][0], l->buf[0][1], s->n, one_a, one_b);
        else k_sparse_fill<1><<<grid_for(s->n), PT, 0, ctx->stream>>>(l->buf[0][0], nullptr, s->n, one_a, one_b);
        HIP_TRY(hipGetLastError());
        if (s->cnt) {
            if (s->mode == COZK_MODE_REP3)
                k_sparse_scatter<2><<<grid_for(s->cnt), PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), sp_v(s, 1), s->cnt, s->n / 2, l->buf[0][0], l->buf[0][1]);
            else
                k_sparse_scatter<1><<<grid_for(s->cnt), PT, 0, ctx->stream>>>(s->idx[s->cur], sp_v(s, 0), nullptr, s->cnt, s->n / 2, l->buf[0][0], nullptr);
            HIP_TRY(hipGetLastError());
        }
        if (s->rounds_run) ctx->sparse_stats.handovers++;
        else ctx->sparse_stats.layers_scattered++;
        guard.l = nullptr;
        *out = l;
    });
}

// the lists -> host: idx count x u32, a / b 2 * count x 4 u64; any output pointer may be NULL
int cozk_sparse_layer_download(cozk_ctx* ctx, const cozk_sparse_layer* s, uint32_t* idx, uint64_t* a, uint64_t* b) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && s, "sparse_layer_download: null argument");
        if (s->cnt) {
            if (idx) HIP_TRY(hipMemcpyAsync(idx, s->idx[s->cur], s->cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            if (a) HIP_TRY(hipMemcpyAsync(a, sp_v(s, 0), 2 * s->cnt * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
            if (b && s->mode == COZK_MODE_REP3) HIP_TRY(hipMemcpyAsync(b, sp_v(s, 1), 2 * s->cnt * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    });
}

int cozk_sparse_get_stats(const cozk_ctx* ctx, cozk_sparse_stats* out) {
    if (!ctx || !out) return COZK_ERR_INVALID_ARG;
    *out = ctx->sparse_stats;
    return COZK_OK;
}
int cozk_sparse_reset_stats(cozk_ctx* ctx) {
    if (!ctx) return COZK_ERR_INVALID_ARG;
    ctx->sparse_stats = cozk_sparse_stats{};
    return COZK_OK;
}

}  // extern "C"
