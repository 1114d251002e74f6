// Toggle layer of the toggled (sparse) batched grand product -- part of poly.hip's translation unit.
//
//   cozk_toggle  <->  Rep3BatchedGrandProductToggleLayer (co-jolt/src/subprotocols/sparse_grand_product.rs:30-70): the bottom
//   layer of Rep3ToggledBatchedGrandProduct, whose left nodes are public 0/1 FLAGS and whose right nodes are shared
//   FINGERPRINTS; its output node is flag * fingerprint + (1 - flag).  The layers above it are
//   Rep3SparseInterleavedPolynomial (co-jolt/src/poly/sparse_interleaved_poly.rs): interleaved layers whose missing entries
//   are a share of ONE.
//
// MI355X formulation: DENSE-EQUIVALENT.  The reference keeps (index, value) lists and walks them with a dozen neighbour
// cases per entry (sparse_interleaved_poly.rs:210-380, sparse_grand_product.rs:153-290) because a CPU cannot afford the
// ones; what it computes per party is, term by term, the dense round polynomial of the layer with the ones filled in
// (compute_cubic adds the all-ones sums back: sparse_interleaved_poly.rs:455-490,560-700).  Here the layers ARE dense:
//   * the sparse layers are ordinary cozk_layer objects (k_layer_bind_cubic streams them at HBM rate, no index
//     arithmetic, no divergence) whose leaves come from k_toggle_output (flag ? fingerprint : share of one);
//   * the toggle layer keeps flags and fingerprints as two dense arrays; its round uses the reference's own delta form
//     (all-ones sums in closed form + corrections for the pairs with a set flag), reads 2 bytes per pair in the first
//     round, and compacts the active pairs per wave through an LDS queue so the heavy path runs with full lanes -- with
//     Jolt's ~10 % flag density that is where the sparsity pays on this machine, without a global compaction pass.
// Every party's message equals the reference's sparse computation exactly (field arithmetic is exact and the terms
// are the same); the oracle (oracle/pysparse.py) restates the SPARSE algorithms literally and the parity tests compare
// against it.

static inline int log2_sz(size_t n) {
    int l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

// Where a toggle layer stands in its binds -- the ONE copy of the progression for cozk_toggle and cozk_toggle_group
// (sparse_grand_product.rs:104-290): n_cur halves per bind; the bind that leaves one entry per circuit (layer_len == 2) coalesces to
// per-circuit vectors of L = next_power_of_two(batch) entries, which then halve.
struct ToggleShape {
    size_t batch;    // circuits (2 per flag column)
    size_t n0;       // fingerprints per circuit (power of two)
    size_t n_cur;    // current per-circuit length (n0 / 2^binds) while not coalesced
    size_t L;        // length of the coalesced vectors
    bool coalesced;  // flags / fingerprints are per-circuit vectors of length L (:104-134)
    int cur;         // -1: unbound (the packed 0/1 flag bytes); else which ping-pong side is live
    void init(size_t batch_, size_t n0_) {
        batch = batch_;
        n0 = n_cur = n0_;
        coalesced = false;
        L = 1;
        while (L < batch) L <<= 1;
        cur = -1;
    }
    size_t npairs() const { return coalesced ? L / 2 : batch * n_cur / 2; }
    int log_half_n() const { return coalesced ? -1 : log2_sz(n_cur / 2); }
    bool bound() const { return coalesced && L == 1; }
    bool last_bind() const { return coalesced && L == 2; }  // the bind that leaves no round to run
    int dst() const { return cur < 0 ? 0 : 1 - cur; }
    // entries the next bind writes, and whether it is the one that coalesces
    struct BindSizes {
        size_t n_fp, n_fl;
        bool coalesces;
    };
    BindSizes bind_sizes() const {
        if (coalesced) return BindSizes{L / 2, L / 2, false};
        return BindSizes{batch * n_cur / 2, (batch / 2) * n_cur / 2, n_cur == 2};
    }
    void advance() {  // the bind went to side dst()
        cur = dst();
        if (coalesced) L /= 2;
        else if ((n_cur /= 2) == 1) coalesced = true;
    }
};

struct cozk_toggle {
    cozk_ctx* ctx;
    int mode;
    ToggleShape s;
    fe* fp0[2];          // unbound fingerprints [component] (owned)
    uint8_t* fl0;        // unbound flags, packed 0/1 bytes, (batch / 2) x n0 (owned): 32x less traffic than field elements
                         // for the layer output, the first round and the first bind
    fe* fp[2][2];        // ping-pong bound fingerprints [which][component]
    fe* fl[2];           // ping-pong bound flags
    size_t fp_cap[2], fl_cap[2];
};

static const fe* tg_fp(const cozk_toggle* t, int c) { return t->s.cur < 0 ? t->fp0[c] : t->fp[t->s.cur][c]; }  // null for c = 1 of a plain layer
// the flags the kernels read: the packed bytes while unbound (FT = 0), field elements after (FT = 1)
static const void* tg_fl(const cozk_toggle* t) { return t->s.cur < 0 ? (const void*)t->fl0 : (const void*)t->fl[t->s.cur]; }

// flags arrive as 0/1 bytes, one column of n0 entries per PAIR of circuits (the read and the write circuit of a memory
// share their flags: sparse_grand_product.rs:84 `flag_indices[batch_index / 2]`); they are packed into one array
__global__ void __launch_bounds__(PT) k_toggle_flags_pack(const uint8_t* const* __restrict__ cols, size_t n, size_t total, uint8_t* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i >= total) return;
    size_t c = i / n, k = i - c * n;
    out[i] = cols[c][k] ? 1 : 0;
}

// layer_output of the toggle layer (sparse_grand_product.rs:76-97) as a dense interleaved layer: entry b * n + i is the
// fingerprint where the flag is set and a share of one elsewhere (the "missing" entries of the sparse layer)
template <int NC>
__global__ void __launch_bounds__(PT) k_toggle_output(const fe* __restrict__ pa, const fe* __restrict__ pb, const uint8_t* __restrict__ fl, int log_n,
                                                   size_t total, fe one_a, fe one_b, fe* __restrict__ oa, fe* __restrict__ ob) {
    size_t idx = (size_t)blockIdx.x * PT + threadIdx.x;
    if (idx >= total) return;
    size_t b = idx >> log_n, i = idx & (((size_t)1 << log_n) - 1);
    bool on = fl[((b >> 1) << log_n) + i] != 0;
    fe_store(oa + idx, on ? fe_load(pa + idx) : one_a);
    if (NC == 2) fe_store(ob + idx, on ? fe_load(pb + idx) : one_b);
}

// a flag pair as field elements: FT = 0 packed 0/1 bytes (unbound), FT = 1 field elements
template <int FT>
static __device__ __forceinline__ bool toggle_flag_pair(const void* __restrict__ fl, size_t fj, fe& f0, fe& f1) {
    if (FT == 0) {
        const uint8_t* p = (const uint8_t*)fl;
        uint16_t v = *(const uint16_t*)(p + 2 * fj);  // 2 fj is even: aligned
        if (v == 0) return false;
        f0 = (v & 0xff) ? Fr::one() : Fr::zero();
        f1 = (v >> 8) ? Fr::one() : Fr::zero();
        return true;
    }
    const fe* p = (const fe*)fl;
    f0 = fe_load(p + 2 * fj);
    f1 = fe_load(p + 2 * fj + 1);
    return !(Fr::is_zero(f0) && Fr::is_zero(f1));
}

// bind (sparse_grand_product.rs:153-290): pairs (2i, 2i+1) of the fingerprints and of the flags, LowToHigh
template <int NC, int FT>
__global__ void __launch_bounds__(PT) k_toggle_bind(const fe* __restrict__ ia, const fe* __restrict__ ib, fe* __restrict__ oa, fe* __restrict__ ob,
                                                 size_t n_fp, const void* __restrict__ fin, fe* __restrict__ fout, size_t n_fl, fe r) {
    size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    if (i < n_fp) sh_store<NC>(oa, ob, i, sh_lerp<NC>(sh_load<NC>(ia, ib, 2 * i), sh_load<NC>(ia, ib, 2 * i + 1), r));
    if (i < n_fl) {
        fe lo, hi;
        if (toggle_flag_pair<FT>(fin, i, lo, hi)) fe_store(fout + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
        else fe_store(fout + i, Fr::zero());
    }
}

// coalesce (sparse_grand_product.rs:104-134): one flag and one fingerprint per circuit, padded to a power of two with
// ones (flags) and zeros (fingerprints)
template <int NC>
__global__ void __launch_bounds__(PT) k_toggle_coalesce(const fe* __restrict__ pa, const fe* __restrict__ pb, const fe* __restrict__ fl, size_t batch, size_t L,
                                                     fe* __restrict__ oa, fe* __restrict__ ob, fe* __restrict__ ofl) {
    size_t c = (size_t)blockIdx.x * PT + threadIdx.x;
    if (c >= L) return;
    bool in = c < batch;
    fe_store(ofl + c, in ? fe_load(fl + (c >> 1)) : Fr::one());
    fe_store(oa + c, in ? fe_load(pa + c) : Fr::zero());
    if (NC == 2) fe_store(ob + c, in ? fe_load(pb + c) : Fr::zero());
}

// Cubic round sums of sum_x eq(x) * (flag(x) * fingerprint(x) + 1 - flag(x))  (compute_cubic, sparse_grand_product.rs:311-823)
// in the reference's own DELTA form (:455-490): sum_all eq(X)  [k_toggle_eq_sums: closed form over the split-eq tables]
// plus, for the pairs whose flags are not both zero, A(X) = eq * flag * (a + b of the fingerprint) and C(X) = eq * flag:
//     g(X) = A(X) * TWO_INV (into_additive) + [party 0] (S_all(X) - C(X))                      X = 0, 2, 3.
// A lane only LOOKS at its pair's flags (2 bytes in the first round); pairs with a set flag are compacted per wave
// through an LDS queue so that the expensive part -- the eq weights, the 128-byte fingerprint loads and 15 field products
// -- runs with all 64 lanes busy: with Jolt's ~10 % flag density ~19 % of the pairs are active in the first round, and
// without the queue every wave would pay the full path for its few active lanes.
// log_half_n = log2(pairs per circuit) selects the flag pair of circuit b >> 1; log_half_n < 0: coalesced vectors.

// the flag pair of pair j: circuits 2q and 2q + 1 share the flags of memory q
static __device__ __forceinline__ size_t toggle_flag_index(size_t j, int log_half_n) {
    if (log_half_n < 0) return j;
    const size_t b = j >> log_half_n, i = j & (((size_t)1 << log_half_n) - 1);
    return ((b >> 1) << log_half_n) + i;
}
// the look: is one of the pair's two flags set?  Packed bytes: one 16-bit load and no field elements
template <int FT>
static __device__ __forceinline__ bool toggle_pair_active(const void* __restrict__ fl, size_t fj) {
    if (FT == 0) return *(const uint16_t*)((const uint8_t*)fl + 2 * fj) != 0;
    fe f0, f1;
    return toggle_flag_pair<FT>(fl, fj, f0, f1);
}

// The wave queue, the ONE copy of the compaction: every wave walks its pairs in a grid-stride loop, look(j) says whether pair j is
// active, the active pairs' offsets from the wave's first pair are enqueued by ballot (wave_queue_push), and whenever 64 are waiting
// the wave runs heavy(j) on them with full lanes and carries the rest to the front (wave_queue_pop); what is left when the pairs run
// out is flushed the same way.  `queue` is this wave's 128 entries, qn (wave-uniform) how many wait.  A wave's LDS operations
// execute in program order; the wave barriers keep the compiler from moving them.

// enqueue: the lanes with `active` append their pair's offset, in lane order
static __device__ __forceinline__ void wave_queue_push(uint32_t* queue, int& qn, int lane, bool active, uint32_t off) {
    const unsigned long long m = __ballot(active);
    if (active) queue[qn + __popcll(m & ((1ull << lane) - 1ull))] = off;
    qn += __popcll(m);
    __builtin_amdgcn_wave_barrier();
}
// the first `take` entries are done: carry the rest (fewer than 64) to the front
static __device__ __forceinline__ void wave_queue_pop(uint32_t* queue, int& qn, int lane, int take) {
    const uint32_t keep = lane < qn - take ? queue[take + lane] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (lane < qn - take) queue[lane] = keep;
    __builtin_amdgcn_wave_barrier();
    qn -= take;
}
// The two loop shapes over those steps.  TWO call sites of heavy, a full flush inside the loop and the remainder behind it, with
// pre_flush() (wave-uniform; k_toggle_cubic9's periodic fold) in front of either: the single-layer kernels.  In the one-call-site
// shape below their register allocation moves (VGPRs here -> there: k_toggle_cubic<1, 1, 0> 91 -> 98, occupancy 5 -> 4; <1, 0, 0>
// 76 -> 90, occupancy 6 -> 5; <1, 1, 1> 86 -> 74; k_toggle_cubic9<2, 1, 0> 189 -> 178; <1, 1, 1> 165 -> 157).
template <class Look, class Heavy, class PreFlush>
static __device__ __forceinline__ void toggle_wave_queue(uint32_t* queue, size_t npairs, Look look, Heavy heavy, PreFlush pre_flush) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int qn = 0;  // wave-uniform
    const size_t stride = (size_t)gridDim.x * PT;
    const size_t wave_base0 = (size_t)blockIdx.x * PT + (size_t)wv * 64;
    for (size_t jb = wave_base0; jb < npairs; jb += stride) {  // wave-uniform trip count
        const size_t j = jb + lane;
        bool active = false;
        if (j < npairs) active = look(j);
        wave_queue_push(queue, qn, lane, active, (uint32_t)(j - wave_base0));
        if (qn >= 64) {
            pre_flush();
            heavy(wave_base0 + (size_t)queue[lane]);
            wave_queue_pop(queue, qn, lane, 64);
        }
    }
    if (qn > 0) pre_flush();
    if (lane < qn) heavy(wave_base0 + (size_t)queue[lane]);
}
// ONE call site of heavy, so that it is inlined and the caller's accumulators stay in registers: k_toggle_group_cubic, with 15 of
// them.  The loop goes on, looking at no further pairs, until the queue is empty.
template <class Look, class Heavy>
static __device__ __forceinline__ void toggle_wave_queue_one_site(uint32_t* queue, size_t npairs, Look look, Heavy heavy) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int qn = 0;  // wave-uniform
    const size_t stride = (size_t)gridDim.x * PT;
    const size_t wave_base0 = (size_t)blockIdx.x * PT + (size_t)wv * 64;
    for (size_t jb = wave_base0;; jb += stride) {  // wave-uniform trip count
        const bool more = jb < npairs;
        if (more) {
            const size_t j = jb + lane;
            bool active = false;
            if (j < npairs) active = look(j);
            wave_queue_push(queue, qn, lane, active, (uint32_t)(j - wave_base0));
        }
        if (qn >= 64 || (!more && qn > 0)) {
            const int take = qn < 64 ? qn : 64;
            if (lane < take) heavy(wave_base0 + (size_t)queue[lane]);
            wave_queue_pop(queue, qn, lane, take);
        }
        if (!more && qn == 0) break;
    }
}

template <int NC, int NESTED, int FT>
__global__ void __launch_bounds__(PT) k_toggle_cubic(const fe* __restrict__ pa, const fe* __restrict__ pb, const void* __restrict__ fl, size_t npairs,
                                                  int log_half_n, const fe* __restrict__ E1, int log_E1_half, const fe* __restrict__ E2, size_t E2_len,
                                                  fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ uint32_t queue[PT / 64][128];
    const size_t limit = split_eq_limit<NESTED>(E2_len, log_E1_half);
    if (npairs > limit) npairs = limit;
    fe A[3], C[3];
    for (int k = 0; k < 3; k++) A[k] = C[k] = Fr::zero();
    auto heavy = [&](size_t j) {
        // split_eq_at and the E2 factor, written out: with the helper k_toggle_cubic<1, 0, 1> takes 73 VGPRs for 74
        fe e[3];
        if (NESTED) {
            size_t x2 = j >> log_E1_half, x1 = j & (((size_t)1 << log_E1_half) - 1);
            eq3(fe_load(E1 + 2 * x1), fe_load(E1 + 2 * x1 + 1), e);
            fe sc = fe_load(E2 + x2);
            for (int k = 0; k < 3; k++) e[k] = Fr::mul(e[k], sc);
        } else {
            eq3(fe_load(E2 + 2 * j), fe_load(E2 + 2 * j + 1), e);
        }
        fe f0, f1;
        (void)toggle_flag_pair<FT>(fl, toggle_flag_index(j, log_half_n), f0, f1);
        fe p0 = sh_ab_sum<NC>(sh_load<NC>(pa, pb, 2 * j)), p1 = sh_ab_sum<NC>(sh_load<NC>(pa, pb, 2 * j + 1));
        fe f[3], p[3];
        eq3(f0, f1, f);
        eq3(p0, p1, p);
        for (int k = 0; k < 3; k++) {
            fe fe_k = Fr::mul(f[k], e[k]);
            C[k] = Fr::add(C[k], fe_k);
            A[k] = Fr::add(A[k], Fr::mul(fe_k, p[k]));
        }
    };
    toggle_wave_queue(queue[threadIdx.x >> 6], npairs, [&](size_t j) { return toggle_pair_active<FT>(fl, toggle_flag_index(j, log_half_n)); }, heavy, [] {});
    for (int k = 0; k < 3; k++) {  // partial_row_sum, written out: with the helper <1, 1, 0> takes 88 VGPRs for 91 and <2, 1, 0> 110 for 112
        fe v = fr_block_sum(A[k], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)k * gridDim.x + blockIdx.x, v);
        v = fr_block_sum(C[k], sh4);
        if (threadIdx.x == 0) fe_store(partial + (size_t)(3 + k) * gridDim.x + blockIdx.x, v);
    }
}

// X = 0, 2, 3 of the line through (v0, v1) on the 9 x 29 multiplier, lazily: normalised v0, v1 in, limbs < 2^30.6 out; CS = FR9_C2 for
// canonical v0, FR9_C3 for a Rep3 sum a + b (< 2 r: its top limb can be one above FR9_C2's)
static __device__ __forceinline__ void f9_line3(const f9& v0, const f9& v1, const uint32_t (&CS)[9], f9& x0, f9& x2, f9& x3) {
    const f9 m = f9_norm(f9_sub(v1, CS, v0));
    x0 = v0;
    x2 = fr9_add(v1, m);
    x3 = fr9_add(x2, m);
}
// split_eq_at on the 9 x 29 multiplier with the E2 factor multiplied in: normalised weights, which carry lambda when nested (the E2 product) and none when flat
template <int NESTED>
static __device__ __forceinline__ void split_eq_weights9(const fe* E1, int log_E1_half, const fe* E2, size_t j, f9& e0, f9& e2, f9& e3) {
    f9 r0, r2, r3;
    if (NESTED) {
        const size_t x2i = j >> log_E1_half, x1 = j & (((size_t)1 << log_E1_half) - 1);
        f9_line3(f9_from_fe(fe_load(E1 + 2 * x1)), f9_from_fe(fe_load(E1 + 2 * x1 + 1)), FR9_C2, r0, r2, r3);
        const f9 sc = f9_from_fe(fe_load(E2 + x2i));
        e0 = fr9_mul(r0, sc);
        e2 = fr9_mul(r2, sc);
        e3 = fr9_mul(r3, sc);
    } else {
        f9_line3(f9_from_fe(fe_load(E2 + 2 * j)), f9_from_fe(fe_load(E2 + 2 * j + 1)), FR9_C2, r0, r2, r3);
        e0 = r0;
        e2 = f9_norm(r2);
        e3 = f9_norm(r3);
    }
}

template <int NC, int NESTED, int FT>
__global__ void __launch_bounds__(PT) k_toggle_cubic9(const fe* __restrict__ pa, const fe* __restrict__ pb, const void* __restrict__ fl, size_t npairs,
                                                  int log_half_n, const fe* __restrict__ E1, int log_E1_half, const fe* __restrict__ E2, size_t E2_len,
                                                  fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ uint32_t queue[PT / 64][128];
    const size_t limit = split_eq_limit<NESTED>(E2_len, log_E1_half);
    if (npairs > limit) npairs = limit;
    // the heavy path on the 9 x 29 multiplier (fr9.hip.hpp): C(X) = eq x flag carries lambda (lambda^2 with the E2 factor), A(X) =
    // C(X) x fingerprint one more; sums are lazy, one product with the matching constant per lane at the end
    f9 A0 = fr9_zero(), A2 = fr9_zero(), A3 = fr9_zero(), C0 = fr9_zero(), C2 = fr9_zero(), C3 = fr9_zero();
    auto heavy = [&](size_t j) {
        f9 e0, e2, e3;
        split_eq_weights9<NESTED>(E1, log_E1_half, E2, j, e0, e2, e3);
        fe f0, f1;
        (void)toggle_flag_pair<FT>(fl, toggle_flag_index(j, log_half_n), f0, f1);
        f9 g0, g2, g3, p0, p2, p3;
        f9_line3(f9_from_fe(f0), f9_from_fe(f1), FR9_C2, g0, g2, g3);
        {
            const Sh9<NC> q0 = sh9_load_or_zero<NC>(pa, pb, 2 * j, (size_t)-1), q1 = sh9_load_or_zero<NC>(pa, pb, 2 * j + 1, (size_t)-1);
            // (a + b) of a Rep3 fingerprint: < 2 r, limbs < 2^30 -- normalised for f9_line3
            const f9 s0 = NC == 2 ? f9_norm(fr9_add(q0.c[0], q0.c[NC - 1])) : q0.c[0];
            const f9 s1 = NC == 2 ? f9_norm(fr9_add(q1.c[0], q1.c[NC - 1])) : q1.c[0];
            f9_line3(s0, s1, NC == 2 ? FR9_C3 : FR9_C2, p0, p2, p3);
        }
        const f9 c0 = fr9_mul(g0, e0), c2 = fr9_mul(g2, e2), c3 = fr9_mul(g3, e3);  // flag x eq: normalised outputs
        C0 = f9_norm(fr9_add(C0, c0));
        C2 = f9_norm(fr9_add(C2, c2));
        C3 = f9_norm(fr9_add(C3, c3));
        A0 = f9_norm(fr9_add(A0, fr9_mul(p0, c0)));
        A2 = f9_norm(fr9_add(A2, fr9_mul(p2, c2)));
        A3 = f9_norm(fr9_add(A3, fr9_mul(p3, c3)));
    };
    // the periodic fold of the lazy sums (fr9.hip.hpp): a lane takes at most one heavy() per flush of the wave's queue
    unsigned nflush = 0;  // wave-uniform
    auto fold = [&]() {
        if (nflush != 0 && (nflush & (FR9_FOLD_PERIOD - 1)) == 0) {
            fr9_fold(A0);
            fr9_fold(A2);
            fr9_fold(A3);
            fr9_fold(C0);
            fr9_fold(C2);
            fr9_fold(C3);
        }
        nflush++;
    };
    toggle_wave_queue(queue[threadIdx.x >> 6], npairs, [&](size_t j) { return toggle_pair_active<FT>(fl, toggle_flag_index(j, log_half_n)); }, heavy, fold);
    {
        // C carries lambda (lambda^2 nested), A one more
        const f9 KC = NESTED ? f9_const(FR9_K2) : f9_const(FR9_K1), KA = NESTED ? f9_const(FR9_K3) : f9_const(FR9_K2);
        const f9* As[3] = {&A0, &A2, &A3};
        const f9* Cs[3] = {&C0, &C2, &C3};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            partial_row_sum(fr9_to_canonical(fr9_mul(*As[k], KA)), sh4, partial, k);
            partial_row_sum(fr9_to_canonical(fr9_mul(*Cs[k], KC)), sh4, partial, 3 + k);
        }
    }
}

// S_all(X) = sum_{j < npairs} eq_j(X), X = 0, 2, 3 -- "the cubic evals assuming all the coefficients are ones"
// (sparse_grand_product.rs:455-470 eq_eval_sums; :735-790 with the E2 prefix for layers that are not a power of two):
//   nested:  sum_{x2 < nfull} E2[x2] * S1 + E2[nfull] * S1_partial,  S1 = sum over the E1 pairs, nfull = npairs >> log E1_half
//   else:    sum over the first npairs pairs of E2
// One workgroup: the tables are the two halves of a split-eq (<= 2^14 entries).
template <int NESTED>
__global__ void __launch_bounds__(RT) k_toggle_eq_sums(const fe* __restrict__ E1, int log_E1_half, const fe* __restrict__ E2, size_t E2_len, size_t npairs,
                                                    fe* __restrict__ out) {
    __shared__ fe sh16[16];
    const size_t limit = split_eq_limit<NESTED>(E2_len, log_E1_half);
    if (npairs > limit) npairs = limit;
    fe s[3], sp[3];
    for (int k = 0; k < 3; k++) s[k] = sp[k] = Fr::zero();
    if (NESTED) {
        const size_t E1_half = (size_t)1 << log_E1_half;
        const size_t nfull = npairs >> log_E1_half, rem = npairs & (E1_half - 1);
        for (size_t x1 = threadIdx.x; x1 < E1_half; x1 += RT) {
            fe e[3];
            eq3(fe_load(E1 + 2 * x1), fe_load(E1 + 2 * x1 + 1), e);
            for (int k = 0; k < 3; k++) {
                s[k] = Fr::add(s[k], e[k]);
                if (x1 < rem) sp[k] = Fr::add(sp[k], e[k]);
            }
        }
        fe e2 = Fr::zero();
        for (size_t x2 = threadIdx.x; x2 < nfull; x2 += RT) e2 = Fr::add(e2, fe_load(E2 + x2));
        fe S1[3], S1p[3];
        for (int k = 0; k < 3; k++) {
            S1[k] = fr_block_sum(s[k], sh16);
            S1p[k] = fr_block_sum(sp[k], sh16);
        }
        fe E2s = fr_block_sum(e2, sh16);
        if (threadIdx.x == 0) {
            fe last = rem ? fe_load(E2 + nfull) : Fr::zero();
            for (int k = 0; k < 3; k++) fe_store(out + k, Fr::add(Fr::mul(E2s, S1[k]), Fr::mul(last, S1p[k])));
        }
    } else {
        for (size_t j = threadIdx.x; j < npairs; j += RT) {
            fe e[3];
            eq3(fe_load(E2 + 2 * j), fe_load(E2 + 2 * j + 1), e);
            for (int k = 0; k < 3; k++) s[k] = Fr::add(s[k], e[k]);
        }
        for (int k = 0; k < 3; k++) {
            fe v = fr_block_sum(s[k], sh16);
            if (threadIdx.x == 0) fe_store(out + k, v);
        }
    }
}

// ------------------------------------------------------------------ toggle groups (cozk_toggle_group_*)
// ONE PLAIN toggle layer with k fingerprint planes over ONE copy of the public flags: the senders of a Shamir prover
// (csrc/host/shamir_gp.hpp).  The flags are public and the toggle layer's output and round polynomial are affine in the
// fingerprints, so everything but the fingerprint loads and the products A_m(X) = sum eq * flag * fp_m is the same for every
// member: the flag look, the compaction, the eq weights, the flag interpolation, C(X) and S_all(X) are done once.  The planes'
// pointers travel in the kernel arguments as LayerGroupArgs' do (one table of COZK_LAYER_GROUP_MAX pointers, indexed by
// wave-uniform values: scalar loads, nothing staged).
struct ToggleGroupIn {
    const fe* p[COZK_LAYER_GROUP_MAX];
};
struct ToggleGroupOut {
    fe* p[COZK_LAYER_GROUP_MAX];
};

// k_toggle_output (PLAIN, one = 1) for every member: the flag byte is read once per element
__global__ void __launch_bounds__(PT) k_toggle_group_output(ToggleGroupIn in, ToggleGroupOut out, const uint8_t* __restrict__ fl, int log_n, size_t total, int k) {
    size_t idx = (size_t)blockIdx.x * PT + threadIdx.x;
    if (idx >= total) return;
    size_t b = idx >> log_n, i = idx & (((size_t)1 << log_n) - 1);
    const bool on = fl[((b >> 1) << log_n) + i] != 0;
    const fe one = Fr::one();
    for (int m = 0; m < k; m++) fe_store(out.p[m] + idx, on ? fe_load(in.p[m] + idx) : one);
}

// k_toggle_bind for the k planes (blockIdx.y = member) and, by the workgroups of member 0, the one flag array.  CO = 1: the bind
// that leaves one entry per circuit writes the coalesced vectors of k_toggle_coalesce directly -- n_fp = n_fl = L entries, circuit
// c's flag the bound flag pair c >> 1, padded with ones (flags) and zeros (fingerprints) from `batch` upwards.
template <int FT, int CO>
__global__ void __launch_bounds__(PT) k_toggle_group_bind(ToggleGroupIn in, fe* __restrict__ out, size_t out_stride, size_t n_fp, const void* __restrict__ fin,
                                                       fe* __restrict__ fout, size_t n_fl, size_t batch, fe r) {
    const size_t i = (size_t)blockIdx.x * PT + threadIdx.x;
    const unsigned m = blockIdx.y;
    const fe* ia = in.p[m];
    fe* oa = out + (size_t)m * out_stride;
    if (CO) {
        if (i >= n_fp) return;
        const bool inb = i < batch;
        if (inb) sh_store<1>(oa, nullptr, i, sh_lerp<1>(sh_load<1>(ia, nullptr, 2 * i), sh_load<1>(ia, nullptr, 2 * i + 1), r));
        else fe_store(oa + i, Fr::zero());
        if (m == 0) {
            fe lo, hi, v = Fr::one();
            if (inb) v = toggle_flag_pair<FT>(fin, i >> 1, lo, hi) ? Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)) : Fr::zero();
            fe_store(fout + i, v);
        }
        return;
    }
    if (i < n_fp) sh_store<1>(oa, nullptr, i, sh_lerp<1>(sh_load<1>(ia, nullptr, 2 * i), sh_load<1>(ia, nullptr, 2 * i + 1), r));
    if (m == 0 && i < n_fl) {
        fe lo, hi;
        if (toggle_flag_pair<FT>(fin, i, lo, hi)) fe_store(fout + i, Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r)));
        else fe_store(fout + i, Fr::zero());
    }
}

// k_toggle_cubic (PLAIN, Montgomery path) for the members of one chunk: blockIdx.y selects members TOGGLE_GROUP_CHUNK y ..
// TOGGLE_GROUP_CHUNK (y + 1) - 1 -- 31 members' accumulators (3 field elements each) do not fit a lane, a chunk's do.  The flag look, the
// per-wave compaction and, per active pair, the eq weights, the flag interpolation and flag x eq are computed once per chunk; the
// member loop does the two fingerprint loads, eq3 and three multiply-adds.  C(X) is accumulated by chunk 0 only.
// partial rows: 3 m + X' for A_m (X' = 0, 1, 2 for X = 0, 2, 3), 3 k + X' for C.
static constexpr int TOGGLE_GROUP_CHUNK = 4;
template <int NESTED, int FT>
__global__ void __launch_bounds__(PT) k_toggle_group_cubic(ToggleGroupIn in, int k, const void* __restrict__ fl, size_t npairs, int log_half_n,
                                                        const fe* __restrict__ E1, int log_E1_half, const fe* __restrict__ E2, size_t E2_len,
                                                        fe* __restrict__ partial) {
    __shared__ fe sh4[4];
    __shared__ uint32_t queue[PT / 64][128];
    const int m0 = (int)blockIdx.y * TOGGLE_GROUP_CHUNK;
    const int nm = k - m0 < TOGGLE_GROUP_CHUNK ? k - m0 : TOGGLE_GROUP_CHUNK;  // workgroup-uniform
    const bool first = blockIdx.y == 0;
    const size_t limit = split_eq_limit<NESTED>(E2_len, log_E1_half);
    if (npairs > limit) npairs = limit;
    fe A[TOGGLE_GROUP_CHUNK][3], C[3];
#pragma unroll
    for (int w = 0; w < TOGGLE_GROUP_CHUNK; w++)
#pragma unroll
        for (int x = 0; x < 3; x++) A[w][x] = Fr::zero();
#pragma unroll
    for (int x = 0; x < 3; x++) C[x] = Fr::zero();
    auto heavy = [&](size_t j) __attribute__((always_inline)) {
        fe e[3], sc;
        split_eq_at(NESTED, E1, log_E1_half, E2, j, e, sc);
        if (NESTED) {
#pragma unroll
            for (int x = 0; x < 3; x++) e[x] = Fr::mul(e[x], sc);
        }
        fe f0, f1, f[3];
        (void)toggle_flag_pair<FT>(fl, toggle_flag_index(j, log_half_n), f0, f1);
        eq3(f0, f1, f);
#pragma unroll
        for (int x = 0; x < 3; x++) e[x] = Fr::mul(f[x], e[x]);  // flag x eq, once for all members
        if (first) {
#pragma unroll
            for (int x = 0; x < 3; x++) C[x] = Fr::add(C[x], e[x]);
        }
#pragma unroll
        for (int w = 0; w < TOGGLE_GROUP_CHUNK; w++) {
            if (w < nm) {
                const fe* pa = in.p[m0 + w];
                fe p[3];
                eq3(fe_load(pa + 2 * j), fe_load(pa + 2 * j + 1), p);
#pragma unroll
                for (int x = 0; x < 3; x++) A[w][x] = Fr::add(A[w][x], Fr::mul(e[x], p[x]));
            }
        }
    };
    toggle_wave_queue_one_site(queue[threadIdx.x >> 6], npairs, [&](size_t j) { return toggle_pair_active<FT>(fl, toggle_flag_index(j, log_half_n)); }, heavy);
#pragma unroll
    for (int w = 0; w < TOGGLE_GROUP_CHUNK; w++) {
        if (w < nm) {
#pragma unroll
            for (int x = 0; x < 3; x++) partial_row_sum(A[w][x], sh4, partial, 3 * (m0 + w) + x);
        }
    }
    if (first) {
#pragma unroll
        for (int x = 0; x < 3; x++) partial_row_sum(C[x], sh4, partial, 3 * k + x);
    }
}

// the final claims of a fully bound layer or group into the pinned result slot: res[0] = the flag, res[1 + m] = plane m's fingerprint
__global__ void __launch_bounds__(64) k_toggle_group_claims(ToggleGroupIn in, const fe* __restrict__ fl, int k_final, fe* __restrict__ res) {
    if (threadIdx.x != 0) return;  // one lane: the table is indexed by a uniform value
    fe_store(res, fe_load(fl));
    for (int m = 0; m < k_final; m++) fe_store(res + 1 + m, fe_load(in.p[m]));
}
// ... and to the host: h[0 .. k_final]
static void toggle_claims_fetch(cozk_ctx* ctx, const ToggleGroupIn& in, const fe* fl, int k_final, fe* h) {
    fe* res = result_slot(ctx, (size_t)k_final + 1);
    k_toggle_group_claims<<<1, 64, 0, ctx->stream>>>(in, fl, k_final, res);
    HIP_TRY(hipGetLastError());
    fetch_fe(ctx, res, (size_t)k_final + 1, h);
}

static void toggle_reserve(cozk_toggle* t, int w, size_t n_fp, size_t n_fl) {
    if (t->fp_cap[w] < n_fp) {
        for (int c = 0; c < 2; c++) {
            if (t->fp[w][c]) ctx_dev_free(t->ctx, t->fp[w][c]);
            t->fp[w][c] = nullptr;
        }
        t->fp[w][0] = dev_alloc_fe(n_fp);
        if (t->mode == COZK_MODE_REP3) t->fp[w][1] = dev_alloc_fe(n_fp);
        t->fp_cap[w] = n_fp;
    }
    if (t->fl_cap[w] < n_fl) {
        if (t->fl[w]) ctx_dev_free(t->ctx, t->fl[w]);
        t->fl[w] = dev_alloc_fe(n_fl);
        t->fl_cap[w] = n_fl;
    }
}

// the flag columns of a create, checked and packed into one array of n_pairs x n0 bytes from ctx's pool (*fl0, set as soon as it
// exists so that the caller's clean-up finds it); `who` prefixes the messages
static void toggle_pack_flags(cozk_ctx* ctx, const cozk_vec* const* flags, size_t n_pairs, size_t n0, const char* who, uint8_t** fl0) {
    std::vector<const uint8_t*> cols(n_pairs);
    for (size_t q = 0; q < n_pairs; q++) {
        if (!(flags[q] && flags[q]->ctx && flags[q]->kind == COZK_SCALAR_U8 && flags[q]->n == n0))
            throw CozkError(COZK_ERR_INVALID_ARG, std::string(who) + ": every flag column is a U8 vector of N entries");
        cols[q] = (const uint8_t*)flags[q]->d;
    }
    *fl0 = (uint8_t*)ctx_dev_alloc(ctx, n_pairs * n0 + 16);
    ctx->scratch2.reserve(n_pairs * sizeof(void*));
    HIP_TRY(hipMemcpyAsync(ctx->scratch2.p, cols.data(), n_pairs * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // `cols` lives on the stack of this call
    k_toggle_flags_pack<<<grid_for(n_pairs * n0), PT, 0, ctx->stream>>>((const uint8_t* const*)ctx->scratch2.p, n0, n_pairs * n0, *fl0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // scratch2 is shared with other calls
}

// the view of a split-eq polynomial that the round kernels take: nested = E1 is not yet a single value (lg1 = log2 of its pairs)
struct EqView {
    bool nested;
    const fe* E1;
    const fe* E2;
    int lg1;
    size_t E2_len;
};
static EqView eq_view(const cozk_spliteq* e) {
    const bool nested = e->E1_len != 1;
    return EqView{nested, e->E1[e->c1], e->E2[e->c2], nested ? log2_sz(e->E1_len / 2) : 0, e->E2_len};
}
// S_all(X) over the first n items into dst[0 .. 2]: the sums as if every node were one (the reference's eq_eval_sums /
// evals_assuming_all_ones); in a round it goes before the finishing kernel, which publishes the round
static void eq_sums_launch(cozk_ctx* ctx, const EqView& v, size_t n, fe* dst) {
    auto* const kernel = v.nested ? k_toggle_eq_sums<1> : k_toggle_eq_sums<0>;
    kernel<<<1, RT, 0, ctx->stream>>>(v.E1, v.lg1, v.E2, v.E2_len, n, dst);
    HIP_TRY(hipGetLastError());
}

// Rep3Bindable::bind (sparse_grand_product.rs:153-290) incl. the switch to the coalesced vectors when layer_len reaches 2 (a second
// launch; the group fuses it).  The caller has checked !t->s.bound().
static void toggle_bind_launch(cozk_toggle* t, const fe& rr) {
    cozk_ctx* const ctx = t->ctx;
    const ToggleShape::BindSizes b = t->s.bind_sizes();
    const int dst = t->s.dst();
    const bool rep3 = t->mode == COZK_MODE_REP3, u8 = t->s.cur < 0;  // the first bind reads the packed 0/1 bytes
    toggle_reserve(t, dst, b.n_fp, b.n_fl);
    auto* const kernel = rep3 ? (u8 ? k_toggle_bind<2, 0> : k_toggle_bind<2, 1>) : (u8 ? k_toggle_bind<1, 0> : k_toggle_bind<1, 1>);
    kernel<<<grid_for(b.n_fp), PT, 0, ctx->stream>>>(tg_fp(t, 0), tg_fp(t, 1), t->fp[dst][0], t->fp[dst][1], b.n_fp, tg_fl(t), t->fl[dst], b.n_fl, rr);
    HIP_TRY(hipGetLastError());
    t->s.advance();
    if (b.coalesces) {  // layer_len == 2: coalesce, to the other side
        const size_t L = t->s.L;
        const int d2 = 1 - t->s.cur;
        toggle_reserve(t, d2, L, L);
        auto* const coalesce = rep3 ? k_toggle_coalesce<2> : k_toggle_coalesce<1>;
        coalesce<<<grid_for(L), PT, 0, ctx->stream>>>(tg_fp(t, 0), tg_fp(t, 1), t->fl[t->s.cur], t->s.batch, L, t->fp[d2][0], t->fp[d2][1], t->fl[d2]);
        HIP_TRY(hipGetLastError());
        t->s.cur = d2;
    }
}

extern "C" {

int cozk_toggle_create(cozk_ctx* ctx, int mode, const cozk_vec* const* flags, size_t n_pairs, cozk_vec* fp_a, cozk_vec* fp_b, int take_ownership,
                       cozk_toggle** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && flags && n_pairs > 0 && fp_a && out && (mode == COZK_MODE_PLAIN || mode == COZK_MODE_REP3), "toggle_create: bad argument");
        COZK_REQUIRE(fp_a->kind == COZK_SCALAR_FR && (mode == COZK_MODE_PLAIN || (fp_b && fp_b->kind == COZK_SCALAR_FR && fp_b->n == fp_a->n)),
                     "toggle_create: fingerprints must be FR vectors (a and b for Rep3)");
        const size_t batch = 2 * n_pairs;
        COZK_REQUIRE(fp_a->n % batch == 0, "toggle_create: fingerprints.len() must be 2 * n_pairs * N");
        const size_t n0 = fp_a->n / batch;
        COZK_REQUIRE(n0 >= 2 && (n0 & (n0 - 1)) == 0, "toggle_create: fingerprints per circuit must be a power of two >= 2");
        cozk_toggle* t = new cozk_toggle();  // value-initialised: no buffers yet
        struct Guard {
            cozk_toggle* t;
            ~Guard() { if (t) cozk_toggle_free(t); }
        } guard{t};
        t->ctx = ctx;
        t->mode = mode;
        t->s.init(batch, n0);
        toggle_pack_flags(ctx, flags, n_pairs, n0, "toggle_create", &t->fl0);
        cozk_vec* src[2] = {fp_a, mode == COZK_MODE_REP3 ? fp_b : nullptr};
        for (int c = 0; c < 2; c++) {
            if (!src[c]) continue;
            if (take_ownership && src[c]->owned) {
                t->fp0[c] = (fe*)vec_adopt(src[c]);
            } else {
                t->fp0[c] = dev_alloc_fe(batch * n0);
                HIP_TRY(hipMemcpyAsync(t->fp0[c], src[c]->d, batch * n0 * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        guard.t = nullptr;
        *out = t;
    });
}

int cozk_toggle_free(cozk_toggle* t) {
    if (!t) return COZK_OK;
    for (int c = 0; c < 2; c++)
        if (t->fp0[c]) ctx_dev_free(t->ctx, t->fp0[c]);
    if (t->fl0) ctx_dev_free(t->ctx, t->fl0);
    for (int w = 0; w < 2; w++) {
        for (int c = 0; c < 2; c++)
            if (t->fp[w][c]) ctx_dev_free(t->ctx, t->fp[w][c]);
        if (t->fl[w]) ctx_dev_free(t->ctx, t->fl[w]);
    }
    delete t;
    return COZK_OK;
}

size_t cozk_toggle_batch(const cozk_toggle* t) { return t ? t->s.batch : 0; }
size_t cozk_toggle_len(const cozk_toggle* t) { return t ? t->s.n0 : 0; }

// layer_output (sparse_grand_product.rs:76-97) as the dense interleaved layer the sparse layers are kept as
int cozk_toggle_layer_output(cozk_ctx* ctx, const cozk_toggle* t, int party_id, cozk_layer** out) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t && out && t->s.cur < 0 && party_id >= 0 && party_id < 3, "toggle_layer_output: needs an unbound toggle layer");
        const size_t total = t->s.batch * t->s.n0;
        cozk_layer* l = new cozk_layer();
        l->ctx = ctx;
        l->mode = t->mode;
        l->cur = 0;
        l->len = total;
        for (int w = 0; w < 2; w++) {
            l->buf[w][0] = l->buf[w][1] = nullptr;
            l->cap[w] = 0;
        }
        l->buf[0][0] = dev_alloc_fe(total);
        if (t->mode == COZK_MODE_REP3) l->buf[0][1] = dev_alloc_fe(total);
        l->cap[0] = total;
        // promote_to_trivial_share(party_id, one): P0 (1, 0), P1 (0, 1), P2 (0, 0); the plain prover's one is 1
        fe one_a = (t->mode == COZK_MODE_PLAIN || party_id == 0) ? Fr::one() : Fr::zero();
        fe one_b = (t->mode == COZK_MODE_REP3 && party_id == 1) ? Fr::one() : Fr::zero();
        auto* const kernel = t->mode == COZK_MODE_REP3 ? k_toggle_output<2> : k_toggle_output<1>;
        kernel<<<grid_for(total), PT, 0, ctx->stream>>>(t->fp0[0], t->fp0[1], t->fl0, log2_sz(t->s.n0), total, one_a, one_b, l->buf[0][0], l->buf[0][1]);
        HIP_TRY(hipGetLastError());
        *out = l;
    });
}

int cozk_toggle_bind(cozk_ctx* ctx, cozk_toggle* t, const uint64_t r[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t && r, "toggle_bind: bad argument");
        COZK_REQUIRE(!t->s.bound(), "toggle_bind: fully bound");
        toggle_bind_launch(t, fe_from_u64x4(r));
    });
}

// The cubic-sum kernel of a toggle round.  F9: the 9 x 29 kernel, which exists for the throughput-bound rounds only (nested eq tables,
// TOGGLE_F9_MIN_PAIRS pairs or more); COZK_TOGGLE_F9=0: the saturated kernel everywhere.  u8: the flags are still the packed 0/1 bytes.
static constexpr size_t TOGGLE_F9_MIN_PAIRS = 4096;
using ToggleCubicKernel = void (*)(const fe*, const fe*, const void*, size_t, int, const fe*, int, const fe*, size_t, fe*);
static ToggleCubicKernel toggle_cubic_kernel(int mode, bool nested, bool u8, size_t npairs) {
    static const bool f9_env = !(getenv("COZK_TOGGLE_F9") && atoi(getenv("COZK_TOGGLE_F9")) == 0);
    const bool f9 = f9_env && nested && npairs >= TOGGLE_F9_MIN_PAIRS;
    if (mode == COZK_MODE_REP3) {
        if (f9) return u8 ? k_toggle_cubic9<2, 1, 0> : k_toggle_cubic9<2, 1, 1>;
        if (nested) return u8 ? k_toggle_cubic<2, 1, 0> : k_toggle_cubic<2, 1, 1>;
        return u8 ? k_toggle_cubic<2, 0, 0> : k_toggle_cubic<2, 0, 1>;
    }
    if (f9) return u8 ? k_toggle_cubic9<1, 1, 0> : k_toggle_cubic9<1, 1, 1>;
    if (nested) return u8 ? k_toggle_cubic<1, 1, 0> : k_toggle_cubic<1, 1, 1>;
    return u8 ? k_toggle_cubic<1, 0, 0> : k_toggle_cubic<1, 0, 1>;
}

// one round of prove_sumcheck over the toggle layer: bind layer + split-eq tables with the previous challenge (NULL in
// the first round), then the three round sums g(0), g(2), g(3) of compute_cubic as this party's additive shares.  Every check comes
// before the first bind: a refused call leaves the layer and the eq as they were.
int cozk_toggle_round(cozk_ctx* ctx, cozk_toggle* t, cozk_spliteq* e, const uint64_t* r, int party_id, uint64_t out_evals[12]) {
    if (!ctx || !t || !e || !out_evals || party_id < 0 || party_id > 2) return COZK_ERR_INVALID_ARG;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(e->ctx == ctx, "toggle_round: the eq polynomial belongs to another context");
        COZK_REQUIRE(!t->s.bound(), "toggle_round: fully bound");
        if (r) {
            COZK_REQUIRE(!spliteq_bound(e), "toggle_round: eq polynomial already fully bound");
            COZK_REQUIRE(!t->s.last_bind(), "toggle_round: the bind leaves the layer fully bound, with no round to run (cozk_toggle_bind)");
            const fe rr = fe_from_u64x4(r);
            toggle_bind_launch(t, rr);
            spliteq_bind_launch(ctx, e, rr);
        }
        const size_t npairs = t->s.npairs();
        const unsigned gx = sum_grid(grid_capped(npairs, ROUND_GRID_MAX));
        const SumLaunch sl = sum_launch(ctx, 6, gx, 9);
        const EqView v = eq_view(e);
        const ToggleCubicKernel kernel = toggle_cubic_kernel(t->mode, v.nested, t->s.cur < 0, npairs);
        kernel<<<gx, PT, 0, ctx->stream>>>(tg_fp(t, 0), tg_fp(t, 1), tg_fl(t), npairs, t->s.log_half_n(), v.E1, v.lg1, v.E2, v.E2_len, sl.partial);
        eq_sums_launch(ctx, v, npairs, sl.res + 6);
        fe s[9];
        finish_sums(ctx, sl, 6, gx, Fr::one(), 0, s);
        const bool pub = t->mode == COZK_MODE_PLAIN || party_id == 0;  // additive::add_public: party 0 only
        for (int k = 0; k < 3; k++) {
            fe a = t->mode == COZK_MODE_REP3 ? Fr::mul(s[k], fr_two_inv()) : s[k];  // into_additive
            fe_to_u64x4(pub ? Fr::add(a, Fr::sub(s[6 + k], s[3 + k])) : a, out_evals + 4 * k);
        }
    });
}

// final_claims (sparse_grand_product.rs:825-835): the bound flag (a public value) and the bound fingerprint share
int cozk_toggle_final_claims(cozk_ctx* ctx, const cozk_toggle* t, uint64_t flag[4], uint64_t fp_a[4], uint64_t fp_b[4]) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t && flag && fp_a && t->s.bound(), "toggle_final_claims: the layer is not fully bound");
        const int nc = t->mode == COZK_MODE_REP3 ? 2 : 1;
        ToggleGroupIn in;
        memset(&in, 0, sizeof in);
        for (int c = 0; c < nc; c++) in.p[c] = tg_fp(t, c);
        fe h[3];
        toggle_claims_fetch(ctx, in, t->fl[t->s.cur], nc, h);
        fe_to_u64x4(h[0], flag);
        fe_to_u64x4(h[1], fp_a);
        if (fp_b) fe_to_u64x4(nc == 2 ? h[2] : Fr::zero(), fp_b);
    });
}

// current flags / fingerprints -> host (tests): flags n_fl x 4 u64, fingerprints n_fp x 4 u64 per component
int cozk_toggle_download(cozk_ctx* ctx, const cozk_toggle* t, uint64_t* flags, uint64_t* fp_a, uint64_t* fp_b, size_t* n_flags, size_t* n_fp) {
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(ctx && t, "toggle_download: bad argument");
        const ToggleShape& sh = t->s;
        size_t nfp = sh.coalesced ? sh.L : sh.batch * sh.n_cur, nfl = sh.coalesced ? sh.L : (sh.batch / 2) * sh.n_cur;
        if (n_flags) *n_flags = nfl;
        if (n_fp) *n_fp = nfp;
        std::vector<uint8_t> raw;
        if (flags && sh.cur < 0) {  // unbound: the packed bytes, expanded to field elements here
            raw.resize(nfl);
            HIP_TRY(hipMemcpyAsync(raw.data(), t->fl0, nfl, hipMemcpyDeviceToHost, ctx->stream));
        } else if (flags) {
            HIP_TRY(hipMemcpyAsync(flags, t->fl[sh.cur], nfl * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        }
        if (fp_a) HIP_TRY(hipMemcpyAsync(fp_a, tg_fp(t, 0), nfp * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        if (fp_b && t->mode == COZK_MODE_REP3) HIP_TRY(hipMemcpyAsync(fp_b, tg_fp(t, 1), nfp * sizeof(fe), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < raw.size(); i++) fe_to_u64x4(raw[i] ? Fr::one() : Fr::zero(), flags + 4 * i);
    });
}

}  // extern "C"

// ------------------------------------------------------------------ C ABI: toggle groups
struct cozk_toggle_group {
    cozk_ctx* driver;
    int k;
    ToggleShape s;
    const fe* fp0[COZK_LAYER_GROUP_MAX];  // unbound fingerprints: adopted (owner != null) or the caller's, which outlive the group
    cozk_ctx* owner[COZK_LAYER_GROUP_MAX];
    uint8_t* fl0;                         // packed 0/1 flags (owned)
    fe* fp[2];                            // ping-pong bound planes: member m at fp[w] + m * fp_cap[w]
    fe* fl[2];                            // ping-pong bound flags
    size_t fp_cap[2], fl_cap[2];
};

static ToggleGroupIn toggle_group_in(const cozk_toggle_group* g) {
    ToggleGroupIn a;
    memset(&a, 0, sizeof a);
    for (int m = 0; m < g->k; m++) a.p[m] = g->s.cur < 0 ? g->fp0[m] : g->fp[g->s.cur] + (size_t)m * g->fp_cap[g->s.cur];
    return a;
}
static const void* toggle_group_fl(const cozk_toggle_group* g) { return g->s.cur < 0 ? (const void*)g->fl0 : (const void*)g->fl[g->s.cur]; }

// one bind of the planes and the flags: ONE launch, which at layer_len == 2 writes the coalesced vectors (L entries each)
static void toggle_group_bind_launch(cozk_toggle_group* g, const fe& rr) {
    cozk_ctx* const ctx = g->driver;
    ToggleShape::BindSizes b = g->s.bind_sizes();
    if (b.coalesces) b.n_fp = b.n_fl = g->s.L;
    const int dst = g->s.dst();
    const bool u8 = g->s.cur < 0;  // the first bind reads the packed 0/1 bytes
    COZK_REQUIRE(b.n_fp <= g->fp_cap[dst] && b.n_fl <= g->fl_cap[dst], "toggle_group: bound planes larger than their storage");
    const dim3 grid(grid_for(b.n_fp), (unsigned)g->k);
    auto* const kernel = b.coalesces ? (u8 ? k_toggle_group_bind<0, 1> : k_toggle_group_bind<1, 1>) : (u8 ? k_toggle_group_bind<0, 0> : k_toggle_group_bind<1, 0>);
    kernel<<<grid, PT, 0, ctx->stream>>>(toggle_group_in(g), g->fp[dst], g->fp_cap[dst], b.n_fp, toggle_group_fl(g), g->fl[dst], b.n_fl, g->s.batch, rr);
    HIP_TRY(hipGetLastError());
    g->s.advance();
}

extern "C" {

int cozk_toggle_group_free(cozk_toggle_group* g) {
    if (!g) return COZK_OK;
    for (int m = 0; m < g->k; m++)
        if (g->owner[m]) ctx_dev_free(g->owner[m], (void*)g->fp0[m]);
    if (g->fl0) ctx_dev_free(g->driver, g->fl0);
    for (int w = 0; w < 2; w++) {
        if (g->fp[w]) ctx_dev_free(g->driver, g->fp[w]);
        if (g->fl[w]) ctx_dev_free(g->driver, g->fl[w]);
    }
    delete g;
    return COZK_OK;
}

int cozk_toggle_group_create(cozk_ctx* driver, const cozk_vec* const* flags, size_t n_pairs, cozk_vec* const* fingerprints, int k, int take_ownership,
                             cozk_toggle_group** out) {
    if (out) *out = nullptr;
    cozk_toggle_group* g = nullptr;
    int rc = cozk_guard(driver, [&] {
        COZK_REQUIRE(driver && flags && fingerprints && out && n_pairs > 0, "toggle_group_create: null argument");
        COZK_REQUIRE(k >= 1 && k <= COZK_LAYER_GROUP_MAX, "toggle_group_create: 1 <= k <= COZK_LAYER_GROUP_MAX");
        const size_t batch = 2 * n_pairs;
        std::vector<cozk_ctx*> owners;
        for (int m = 0; m < k; m++) {
            const cozk_vec* v = fingerprints[m];
            group_member_check<false>("toggle_group_create", MemberNouns{"fingerprint vector", "fingerprint vector", "fingerprint vector"}, driver, fingerprints, m);
            COZK_REQUIRE(v->kind == COZK_SCALAR_FR, "toggle_group_create: the fingerprints must be FR vectors");
            COZK_REQUIRE(v->n == fingerprints[0]->n, "toggle_group_create: the fingerprint vectors must have one length");
            owners.push_back(v->ctx);
        }
        const size_t total = fingerprints[0]->n;
        COZK_REQUIRE(total % batch == 0, "toggle_group_create: fingerprints.len() must be 2 * n_pairs * N");
        const size_t n0 = total / batch;
        COZK_REQUIRE(n0 >= 2 && (n0 & (n0 - 1)) == 0, "toggle_group_create: fingerprints per circuit must be a power of two >= 2");
        for (size_t q = 0; q < n_pairs; q++) {  // a column that is missing or of another shape is toggle_pack_flags' to refuse
            if (!flags[q] || !flags[q]->ctx) continue;
            COZK_REQUIRE(flags[q]->ctx->device == driver->device, "toggle_group_create: every flag column must live on the driver's device");
            owners.push_back(flags[q]->ctx);
        }
        drain_streams(owners, driver);  // the inputs' own streams; the driver's own work is in order with its launches
        g = new cozk_toggle_group();  // value-initialised: k = 0, no buffers yet
        g->driver = driver;
        g->s.init(batch, n0);
        // both ping-pong sides, once, from the driver's pool: the first bind writes side 0, the second side 1, and every later
        // bind no more than the one two before it; the coalesced vectors have L entries.  Later rounds allocate nothing.
        for (int w = 0; w < 2; w++) {
            const size_t fpn = batch * n0 >> (w + 1), fln = n_pairs * n0 >> (w + 1), L = g->s.L;
            g->fp_cap[w] = fpn > L ? fpn : L;
            g->fl_cap[w] = fln > L ? fln : L;
            g->fp[w] = dev_alloc_fe((size_t)k * g->fp_cap[w]);
            g->fl[w] = dev_alloc_fe(g->fl_cap[w]);
        }
        toggle_pack_flags(driver, flags, n_pairs, n0, "toggle_group_create", &g->fl0);
        for (int m = 0; m < k; m++) {  // nothing fails from here on: adopt
            cozk_vec* v = fingerprints[m];
            g->fp0[m] = (const fe*)v->d;
            g->owner[m] = nullptr;
            if (take_ownership && v->owned) {
                g->owner[m] = v->ctx;
                (void)vec_adopt(v);
            }
        }
        g->k = k;
        *out = g;
    });
    if (rc != COZK_OK && g) {
        (void)hipStreamSynchronize(driver->stream);
        cozk_toggle_group_free(g);
    }
    return rc;
}

int cozk_toggle_group_layer_outputs(cozk_toggle_group* g, cozk_ctx* const* owners, cozk_vec** out) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    if (out)
        for (int m = 0; m < g->k; m++) out[m] = nullptr;
    ToggleGroupOut o;
    memset(&o, 0, sizeof o);
    int rc = cozk_guard(ctx, [&] {
        COZK_REQUIRE(owners && out, "toggle_group_layer_outputs: null argument");
        COZK_REQUIRE(g->s.cur < 0, "toggle_group_layer_outputs: needs an unbound group");
        for (int m = 0; m < g->k; m++) {
            COZK_REQUIRE(owners[m], "toggle_group_layer_outputs: null owner");
            COZK_REQUIRE(owners[m]->device == ctx->device, "toggle_group_layer_outputs: every owner must live on the driver's device");
        }
        const size_t total = g->s.batch * g->s.n0;
        for (int m = 0; m < g->k; m++) o.p[m] = (fe*)ctx_dev_alloc(owners[m], total * sizeof(fe));
        k_toggle_group_output<<<grid_for(total), PT, 0, ctx->stream>>>(toggle_group_in(g), o, g->fl0, log2_sz(g->s.n0), total, g->k);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the outputs are their owners' from here on
        for (int m = 0; m < g->k; m++) out[m] = new cozk_vec{owners[m], total, COZK_SCALAR_FR, o.p[m], total * sizeof(fe), true};
    });
    if (rc != COZK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        for (int m = 0; m < g->k; m++) {
            if (out && out[m]) delete out[m], out[m] = nullptr;
            if (o.p[m] && owners && owners[m]) ctx_dev_free(owners[m], o.p[m]);
        }
    }
    return rc;
}

int cozk_toggle_group_bind(cozk_toggle_group* g, const uint64_t r[4]) {
    if (!g) return COZK_ERR_INVALID_ARG;
    return cozk_guard(g->driver, [&] {
        COZK_REQUIRE(r, "toggle_group_bind: null argument");
        COZK_REQUIRE(!g->s.bound(), "toggle_group_bind: the group is fully bound");
        toggle_group_bind_launch(g, fe_from_u64x4(r));
    });
}

int cozk_toggle_group_round(cozk_toggle_group* g, cozk_spliteq* e, const uint64_t* r, uint64_t* out_evals) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(e && out_evals, "toggle_group_round: null argument");
        COZK_REQUIRE(e->ctx == ctx, "toggle_group_round: the eq polynomial must be the driver's");
        COZK_REQUIRE(!g->s.bound(), "toggle_group_round: the group is fully bound");
        if (r) {
            COZK_REQUIRE(!spliteq_bound(e), "toggle_group_round: eq polynomial already fully bound");
            COZK_REQUIRE(!g->s.last_bind(), "toggle_group_round: the bind leaves the group fully bound, with no round to run (cozk_toggle_group_bind)");
            const fe rr = fe_from_u64x4(r);
            toggle_group_bind_launch(g, rr);
            spliteq_bind_launch(ctx, e, rr);  // once for all members
        }
        const unsigned k = (unsigned)g->k;
        const size_t npairs = g->s.npairs();
        const unsigned gx = sum_grid(grid_capped(npairs, ROUND_GRID_MAX));
        const unsigned rows = 3 * k + 3;
        const SumLaunch sl = sum_launch(ctx, rows, gx, rows + 3);
        const EqView v = eq_view(e);
        const bool u8 = g->s.cur < 0;  // first round: the packed 0/1 bytes
        const dim3 grid(gx, (k + TOGGLE_GROUP_CHUNK - 1) / TOGGLE_GROUP_CHUNK);
        auto* const kernel = v.nested ? (u8 ? k_toggle_group_cubic<1, 0> : k_toggle_group_cubic<1, 1>) : (u8 ? k_toggle_group_cubic<0, 0> : k_toggle_group_cubic<0, 1>);
        kernel<<<grid, PT, 0, ctx->stream>>>(toggle_group_in(g), (int)k, toggle_group_fl(g), npairs, g->s.log_half_n(), v.E1, v.lg1, v.E2, v.E2_len, sl.partial);
        eq_sums_launch(ctx, v, npairs, sl.res + rows);  // behind the finished rows
        fe s[3 * COZK_LAYER_GROUP_MAX + 6];
        finish_sums(ctx, sl, rows, gx, Fr::one(), 0, s);
        for (unsigned m = 0; m < k; m++)
            for (int x = 0; x < 3; x++) fe_to_u64x4(Fr::add(s[3 * m + x], Fr::sub(s[rows + x], s[3 * k + x])), out_evals + 12 * m + 4 * x);
    });
}

int cozk_toggle_group_final_claims(cozk_toggle_group* g, uint64_t flag[4], uint64_t* fingerprints, int k_final) {
    if (!g) return COZK_ERR_INVALID_ARG;
    cozk_ctx* const ctx = g->driver;
    return cozk_guard(ctx, [&] {
        COZK_REQUIRE(flag && (fingerprints || k_final == 0), "toggle_group_final_claims: null argument");
        COZK_REQUIRE(k_final >= 0 && k_final <= g->k, "toggle_group_final_claims: 0 <= k_final <= k");
        COZK_REQUIRE(g->s.bound(), "toggle_group_final_claims: the group is not fully bound");
        fe h[COZK_LAYER_GROUP_MAX + 1];
        toggle_claims_fetch(ctx, toggle_group_in(g), g->fl[g->s.cur], k_final, h);
        fe_to_u64x4(h[0], flag);
        for (int m = 0; m < k_final; m++) fe_to_u64x4(h[1 + m], fingerprints + 4 * m);
    });
}

}  // extern "C"
