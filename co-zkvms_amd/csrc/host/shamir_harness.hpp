// What the in-process Shamir provers share (shamir_spartan.hpp, shamir_jolt_spartan.hpp, shamir_primary.hpp): the handle base, the keys
// and the dealing of a create, the context of one prove -- the parties, the Lagrange vectors, the zero masks, the two kinds of opening
// -- and the prove / read-back plumbing of the C ABI.  Each prover keeps its protocol steps, timing marks and stats of its own.
// Included by harness.hip behind shamir_gp.hpp (ShamirGpArgs, shamir_gp_zero_masks, shamir_open, fe_copy_out), ahead of the provers.
#pragma once

namespace cozk {

struct ShamirHarness : HarnessHandle {
    int t = 0, n = 0;
    std::vector<cozk_ctx*> pcs;                    // party p's context, referred to (its party struct owns it)
    std::vector<std::vector<uint8_t>> rand_keys;  // [p][3t + 1]: the keys of the zero masks' preprocessing
    std::vector<fe> msgs;                          // [m][p <= 2t]: opening m of degree 2t, masked
    std::vector<fe> finals;                        // [value][p <= t]: the openings of degree t, in the order opened
    cozk_shamir_gp_stats stats{};
};

// The keys of a harness of `seed`: the t sharing keys of the dealer, key c = (seed ^ 0x53484152, c), returned; party p's 3t + 1 mask
// keys, key j = (seed ^ 0x52414E44, 64 p + j), into h->rand_keys.
static std::vector<uint8_t> shamir_harness_keys(ShamirHarness* h, uint64_t seed) {
    const int t = h->t;
    std::vector<uint8_t> skeys((size_t)t * COZK_PRF_KEY_BYTES);
    for (int c = 0; c < t; c++) harness_prf_key(seed ^ 0x53484152ull, (uint64_t)c, skeys.data() + (size_t)c * COZK_PRF_KEY_BYTES);
    h->rand_keys.assign((size_t)h->n, std::vector<uint8_t>((size_t)(3 * t + 1) * COZK_PRF_KEY_BYTES));
    for (int p = 0; p < h->n; p++)
        for (int j = 0; j <= 3 * t; j++)
            harness_prf_key(seed ^ 0x52414E44ull, (uint64_t)(64 * p + j), h->rand_keys[(size_t)p].data() + (size_t)j * COZK_PRF_KEY_BYTES);
    return skeys;
}

// One clear column (a vector of party 0's context) dealt to all n parties by cozk_shamir_scatter's rule at `counter`: party p < holders
// gets its share as a PLAIN polynomial of its own context.  keep: where the share vectors go (party p's at [p]); without it they
// return to their parties' pools.  Party 0's device is current at both ends.
static std::vector<PolyH> shamir_deal_column(ShamirHarness* h, const VecH& clear, const std::vector<uint8_t>& skeys, uint64_t counter, int holders,
                                             std::vector<VecH>* keep = nullptr) {
    const std::vector<cozk_ctx*>& pcs = h->pcs;
    HIP_TRY(hipSetDevice(pcs[0]->device));
    std::vector<cozk_vec*> sh((size_t)h->n, nullptr);
    rc_check(cozk_shamir_scatter(pcs[0], clear.h, skeys.data(), h->t, h->n, counter, pcs.data(), sh.data()), pcs[0], "shamir_scatter");
    std::vector<VecH> own;
    for (int p = 0; p < h->n; p++) own.emplace_back(sh[(size_t)p]);
    std::vector<PolyH> polys((size_t)holders);
    for (int p = 0; p < h->n; p++) {
        HIP_TRY(hipSetDevice(pcs[(size_t)p]->device));
        if (p < holders) polys[(size_t)p] = plain_poly(pcs[(size_t)p], own[(size_t)p]);
        HIP_TRY(hipStreamSynchronize(pcs[(size_t)p]->stream));
        if (!keep) own[(size_t)p] = VecH();
    }
    if (keep) *keep = std::move(own);
    HIP_TRY(hipSetDevice(pcs[0]->device));
    return polys;
}

// One prove of a Shamir harness: built at its top (h->msgs, finals and stats start empty), it carries what every step needs.
struct ShamirProve {
    ShamirHarness* const h;
    const int t, n, senders, openers;
    const std::vector<cozk_ctx*>& pcs;
    cozk_ctx* const c0;
    const ShamirGpArgs a;
    const bool grouped;                   // the senders' contexts are on one device: the rounds run as groups (shamir_gp_grouped)
    const std::vector<fe> lam2t, lamt;    // lagrange(1..2t + 1), lagrange(1..t + 1)
    std::vector<std::vector<fe>> zero;    // zero[p][m], p <= 2t: the degree-2t sharings of zero (deal_masks)

    ShamirProve(ShamirHarness* h_, bool verify)
        : h(h_), t(h_->t), n(h_->n), senders(2 * t + 1), openers(t + 1), pcs(h_->pcs), c0(pcs[0]), a{pcs.data(), nullptr, 0, t, n, nullptr, verify},
          grouped(shamir_gp_grouped(a)), lam2t(shamir_lagrange_first(senders)), lamt(shamir_lagrange_first(openers)) {
        h->msgs.clear();
        h->finals.clear();
        h->stats = cozk_shamir_gp_stats{};
    }
    ShamirProve(const ShamirProve&) = delete;

    void set_dev(int p) const { HIP_TRY(hipSetDevice(pcs[(size_t)p]->device)); }
    void sync_all() const { shamir_gp_sync_all(a); }
    // M masks: ONE dealing at rand_counter, pair 0 only (shamir_gp_zero_masks); the pair-reuse contract of the grand product applies
    void deal_masks(uint64_t rand_counter, size_t M) {
        std::vector<const uint8_t*> rk((size_t)n);
        for (int p = 0; p < n; p++) rk[(size_t)p] = h->rand_keys[(size_t)p].data();
        zero = shamir_gp_zero_masks(a, rk.data(), rand_counter, M);
    }
    // degree t, unmasked, from parties 0..t; the openers' shares are part of `finals`
    fe open_t(const fe* sh) const {
        for (int p = 0; p < openers; p++) h->finals.push_back(sh[p]);
        return shamir_open(lamt, sh);
    }
    // degree 2t, from senders 0..2t behind mask m: sender p's local value is the 4 words at local + stride p; what it sends is part of `msgs`
    fe open_2t(const uint64_t* local, size_t stride, size_t m) const {
        fe sh[COZK_SHAMIR_MAX_PARTIES];
        for (int p = 0; p < senders; p++) {
            sh[p] = Fr::add(fe_from_u64x4(local + stride * (size_t)p), zero[(size_t)p][m]);
            h->msgs.push_back(sh[p]);
        }
        return shamir_open(lam2t, sh);
    }
    // one round message of a degree-2 sumcheck from the openers' (g(0), g(2)) and the public running claim: every coefficient is opened
    fe open_quadratic(fe (*e02)[2], fe& claim, std::vector<std::vector<fe>>& compressed, Transcript& tr) const {
        fe cf[COZK_SHAMIR_MAX_PARTIES][3];
        for (int p = 0; p < openers; p++) {
            const fe pts[3] = {e02[p][0], Fr::sub(claim, e02[p][0]), e02[p][1]};
            unipoly_from_evals(pts, 3, cf[p]);
        }
        std::vector<fe> poly(3);
        for (int i = 0; i < 3; i++) {
            fe sh[COZK_SHAMIR_MAX_PARTIES];
            for (int p = 0; p < openers; p++) sh[p] = cf[p][i];
            poly[(size_t)i] = open_t(sh);
        }
        const std::vector<fe> comp = unipoly_compress(poly);
        tr.append_scalars(comp);
        const fe r = tr.challenge_scalar();
        claim = unipoly_eval(poly, r);
        compressed.push_back(comp);
        return r;
    }
    // free the handles of parties 0 .. first.size() - 1, each with its party's device current
    template <class V, class... W>
    void release(V& first, W&... rest) const {
        for (size_t p = 0; p < first.size(); p++) {
            set_dev((int)p);
            first[p] = typename V::value_type();
            ((rest[p] = typename W::value_type()), ...);
        }
    }
};

// *_prove of the C ABI: built(h) says whether create went through; prove(h, res) throws.  After a device error every party's stream is
// drained, so that the harness can be destroyed.
template <class H, class R, class Built, class Prove>
int shamir_harness_prove(H* h, R* res, const char* name, Built built, Prove prove) {
    if (!h || !res) return COZK_ERR_INVALID_ARG;
    memset(res, 0, sizeof *res);
    res->verified = -1;
    if (h->n == 0 || h->pcs.size() != (size_t)h->n || !built(h)) {
        h->error = std::string(name) + "_prove: the harness was not built";
        return COZK_ERR_INVALID_ARG;
    }
    h->error.clear();
    try {
        prove(h, res);
    } catch (const CozkError& e) {
        h->error = e.what();
        for (cozk_ctx* c : h->pcs) (void)hipStreamSynchronize(c->stream);
        return e.code;
    } catch (const std::exception& e) {
        h->error = e.what();
        return COZK_ERR_INTERNAL;
    }
    return COZK_OK;
}

inline int shamir_harness_stats(const ShamirHarness* h, cozk_shamir_gp_stats* stats) {
    if (!h || !stats) return COZK_ERR_INVALID_ARG;
    *stats = h->stats;
    return COZK_OK;
}

}  // namespace cozk
