// The dense batched grand product (GKR) proved by n Shamir parties, all driven from the one thread that owns their contexts and
// plays the coordinator (cozk_shamir_gp_prove_inproc).  The reference has no Shamir prover; tests/shamir_gp_ref.py restates this
// file in big integers.  Included by harness.hip behind prover.hpp.
//
// Why the PLAIN kernels serve: eq is public, so every term of every sumcheck here multiplies at most TWO secret factors.  A party
// that runs the COZK_MODE_PLAIN kernels on its degree-t share vectors, with the PUBLIC claim as its prev_claim, therefore holds a
// degree-2t sharing of the plain prover's round message (the four coefficients are linear in the three sums and the claim, and
// the Lagrange coefficients sum to one), and opening it from parties 0..2t with lagrange(1..2t + 1) gives that message exactly:
// the proof is byte-identical to the plain prover's proof of the same witness.
//
//   construct   layer[0] = the leaves; layer[i + 1] = cozk_shamir_mul_pairs_inproc(layer[i]) with counter = mul_counter + the sum
//               of the earlier levels' output lengths (the discipline of WorkerEnv::mask_ctr)
//   masks       M = batch_size + 4 sum_layers rounds(layer); ONE cozk_shamir_rand_inproc of M elements at rand_counter; pair 0 only:
//               zero_p[m] = r2t_p^0[m] - rt_p^0[m], a degree-2t sharing of zero, downloaded once per sender
//   openings    of degree 2t, indexed m = 0, 1, .. in the order opened -- the outputs, then layer by layer from the top and round
//               by round the coefficients 0..3: sender p <= 2t sends local_p + zero_p[m], the coordinator combines the 2t + 1
//               messages with lagrange(1..2t + 1)
//   finals      L, R after the last bind are linear combinations (public challenges) of freshly dealt degree-t sharings: opened
//               from parties 0..t with lagrange(1..t + 1), unmasked
//   transcript  and proof layout: exactly coordinate_prove_grand_product / coordinate_prove_layer (prover.hpp)
// Parties above 2t take part in the construction (they receive their shares of every level) and send nothing afterwards.
// The senders' layers of one tree level share the public eq polynomial, the challenge and the claim: when their contexts are on one
// device a layer's sumcheck runs as ONE layer group (cozk_layer_group_round / _final, poly.hip) with ONE eq on sender 0's context --
// one launch and one fetch per round for all senders; otherwise sender by sender (shamir_gp_grouped).  Same bytes either way.
//
// The king variant (cozk_shamir_gp_prep_inproc + cozk_shamir_gp_prove_king_inproc; tests/shamir_gp_king_ref.py) moves everything
// that needs fresh randomness before the witness: the masks above and two double-random pairs of n_leaves / 2 elements are dealt
// into a preprocessing object, and the construct becomes layer[i + 1] = cozk_shamir_mul_king_pairs_inproc(layer[i]) on slices of
// those pairs.  Both provers are one construct loop with the level's multiplication as a parameter (shamir_gp_construct) in front
// of one copy of the openings, rounds, finals, transcript and proof (shamir_gp_prove_layers).
//
// The TOGGLED grand product (cozk_shamir_tgp_*; tests/shamir_tgp_ref.py) puts the toggle layer of Lasso's read / write memory checking
// under that tree.  Its flags are public, so its output flag ? fingerprint : 1 and its round polynomial eq (flag fingerprint + 1 - flag)
// are AFFINE in the fingerprint share: a party that runs the PLAIN toggle calls on its degree-t share, with the public claim as its
// previous claim, holds a degree-t sharing of the plain prover's values (the share of a public constant is that constant for every
// party, which is what PLAIN mode adds).  Level 0 of the tree is the senders' toggle outputs; the dense layers run as above; the
// toggle layer's nv + d rounds follow (no r_layer, no claim fold), opened from senders 0..2t with 4 (nv + d) more of the same zero
// masks; the flag claim is public and the fingerprint claim is opened from parties 0..t, unmasked.  The senders' toggle layers run
// as ONE cozk_toggle_group on sender 0's context under the same rule as the layer groups, otherwise as a cozk_toggle per sender.
#pragma once
#include "prover.hpp"
#include "runner.hpp"

// shamir.hip: the double-random preprocessing that extracts only `count` pairs, the degree-t halves for parties 0..rcp_t - 1, the
// degree-2t halves for the senders
int shamir_rand_pairs_inproc(cozk_ctx* const* pcs, const uint8_t* const* keys, size_t n_elems, int t, int np, uint64_t counter, int count, int rcp_t,
                             cozk_vec** r_t, cozk_vec** r_2t);

struct cozk_shamir_gp {
    cozk::Bytes proof;
    fe claim;
    std::vector<fe> r;
    std::vector<fe> msgs;    // [m][p]: opening m, sender p <= 2t
    std::vector<fe> finals;  // [layer, top first][p <= t][L, R]
    cozk_shamir_gp_result res;
    cozk_shamir_gp_stats stats{};
    bool toggled = false;  // a toggled proof: the toggle layer's final claims and how its rounds ran
    fe tg_flag, tg_fingerprint;
    cozk_shamir_gp_toggle_stats tstats{};
};

namespace cozk {

static inline fe shamir_open(const std::vector<fe>& lambda, const fe* shares) {
    fe acc = Fr::zero();
    for (size_t p = 0; p < lambda.size(); p++) acc = Fr::add(acc, Fr::mul(lambda[p], shares[p]));
    return acc;
}

// the read-back of recorded openings (*_msgs, *_finals): v = NULL stands for a null handle
static inline int fe_copy_out(const std::vector<fe>* v, uint64_t* out, size_t cap) {
    if (!v || !out || cap < v->size()) return COZK_ERR_INVALID_ARG;
    for (size_t k = 0; k < v->size(); k++) fe_to_u64x4((*v)[k], out + 4 * k);
    return COZK_OK;
}

static inline std::vector<fe> shamir_lagrange_first(int k) {
    std::vector<uint32_t> pts((size_t)k);
    for (int p = 0; p < k; p++) pts[(size_t)p] = (uint32_t)p + 1;
    std::vector<uint64_t> raw((size_t)4 * k);
    if (cozk_shamir_lagrange(pts.data(), (size_t)k, raw.data()) != COZK_OK) throw CozkError(COZK_ERR_INTERNAL, "shamir_gp: lagrange");
    std::vector<fe> l((size_t)k);
    for (int p = 0; p < k; p++) l[(size_t)p] = fe_from_u64x4(raw.data() + 4 * p);
    return l;
}

struct ShamirGpArgs {
    cozk_ctx* const* pcs;
    const cozk_vec* const* leaves;
    size_t batch_size;
    int t, n;
    const char* label;
    bool verify;
    bool adopt_leaves = false;  // the leaves are vectors of our own (a toggled proof's level 0): adopted, not copied
};

static inline void shamir_gp_sync_all(const ShamirGpArgs& a) {
    for (int p = 0; p < a.n; p++) rc_check(cozk_ctx_synchronize(a.pcs[p]), a.pcs[p], "ctx_synchronize");
}

typedef Handle<cozk_layer_group, cozk_layer_group_free> GroupH;
typedef Handle<cozk_toggle_group, cozk_toggle_group_free> ToggleGroupH;

// Whether the rounds run as layer groups (cozk_layer_group_*): one launch per round for all senders instead of one per sender, one
// fold of the public eq tables instead of 2t + 1.  That needs every sender's context on ONE device (one group per device for
// senders spread over several is not built).  COZK_SHAMIR_GP_GROUP=0: the per-sender loop, for A/B runs; read on every call, as
// COZK_SUM_GRID_MAX is, so that one process can compare both.
static inline bool shamir_gp_grouped(const ShamirGpArgs& a) {
    const char* e = getenv("COZK_SHAMIR_GP_GROUP");
    if (e && atoi(e) == 0) return false;
    for (int p = 1; p <= 2 * a.t; p++)
        if (a.pcs[p]->device != a.pcs[0]->device) return false;
    return true;
}

// M = batch_size + 4 sum_layers rounds(layer): the openings of degree 2t of one proof
static inline size_t shamir_gp_num_openings(size_t n_leaves, size_t batch_size) {
    const int num_layers = ceil_log2(n_leaves / batch_size), nv_out = ceil_log2(batch_size);
    size_t M = batch_size;
    for (int k = 0; k < num_layers; k++) M += (size_t)4 * (size_t)(nv_out + k);
    return M;
}

// ---- construct: layers[i][p], senders only (a party above 2t multiplies nothing and opens nothing: its share of a level is
// dropped).  mul_level(i, v, next) is one tree level for all parties, next[q][j] = party q's share of v[2j] v[2j + 1]: the
// resharing multiplication or the king's.  Every stream is drained at both ends; returns the host time between them.
template <class MulLevel>
static double shamir_gp_construct(const ShamirGpArgs& a, std::vector<std::vector<LayerH>>& layers, MulLevel mul_level) {
    const int senders = 2 * a.t + 1;
    const int num_layers = ceil_log2(a.leaves[0]->n / a.batch_size);
    shamir_gp_sync_all(a);
    const double t0 = now_ms();
    layers.clear();
    layers.resize((size_t)num_layers);
    std::vector<VecH> cur((size_t)a.n);  // level i as vectors (level 0: the caller's)
    for (int i = 0; i < num_layers; i++) {
        std::vector<const cozk_vec*> v((size_t)a.n, nullptr);
        for (int p = 0; p < senders; p++) v[(size_t)p] = i ? cur[(size_t)p].h : a.leaves[p];
        std::vector<cozk_vec*> next((size_t)a.n, nullptr);
        if (i + 1 < num_layers) mul_level(i, v.data(), next.data());
        std::vector<VecH> nx((size_t)a.n);
        for (int p = 0; p < a.n; p++) nx[(size_t)p] = VecH(next[(size_t)p]);
        for (int p = 0; p < senders; p++) {  // the caller's leaves are copied (it keeps them), a level of our own is adopted
            cozk_layer* l = nullptr;
            rc_check(cozk_layer_create(a.pcs[p], COZK_MODE_PLAIN, v[(size_t)p], nullptr, i || a.adopt_leaves ? 1 : 0, &l), a.pcs[p], "layer_create");
            layers[(size_t)i].push_back(LayerH(l));
        }
        cur = std::move(nx);
    }
    cur.clear();
    shamir_gp_sync_all(a);
    return now_ms() - t0;
}

// ---- masks: pair 0 of one preprocessing call of M elements, as a sharing of zero of degree 2t; zero[p][m] for the senders.  Only
// the senders' halves of that one pair are dealt to and extracted: the values are those of cozk_shamir_rand_inproc
static std::vector<std::vector<fe>> shamir_gp_zero_masks(const ShamirGpArgs& a, const uint8_t* const* rand_keys, uint64_t rand_counter, size_t M) {
    const int senders = 2 * a.t + 1;
    std::vector<std::vector<fe>> zero((size_t)senders, std::vector<fe>(M));
    std::vector<cozk_vec*> rt((size_t)senders, nullptr), r2t((size_t)senders, nullptr);
    rc_check(shamir_rand_pairs_inproc(a.pcs, rand_keys, M, a.t, a.n, rand_counter, 1, senders, rt.data(), r2t.data()), a.pcs[0], "shamir_rand_pairs_inproc");
    std::vector<VecH> own;
    for (int p = 0; p < senders; p++) {
        own.emplace_back(rt[(size_t)p]);
        own.emplace_back(r2t[(size_t)p]);
    }
    for (int p = 0; p < senders; p++) {
        cozk_vec* z = nullptr;
        rc_check(cozk_vec_alloc(a.pcs[p], M, COZK_SCALAR_FR, &z), a.pcs[p], "vec_alloc");
        VecH zh(z);
        rc_check(cozk_vec_binop(a.pcs[p], COZK_OP_SUB, 0, r2t[(size_t)p], rt[(size_t)p], z), a.pcs[p], "vec_binop");
        std::vector<uint64_t> raw(4 * M);
        rc_check(cozk_vec_download(a.pcs[p], z, raw.data()), a.pcs[p], "vec_download");
        for (size_t m = 0; m < M; m++) zero[(size_t)p][m] = fe_from_u64x4(raw.data() + 4 * m);
    }
    shamir_gp_sync_all(a);  // the pairs go back to their parties' pools behind everything that read them
    return zero;
}

// ---- the toggle layer of a toggled proof: ONE group on sender 0's context (grouped) or a PLAIN cozk_toggle per sender, and the
// senders' toggle outputs, level 0 of the tree
struct ShamirToggleLayer {
    ToggleGroupH group;
    std::vector<ToggleH> toggles;
    std::vector<VecH> outputs;  // [p <= 2t], a vector of pcs[p]
    size_t rounds = 0;          // nv + d
};

// the openings the toggle layer adds to the dense tree's: 4 per round, nv + d rounds
static inline size_t shamir_tgp_rounds(size_t n_pairs, size_t n_per) { return (size_t)(ceil_log2(2 * n_pairs) + ceil_log2(n_per)); }

// flags: n_pairs U8 columns of pcs[0]; fingerprints[p]: sender p's shares.  Grouped: the group refers to the senders' fingerprints
// (they are only read) and writes every sender's output in one launch.  Otherwise sender p gets the flags on its own context, a
// toggle of its own for the rounds, and its output from a one-plane group driven by its own context (the one output kernel)
static void shamir_tgp_make_toggle(const ShamirGpArgs& a, const cozk_vec* const* flags, size_t n_pairs, const cozk_vec* const* fingerprints, bool grouped,
                                   ShamirToggleLayer& tg) {
    const int senders = 2 * a.t + 1;
    tg.rounds = shamir_tgp_rounds(n_pairs, fingerprints[0]->n / (2 * n_pairs));
    tg.outputs.resize((size_t)senders);
    shamir_gp_sync_all(a);
    if (grouped) {
        cozk_vec* fps[COZK_SHAMIR_MAX_PARTIES];
        cozk_vec* outs[COZK_SHAMIR_MAX_PARTIES];
        for (int p = 0; p < senders; p++) fps[p] = const_cast<cozk_vec*>(fingerprints[p]);  // take_ownership = 0: read only
        rc_check(cozk_toggle_group_create(a.pcs[0], flags, n_pairs, fps, senders, 0, &tg.group.h), a.pcs[0], "toggle_group_create");
        rc_check(cozk_toggle_group_layer_outputs(tg.group.h, a.pcs, outs), a.pcs[0], "toggle_group_layer_outputs");
        for (int p = 0; p < senders; p++) tg.outputs[(size_t)p] = VecH(outs[p]);
        return;
    }
    tg.toggles.resize((size_t)senders);
    for (int p = 0; p < senders; p++) {
        std::vector<VecH> own;  // the flags on sender p's context
        std::vector<const cozk_vec*> fl(n_pairs);
        for (size_t q = 0; q < n_pairs; q++) {
            fl[q] = flags[q];
            if (a.pcs[p] == a.pcs[0]) continue;
            cozk_vec* c = nullptr;
            rc_check(cozk_vec_alloc(a.pcs[p], flags[q]->n, COZK_SCALAR_U8, &c), a.pcs[p], "vec_alloc");
            own.emplace_back(c);
            HIP_TRY(hipMemcpy(c->d, flags[q]->d, flags[q]->n, hipMemcpyDefault));
            fl[q] = c;
        }
        cozk_vec* fp = const_cast<cozk_vec*>(fingerprints[p]);
        cozk_vec* out = nullptr;
        ToggleGroupH one;
        rc_check(cozk_toggle_group_create(a.pcs[p], fl.data(), n_pairs, &fp, 1, 0, &one.h), a.pcs[p], "toggle_group_create");
        rc_check(cozk_toggle_group_layer_outputs(one.h, a.pcs + p, &out), a.pcs[p], "toggle_group_layer_outputs");
        tg.outputs[(size_t)p] = VecH(out);
        rc_check(cozk_toggle_create(a.pcs[p], COZK_MODE_PLAIN, fl.data(), n_pairs, fp, nullptr, 0, &tg.toggles[(size_t)p].h), a.pcs[p], "toggle_create");
        rc_check(cozk_ctx_synchronize(a.pcs[p]), a.pcs[p], "ctx_synchronize");  // the copies of the flags go out of scope
    }
}

// ---- openings, rounds, finals, transcript and proof on constructed layers with given masks: what both constructs share.
// tg != null: a toggled proof -- the toggle layer's rounds and claims follow the dense layers
// t_prove_ms runs from t_start (the caller's clock, every stream drained) to the drain behind the last round
static void shamir_gp_prove_layers(const ShamirGpArgs& a, std::vector<std::vector<LayerH>>& layers, const std::vector<std::vector<fe>>& zero, double t_start,
                                   cozk_shamir_gp& h, ShamirToggleLayer* tg = nullptr) {
    const int senders = 2 * a.t + 1, openers = a.t + 1;
    const int num_layers = (int)layers.size();
    const size_t M = zero[0].size();
    const std::vector<fe> lam2t = shamir_lagrange_first(senders), lamt = shamir_lagrange_first(openers);
    const bool grouped = shamir_gp_grouped(a);

    // the openings of degree 2t: local[p] = sender p's unmasked value of opening m
    size_t m_next = 0;
    h.msgs.assign(M * (size_t)senders, Fr::zero());
    auto open_2t = [&](const fe* local) {
        COZK_REQUIRE(m_next < M, "shamir_gp: more openings than masks");
        fe* msg = &h.msgs[m_next * (size_t)senders];
        for (int p = 0; p < senders; p++) msg[p] = Fr::add(local[p], zero[(size_t)p][m_next]);
        m_next++;
        return shamir_open(lam2t, msg);
    };

    Transcript tr(a.label);
    GrandProductProof proof;
    {
        std::vector<std::vector<uint64_t>> outs((size_t)senders, std::vector<uint64_t>(4 * a.batch_size));
        for (int p = 0; p < senders; p++)
            rc_check(cozk_layer_claimed_outputs(a.pcs[p], layers.back()[(size_t)p].h, outs[(size_t)p].data()), a.pcs[p], "claimed_outputs");
        std::vector<fe> local((size_t)senders);
        for (size_t i = 0; i < a.batch_size; i++) {
            for (int p = 0; p < senders; p++) local[(size_t)p] = fe_from_u64x4(outs[(size_t)p].data() + 4 * i);
            proof.outputs.push_back(open_2t(local.data()));
        }
    }
    tr.append_scalars(proof.outputs);
    std::vector<fe> r;
    fe claim = mle_claim_padded(proof.outputs, tr, r);
    for (int i = num_layers; i-- > 0;) {
        GrandProductLayerProof lp;
        const int num_rounds = (int)r.size();
        std::vector<uint64_t> w = to_abi(r);
        // grouped: ONE eq on sender 0's context and one group over the senders' layers; otherwise an eq per sender
        std::vector<EqH> eqs((size_t)(grouped ? 1 : senders));
        for (size_t p = 0; p < eqs.size(); p++) rc_check(cozk_spliteq_new(a.pcs[p], w.data(), num_rounds, &eqs[p].h), a.pcs[p], "spliteq_new");
        GroupH group;
        if (grouped) {
            cozk_layer* members[COZK_SHAMIR_MAX_PARTIES];
            for (int p = 0; p < senders; p++) members[p] = layers[(size_t)i][(size_t)p].h;
            rc_check(cozk_layer_group_create(a.pcs[0], members, senders, &group.h), a.pcs[0], "layer_group_create");
        }
        std::vector<fe> r_sumcheck;
        uint64_t rj[4], pc[4];
        std::vector<uint64_t> co((size_t)16 * senders);
        for (int j = 0; j < num_rounds; j++) {
            fe_to_u64x4(claim, pc);  // every party's prev_claim is the public claim
            fe cf[4][COZK_SHAMIR_MAX_PARTIES];
            if (grouped) {
                rc_check(cozk_layer_group_round(group.h, eqs[0].h, j ? rj : nullptr, pc, co.data()), a.pcs[0], "layer_group_round");
                h.stats.group_rounds++;
            } else {
                for (int p = 0; p < senders; p++) {
                    rc_check(cozk_layer_round(a.pcs[p], layers[(size_t)i][(size_t)p].h, eqs[(size_t)p].h, j ? rj : nullptr, pc, co.data() + 16 * p), a.pcs[p],
                             "layer_round");
                    h.stats.single_rounds++;
                }
            }
            for (int p = 0; p < senders; p++)
                for (int k = 0; k < 4; k++) cf[k][p] = fe_from_u64x4(co.data() + 16 * p + 4 * k);
            std::vector<fe> poly(4);
            for (int k = 0; k < 4; k++) poly[(size_t)k] = open_2t(cf[k]);
            std::vector<fe> comp = unipoly_compress(poly);
            tr.append_scalars(comp);
            fe r_j = tr.challenge_scalar();
            r_sumcheck.push_back(r_j);
            fe_to_u64x4(r_j, rj);
            claim = unipoly_eval(poly, r_j);
            lp.proof.compressed_polys.push_back(comp);
        }
        fe fl[COZK_SHAMIR_MAX_PARTIES], fr[COZK_SHAMIR_MAX_PARTIES];
        std::vector<uint64_t> fc((size_t)16 * openers);
        if (grouped) {  // the last bind and the final claims: the t + 1 openers only
            rc_check(cozk_layer_group_final(group.h, eqs[0].h, num_rounds ? rj : nullptr, openers, fc.data()), a.pcs[0], "layer_group_final");
            h.stats.group_finals++;
        } else {
            for (int p = 0; p < openers; p++) {
                cozk_layer* l = layers[(size_t)i][(size_t)p].h;
                if (num_rounds) rc_check(cozk_layer_bind(a.pcs[p], l, rj), a.pcs[p], "layer_bind");
                rc_check(cozk_layer_final_claims(a.pcs[p], l, fc.data() + 16 * p), a.pcs[p], "layer_final_claims");
                h.stats.single_finals++;
            }
        }
        for (int p = 0; p < openers; p++) {
            fl[p] = fe_from_u64x4(fc.data() + 16 * p);
            fr[p] = fe_from_u64x4(fc.data() + 16 * p + 8);
            h.finals.push_back(fl[p]);
            h.finals.push_back(fr[p]);
        }
        lp.left_claim = shamir_open(lamt, fl);
        lp.right_claim = shamir_open(lamt, fr);
        tr.append_scalar(lp.left_claim);
        tr.append_scalar(lp.right_claim);
        r.assign(r_sumcheck.rbegin(), r_sumcheck.rend());
        fe r_layer = tr.challenge_scalar();
        claim = Fr::add(lp.left_claim, Fr::mul(r_layer, Fr::sub(lp.right_claim, lp.left_claim)));
        r.push_back(r_layer);
        proof.gkr_layers.push_back(std::move(lp));
        layers[(size_t)i].clear();  // bound: nothing reads it again
    }
    if (tg) {
        // prove_layer of the toggle layer as coordinate_prove_toggle_layer sees it: nv + d rounds against eq(r), no r_layer and no claim
        // fold.  Sender p's four coefficients are unipoly_from_evals(g0, claim - g0, g2, g3) of its PLAIN toggle round with the public
        // claim: a degree-t sharing of the plain prover's, opened with the degree-2t zero masks from senders 0..2t
        GrandProductLayerProof lp;
        const int num_rounds = (int)r.size();
        COZK_REQUIRE((size_t)num_rounds == tg->rounds, "shamir_tgp: the toggle layer's rounds do not match the point");
        std::vector<uint64_t> w = to_abi(r);
        std::vector<EqH> eqs((size_t)(grouped ? 1 : senders));
        for (size_t p = 0; p < eqs.size(); p++) rc_check(cozk_spliteq_new(a.pcs[p], w.data(), num_rounds, &eqs[p].h), a.pcs[p], "spliteq_new");
        std::vector<fe> r_sumcheck;
        uint64_t rj[4];
        std::vector<uint64_t> ev((size_t)12 * senders);
        for (int j = 0; j < num_rounds; j++) {
            fe cf[4][COZK_SHAMIR_MAX_PARTIES];
            if (grouped) {
                rc_check(cozk_toggle_group_round(tg->group.h, eqs[0].h, j ? rj : nullptr, ev.data()), a.pcs[0], "toggle_group_round");
                h.tstats.toggle_group_rounds++;
            } else {
                for (int p = 0; p < senders; p++) {
                    rc_check(cozk_toggle_round(a.pcs[p], tg->toggles[(size_t)p].h, eqs[(size_t)p].h, j ? rj : nullptr, 0, ev.data() + 12 * p), a.pcs[p],
                             "toggle_round");
                    h.tstats.toggle_single_rounds++;
                }
            }
            for (int p = 0; p < senders; p++) {
                fe c4[4];
                cubic_from_round_evals(claim, ev.data() + 12 * p, c4);
                for (int k = 0; k < 4; k++) cf[k][p] = c4[k];
            }
            std::vector<fe> poly(4);
            for (int k = 0; k < 4; k++) poly[(size_t)k] = open_2t(cf[k]);
            std::vector<fe> comp = unipoly_compress(poly);
            tr.append_scalars(comp);
            fe r_j = tr.challenge_scalar();
            r_sumcheck.push_back(r_j);
            fe_to_u64x4(r_j, rj);
            claim = unipoly_eval(poly, r_j);
            lp.proof.compressed_polys.push_back(comp);
        }
        // the last bind and the final claims: the flag is public, the fingerprint is opened from the t + 1 openers, unmasked
        uint64_t flag[4], fps[4 * COZK_SHAMIR_MAX_PARTIES], unused[4];
        if (grouped) {
            rc_check(cozk_toggle_group_bind(tg->group.h, rj), a.pcs[0], "toggle_group_bind");
            rc_check(cozk_toggle_group_final_claims(tg->group.h, flag, fps, openers), a.pcs[0], "toggle_group_final_claims");
        } else {
            for (int p = 0; p < openers; p++) {
                cozk_toggle* t = tg->toggles[(size_t)p].h;
                rc_check(cozk_toggle_bind(a.pcs[p], t, rj), a.pcs[p], "toggle_bind");
                rc_check(cozk_toggle_final_claims(a.pcs[p], t, p ? unused : flag, fps + 4 * p, nullptr), a.pcs[p], "toggle_final_claims");
            }
        }
        fe sh[COZK_SHAMIR_MAX_PARTIES];
        lp.left_claim = fe_from_u64x4(flag);
        for (int p = 0; p < openers; p++) {
            sh[p] = fe_from_u64x4(fps + 4 * p);
            h.finals.push_back(lp.left_claim);
            h.finals.push_back(sh[p]);
        }
        lp.right_claim = shamir_open(lamt, sh);
        tr.append_scalar(lp.left_claim);
        tr.append_scalar(lp.right_claim);
        r.assign(r_sumcheck.rbegin(), r_sumcheck.rend());
        proof.gkr_layers.push_back(std::move(lp));
        h.toggled = true;
        h.tg_flag = proof.gkr_layers.back().left_claim;
        h.tg_fingerprint = proof.gkr_layers.back().right_claim;
        tg->group = ToggleGroupH();
        tg->toggles.clear();
    }
    COZK_REQUIRE(m_next == M, "shamir_gp: fewer openings than masks");
    shamir_gp_sync_all(a);
    h.res.t_prove_ms = now_ms() - t_start;

    Writer wr;
    proof.write(wr);
    h.proof = std::move(wr.b);
    h.claim = claim;
    h.r = r;
    h.res.proof_len = h.proof.size();
    h.res.n_layers = num_layers + (tg ? 1 : 0);
    h.res.n_opened = M;
    h.res.verified = -1;
    if (a.verify) {
        Transcript vt(a.label);
        fe vc;
        std::vector<fe> vr;
        bool ok;
        if (tg) {
            fe vf, vp;
            ok = verify_toggled_grand_product(proof, vt, vf, vp, vr) && Fr::eq(vf, h.tg_flag) && Fr::eq(vp, h.tg_fingerprint) && vr.size() == r.size();
        } else {
            ok = verify_grand_product(proof, vt, vc, vr) && Fr::eq(vc, claim) && vr.size() == r.size();
        }
        for (size_t k = 0; ok && k < r.size(); k++) ok = Fr::eq(vr[k], r[k]);
        h.res.verified = ok ? 1 : 0;
    }
}

// what both provers require of their arguments once degree and num_parties are known to be in range
static void shamir_gp_require_leaves(const std::string& w, cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, int degree, const char* missing,
                                     const std::string& what = "leaves") {
    for (int p = 0; p <= 2 * degree; p++) {
        COZK_REQUIRE(leaves[p], w + missing);
        COZK_REQUIRE(leaves[p]->kind == COZK_SCALAR_FR, w + ": the " + what + " must be FR vectors");
        COZK_REQUIRE(leaves[p]->n == leaves[0]->n, w + ": the " + what + " must have one length");
        COZK_REQUIRE(leaves[p]->ctx == party_ctxs[p], w + ": party p's " + what + " must be a vector of party_ctxs[p]");
    }
}
static void shamir_gp_require_shape(const std::string& w, size_t n, size_t batch_size) {
    COZK_REQUIRE(batch_size > 0 && n > 0 && n % batch_size == 0, w + ": leaves.len() % batch_size != 0");
    const size_t per = n / batch_size;
    COZK_REQUIRE(per >= 2 && (per & (per - 1)) == 0, w + ": leaves per circuit must be a power of two >= 2");
}
static void shamir_gp_require_parties(const std::string& w, int degree, int num_parties) {
    COZK_REQUIRE(degree >= 1 && 2 * degree <= COZK_SHAMIR_MAX_DEGREE, w + ": 1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE (the masks are dealt with degree 2t)");
    COZK_REQUIRE(2 * degree + 1 <= num_parties && num_parties <= COZK_SHAMIR_MAX_PARTIES, w + ": 2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES");
}

}  // namespace cozk

// The preprocessing of one king grand product (cozk_shamir_gp_prep_inproc): everything that needs fresh randomness, made before the
// leaves exist.  (A) the opening masks of cozk_shamir_gp_prove_inproc, M elements at rand_counter, pair 0, held on the host as the
// senders' sharings of zero; (B) ONE dealing of n_leaves / 2 elements at rand_counter + M, of which pair 0 serves level 0 whole and
// pair 1 serves level i >= 1 at the element offset n_leaves / 2 - n_leaves / 2^i (the sum of the output lengths of levels 1..i - 1;
// the last level ends at n_leaves / 2 - 2 batch_size).  Only what a proof uses is extracted: no pair for 2 leaves per circuit, one
// for 4, two otherwise; the degree-2t halves for the senders only.
struct cozk_shamir_gp_prep {
    std::vector<cozk_ctx*> pcs;
    int t = 0, n = 0, pairs = 0;
    size_t n_leaves = 0, batch_size = 0, pair_elems = 0;
    bool used = false;
    bool toggled = false;  // made by cozk_shamir_tgp_prep_inproc: 4 (nv + d) more masks, the construct pairs behind them
    double t_offline_ms = 0;
    std::vector<std::vector<fe>> zero;  // [p <= 2t][m < M]
    std::vector<cozk_vec*> rt, r2t;     // rt[q * pairs + k], every party; r2t[p * pairs + k], senders
    void release_pairs() {
        for (cozk_vec* v : rt) cozk_vec_free(v);
        for (cozk_vec* v : r2t) cozk_vec_free(v);
        rt.clear();
        r2t.clear();
    }
    ~cozk_shamir_gp_prep() { release_pairs(); }
};

// both preps: the dense tree of (n_leaves, batch_size) with toggle_rounds more rounds' masks (0: a dense proof's prep)
static int shamir_gp_prep_make(const std::string& w, cozk_ctx* const* party_ctxs, const uint8_t* const* rand_keys, size_t n_leaves, size_t batch_size,
                               size_t toggle_rounds, bool toggled, int degree, int num_parties, uint64_t rand_counter, cozk_shamir_gp_prep** prep) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES ? party_ctxs[0] : nullptr;  // receives the error message
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(prep, w + ": null output"); });
    if (rc != COZK_OK) return rc;
    *prep = nullptr;
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && rand_keys, w + ": null argument");
        shamir_gp_require_parties(w, degree, num_parties);
        for (int p = 0; p < num_parties; p++) {
            COZK_REQUIRE(party_ctxs[p], w + ": null party context");
            COZK_REQUIRE(rand_keys[p], w + ": every party needs its mask key block");
        }
        if (toggled) COZK_REQUIRE(n_leaves > 0, w + ": n_pairs > 0 and N a power of two >= 2");
        shamir_gp_require_shape(w, n_leaves, batch_size);
    });
    if (rc != COZK_OK) return rc;
    cozk_shamir_gp_prep* h = new cozk_shamir_gp_prep();
    rc = cozk_guard(c0, [&] {
        const ShamirGpArgs a{party_ctxs, nullptr, batch_size, degree, num_parties, nullptr, false};
        const int senders = 2 * degree + 1, levels = ceil_log2(n_leaves / batch_size) - 1;
        h->pcs.assign(party_ctxs, party_ctxs + num_parties);
        h->t = degree, h->n = num_parties, h->n_leaves = n_leaves, h->batch_size = batch_size;
        h->toggled = toggled;
        h->pairs = levels <= 0 ? 0 : levels == 1 ? 1 : 2;
        h->pair_elems = h->pairs ? n_leaves / 2 : 0;
        shamir_gp_sync_all(a);
        const double t0 = now_ms();
        const size_t M = shamir_gp_num_openings(n_leaves, batch_size) + 4 * toggle_rounds;
        h->zero = shamir_gp_zero_masks(a, rand_keys, rand_counter, M);
        if (h->pairs) {
            h->rt.assign((size_t)num_parties * h->pairs, nullptr);
            h->r2t.assign((size_t)senders * h->pairs, nullptr);
            rc_check(shamir_rand_pairs_inproc(party_ctxs, rand_keys, h->pair_elems, degree, num_parties, rand_counter + M, h->pairs, num_parties, h->rt.data(),
                                              h->r2t.data()),
                     c0, "shamir_rand_pairs_inproc");
        }
        shamir_gp_sync_all(a);
        h->t_offline_ms = now_ms() - t0;
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *prep = h;
    return COZK_OK;
}

// the king's tree level on slices of a prep's pairs: pair 0 serves level 0 whole, pair 1 the levels above at their offsets
static auto shamir_gp_king_level(cozk_ctx* const* party_ctxs, cozk_shamir_gp_prep* prep, int king) {
    return [=](int i, const cozk_vec* const* v, cozk_vec** next) {
        const int k = i ? 1 : 0, num_parties = prep->n;
        std::vector<const cozk_vec*> rt((size_t)num_parties, nullptr), r2t((size_t)num_parties, nullptr);
        for (int q = 0; q < num_parties; q++) rt[(size_t)q] = prep->rt[(size_t)q * prep->pairs + k];
        for (int p = 0; p <= 2 * prep->t; p++) r2t[(size_t)p] = prep->r2t[(size_t)p * prep->pairs + k];
        const size_t off = i ? prep->n_leaves / 2 - (prep->n_leaves >> i) : 0;
        cozk::rc_check(cozk_shamir_mul_king_pairs_inproc(party_ctxs, v, rt.data(), r2t.data(), off, prep->t, num_parties, king, next), party_ctxs[0],
                       "shamir_mul_king_pairs_inproc");
    };
}

// what the toggled provers require of the flags and the fingerprints once the parties are known to be in range
static void shamir_tgp_require_inputs(const std::string& w, cozk_ctx* const* party_ctxs, const cozk_vec* const* flags, size_t n_pairs,
                                      const cozk_vec* const* fingerprints, int degree) {
    using namespace cozk;
    COZK_REQUIRE(n_pairs > 0, w + ": n_pairs == 0");
    shamir_gp_require_leaves(w, party_ctxs, fingerprints, degree, ": parties 0..2 * degree need their fingerprints", "fingerprints");
    const size_t batch = 2 * n_pairs, total = fingerprints[0]->n;
    COZK_REQUIRE(total % batch == 0, w + ": fingerprints.len() must be 2 * n_pairs * N");
    const size_t per = total / batch;
    COZK_REQUIRE(per >= 2 && (per & (per - 1)) == 0, w + ": fingerprints per circuit must be a power of two >= 2");
    for (size_t q = 0; q < n_pairs; q++) {
        COZK_REQUIRE(flags[q] && flags[q]->kind == COZK_SCALAR_U8 && flags[q]->n == per, w + ": every flag column is a U8 vector of N entries");
        COZK_REQUIRE(flags[q]->ctx == party_ctxs[0], w + ": the flag columns must be vectors of party_ctxs[0]");
    }
}

extern "C" {

int cozk_shamir_gp_prep_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* rand_keys, size_t n_leaves, size_t batch_size, int degree,
                               int num_parties, uint64_t rand_counter, cozk_shamir_gp_prep** prep) {
    return shamir_gp_prep_make("shamir_gp_prep_inproc", party_ctxs, rand_keys, n_leaves, batch_size, 0, false, degree, num_parties, rand_counter, prep);
}

// n_per = N fingerprints per circuit: the dense tree above the toggle layer has 2 n_pairs N leaves in 2 n_pairs circuits
int cozk_shamir_tgp_prep_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* rand_keys, size_t n_pairs, size_t n_per, int degree, int num_parties,
                                uint64_t rand_counter, cozk_shamir_gp_prep** prep) {
    const bool shape = n_pairs > 0 && n_per >= 2 && (n_per & (n_per - 1)) == 0;  // otherwise n_leaves = 0, refused with its text
    return shamir_gp_prep_make("shamir_tgp_prep_inproc", party_ctxs, rand_keys, shape ? 2 * n_pairs * n_per : 0, 2 * n_pairs,
                               shape ? cozk::shamir_tgp_rounds(n_pairs, n_per) : 0, true, degree, num_parties, rand_counter, prep);
}

int cozk_shamir_gp_prep_free(cozk_shamir_gp_prep* prep) {
    delete prep;
    return COZK_OK;
}

int cozk_shamir_gp_prep_get_result(const cozk_shamir_gp_prep* prep, cozk_shamir_gp_prep_result* res) {
    if (!prep || !res) return COZK_ERR_INVALID_ARG;
    res->n_openings = prep->zero.empty() ? 0 : prep->zero[0].size();
    res->pair_elems = prep->pair_elems;
    res->pairs_held = (int)(prep->rt.size() / (size_t)prep->n);
    res->used = prep->used ? 1 : 0;
    res->t_offline_ms = prep->t_offline_ms;
    return COZK_OK;
}

int cozk_shamir_gp_prove_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, size_t batch_size, cozk_shamir_gp_prep* prep, int king,
                                     const char* label, int verify, cozk_shamir_gp** out) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs ? party_ctxs[0] : nullptr;  // receives the error message (a prover has at least three parties)
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(out, "shamir_gp_prove_king_inproc: null output"); });
    if (rc != COZK_OK) return rc;
    *out = nullptr;
    const std::string w = "shamir_gp_prove_king_inproc";
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && leaves && prep && label, w + ": null argument");
        COZK_REQUIRE(!prep->toggled, w + ": the preprocessing was made for a toggled grand product (cozk_shamir_tgp_prove_king_inproc)");
        COZK_REQUIRE(king >= 0 && king < prep->n, w + ": 0 <= king < num_parties");
        for (int p = 0; p < prep->n; p++) {
            COZK_REQUIRE(party_ctxs[p], w + ": null party context");
            COZK_REQUIRE(party_ctxs[p] == prep->pcs[(size_t)p], w + ": the preprocessing was made for other party contexts");
        }
        shamir_gp_require_leaves(w, party_ctxs, leaves, prep->t, ": parties 0..2 * degree need their leaves");
        shamir_gp_require_shape(w, leaves[0]->n, batch_size);
        COZK_REQUIRE(leaves[0]->n == prep->n_leaves && batch_size == prep->batch_size, w + ": the preprocessing was made for another (n_leaves, batch_size)");
        COZK_REQUIRE(!prep->used, w + ": the preprocessing has been used (a pair must never be used twice)");
    });
    if (rc != COZK_OK) return rc;
    const int num_parties = prep->n;
    prep->used = true;
    cozk_shamir_gp* h = new cozk_shamir_gp();
    memset(&h->res, 0, sizeof h->res);
    rc = cozk_guard(c0, [&] {
        const ShamirGpArgs a{party_ctxs, leaves, batch_size, prep->t, num_parties, label, verify != 0};
        std::vector<std::vector<LayerH>> layers;
        h->res.t_construct_ms = shamir_gp_construct(a, layers, shamir_gp_king_level(party_ctxs, prep, king));
        prep->release_pairs();  // consumed: every stream has drained behind the construct
        shamir_gp_prove_layers(a, layers, prep->zero, now_ms(), *h);
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *out = h;
    return COZK_OK;
}

int cozk_shamir_gp_prove_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, size_t batch_size, const uint8_t* const* mul_keys,
                                const uint8_t* const* rand_keys, int degree, int num_parties, uint64_t mul_counter, uint64_t rand_counter,
                                const char* label, int verify, cozk_shamir_gp** out) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES ? party_ctxs[0] : nullptr;  // receives the error message
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(out, "shamir_gp_prove_inproc: null output"); });
    if (rc != COZK_OK) return rc;
    *out = nullptr;
    const std::string w = "shamir_gp_prove_inproc";
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && leaves && mul_keys && rand_keys && label, "shamir_gp_prove_inproc: null argument");
        shamir_gp_require_parties(w, degree, num_parties);
        for (int p = 0; p < num_parties; p++) {
            COZK_REQUIRE(party_ctxs[p], "shamir_gp_prove_inproc: null party context");
            COZK_REQUIRE(rand_keys[p], "shamir_gp_prove_inproc: every party needs its mask key block");
        }
        for (int p = 0; p <= 2 * degree; p++) COZK_REQUIRE(leaves[p] && mul_keys[p], "shamir_gp_prove_inproc: parties 0..2 * degree need their leaves and their key block");
        shamir_gp_require_leaves(w, party_ctxs, leaves, degree, ": parties 0..2 * degree need their leaves and their key block");
        shamir_gp_require_shape(w, leaves[0]->n, batch_size);
    });
    if (rc != COZK_OK) return rc;
    cozk_shamir_gp* h = new cozk_shamir_gp();
    memset(&h->res, 0, sizeof h->res);
    rc = cozk_guard(c0, [&] {
        const ShamirGpArgs a{party_ctxs, leaves, batch_size, degree, num_parties, label, verify != 0};
        std::vector<std::vector<LayerH>> layers;
        uint64_t ctr = mul_counter;  // level i: mul_counter + the sum of the earlier levels' output lengths
        h->res.t_construct_ms = shamir_gp_construct(a, layers, [&](int, const cozk_vec* const* v, cozk_vec** next) {
            rc_check(cozk_shamir_mul_pairs_inproc(party_ctxs, v, mul_keys, degree, num_parties, ctr, next), c0, "shamir_mul_pairs_inproc");
            ctr += v[0]->n / 2;
        });
        const double t1 = now_ms();
        const std::vector<std::vector<fe>> zero = shamir_gp_zero_masks(a, rand_keys, rand_counter, shamir_gp_num_openings(leaves[0]->n, batch_size));
        shamir_gp_prove_layers(a, layers, zero, t1, *h);
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *out = h;
    return COZK_OK;
}

}  // extern "C"

// The toggled provers: the toggle layer and its outputs (level 0, adopted), the construct with the level's multiplication as a
// parameter, the masks, and the one copy of the openings, rounds, finals, transcript and proof.  t_construct_ms includes the
// toggle outputs.
template <class MulLevel, class Masks>
static void shamir_tgp_prove(const cozk::ShamirGpArgs& a0, const cozk_vec* const* flags, size_t n_pairs, const cozk_vec* const* fingerprints, MulLevel mul_level,
                             Masks masks, cozk_shamir_gp& h) {
    using namespace cozk;
    shamir_gp_sync_all(a0);
    const double t0 = now_ms();
    ShamirToggleLayer tg;
    shamir_tgp_make_toggle(a0, flags, n_pairs, fingerprints, shamir_gp_grouped(a0), tg);
    std::vector<const cozk_vec*> level0((size_t)a0.n, nullptr);
    for (int p = 0; p <= 2 * a0.t; p++) level0[(size_t)p] = tg.outputs[(size_t)p].h;
    ShamirGpArgs a = a0;
    a.leaves = level0.data();
    a.adopt_leaves = true;
    std::vector<std::vector<LayerH>> layers;
    shamir_gp_construct(a, layers, mul_level);
    tg.outputs.clear();  // adopted by level 0
    h.res.t_construct_ms = now_ms() - t0;
    const double t1 = now_ms();
    const std::vector<std::vector<fe>>& zero = masks();
    shamir_gp_prove_layers(a, layers, zero, t1, h, &tg);
}

extern "C" {

int cozk_shamir_tgp_prove_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* flags, size_t n_pairs, const cozk_vec* const* fingerprints,
                                 const uint8_t* const* mul_keys, const uint8_t* const* rand_keys, int degree, int num_parties, uint64_t mul_counter,
                                 uint64_t rand_counter, const char* label, int verify, cozk_shamir_gp** out) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES ? party_ctxs[0] : nullptr;  // receives the error message
    const std::string w = "shamir_tgp_prove_inproc";
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(out, w + ": null output"); });
    if (rc != COZK_OK) return rc;
    *out = nullptr;
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && flags && fingerprints && mul_keys && rand_keys && label, w + ": null argument");
        shamir_gp_require_parties(w, degree, num_parties);
        for (int p = 0; p < num_parties; p++) {
            COZK_REQUIRE(party_ctxs[p], w + ": null party context");
            COZK_REQUIRE(rand_keys[p], w + ": every party needs its mask key block");
        }
        for (int p = 0; p <= 2 * degree; p++) COZK_REQUIRE(fingerprints[p] && mul_keys[p], w + ": parties 0..2 * degree need their fingerprints and their key block");
        shamir_tgp_require_inputs(w, party_ctxs, flags, n_pairs, fingerprints, degree);
    });
    if (rc != COZK_OK) return rc;
    cozk_shamir_gp* h = new cozk_shamir_gp();
    memset(&h->res, 0, sizeof h->res);
    rc = cozk_guard(c0, [&] {
        const size_t batch = 2 * n_pairs, n_leaves = fingerprints[0]->n;
        const ShamirGpArgs a{party_ctxs, nullptr, batch, degree, num_parties, label, verify != 0};
        uint64_t ctr = mul_counter;  // level i: mul_counter + the sum of the earlier levels' output lengths
        std::vector<std::vector<fe>> zero;
        shamir_tgp_prove(
            a, flags, n_pairs, fingerprints,
            [&](int, const cozk_vec* const* v, cozk_vec** next) {
                rc_check(cozk_shamir_mul_pairs_inproc(party_ctxs, v, mul_keys, degree, num_parties, ctr, next), c0, "shamir_mul_pairs_inproc");
                ctr += v[0]->n / 2;
            },
            [&]() -> const std::vector<std::vector<fe>>& {
                zero = shamir_gp_zero_masks(a, rand_keys, rand_counter, shamir_gp_num_openings(n_leaves, batch) + 4 * shamir_tgp_rounds(n_pairs, n_leaves / batch));
                return zero;
            },
            *h);
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *out = h;
    return COZK_OK;
}

int cozk_shamir_tgp_prove_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* flags, size_t n_pairs, const cozk_vec* const* fingerprints,
                                      cozk_shamir_gp_prep* prep, int king, const char* label, int verify, cozk_shamir_gp** out) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs ? party_ctxs[0] : nullptr;  // receives the error message (a prover has at least three parties)
    const std::string w = "shamir_tgp_prove_king_inproc";
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(out, w + ": null output"); });
    if (rc != COZK_OK) return rc;
    *out = nullptr;
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && flags && fingerprints && prep && label, w + ": null argument");
        COZK_REQUIRE(prep->toggled, w + ": the preprocessing was made for a dense grand product (cozk_shamir_gp_prove_king_inproc)");
        COZK_REQUIRE(king >= 0 && king < prep->n, w + ": 0 <= king < num_parties");
        for (int p = 0; p < prep->n; p++) {
            COZK_REQUIRE(party_ctxs[p], w + ": null party context");
            COZK_REQUIRE(party_ctxs[p] == prep->pcs[(size_t)p], w + ": the preprocessing was made for other party contexts");
        }
        shamir_tgp_require_inputs(w, party_ctxs, flags, n_pairs, fingerprints, prep->t);
        COZK_REQUIRE(fingerprints[0]->n == prep->n_leaves && 2 * n_pairs == prep->batch_size, w + ": the preprocessing was made for another (n_pairs, N)");
        COZK_REQUIRE(!prep->used, w + ": the preprocessing has been used (a pair must never be used twice)");
    });
    if (rc != COZK_OK) return rc;
    const int num_parties = prep->n;
    prep->used = true;
    cozk_shamir_gp* h = new cozk_shamir_gp();
    memset(&h->res, 0, sizeof h->res);
    rc = cozk_guard(c0, [&] {
        const ShamirGpArgs a{party_ctxs, nullptr, 2 * n_pairs, prep->t, num_parties, label, verify != 0};
        shamir_tgp_prove(a, flags, n_pairs, fingerprints, shamir_gp_king_level(party_ctxs, prep, king),
                         [&]() -> const std::vector<std::vector<fe>>& {
                             prep->release_pairs();  // consumed: every stream has drained behind the construct
                             return prep->zero;
                         },
                         *h);
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *out = h;
    return COZK_OK;
}

int cozk_shamir_gp_toggle_claims(const cozk_shamir_gp* h, uint64_t flag[4], uint64_t fingerprint[4]) {
    if (!h || !flag || !fingerprint || !h->toggled) return COZK_ERR_INVALID_ARG;  // a dense proof has no toggle layer
    fe_to_u64x4(h->tg_flag, flag);
    fe_to_u64x4(h->tg_fingerprint, fingerprint);
    return COZK_OK;
}

int cozk_shamir_gp_get_toggle_stats(const cozk_shamir_gp* h, cozk_shamir_gp_toggle_stats* stats) {
    if (!h || !stats) return COZK_ERR_INVALID_ARG;
    *stats = h->tstats;
    return COZK_OK;
}

int cozk_shamir_gp_free(cozk_shamir_gp* h) {
    delete h;
    return COZK_OK;
}

int cozk_shamir_gp_get_result(const cozk_shamir_gp* h, cozk_shamir_gp_result* res) {
    if (!h || !res) return COZK_ERR_INVALID_ARG;
    *res = h->res;
    return COZK_OK;
}

int cozk_shamir_gp_get_stats(const cozk_shamir_gp* h, cozk_shamir_gp_stats* stats) {
    if (!h || !stats) return COZK_ERR_INVALID_ARG;
    *stats = h->stats;
    return COZK_OK;
}

int cozk_shamir_gp_proof_bytes(const cozk_shamir_gp* h, uint8_t* out, size_t cap) {
    if (!h || !out || cap < h->proof.size()) return COZK_ERR_INVALID_ARG;
    memcpy(out, h->proof.data(), h->proof.size());
    return COZK_OK;
}

size_t cozk_shamir_gp_point_len(const cozk_shamir_gp* h) { return h ? h->r.size() : 0; }

int cozk_shamir_gp_final(const cozk_shamir_gp* h, uint64_t claim[4], uint64_t* r) {
    if (!h || !claim || (!r && !h->r.empty())) return COZK_ERR_INVALID_ARG;
    fe_to_u64x4(h->claim, claim);
    for (size_t k = 0; k < h->r.size(); k++) fe_to_u64x4(h->r[k], r + 4 * k);
    return COZK_OK;
}

size_t cozk_shamir_gp_msgs_len(const cozk_shamir_gp* h) { return h ? h->msgs.size() : 0; }
size_t cozk_shamir_gp_finals_len(const cozk_shamir_gp* h) { return h ? h->finals.size() : 0; }

int cozk_shamir_gp_msgs(const cozk_shamir_gp* h, uint64_t* out, size_t cap) { return cozk::fe_copy_out(h ? &h->msgs : nullptr, out, cap); }
int cozk_shamir_gp_finals(const cozk_shamir_gp* h, uint64_t* out, size_t cap) { return cozk::fe_copy_out(h ? &h->finals : nullptr, out, cap); }

}  // extern "C"
