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
#pragma once
#include "prover.hpp"
#include "runner.hpp"

struct cozk_shamir_gp {
    cozk::Bytes proof;
    fe claim;
    std::vector<fe> r;
    std::vector<fe> msgs;    // [m][p]: opening m, sender p <= 2t
    std::vector<fe> finals;  // [layer, top first][p <= t][L, R]
    cozk_shamir_gp_result res;
};

namespace cozk {

static inline fe shamir_open(const std::vector<fe>& lambda, const fe* shares) {
    fe acc = Fr::zero();
    for (size_t p = 0; p < lambda.size(); p++) acc = Fr::add(acc, Fr::mul(lambda[p], shares[p]));
    return acc;
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
    const uint8_t* const* mul_keys;
    const uint8_t* const* rand_keys;
    int t, n;
    uint64_t mul_counter, rand_counter;
    const char* label;
    bool verify;
};

static void shamir_gp_prove(const ShamirGpArgs& a, cozk_shamir_gp& h) {
    const int senders = 2 * a.t + 1, openers = a.t + 1;
    const size_t len0 = a.leaves[0]->n, per = len0 / a.batch_size;
    const int num_layers = ceil_log2(per);
    const std::vector<fe> lam2t = shamir_lagrange_first(senders), lamt = shamir_lagrange_first(openers);
    auto sync_all = [&] {
        for (int p = 0; p < a.n; p++) rc_check(cozk_ctx_synchronize(a.pcs[p]), a.pcs[p], "ctx_synchronize");
    };

    // ---- construct: layers[i][p], senders only (a party above 2t re-deals nothing and opens nothing: its share of a level is dropped)
    sync_all();
    double t0 = now_ms();
    std::vector<std::vector<LayerH>> layers((size_t)num_layers);
    std::vector<VecH> cur((size_t)a.n);  // level i as vectors (level 0: the caller's)
    uint64_t ctr = a.mul_counter;
    for (int i = 0; i < num_layers; i++) {
        std::vector<const cozk_vec*> v((size_t)a.n, nullptr);
        for (int p = 0; p < senders; p++) v[(size_t)p] = i ? cur[(size_t)p].h : a.leaves[p];
        std::vector<cozk_vec*> next((size_t)a.n, nullptr);
        if (i + 1 < num_layers) {
            rc_check(cozk_shamir_mul_pairs_inproc(a.pcs, v.data(), a.mul_keys, a.t, a.n, ctr, next.data()), a.pcs[0], "shamir_mul_pairs_inproc");
            ctr += v[0]->n / 2;
        }
        std::vector<VecH> nx((size_t)a.n);
        for (int p = 0; p < a.n; p++) nx[(size_t)p] = VecH(next[(size_t)p]);
        for (int p = 0; p < senders; p++) {  // level 0 is copied (the caller keeps its leaves), a level of our own is adopted
            cozk_layer* l = nullptr;
            rc_check(cozk_layer_create(a.pcs[p], COZK_MODE_PLAIN, v[(size_t)p], nullptr, i ? 1 : 0, &l), a.pcs[p], "layer_create");
            layers[(size_t)i].push_back(LayerH(l));
        }
        cur = std::move(nx);
    }
    cur.clear();
    sync_all();
    double t1 = now_ms();
    h.res.t_construct_ms = t1 - t0;

    // ---- masks: pair 0 of one preprocessing call, as a sharing of zero of degree 2t
    const int nv_out = ceil_log2(a.batch_size);
    size_t M = a.batch_size;
    for (int k = 0; k < num_layers; k++) M += (size_t)4 * (size_t)(nv_out + k);
    std::vector<std::vector<fe>> zero((size_t)senders, std::vector<fe>(M));
    {
        const size_t cnt = (size_t)(a.n - a.t), tbl = (size_t)a.n * cnt;
        std::vector<cozk_vec*> rt(tbl, nullptr), r2t(tbl, nullptr);
        rc_check(cozk_shamir_rand_inproc(a.pcs, a.rand_keys, M, a.t, a.n, a.rand_counter, rt.data(), r2t.data()), a.pcs[0], "shamir_rand_inproc");
        std::vector<VecH> own;
        for (size_t i = 0; i < tbl; i++) {
            own.emplace_back(rt[i]);
            own.emplace_back(r2t[i]);
        }
        for (int p = 0; p < senders; p++) {
            cozk_vec* z = nullptr;
            rc_check(cozk_vec_alloc(a.pcs[p], M, COZK_SCALAR_FR, &z), a.pcs[p], "vec_alloc");
            VecH zh(z);
            rc_check(cozk_vec_binop(a.pcs[p], COZK_OP_SUB, 0, r2t[(size_t)p * cnt], rt[(size_t)p * cnt], z), a.pcs[p], "vec_binop");
            std::vector<uint64_t> raw(4 * M);
            rc_check(cozk_vec_download(a.pcs[p], z, raw.data()), a.pcs[p], "vec_download");
            for (size_t m = 0; m < M; m++) zero[(size_t)p][m] = fe_from_u64x4(raw.data() + 4 * m);
        }
        sync_all();  // the pairs go back to their parties' pools behind everything that read them
    }

    // ---- the openings of degree 2t: local[p] = sender p's unmasked value of opening m
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
        std::vector<EqH> eqs((size_t)senders);
        std::vector<uint64_t> w = to_abi(r);
        for (int p = 0; p < senders; p++) rc_check(cozk_spliteq_new(a.pcs[p], w.data(), num_rounds, &eqs[(size_t)p].h), a.pcs[p], "spliteq_new");
        std::vector<fe> r_sumcheck;
        uint64_t rj[4], pc[4];
        for (int j = 0; j < num_rounds; j++) {
            fe_to_u64x4(claim, pc);  // every party's prev_claim is the public claim
            fe cf[4][COZK_SHAMIR_MAX_PARTIES];
            for (int p = 0; p < senders; p++) {
                uint64_t co[16];
                rc_check(cozk_layer_round(a.pcs[p], layers[(size_t)i][(size_t)p].h, eqs[(size_t)p].h, j ? rj : nullptr, pc, co), a.pcs[p], "layer_round");
                for (int k = 0; k < 4; k++) cf[k][p] = fe_from_u64x4(co + 4 * k);
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
        fe fl[COZK_SHAMIR_MAX_PARTIES], fr[COZK_SHAMIR_MAX_PARTIES];
        for (int p = 0; p < openers; p++) {  // the last bind and the final claims: the t + 1 openers only
            cozk_layer* l = layers[(size_t)i][(size_t)p].h;
            if (num_rounds) rc_check(cozk_layer_bind(a.pcs[p], l, rj), a.pcs[p], "layer_bind");
            uint64_t fc[16];
            rc_check(cozk_layer_final_claims(a.pcs[p], l, fc), a.pcs[p], "layer_final_claims");
            fl[p] = fe_from_u64x4(fc);
            fr[p] = fe_from_u64x4(fc + 8);
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
    COZK_REQUIRE(m_next == M, "shamir_gp: fewer openings than masks");
    sync_all();
    h.res.t_prove_ms = now_ms() - t1;

    Writer wr;
    proof.write(wr);
    h.proof = std::move(wr.b);
    h.claim = claim;
    h.r = r;
    h.res.proof_len = h.proof.size();
    h.res.n_layers = num_layers;
    h.res.n_opened = M;
    h.res.verified = -1;
    if (a.verify) {
        Transcript vt(a.label);
        fe vc;
        std::vector<fe> vr;
        bool ok = verify_grand_product(proof, vt, vc, vr) && Fr::eq(vc, claim) && vr.size() == r.size();
        for (size_t k = 0; ok && k < r.size(); k++) ok = Fr::eq(vr[k], r[k]);
        h.res.verified = ok ? 1 : 0;
    }
}

}  // namespace cozk

extern "C" {

int cozk_shamir_gp_prove_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, size_t batch_size, const uint8_t* const* mul_keys,
                                const uint8_t* const* rand_keys, int degree, int num_parties, uint64_t mul_counter, uint64_t rand_counter,
                                const char* label, int verify, cozk_shamir_gp** out) {
    using namespace cozk;
    cozk_ctx* const c0 = party_ctxs && num_parties >= 1 && num_parties <= COZK_SHAMIR_MAX_PARTIES ? party_ctxs[0] : nullptr;  // receives the error message
    int rc = cozk_guard(c0, [&] { COZK_REQUIRE(out, "shamir_gp_prove_inproc: null output"); });
    if (rc != COZK_OK) return rc;
    *out = nullptr;
    rc = cozk_guard(c0, [&] {
        COZK_REQUIRE(party_ctxs && leaves && mul_keys && rand_keys && label, "shamir_gp_prove_inproc: null argument");
        COZK_REQUIRE(degree >= 1 && 2 * degree <= COZK_SHAMIR_MAX_DEGREE,
                     "shamir_gp_prove_inproc: 1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE (the masks are dealt with degree 2t)");
        COZK_REQUIRE(2 * degree + 1 <= num_parties && num_parties <= COZK_SHAMIR_MAX_PARTIES,
                     "shamir_gp_prove_inproc: 2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES");
        for (int p = 0; p < num_parties; p++) {
            COZK_REQUIRE(party_ctxs[p], "shamir_gp_prove_inproc: null party context");
            COZK_REQUIRE(rand_keys[p], "shamir_gp_prove_inproc: every party needs its mask key block");
        }
        for (int p = 0; p <= 2 * degree; p++) {
            COZK_REQUIRE(leaves[p] && mul_keys[p], "shamir_gp_prove_inproc: parties 0..2 * degree need their leaves and their key block");
            COZK_REQUIRE(leaves[p]->kind == COZK_SCALAR_FR, "shamir_gp_prove_inproc: the leaves must be FR vectors");
            COZK_REQUIRE(leaves[p]->n == leaves[0]->n, "shamir_gp_prove_inproc: the leaves must have one length");
            COZK_REQUIRE(leaves[p]->ctx == party_ctxs[p], "shamir_gp_prove_inproc: party p's leaves must be a vector of party_ctxs[p]");
        }
        const size_t n = leaves[0]->n;
        COZK_REQUIRE(batch_size > 0 && n > 0 && n % batch_size == 0, "shamir_gp_prove_inproc: leaves.len() % batch_size != 0");
        const size_t per = n / batch_size;
        COZK_REQUIRE(per >= 2 && (per & (per - 1)) == 0, "shamir_gp_prove_inproc: leaves per circuit must be a power of two >= 2");
    });
    if (rc != COZK_OK) return rc;
    cozk_shamir_gp* h = new cozk_shamir_gp();
    memset(&h->res, 0, sizeof h->res);
    rc = cozk_guard(c0, [&] {
        shamir_gp_prove(ShamirGpArgs{party_ctxs, leaves, batch_size, mul_keys, rand_keys, degree, num_parties, mul_counter, rand_counter, label, verify != 0}, *h);
    });
    if (rc != COZK_OK) {
        for (int p = 0; p < num_parties; p++) (void)hipStreamSynchronize(party_ctxs[p]->stream);
        delete h;
        return rc;
    }
    *out = h;
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

int cozk_shamir_gp_msgs(const cozk_shamir_gp* h, uint64_t* out, size_t cap) {
    if (!h || !out || cap < h->msgs.size()) return COZK_ERR_INVALID_ARG;
    for (size_t k = 0; k < h->msgs.size(); k++) fe_to_u64x4(h->msgs[k], out + 4 * k);
    return COZK_OK;
}

int cozk_shamir_gp_finals(const cozk_shamir_gp* h, uint64_t* out, size_t cap) {
    if (!h || !out || cap < h->finals.size()) return COZK_ERR_INVALID_ARG;
    for (size_t k = 0; k < h->finals.size(); k++) fe_to_u64x4(h->finals[k], out + 4 * k);
    return COZK_OK;
}

}  // extern "C"
