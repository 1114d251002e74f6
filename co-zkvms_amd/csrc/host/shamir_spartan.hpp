// co-noir-spartan (BASELINE config 4, spartan_harness.hpp) proved by n Shamir parties, all driven from the one thread that owns their
// contexts and plays the coordinator, as the Shamir grand products are (shamir_gp.hpp).  The reference has no Shamir prover;
// tests/shamir_spartan_ref.py restates this file in big integers.  Included by harness.hip behind spartan_harness.hpp and
// shamir_harness.hpp (the handle base, the keys and the dealing, ShamirProve: the openings, the masks).
//
// Why the PLAIN kernels serve: every step of the worker is linear in the witness share or multiplies at most two secret factors.
//   zero_round       public CSR matrices times shared z: degree-t sharings of Az, Bz, Cz (cozk_sparse_matvec3 per sender)
//   commit, z(ry),   linear in z: parties 0..t run the PLAIN calls on their shares, scalars are combined with lagrange(1..t + 1), G1
//   PST13::open      points with cozk_shamir_combine_points
//   first sumcheck   sum_x eq(tau, x) (Az(x) Bz(x) - Cz(x)): eq is public, Az Bz is ONE product of two shares and a degree-t share of
//                    Cz lies on a polynomial of degree <= 2t, so g(0..3) computed by a party on its shares is a degree-2t share of the
//                    plain message: opened from senders 0..2t behind a degree-2t zero mask, as the grand product's coefficients are
//   second sumcheck  sum_y z(y) (alpha A(rx, y) + beta B(rx, y) + gamma C(rx, y)): the matrices are public, the message is a degree-t
//                    sharing, opened from parties 0..t unmasked, as the grand product's final claims are
// So the proof is the plain prover's, byte for byte (oracle/pyspartan.py, SpartanHarness(mode = plain)), accepted by spartan_verify.
//
//   masks     M = 4 log_n openings of degree 2t (ShamirProve::deal_masks at rand_counter), m = 4 round + evaluation index: (rand keys,
//             rand_counter .. + M) must not be used again.
//   grouped   when the senders' contexts are on one device (shamir_gp_grouped; COZK_SHAMIR_GP_GROUP=0 switches it off, read on every call):
//             the first sumcheck is ONE cozk_spartan_group (FIRST) over the 2t + 1 senders with one eq on sender 0's context, the second
//             ONE group (SECOND) over copies of the shares of parties 0..t against lin = alpha A + beta B + gamma C formed once; A, B,
//             C(rx, ry) are one public evaluation at ry behind the rounds.  Otherwise every sender runs the per-poly calls -- the rounds
//             loop of rep3_first_sumcheck_worker / rep3_second_sumcheck_worker in PLAIN mode without the star -- with an eq and matrix
//             columns of its own.  Same bytes either way.
// Semi-honest.  Not built: the public lookup round (cfg.lookup_round of the Rep3 harness), one party per process, senders spread over
// several GPUs as groups, a king variant (there is no secret-by-secret multiplication to reshare, so a king has nothing to do).
#pragma once

// finals: za, zb, zc(rx); log_n x 3 second-sumcheck evaluations; z's final value; z(ry)
struct cozk_shamir_spartan : cozk::ShamirHarness {
    cozk_shamir_spartan_config cfg;
    cozk_spartan inst;  // the instance of (seed, log_n) and the verifier's view; inst.parties[p] = party p (CSR, SRS: senders only)
    std::vector<cozk::VecH> zvec;  // party p's share vector of z, a vector of its context
};

namespace {

typedef Handle<cozk_spartan_group, cozk_spartan_group_free> SpartanGroupH;

static g1_affine shamir_spartan_combine_points(cozk_ctx* ctx, const std::vector<g1_affine>& pts, int t) {
    const size_t k = pts.size();
    std::vector<uint64_t> xy(8 * k);
    std::vector<int> inf(k);
    std::vector<uint32_t> at(k);
    for (size_t p = 0; p < k; p++) {
        fe_to_u64x4(pts[p].x, xy.data() + 8 * p);
        fe_to_u64x4(pts[p].y, xy.data() + 8 * p + 4);
        inf[p] = G1::is_inf(pts[p]) ? 1 : 0;
        at[p] = (uint32_t)p + 1;
    }
    uint64_t out[8];
    int oinf = 0;
    rc_check(cozk_shamir_combine_points(ctx, xy.data(), inf.data(), at.data(), k, t, out, &oinf), ctx, "shamir_combine_points");
    return abi_to_g1(out, oinf);
}

static void shamir_spartan_bind(cozk_ctx* ctx, std::initializer_list<cozk_poly*> polys, const uint64_t rr[4]) {
    for (cozk_poly* p : polys) rc_check(cozk_poly_bind(ctx, p, rr, COZK_LOW_TO_HIGH), ctx, "fix_variables");
}
static fe shamir_spartan_coeff0(cozk_ctx* ctx, const cozk_poly* p) {
    uint64_t a[4], b[4];
    rc_check(cozk_poly_get_coeff(ctx, p, 0, a, b), ctx, "get_coeff");
    return fe_from_u64x4(a);
}

static void shamir_spartan_prove(cozk_shamir_spartan* h, bool verify, cozk_shamir_spartan_result* res) {
    ShamirProve sp(h, verify);
    const int t = sp.t, nv = h->cfg.log_n, senders = sp.senders, openers = sp.openers;
    const std::vector<cozk_ctx*>& pcs = sp.pcs;
    cozk_ctx* const c0 = sp.c0;
    const bool grouped = sp.grouped;
    auto set_dev = [&](int p) { sp.set_dev(p); };
    auto open_t = [&](const fe* sh) { return sp.open_t(sh); };
    SpartanProof pf;
    sp.sync_all();
    const double t0 = now_ms();
    // ---- zero_round, per sender on its share
    std::vector<PolyH> za((size_t)senders), zb((size_t)senders), zc((size_t)senders);
    for (int p = 0; p < senders; p++) {
        SpartanParty& ps = h->inst.parties[(size_t)p];
        set_dev(p);
        rc_check(cozk_sparse_matvec3(pcs[(size_t)p], ps.row_ptr.h, ps.col.h, ps.va.h, ps.vb.h, ps.vc.h, ps.z.h, &za[(size_t)p].h, &zb[(size_t)p].h, &zc[(size_t)p].h),
                 pcs[(size_t)p], "zero_round");
    }
    sp.sync_all();
    const double t1 = now_ms();
    // ---- commit: parties 0..t commit to their share, the points are combined with lagrange(1..t + 1)
    Transcript tr("cozk-spartan");
    {
        std::vector<g1_affine> pts;
        for (int p = 0; p < openers; p++) {
            set_dev(p);
            pts.push_back(PST13::batch_commit(pcs[(size_t)p], *h->inst.parties[(size_t)p].setup, {h->zvec[(size_t)p].h})[0].g_product);
        }
        pf.cz = PST13Commitment{(uint64_t)nv, shamir_spartan_combine_points(c0, pts, t)};
        tr.append_point(pf.cz.g_product);
    }
    const std::vector<fe> tau = tr.challenge_vector(nv);
    const double t2 = now_ms();
    // ---- masks
    const size_t M = (size_t)4 * (size_t)nv;
    sp.deal_masks(h->cfg.rand_counter, M);
    const double t3 = now_ms();
    // ---- first sumcheck
    std::vector<fe> rx, ry;
    uint64_t rr[4];
    fe eq_final;
    {
        std::vector<PolyH> eqs((size_t)(grouped ? 1 : senders));
        for (size_t p = 0; p < eqs.size(); p++) {
            set_dev((int)p);
            VecH eqv = eq_le_device(pcs[p], tau);
            eqs[p] = plain_poly(pcs[p], eqv);
        }
        SpartanGroupH g;
        if (grouped) {
            std::vector<cozk_poly*> planes;
            for (int p = 0; p < senders; p++)
                for (cozk_poly* q : {za[(size_t)p].h, zb[(size_t)p].h, zc[(size_t)p].h}) planes.push_back(q);
            set_dev(0);
            rc_check(cozk_spartan_group_create(c0, COZK_SPARTAN_GROUP_FIRST, planes.data(), senders, eqs[0].h, &g.h), c0, "spartan_group_create");
        }
        std::vector<uint64_t> ev((size_t)16 * senders);
        for (int j = 0; j < nv; j++) {
            if (grouped) {
                rc_check(cozk_spartan_group_round(g.h, j ? rr : nullptr, ev.data()), c0, "spartan_group_round");
                h->stats.group_rounds++;
            } else {
                for (int p = 0; p < senders; p++) {
                    cozk_ctx* c = pcs[(size_t)p];
                    set_dev(p);
                    if (j) shamir_spartan_bind(c, {za[(size_t)p].h, zb[(size_t)p].h, zc[(size_t)p].h, eqs[(size_t)p].h}, rr);
                    rc_check(cozk_spartan_first_round(c, za[(size_t)p].h, zb[(size_t)p].h, zc[(size_t)p].h, eqs[(size_t)p].h, ev.data() + 16 * p), c, "spartan_first_round");
                    h->stats.single_rounds++;
                }
            }
            std::vector<fe> msg(4);
            for (int e = 0; e < 4; e++) msg[(size_t)e] = sp.open_2t(ev.data() + 4 * e, 16, (size_t)(4 * j + e));
            tr.append_scalars(msg);
            const fe r = tr.challenge_scalar();
            rx.push_back(r);
            fe_to_u64x4(r, rr);
            pf.sc1.push_back(msg);
        }
        // the last bind; za, zb, zc(rx) from the openers, eq(tau, rx) is public
        fe fin[3][COZK_SHAMIR_MAX_PARTIES];
        if (grouped) {
            std::vector<uint64_t> out((size_t)4 * (3 * openers + 1));
            rc_check(cozk_spartan_group_final(g.h, rr, openers, out.data()), c0, "spartan_group_final");
            h->stats.group_finals++;
            for (int p = 0; p < openers; p++)
                for (int i = 0; i < 3; i++) fin[i][p] = fe_from_u64x4(out.data() + 4 * (3 * p + i));
            eq_final = fe_from_u64x4(out.data() + 4 * (3 * openers));
        } else {
            for (int p = 0; p < openers; p++) {
                cozk_ctx* c = pcs[(size_t)p];
                set_dev(p);
                shamir_spartan_bind(c, {za[(size_t)p].h, zb[(size_t)p].h, zc[(size_t)p].h, eqs[(size_t)p].h}, rr);
                fin[0][p] = shamir_spartan_coeff0(c, za[(size_t)p].h);
                fin[1][p] = shamir_spartan_coeff0(c, zb[(size_t)p].h);
                fin[2][p] = shamir_spartan_coeff0(c, zc[(size_t)p].h);
                if (p == 0) eq_final = shamir_spartan_coeff0(c, eqs[0].h);
                h->stats.single_finals++;
            }
        }
        for (int i = 0; i < 3; i++) pf.sc1_finals.push_back(open_t(fin[i]));
        pf.sc1_finals.push_back(eq_final);
        g = SpartanGroupH();
        sp.release(za, zb, zc);
        sp.release(eqs);
    }
    tr.append_scalars({pf.sc1_finals[0], pf.sc1_finals[1], pf.sc1_finals[2]});
    const std::vector<fe> abc = tr.challenge_vector(3);
    sp.sync_all();
    const double t4 = now_ms();
    // ---- A(rx, .), B(rx, .), C(rx, .): public, the transposed mat-vec with eq(rx, .); grouped: ONCE on sender 0's context
    const int builders = grouped ? 1 : openers;
    std::vector<PolyH> arx((size_t)builders), brx((size_t)builders), crx((size_t)builders);
    for (int p = 0; p < builders; p++) {
        SpartanParty& ps = h->inst.parties[(size_t)p];
        cozk_ctx* c = pcs[(size_t)p];
        set_dev(p);
        VecH eqrx = eq_le_device(c, rx);
        PolyH eqp = plain_poly(c, eqrx);
        rc_check(cozk_sparse_matvec3(c, ps.t_ptr.h, ps.t_row.h, ps.t_va.h, ps.t_vb.h, ps.t_vc.h, eqp.h, &arx[(size_t)p].h, &brx[(size_t)p].h, &crx[(size_t)p].h), c,
                 "A(rx,.) build");
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const double t5 = now_ms();
    // ---- second sumcheck on copies of the openers' shares: the witness stays for the opening
    {
        std::vector<PolyH> zw((size_t)openers);
        for (int p = 0; p < openers; p++) {
            set_dev(p);
            zw[(size_t)p] = plain_poly(pcs[(size_t)p], h->zvec[(size_t)p]);
        }
        uint64_t cf[12];
        for (int i = 0; i < 3; i++) fe_to_u64x4(abc[(size_t)i], cf + 4 * i);
        SpartanGroupH g;
        if (grouped) {
            set_dev(0);
            const cozk_poly* cols[3] = {arx[0].h, brx[0].h, crx[0].h};
            PolyH lin;
            rc_check(cozk_poly_linear_combination(c0, cols, cf, 3, COZK_MODE_PLAIN, 0, &lin.h), c0, "lin = alpha A + beta B + gamma C");
            std::vector<cozk_poly*> planes;
            for (int p = 0; p < openers; p++) planes.push_back(zw[(size_t)p].h);
            rc_check(cozk_spartan_group_create(c0, COZK_SPARTAN_GROUP_SECOND, planes.data(), openers, lin.h, &g.h), c0, "spartan_group_create");
        }
        std::vector<uint64_t> ev((size_t)12 * openers), unused(12);
        for (int j = 0; j < nv; j++) {
            if (grouped) {
                rc_check(cozk_spartan_group_round(g.h, j ? rr : nullptr, ev.data()), c0, "spartan_group_round");
                h->stats.group_rounds++;
            } else {
                for (int p = 0; p < openers; p++) {
                    cozk_ctx* c = pcs[(size_t)p];
                    set_dev(p);
                    if (j) shamir_spartan_bind(c, {zw[(size_t)p].h, arx[(size_t)p].h, brx[(size_t)p].h, crx[(size_t)p].h}, rr);
                    rc_check(cozk_spartan_second_round(c, zw[(size_t)p].h, arx[(size_t)p].h, brx[(size_t)p].h, crx[(size_t)p].h, cf, ev.data() + 12 * p, unused.data()), c,
                             "spartan_second_round");
                    h->stats.single_rounds++;
                }
            }
            std::vector<fe> msg(3);
            for (int e = 0; e < 3; e++) {
                fe sh[COZK_SHAMIR_MAX_PARTIES];
                for (int p = 0; p < openers; p++) sh[p] = fe_from_u64x4(ev.data() + 12 * p + 4 * e);
                msg[(size_t)e] = open_t(sh);
            }
            tr.append_scalars(msg);
            const fe r = tr.challenge_scalar();
            ry.push_back(r);
            fe_to_u64x4(r, rr);
            pf.sc2.push_back(msg);
        }
        fe zf[COZK_SHAMIR_MAX_PARTIES], mat[3];
        if (grouped) {
            std::vector<uint64_t> out((size_t)4 * (openers + 1));
            rc_check(cozk_spartan_group_final(g.h, rr, openers, out.data()), c0, "spartan_group_final");
            h->stats.group_finals++;
            for (int p = 0; p < openers; p++) zf[p] = fe_from_u64x4(out.data() + 4 * p);
            // A, B, C(rx, ry): one public evaluation at ry of the columns the rounds never bound
            set_dev(0);
            VecH chi = eq_le_device(c0, ry);
            const cozk_poly* cols[3] = {arx[0].h, brx[0].h, crx[0].h};
            uint64_t m3[12];
            rc_check(cozk_poly_batch_evaluate_at_chi(c0, cols, 3, chi.h, m3), c0, "A, B, C(rx, ry)");
            for (int i = 0; i < 3; i++) mat[i] = fe_from_u64x4(m3 + 4 * i);
        } else {
            for (int p = 0; p < openers; p++) {
                cozk_ctx* c = pcs[(size_t)p];
                set_dev(p);
                shamir_spartan_bind(c, {zw[(size_t)p].h, arx[(size_t)p].h, brx[(size_t)p].h, crx[(size_t)p].h}, rr);
                zf[p] = shamir_spartan_coeff0(c, zw[(size_t)p].h);
                if (p == 0) {
                    mat[0] = shamir_spartan_coeff0(c, arx[0].h);
                    mat[1] = shamir_spartan_coeff0(c, brx[0].h);
                    mat[2] = shamir_spartan_coeff0(c, crx[0].h);
                }
                h->stats.single_finals++;
            }
        }
        pf.sc2_finals.push_back(open_t(zf));
        for (int i = 0; i < 3; i++) pf.sc2_finals.push_back(mat[i]);
        g = SpartanGroupH();
        sp.release(zw);
        sp.release(arx, brx, crx);
    }
    sp.sync_all();
    const double t6 = now_ms();
    // ---- z(ry) and the opening, per opener on its share
    {
        fe ze[COZK_SHAMIR_MAX_PARTIES];
        std::vector<std::vector<g1_affine>> open_p((size_t)openers);
        for (int p = 0; p < openers; p++) {
            cozk_ctx* c = pcs[(size_t)p];
            SpartanParty& ps = h->inst.parties[(size_t)p];
            set_dev(p);
            VecH chi = eq_le_device(c, ry);
            uint64_t v[4];
            const cozk_poly* arr[1] = {ps.z.h};
            rc_check(cozk_poly_batch_evaluate_at_chi(c, arr, 1, chi.h, v), c, "eval z(ry)");
            ze[p] = fe_from_u64x4(v);
            open_p[(size_t)p] = PST13::open(c, *ps.setup, h->zvec[(size_t)p].h, ry);
        }
        pf.z_eval = open_t(ze);
        for (int i = 0; i < nv; i++) {
            std::vector<g1_affine> pts;
            for (int p = 0; p < openers; p++) pts.push_back(open_p[(size_t)p][(size_t)i]);
            pf.opening.push_back(shamir_spartan_combine_points(c0, pts, t));
        }
    }
    sp.sync_all();
    const double t7 = now_ms();
    res->verified = -1;
    if (verify) {
        std::string why;
        res->verified = spartan_verify(&h->inst, pf, why) ? 1 : 0;
        if (!res->verified) h->error = "verification failed: " + why;
    }
    res->grouped = grouped ? 1 : 0;
    res->n_opened = M;
    res->wall_ms = t7 - t0;
    res->t_zero_round_ms = t1 - t0;
    res->t_commit_ms = t2 - t1;
    res->t_masks_ms = t3 - t2;
    res->t_sumcheck1_ms = t4 - t3;
    res->t_matrix_build_ms = t5 - t4;
    res->t_sumcheck2_ms = t6 - t5;
    res->t_open_ms = t7 - t6;
    finish_proof(h, pf.serialize(), res);
}

static void shamir_spartan_release(cozk_shamir_spartan* h) {
    for (size_t p = 0; p < h->inst.parties.size(); p++) {
        SpartanParty& ps = h->inst.parties[p];
        if (ps.ctx) (void)hipSetDevice(ps.ctx->device);
        if (p < h->zvec.size()) h->zvec[p] = VecH();
    }
    release_parties(h->inst.parties, [](SpartanParty& ps) {
        ps.z = PolyH();
        for (VecH* v : {&ps.row_ptr, &ps.col, &ps.va, &ps.vb, &ps.vc, &ps.t_ptr, &ps.t_row, &ps.t_va, &ps.t_vb, &ps.t_vc}) *v = VecH();
        ps.setup.reset();
    });
}

}  // namespace

extern "C" {

int cozk_shamir_spartan_create(const cozk_shamir_spartan_config* cfg, cozk_shamir_spartan** out) {
    return harness_create(cfg, out, [&](cozk_shamir_spartan* h) {
        const std::string w = "shamir_spartan";
        shamir_gp_require_parties(w, cfg->degree, cfg->num_parties);
        COZK_REQUIRE(cfg->log_n >= 1 && cfg->log_n <= 24, w + ": log_n out of range (1..24)");
        const int t = h->t = cfg->degree, n = h->n = cfg->num_parties, senders = 2 * t + 1;
        cozk_spartan_config& ic = h->inst.cfg;
        memset(&ic, 0, sizeof ic);
        ic.mode = COZK_MODE_PLAIN;
        ic.log_n = cfg->log_n;
        ic.precompute = cfg->precompute;
        ic.seed = cfg->seed;
        h->inst.nparties = n;
        h->inst.n = (size_t)1 << cfg->log_n;
        std::vector<fe> z_plain;
        spartan_build_instance(&h->inst, z_plain);
        h->inst.parties.resize((size_t)n);
        for (int p = 0; p < n; p++) {
            SpartanParty& ps = h->inst.parties[(size_t)p];
            ps.party = p;
            ps.open_ctx(cfg->devices[p], "shamir_spartan: cannot create a context (no HIP device?)");
            h->pcs.push_back(ps.ctx);
            // the public instance and the SRS: the senders run zero_round, the openers among them commit and open
            if (p < senders) spartan_setup_party(&h->inst, ps, z_plain);
        }
        // the witness: degree-t shares dealt once, party p's as a vector and a PLAIN polynomial of its own context
        const std::vector<uint8_t> skeys = shamir_harness_keys(h, cfg->seed);
        HIP_TRY(hipSetDevice(h->pcs[0]->device));
        VecH zv = upload_fe(h->pcs[0], z_plain);
        std::vector<PolyH> z = shamir_deal_column(h, zv, skeys, cfg->share_counter, n, &h->zvec);
        for (int p = 0; p < n; p++) h->inst.parties[(size_t)p].z = std::move(z[(size_t)p]);
    });
}

const char* cozk_shamir_spartan_error(const cozk_shamir_spartan* h) { return harness_error(h); }

int cozk_shamir_spartan_destroy(cozk_shamir_spartan* h) {
    if (!h) return COZK_OK;
    shamir_spartan_release(h);
    delete h;
    return COZK_OK;
}

int cozk_shamir_spartan_prove(cozk_shamir_spartan* h, int verify, cozk_shamir_spartan_result* res) {
    return shamir_harness_prove(
        h, res, "shamir_spartan", [](const cozk_shamir_spartan* x) { return (int)x->inst.parties.size() == x->n && x->zvec.size() == (size_t)x->n; },
        [&](cozk_shamir_spartan* x, cozk_shamir_spartan_result* r) { shamir_spartan_prove(x, verify != 0, r); });
}

int cozk_shamir_spartan_proof_bytes(const cozk_shamir_spartan* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

size_t cozk_shamir_spartan_msgs_len(const cozk_shamir_spartan* h) { return h ? h->msgs.size() : 0; }
size_t cozk_shamir_spartan_finals_len(const cozk_shamir_spartan* h) { return h ? h->finals.size() : 0; }

int cozk_shamir_spartan_msgs(const cozk_shamir_spartan* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->msgs : nullptr, out, cap); }
int cozk_shamir_spartan_finals(const cozk_shamir_spartan* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->finals : nullptr, out, cap); }
int cozk_shamir_spartan_get_stats(const cozk_shamir_spartan* h, cozk_shamir_gp_stats* stats) { return shamir_harness_stats(h, stats); }

}  // extern "C"
