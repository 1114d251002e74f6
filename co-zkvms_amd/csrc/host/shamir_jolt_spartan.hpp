// co-jolt's Spartan worker (Rep3UniformSpartanProver::prove, spartan_jolt.hpp; BASELINE's co-jolt configuration) proved by n Shamir
// parties, all driven from the one thread that owns their contexts and plays the coordinator, as co-noir-spartan is
// (shamir_spartan.hpp).  The reference has no Shamir prover; tests/shamir_jolt_spartan_ref.py restates this file in big integers.
// Included by harness.hip behind outer_harness.hpp (the instance, the verifier's view) and shamir_harness.hpp (the handle base, the keys
// and the dealing, ShamirProve: the openings, the masks).
//
// Why the PLAIN kernels serve: every step of the worker is linear in the witness share or multiplies exactly two secret factors.
//   Az, Bz, Cz       affine in the witness columns; a constant or a public column is the constant sharing, added to every party's value
//                    (k_r1cs_rows in PLAIN mode does that): degree-t sharings
//   outer sumcheck   the message is linear in (t(0), t(inf), claim) once l0, l1 are public; t(0), t(inf) are sums of eq (Az Bz - Cz)
//                    terms: degree 2t; the running claim is public once opened and is every sender's hint.  In the first round every
//                    party sets t(0) = 0, as the plain kernel does: the Lagrange combination is the plain prover's 0.  Opened from
//                    senders 0..2t behind a degree-2t zero mask; Az, Bz, Cz(r) from parties 0..t, unmasked
//   inner sumcheck   sum_y ABC(y) z(y) with ABC public: degree t.  On the host (4 V <= 512 entries), parties 0..t, from ONE
//                    cozk_poly_batch_dot_public per party; the constant column of z is 1 at every party
//   shift sumcheck   sum_t z_ry(t) eq_plus_one(rx_step, t): degree t, parties 0..t; shift_claim is opened and not appended to the transcript
//   claim exchanges  two batch evaluations, linear: degree t, every column's value opened from parties 0..t (a public column's opens to itself)
// Every party's running claim is the opened, public one (the plain worker's own additive claim is that value).  So the proof is the plain
// prover's, byte for byte (OuterHarness(mode = plain, full = 1), oracle/pyspartan_outer.py run_full), accepted by verify_spartan.
//
//   masks     M = 4 (steps_bits + constr_bits) openings of degree 2t (ShamirProve::deal_masks at rand_counter), m = 4 round + coefficient.
//   grouped   when the senders' contexts are on one device (shamir_gp_grouped; COZK_SHAMIR_GP_GROUP=0 switches it off, read on every
//             call): the outer sumcheck is ONE cozk_outer_group over the 2t + 1 senders on sender 0's context, the shift sumcheck ONE
//             cozk_shift_group over the openers' z_ry against one eq_plus_one.  Otherwise every sender runs cozk_outer_round /
//             cozk_prod_sumcheck_evals + cozk_poly_bind.  Same bytes either way.
// Semi-honest.  The Lasso primary sumcheck has a Shamir prover of its own (shamir_primary.hpp).  Not built: one party per process,
// groups over several GPUs.
#pragma once

struct cozk_shamir_jolt_spartan : cozk::ShamirHarness {
    cozk_shamir_jolt_spartan_config cfg;
    cozk_outer_harness inst;  // the outer harness's instance of (seed, log_steps, system) and the verifier's view; it has no parties here
    std::vector<cozk::HarnessParty> parties;
    std::vector<std::vector<cozk::PolyH>> cols;  // [p][v]: party p's column v (public columns: the clear values), PLAIN, of its context
};

namespace {

typedef Handle<cozk_outer_group, cozk_outer_group_free> OuterGroupH;
typedef Handle<cozk_shift_group, cozk_shift_group_free> ShiftGroupH;

static void shamir_jolt_spartan_prove(cozk_shamir_jolt_spartan* h, bool verify, cozk_shamir_jolt_spartan_result* res) {
    ShamirProve sp(h, verify);
    const int senders = sp.senders, openers = sp.openers;
    const jolt::System& sys = h->inst.sys;
    const size_t N = h->inst.N, V = spartan_vars_padded(sys), nvars = (size_t)h->inst.ncols;
    const int steps_bits = h->cfg.log_steps, constr_bits = ceil_log2(sys.padded), n_tau = steps_bits + constr_bits;
    const std::vector<cozk_ctx*>& pcs = sp.pcs;
    cozk_ctx* const c0 = sp.c0;
    const bool grouped = sp.grouped;
    auto set_dev = [&](int p) { sp.set_dev(p); };
    auto open_t = [&](const fe* sh) { return sp.open_t(sh); };
    auto col_ptrs = [&](int p) {
        std::vector<const cozk_poly*> cc;
        for (const PolyH& c : h->cols[(size_t)p]) cc.push_back(c.h);
        return cc;
    };
    JoltSpartanProof pf;
    sp.sync_all();
    const double t0 = now_ms();
    Transcript tr("cozk-spartan");
    const std::vector<fe> tau = tr.challenge_vector((size_t)n_tau);
    // ---- Az, Bz, Cz per sender on its columns
    std::vector<OuterH> st((size_t)senders);
    {
        const std::vector<uint64_t> w = to_abi(tau);
        for (int p = 0; p < senders; p++) {
            set_dev(p);
            const std::vector<const cozk_poly*> cc = col_ptrs(p);
            rc_check(cozk_outer_create(pcs[(size_t)p], COZK_MODE_PLAIN, 0, &sys.desc, cc.data(), cc.size(), w.data(), tau.size(), &st[(size_t)p].h), pcs[(size_t)p],
                     "outer_create");
        }
    }
    sp.sync_all();
    const double t1 = now_ms();
    // ---- masks
    const size_t M = (size_t)4 * (size_t)n_tau;
    sp.deal_masks(h->cfg.rand_counter, M);
    const double t2 = now_ms();
    // ---- outer sumcheck
    std::vector<fe> outer_rs;
    uint64_t rr[4];
    {
        OuterGroupH g;
        if (grouped) {
            std::vector<cozk_outer*> members;
            for (int p = 0; p < senders; p++) members.push_back(st[(size_t)p].h);
            set_dev(0);
            rc_check(cozk_outer_group_create(c0, members.data(), senders, &g.h), c0, "outer_group_create");
        }
        fe claim = Fr::zero();
        std::vector<uint64_t> cf((size_t)16 * senders), cl((size_t)4 * senders);
        for (int j = 0; j < n_tau; j++) {
            for (int p = 0; p < senders; p++) fe_to_u64x4(claim, cl.data() + 4 * p);  // the opened claim is every sender's hint
            if (grouped) {
                rc_check(cozk_outer_group_round(g.h, j ? rr : nullptr, cl.data(), cf.data()), c0, "outer_group_round");
                h->stats.group_rounds++;
            } else {
                for (int p = 0; p < senders; p++) {
                    set_dev(p);
                    rc_check(cozk_outer_round(pcs[(size_t)p], st[(size_t)p].h, j ? rr : nullptr, cl.data() + 4 * p, cf.data() + 16 * p), pcs[(size_t)p], "outer_round");
                    h->stats.single_rounds++;
                }
            }
            std::vector<fe> poly(4);
            for (int i = 0; i < 4; i++) poly[(size_t)i] = sp.open_2t(cf.data() + 4 * i, 16, (size_t)(4 * j + i));
            const std::vector<fe> comp = unipoly_compress(poly);
            tr.append_scalars(comp);
            const fe r = tr.challenge_scalar();
            outer_rs.push_back(r);
            fe_to_u64x4(r, rr);
            claim = unipoly_eval(poly, r);
            pf.outer.compressed_polys.push_back(comp);
        }
        // the last bind; Az, Bz, Cz(r) from the openers
        fe fin[3][COZK_SHAMIR_MAX_PARTIES];
        std::vector<uint64_t> out((size_t)12 * openers);
        if (grouped) {
            rc_check(cozk_outer_group_final(g.h, rr, openers, out.data()), c0, "outer_group_final");
            h->stats.group_finals++;
        } else {
            for (int p = 0; p < openers; p++) {
                set_dev(p);
                rc_check(cozk_outer_final_evals(pcs[(size_t)p], st[(size_t)p].h, rr, out.data() + 12 * p), pcs[(size_t)p], "outer_final_evals");
                h->stats.single_finals++;
            }
        }
        for (int p = 0; p < openers; p++)
            for (int q = 0; q < 3; q++) fin[q][p] = fe_from_u64x4(out.data() + 12 * p + 4 * q);
        for (int q = 0; q < 3; q++) pf.outer.claims.push_back(open_t(fin[q]));
        tr.append_scalars(pf.outer.claims);
        g = OuterGroupH();
        sp.release(st);
    }
    sp.sync_all();
    const double t3 = now_ms();
    // ---- inner sumcheck, on the host
    const std::vector<fe> outer_r(outer_rs.rbegin(), outer_rs.rend());
    const std::vector<fe> rx_step(outer_r.begin(), outer_r.begin() + steps_bits), rx_constr(outer_r.begin() + steps_bits, outer_r.end());
    const fe rlc = tr.challenge_scalar();
    fe claim = Fr::add(pf.outer.claims[0], Fr::add(Fr::mul(rlc, pf.outer.claims[1]), Fr::mul(Fr::mul(rlc, rlc), pf.outer.claims[2])));
    std::vector<VecH> eq_step((size_t)openers), eqp1_step((size_t)openers);
    std::vector<std::vector<fe>> z((size_t)openers, std::vector<fe>(4 * V, Fr::zero()));  // bind_z (2 V) then bind_shift_z (2 V)
    {
        const std::vector<uint64_t> rxs = to_abi(rx_step);
        for (int p = 0; p < openers; p++) {
            cozk_ctx* c = pcs[(size_t)p];
            set_dev(p);
            rc_check(cozk_eq_evals(c, rxs.data(), steps_bits, &eq_step[(size_t)p].h), c, "eq_evals(rx_step)");
            rc_check(cozk_eq_plus_one_evals(c, rxs.data(), steps_bits, &eqp1_step[(size_t)p].h), c, "eq_plus_one_evals(rx_step)");
            const cozk_vec* pubs[2] = {eq_step[(size_t)p].h, eqp1_step[(size_t)p].h};
            const std::vector<const cozk_poly*> cc = col_ptrs(p);
            std::vector<uint64_t> dots(cc.size() * 2 * 8);
            rc_check(cozk_poly_batch_dot_public(c, cc.data(), cc.size(), pubs, 2, dots.data()), c, "batch_dot_public");
            for (size_t i = 0; i < cc.size(); i++)
                for (int q = 0; q < 2; q++) z[(size_t)p][(size_t)q * 2 * V + i] = fe_from_u64x4(dots.data() + (i * 2 + q) * 8);
            z[(size_t)p][V] = Fr::one();  // bind_z[num_vars_uniform] = 1: the constant sharing
        }
    }
    std::vector<fe> inner_r;
    {
        std::vector<fe> abc = spartan_matrix_mle_partial(sys, rx_constr, rlc);
        const int rounds = ceil_log2(4 * V);
        for (int round = 0; round < rounds; round++) {
            const size_t half = abc.size() / 2;
            fe e02[COZK_SHAMIR_MAX_PARTIES][2];
            for (int p = 0; p < openers; p++) {  // sumcheck_evals(i, 2, HighToLow) of both polynomials, comb_func, sum
                const std::vector<fe>& zp = z[(size_t)p];
                fe e0 = Fr::zero(), e2 = Fr::zero();
                for (size_t i = 0; i < half; i++) {
                    e0 = Fr::add(e0, Fr::mul(abc[i], zp[i]));
                    const fe a2 = Fr::sub(Fr::dbl(abc[i + half]), abc[i]), z2 = Fr::sub(Fr::dbl(zp[i + half]), zp[i]);
                    e2 = Fr::add(e2, Fr::mul(a2, z2));
                }
                e02[p][0] = e0;
                e02[p][1] = e2;
            }
            const fe r_j = sp.open_quadratic(e02, claim, pf.inner.compressed_polys, tr);
            inner_r.push_back(r_j);
            for (size_t i = 0; i < half; i++) abc[i] = Fr::add(abc[i], Fr::mul(Fr::sub(abc[i + half], abc[i]), r_j));
            abc.resize(half);
            for (int p = 0; p < openers; p++) {
                std::vector<fe>& zp = z[(size_t)p];
                for (size_t i = 0; i < half; i++) zp[i] = Fr::add(zp[i], Fr::mul(Fr::sub(zp[i + half], zp[i]), r_j));
                zp.resize(half);
            }
        }
    }
    const double t4 = now_ms();
    // ---- shift sumcheck
    std::vector<fe> shift_r;
    {
        const std::vector<fe> ry_var(inner_r.begin() + 1, inner_r.end());
        const std::vector<fe> eq_ry = eq_evals_host(ry_var);
        const std::vector<uint64_t> cfa = to_abi(std::vector<fe>(eq_ry.begin(), eq_ry.begin() + (long)nvars));
        std::vector<PolyH> zry((size_t)openers);
        fe sc[COZK_SHAMIR_MAX_PARTIES];
        for (int p = 0; p < openers; p++) {
            cozk_ctx* c = pcs[(size_t)p];
            set_dev(p);
            const std::vector<const cozk_poly*> cc = col_ptrs(p);
            rc_check(cozk_poly_linear_combination(c, cc.data(), cfa.data(), cc.size(), COZK_MODE_PLAIN, 0, &zry[(size_t)p].h), c, "bind_z_ry_var");
            uint64_t cl[4];
            const cozk_poly* one_poly[1] = {zry[(size_t)p].h};
            rc_check(cozk_poly_batch_evaluate_at_chi(c, one_poly, 1, eqp1_step[(size_t)p].h, cl), c, "shift_sumcheck_claim");
            sc[p] = fe_from_u64x4(cl);
        }
        pf.shift_claim = claim = open_t(sc);  // not appended to the transcript (coordinator.rs:113-117)
        if (steps_bits > 0) {
            std::vector<PolyH> ep((size_t)(grouped ? 1 : openers));
            for (size_t p = 0; p < ep.size(); p++) {
                set_dev((int)p);
                ep[p] = plain_poly(pcs[p], eqp1_step[p]);
            }
            ShiftGroupH g;
            if (grouped) {
                std::vector<cozk_poly*> members;
                for (int p = 0; p < openers; p++) members.push_back(zry[(size_t)p].h);
                set_dev(0);
                rc_check(cozk_shift_group_create(c0, members.data(), openers, ep[0].h, &g.h), c0, "shift_group_create");
            }
            std::vector<uint64_t> ev((size_t)8 * openers);
            for (int j = 0; j < steps_bits; j++) {
                if (grouped) {
                    rc_check(cozk_shift_group_round(g.h, j ? rr : nullptr, ev.data()), c0, "shift_group_round");
                    h->stats.group_rounds++;
                } else {
                    for (int p = 0; p < openers; p++) {
                        cozk_ctx* c = pcs[(size_t)p];
                        set_dev(p);
                        const cozk_poly* pair[2] = {zry[(size_t)p].h, ep[(size_t)p].h};
                        if (j)
                            for (cozk_poly* q : {zry[(size_t)p].h, ep[(size_t)p].h}) rc_check(cozk_poly_bind(c, q, rr, COZK_HIGH_TO_LOW), c, "bind");
                        rc_check(cozk_prod_sumcheck_evals(c, pair, 2, 2, ev.data() + 8 * p), c, "prod_sumcheck_evals");
                        h->stats.single_rounds++;
                    }
                }
                fe e02[COZK_SHAMIR_MAX_PARTIES][2];
                for (int p = 0; p < openers; p++)
                    for (int e = 0; e < 2; e++) e02[p][e] = fe_from_u64x4(ev.data() + 8 * p + 4 * e);
                const fe r_j = sp.open_quadratic(e02, claim, pf.shift.compressed_polys, tr);
                shift_r.push_back(r_j);
                fe_to_u64x4(r_j, rr);
            }
            // the last bind, as prove_arbitrary_worker leaves its polynomials (their final values are not part of the proof)
            if (grouped) {
                std::vector<uint64_t> out((size_t)4 * (openers + 1));
                rc_check(cozk_shift_group_final(g.h, rr, openers, out.data()), c0, "shift_group_final");
                h->stats.group_finals++;
            } else {
                for (int p = 0; p < openers; p++) {
                    set_dev(p);
                    for (cozk_poly* q : {zry[(size_t)p].h, ep[(size_t)p].h}) rc_check(cozk_poly_bind(pcs[(size_t)p], q, rr, COZK_HIGH_TO_LOW), pcs[(size_t)p], "bind");
                    h->stats.single_finals++;
                }
            }
            g = ShiftGroupH();
            sp.release(ep);
        }
        sp.release(zry);
    }
    sp.sync_all();
    const double t5 = now_ms();
    // ---- the two claim exchanges: every column at rx_step, then at the shift point
    for (int which = 0; which < 2; which++) {
        const std::vector<fe>& point = which ? shift_r : rx_step;
        const std::vector<uint64_t> pt = to_abi(point);
        std::vector<std::vector<uint64_t>> ev((size_t)openers, std::vector<uint64_t>(4 * nvars));
        for (int p = 0; p < openers; p++) {
            cozk_ctx* c = pcs[(size_t)p];
            set_dev(p);
            VecH chi;
            if (which) rc_check(cozk_eq_evals(c, pt.data(), (int)point.size(), &chi.h), c, "eq_evals(shift_r)");
            const std::vector<const cozk_poly*> cc = col_ptrs(p);
            rc_check(cozk_poly_batch_evaluate_at_chi(c, cc.data(), cc.size(), which ? chi.h : eq_step[(size_t)p].h, ev[(size_t)p].data()), c, "batch_evaluate");
        }
        std::vector<fe>& claims = which ? pf.shift_witness_evals : pf.witness_evals;
        for (size_t i = 0; i < nvars; i++) {
            fe sh[COZK_SHAMIR_MAX_PARTIES];
            for (int p = 0; p < openers; p++) sh[p] = fe_from_u64x4(ev[(size_t)p].data() + 4 * i);
            claims.push_back(open_t(sh));
        }
        (void)tr.challenge_scalar();  // receive_claims draws rho for the batched opening that a whole Jolt proof reduces
    }
    sp.release(eq_step, eqp1_step);
    sp.sync_all();
    const double t6 = now_ms();
    res->verified = -1;
    if (verify) {
        std::string why;
        Transcript vt("cozk-spartan");
        std::vector<fe> v_rx, v_shift;
        fe rho[2];
        bool ok = verify_spartan(pf, sys, N, vt, v_rx, v_shift, rho, why);
        if (ok) {
            outer_setup_verifier(&h->inst);
            if (!outer_check_openings(&h->inst, v_rx, pf.witness_evals)) {
                ok = false;
                why = "spartan: claimed_witness_evals != the columns at rx_step";
            } else if (!outer_check_openings(&h->inst, v_shift, pf.shift_witness_evals)) {
                ok = false;
                why = "spartan: shift_sumcheck_witness_evals != the columns at the shift point";
            }
        }
        res->verified = ok ? 1 : 0;
        if (!ok) h->error = "verification failed: " + why;
    }
    res->grouped = grouped ? 1 : 0;
    res->n_opened = M;
    res->wall_ms = t6 - t0;
    res->t_build_ms = t1 - t0;
    res->t_masks_ms = t2 - t1;
    res->t_outer_ms = t3 - t2;
    res->t_inner_ms = t4 - t3;
    res->t_shift_ms = t5 - t4;
    res->t_openings_ms = t6 - t5;
    Writer w;
    pf.write(w);
    finish_proof(h, w.b, res);
}

static void shamir_jolt_spartan_release(cozk_shamir_jolt_spartan* h) {
    for (size_t p = 0; p < h->parties.size(); p++) {
        if (h->parties[p].ctx) (void)hipSetDevice(h->parties[p].ctx->device);
        if (p < h->cols.size()) h->cols[p].clear();
    }
    release_parties(h->parties, [](HarnessParty&) {});
    if (h->inst.vctx) {
        (void)hipSetDevice(h->inst.vctx->device);
        h->inst.v_cols.clear();
        cozk_ctx_destroy(h->inst.vctx);
        h->inst.vctx = nullptr;
    }
}

}  // namespace

extern "C" {

int cozk_shamir_jolt_spartan_create(const cozk_shamir_jolt_spartan_config* cfg, cozk_shamir_jolt_spartan** out) {
    return harness_create(cfg, out, [&](cozk_shamir_jolt_spartan* h) {
        const std::string w = "shamir_jolt_spartan";
        shamir_gp_require_parties(w, cfg->degree, cfg->num_parties);
        COZK_REQUIRE(cfg->log_steps >= 0 && cfg->log_steps <= 24, w + ": log_steps out of range (0..24)");
        COZK_REQUIRE(cfg->system == 0 || cfg->system == 1, w + ": system is 0 (toy) or 1 (the Jolt constraint set)");
        h->t = cfg->degree;
        const int n = h->n = cfg->num_parties;
        // the outer harness's own instance
        cozk_outer_harness& in = h->inst;
        memset(&in.cfg, 0, sizeof in.cfg);
        in.cfg.mode = COZK_MODE_PLAIN;
        in.cfg.log_steps = cfg->log_steps;
        in.cfg.devices[0] = cfg->devices[0];
        in.cfg.seed = cfg->seed;
        in.cfg.system = cfg->system;
        in.cfg.full = 1;
        in.N = (size_t)1 << cfg->log_steps;
        if (cfg->system == 1) {
            jolt::build_system(in.sys);
            in.ncols = jolt::NUM_INPUTS;
            for (int v = 0; v < in.ncols; v++) in.is_public.push_back(jolt::public_bytes(v) ? 1 : 0);
        } else {
            outer_build_system(in.sys);
            in.ncols = 14;
            in.is_public = {0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0};
        }
        outer_build_clear(&in);
        h->parties.resize((size_t)n);
        for (int p = 0; p < n; p++) {
            h->parties[(size_t)p].party = p;
            h->parties[(size_t)p].open_ctx(cfg->devices[p], "shamir_jolt_spartan: cannot create a context (no HIP device?)");
            h->pcs.push_back(h->parties[(size_t)p].ctx);
        }
        const std::vector<cozk_ctx*>& pcs = h->pcs;
        const std::vector<uint8_t> skeys = shamir_harness_keys(h, cfg->seed);
        // the witness: a public column stays public at every party, a shared one is dealt once, column v at share_counter + v num_steps
        h->cols.resize((size_t)n);
        for (int v = 0; v < in.ncols; v++) {
            if (in.is_public[(size_t)v]) {
                for (int p = 0; p < n; p++) {
                    HIP_TRY(hipSetDevice(pcs[(size_t)p]->device));
                    h->cols[(size_t)p].push_back(plain_poly(pcs[(size_t)p], upload_fe(pcs[(size_t)p], in.clear[(size_t)v])));
                    HIP_TRY(hipStreamSynchronize(pcs[(size_t)p]->stream));
                }
                continue;
            }
            HIP_TRY(hipSetDevice(pcs[0]->device));
            VecH cv = upload_fe(pcs[0], in.clear[(size_t)v]);
            std::vector<PolyH> dealt = shamir_deal_column(h, cv, skeys, cfg->share_counter + (uint64_t)v * (uint64_t)in.N, n);
            for (int p = 0; p < n; p++) h->cols[(size_t)p].push_back(std::move(dealt[(size_t)p]));
        }
    });
}

const char* cozk_shamir_jolt_spartan_error(const cozk_shamir_jolt_spartan* h) { return harness_error(h); }

int cozk_shamir_jolt_spartan_destroy(cozk_shamir_jolt_spartan* h) {
    if (!h) return COZK_OK;
    shamir_jolt_spartan_release(h);
    delete h;
    return COZK_OK;
}

int cozk_shamir_jolt_spartan_prove(cozk_shamir_jolt_spartan* h, int verify, cozk_shamir_jolt_spartan_result* res) {
    return shamir_harness_prove(
        h, res, "shamir_jolt_spartan",
        [](const cozk_shamir_jolt_spartan* x) { return x->cols.size() == (size_t)x->n && x->cols.back().size() == (size_t)x->inst.ncols; },
        [&](cozk_shamir_jolt_spartan* x, cozk_shamir_jolt_spartan_result* r) { shamir_jolt_spartan_prove(x, verify != 0, r); });
}

int cozk_shamir_jolt_spartan_proof_bytes(const cozk_shamir_jolt_spartan* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

size_t cozk_shamir_jolt_spartan_msgs_len(const cozk_shamir_jolt_spartan* h) { return h ? h->msgs.size() : 0; }
size_t cozk_shamir_jolt_spartan_finals_len(const cozk_shamir_jolt_spartan* h) { return h ? h->finals.size() : 0; }

int cozk_shamir_jolt_spartan_msgs(const cozk_shamir_jolt_spartan* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->msgs : nullptr, out, cap); }
int cozk_shamir_jolt_spartan_finals(const cozk_shamir_jolt_spartan* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->finals : nullptr, out, cap); }
int cozk_shamir_jolt_spartan_get_stats(const cozk_shamir_jolt_spartan* h, cozk_shamir_gp_stats* stats) { return shamir_harness_stats(h, stats); }

}  // extern "C"
