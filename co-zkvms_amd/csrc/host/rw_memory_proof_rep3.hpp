// In-process harness of the read-write memory proof by three Rep3 parties over the consistent witness of cozk_rw_proof
// (Rep3ReadWriteMemoryProver, co-jolt/src/jolt/vm/read_write_memory/worker.rs:196-344: the memory check init * writes == reads * final
// with the addresses and the timestamps public compact columns and v_read, v_write, v_final Rep3 shares).  The instance, the
// commitment order, the transcript and the verifier are cozk_rw_proof's with with_ts = 0 (rw_memory_proof.hpp): the handle holds that
// harness's own state for party 0 (`plain`: its context, SRS, compact columns and v_init), the coordinator fills its RwProof and
// rw_proof_verify checks it, so the proof is byte for byte the plain proof of the same seed and the multiset check runs.  Every step is
// one of memcheck_steps.hpp / prover.hpp; what is new is the sharing of the secret columns at create, the leaves from
// cozk_rw_memory_shared_leaves / cozk_rw_memory_shared_init_final_leaves, and the openings that join public compact columns with
// shared polynomials.  cozk_memory_proof_rep3 (memory_proof_rep3.hpp) runs the same steps with the output check behind them.  Not here
// (DESIGN 7): the timestamp range check by Rep3 parties, one party per process.
#pragma once

struct RwRep3Party : HarnessParty {
    std::vector<VecH> own;  // the compact columns this party uploaded itself (parties 1 and 2); party 0 reads the plain harness's
    std::vector<const cozk_vec*> addr, t_read;  // the public compact columns, wherever they live
    const cozk_vec *t_final = nullptr, *iota_n = nullptr, *iota_mem = nullptr;
    PolyH v_init;                           // PLAIN: public preprocessing
    std::vector<PolyH> v_read, v_written;   // REP3; v_written[s] empty: the slot only reads
    PolyH v_final;                          // REP3
    std::vector<VecH> commit_views;         // the a components of the shares, for the MSM
    std::unique_ptr<PST13Setup> own_setup;  // parties 1 and 2
    const PST13Setup* setup = nullptr;
    double t_share = 0, t_commit = 0, t_leaves = 0, t_gp = 0, t_open = 0;
};

struct cozk_rw_proof_rep3 : HarnessHandle {
    cozk_rw_proof_rep3_config cfg;
    cozk_rw_proof plain;  // party 0's plain harness with with_ts = 0: the instance, and what the verifier reads
    bool built = false;
    std::vector<RwRep3Party> parties;
};

namespace {

inline size_t rw3_elem_bytes(int kind) { return kind == COZK_SCALAR_U8 ? 1 : 4; }

// a compact column of party 0's device on the host, and on another party's device
struct Rw3HostCol {
    std::vector<uint8_t> bytes;
    size_t n = 0;
    int kind = 0;
};
Rw3HostCol rw3_download(cozk_ctx* ctx, const cozk_vec* v) {
    Rw3HostCol c;
    c.n = v->n, c.kind = v->kind;
    c.bytes.resize(c.n * rw3_elem_bytes(c.kind));
    rc_check(cozk_vec_download(ctx, v, c.bytes.data()), ctx, "vec_download");
    return c;
}
VecH rw3_upload(cozk_ctx* ctx, const Rw3HostCol& c) { return upload_vec(ctx, c.bytes.data(), c.n, c.kind, "vec_upload(column)"); }

// a secret compact column widened to Fr (cozk_compact_linear_combination with coefficient 1) and shared under the harness keys
PolyH rw3_share_column(RwRep3Party& ps, const cozk_vec* col, uint64_t seed) {
    const std::vector<uint64_t> one = to_abi({Fr::one()});
    cozk_vec* wide = nullptr;
    rc_check(cozk_compact_linear_combination(ps.ctx, &col, one.data(), 1, &wide), ps.ctx, "compact_linear_combination(widen)");
    VecH wh(wide);
    PolyH p = make_shared_poly(ps.ctx, COZK_MODE_REP3, wh, seed, ps.party);
    cozk_vec* view = nullptr;
    rc_check(cozk_poly_share_view(ps.ctx, p.h, 0, &view), ps.ctx, "share_view");
    ps.commit_views.push_back(VecH(view));
    return p;
}

// create, after party 0's plain harness stands: every party gets the public columns and its shares of the secret ones
void rw3_setup(cozk_rw_proof& plain, const cozk_rw_proof_rep3_config& c, std::vector<RwRep3Party>& parties) {
    RwProofParty& p0 = plain.parties[0];
    const size_t ns = (size_t)plain.ns;
    // the dealer's columns on the host, once: public ones for parties 1 and 2, secret ones for every party's sharing
    std::vector<Rw3HostCol> addr, t_read, v_read, v_written(ns);
    for (size_t s = 0; s < ns; s++) {
        addr.push_back(rw3_download(p0.ctx, p0.addr[s].h));
        t_read.push_back(rw3_download(p0.ctx, p0.t_read[s].h));
        v_read.push_back(rw3_download(p0.ctx, p0.v_read[s].h));
        if (p0.v_written[s].h) v_written[s] = rw3_download(p0.ctx, p0.v_written[s].h);
    }
    const Rw3HostCol t_final = rw3_download(p0.ctx, p0.t_final.h), v_final = rw3_download(p0.ctx, p0.v_final.h), v_init = rw3_download(p0.ctx, p0.v_init.h);
    parties.resize(3);
    for (int p = 0; p < 3; p++) {
        RwRep3Party& ps = parties[(size_t)p];
        ps.party = p;
        if (p == 0) {
            ps.ctx = p0.ctx;  // the plain harness owns it
            ps.setup = p0.setup.get();
            HIP_TRY(hipSetDevice(ps.ctx->device));
        } else {
            ps.open_ctx(c.devices[p], "rw_proof_rep3: cannot create a context (no HIP device?)");
            std::vector<fe> t(p0.setup->trapdoor);
            ps.own_setup = PST13::setup(ps.ctx, t, c.precompute);
            ps.setup = ps.own_setup.get();
        }
        cozk_ctx_set_resident_rounds(ps.ctx, 0);  // three parties share the machine, as in the chained flow
        const double t0 = now_ms();
        auto keep = [&](VecH v) {
            ps.own.push_back(std::move(v));
            return (const cozk_vec*)ps.own.back().h;
        };
        for (size_t s = 0; s < ns; s++) {
            ps.addr.push_back(p == 0 ? p0.addr[s].h : keep(rw3_upload(ps.ctx, addr[s])));
            ps.t_read.push_back(p == 0 ? p0.t_read[s].h : keep(rw3_upload(ps.ctx, t_read[s])));
        }
        ps.t_final = p == 0 ? p0.t_final.h : keep(rw3_upload(ps.ctx, t_final));
        {  // v_init: a PLAIN polynomial
            const cozk_vec* col = p == 0 ? p0.v_init.h : keep(rw3_upload(ps.ctx, v_init));
            const std::vector<uint64_t> one = to_abi({Fr::one()});
            cozk_vec* wide = nullptr;
            rc_check(cozk_compact_linear_combination(ps.ctx, &col, one.data(), 1, &wide), ps.ctx, "compact_linear_combination(v_init)");
            VecH wh(wide);
            ps.v_init = plain_poly(ps.ctx, wh);
        }
        // the secret columns in the commit order v_read, v_written, v_final, each under a seed of its own
        // (the harness deals in the clear on every party's device; the clear copy of parties 1 and 2 goes once the shares stand)
        auto share = [&](const VecH& dealer, const Rw3HostCol& host, uint64_t seed) {
            if (p == 0) return rw3_share_column(ps, dealer.h, seed);
            VecH clear = rw3_upload(ps.ctx, host);
            return rw3_share_column(ps, clear.h, seed);
        };
        ps.v_written.resize(ns);
        for (size_t s = 0; s < ns; s++) ps.v_read.push_back(share(p0.v_read[s], v_read[s], c.seed + 1000ull * (uint64_t)(s + 1)));
        for (size_t s = 0; s < ns; s++)
            if (p0.v_written[s].h) ps.v_written[s] = share(p0.v_written[s], v_written[s], c.seed + 1000ull * (uint64_t)(ns + s + 1));
        ps.v_final = share(p0.v_final, v_final, c.seed + 46000ull);
        if (!c.leaves_fused) {
            if (p == 0) {
                ps.iota_n = p0.iota_n.h, ps.iota_mem = p0.iota_mem.h;
            } else {
                std::vector<uint32_t> io(std::max(plain.N, plain.MEM));
                for (size_t j = 0; j < io.size(); j++) io[j] = (uint32_t)j;
                ps.iota_n = keep(upload_vec(ps.ctx, io.data(), plain.N, COZK_SCALAR_U32, "vec_upload(iota)"));
                ps.iota_mem = keep(upload_vec(ps.ctx, io.data(), plain.MEM, COZK_SCALAR_U32, "vec_upload(iota)"));
            }
        }
        HIP_TRY(hipStreamSynchronize(ps.ctx->stream));
        ps.t_share = now_ms() - t0;
    }
}

// One opening that joins public compact columns with shared polynomials, at `point`.  order[i]: the i-th column of the plain proof's
// order, a compact public column (col) or a shared polynomial (poly).  The claims: public ones from
// cozk_compact_batch_evaluate_at_chi, reported by the party env.additive_trivial names (the convention of the flow's openings);
// shared ones from cozk_poly_batch_evaluate_at_chi, additive.  ONE exchange, then ONE joint polynomial: the compact combination of
// the public columns over their rho powers as a PLAIN polynomial, plus the shared polynomials over theirs.
void rw3_open_worker(WorkerEnv& env, Rep3ProverOpeningAccumulator& acc, const std::vector<LeafTerm>& order, const std::vector<fe>& point, bool tamper_claim) {
    VecH chih = mc_eq_table(env, point);
    std::vector<const cozk_vec*> cols;
    std::vector<const cozk_poly*> polys;
    std::vector<size_t> col_at, poly_at;
    for (size_t i = 0; i < order.size(); i++) {
        if (order[i].col) cols.push_back(order[i].col), col_at.push_back(i);
        else polys.push_back(order[i].poly), poly_at.push_back(i);
    }
    std::vector<fe> claims(order.size());
    if (!cols.empty()) {
        std::vector<uint64_t> ev(4 * cols.size());
        rc_check(cozk_compact_batch_evaluate_at_chi(env.ctx, cols.data(), cols.size(), chih.h, ev.data()), env.ctx, "compact_batch_evaluate");
        for (size_t k = 0; k < cols.size(); k++) claims[col_at[k]] = env.additive_trivial(fe_from_u64x4(ev.data() + 4 * k));
    }
    if (!polys.empty()) {
        std::vector<uint64_t> ev(4 * polys.size());
        rc_check(cozk_poly_batch_evaluate_at_chi(env.ctx, polys.data(), polys.size(), chih.h, ev.data()), env.ctx, "batch_evaluate");
        for (size_t k = 0; k < polys.size(); k++) claims[poly_at[k]] = fe_from_u64x4(ev.data() + 4 * k);
    }
    if (tamper_claim && env.party == 0) claims[0] = Fr::add(claims[0], Fr::one());
    fe batched_claim;
    const std::vector<fe> rho_powers = Rep3ProverOpeningAccumulator::exchange_claims(env, claims, batched_claim);
    std::vector<const cozk_poly*> joint;
    std::vector<fe> jc;
    PolyH pub;
    if (!cols.empty()) {
        std::vector<fe> cc;
        for (size_t at : col_at) cc.push_back(rho_powers[at]);
        const std::vector<uint64_t> cf = to_abi(cc);
        cozk_vec* jv = nullptr;
        rc_check(cozk_compact_linear_combination(env.ctx, cols.data(), cf.data(), cols.size(), &jv), env.ctx, "compact_linear_combination");
        VecH jvh(jv);
        pub = plain_poly(env.ctx, jvh);
        joint.push_back(pub.h);
        jc.push_back(Fr::one());
    }
    for (size_t k = 0; k < polys.size(); k++) joint.push_back(polys[k]), jc.push_back(rho_powers[poly_at[k]]);
    const std::vector<uint64_t> cf = to_abi(jc);
    cozk_poly* batched = nullptr;
    rc_check(cozk_poly_linear_combination(env.ctx, joint.data(), cf.data(), joint.size(), env.mode, env.party, &batched), env.ctx, "linear_combination(joint)");
    acc.append_joint(env, PolyH(batched), chih.h, point, batched_claim);
}

// Steps 1-4 of the worker, shared with cozk_memory_proof_rep3 (memory_proof_rep3.hpp): the commit, gamma and tau, the leaves, the two
// grand products and the two openings into `acc`.  Sets t_commit, t_leaves and t_gp; returns the clock taken after the grand products
// (the openings belong to t_open).
double rw3_memory_check_worker(cozk_rw_proof& plain, const cozk_rw_proof_rep3_config& c, RwRep3Party& ps, WorkerEnv& env, Rep3ProverOpeningAccumulator& acc) {
    const size_t ns = (size_t)plain.ns, N = plain.N, MEM = plain.MEM;
    StarNetWorker* star = env.star;
    // the plain proof's column order: addr, v_read, v_written (the slots that write), t_read | v_final, t_final
    std::vector<LeafTerm> rw_order, if_order;
    for (size_t s = 0; s < ns; s++) rw_order.push_back(mc_col_term(ps.addr[s]));
    for (size_t s = 0; s < ns; s++) rw_order.push_back(LeafTerm{nullptr, ps.v_read[s].h, Fr::zero()});
    for (size_t s = 0; s < ns; s++)
        if (ps.v_written[s].h) rw_order.push_back(LeafTerm{nullptr, ps.v_written[s].h, Fr::zero()});
    for (size_t s = 0; s < ns; s++) rw_order.push_back(mc_col_term(ps.t_read[s]));
    if_order.push_back(LeafTerm{nullptr, ps.v_final.h, Fr::zero()});
    if_order.push_back(mc_col_term(ps.t_final));
    const double t0 = now_ms();
    // ---- 1. commit: each party the a components of its shares and the public columns; party 0's public commitments are the ones kept
    {
        std::vector<cozk_vec*> vs;
        std::vector<int> is_public;
        size_t view = 0;
        for (const std::vector<LeafTerm>* part : {&rw_order, &if_order})
            for (const LeafTerm& t : *part) {
                vs.push_back(t.col ? const_cast<cozk_vec*>(t.col) : ps.commit_views[view++].h);
                is_public.push_back(t.col ? 1 : 0);
            }
        Writer w;
        put_commitments(w, PST13::batch_commit(ps.ctx, *ps.setup, vs), is_public, ps.party);
        star->send_response(w.b);
    }
    const double t1 = now_ms();
    ps.t_commit = t1 - t0;
    // ---- 2. gamma, tau; the leaves
    fe gamma, tau;
    mc_receive_gamma_tau(star, gamma, tau);
    const double t2 = now_ms();
    LeafBuf rw = mc_leaf_alloc(env, 2 * ns * N), inf = mc_leaf_alloc(env, 2 * MEM);
    if (c.leaves_fused) {
        std::vector<const cozk_vec*> a, tr;
        std::vector<const cozk_poly*> vr, vw;
        for (size_t s = 0; s < ns; s++) a.push_back(ps.addr[s]), tr.push_back(ps.t_read[s]), vr.push_back(ps.v_read[s].h), vw.push_back(ps.v_written[s].h);
        uint64_t g[4], t[4];
        fe_to_u64x4(gamma, g);
        fe_to_u64x4(tau, t);
        rc_check(cozk_rw_memory_shared_leaves(env.ctx, a.data(), vr.data(), tr.data(), vw.data(), ns, g, t, env.mode, env.party, rw.a.h, rw.b.h, 0), env.ctx,
                 "rw_memory_shared_leaves");
        rc_check(cozk_rw_memory_shared_init_final_leaves(env.ctx, ps.v_init.h, ps.v_final.h, ps.t_final, g, t, env.mode, env.party, inf.a.h, inf.b.h, 0), env.ctx,
                 "rw_memory_shared_init_final_leaves");
    } else {
        std::vector<RwSlotLeaves> slots;
        for (size_t s = 0; s < ns; s++) {
            const LeafTerm v{nullptr, ps.v_read[s].h, Fr::zero()}, w{nullptr, ps.v_written[s].h ? ps.v_written[s].h : ps.v_read[s].h, Fr::zero()};
            slots.push_back({mc_col_term(ps.addr[s]), v, w, mc_col_term(ps.t_read[s])});
        }
        rw_memory_leaves_composed(env, slots, LeafTerm{nullptr, ps.v_init.h, Fr::zero()}, if_order[0], if_order[1], mc_col_term(ps.iota_n), mc_col_term(ps.iota_mem), N, MEM, gamma,
                                  tau, rw, inf);
    }
    rc_check(cozk_ctx_synchronize(env.ctx), env.ctx, "synchronize");
    const double t3 = now_ms();
    ps.t_leaves = t3 - t2;
    // ---- 3. the two grand products in REP3
    std::vector<fe> r_rw, r_if;
    mc_memory_checking(env, mc_leaves_to_layer(env, rw), 2 * ns, ToggleH(), mc_leaves_to_layer(env, inf), 2, r_rw, r_if);
    const double t4 = now_ms();
    ps.t_gp = t4 - t3;
    // ---- 4. the two openings
    rw3_open_worker(env, acc, rw_order, r_rw, c.tamper == 2);
    rw3_open_worker(env, acc, if_order, r_if, false);
    return t4;
}

// Step 5, shared likewise: ONE reduce_and_prove over every opening in `acc`.  t45: what the openings before this call took.  Sets t_open.
void rw3_open_and_finish_worker(RwRep3Party& ps, WorkerEnv& env, Rep3ProverOpeningAccumulator& acc, double t45) {
    const double t5 = now_ms();
    acc.reduce_and_prove_worker(env, *ps.setup);
    ps.t_open = t45 + (now_ms() - t5);
    ps.record_net(env.star, env.ring);
}

void rw3_worker_main(cozk_rw_proof_rep3* h, RwRep3Party& ps, StarNetWorker* star, RingNet* ring) {
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_REP3, ps.party, star, ring, &h->cfg.seed);
    Rep3ProverOpeningAccumulator acc;
    const double t4 = rw3_memory_check_worker(h->plain, h->cfg, ps, env, acc);
    rw3_open_and_finish_worker(ps, env, acc, now_ms() - t4);
}

// the commitments combined over the three parties, into the proof and the transcript
void rw3_coordinate_commitments(StarNetCoordinator& net, Transcript& tr, std::vector<PST13Commitment>& commitments) {
    std::vector<Bytes> msgs = net.receive_responses();
    std::vector<Reader> rds;
    for (auto& m : msgs) rds.emplace_back(m);
    commitments = combine_commitments_from_parties(rds, 3);
    for (auto& cm : commitments) tr.append_point(cm.g_product);
}

// the coordinator: cozk_rw_proof's with the commitments combined over the three parties
void rw3_coordinate(cozk_rw_proof_rep3* h, StarNetCoordinator& net, RwProof& proof) {
    const cozk_rw_proof_config& c = h->plain.cfg;
    Transcript tr("cozk-rw-memory");
    rw3_coordinate_commitments(net, tr, proof.commitments);
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.mem, (size_t)c.log_n, false, (size_t)c.log_mem);
    rw_proof_coordinate_range_check_and_open(c, net, tr, proof.with_ts, proof.range, proof.reduced);
}

void rw3_release(cozk_rw_proof& plain, std::vector<RwRep3Party>& parties) {
    for (RwRep3Party& ps : parties) {
        if (ps.ctx) (void)hipSetDevice(ps.ctx->device);
        ps.v_init = PolyH(), ps.v_final = PolyH();
        ps.v_read.clear(), ps.v_written.clear(), ps.commit_views.clear(), ps.own.clear();
        ps.own_setup.reset();
        if (ps.own_ctx && ps.ctx) cozk_ctx_destroy(ps.ctx);
        ps.ctx = nullptr;
    }
    parties.clear();
    rw_proof_release(&plain);
}

}  // namespace

extern "C" {

int cozk_rw_proof_rep3_create(const cozk_rw_proof_rep3_config* cfg, cozk_rw_proof_rep3** out) {
    return harness_create(cfg, out, [&](cozk_rw_proof_rep3* h) {
        cozk_rw_proof_config& pc = h->plain.cfg;
        pc = cozk_rw_proof_config{};
        pc.mode = COZK_MODE_PLAIN, pc.device = cfg->devices[0], pc.log_n = cfg->log_n, pc.log_mem = cfg->log_mem, pc.n_slots = cfg->n_slots, pc.seed = cfg->seed;
        pc.precompute = cfg->precompute, pc.with_ts = 0, pc.leaves_fused = cfg->leaves_fused, pc.tamper = cfg->tamper;
        rw_proof_check_config(pc, "rw_proof_rep3", 2);
        rw_proof_build(&h->plain, "rw_proof_rep3");  // the instance on party 0's context, tamper 1 included
        rw3_setup(h->plain, h->cfg, h->parties);
        h->built = true;
    });
}

const char* cozk_rw_proof_rep3_error(const cozk_rw_proof_rep3* h) { return harness_error(h); }

int cozk_rw_proof_rep3_destroy(cozk_rw_proof_rep3* h) {
    if (!h) return COZK_OK;
    rw3_release(h->plain, h->parties);
    delete h;
    return COZK_OK;
}

int cozk_rw_proof_rep3_prove(cozk_rw_proof_rep3* h, int verify, cozk_rw_proof_rep3_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (!h->built) return COZK_ERR_INVALID_ARG;  // create failed
    InProcNets nets(3, true);
    std::vector<Participant> parts;
    add_participants(parts, "party", h->parties, [&](RwRep3Party& ps, int p) { rw3_worker_main(h, ps, nets.worker(p), nets.ring(p)); });
    RwProof proof;
    double wall_ms = 0;
    int rc = run_in_process(nets, parts, [&] {
        InProcStarCoordinator coord(&nets.star);
        rw3_coordinate(h, coord, proof);
    }, h->error, wall_ms);
    if (rc != COZK_OK) return rc;
    res->wall_ms = wall_ms;  // the verifier below is outside the clock
    if (verify) harness_verify(h, res, h->parties[0].ctx->device, [&](std::string& why) { return rw_proof_verify(&h->plain, proof, why); });
    res->t_witness_ms = h->plain.t_witness;
    for (const RwRep3Party& ps : h->parties) {
        res->t_share_ms = std::max(res->t_share_ms, ps.t_share);
        res->t_commit_ms = std::max(res->t_commit_ms, ps.t_commit);
        res->t_leaves_ms = std::max(res->t_leaves_ms, ps.t_leaves);
        res->t_gp_ms = std::max(res->t_gp_ms, ps.t_gp);
        res->t_open_ms = std::max(res->t_open_ms, ps.t_open);
        res->ring_bytes += ps.ring_bytes;
    }
    finish_proof(h, proof.serialize(), res);
    return COZK_OK;
}

int cozk_rw_proof_rep3_proof_bytes(const cozk_rw_proof_rep3* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
