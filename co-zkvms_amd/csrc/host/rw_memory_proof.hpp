// In-process harness of party 0's read-write memory proof over a consistent witness (the dealer's side of Jolt's ReadWriteMemoryProof:
// the memory check init * writes == reads * final of read_write_memory/worker.rs:196-344 with the timestamp range check of
// ts_range_proof.hpp chained behind it under the same transcript and the same opening accumulator, ONE reduce_and_prove for
// everything).  The chained flow (flow_rw_memory_worker, flow_verify_rw_memory) runs the same shared steps of
// memcheck_steps.hpp -- rw_memory_leaves_composed, mc_memory_checking, mc_verify_grand_products, rw_memory_verify_leaves -- on seeded
// streams, whose multiset check cannot hold; here the witness comes from cozk_rw_memory_witness, so the verifier runs it.  jolt-core
// is not in the reference tree, so the circuit order, the transcript order and the proof bytes are this project's: PARITY UNPINNED.
// What pins them is the plain verifier at the end of this file and tests/rw_proof_ref.py (include/cozk.h has the protocol).
// Every polynomial is a compact column on the device (U8 register addresses, U32 everything else): the commit takes the MSM's
// small-scalar path, the leaves come from cozk_rw_memory_leaves / cozk_rw_memory_init_final_leaves, the claims and the joint
// polynomials from the compact opening calls; no Fr copy of a column exists.
#pragma once

struct RwProofParty : HarnessParty {
    std::vector<VecH> addr, v_read, t_read;
    std::vector<VecH> v_written;  // n_slots entries; empty handle: the slot only reads
    VecH v_init, v_final, t_final;
    std::vector<VecH> rc_rt, rc_gmr, fc_rt, fc_gmr;  // with_ts
    VecH iota_n, iota_mem;                           // the composition's step / address columns (leaves_fused = 0)
    std::unique_ptr<PST13Setup> setup;
    double t_commit = 0, t_leaves = 0, t_gp = 0, t_ts = 0, t_open = 0;
};

struct cozk_rw_proof : HarnessHandle {
    cozk_rw_proof_config cfg;
    size_t N = 0, MEM = 0;
    int ns = 0;
    double t_witness = 0;
    std::vector<uint32_t> v_init_clear;  // public preprocessing: the verifier evaluates its MLE itself
    std::vector<RwProofParty> parties;   // party 0 alone
};

namespace {

struct RwProof {
    std::vector<PST13Commitment> commitments;
    MemCheckProof mem;
    bool with_ts = false;
    TsRangeProof range;
    ReducedOpeningProof reduced;
    Bytes serialize() const {
        Writer w;
        w.u64(commitments.size());
        for (auto& c : commitments) c.write(w);
        mem.write(w);
        if (with_ts) range.write(w);
        reduced.write(w);
        return w.b;
    }
};

// slot s writes: rd (2) and ram (3)
inline bool rw_slot_writes(int s) { return s >= 2; }

// where each committed column sits in the proof's order
struct RwProofIdx {
    size_t ns, nw, addr, v_read, v_written, t_read, v_final, t_final, rc_rt, n_rw, count;
    RwProofIdx(size_t ns_, bool with_ts) : ns(ns_) {
        nw = ns > 2 ? ns - 2 : 0;
        addr = 0, v_read = ns, v_written = 2 * ns, t_read = 2 * ns + nw, n_rw = 3 * ns + nw;
        v_final = n_rw, t_final = n_rw + 1, rc_rt = n_rw + 2;
        count = n_rw + 2 + (with_ts ? 4 * ns : 0);
    }
};

std::vector<const cozk_vec*> rw_proof_rw_columns(const RwProofParty& ps) {
    std::vector<const cozk_vec*> cols;
    for (const VecH& v : ps.addr) cols.push_back(v.h);
    for (const VecH& v : ps.v_read) cols.push_back(v.h);
    for (const VecH& v : ps.v_written)
        if (v.h) cols.push_back(v.h);
    for (const VecH& v : ps.t_read) cols.push_back(v.h);
    return cols;
}

// create: the trace of ts_proof_setup restricted to the first n_slots slots, both witness walks on the device
void rw_proof_setup(cozk_rw_proof* h, RwProofParty& ps) {
    const cozk_rw_proof_config& c = h->cfg;
    cozk_ctx* ctx = ps.ctx;
    const size_t N = h->N, MEM = h->MEM;
    const int ns = h->ns, nv = c.log_n > c.log_mem ? c.log_n : c.log_mem;
    std::vector<fe> t((size_t)nv);
    for (int i = 0; i < nv; i++) t[(size_t)i] = synthetic_fr_host(c.seed ^ 0x7A7A7A7Aull, (uint64_t)i);
    ps.setup = PST13::setup(ctx, t, c.precompute);
    const TsTrace trace = ts_trace(c.seed, N, MEM);
    h->v_init_clear = trace.v_init;
    double t0 = now_ms();
    std::vector<VecH> d_vw(4);
    for (int s = 0; s < ns; s++) {
        if (s < 3) {  // a register index is below 32: a U8 column
            std::vector<uint8_t> a8(trace.addr[(size_t)s].begin(), trace.addr[(size_t)s].end());
            ps.addr.push_back(upload_vec(ctx, a8.data(), N, COZK_SCALAR_U8, "vec_upload(register addresses)"));
        } else {
            ps.addr.push_back(upload_vec(ctx, trace.addr[3].data(), N, COZK_SCALAR_U32, "vec_upload(ram addresses)"));
        }
        if (rw_slot_writes(s)) d_vw[(size_t)s] = upload_vec(ctx, trace.vw[(size_t)s - 2].data(), N, COZK_SCALAR_U32, "vec_upload(written values)");
    }
    VecH d_iw;
    if (ns == 4) d_iw = upload_vec(ctx, trace.iw.data(), N, COZK_SCALAR_U8, "vec_upload(store flags)");
    ps.v_init = upload_vec(ctx, trace.v_init.data(), MEM, COZK_SCALAR_U32, "vec_upload(v_init)");
    const cozk_vec *pa[4] = {}, *pw[4] = {}, *pf[4] = {};
    for (int s = 0; s < ns; s++) pa[s] = ps.addr[(size_t)s].h, pw[s] = d_vw[(size_t)s].h;
    pf[3] = d_iw.h;
    cozk_vec *v_read[4] = {}, *t_read[4] = {}, *v_written[4] = {}, *v_final = nullptr, *t_final = nullptr;
    rc_check(cozk_rw_memory_witness(ctx, pa, pw, pf, (size_t)ns, ps.v_init.h, v_read, t_read, v_written, &v_final, &t_final), ctx, "rw_memory_witness");
    for (int s = 0; s < ns; s++) {
        ps.v_read.push_back(VecH(v_read[s]));
        ps.t_read.push_back(VecH(t_read[s]));
        // the word a writing slot leaves behind: rd writes every step (its v_write), ram where flagged (the witness's v_written)
        if (v_written[s]) ps.v_written.push_back(VecH(v_written[s]));
        else ps.v_written.push_back(std::move(d_vw[(size_t)s]));
    }
    ps.v_final = VecH(v_final);
    ps.t_final = VecH(t_final);
    if (c.with_ts) {
        std::vector<const cozk_vec*> tr;
        for (auto& v : ps.t_read) tr.push_back(v.h);
        cozk_vec *a[COZK_RW_MEMORY_MAX_SLOTS] = {}, *b[COZK_RW_MEMORY_MAX_SLOTS] = {}, *cc[COZK_RW_MEMORY_MAX_SLOTS] = {}, *d[COZK_RW_MEMORY_MAX_SLOTS] = {};
        rc_check(cozk_timestamp_range_witness(ctx, tr.data(), (size_t)ns, N, a, b, cc, d), ctx, "timestamp_range_witness");
        for (int s = 0; s < ns; s++) {
            ps.rc_rt.push_back(VecH(a[s]));
            ps.rc_gmr.push_back(VecH(b[s]));
            ps.fc_rt.push_back(VecH(cc[s]));
            ps.fc_gmr.push_back(VecH(d[s]));
        }
    }
    h->t_witness = now_ms() - t0;
    if (c.tamper == 1) {  // a read that no write made: every relation but the multiset's holds
        std::vector<uint32_t> vr(N);
        rc_check(cozk_vec_download(ctx, ps.v_read[(size_t)ns - 1].h, vr.data()), ctx, "vec_download");
        vr[N / 2] += 1;
        ps.v_read[(size_t)ns - 1] = upload_vec(ctx, vr.data(), N, COZK_SCALAR_U32, "vec_upload(tampered v_read)");
    }
    if (c.tamper == 3) ts_tamper_final_counter(ctx, ps.t_read[0], ps.fc_rt[0], N);
    if (!c.leaves_fused) {
        std::vector<uint32_t> io(N > MEM ? N : MEM);
        for (size_t j = 0; j < io.size(); j++) io[j] = (uint32_t)j;
        ps.iota_n = upload_vec(ctx, io.data(), N, COZK_SCALAR_U32, "vec_upload(iota)");
        ps.iota_mem = upload_vec(ctx, io.data(), MEM, COZK_SCALAR_U32, "vec_upload(iota)");
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// the 2 n_slots + 2 circuits as cozk_fingerprint_leaves calls (rw_memory_leaves_composed, ten at 4 slots): what the two fused calls replace
void rw_proof_leaves_composed(WorkerEnv& env, const RwProofParty& ps, size_t N, size_t MEM, const fe& gamma, const fe& tau, LeafBuf& rw, LeafBuf& inf) {
    std::vector<RwSlotLeaves> slots;
    for (size_t u = 0; u < ps.addr.size(); u++) {
        const VecH& w = ps.v_written[u].h ? ps.v_written[u] : ps.v_read[u];
        slots.push_back({mc_col_term(ps.addr[u].h), mc_col_term(ps.v_read[u].h), mc_col_term(w.h), mc_col_term(ps.t_read[u].h)});
    }
    rw_memory_leaves_composed(env, slots, mc_col_term(ps.v_init.h), mc_col_term(ps.v_final.h), mc_col_term(ps.t_final.h), mc_col_term(ps.iota_n.h),
                              mc_col_term(ps.iota_mem.h), N, MEM, gamma, tau, rw, inf);
}

// Steps 1-4 of the worker, shared with cozk_memory_proof (memory_proof.hpp): the commit, gamma and tau, the leaves, the two grand
// products and the two openings from the compact columns into `acc`.  Sets t_commit, t_leaves and t_gp; returns the clock taken after
// the grand products (the openings belong to t_open).
double rw_proof_memory_check_worker(cozk_rw_proof* h, RwProofParty& ps, WorkerEnv& env, const TsRangeCols& range, Rep3ProverOpeningAccumulator& acc) {
    const cozk_rw_proof_config& c = h->cfg;
    const int ns = h->ns;
    const size_t N = h->N, MEM = h->MEM;
    StarNetWorker* star = env.star;
    const std::vector<const cozk_vec*> rw_cols = rw_proof_rw_columns(ps);
    const std::vector<const cozk_vec*> if_cols = {ps.v_final.h, ps.t_final.h};
    double t0 = now_ms();
    // ---- 1. commit: mixed lengths and compact kinds
    {
        std::vector<const cozk_vec*> all = rw_cols;
        all.insert(all.end(), if_cols.begin(), if_cols.end());
        if (c.with_ts)
            for (const std::vector<const cozk_vec*>* fam : {&range.rc_rt, &range.rc_gmr, &range.fc_rt, &range.fc_gmr}) all.insert(all.end(), fam->begin(), fam->end());
        mc_commit_worker(env, *ps.setup, all);
    }
    double t1 = now_ms();
    ps.t_commit = t1 - t0;
    // ---- 2. gamma, tau; the leaves
    fe gamma, tau;
    mc_receive_gamma_tau(star, gamma, tau);
    double t2 = now_ms();
    LeafBuf rw = mc_leaf_alloc(env, 2 * (size_t)ns * N), inf = mc_leaf_alloc(env, 2 * MEM);
    if (c.leaves_fused) {
        std::vector<const cozk_vec*> a, vr, tr, vw;
        for (int s = 0; s < ns; s++) {
            const size_t u = (size_t)s;
            a.push_back(ps.addr[u].h), vr.push_back(ps.v_read[u].h), tr.push_back(ps.t_read[u].h), vw.push_back(ps.v_written[u].h);
        }
        uint64_t g[4], t[4];
        fe_to_u64x4(gamma, g);
        fe_to_u64x4(tau, t);
        rc_check(cozk_rw_memory_leaves(env.ctx, a.data(), vr.data(), tr.data(), vw.data(), (size_t)ns, g, t, rw.a.h, 0), env.ctx, "rw_memory_leaves");
        rc_check(cozk_rw_memory_init_final_leaves(env.ctx, ps.v_init.h, ps.v_final.h, ps.t_final.h, g, t, inf.a.h, 0), env.ctx, "rw_memory_init_final_leaves");
    } else {
        rw_proof_leaves_composed(env, ps, N, MEM, gamma, tau, rw, inf);
    }
    rc_check(cozk_ctx_synchronize(env.ctx), env.ctx, "synchronize");
    double t3 = now_ms();
    ps.t_leaves = t3 - t2;
    // ---- 3. the two grand products; their claimed outputs are the multiset hashes
    std::vector<fe> r_rw, r_if;
    mc_memory_checking(env, mc_leaves_to_layer(env, rw), 2 * (size_t)ns, ToggleH(), mc_leaves_to_layer(env, inf), 2, r_rw, r_if);
    double t4 = now_ms();
    ps.t_gp = t4 - t3;
    // ---- 4. two openings from the compact columns
    compact_open_worker(env, acc, rw_cols, r_rw, c.tamper == 2);
    compact_open_worker(env, acc, if_cols, r_if, false);
    return t4;
}

// Steps 5 and 6, shared likewise: with with_ts the timestamp range check, chained (t_read is not committed again), then ONE
// reduce_and_prove.  t45: what the openings before this call took.  Sets t_ts and t_open.
void rw_proof_range_check_and_open_worker(cozk_rw_proof* h, RwProofParty& ps, WorkerEnv& env, const TsRangeCols& range, Rep3ProverOpeningAccumulator& acc, double t45) {
    const cozk_rw_proof_config& c = h->cfg;
    double t5 = now_ms();
    if (c.with_ts) {
        double tl = 0, tg = 0;
        ts_range_check_worker(env, range, h->N, c.leaves_fused != 0, false, acc, tl, tg);
    }
    double t6 = now_ms();
    ps.t_ts = t6 - t5;
    acc.reduce_and_prove_worker(env, *ps.setup);
    ps.t_open = t45 + (now_ms() - t6);
    ps.record_net(env.star);
}

void rw_proof_worker_main(cozk_rw_proof* h, RwProofParty& ps, StarNetWorker* star) {
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_PLAIN, 0, star, nullptr);
    const TsRangeCols range = ts_range_columns(ps, ps.iota_n);
    Rep3ProverOpeningAccumulator acc;
    const double t4 = rw_proof_memory_check_worker(h, ps, env, range, acc);
    rw_proof_range_check_and_open_worker(h, ps, env, range, acc, now_ms() - t4);
}

// the coordinator's halves of the two worker steps above, under the caller's transcript
void rw_proof_coordinate_memory_check(const cozk_rw_proof_config& c, StarNetCoordinator& net, Transcript& tr, std::vector<PST13Commitment>& commitments, MemCheckProof& mem) {
    mc_receive_commitments(net, tr, commitments);
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, mem, (size_t)c.log_n, false, (size_t)c.log_mem);
}
void rw_proof_coordinate_range_check_and_open(const cozk_rw_proof_config& c, StarNetCoordinator& net, Transcript& tr, bool& with_ts, TsRangeProof& range, ReducedOpeningProof& reduced) {
    with_ts = c.with_ts != 0;
    if (c.with_ts) ts_range_check_coordinate(net, tr, (size_t)c.log_n, range);
    reduced = mc_coordinate_reduce_and_prove(net, tr);
}

void rw_proof_coordinate(cozk_rw_proof* h, StarNetCoordinator& net, RwProof& proof) {
    const cozk_rw_proof_config& c = h->cfg;
    Transcript tr("cozk-rw-memory");
    rw_proof_coordinate_memory_check(c, net, tr, proof.commitments, proof.mem);
    rw_proof_coordinate_range_check_and_open(c, net, tr, proof.with_ts, proof.range, proof.reduced);
}

// The plain verifier, in the two steps of the worker (shared with cozk_memory_proof): it replays the transcript `vt`; the first check that
// fails names itself in `why`.  The memory check leaves its two openings in `opens`.
bool rw_proof_verify_memory_check(cozk_rw_proof* h, const std::vector<PST13Commitment>& commitments, const MemCheckProof& mp, Transcript& vt, VerifierOpenings& opens, std::string& why) {
    const cozk_rw_proof_config& c = h->cfg;
    const size_t ns = (size_t)h->ns;
    const RwProofIdx ix(ns, c.with_ts != 0);
    if (commitments.size() != ix.count || mp.rw_hashes.size() != 2 * ns || mp.if_hashes.size() != 2 || mp.rw_claims.size() != ix.n_rw || mp.if_claims.size() != 2) {
        why = "shape: commitments, hashes or claims";
        return false;
    }
    for (auto& cm : commitments) vt.append_point(cm.g_product);
    const fe gamma = vt.challenge_scalar(), tau = vt.challenge_scalar();
    fe lhs = mp.if_hashes[0], rhs = mp.if_hashes[1];
    for (size_t s = 0; s < ns; s++) {
        lhs = Fr::mul(lhs, mp.rw_hashes[2 * s + 1]);
        rhs = Fr::mul(rhs, mp.rw_hashes[2 * s]);
    }
    if (!Fr::eq(lhs, rhs)) {
        why = "multiset equality: init * writes != reads * final";
        return false;
    }
    MemCheckPoints pts;
    if (!mc_verify_grand_products(mp, false, 2 * ns, 2, (size_t)c.log_n, (size_t)c.log_mem, vt, pts)) {
        why = "grand product: the hashes are not the outputs, or a round or a layer reduction does not hold";
        return false;
    }
    std::vector<size_t> rw_polys(ix.n_rw);
    for (size_t i = 0; i < ix.n_rw; i++) rw_polys[i] = i;
    opens.take(rw_polys, pts.lo, mp.rw_claims);
    opens.take(std::vector<size_t>{ix.v_final, ix.t_final}, pts.lo2, mp.if_claims);
    std::vector<RwSlotClaims> slots;
    for (size_t s = 0; s < ns; s++) slots.push_back({ix.addr + s, ix.v_read + s, rw_slot_writes((int)s) ? ix.v_written + (s - 2) : ix.v_read + s, ix.t_read + s});
    std::vector<fe> vi(h->v_init_clear.size());
    for (size_t a = 0; a < vi.size(); a++) vi[a] = Fr::from_u64(h->v_init_clear[a]);
    fe rw_claim, if_claim;  // VerifierComputedOpening of the public v_init
    rw_memory_verify_leaves(mp.rw_claims, mp.if_claims, slots, mc_mle_host(vi, pts.lo2), gamma, tau, pts, rw_claim, if_claim);
    if (!Fr::eq(rw_claim, pts.rw_claim) || !Fr::eq(if_claim, pts.if_claim)) {
        why = "leaf claim: the fingerprints of the claims != a grand product's final claim";
        return false;
    }
    return true;
}
// the range check (with with_ts) and the reduced opening over `opens` and the range check's own
bool rw_proof_verify_range_check_and_open(cozk_rw_proof* h, const std::vector<PST13Commitment>& commitments, const TsRangeProof& range, const ReducedOpeningProof& reduced,
                                          Transcript& vt, VerifierOpenings& opens, std::string& why) {
    const cozk_rw_proof_config& c = h->cfg;
    const size_t ns = (size_t)h->ns;
    const RwProofIdx ix(ns, c.with_ts != 0);
    if (c.with_ts) {
        std::vector<size_t> polys;
        for (size_t f = 0; f < 4; f++)
            for (size_t s = 0; s < ns; s++) polys.push_back(ix.rc_rt + f * ns + s);
        for (size_t s = 0; s < ns; s++) polys.push_back(ix.t_read + s);  // the step-1 commitments
        std::string inner;
        if (!ts_range_check_verify(vt, ns, (size_t)c.log_n, range, polys, inner, opens)) {
            why = "timestamp: " + inner;
            return false;
        }
    }
    return mc_verify_opening(opens, commitments, reduced, *h->parties[0].setup, why);
}
bool rw_proof_verify(cozk_rw_proof* h, const RwProof& proof, std::string& why) {
    Transcript vt("cozk-rw-memory");
    VerifierOpenings opens(vt);
    return rw_proof_verify_memory_check(h, proof.commitments, proof.mem, vt, opens, why) &&
           rw_proof_verify_range_check_and_open(h, proof.commitments, proof.range, proof.reduced, vt, opens, why);
}

// what create checks of a config and builds from it, for both harnesses (`who` names the harness in the refusals; max_tamper: its last tamper)
void rw_proof_check_config(const cozk_rw_proof_config& c, const std::string& who, int max_tamper) {
    COZK_REQUIRE(c.mode == COZK_MODE_PLAIN, who + ": the proof is party 0's public one: mode is COZK_MODE_PLAIN");
    COZK_REQUIRE(c.log_n >= 1 && c.log_n <= 22, who + ": log_n in 1..22");
    COZK_REQUIRE(c.log_mem >= 5 && c.log_mem <= 24, who + ": log_mem in 5..24");
    COZK_REQUIRE(c.n_slots >= 1 && c.n_slots <= 4, who + ": n_slots in 1..4");
    COZK_REQUIRE((c.with_ts == 0 || c.with_ts == 1) && (c.leaves_fused == 0 || c.leaves_fused == 1), who + ": with_ts and leaves_fused are 0 or 1");
    COZK_REQUIRE(c.tamper >= 0 && c.tamper <= max_tamper && (c.tamper != 3 || c.with_ts), who + ": tamper in 0.." + std::to_string(max_tamper) + ", 3 only with with_ts");
}
void rw_proof_build(cozk_rw_proof* h, const std::string& who) {
    const cozk_rw_proof_config& c = h->cfg;
    h->N = (size_t)1 << c.log_n;
    h->MEM = (size_t)1 << c.log_mem;
    h->ns = c.n_slots;
    h->parties.resize(1);
    RwProofParty& ps = h->parties[0];
    ps.party = 0;
    ps.open_ctx(c.device, (who + ": cannot create a context (no HIP device?)").c_str());
    rw_proof_setup(h, ps);
}
void rw_proof_release(cozk_rw_proof* h) {
    release_parties(h->parties, [](RwProofParty& ps) {
        for (std::vector<VecH>* fam : {&ps.addr, &ps.v_read, &ps.t_read, &ps.v_written, &ps.rc_rt, &ps.rc_gmr, &ps.fc_rt, &ps.fc_gmr}) fam->clear();
        for (VecH* v : {&ps.v_init, &ps.v_final, &ps.t_final, &ps.iota_n, &ps.iota_mem}) *v = VecH();
        ps.setup.reset();
    });
}

}  // namespace

extern "C" {

int cozk_rw_proof_create(const cozk_rw_proof_config* cfg, cozk_rw_proof** out) {
    return harness_create(cfg, out, [&](cozk_rw_proof* h) {
        rw_proof_check_config(*cfg, "rw_proof", 3);
        rw_proof_build(h, "rw_proof");
    });
}

const char* cozk_rw_proof_error(const cozk_rw_proof* h) { return harness_error(h); }

int cozk_rw_proof_destroy(cozk_rw_proof* h) {
    if (!h) return COZK_OK;
    rw_proof_release(h);
    delete h;
    return COZK_OK;
}

int cozk_rw_proof_prove(cozk_rw_proof* h, int verify, cozk_rw_proof_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (h->parties.empty() || !h->parties[0].setup) return COZK_ERR_INVALID_ARG;  // create failed
    RwProof proof;
    int rc = prove_by_one_party(
        h, h->parties, verify, res, [&](RwProofParty& ps, StarNetWorker* star) { rw_proof_worker_main(h, ps, star); },
        [&](StarNetCoordinator& net) { rw_proof_coordinate(h, net, proof); }, [&](std::string& why) { return rw_proof_verify(h, proof, why); });
    if (rc != COZK_OK) return rc;
    const RwProofParty& ps = h->parties[0];
    res->t_witness_ms = h->t_witness;
    res->t_commit_ms = ps.t_commit;
    res->t_leaves_ms = ps.t_leaves;
    res->t_gp_ms = ps.t_gp;
    res->t_ts_ms = ps.t_ts;
    res->t_open_ms = ps.t_open;
    finish_proof(h, proof.serialize(), res);
    return COZK_OK;
}

int cozk_rw_proof_proof_bytes(const cozk_rw_proof* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
