// In-process harness of party 0's timestamp range-check proof (TimestampValidityProof::prove, called after the output check at
// co-jolt/src/jolt/vm/read_write_memory/worker.rs:78-105; its single batched opening goes to the other parties through append_public /
// receive_public_opening): over public data, every t_read[s][j] and every j - t_read[s][j] lies in [0, N) -- a Lasso memory check over
// an identity table of N entries with ONE batched dense grand product and ONE batched opening.  jolt-core is not in the reference
// tree, so the circuit order, the transcript order and the proof bytes are this project's: PARITY UNPINNED.  What pins them is the
// plain verifier at the end of this file and the Python restatement tests/ts_proof_ref.py (include/cozk.h has the protocol).
// Every polynomial is a compact U32 column on the device: the commit takes the MSM's small-scalar path, the leaves come from
// cozk_timestamp_range_leaves, the claims and the joint polynomial from the compact opening calls; no Fr copy of a column exists.
// Worker on the device, coordinator and verifier on the calling thread through run_in_process, one transcript.
#pragma once

struct TsProofParty : HarnessParty {
    std::vector<VecH> t_read, rc_rt, rc_gmr, fc_rt, fc_gmr;  // n_slots U32[N] each
    VecH iota;                                               // the composition's step column (leaves_fused = 0)
    std::unique_ptr<PST13Setup> setup;
    double t_commit = 0, t_leaves = 0, t_gp = 0, t_open = 0;
};

struct cozk_ts_proof : HarnessHandle {
    cozk_ts_proof_config cfg;
    size_t N = 0;
    int ns = 0;
    double t_witness = 0;
    std::vector<TsProofParty> parties;  // party 0 alone
};

namespace {

// what the range check itself adds to a proof (steps 2-5): cozk_rw_proof chains it behind the memory check
struct TsRangeProof {
    std::vector<fe> hashes;
    GrandProductProof gp;
    std::vector<fe> claims;
    void write(Writer& w) const {
        w.vec_fr(hashes);
        gp.write(w);
        w.vec_fr(claims);
    }
};

struct TsProof {
    std::vector<PST13Commitment> commitments;
    TsRangeProof range;
    ReducedOpeningProof reduced;
    Bytes serialize() const {
        Writer w;
        w.u64(commitments.size());
        for (auto& c : commitments) c.write(w);
        range.write(w);
        reduced.write(w);
        return w.b;
    }
};

// the range check's columns as the steps below take them: n_slots U32[N] handles per family; iota only for the composed leaves
struct TsRangeCols {
    std::vector<const cozk_vec*> t_read, rc_rt, rc_gmr, fc_rt, fc_gmr;
    const cozk_vec* iota = nullptr;
    // the order of the claims (and of cozk_ts_proof's commitments): family-major, then t_read
    std::vector<const cozk_vec*> columns() const {
        std::vector<const cozk_vec*> cols;
        for (const std::vector<const cozk_vec*>* fam : {&rc_rt, &rc_gmr, &fc_rt, &fc_gmr, &t_read}) cols.insert(cols.end(), fam->begin(), fam->end());
        return cols;
    }
};

// SplitMix64 as oracle/pyref.py's class: one sequential stream
struct TsSplitMix {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

// P: a party that holds the five families as std::vector<VecH> (TsProofParty, RwProofParty)
template <class P>
TsRangeCols ts_range_columns(const P& ps, const VecH& iota) {
    TsRangeCols c;
    const std::vector<VecH>* fam[5] = {&ps.t_read, &ps.rc_rt, &ps.rc_gmr, &ps.fc_rt, &ps.fc_gmr};
    std::vector<const cozk_vec*>* dst[5] = {&c.t_read, &c.rc_rt, &c.rc_gmr, &c.fc_rt, &c.fc_gmr};
    for (int k = 0; k < 5; k++)
        for (const VecH& v : *fam[k]) dst[k]->push_back(v.h);
    c.iota = iota.h;
    return c;
}

// tests/rw_witness_ref.py's jolt_instance(seed, N, MEM, store_pct = 30, n_regs = 32): the addresses of rs1, rs2, rd, ram, the written values
// of rd and ram, ram's store flags and v_init
struct TsTrace {
    std::vector<std::vector<uint32_t>> addr, vw;
    std::vector<uint8_t> iw;
    std::vector<uint32_t> v_init;
};
TsTrace ts_trace(uint64_t seed, size_t N, size_t MEM) {
    TsTrace t;
    t.addr.assign(4, std::vector<uint32_t>(N));
    t.vw.assign(2, std::vector<uint32_t>(N));
    t.iw.resize(N);
    t.v_init.resize(MEM);
    TsSplitMix rng{seed};
    const uint64_t n_regs = MEM < 32 ? MEM : 32;
    for (int s = 0; s < 3; s++)
        for (size_t j = 0; j < N; j++) t.addr[(size_t)s][j] = (uint32_t)(rng.next() % n_regs);
    for (size_t j = 0; j < N; j++) t.addr[3][j] = (uint32_t)(rng.next() % MEM);
    for (int k = 0; k < 2; k++)
        for (size_t j = 0; j < N; j++) t.vw[(size_t)k][j] = (uint32_t)rng.next();
    for (size_t j = 0; j < N; j++) t.iw[j] = rng.next() % 100 < 30 ? 1 : 0;
    for (size_t a = 0; a < MEM; a++) t.v_init[a] = (uint32_t)rng.next();
    return t;
}

// tamper 1: one final counter of the read-timestamp family of slot 0 is bumped: every relation but the multiset's holds
void ts_tamper_final_counter(cozk_ctx* ctx, const VecH& t_read0, VecH& fc_rt0, size_t N) {
    std::vector<uint32_t> tr0(N), fc(N);
    rc_check(cozk_vec_download(ctx, t_read0.h, tr0.data()), ctx, "vec_download");
    rc_check(cozk_vec_download(ctx, fc_rt0.h, fc.data()), ctx, "vec_download");
    fc[tr0[N / 2]] += 1;
    fc_rt0 = upload_vec(ctx, fc.data(), N, COZK_SCALAR_U32, "vec_upload(tampered counters)");
}

// create: tests/rw_witness_ref.py's jolt_instance(seed, N, MEM, store_pct = 30, n_regs = 32), both witness walks on the device
void ts_proof_setup(cozk_ts_proof* h, TsProofParty& ps) {
    const cozk_ts_proof_config& c = h->cfg;
    cozk_ctx* ctx = ps.ctx;
    const size_t N = h->N, MEM = (size_t)1 << c.log_mem;
    const int ns = h->ns;
    std::vector<fe> t((size_t)c.log_n);
    for (int i = 0; i < c.log_n; i++) t[(size_t)i] = synthetic_fr_host(c.seed ^ 0x7A7A7A7Aull, (uint64_t)i);
    ps.setup = PST13::setup(ctx, t, c.precompute);
    const TsTrace trace = ts_trace(c.seed, N, MEM);
    double t0 = now_ms();
    std::vector<VecH> d_addr, d_vw;
    for (int s = 0; s < 4; s++) d_addr.push_back(upload_vec(ctx, trace.addr[(size_t)s].data(), N, COZK_SCALAR_U32, "vec_upload(addresses)"));
    for (int k = 0; k < 2; k++) d_vw.push_back(upload_vec(ctx, trace.vw[(size_t)k].data(), N, COZK_SCALAR_U32, "vec_upload(written values)"));
    VecH d_iw = upload_vec(ctx, trace.iw.data(), N, COZK_SCALAR_U8, "vec_upload(store flags)");
    VecH d_init = upload_vec(ctx, trace.v_init.data(), MEM, COZK_SCALAR_U32, "vec_upload(v_init)");
    const cozk_vec* pa[4] = {d_addr[0].h, d_addr[1].h, d_addr[2].h, d_addr[3].h};
    const cozk_vec* pw[4] = {nullptr, nullptr, d_vw[0].h, d_vw[1].h};
    const cozk_vec* pf[4] = {nullptr, nullptr, nullptr, d_iw.h};
    cozk_vec *v_read[4] = {}, *t_read[4] = {}, *v_written[4] = {}, *v_final = nullptr, *t_final = nullptr;
    rc_check(cozk_rw_memory_witness(ctx, pa, pw, pf, 4, d_init.h, v_read, t_read, v_written, &v_final, &t_final), ctx, "rw_memory_witness");
    for (int s = 0; s < 4; s++) {
        cozk_vec_free(v_read[s]);
        cozk_vec_free(v_written[s]);
        if (s < ns) ps.t_read.push_back(VecH(t_read[s]));
        else cozk_vec_free(t_read[s]);
    }
    cozk_vec_free(v_final);
    cozk_vec_free(t_final);
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
    h->t_witness = now_ms() - t0;
    if (c.tamper == 1) ts_tamper_final_counter(ctx, ps.t_read[0], ps.fc_rt[0], N);
    if (!c.leaves_fused) {
        std::vector<uint32_t> io(N);
        for (size_t j = 0; j < N; j++) io[j] = (uint32_t)j;
        ps.iota = upload_vec(ctx, io.data(), N, COZK_SCALAR_U32, "vec_upload(iota)");
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// the 6 n_slots + 1 circuits as 25 (at 4 slots) cozk_fingerprint_leaves calls: what cozk_timestamp_range_leaves replaces
void ts_proof_leaves_composed(WorkerEnv& env, const TsRangeCols& ps, int ns, size_t N, const fe& gamma, const fe& tau, LeafBuf& lb) {
    const fe g1 = Fr::add(gamma, Fr::one()), g2 = Fr::mul(gamma, gamma), ntau = Fr::neg(tau), w = Fr::sub(g2, tau);
    for (int s = 0; s < ns; s++) {
        const size_t u = (size_t)s;
        std::vector<LeafTerm> rt = {mc_col_term(ps.t_read[u], g1), mc_col_term(ps.rc_rt[u], g2)};
        std::vector<LeafTerm> gmr = {mc_col_term(ps.iota, g1), mc_col_term(ps.t_read[u], Fr::neg(g1)), mc_col_term(ps.rc_gmr[u], g2)};
        mc_fingerprint_leaves(env, rt, ntau, lb, (4 * u) * N, N);
        mc_fingerprint_leaves(env, rt, w, lb, (4 * u + 1) * N, N);
        mc_fingerprint_leaves(env, gmr, ntau, lb, (4 * u + 2) * N, N);
        mc_fingerprint_leaves(env, gmr, w, lb, (4 * u + 3) * N, N);
        mc_fingerprint_leaves(env, {mc_col_term(ps.iota, g1), mc_col_term(ps.fc_rt[u], g2)}, ntau, lb, (4 * (size_t)ns + 1 + 2 * u) * N, N);
        mc_fingerprint_leaves(env, {mc_col_term(ps.iota, g1), mc_col_term(ps.fc_gmr[u], g2)}, ntau, lb, (4 * (size_t)ns + 2 + 2 * u) * N, N);
    }
    mc_fingerprint_leaves(env, {mc_col_term(ps.iota, g1)}, ntau, lb, (4 * (size_t)ns) * N, N);
    rc_check(cozk_ctx_synchronize(env.ctx), env.ctx, "synchronize");
}

// steps 2-5 of the worker under the caller's transcript and accumulator (cozk_ts_proof after its commit, cozk_rw_proof after the memory
// check): gamma and tau, the leaves, the batched grand product, the claims at r_lo and the joint opening.  tamper_claim: claim 0 plus one.
// Returns the clock taken after the grand product: step 5 belongs to the opening phase of cozk_ts_proof (t_open_ms).
double ts_range_check_worker(WorkerEnv& env, const TsRangeCols& rc, size_t N, bool leaves_fused, bool tamper_claim, Rep3ProverOpeningAccumulator& acc, double& t_leaves,
                           double& t_gp) {
    StarNetWorker* star = env.star;
    const int ns = (int)rc.t_read.size();
    const size_t circuits = 6 * (size_t)ns + 1;
    const std::vector<const cozk_vec*> cols = rc.columns();
    // ---- 2, 3. gamma, tau; the leaves
    fe gamma, tau;
    mc_receive_gamma_tau(star, gamma, tau);
    double t2 = now_ms();
    LeafBuf lb = mc_leaf_alloc(env, circuits * N);
    if (leaves_fused) {
        uint64_t g[4], t[4];
        fe_to_u64x4(gamma, g);
        fe_to_u64x4(tau, t);
        rc_check(cozk_timestamp_range_leaves(env.ctx, rc.t_read.data(), rc.rc_rt.data(), rc.rc_gmr.data(), rc.fc_rt.data(), rc.fc_gmr.data(), (size_t)ns, g, t, lb.a.h, 0),
                 env.ctx, "timestamp_range_leaves");
    } else {
        ts_proof_leaves_composed(env, rc, ns, N, gamma, tau, lb);
    }
    double t3 = now_ms();
    t_leaves = t3 - t2;
    // ---- 4. ONE dense batched grand product; its claimed outputs are the multiset hashes
    Rep3BatchedDenseGrandProduct gp = Rep3BatchedDenseGrandProduct::construct(env, mc_leaves_to_layer(env, lb), circuits);
    {
        Writer w;
        w.vec_fr(gp.claimed_outputs(env));
        star->send_response(w.b);
    }
    std::vector<fe> r = gp.prove_grand_product_worker(env);
    std::vector<fe> r_lo(r.begin() + ceil_log2(circuits), r.end());
    const double t4 = now_ms();
    t_gp = t4 - t3;
    // ---- 5. the claims at r_lo, one exchange, the joint polynomial from the compact columns
    compact_open_worker(env, acc, cols, r_lo, tamper_claim);
    return t4;
}

void ts_proof_worker_main(cozk_ts_proof* h, TsProofParty& ps, StarNetWorker* star) {
    const cozk_ts_proof_config& c = h->cfg;
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_PLAIN, 0, star, nullptr);
    const TsRangeCols rc = ts_range_columns(ps, ps.iota);
    const std::vector<const cozk_vec*> cols = rc.columns();
    double t0 = now_ms();
    // ---- 1. commit (the U32 small-scalar path).  Not mc_commit_worker: this is cozk_batch_msm_vec, which refuses columns of unequal
    // length and names itself in a failure, where PST13::batch_commit calls cozk_batch_msm_slices
    {
        std::vector<uint64_t> xy(8 * cols.size());
        std::vector<int> inf(cols.size());
        rc_check(cozk_batch_msm_vec(ps.ctx, ps.setup->powers_all, 0, cols.data(), cols.size(), xy.data(), inf.data()), ps.ctx, "batch_msm_vec");
        Writer w;
        w.u64(cols.size());
        for (size_t i = 0; i < cols.size(); i++) PST13Commitment{(uint64_t)c.log_n, abi_to_g1(xy.data() + 8 * i, inf[i])}.write(w);
        star->send_response(w.b);
    }
    ps.t_commit = now_ms() - t0;
    // ---- 2-5. the range check
    Rep3ProverOpeningAccumulator acc;
    const double t4 = ts_range_check_worker(env, rc, h->N, c.leaves_fused != 0, c.tamper == 2, acc, ps.t_leaves, ps.t_gp);
    // ---- 6. one reduce_and_prove (t_open: step 5 and this)
    acc.reduce_and_prove_worker(env, *ps.setup);
    ps.t_open = now_ms() - t4;
    ps.record_net(star);
}

// the coordinator's half of ts_range_check_worker
void ts_range_check_coordinate(StarNetCoordinator& net, Transcript& tr, size_t log_n, TsRangeProof& proof) {
    mc_broadcast_gamma_tau(net, tr);
    proof.hashes = gather_additive(net);
    tr.append_scalars(proof.hashes);
    fe claim;
    std::vector<fe> r;
    proof.gp = coordinate_prove_grand_product(net, tr, log_n, claim, r);
    proof.claims = Rep3ProverOpeningAccumulator::receive_claims(net, tr);
}

void ts_proof_coordinate(cozk_ts_proof* h, StarNetCoordinator& net, TsProof& proof) {
    Transcript tr("cozk-ts-range");
    mc_receive_commitments(net, tr, proof.commitments);
    ts_range_check_coordinate(net, tr, (size_t)h->cfg.log_n, proof.range);
    proof.reduced = mc_coordinate_reduce_and_prove(net, tr);
}

// The verifier's half of the range check after the commitments are in the transcript: the first three checks; `opens` takes the
// opening of the commitments `polys` (family-major, then t_read).
bool ts_range_check_verify(Transcript& vt, size_t ns, size_t log_n, const TsRangeProof& proof, const std::vector<size_t>& polys, std::string& why, VerifierOpenings& opens) {
    const size_t circuits = 6 * ns + 1, ncols = 5 * ns;
    if (proof.hashes.size() != circuits || proof.claims.size() != ncols) {
        why = "shape: commitments, hashes or claims";
        return false;
    }
    const fe gamma = vt.challenge_scalar(), tau = vt.challenge_scalar();
    const fe g1 = Fr::add(gamma, Fr::one()), g2 = Fr::mul(gamma, gamma);
    vt.append_scalars(proof.hashes);
    const std::vector<fe>& hs = proof.hashes;
    for (size_t s = 0; s < ns; s++)
        for (size_t kind = 0; kind < 2; kind++)
            if (!Fr::eq(Fr::mul(hs[4 * ns], hs[4 * s + 2 * kind + 1]), Fr::mul(hs[4 * s + 2 * kind], hs[4 * ns + 1 + 2 * s + kind]))) {
                why = "multiset equality: init * write != read * final (slot " + std::to_string(s) + (kind ? ", global minus read)" : ", read timestamp)");
                return false;
            }
    fe claim, unused;
    std::vector<fe> hi, lo;
    if (!mc_verify_grand_product(proof.gp, proof.hashes, false, circuits, log_n, vt, claim, unused, hi, lo)) {
        why = "grand product: the hashes are not its outputs, or a round or a layer reduction does not hold";
        return false;
    }
    const std::vector<fe>& cl = proof.claims;
    const fe iota = mc_iota_eval(lo), init = Fr::sub(Fr::mul(iota, g1), tau);
    std::vector<fe> leaves(circuits);
    for (size_t s = 0; s < ns; s++) {
        const fe &rc_rt = cl[s], &rc_gmr = cl[ns + s], &fc_rt = cl[2 * ns + s], &fc_gmr = cl[3 * ns + s], &t_read = cl[4 * ns + s];
        const fe xg = Fr::mul(t_read, g1);
        leaves[4 * s] = Fr::add(Fr::sub(xg, tau), Fr::mul(rc_rt, g2));
        leaves[4 * s + 1] = Fr::add(leaves[4 * s], g2);
        leaves[4 * s + 2] = Fr::add(Fr::sub(init, xg), Fr::mul(rc_gmr, g2));
        leaves[4 * s + 3] = Fr::add(leaves[4 * s + 2], g2);
        leaves[4 * ns + 1 + 2 * s] = Fr::add(init, Fr::mul(fc_rt, g2));
        leaves[4 * ns + 2 + 2 * s] = Fr::add(init, Fr::mul(fc_gmr, g2));
    }
    leaves[4 * ns] = init;
    if (!Fr::eq(mc_batch_eval(leaves, hi, Fr::zero()), claim)) {
        why = "leaf claim: the fingerprints of the claims != the grand product's final claim";
        return false;
    }
    opens.take(polys, lo, cl);
    return true;
}

// the plain verifier: replays the transcript; the first check that fails names itself in `why`
bool ts_proof_verify(cozk_ts_proof* h, const TsProof& proof, std::string& why) {
    const size_t ns = (size_t)h->ns, ncols = 5 * ns;
    Transcript vt("cozk-ts-range");
    if (proof.commitments.size() != ncols) {
        why = "shape: commitments, hashes or claims";
        return false;
    }
    for (auto& cm : proof.commitments) vt.append_point(cm.g_product);
    std::vector<size_t> polys(ncols);
    for (size_t i = 0; i < ncols; i++) polys[i] = i;
    VerifierOpenings opens(vt);
    return ts_range_check_verify(vt, ns, (size_t)h->cfg.log_n, proof.range, polys, why, opens) &&
           mc_verify_opening(opens, proof.commitments, proof.reduced, *h->parties[0].setup, why);
}

}  // namespace

extern "C" {

int cozk_ts_proof_create(const cozk_ts_proof_config* cfg, cozk_ts_proof** out) {
    return harness_create(cfg, out, [&](cozk_ts_proof* h) {
        COZK_REQUIRE(cfg->mode == COZK_MODE_PLAIN, "ts_proof: the proof is party 0's public one: mode is COZK_MODE_PLAIN");
        COZK_REQUIRE(cfg->log_n >= 1 && cfg->log_n <= 22, "ts_proof: log_n in 1..22");
        COZK_REQUIRE(cfg->log_mem >= 5 && cfg->log_mem <= 24, "ts_proof: log_mem in 5..24");
        COZK_REQUIRE(cfg->n_slots >= 1 && cfg->n_slots <= 4, "ts_proof: n_slots in 1..4");
        COZK_REQUIRE(cfg->tamper >= 0 && cfg->tamper <= 2 && (cfg->leaves_fused == 0 || cfg->leaves_fused == 1), "ts_proof: tamper in 0..2, leaves_fused 0 or 1");
        h->N = (size_t)1 << cfg->log_n;
        h->ns = cfg->n_slots;
        h->parties.resize(1);
        TsProofParty& ps = h->parties[0];
        ps.party = 0;
        ps.open_ctx(cfg->device, "ts_proof: cannot create a context (no HIP device?)");
        ts_proof_setup(h, ps);
    });
}

const char* cozk_ts_proof_error(const cozk_ts_proof* h) { return harness_error(h); }

int cozk_ts_proof_destroy(cozk_ts_proof* h) {
    if (!h) return COZK_OK;
    release_parties(h->parties, [](TsProofParty& ps) {
        for (std::vector<VecH>* fam : {&ps.t_read, &ps.rc_rt, &ps.rc_gmr, &ps.fc_rt, &ps.fc_gmr}) fam->clear();
        ps.iota = VecH();
        ps.setup.reset();
    });
    delete h;
    return COZK_OK;
}

int cozk_ts_proof_prove(cozk_ts_proof* h, int verify, cozk_ts_proof_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (h->parties.empty() || !h->parties[0].setup) return COZK_ERR_INVALID_ARG;  // create failed
    TsProof proof;
    int rc = prove_by_one_party(
        h, h->parties, verify, res, [&](TsProofParty& ps, StarNetWorker* star) { ts_proof_worker_main(h, ps, star); },
        [&](StarNetCoordinator& net) { ts_proof_coordinate(h, net, proof); }, [&](std::string& why) { return ts_proof_verify(h, proof, why); });
    if (rc != COZK_OK) return rc;
    const TsProofParty& ps = h->parties[0];
    res->t_witness_ms = h->t_witness;
    res->t_commit_ms = ps.t_commit;
    res->t_leaves_ms = ps.t_leaves;
    res->t_gp_ms = ps.t_gp;
    res->t_open_ms = ps.t_open;
    finish_proof(h, proof.serialize(), res);
    return COZK_OK;
}

int cozk_ts_proof_proof_bytes(const cozk_ts_proof* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
