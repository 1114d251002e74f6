// In-process harness of party 0's bytecode proof over a consistent witness (Rep3BytecodeProver, bytecode/worker.rs:43-142, as the plain
// dealer runs it): init * writes == reads * final over what cozk_bytecode_witness returns.  The chained flow's phase 2
// (flow_bytecode_worker) runs the same circuits on seeded values, whose multiset check cannot hold; here the verifier runs it.  The
// steps are memcheck_steps.hpp's; what is this file's own is the ONE opening at r_rw that joins the seven compact columns with the
// field column v_imm, and the leaf check over the six public table columns.  jolt-core is not in the reference tree: the transcript
// order and the proof bytes are this project's, PARITY UNPINNED; the plain verifier at the end of this file and tests/bytecode_ref.py
// pin them (include/cozk.h has the protocol).
#pragma once

struct BytecodeProofParty : HarnessParty {
    VecH a, t_read, t_final, v_imm_view;  // v_imm_view: the FR vector of v_imm, for the commit
    std::vector<VecH> v_read, table;      // five gathered columns; the six table columns (imm as I64)
    PolyH v_imm;
    VecH iota, imm_u64;                   // the composition's row column and the imm bits as U64 (leaves_fused = 0)
    std::unique_ptr<PST13Setup> setup;
    double t_commit = 0, t_leaves = 0, t_gp = 0, t_open = 0;
};

struct cozk_bytecode_proof : HarnessHandle {
    cozk_bytecode_proof_config cfg;
    size_t N = 0, B = 0;
    double t_witness = 0;
    std::vector<uint64_t> table_clear[5];  // public preprocessing: the verifier evaluates the MLEs itself
    std::vector<int64_t> imm_clear;
    std::vector<BytecodeProofParty> parties;  // party 0 alone
};

namespace {

struct BytecodeProof {
    std::vector<PST13Commitment> commitments;
    MemCheckProof mem;
    ReducedOpeningProof reduced;
    Bytes serialize() const {
        Writer w;
        w.u64(commitments.size());
        for (auto& c : commitments) c.write(w);
        mem.write(w);
        reduced.write(w);
        return w.b;
    }
};

// tests/bytecode_ref.py bytecode_instance(seed, N, B): the table into h, the trace returned
std::vector<uint32_t> bytecode_instance(cozk_bytecode_proof* h) {
    const size_t N = h->N, B = h->B;
    TsSplitMix rng{h->cfg.seed};
    for (auto& c : h->table_clear) c.assign(B, 0);
    h->imm_clear.assign(B, 0);
    for (size_t i = 1; i < B; i++) {
        h->table_clear[0][i] = 0x80000000ull + 4 * i;
        h->table_clear[1][i] = rng.next() | (i % 3 == 0 ? 1ull << 63 : 0);
        const uint64_t w = rng.next();
        h->table_clear[2][i] = w & 31, h->table_clear[3][i] = (w >> 5) & 31, h->table_clear[4][i] = (w >> 10) & 31;
        h->imm_clear[i] = (int64_t)rng.next();
    }
    if (B > 2) h->imm_clear[1] = INT64_MIN, h->imm_clear[2] = INT64_MAX;
    const size_t pad = N / 8;
    std::vector<uint32_t> a(N, 0);
    uint64_t pc = 1 % B;
    for (size_t j = 0; j < N - pad; j++) {
        a[j] = (uint32_t)pc;
        const uint64_t w = rng.next();
        if (B > 1 && (w & 7) == 0) pc = 1 + (w >> 3) % (B - 1);
        else pc = pc + 1 < B ? pc + 1 : 1 % B;
    }
    return a;
}

void bytecode_proof_setup(cozk_bytecode_proof* h, BytecodeProofParty& ps) {
    const cozk_bytecode_proof_config& c = h->cfg;
    cozk_ctx* ctx = ps.ctx;
    const size_t N = h->N, B = h->B;
    const int nv = c.log_n > c.log_b ? c.log_n : c.log_b;
    std::vector<fe> t((size_t)nv);
    for (int i = 0; i < nv; i++) t[(size_t)i] = synthetic_fr_host(c.seed ^ 0x7A7A7A7Aull, (uint64_t)i);
    ps.setup = PST13::setup(ctx, t, c.precompute);
    const std::vector<uint32_t> a = bytecode_instance(h);
    ps.a = upload_vec(ctx, a.data(), N, COZK_SCALAR_U32, "vec_upload(a)");
    for (int k = 0; k < 2; k++) ps.table.push_back(upload_vec(ctx, h->table_clear[k].data(), B, COZK_SCALAR_U64, "vec_upload(table)"));
    for (int k = 2; k < 5; k++) {
        std::vector<uint8_t> r8(h->table_clear[k].begin(), h->table_clear[k].end());
        ps.table.push_back(upload_vec(ctx, r8.data(), B, COZK_SCALAR_U8, "vec_upload(table registers)"));
    }
    ps.table.push_back(upload_vec(ctx, h->imm_clear.data(), B, COZK_SCALAR_I64, "vec_upload(table imm)"));
    double t0 = now_ms();
    const cozk_vec* tb[6];
    for (int k = 0; k < 6; k++) tb[k] = ps.table[(size_t)k].h;
    cozk_vec *v_read[5] = {}, *v_imm = nullptr, *t_read = nullptr, *t_final = nullptr;
    rc_check(cozk_bytecode_witness(ctx, ps.a.h, tb, v_read, &v_imm, &t_read, &t_final), ctx, "bytecode_witness");
    h->t_witness = now_ms() - t0;
    for (int k = 0; k < 5; k++) ps.v_read.push_back(VecH(v_read[k]));
    ps.t_read = VecH(t_read);
    ps.t_final = VecH(t_final);
    {
        VecH vi(v_imm);
        ps.v_imm = plain_poly(ctx, vi);
    }
    cozk_vec* view = nullptr;
    rc_check(cozk_poly_share_view(ctx, ps.v_imm.h, 0, &view), ctx, "share_view");
    ps.v_imm_view = VecH(view);
    if (c.tamper == 1) {  // a read that the table does not hold: every relation but the multiset's holds
        std::vector<uint8_t> rd(N);
        rc_check(cozk_vec_download(ctx, ps.v_read[2].h, rd.data()), ctx, "vec_download");
        rd[N / 2] += 1;
        ps.v_read[2] = upload_vec(ctx, rd.data(), N, COZK_SCALAR_U8, "vec_upload(tampered v_rd)");
    }
    if (c.tamper == 3) {
        std::vector<uint32_t> tf(B);
        rc_check(cozk_vec_download(ctx, ps.t_final.h, tf.data()), ctx, "vec_download");
        tf[a[N / 2]] += 1;
        ps.t_final = upload_vec(ctx, tf.data(), B, COZK_SCALAR_U32, "vec_upload(tampered t_final)");
    }
    if (!c.leaves_fused) {
        std::vector<uint32_t> io(B);
        for (size_t j = 0; j < B; j++) io[j] = (uint32_t)j;
        ps.iota = upload_vec(ctx, io.data(), B, COZK_SCALAR_U32, "vec_upload(iota)");
        ps.imm_u64 = upload_vec(ctx, h->imm_clear.data(), B, COZK_SCALAR_U64, "vec_upload(imm bits)");
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// the seven compact columns of the read / write circuits in the commit order
std::vector<const cozk_vec*> bytecode_proof_read_columns(const BytecodeProofParty& ps) {
    std::vector<const cozk_vec*> cols = {ps.a.h};
    for (const VecH& v : ps.v_read) cols.push_back(v.h);
    cols.push_back(ps.t_read.h);
    return cols;
}

// the four circuits as flow_bytecode_worker's cozk_fingerprint_leaves launches with an iota column: what the two fused calls replace.
// The composition takes no I64 column, so the table's imm enters as from_i64(v) = bits(v) - 2^64 [v < 0]: its bits as a U64 column
// times ONE, and a U8 column of the signs (neg_flags) times -2^64.
void bytecode_proof_leaves_composed(WorkerEnv& env, const BytecodeProofParty& ps, const VecH& neg_flags, size_t N, size_t B, const fe& gamma, const fe& tau, LeafBuf& rw,
                                    LeafBuf& inf) {
    std::vector<fe> g = {Fr::one()};
    for (int j = 0; j < 7; j++) g.push_back(Fr::mul(g.back(), gamma));
    const std::vector<const cozk_vec*> rc = bytecode_proof_read_columns(ps);
    std::vector<LeafTerm> read;
    for (size_t k = 0; k < 7; k++) read.push_back(mc_col_term(rc[k], g[k + 1]));
    read.push_back(LeafTerm{nullptr, ps.v_imm.h, Fr::one()});
    mc_fingerprint_leaves(env, read, Fr::neg(tau), rw, 0, N);
    mc_fingerprint_leaves(env, read, Fr::sub(g[7], tau), rw, N, N);
    const fe m = Fr::neg(Fr::mul(Fr::from_u64(1ull << 32), Fr::from_u64(1ull << 32)));  // -2^64
    std::vector<LeafTerm> init = {mc_col_term(ps.iota.h, g[1])};
    for (size_t k = 0; k < 5; k++) init.push_back(mc_col_term(ps.table[k].h, g[k + 2]));
    init.push_back(mc_col_term(ps.imm_u64.h, Fr::one()));
    init.push_back(mc_col_term(neg_flags.h, m));
    mc_fingerprint_leaves(env, init, Fr::neg(tau), inf, 0, B);
    init.push_back(mc_col_term(ps.t_final.h, g[7]));
    mc_fingerprint_leaves(env, init, Fr::neg(tau), inf, B, B);
}

void bytecode_proof_worker_main(cozk_bytecode_proof* h, BytecodeProofParty& ps, StarNetWorker* star) {
    const cozk_bytecode_proof_config& c = h->cfg;
    const size_t N = h->N, B = h->B;
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_PLAIN, 0, star, nullptr);
    Rep3ProverOpeningAccumulator acc;
    const std::vector<const cozk_vec*> rc = bytecode_proof_read_columns(ps);
    double t0 = now_ms();
    // ---- 1. commit: a, v_address, v_bitflags, v_rd, v_rs1, v_rs2, t_read, v_imm (FR), t_final
    {
        std::vector<const cozk_vec*> all = rc;
        all.push_back(ps.v_imm_view.h);
        all.push_back(ps.t_final.h);
        mc_commit_worker(env, *ps.setup, all);
    }
    double t1 = now_ms();
    ps.t_commit = t1 - t0;
    // ---- 2. gamma, tau; the leaves
    fe gamma, tau;
    mc_receive_gamma_tau(star, gamma, tau);
    double t2 = now_ms();
    LeafBuf rw = mc_leaf_alloc(env, 2 * N), inf = mc_leaf_alloc(env, 2 * B);
    if (c.leaves_fused) {
        const cozk_vec *v[5], *tb[6];
        for (int k = 0; k < 5; k++) v[k] = ps.v_read[(size_t)k].h;
        for (int k = 0; k < 6; k++) tb[k] = ps.table[(size_t)k].h;
        uint64_t g[4], t[4];
        fe_to_u64x4(gamma, g);
        fe_to_u64x4(tau, t);
        rc_check(cozk_bytecode_leaves(env.ctx, ps.a.h, v, ps.t_read.h, ps.v_imm.h, g, t, COZK_MODE_PLAIN, 0, rw.a.h, nullptr, 0), env.ctx, "bytecode_leaves");
        rc_check(cozk_bytecode_init_final_leaves(env.ctx, tb, ps.t_final.h, g, t, COZK_MODE_PLAIN, 0, inf.a.h, nullptr, 0), env.ctx, "bytecode_init_final_leaves");
    } else {
        std::vector<uint8_t> neg(B);
        for (size_t i = 0; i < B; i++) neg[i] = h->imm_clear[i] < 0;
        VecH neg_flags = upload_vec(env.ctx, neg.data(), B, COZK_SCALAR_U8, "vec_upload(imm signs)");
        bytecode_proof_leaves_composed(env, ps, neg_flags, N, B, gamma, tau, rw, inf);
        rc_check(cozk_ctx_synchronize(env.ctx), env.ctx, "synchronize");  // neg_flags lives to the end of the launches
    }
    rc_check(cozk_ctx_synchronize(env.ctx), env.ctx, "synchronize");
    double t3 = now_ms();
    ps.t_leaves = t3 - t2;
    // ---- 3. the two grand products; their claimed outputs are the multiset hashes
    std::vector<fe> r_rw, r_if;
    mc_memory_checking(env, mc_leaves_to_layer(env, rw), 2, ToggleH(), mc_leaves_to_layer(env, inf), 2, r_rw, r_if);
    double t4 = now_ms();
    ps.t_gp = t4 - t3;
    // ---- 4. ONE opening at r_rw: seven compact claims and v_imm's on one eq table, one exchange, the joint polynomial over rho^0..rho^7
    {
        VecH chih = mc_eq_table(env, r_rw);
        std::vector<uint64_t> ev(4 * 8);
        rc_check(cozk_compact_batch_evaluate_at_chi(env.ctx, rc.data(), 7, chih.h, ev.data()), env.ctx, "compact_batch_evaluate");
        const cozk_poly* one[1] = {ps.v_imm.h};
        rc_check(cozk_poly_batch_evaluate_at_chi(env.ctx, one, 1, chih.h, ev.data() + 28), env.ctx, "batch_evaluate(v_imm)");
        std::vector<fe> claims(8);
        for (size_t i = 0; i < 8; i++) claims[i] = fe_from_u64x4(ev.data() + 4 * i);
        if (c.tamper == 2) claims[0] = Fr::add(claims[0], Fr::one());
        fe batched_claim;
        const std::vector<fe> rho = Rep3ProverOpeningAccumulator::exchange_claims(env, claims, batched_claim);
        const std::vector<uint64_t> cf = to_abi(std::vector<fe>(rho.begin(), rho.begin() + 7));
        cozk_vec* jv = nullptr;
        rc_check(cozk_compact_linear_combination(env.ctx, rc.data(), cf.data(), 7, &jv), env.ctx, "compact_linear_combination");
        VecH jvh(jv);
        PolyH j7 = plain_poly(env.ctx, jvh);
        const cozk_poly* two[2] = {j7.h, ps.v_imm.h};
        const std::vector<uint64_t> cf2 = to_abi({Fr::one(), rho[7]});
        cozk_poly* joint = nullptr;
        rc_check(cozk_poly_linear_combination(env.ctx, two, cf2.data(), 2, COZK_MODE_PLAIN, 0, &joint), env.ctx, "joint + rho^7 v_imm");
        acc.append_joint(env, PolyH(joint), chih.h, r_rw, batched_claim);
    }
    compact_open_worker(env, acc, {ps.t_final.h}, r_if, false);
    // ---- 5. ONE reduce_and_prove
    acc.reduce_and_prove_worker(env, *ps.setup);
    ps.t_open = now_ms() - t4;
    ps.record_net(star);
}

void bytecode_proof_coordinate(cozk_bytecode_proof* h, StarNetCoordinator& net, BytecodeProof& proof) {
    const cozk_bytecode_proof_config& c = h->cfg;
    Transcript tr("cozk-bytecode");
    mc_receive_commitments(net, tr, proof.commitments);
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.mem, (size_t)c.log_n, false, (size_t)c.log_b);
    proof.reduced = mc_coordinate_reduce_and_prove(net, tr);
}

// The plain verifier: it replays the transcript; the first check that fails names itself in `why`.
bool bytecode_proof_verify(cozk_bytecode_proof* h, const BytecodeProof& proof, std::string& why) {
    const cozk_bytecode_proof_config& c = h->cfg;
    const MemCheckProof& mp = proof.mem;
    Transcript vt("cozk-bytecode");
    VerifierOpenings opens(vt);
    if (proof.commitments.size() != 9 || mp.rw_hashes.size() != 2 || mp.if_hashes.size() != 2 || mp.rw_claims.size() != 8 || mp.if_claims.size() != 1) {
        why = "shape: commitments, hashes or claims";
        return false;
    }
    for (auto& cm : proof.commitments) vt.append_point(cm.g_product);
    const fe gamma = vt.challenge_scalar(), tau = vt.challenge_scalar();
    if (!Fr::eq(Fr::mul(mp.if_hashes[0], mp.rw_hashes[1]), Fr::mul(mp.rw_hashes[0], mp.if_hashes[1]))) {
        why = "multiset equality: init * writes != reads * final";
        return false;
    }
    MemCheckPoints pts;
    if (!mc_verify_grand_products(mp, false, 2, 2, (size_t)c.log_n, (size_t)c.log_b, vt, pts)) {
        why = "grand product: the hashes are not the outputs, or a round or a layer reduction does not hold";
        return false;
    }
    opens.take(std::vector<size_t>{0, 1, 2, 3, 4, 5, 6, 7}, pts.lo, mp.rw_claims);
    opens.take(std::vector<size_t>{8}, pts.lo2, mp.if_claims);
    std::vector<fe> g = {Fr::one()};
    for (int j = 0; j < 7; j++) g.push_back(Fr::mul(g.back(), gamma));
    // claims in the commit order: a, v_address .. v_rs2, t_read, v_imm
    fe read = Fr::sub(mp.rw_claims[7], tau);
    for (size_t k = 0; k < 7; k++) read = Fr::add(read, Fr::mul(g[k + 1], mp.rw_claims[k]));
    const std::vector<fe> eq2 = eq_evals_host(pts.lo2);
    fe init = Fr::sub(Fr::mul(g[1], mc_iota_eval(pts.lo2)), tau);
    for (size_t k = 0; k < 5; k++) {
        fe acc = Fr::zero();
        for (size_t i = 0; i < h->B; i++) acc = Fr::add(acc, Fr::mul(eq2[i], Fr::from_u64(h->table_clear[k][i])));
        init = Fr::add(init, Fr::mul(g[k + 2], acc));
    }
    for (size_t i = 0; i < h->B; i++) {
        const int64_t v = h->imm_clear[i];
        const fe m = Fr::from_u64(v < 0 ? 0 - (uint64_t)v : (uint64_t)v);
        init = Fr::add(init, Fr::mul(eq2[i], v < 0 ? Fr::neg(m) : m));
    }
    const fe fin = Fr::add(init, Fr::mul(g[7], mp.if_claims[0]));
    if (!Fr::eq(mc_batch_eval({read, Fr::add(read, g[7])}, pts.hi, Fr::zero()), pts.rw_claim) ||
        !Fr::eq(mc_batch_eval({init, fin}, pts.hi2, Fr::zero()), pts.if_claim)) {
        why = "leaf claim: the fingerprints of the claims != a grand product's final claim";
        return false;
    }
    return mc_verify_opening(opens, proof.commitments, proof.reduced, *h->parties[0].setup, why);
}

}  // namespace

extern "C" {

int cozk_bytecode_proof_create(const cozk_bytecode_proof_config* cfg, cozk_bytecode_proof** out) {
    return harness_create(cfg, out, [&](cozk_bytecode_proof* h) {
        const cozk_bytecode_proof_config& c = *cfg;
        COZK_REQUIRE(c.mode == COZK_MODE_PLAIN, "bytecode_proof: the proof is party 0's public one: mode is COZK_MODE_PLAIN");
        COZK_REQUIRE(c.log_n >= 1 && c.log_n <= 22, "bytecode_proof: log_n in 1..22");
        COZK_REQUIRE(c.log_b >= 1 && c.log_b <= 22, "bytecode_proof: log_b in 1..22");
        COZK_REQUIRE(c.leaves_fused == 0 || c.leaves_fused == 1, "bytecode_proof: leaves_fused is 0 or 1");
        COZK_REQUIRE(c.tamper >= 0 && c.tamper <= 3, "bytecode_proof: tamper in 0..3");
        h->N = (size_t)1 << c.log_n;
        h->B = (size_t)1 << c.log_b;
        h->parties.resize(1);
        BytecodeProofParty& ps = h->parties[0];
        ps.party = 0;
        ps.open_ctx(c.device, "bytecode_proof: cannot create a context (no HIP device?)");
        bytecode_proof_setup(h, ps);
    });
}

const char* cozk_bytecode_proof_error(const cozk_bytecode_proof* h) { return harness_error(h); }

int cozk_bytecode_proof_destroy(cozk_bytecode_proof* h) {
    if (!h) return COZK_OK;
    release_parties(h->parties, [](BytecodeProofParty& ps) {
        ps.v_read.clear();
        ps.table.clear();
        for (VecH* v : {&ps.a, &ps.t_read, &ps.t_final, &ps.v_imm_view, &ps.iota, &ps.imm_u64}) *v = VecH();
        ps.v_imm = PolyH();
        ps.setup.reset();
    });
    delete h;
    return COZK_OK;
}

int cozk_bytecode_proof_prove(cozk_bytecode_proof* h, int verify, cozk_bytecode_proof_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (h->parties.empty() || !h->parties[0].setup) return COZK_ERR_INVALID_ARG;  // create failed
    BytecodeProof proof;
    int rc = prove_by_one_party(
        h, h->parties, verify, res, [&](BytecodeProofParty& ps, StarNetWorker* star) { bytecode_proof_worker_main(h, ps, star); },
        [&](StarNetCoordinator& net) { bytecode_proof_coordinate(h, net, proof); }, [&](std::string& why) { return bytecode_proof_verify(h, proof, why); });
    if (rc != COZK_OK) return rc;
    const BytecodeProofParty& ps = h->parties[0];
    res->t_witness_ms = h->t_witness;
    res->t_commit_ms = ps.t_commit;
    res->t_leaves_ms = ps.t_leaves;
    res->t_gp_ms = ps.t_gp;
    res->t_open_ms = ps.t_open;
    finish_proof(h, proof.serialize(), res);
    return COZK_OK;
}

int cozk_bytecode_proof_proof_bytes(const cozk_bytecode_proof* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
