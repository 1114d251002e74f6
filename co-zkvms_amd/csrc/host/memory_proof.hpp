// In-process harness of party 0's whole ReadWriteMemoryProof in the reference's order (Rep3ReadWriteMemoryProver::prove,
// co-jolt/src/jolt/vm/read_write_memory/worker.rs:54-180): the memory check, the output check (prove_outputs, :110-175), the timestamp
// range check, under one transcript and one opening accumulator, with ONE reduce_and_prove.  The memory check and the range check
// are the steps of rw_memory_proof.hpp, called as they stand, so everything up to and including the claims at r_if is byte for byte
// cozk_rw_proof's proof at the same config.  New here is the output check over the CONSISTENT v_final:
//     sum_x eq(r_eq, x) io_range(x) (v_final(x) - v_io(x)) = 0,   degree 3, HighToLow, then one opening of v_final at the sumcheck's point.
// The io window is [io_start, io_start + io_len) words and v_io is v_final over it, so an honest run verifies.  windowed = 1: the rounds
// are cozk_output_check_* over the compact columns (output_check.inc); windowed = 0: the chained flow's composition (prove_outputs_dense_worker,
// memcheck_steps.hpp) on Fr copies of eq, io_range, v_io and v_final -- three MEM-entry Fr polynomials bound every round -- kept for the A/B, the same bytes.
// Either way the messages are prove_arbitrary_worker's (prove_arbitrary_rounds, the one round loop) and coordinate_prove_arbitrary serves
// them.  jolt-core is not in the reference tree: PARITY UNPINNED, pinned by the verifier below and tests/memory_proof_ref.py.
#pragma once

struct cozk_memory_proof : HarnessHandle {
    cozk_memory_proof_config cfg;
    cozk_rw_proof rw;                  // the trace, the witness, party 0 and the SRS: what cozk_rw_proof_create builds for the same fields
    std::vector<uint32_t> v_io_clear;  // the program's public output: the verifier evaluates it itself
    VecH v_io;                         // U32, io_len words
    VecH io_range_fr, v_io_fr, v_final_fr;  // windowed = 0: the Fr copies of MEM entries (made in create, as the flow's setup makes its own)
    double t_out = 0;
    uint64_t out_peak_bytes = 0;
};

namespace {

struct MemoryProof {
    std::vector<PST13Commitment> commitments;
    MemCheckProof mem;
    SumcheckProof outputs;
    std::vector<fe> outputs_claims;
    bool with_ts = false;
    TsRangeProof range;
    ReducedOpeningProof reduced;
    size_t prefix_len = 0;
    Bytes serialize() {
        Writer w;
        w.u64(commitments.size());
        for (auto& c : commitments) c.write(w);
        mem.write(w);
        prefix_len = w.b.size();
        outputs.write(w);
        w.vec_fr(outputs_claims);
        if (with_ts) range.write(w);
        reduced.write(w);
        return w.b;
    }
};

// what the phase holds on the device beyond what it found: the pool's peak over the phase plus the growth of the two scratch buffers
struct PhasePeak {
    cozk_ctx* ctx;
    size_t live0, scratch0;
    explicit PhasePeak(cozk_ctx* c) : ctx(c), live0(c->pool.live_bytes), scratch0(c->scratch.cap + c->scratch2.cap) { c->pool.peak_bytes = c->pool.live_bytes; }
    uint64_t bytes() const { return (uint64_t)(ctx->pool.peak_bytes - live0) + (uint64_t)(ctx->scratch.cap + ctx->scratch2.cap - scratch0); }
};

// the output check's sumcheck, windowed: the shared round loop (prove_outputs_windowed_worker, memcheck_steps.hpp) on the compact column's handle
std::vector<fe> memory_proof_outputs_windowed(cozk_memory_proof* h, WorkerEnv& env, const RwProofParty& ps, const std::vector<fe>& r_eq) {
    const std::vector<uint64_t> wabi = to_abi(r_eq);
    OutputCheckH oc;
    rc_check(cozk_output_check_create(env.ctx, ps.v_final.h, h->v_io.h, (size_t)h->cfg.io_start, wabi.data(), &oc.h), env.ctx, "output_check_create");
    return prove_outputs_windowed_worker(env, oc.h, h->cfg.log_mem, false);
}

// ... dense: the flow's composition on Fr copies
std::vector<fe> memory_proof_outputs_dense(cozk_memory_proof* h, WorkerEnv& env, const std::vector<fe>& r_eq) {
    PolyH pvf = plain_poly(env.ctx, h->v_final_fr);
    return prove_outputs_dense_worker(env, pvf.h, h->io_range_fr, h->v_io_fr, h->cfg.log_mem, r_eq);
}

void memory_proof_worker_main(cozk_memory_proof* h, RwProofParty& ps, StarNetWorker* star) {
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_PLAIN, 0, star, nullptr);
    const TsRangeCols range = ts_range_columns(ps, ps.iota_n);
    Rep3ProverOpeningAccumulator acc;
    // ---- 1-4. the memory check: cozk_rw_proof's steps
    const double t4 = rw_proof_memory_check_worker(&h->rw, ps, env, range, acc);
    const double t5 = now_ms();
    // ---- the output check: r_eq, log_mem rounds, one opening of v_final at the sumcheck's point
    {
        const std::vector<fe> r_eq = mc_receive_point(star);
        const double t0 = now_ms();
        std::vector<fe> r;
        {
            PhasePeak peak(env.ctx);
            r = h->cfg.windowed ? memory_proof_outputs_windowed(h, env, ps, r_eq) : memory_proof_outputs_dense(h, env, r_eq);
            h->out_peak_bytes = peak.bytes();
        }
        compact_open_worker(env, acc, {ps.v_final.h}, r, false);
        h->t_out = now_ms() - t0;
    }
    // ---- 5, 6. the range check and ONE reduce_and_prove: cozk_rw_proof's steps
    rw_proof_range_check_and_open_worker(&h->rw, ps, env, range, acc, t5 - t4);
}

void memory_proof_coordinate(cozk_memory_proof* h, StarNetCoordinator& net, MemoryProof& proof) {
    const cozk_rw_proof_config& c = h->rw.cfg;
    Transcript tr("cozk-rw-memory");
    rw_proof_coordinate_memory_check(c, net, tr, proof.commitments, proof.mem);
    coordinate_outputs(net, tr, c.log_mem, proof.outputs, proof.outputs_claims);
    rw_proof_coordinate_range_check_and_open(c, net, tr, proof.with_ts, proof.range, proof.reduced);
}

// io_range(r) and v_io(r) over the window only: O(W m), not MEM
void memory_proof_window_evals(const cozk_memory_proof* h, const std::vector<fe>& r, fe& range_r, fe& v_io_r) {
    const size_t m = r.size(), lo = (size_t)h->cfg.io_start;
    const fe one = Fr::one();
    std::vector<fe> omr(m);
    for (size_t i = 0; i < m; i++) omr[i] = Fr::sub(one, r[i]);
    range_r = v_io_r = Fr::zero();
    for (size_t j = 0; j < h->v_io_clear.size(); j++) {
        const size_t x = lo + j;
        fe e = one;
        for (size_t i = 0; i < m; i++) e = Fr::mul(e, ((x >> (m - 1 - i)) & 1) ? r[i] : omr[i]);
        range_r = Fr::add(range_r, e);
        v_io_r = Fr::add(v_io_r, Fr::mul(e, Fr::from_u64(h->v_io_clear[j])));
    }
}

bool memory_proof_verify(cozk_memory_proof* h, const MemoryProof& proof, std::string& why) {
    const cozk_rw_proof_config& c = h->rw.cfg;
    const RwProofIdx ix((size_t)h->rw.ns, c.with_ts != 0);
    Transcript vt("cozk-rw-memory");
    VerifierOpenings opens(vt);
    if (!rw_proof_verify_memory_check(&h->rw, proof.commitments, proof.mem, vt, opens, why)) return false;
    std::vector<fe> r_eq, r_out;
    fe claim, range_r, v_io_r;
    if (!verify_outputs(vt, c.log_mem, proof.outputs, proof.outputs_claims, r_eq, r_out, claim)) {
        why = "output check: shape";
        return false;
    }
    memory_proof_window_evals(h, r_out, range_r, v_io_r);
    if (!outputs_final_holds(r_eq, r_out, range_r, v_io_r, proof.outputs_claims[0], claim)) {
        why = "output check: final claim";
        return false;
    }
    opens.take(std::vector<size_t>{ix.v_final}, r_out, proof.outputs_claims);
    return rw_proof_verify_range_check_and_open(&h->rw, proof.commitments, proof.range, proof.reduced, vt, opens, why);
}

void memory_proof_setup(cozk_memory_proof* h) {
    const cozk_memory_proof_config& c = h->cfg;
    RwProofParty& ps = h->rw.parties[0];
    cozk_ctx* ctx = ps.ctx;
    const size_t MEM = h->rw.MEM, lo = (size_t)c.io_start, W = (size_t)c.io_len;
    std::vector<uint32_t> vf(MEM);
    rc_check(cozk_vec_download(ctx, ps.v_final.h, vf.data()), ctx, "vec_download(v_final)");
    h->v_io_clear.assign(vf.begin() + (long)lo, vf.begin() + (long)(lo + W));
    if (c.tamper == 4) h->v_io_clear[W / 2] += 1;  // the program's claimed output is wrong (a U32 word: 0xFFFFFFFF wraps to 0)
    h->v_io = upload_vec(ctx, h->v_io_clear.data(), W, COZK_SCALAR_U32, "vec_upload(v_io)");
    if (!c.windowed) {
        std::vector<fe> rng(MEM, Fr::zero()), vio(MEM, Fr::zero()), vff(MEM);
        for (size_t x = 0; x < MEM; x++) vff[x] = Fr::from_u64(vf[x]);
        for (size_t j = 0; j < W; j++) rng[lo + j] = Fr::one(), vio[lo + j] = Fr::from_u64(h->v_io_clear[j]);
        h->io_range_fr = upload_vec(ctx, rng.data(), MEM, COZK_SCALAR_FR, "vec_upload(io_range)");
        h->v_io_fr = upload_vec(ctx, vio.data(), MEM, COZK_SCALAR_FR, "vec_upload(v_io)");
        h->v_final_fr = upload_vec(ctx, vff.data(), MEM, COZK_SCALAR_FR, "vec_upload(v_final)");
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// what create checks of h->cfg and builds from it, for this harness and the three-party one (`who` names the harness in the refusals)
void memory_proof_build(cozk_memory_proof* h, const std::string& who) {
    const cozk_memory_proof_config* cfg = &h->cfg;
    cozk_rw_proof_config& rc = h->rw.cfg;
    rc.mode = cfg->mode, rc.device = cfg->device, rc.log_n = cfg->log_n, rc.log_mem = cfg->log_mem, rc.n_slots = cfg->n_slots, rc.seed = cfg->seed;
    rc.precompute = cfg->precompute, rc.with_ts = cfg->with_ts, rc.leaves_fused = cfg->leaves_fused, rc.tamper = cfg->tamper;
    rw_proof_check_config(rc, who, 4);
    COZK_REQUIRE(cfg->io_len >= 1, who + ": io_len is at least 1 word");
    const uint64_t MEM = (uint64_t)1 << cfg->log_mem;
    COZK_REQUIRE(cfg->io_start <= MEM && cfg->io_len <= MEM - cfg->io_start, who + ": io_start + io_len > MEM");
    COZK_REQUIRE(cfg->windowed == 0 || cfg->windowed == 1, who + ": windowed is 0 or 1");
    if (rc.tamper == 4) rc.tamper = 0;  // tamper 4 is the output check's: the witness is honest
    rw_proof_build(&h->rw, who);
    memory_proof_setup(h);
}

// destroy, in two steps: the harness's own vectors while party 0's context stands (the three-party harness releases its parties between
// the two), then the read-write proof's state
void memory_proof_release_vectors(cozk_memory_proof* h) {
    if (!h->rw.parties.empty() && h->rw.parties[0].ctx) (void)hipSetDevice(h->rw.parties[0].ctx->device);
    for (VecH* v : {&h->v_io, &h->io_range_fr, &h->v_io_fr, &h->v_final_fr}) *v = VecH();
}
void memory_proof_release(cozk_memory_proof* h) {
    memory_proof_release_vectors(h);
    rw_proof_release(&h->rw);
}

}  // namespace

extern "C" {

int cozk_memory_proof_create(const cozk_memory_proof_config* cfg, cozk_memory_proof** out) {
    return harness_create(cfg, out, [&](cozk_memory_proof* h) { memory_proof_build(h, "memory_proof"); });
}

const char* cozk_memory_proof_error(const cozk_memory_proof* h) { return harness_error(h); }

int cozk_memory_proof_destroy(cozk_memory_proof* h) {
    if (!h) return COZK_OK;
    memory_proof_release(h);
    delete h;
    return COZK_OK;
}

int cozk_memory_proof_prove(cozk_memory_proof* h, int verify, cozk_memory_proof_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (h->rw.parties.empty() || !h->rw.parties[0].setup || !h->v_io.h) return COZK_ERR_INVALID_ARG;  // create failed
    MemoryProof proof;
    int rc = prove_by_one_party(
        h, h->rw.parties, verify, res, [&](RwProofParty& ps, StarNetWorker* star) { memory_proof_worker_main(h, ps, star); },
        [&](StarNetCoordinator& net) { memory_proof_coordinate(h, net, proof); }, [&](std::string& why) { return memory_proof_verify(h, proof, why); });
    if (rc != COZK_OK) return rc;
    const RwProofParty& ps = h->rw.parties[0];
    res->t_witness_ms = h->rw.t_witness;
    res->t_commit_ms = ps.t_commit;
    res->t_leaves_ms = ps.t_leaves;
    res->t_gp_ms = ps.t_gp;
    res->t_out_ms = h->t_out;
    res->t_ts_ms = ps.t_ts;
    res->t_open_ms = ps.t_open;
    res->out_peak_bytes = h->out_peak_bytes;
    Bytes bytes = proof.serialize();
    res->prefix_len = proof.prefix_len;
    finish_proof(h, std::move(bytes), res);
    return COZK_OK;
}

int cozk_memory_proof_proof_bytes(const cozk_memory_proof* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
