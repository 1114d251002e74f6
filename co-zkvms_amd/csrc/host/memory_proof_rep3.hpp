// In-process harness of the memory check and the output check of ReadWriteMemoryProof by three Rep3 parties, in the reference's order
// (Rep3ReadWriteMemoryProver::prove, co-jolt/src/jolt/vm/read_write_memory/worker.rs:54-180, without the timestamp range check):
// cozk_rw_proof_rep3's steps (rw_memory_proof_rep3.hpp), then prove_outputs (:110-175) on each party's share of v_final, under one
// transcript and one opening accumulator, with ONE reduce_and_prove.  The handle holds cozk_memory_proof's own state for party 0 with
// with_ts = 0 (`mp`): the instance, v_io, tamper 4, the MemoryProof bytes and memory_proof_verify are that harness's code, the sharing, the
// memory-check step and the finish are cozk_rw_proof_rep3's, so no step exists twice and the proof is byte for byte cozk_memory_proof's
// PLAIN proof of the same seed and window.  windowed = 1: the rounds are cozk_output_check_shared_create / _round / _final on the party's
// polynomial (output_check.inc); windowed = 0: prove_outputs_dense_worker in REP3 on Fr vectors of MEM entries -- eq, io_range, v_io and the
// two-component difference, bound every round -- kept for the A/B, the same bytes.  The worker follows the plain proof's order (the
// coordinator reads the memory check's claims before it draws r_eq): the memory check with its two openings, r_eq, log_mem rounds, the
// opening of the shared v_final at the sumcheck's point (rw3_open_worker), ONE reduce_and_prove.  Not here: the timestamp range
// check by Rep3 parties, one party per process.
#pragma once

// what a party holds for the output check beside its RwRep3Party
struct MemRep3Out {
    VecH v_io_own;                    // parties 1 and 2: the public io words on their device (party 0 reads mp's)
    const cozk_vec* v_io = nullptr;   // U32, io_len words
    VecH io_range_fr, v_io_fr;        // windowed = 0: the public Fr vectors of MEM entries
    double t_out = 0;
    uint64_t out_peak_bytes = 0;
};

struct cozk_memory_proof_rep3 : HarnessHandle {
    cozk_memory_proof_rep3_config cfg;
    cozk_memory_proof mp;           // party 0's plain harness with with_ts = 0: the instance, v_io, and what the verifier reads
    cozk_rw_proof_rep3_config rc;   // the fields the memory-check steps read
    bool built = false;
    std::vector<RwRep3Party> parties;
    std::vector<MemRep3Out> outs;
};

namespace {

void mp3_setup(cozk_memory_proof_rep3* h) {
    const cozk_memory_proof_rep3_config& c = h->cfg;
    const size_t MEM = h->mp.rw.MEM, lo = (size_t)c.io_start, W = (size_t)c.io_len;
    h->outs.resize(3);
    std::vector<fe> rng, vio;
    if (!c.windowed) {
        rng.assign(MEM, Fr::zero()), vio.assign(MEM, Fr::zero());
        for (size_t j = 0; j < W; j++) rng[lo + j] = Fr::one(), vio[lo + j] = Fr::from_u64(h->mp.v_io_clear[j]);
    }
    for (int p = 0; p < 3; p++) {
        RwRep3Party& ps = h->parties[(size_t)p];
        MemRep3Out& o = h->outs[(size_t)p];
        HIP_TRY(hipSetDevice(ps.ctx->device));
        if (p == 0) {
            o.v_io = h->mp.v_io.h;
        } else {
            o.v_io_own = upload_vec(ps.ctx, h->mp.v_io_clear.data(), W, COZK_SCALAR_U32, "vec_upload(v_io)");
            o.v_io = o.v_io_own.h;
        }
        if (!c.windowed) {
            o.io_range_fr = upload_vec(ps.ctx, rng.data(), MEM, COZK_SCALAR_FR, "vec_upload(io_range)");
            o.v_io_fr = upload_vec(ps.ctx, vio.data(), MEM, COZK_SCALAR_FR, "vec_upload(v_io)");
        }
        HIP_TRY(hipStreamSynchronize(ps.ctx->stream));
    }
}

void mp3_worker_main(cozk_memory_proof_rep3* h, RwRep3Party& ps, MemRep3Out& o, StarNetWorker* star, RingNet* ring) {
    const cozk_memory_proof_rep3_config& c = h->cfg;
    WorkerEnv env = make_worker_env(ps.ctx, COZK_MODE_REP3, ps.party, star, ring, &c.seed);
    Rep3ProverOpeningAccumulator acc;
    // ---- 1-4. the memory check: cozk_rw_proof_rep3's steps
    const double t4 = rw3_memory_check_worker(h->mp.rw, h->rc, ps, env, acc);
    const double t5 = now_ms();
    // ---- the output check: r_eq, log_mem rounds, one opening of the shared v_final at the sumcheck's point
    {
        const std::vector<fe> r_eq = mc_receive_point(star);
        const double t0 = now_ms();
        std::vector<fe> r;
        {
            PhasePeak peak(env.ctx);
            if (c.windowed) {
                const std::vector<uint64_t> wabi = to_abi(r_eq);
                OutputCheckH oc;
                rc_check(cozk_output_check_shared_create(env.ctx, ps.v_final.h, o.v_io, (size_t)c.io_start, wabi.data(), ps.party, &oc.h), env.ctx,
                         "output_check_shared_create");
                r = prove_outputs_windowed_worker(env, oc.h, c.log_mem, true);
            } else {
                r = prove_outputs_dense_worker(env, ps.v_final.h, o.io_range_fr, o.v_io_fr, c.log_mem, r_eq);
            }
            o.out_peak_bytes = peak.bytes();
        }
        rw3_open_worker(env, acc, {LeafTerm{nullptr, ps.v_final.h, Fr::zero()}}, r, false);
        o.t_out = now_ms() - t0;
    }
    // ---- ONE reduce_and_prove: cozk_rw_proof_rep3's step
    rw3_open_and_finish_worker(ps, env, acc, t5 - t4);
}

void mp3_coordinate(cozk_memory_proof_rep3* h, StarNetCoordinator& net, MemoryProof& proof) {
    const cozk_rw_proof_config& c = h->mp.rw.cfg;
    Transcript tr("cozk-rw-memory");
    rw3_coordinate_commitments(net, tr, proof.commitments);
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.mem, (size_t)c.log_n, false, (size_t)c.log_mem);
    coordinate_outputs(net, tr, c.log_mem, proof.outputs, proof.outputs_claims);
    rw_proof_coordinate_range_check_and_open(c, net, tr, proof.with_ts, proof.range, proof.reduced);
}

void mp3_release(cozk_memory_proof_rep3* h) {
    for (size_t p = 0; p < h->outs.size() && p < h->parties.size(); p++) {
        if (h->parties[p].ctx) (void)hipSetDevice(h->parties[p].ctx->device);
        h->outs[p] = MemRep3Out();
    }
    h->outs.clear();
    // memory_proof_release's two steps with the parties' release between them: rw3_release frees the parties' handles and the contexts of
    // parties 1 and 2 and ends with rw_proof_release
    memory_proof_release_vectors(&h->mp);
    rw3_release(h->mp.rw, h->parties);
}

}  // namespace

extern "C" {

int cozk_memory_proof_rep3_create(const cozk_memory_proof_rep3_config* cfg, cozk_memory_proof_rep3** out) {
    return harness_create(cfg, out, [&](cozk_memory_proof_rep3* h) {
        cozk_memory_proof_config& mc = h->mp.cfg;
        mc = cozk_memory_proof_config{};
        mc.mode = COZK_MODE_PLAIN, mc.device = cfg->devices[0], mc.log_n = cfg->log_n, mc.log_mem = cfg->log_mem, mc.n_slots = cfg->n_slots, mc.seed = cfg->seed;
        mc.precompute = cfg->precompute, mc.with_ts = 0, mc.leaves_fused = cfg->leaves_fused, mc.tamper = cfg->tamper;
        mc.io_start = cfg->io_start, mc.io_len = cfg->io_len;
        COZK_REQUIRE(cfg->windowed == 0 || cfg->windowed == 1, "memory_proof_rep3: windowed is 0 or 1");
        mc.windowed = 1;  // party 0's harness keeps no Fr copies: with windowed = 0 every party gets its public vectors in mp3_setup
        cozk_rw_proof_rep3_config& rc = h->rc;
        rc = cozk_rw_proof_rep3_config{};
        for (int p = 0; p < 3; p++) rc.devices[p] = cfg->devices[p];
        rc.log_n = cfg->log_n, rc.log_mem = cfg->log_mem, rc.n_slots = cfg->n_slots, rc.seed = cfg->seed;
        rc.precompute = cfg->precompute, rc.leaves_fused = cfg->leaves_fused, rc.tamper = cfg->tamper;
        memory_proof_build(&h->mp, "memory_proof_rep3");  // the instance on party 0's context, tampers 1 and 4 included; with_ts = 0 refuses tamper 3
        rw3_setup(h->mp.rw, rc, h->parties);
        mp3_setup(h);
        h->built = true;
    });
}

const char* cozk_memory_proof_rep3_error(const cozk_memory_proof_rep3* h) { return harness_error(h); }

int cozk_memory_proof_rep3_destroy(cozk_memory_proof_rep3* h) {
    if (!h) return COZK_OK;
    mp3_release(h);
    delete h;
    return COZK_OK;
}

int cozk_memory_proof_rep3_prove(cozk_memory_proof_rep3* h, int verify, cozk_memory_proof_rep3_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    if (!h->built) return COZK_ERR_INVALID_ARG;  // create failed
    InProcNets nets(3, true);
    std::vector<Participant> parts;
    add_participants(parts, "party", h->parties, [&](RwRep3Party& ps, int p) { mp3_worker_main(h, ps, h->outs[(size_t)p], nets.worker(p), nets.ring(p)); });
    MemoryProof proof;
    double wall_ms = 0;
    int rc = run_in_process(nets, parts, [&] {
        InProcStarCoordinator coord(&nets.star);
        mp3_coordinate(h, coord, proof);
    }, h->error, wall_ms);
    if (rc != COZK_OK) return rc;
    res->wall_ms = wall_ms;  // the verifier below is outside the clock
    if (verify) harness_verify(h, res, h->parties[0].ctx->device, [&](std::string& why) { return memory_proof_verify(&h->mp, proof, why); });
    res->t_witness_ms = h->mp.rw.t_witness;
    for (size_t p = 0; p < h->parties.size(); p++) {
        const RwRep3Party& ps = h->parties[p];
        res->t_share_ms = std::max(res->t_share_ms, ps.t_share);
        res->t_commit_ms = std::max(res->t_commit_ms, ps.t_commit);
        res->t_leaves_ms = std::max(res->t_leaves_ms, ps.t_leaves);
        res->t_gp_ms = std::max(res->t_gp_ms, ps.t_gp);
        res->t_out_ms = std::max(res->t_out_ms, h->outs[p].t_out);
        res->t_open_ms = std::max(res->t_open_ms, ps.t_open);
        res->out_peak_bytes = std::max(res->out_peak_bytes, h->outs[p].out_peak_bytes);
        res->ring_bytes += ps.ring_bytes;
    }
    Bytes bytes = proof.serialize();
    res->prefix_len = proof.prefix_len;
    finish_proof(h, std::move(bytes), res);
    return COZK_OK;
}

int cozk_memory_proof_rep3_proof_bytes(const cozk_memory_proof_rep3* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
