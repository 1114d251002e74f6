// The steps of a memory check that more than one harness runs, each written once: the chained flow (flow_harness.hpp), the timestamp
// range check (ts_range_proof.hpp), the read-write memory proof (rw_memory_proof.hpp) and the whole ReadWriteMemoryProof
// (memory_proof.hpp) call them under their own transcripts, and each keeps the reason string it reports a failure under.  Plain
// functions and small structs, as prover.hpp: a party's env, then the worker's, the coordinator's and the plain verifier's steps.
// tests/memcheck_ref.py holds the same steps for the plain-Python restatements of the four proofs.  Included by harness.hip after its upload helpers, ahead of every harness.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ a party's env
// The env of one in-process party with its device current.  seed given: the two pairwise PRF keys of harness_prf_key (REP3 reads them;
// a plain prover draws no masks).  No seed: the keys stay zero, and a caller with keys of its own sets them afterwards.
WorkerEnv make_worker_env(cozk_ctx* ctx, int mode, int party, StarNetWorker* star, RingNet* ring, const uint64_t* seed = nullptr) {
    WorkerEnv env;
    env.ctx = ctx;
    env.mode = mode;
    env.party = party;
    env.star = star;
    env.ring = ring;
    if (seed) {
        harness_prf_key(*seed, (uint64_t)party, env.key_self);
        harness_prf_key(*seed, (uint64_t)((party + 2) % 3), env.key_prev);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    return env;
}

// ------------------------------------------------------------------------------------------------ proof of one memory check
struct MemCheckProof {
    std::vector<fe> rw_hashes, if_hashes;
    GrandProductProof rw, init_final;
    std::vector<fe> rw_claims, if_claims;
    void write(Writer& w) const {
        w.vec_fr(rw_hashes);
        w.vec_fr(if_hashes);
        rw.write(w);
        init_final.write(w);
        w.vec_fr(rw_claims);
        w.vec_fr(if_claims);
    }
};

inline bool mc_vec_eq(const std::vector<fe>& a, const std::vector<fe>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!Fr::eq(a[i], b[i])) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------ worker
// the commit of columns of any lengths and kinds, sent as the count and the commitments (mc_receive_commitments takes them)
void mc_commit_worker(WorkerEnv& env, const PST13Setup& setup, const std::vector<const cozk_vec*>& cols) {
    std::vector<cozk_vec*> all;
    for (const cozk_vec* v : cols) all.push_back(const_cast<cozk_vec*>(v));
    Writer w;
    w.u64(all.size());
    for (const PST13Commitment& cm : PST13::batch_commit(env.ctx, setup, all)) cm.write(w);
    env.star->send_response(w.b);
}
void mc_receive_gamma_tau(StarNetWorker* star, fe& gamma, fe& tau) {
    Bytes req = star->receive_request();
    Reader rd(req);
    gamma = rd.fr();
    tau = rd.fr();
}
std::vector<fe> mc_receive_point(StarNetWorker* star) {
    Bytes req = star->receive_request();
    Reader rd(req);
    return rd.vec_fr();
}
VecH mc_eq_table(WorkerEnv& env, const std::vector<fe>& point) {
    std::vector<uint64_t> rr = to_abi(point);
    cozk_vec* chi = nullptr;
    rc_check(cozk_eq_evals(env.ctx, rr.data(), (int)point.size(), &chi), env.ctx, "eq_evals");
    return VecH(chi);
}

// one term of a fingerprint: a compact public column or a polynomial (shared, or public as Fr), times coeff.  Where a step takes a
// term as a SOURCE it sets the coefficient itself.
struct LeafTerm {
    const cozk_vec* col = nullptr;
    const cozk_poly* poly = nullptr;
    fe coeff;
};
inline LeafTerm mc_col_term(const cozk_vec* col, const fe& coeff = Fr::zero()) { return LeafTerm{col, nullptr, coeff}; }
inline LeafTerm mc_term(const LeafTerm& src, const fe& coeff) { return LeafTerm{src.col, src.poly, coeff}; }
struct LeafBuf {
    VecH a, b;
};

LeafBuf mc_leaf_alloc(WorkerEnv& env, size_t n) {
    LeafBuf lb;
    cozk_vec* v = nullptr;
    rc_check(cozk_vec_alloc(env.ctx, n, COZK_SCALAR_FR, &v), env.ctx, "vec_alloc(leaves)");
    lb.a = VecH(v);
    if (env.mode == COZK_MODE_REP3) {
        rc_check(cozk_vec_alloc(env.ctx, n, COZK_SCALAR_FR, &v), env.ctx, "vec_alloc(leaves)");
        lb.b = VecH(v);
    }
    return lb;
}
// out[offset .. offset + n) = sum of the terms + constant: one cozk_fingerprint_leaves launch
void mc_fingerprint_leaves(WorkerEnv& env, const std::vector<LeafTerm>& terms, const fe& constant, LeafBuf& out, size_t offset, size_t n) {
    std::vector<const cozk_vec*> cols;
    std::vector<const cozk_poly*> polys;
    std::vector<fe> cc, pc;
    for (auto& t : terms) {
        if (t.col) {
            cols.push_back(t.col);
            cc.push_back(t.coeff);
        } else {
            polys.push_back(t.poly);
            pc.push_back(t.coeff);
        }
    }
    std::vector<uint64_t> ccw = to_abi(cc), pcw = to_abi(pc);
    uint64_t cst[4];
    fe_to_u64x4(constant, cst);
    rc_check(cozk_fingerprint_leaves(env.ctx, cols.data(), ccw.data(), cols.size(), polys.data(), pcw.data(), polys.size(), cst, env.mode, env.party, out.a.h,
                                     out.b.h, offset, n),
             env.ctx, "fingerprint_leaves");
}
LayerH mc_leaves_to_layer(WorkerEnv& env, LeafBuf& lb) {
    cozk_layer* l = nullptr;
    rc_check(cozk_layer_create(env.ctx, env.mode, lb.a.h, lb.b.h, 1, &l), env.ctx, "layer_create");
    return LayerH(l);
}

// prove_memory_checking after compute_leaves (lasso/memory_checking/worker.rs:40-127): construct both circuits, send the hashes,
// prove both, return (r_read_write_opening, r_init_final_opening).  toggle != null: the read / write circuit is toggled.
void mc_memory_checking(WorkerEnv& env, LayerH rw_leaves, size_t rw_batch, ToggleH toggle, LayerH if_leaves, size_t if_batch, std::vector<fe>& r_rw_open,
                        std::vector<fe>& r_if_open) {
    Rep3ToggledBatchedGrandProduct tgp;
    Rep3BatchedDenseGrandProduct rw;
    std::vector<fe> rw_hashes;
    if (toggle.h) {
        rw_batch = cozk_toggle_batch(toggle.h);
        tgp = Rep3ToggledBatchedGrandProduct::construct(env, std::move(toggle));
        rw_hashes = tgp.sparse_layers.claimed_outputs(env);
    } else {
        rw = Rep3BatchedDenseGrandProduct::construct(env, std::move(rw_leaves), rw_batch);
        rw_hashes = rw.claimed_outputs(env);
    }
    Rep3BatchedDenseGrandProduct inf = Rep3BatchedDenseGrandProduct::construct(env, std::move(if_leaves), if_batch);
    std::vector<fe> if_hashes = inf.claimed_outputs(env);
    {
        Writer w;
        w.vec_fr(rw_hashes);
        w.vec_fr(if_hashes);
        env.star->send_response(w.b);
    }
    std::vector<fe> r_rw = tgp.toggle_layer.h ? tgp.prove_grand_product_worker(env) : rw.prove_grand_product_worker(env);
    std::vector<fe> r_if = inf.prove_grand_product_worker(env);
    r_rw_open.assign(r_rw.begin() + ceil_log2(rw_batch), r_rw.end());
    r_if_open.assign(r_if.begin() + ceil_log2(if_batch), r_if.end());
}

// The read-write memory's leaves as cozk_fingerprint_leaves launches (read_write_memory/worker.rs:196-344), slots in the order
// rs1, rs2, rd, ram: per slot read = v_read g + t_read g^2 + a - tau and write = v_write g + step g^2 + a - tau into rw, then
// init = v_init g + address - tau and final = v_final g + t_final g^2 + address - tau into inf.  Every column is a SOURCE.
struct RwSlotLeaves {
    LeafTerm a, v_read, v_write, t_read;
};
void rw_memory_leaves_composed(WorkerEnv& env, const std::vector<RwSlotLeaves>& slots, const LeafTerm& v_init, const LeafTerm& v_final, const LeafTerm& t_final,
                               const LeafTerm& iota_n, const LeafTerm& iota_mem, size_t N, size_t MEM, const fe& gamma, const fe& tau, LeafBuf& rw, LeafBuf& inf) {
    const fe one = Fr::one(), g2 = Fr::mul(gamma, gamma), ntau = Fr::neg(tau);
    for (size_t u = 0; u < slots.size(); u++) {
        const RwSlotLeaves& s = slots[u];
        mc_fingerprint_leaves(env, {mc_term(s.v_read, gamma), mc_term(s.t_read, g2), mc_term(s.a, one)}, ntau, rw, (2 * u) * N, N);
        mc_fingerprint_leaves(env, {mc_term(s.v_write, gamma), mc_term(iota_n, g2), mc_term(s.a, one)}, ntau, rw, (2 * u + 1) * N, N);
    }
    mc_fingerprint_leaves(env, {mc_term(v_init, gamma), mc_term(iota_mem, one)}, ntau, inf, 0, MEM);
    mc_fingerprint_leaves(env, {mc_term(v_final, gamma), mc_term(t_final, g2), mc_term(iota_mem, one)}, ntau, inf, MEM, MEM);
}

// prove_outputs on Fr polynomials (read_write_memory/worker.rs:110-175): sum_x eq(r_eq, x) io_range(x) (v_final(x) - v_io(x)) = 0,
// degree 3, HighToLow.  Returns the sumcheck's point; the caller opens v_final there.
std::vector<fe> prove_outputs_dense_worker(WorkerEnv& env, const cozk_poly* v_final, const VecH& io_range, const VecH& v_io, int log_mem, const std::vector<fe>& r_eq) {
    VecH eqh = mc_eq_table(env, r_eq);
    PolyH pe = plain_poly(env.ctx, eqh), pr = plain_poly(env.ctx, io_range), pio = plain_poly(env.ctx, v_io);
    const cozk_poly* two[2] = {v_final, pio.h};
    const std::vector<uint64_t> cfa = to_abi({Fr::one(), Fr::neg(Fr::one())});
    cozk_poly* pd = nullptr;
    rc_check(cozk_poly_linear_combination(env.ctx, two, cfa.data(), 2, env.mode, env.party, &pd), env.ctx, "v_final - v_io");
    PolyH pdh(pd);
    std::vector<cozk_poly*> sp = {pe.h, pr.h, pdh.h};
    return prove_arbitrary_worker(env, Fr::zero(), log_mem, sp, 3).r;
}

struct OutputCheckH {
    cozk_output_check* h = nullptr;
    OutputCheckH() = default;
    OutputCheckH(const OutputCheckH&) = delete;
    OutputCheckH& operator=(const OutputCheckH&) = delete;
    ~OutputCheckH() { cozk_output_check_free(h); }
};

// ... windowed: the same rounds by cozk_output_check_round / _final on a created handle (cozk_output_check_create on the compact column,
// cozk_output_check_shared_create on a party's polynomial).  The device calls bind inside the next round call, so the loop's bind step
// only keeps r.  any_shared: the handle is a REP3 party's, its round values are additive shares already.
std::vector<fe> prove_outputs_windowed_worker(WorkerEnv& env, cozk_output_check* oc, int log_mem, bool any_shared) {
    uint64_t pending[4];
    bool have = false;
    std::vector<fe> r = prove_arbitrary_rounds(
        env, Fr::zero(), log_mem, 3, any_shared, [&](uint64_t* ev) { rc_check(cozk_output_check_round(oc, have ? pending : nullptr, ev), env.ctx, "output_check_round"); },
        [&](const uint64_t rr[4]) {
            memcpy(pending, rr, sizeof pending);
            have = true;
        });
    uint64_t fin[12];
    rc_check(cozk_output_check_final(oc, pending, fin), env.ctx, "output_check_final");  // the last bind, as prove_arbitrary_worker leaves its polynomials
    return r;
}

// one opening of compact columns of one length at `point`: the claims, one exchange, the joint polynomial over the rho powers
void compact_open_worker(WorkerEnv& env, Rep3ProverOpeningAccumulator& acc, const std::vector<const cozk_vec*>& cols, const std::vector<fe>& point, bool tamper_claim) {
    VecH chih = mc_eq_table(env, point);
    std::vector<uint64_t> ev(4 * cols.size());
    rc_check(cozk_compact_batch_evaluate_at_chi(env.ctx, cols.data(), cols.size(), chih.h, ev.data()), env.ctx, "compact_batch_evaluate");
    std::vector<fe> claims(cols.size());
    for (size_t i = 0; i < cols.size(); i++) claims[i] = fe_from_u64x4(ev.data() + 4 * i);
    if (tamper_claim) claims[0] = Fr::add(claims[0], Fr::one());
    fe batched_claim;
    std::vector<fe> rho_powers = Rep3ProverOpeningAccumulator::exchange_claims(env, claims, batched_claim);
    std::vector<uint64_t> cf = to_abi(rho_powers);
    cozk_vec* jv = nullptr;
    rc_check(cozk_compact_linear_combination(env.ctx, cols.data(), cf.data(), cols.size(), &jv), env.ctx, "compact_linear_combination");
    VecH jvh(jv);
    acc.append_joint(env, plain_poly(env.ctx, jvh), chih.h, point, batched_claim);
}

// ------------------------------------------------------------------------------------------------ coordinator
// the commitments party 0 sent after its commit, into the proof and the transcript
void mc_receive_commitments(StarNetCoordinator& net, Transcript& tr, std::vector<PST13Commitment>& out) {
    Bytes m = net.receive_response(0);
    Reader rd(m);
    const uint64_t k = rd.u64();
    rd.need_elems(k, 72);
    for (uint64_t i = 0; i < k; i++) {
        PST13Commitment cm;
        cm.nv = rd.u64();
        cm.g_product = rd.g1();
        out.push_back(cm);
        tr.append_point(cm.g_product);
    }
}

void mc_broadcast_gamma_tau(StarNetCoordinator& net, Transcript& tr) {
    fe gamma = tr.challenge_scalar(), tau = tr.challenge_scalar();
    Writer w;
    w.fr(gamma);
    w.fr(tau);
    net.broadcast_request(w.b);
}
std::vector<fe> broadcast_challenge_vector(StarNetCoordinator& net, Transcript& tr, size_t n) {
    std::vector<fe> r = tr.challenge_vector(n);
    Writer w;
    w.vec_fr(r);
    net.broadcast_request(w.b);
    return r;
}

void mc_coordinate_memory_checking(StarNetCoordinator& net, Transcript& tr, MemCheckProof& mp, size_t rw_layers, bool toggled, size_t if_layers) {
    std::vector<std::vector<fe>> a, b;
    for (Bytes& m : net.receive_responses()) {
        Reader rd(m);
        a.push_back(rd.vec_fr());
        b.push_back(rd.vec_fr());
    }
    mp.rw_hashes = combine_additive(a);
    mp.if_hashes = combine_additive(b);
    tr.append_scalars(mp.rw_hashes);
    tr.append_scalars(mp.if_hashes);
    fe claim;
    std::vector<fe> r;
    if (toggled) mp.rw = coordinate_prove_toggled_grand_product(net, tr, rw_layers, r);
    else mp.rw = coordinate_prove_grand_product(net, tr, rw_layers, claim, r);
    mp.init_final = coordinate_prove_grand_product(net, tr, if_layers, claim, r);
    mp.rw_claims = Rep3ProverOpeningAccumulator::receive_claims(net, tr);
    mp.if_claims = Rep3ProverOpeningAccumulator::receive_claims(net, tr);
}

// the coordinator's half of the output check: r_eq, the rounds, the claim of v_final
void coordinate_outputs(StarNetCoordinator& net, Transcript& tr, int log_mem, SumcheckProof& outputs, std::vector<fe>& claims) {
    (void)broadcast_challenge_vector(net, tr, (size_t)log_mem);
    (void)coordinate_prove_arbitrary(net, tr, log_mem, outputs.compressed_polys);
    claims = Rep3ProverOpeningAccumulator::receive_claims(net, tr);
}

// the coordinator's ending: ONE reduce_and_prove over every opening the workers accumulated
ReducedOpeningProof mc_coordinate_reduce_and_prove(StarNetCoordinator& net, Transcript& tr) {
    std::vector<fe> r_red;
    fe rho, gamma;
    return Rep3ProverOpeningAccumulator::reduce_and_prove(net, tr, r_red, rho, gamma);
}

// ------------------------------------------------------------------------------------------------ plain verifier
fe mc_mle_host(const std::vector<fe>& vals, const std::vector<fe>& r) {
    std::vector<fe> eq = eq_evals_host(r);
    fe acc = Fr::zero();
    for (size_t i = 0; i < vals.size(); i++) acc = Fr::add(acc, Fr::mul(eq[i], vals[i]));
    return acc;
}
// the identity column 0, 1, 2, .. at a big-endian point
fe mc_iota_eval(const std::vector<fe>& r) {
    fe acc = Fr::zero();
    for (size_t j = 0; j < r.size(); j++) acc = Fr::add(Fr::dbl(acc), r[j]);
    return acc;
}
// MLE of circuit-major leaves at r = (r_hi over the circuits, padded to a power of two with `pad`) x r_lo
fe mc_batch_eval(const std::vector<fe>& per_circuit, const std::vector<fe>& r_hi, const fe& pad) {
    std::vector<fe> eq = eq_evals_host(r_hi);
    fe acc = Fr::zero();
    for (size_t cidx = 0; cidx < eq.size(); cidx++) acc = Fr::add(acc, Fr::mul(eq[cidx], cidx < per_circuit.size() ? per_circuit[cidx] : pad));
    return acc;
}

// the openings a verifier collects for verify_reduced_opening.  take: one claim exchange (receive_claims), whose batching challenge is
// drawn right after it (rho given: already drawn); false if there is not one claim per polynomial.
struct VerifierOpenings {
    Transcript& vt;
    std::vector<VerifierOpening> list;
    explicit VerifierOpenings(Transcript& t) : vt(t) {}
    template <class I>
    bool take(const std::vector<I>& polys, const std::vector<fe>& point, const std::vector<fe>& claims, const fe* rho = nullptr) {
        list.push_back(VerifierOpening{point, std::vector<size_t>(polys.begin(), polys.end()), claims, rho ? *rho : vt.challenge_scalar()});
        return polys.size() == claims.size();
    }
};

// the verifier's ending: the reduced opening over everything `opens` took, its refusals under "opening: "
bool mc_verify_opening(const VerifierOpenings& opens, const std::vector<PST13Commitment>& commitments, const ReducedOpeningProof& reduced, const PST13Setup& setup,
                       std::string& why) {
    std::string inner;
    if (verify_reduced_opening(opens.list, commitments, opens.vt, reduced, setup, "reduction sumcheck: shape", "reduction sumcheck: final check", inner)) return true;
    why = "opening: " + inner;
    return false;
}

// One grand product: its outputs are the `batch` hashes, every round and layer reduction holds, and the final point has
// ceil_log2(batch) circuit variables (hi) over `layers` leaf variables (lo; a toggled product's last layer adds none).
bool mc_verify_grand_product(const GrandProductProof& gp, const std::vector<fe>& hashes, bool toggled, size_t batch, size_t layers, Transcript& vt, fe& claim, fe& flag_claim,
                             std::vector<fe>& hi, std::vector<fe>& lo) {
    if (!mc_vec_eq(gp.outputs, hashes) || hashes.size() != batch) return false;
    std::vector<fe> r;
    if (!(toggled ? verify_toggled_grand_product(gp, vt, flag_claim, claim, r) : verify_grand_product(gp, vt, claim, r))) return false;
    const size_t k = (size_t)ceil_log2(batch);
    if (r.size() != k + layers - (toggled ? 1 : 0)) return false;
    hi.assign(r.begin(), r.begin() + (long)k);
    lo.assign(r.begin() + (long)k, r.end());
    return true;
}

// what the grand products of one memory check leave: the final claims and the split points of read / write (hi, lo) and init / final
struct MemCheckPoints {
    fe rw_claim, flag_claim, if_claim;
    std::vector<fe> hi, lo, hi2, lo2;
};
// Both grand products of one memory check, the read / write one toggled or dense: the hashes go into the transcript first.  The layer
// counts are the coordinator's (mc_coordinate_memory_checking).
bool mc_verify_grand_products(const MemCheckProof& mp, bool toggled, size_t rw_batch, size_t if_batch, size_t rw_layers, size_t if_layers, Transcript& vt, MemCheckPoints& out) {
    vt.append_scalars(mp.rw_hashes);
    vt.append_scalars(mp.if_hashes);
    fe unused;
    return mc_verify_grand_product(mp.rw, mp.rw_hashes, toggled, rw_batch, rw_layers, vt, out.rw_claim, out.flag_claim, out.hi, out.lo) &&
           mc_verify_grand_product(mp.init_final, mp.if_hashes, false, if_batch, if_layers, vt, out.if_claim, unused, out.hi2, out.lo2);
}

// the fingerprint a + gamma v + gamma^2 t - tau
inline fe mc_fingerprint(const fe& a, const fe& v, const fe& t, const fe& gamma, const fe& g2, const fe& tau) {
    return Fr::sub(Fr::add(Fr::add(a, Fr::mul(v, gamma)), Fr::mul(t, g2)), tau);
}

// The read-write memory's leaf claims rebuilt from the opened values: per slot the read and the write fingerprint (the write's
// timestamp is the step, the identity at lo), then init (the verifier's own v_init(lo2), timestamp 0) and final = if_claims
// {v_final, t_final}, each batch evaluated at its hi point.  The caller compares them with the grand products' claims.
struct RwSlotClaims {
    size_t a, v_read, v_write, t_read;  // positions in rw_claims
};
void rw_memory_verify_leaves(const std::vector<fe>& rw_claims, const std::vector<fe>& if_claims, const std::vector<RwSlotClaims>& slots, const fe& v_init_at_lo2,
                             const fe& gamma, const fe& tau, const MemCheckPoints& pts, fe& rw_claim, fe& if_claim) {
    const fe g2 = Fr::mul(gamma, gamma), step = mc_iota_eval(pts.lo), io = mc_iota_eval(pts.lo2);
    std::vector<fe> leaves;
    for (const RwSlotClaims& s : slots) {
        leaves.push_back(mc_fingerprint(rw_claims[s.a], rw_claims[s.v_read], rw_claims[s.t_read], gamma, g2, tau));
        leaves.push_back(mc_fingerprint(rw_claims[s.a], rw_claims[s.v_write], step, gamma, g2, tau));
    }
    rw_claim = mc_batch_eval(leaves, pts.hi, Fr::zero());
    const fe init = mc_fingerprint(io, v_init_at_lo2, Fr::zero(), gamma, g2, tau);
    const fe fin = mc_fingerprint(io, if_claims[0], if_claims[1], gamma, g2, tau);
    if_claim = mc_batch_eval({init, fin}, pts.hi2, Fr::zero());
}

// The output check's rounds and shape: draws r_eq, replays log_mem rounds of degree 3 from claim 0, wants one claim (v_final(r_out)).  Then
// the final identity eq(r_eq, r_out) io_range(r_out) (v_final(r_out) - v_io(r_out)) == claim, the public polynomials evaluated by the caller.
bool verify_outputs(Transcript& vt, int log_mem, const SumcheckProof& outputs, const std::vector<fe>& claims, std::vector<fe>& r_eq, std::vector<fe>& r_out, fe& claim) {
    r_eq = vt.challenge_vector((size_t)log_mem);
    claim = Fr::zero();
    return verify_sumcheck_rounds(outputs.compressed_polys, (size_t)log_mem, 3, claim, vt, r_out) && claims.size() == 1;
}
inline bool outputs_final_holds(const std::vector<fe>& r_eq, const std::vector<fe>& r_out, const fe& range_r, const fe& v_io_r, const fe& v_final_claim, const fe& claim) {
    return Fr::eq(Fr::mul(Fr::mul(eq_eval(r_eq, r_out), range_r), Fr::sub(v_final_claim, v_io_r)), claim);
}

}  // namespace
