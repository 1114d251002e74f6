// ONE chained co-jolt worker flow: JoltRep3Prover::prove (co-jolt/src/jolt/vm/jolt/worker.rs:175-266) against its
// coordinator (jolt/vm/jolt/coordinator.rs:118-222) under ONE transcript and ONE Rep3ProverOpeningAccumulator, every polynomial
// committed once:
//
//   1 commit-all                                  Rep3JoltPolynomials::commit, jolt/vm/jolt/witness.rs:304-382 (PST13 batch commit)
//   2 bytecode memory checking                    lasso/memory_checking/worker.rs:40-237 + jolt/vm/bytecode/worker.rs:43-142
//   3 instruction lookups                         jolt/vm/instruction_lookups/worker.rs:95-176: primary sumcheck, then memory checking with
//                                                 the TOGGLED read / write grand product and the dense init / final one (:742-860)
//   4 read-write memory checking + output check   jolt/vm/read_write_memory/worker.rs:54-180 (prove_outputs), :196-344 (leaves)
//   5 Spartan                                     r1cs/spartan/worker.rs:63-273 on the reference's constraint set (spartan_jolt.hpp)
//   6 reduce_and_prove over ALL openings          poly/opening_proof.rs:181-291 -> one PST13 opening
//
// Every grand product's leaves are K11 fingerprints of COMMITTED columns (cozk_fingerprint_leaves) with the reference's formulas.
// The witness is synthetic but Jolt-shaped: the 78 R1CS inputs of a satisfying synthetic trace (jolt_r1cs.hpp) double as
// the bytecode / register / RAM / lookup columns exactly as inputs.rs:269-300 maps them; read_cts / E / final_cts per memory, the
// timestamps, v_init / v_final are seeded streams.  NOT part of the flow (out of this path's scope): party 0's public
// TimestampValidityProof (jolt-core, read_write_memory/worker.rs:78-104) and the verifier's multiset-equality check of the hashes (the
// synthetic counters are not a consistent offline-memory-checking instance; every sumcheck, GKR layer, fingerprint-vs-opening relation and
// the batched PST13 opening ARE verified).  cfg.lookups_witness = 1 replaces the instruction lookups' seeded read_cts / E / final_cts by a
// consistent instance counted on the device (cozk_lasso_witness over the committed query chunks, the memory flags and the subtables),
// and the verifier then DOES run the multiset-equality check of the lookups' hashes; the bytecode and the read-write memory keep
// synthetic counters either way.  The Lasso lookup_outputs polynomial is generated from the E polynomials (sum_i flag_i g_i(E)),
// independently of the R1CS LookupOutput column (a real trace identifies the two).  oracle/pyflow.py restates the flow; proofs are compared
// byte for byte.
#pragma once
#include <functional>

struct FlowIdx {
    int n_mem = 0;
    int r1cs = 0, bc_t_read = 0, rw_t_read = 0, read_cts = 0, E = 0, lasso_out = 0, final_cts = 0, bc_t_final = 0, rw_v_init = 0, rw_v_final = 0, rw_t_final = 0,
        count = 0;
    explicit FlowIdx(int nm = 0) : n_mem(nm) {
        r1cs = 0;
        bc_t_read = jolt::NUM_INPUTS;
        rw_t_read = bc_t_read + 1;
        read_cts = rw_t_read + 4;
        E = read_cts + nm;
        lasso_out = E + nm;
        final_cts = lasso_out + 1;
        bc_t_final = final_cts + nm;
        rw_v_init = bc_t_final + 1;
        rw_v_final = rw_v_init + 1;
        rw_t_final = rw_v_final + 1;
        count = rw_t_final + 1;
    }
};

struct FlowParty : HarnessParty {
    std::vector<PolyH> polys;       // evaluation view (REP3 shares, or PLAIN Fr values for public polynomials), commit order
    std::vector<VecH> commit_vecs;  // what the MSM and the fingerprints consume: share-a view, or the compact public column
    std::vector<VecH> msm_vecs;     // PLAIN mode: a narrow (U32 / U64) copy of a secret column whose values fit, for the MSM only
                                    // (msm_field_elements' dispatch on the scalars' bit length); empty handle = commit_vecs[i]
    std::unique_ptr<PST13Setup> setup;
    VecH iota;                         // 0, 1, 2, .. as U32 (identity / index columns of the leaves)
    std::vector<VecH> bc_table;        // the bytecode table (preprocessing.v_init_final): 6 compact columns of B entries
    std::vector<VecH> subtables;       // materialized subtables: U32 columns of M entries
    std::vector<VecH> mem_flags;       // memory_flag_indices as dense U8 columns
    VecH io_range, v_io;               // FR vectors of MEM entries (output check)
    double t_commit = 0, t_bytecode = 0, t_primary = 0, t_lookups_gp = 0, t_rw = 0, t_spartan = 0, t_open = 0, t_total = 0;
    SpartanTimes sp_times;
};

struct cozk_flow : HarnessHandle {
    cozk_flow_config cfg;
    int nparties = 1;
    size_t N = 0, M = 0, B = 0, MEM = 0;
    FlowIdx ix;
    std::vector<FlowParty> parties;
    jolt::System sys;
    std::vector<cozk_primary_instr> instrs;
    // the dealer's / verifier's clear view
    std::vector<std::vector<fe>> clear;  // per committed polynomial
    std::vector<int> is_public, pub_bytes;
    std::vector<uint64_t> device_stream;  // != 0: the column is the seeded stream of this seed, generated on the device (no host copy)
    std::vector<int> device_bits;         // ... masked to this many bits (cfg.small_witness), 0 = full width
    std::vector<size_t> lens;
    std::vector<std::vector<uint64_t>> bc_table_clear, subtables_clear;
    std::vector<fe> io_range_clear, v_io_clear;
};

namespace {

struct FlowProof {
    std::vector<PST13Commitment> commitments;
    MemCheckProof bytecode, lookups, rw;
    PrimarySumcheckProof primary;
    std::vector<fe> primary_claims;
    SumcheckProof outputs;
    std::vector<fe> outputs_claims;
    JoltSpartanProof spartan;
    ReducedOpeningProof reduced;
    Bytes serialize() const {
        Writer w;
        w.u64(commitments.size());
        for (auto& c : commitments) c.write(w);
        bytecode.write(w);
        primary.write(w);
        w.vec_fr(primary_claims);
        lookups.write(w);
        rw.write(w);
        outputs.write(w);
        w.vec_fr(outputs_claims);
        spartan.write(w);
        reduced.write(w);
        return w.b;
    }
};

// ------------------------------------------------------------------------------------------------ the dealer's view
// host threads over index ranges (the setup of a 2^20-cycle trace generates ~10^8 field elements)
void flow_par_for(size_t n, const std::function<void(size_t, size_t)>& body) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
    if (n < 4096 || nt == 1) {
        body(0, n);
        return;
    }
    std::vector<std::thread> ts;
    for (unsigned k = 0; k < nt; k++) ts.emplace_back([&, k] { body(n * k / nt, n * (k + 1) / nt); });
    for (auto& t : ts) t.join();
}

template <typename T>
VecH flow_upload_ints(cozk_ctx* ctx, const std::vector<uint64_t>& v, int kind) {
    std::vector<T> t(v.size());
    for (size_t i = 0; i < v.size(); i++) t[i] = (T)v[i];
    return upload_vec(ctx, t.data(), t.size(), kind, "vec_upload(compact column)");
}
VecH flow_upload_compact(cozk_ctx* ctx, const std::vector<uint64_t>& v, int bytes) {
    if (bytes == 1) return flow_upload_ints<uint8_t>(ctx, v, COZK_SCALAR_U8);
    if (bytes == 4) return flow_upload_ints<uint32_t>(ctx, v, COZK_SCALAR_U32);
    return flow_upload_ints<uint64_t>(ctx, v, COZK_SCALAR_U64);
}

// memory_flag_indices as a dense 0/1 column: memory m is live at step t iff the step's instruction uses it
std::vector<uint64_t> flow_mem_flag_column(const cozk_flow* h, int m) {
    std::vector<uint64_t> col(h->N, 0);
    for (int i = 0; i < jolt::N_INSTR; i++) {
        const cozk_primary_instr& in = h->instrs[(size_t)i];
        bool uses = false;
        for (int j = 0; j < in.n_mems; j++) uses |= in.mems[j] == m;
        if (!uses) continue;
        const std::vector<fe>& fl = h->clear[(size_t)(jolt::V_INSTR + i)];
        for (size_t t2 = 0; t2 < h->N; t2++)
            if (!Fr::is_zero(fl[t2])) col[t2] = 1;
    }
    return col;
}

// cfg.lookups_witness: read_cts / E / final_cts of every memory as a consistent offline-memory-checking instance
// (instruction_lookups/witness.rs:85-150), counted on party 0's device from the committed query chunks (memory m reads chunk m % 4,
// as its leaves do), the memory flags and the subtables; the results come back as clear columns that are shared like any other
void flow_lasso_witness(cozk_flow* h) {
    const cozk_flow_config& c = h->cfg;
    const FlowIdx& ix = h->ix;
    cozk_ctx* ctx = h->parties[0].ctx;
    const size_t N = h->N, M = h->M;
    std::vector<VecH> dims, subs, flags;
    for (int i = 0; i < 4; i++) {
        const std::vector<fe>& col = h->clear[(size_t)(jolt::V_QUERY + i)];
        std::vector<uint64_t> ints(N);
        for (size_t t = 0; t < N; t++) ints[t] = Fr::from_mont(col[t]).l[0];
        dims.push_back(flow_upload_compact(ctx, ints, 4));
    }
    for (auto& s : h->subtables_clear) subs.push_back(flow_upload_compact(ctx, s, 4));
    for (int m = 0; m < c.n_mem; m++) flags.push_back(flow_upload_compact(ctx, flow_mem_flag_column(h, m), 1));
    std::vector<const cozk_vec*> dv, sv, fv;
    for (auto& v : dims) dv.push_back(v.h);
    for (auto& v : subs) sv.push_back(v.h);
    for (auto& v : flags) fv.push_back(v.h);
    std::vector<int> mem_dim((size_t)c.n_mem), mem_sub((size_t)c.n_mem);
    for (int m = 0; m < c.n_mem; m++) {
        mem_dim[(size_t)m] = m % 4;
        mem_sub[(size_t)m] = m % c.n_subtables;
    }
    std::vector<cozk_vec*> rc((size_t)c.n_mem), E((size_t)c.n_mem), fc((size_t)c.n_mem);
    rc_check(cozk_lasso_witness(ctx, dv.data(), dv.size(), sv.data(), sv.size(), fv.data(), mem_dim.data(), mem_sub.data(), (size_t)c.n_mem, rc.data(), E.data(), fc.data()),
             ctx, "lasso_witness");
    std::vector<VecH> own;
    for (auto* list : {&rc, &E, &fc})
        for (cozk_vec* v : *list) own.push_back(VecH(v));
    auto take = [&](cozk_vec* v, int idx, size_t n) {
        std::vector<uint32_t> w(n);
        rc_check(cozk_vec_download(ctx, v, w.data()), ctx, "vec_download(lookup witness)");
        std::vector<fe>& col = h->clear[(size_t)idx];
        col.resize(n);
        flow_par_for(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) col[i] = Fr::from_u64(w[i]);
        });
    };
    for (int m = 0; m < c.n_mem; m++) {
        take(rc[(size_t)m], ix.read_cts + m, N);
        take(E[(size_t)m], ix.E + m, N);
        take(fc[(size_t)m], ix.final_cts + m, M);
    }
    if (c.lookups_tamper > 0) {  // tests: an inconsistent final counter that every other relation of the proof still accepts
        fe& v = h->clear[(size_t)ix.final_cts][(size_t)(c.lookups_tamper - 1)];
        v = Fr::add(v, Fr::one());
    }
}

void flow_build_clear(cozk_flow* h) {
    const cozk_flow_config& c = h->cfg;
    const uint64_t seed = c.seed;
    const FlowIdx& ix = h->ix;
    const size_t N = h->N, M = h->M, B = h->B, MEM = h->MEM;
    h->clear.assign((size_t)ix.count, {});
    h->is_public.assign((size_t)ix.count, 0);
    h->pub_bytes.assign((size_t)ix.count, 0);
    h->device_stream.assign((size_t)ix.count, 0);
    h->lens.assign((size_t)ix.count, 0);
    std::vector<std::vector<fe>> r1;
    jolt::build_clear(seed, N, r1);
    for (int v = 0; v < jolt::NUM_INPUTS; v++) {
        h->clear[(size_t)v] = std::move(r1[(size_t)v]);
        h->pub_bytes[(size_t)v] = jolt::public_bytes(v);
        h->is_public[(size_t)v] = h->pub_bytes[(size_t)v] ? 1 : 0;
    }
    auto pub = [&](int idx, uint64_t off, size_t n, int bits) {
        std::vector<fe>& col = h->clear[(size_t)idx];
        col.resize(n);
        for (size_t i = 0; i < n; i++) col[i] = Fr::from_u64(synthetic_small_host(seed + off, i, bits));
        h->is_public[(size_t)idx] = 1;
        h->pub_bytes[(size_t)idx] = 4;
    };
    auto par_for = flow_par_for;
    // cfg.small_witness: the widths a real trace gives these columns (0 = uniform field elements, see include/cozk.h)
    const int cnt_bits = c.small_witness ? c.log_n : 0, val_bits = c.small_witness ? 32 : 0;
    h->device_bits.assign((size_t)ix.count, 0);
    auto sh = [&](int idx, uint64_t s, size_t n, int bits) {
        std::vector<fe>& col = h->clear[(size_t)idx];
        col.resize(n);
        par_for(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) col[i] = synthetic_fr_host(s, i, bits);
        });
    };
    auto dev = [&](int idx, uint64_t s, size_t n, int bits) {
        h->device_stream[(size_t)idx] = s;
        h->device_bits[(size_t)idx] = bits;
        h->lens[(size_t)idx] = n;
    };
    pub(ix.bc_t_read, 31, N, 20);
    pub(ix.bc_t_final, 32, B, 20);
    for (int k = 0; k < 4; k++) pub(ix.rw_t_read + k, 41 + (uint64_t)k, N, 20);
    sh(ix.rw_v_init, seed + 45000, MEM, val_bits);
    sh(ix.rw_v_final, seed + 46000, MEM, val_bits);
    pub(ix.rw_t_final, 47, MEM, 20);
    for (int m = 0; m < c.n_mem && !c.lookups_witness; m++) {
        dev(ix.read_cts + m, seed + 11000ull * (uint64_t)(m + 1), N, cnt_bits);
        sh(ix.E + m, seed + 9000ull * (uint64_t)(m + 1), N, val_bits);
        dev(ix.final_cts + m, seed + 13000ull * (uint64_t)(m + 1), M, cnt_bits);
    }
    static const int tab_bits[6] = {20, 32, 6, 6, 6, 12};
    h->bc_table_clear.assign(6, std::vector<uint64_t>(B));
    for (int k = 0; k < 6; k++)
        for (size_t i = 0; i < B; i++) h->bc_table_clear[(size_t)k][i] = synthetic_small_host(seed + 33 + (uint64_t)k, i, tab_bits[k]);
    h->subtables_clear.assign((size_t)c.n_subtables, std::vector<uint64_t>(M));
    for (int s = 0; s < c.n_subtables; s++)
        for (size_t i = 0; i < M; i++) h->subtables_clear[(size_t)s][i] = synthetic_small_host(seed + 15000ull * (uint64_t)(s + 1), i, 32);
    // lookup_outputs = sum_i flag_i g_i(E) in the clear
    h->instrs = lookups_instr_table(c.n_mem);
    if (c.lookups_witness) flow_lasso_witness(h);
    std::vector<fe>& outs = h->clear[(size_t)ix.lasso_out];
    outs.assign(N, Fr::zero());
    par_for(N, [&](size_t lo, size_t hi) {
        std::vector<fe> E((size_t)c.n_mem);
        for (size_t t = lo; t < hi; t++) {
            for (int i = 0; i < jolt::N_INSTR; i++) {
                if (Fr::is_zero(h->clear[(size_t)(jolt::V_INSTR + i)][t])) continue;
                const cozk_primary_instr& in = h->instrs[(size_t)i];
                for (int j = 0; j < in.n_mems; j++) E[(size_t)in.mems[j]] = h->clear[(size_t)(ix.E + in.mems[j])][t];
                outs[t] = primary_g_plain(in, E);
                break;
            }
        }
    });
    h->io_range_clear.assign(MEM, Fr::zero());
    h->v_io_clear.assign(MEM, Fr::zero());
    for (size_t i = MEM / 4; i < MEM / 2; i++) {
        h->io_range_clear[i] = Fr::one();
        h->v_io_clear[i] = h->clear[(size_t)ix.rw_v_final][i];
    }
    for (int i = 0; i < ix.count; i++)
        if (!h->device_stream[(size_t)i]) h->lens[(size_t)i] = h->clear[(size_t)i].size();
}

uint64_t flow_share_seed(const cozk_flow* h, int idx) {
    const FlowIdx& ix = h->ix;
    const uint64_t seed = h->cfg.seed;
    if (idx < jolt::NUM_INPUTS) return seed + 100ull * (uint64_t)(idx + 1);
    if (idx == ix.rw_v_init) return seed + 45000;
    if (idx == ix.rw_v_final) return seed + 46000;
    if (idx == ix.lasso_out) return seed + 555;
    if (idx >= ix.read_cts && idx < ix.E) return seed + 11000ull * (uint64_t)(idx - ix.read_cts + 1);
    if (idx >= ix.E && idx < ix.lasso_out) return seed + 9000ull * (uint64_t)(idx - ix.E + 1);
    return seed + 13000ull * (uint64_t)(idx - ix.final_cts + 1);
}

void flow_setup_party(cozk_flow* h, FlowParty& ps) {
    const cozk_flow_config& c = h->cfg;
    cozk_ctx* ctx = ps.ctx;
    std::vector<fe> t((size_t)c.log_n);
    for (int i = 0; i < c.log_n; i++) t[(size_t)i] = synthetic_fr_host(c.seed ^ 0x7A7A7A7Aull, (uint64_t)i);
    ps.setup = PST13::setup(ctx, t, c.precompute);
    for (int idx = 0; idx < h->ix.count; idx++) {
        if (h->device_stream[(size_t)idx]) {  // a seeded stream: generated and shared on the device (harness.hip make_share_vectors)
            VecH a, b;
            make_share_vectors(ctx, h->lens[(size_t)idx], h->device_stream[(size_t)idx], ps.party, c.mode, a, b, h->device_bits[(size_t)idx]);
            cozk_poly* p = nullptr;
            rc_check(cozk_poly_create(ctx, c.mode, a.h, b.h, &p), ctx, "poly_create");
            ps.polys.push_back(PolyH(p));
            cozk_vec* view = nullptr;
            rc_check(cozk_poly_share_view(ctx, p, 0, &view), ctx, "share_view");
            ps.commit_vecs.push_back(VecH(view));
            ps.msm_vecs.emplace_back();
            const int bits = h->device_bits[(size_t)idx];
            if (c.mode == COZK_MODE_PLAIN && bits > 0 && bits <= 64) {  // masked by construction; cozk_vec_narrow checks it anyway
                cozk_vec* nv = nullptr;
                rc_check(cozk_vec_narrow(ctx, view, bits <= 32 ? COZK_SCALAR_U32 : COZK_SCALAR_U64, &nv), ctx, "vec_narrow");
                ps.msm_vecs.back() = VecH(nv);
            }
            continue;
        }
        const std::vector<fe>& col = h->clear[(size_t)idx];
        VecH plain = upload_vec(ctx, col.data(), col.size(), COZK_SCALAR_FR, "vec_upload(column)");
        if (h->is_public[(size_t)idx]) {
            ps.polys.push_back(plain_poly(ctx, plain));
            std::vector<uint64_t> ints(col.size());
            for (size_t i = 0; i < col.size(); i++) {
                fe v = Fr::from_mont(col[i]);
                ints[i] = (uint64_t)v.l[0] | ((uint64_t)v.l[1] << 32);
            }
            ps.commit_vecs.push_back(flow_upload_compact(ctx, ints, h->pub_bytes[(size_t)idx]));
            ps.msm_vecs.emplace_back();
        } else {
            ps.polys.push_back(make_shared_poly(ctx, c.mode, plain, flow_share_seed(h, idx), ps.party));
            cozk_poly* p = ps.polys.back().h;
            cozk_vec* view = nullptr;
            rc_check(cozk_poly_share_view(ctx, p, 0, &view), ctx, "share_view");
            ps.commit_vecs.push_back(VecH(view));
            ps.msm_vecs.emplace_back();
            if (c.mode == COZK_MODE_PLAIN) {  // a secret column of a plain prover: as wide as its values (the host has them in the clear)
                uint32_t hi32 = 0, hi64 = 0;
                std::vector<uint64_t> ints(col.size());
                for (size_t i = 0; i < col.size(); i++) {
                    const fe v = Fr::from_mont(col[i]);
                    hi32 |= v.l[1];
                    for (int k = 2; k < 8; k++) hi64 |= v.l[k];
                    ints[i] = (uint64_t)v.l[0] | ((uint64_t)v.l[1] << 32);
                }
                if (!hi64) ps.msm_vecs.back() = flow_upload_compact(ctx, ints, (hi32 | hi64) ? 8 : 4);
            }
        }
    }
    size_t imax = std::max(std::max(h->N, h->M), std::max(h->B, h->MEM));
    std::vector<uint64_t> io(imax);
    for (size_t i = 0; i < imax; i++) io[i] = i;
    ps.iota = flow_upload_compact(ctx, io, 4);
    static const int tab_bytes[6] = {4, 8, 1, 1, 1, 4};
    for (int k = 0; k < 6; k++) ps.bc_table.push_back(flow_upload_compact(ctx, h->bc_table_clear[(size_t)k], tab_bytes[k]));
    for (auto& s : h->subtables_clear) ps.subtables.push_back(flow_upload_compact(ctx, s, 4));
    for (int m = 0; m < c.n_mem; m++) ps.mem_flags.push_back(flow_upload_compact(ctx, flow_mem_flag_column(h, m), 1));
    ps.io_range = upload_vec(ctx, h->io_range_clear.data(), h->MEM, COZK_SCALAR_FR, "vec_upload");
    ps.v_io = upload_vec(ctx, h->v_io_clear.data(), h->MEM, COZK_SCALAR_FR, "vec_upload");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// ------------------------------------------------------------------------------------------------ worker
// batch_evaluate + append of one opening group (compute_openings, lasso/memory_checking/worker.rs:132-176)
void flow_open(WorkerEnv& env, Rep3ProverOpeningAccumulator& acc, const std::vector<cozk_poly*>& polys, const std::vector<fe>& point) {
    VecH chih = mc_eq_table(env, point);
    std::vector<fe> claims = spartan_batch_evaluate(env, polys, chih.h);
    acc.append(env, polys, chih.h, point, claims);
}

// One party across the phases.  A phase reads the committed polynomials through P / CV / T, receives its challenges off env.star and
// leaves its openings in acc, the ONE accumulator that the last phase reduces; nothing else passes from phase to phase.
struct FlowWorker {
    cozk_flow* h;
    FlowParty& ps;
    WorkerEnv env;
    Rep3ProverOpeningAccumulator acc;
    FlowWorker(cozk_flow* h_, FlowParty& ps_, StarNetWorker* star, RingNet* ring)
        : h(h_), ps(ps_), env(make_worker_env(ps_.ctx, h_->cfg.mode, ps_.party, star, ring, &h_->cfg.seed)) {}
    cozk_poly* P(int idx) const { return ps.polys[(size_t)idx].h; }
    const cozk_vec* CV(int idx) const { return ps.commit_vecs[(size_t)idx].h; }
    std::vector<cozk_poly*> Ps(int first, int count) const {
        std::vector<cozk_poly*> v;
        for (int i = 0; i < count; i++) v.push_back(P(first + i));
        return v;
    }
    // a committed polynomial as a leaf term: public ones through their compact column, shared ones through their shares
    LeafTerm T(int idx, const fe& coeff = Fr::zero()) const { return h->is_public[(size_t)idx] ? LeafTerm{CV(idx), nullptr, coeff} : LeafTerm{nullptr, P(idx), coeff}; }
    LeafTerm TC(const VecH& col, const fe& coeff = Fr::zero()) const { return mc_col_term(col.h, coeff); }
    void gammas(int k, std::vector<fe>& g, fe& tau) {  // receive (gamma, tau); g[j] = gamma^j
        fe gamma;
        mc_receive_gamma_tau(env.star, gamma, tau);
        g.assign(1, Fr::one());
        for (int j = 0; j < k; j++) g.push_back(Fr::mul(g.back(), gamma));
    }
    void open(const std::vector<cozk_poly*>& polys, const std::vector<fe>& point) { flow_open(env, acc, polys, point); }
};

// ---- 1. commit-all: every party MSMs every polynomial; only P0's public commitments are kept (pst13.rs:165-229)
void flow_commit_worker(FlowWorker& w) {
    FlowParty& ps = w.ps;
    std::vector<cozk_vec*> vs;
    for (size_t i = 0; i < ps.commit_vecs.size(); i++) vs.push_back(ps.msm_vecs[i].h ? ps.msm_vecs[i].h : ps.commit_vecs[i].h);
    std::vector<PST13Commitment> cm = PST13::batch_commit(ps.ctx, *ps.setup, vs);
    Writer wr;
    put_commitments(wr, cm, w.h->is_public, ps.party);
    w.env.star->send_response(wr.b);
}

// COZK_BYTECODE_FUSED=1 (read on every prove, as COZK_TOGGLE_SPARSE is; unset or 0: the four cozk_fingerprint_leaves launches of
// flow_bytecode_worker, untouched): the bytecode leaves come from cozk_bytecode_leaves and cozk_bytecode_init_final_leaves over the
// same compact columns and the V_IMM polynomial, no iota column read.  The leaves, hence the proof bytes, are the same.
static inline bool flow_bytecode_fused_enabled() {
    const char* e = getenv("COZK_BYTECODE_FUSED");
    return e && atoi(e) == 1;
}
void flow_bytecode_leaves_fused(FlowWorker& w, const int (&bcv)[5], const fe& gamma, const fe& tau, LeafBuf& rw, LeafBuf& inf) {
    const FlowIdx& ix = w.h->ix;
    const int pub[7] = {jolt::V_BYTECODE_A, bcv[0], bcv[1], bcv[2], bcv[3], bcv[4], ix.bc_t_read};
    for (int idx : pub)
        if (!w.h->is_public[(size_t)idx]) throw std::runtime_error("COZK_BYTECODE_FUSED: a bytecode read column is not a public compact column");
    if (w.h->is_public[(size_t)jolt::V_IMM] || !w.h->is_public[(size_t)ix.bc_t_final])
        throw std::runtime_error("COZK_BYTECODE_FUSED: v_imm is a polynomial and t_final a public compact column");
    const cozk_vec *v[5], *table[6];
    for (int k = 0; k < 5; k++) v[k] = w.CV(bcv[k]);
    for (int k = 0; k < 6; k++) table[k] = w.ps.bc_table[(size_t)k].h;
    uint64_t gw[4], tw[4];
    fe_to_u64x4(gamma, gw);
    fe_to_u64x4(tau, tw);
    rc_check(cozk_bytecode_leaves(w.env.ctx, w.CV(jolt::V_BYTECODE_A), v, w.CV(ix.bc_t_read), w.P(jolt::V_IMM), gw, tw, w.env.mode, w.env.party, rw.a.h, rw.b.h, 0),
             w.env.ctx, "bytecode_leaves");
    rc_check(cozk_bytecode_init_final_leaves(w.env.ctx, table, w.CV(ix.bc_t_final), gw, tw, w.env.mode, w.env.party, inf.a.h, inf.b.h, 0), w.env.ctx,
             "bytecode_init_final_leaves");
}

// ---- 2. bytecode (bytecode/worker.rs:43-142): read = a g + v_address g^2 + .. + v_rs2 g^6 + t g^7 + imm - tau, write = read + g^7
void flow_bytecode_worker(FlowWorker& w) {
    const FlowIdx& ix = w.h->ix;
    const size_t N = w.h->N, B = w.h->B;
    const fe one = Fr::one();
    std::vector<fe> g, r_rw, r_if;
    fe tau;
    w.gammas(7, g, tau);
    static const int bcv[5] = {jolt::V_ELF, jolt::V_BITFLAGS, jolt::V_BC_RD, jolt::V_BC_RS1, jolt::V_BC_RS2};
    std::vector<LeafTerm> read = {w.T(jolt::V_BYTECODE_A, g[1])};
    for (int k = 0; k < 5; k++) read.push_back(w.T(bcv[k], g[(size_t)(2 + k)]));
    read.push_back(w.T(ix.bc_t_read, g[7]));
    read.push_back(w.T(jolt::V_IMM, one));
    LeafBuf rw = mc_leaf_alloc(w.env, 2 * N), inf = mc_leaf_alloc(w.env, 2 * B);
    if (flow_bytecode_fused_enabled()) {
        flow_bytecode_leaves_fused(w, bcv, g[1], tau, rw, inf);
    } else {
        mc_fingerprint_leaves(w.env, read, Fr::neg(tau), rw, 0, N);
        mc_fingerprint_leaves(w.env, read, Fr::sub(g[7], tau), rw, N, N);
        std::vector<LeafTerm> init = {w.TC(w.ps.iota, g[1])};
        for (int k = 0; k < 5; k++) init.push_back(w.TC(w.ps.bc_table[(size_t)k], g[(size_t)(2 + k)]));
        init.push_back(w.TC(w.ps.bc_table[5], one));
        mc_fingerprint_leaves(w.env, init, Fr::neg(tau), inf, 0, B);
        init.push_back(w.T(ix.bc_t_final, g[7]));
        mc_fingerprint_leaves(w.env, init, Fr::neg(tau), inf, B, B);
    }
    mc_memory_checking(w.env, mc_leaves_to_layer(w.env, rw), 2, ToggleH(), mc_leaves_to_layer(w.env, inf), 2, r_rw, r_if);
    std::vector<cozk_poly*> rwp = {w.P(jolt::V_BYTECODE_A)};
    for (int k = 0; k < 5; k++) rwp.push_back(w.P(bcv[k]));
    rwp.push_back(w.P(jolt::V_IMM));
    rwp.push_back(w.P(ix.bc_t_read));
    w.open(rwp, r_rw);
    w.open({w.P(ix.bc_t_final)}, r_if);
}

// ---- 3a. instruction lookups, the primary sumcheck (instruction_lookups/worker.rs:95-141)
void flow_primary_worker(FlowWorker& w) {
    cozk_flow* h = w.h;
    const cozk_flow_config& c = h->cfg;
    const FlowIdx& ix = h->ix;
    const std::vector<cozk_poly*> E_polys = w.Ps(ix.E, c.n_mem), iflag_polys = w.Ps(jolt::V_INSTR, jolt::N_INSTR);
    VecH eqh = mc_eq_table(w.env, mc_receive_point(w.env.star));
    std::vector<const cozk_vec*> fl;
    for (int i = 0; i < jolt::N_INSTR; i++) fl.push_back(w.CV(jolt::V_INSTR + i));
    std::vector<const cozk_poly*> Ec(E_polys.begin(), E_polys.end());
    cozk_primary* pr = nullptr;
    rc_check(cozk_primary_create(w.env.ctx, c.mode, w.ps.party, h->instrs.data(), h->instrs.size(), fl.data(), Ec.data(), (size_t)c.n_mem, w.P(ix.lasso_out), eqh.h, &pr),
             w.env.ctx, "primary_create");
    PrimaryH prh(pr);
    std::vector<fe> rs = prove_primary_sumcheck_worker(w.env, pr, c.log_n, (size_t)c.n_mem, h->instrs.size());
    std::vector<fe> r_primary(rs.rbegin(), rs.rend());
    std::vector<cozk_poly*> pp(E_polys);
    pp.insert(pp.end(), iflag_polys.begin(), iflag_polys.end());
    pp.push_back(w.P(ix.lasso_out));
    w.open(pp, r_primary);
}

// ---- 3b. instruction lookups, memory checking with the TOGGLED read / write grand product (instruction_lookups/worker.rs:742-860)
void flow_lookups_worker(FlowWorker& w) {
    const cozk_flow_config& c = w.h->cfg;
    const FlowIdx& ix = w.h->ix;
    const size_t N = w.h->N, M = w.h->M;
    const fe one = Fr::one();
    std::vector<fe> g, r_rw, r_if;
    fe tau;
    w.gammas(2, g, tau);
    LeafBuf rw = mc_leaf_alloc(w.env, 2 * (size_t)c.n_mem * N), inf = mc_leaf_alloc(w.env, (size_t)(c.n_subtables + c.n_mem) * M);
    for (int m = 0; m < c.n_mem; m++) {  // read = t g^2 + v g + a - tau, write = read + g^2 (:776-800)
        std::vector<LeafTerm> terms = {w.T(ix.read_cts + m, g[2]), w.T(ix.E + m, g[1]), w.T(jolt::V_QUERY + m % 4, one)};
        mc_fingerprint_leaves(w.env, terms, Fr::neg(tau), rw, (size_t)(2 * m) * N, N);
        mc_fingerprint_leaves(w.env, terms, Fr::sub(g[2], tau), rw, (size_t)(2 * m + 1) * N, N);
    }
    size_t off = 0;
    for (int s = 0; s < c.n_subtables; s++) {  // per subtable: init, then the finals of its memories (:803-833)
        std::vector<LeafTerm> init = {w.TC(w.ps.subtables[(size_t)s], g[1]), w.TC(w.ps.iota, one)};
        mc_fingerprint_leaves(w.env, init, Fr::neg(tau), inf, off, M);
        off += M;
        for (int m = 0; m < c.n_mem; m++) {
            if (m % c.n_subtables != s) continue;
            std::vector<LeafTerm> fin(init);
            fin.push_back(w.T(ix.final_cts + m, g[2]));
            mc_fingerprint_leaves(w.env, fin, Fr::neg(tau), inf, off, M);
            off += M;
        }
    }
    std::vector<const cozk_vec*> mf;
    for (auto& f : w.ps.mem_flags) mf.push_back(f.h);
    cozk_toggle* tg = nullptr;
    rc_check(cozk_toggle_create(w.env.ctx, c.mode, mf.data(), mf.size(), rw.a.h, rw.b.h, 1, &tg), w.env.ctx, "toggle_create");
    mc_memory_checking(w.env, LayerH(), 0, ToggleH(tg), mc_leaves_to_layer(w.env, inf), (size_t)(c.n_subtables + c.n_mem), r_rw, r_if);
    std::vector<cozk_poly*> rwp = w.Ps(jolt::V_QUERY, 4);
    for (const std::vector<cozk_poly*>& part : {w.Ps(ix.read_cts, c.n_mem), w.Ps(ix.E, c.n_mem), w.Ps(jolt::V_INSTR, jolt::N_INSTR)}) rwp.insert(rwp.end(), part.begin(), part.end());
    rwp.push_back(w.P(ix.lasso_out));
    w.open(rwp, r_rw);
    w.open(w.Ps(ix.final_cts, c.n_mem), r_if);
}

// COZK_RW_FUSED=1 (read on every prove, as COZK_BYTECODE_FUSED is; unset or 0: the ten cozk_fingerprint_leaves launches of
// flow_rw_memory_worker, untouched): the read-write memory leaves come from cozk_rw_memory_shared_leaves and
// cozk_rw_memory_shared_init_final_leaves over the same compact address and timestamp columns and the value polynomials (a public value
// column goes in as its PLAIN polynomial), no iota column read.  The leaves, hence the proof bytes, are the same.
static inline bool flow_rw_fused_enabled() {
    const char* e = getenv("COZK_RW_FUSED");
    return e && atoi(e) == 1;
}
// regs: the four slots as {a, v_read, v_write, index of t_read}
void flow_rw_leaves_fused(FlowWorker& w, const int (&regs)[4][4], const fe& gamma, const fe& tau, LeafBuf& rw, LeafBuf& inf) {
    const FlowIdx& ix = w.h->ix;
    auto compact = [&](int idx, bool u8_too) {
        if (!w.h->is_public[(size_t)idx]) return false;
        const int kind = w.CV(idx)->kind;
        return kind == COZK_SCALAR_U32 || (u8_too && kind == COZK_SCALAR_U8);
    };
    const cozk_vec *a[4], *tr[4];
    const cozk_poly *vr[4], *vw[4];
    for (int s = 0; s < 4; s++) {
        const int* r = regs[s];
        if (!compact(r[0], true)) throw std::runtime_error("COZK_RW_FUSED: an address column is not a public U8 or U32 column");
        if (!compact(ix.rw_t_read + r[3], false)) throw std::runtime_error("COZK_RW_FUSED: a read timestamp column is not a public U32 column");
        a[s] = w.CV(r[0]), tr[s] = w.CV(ix.rw_t_read + r[3]);
        vr[s] = w.P(r[1]), vw[s] = r[2] == r[1] ? nullptr : w.P(r[2]);
    }
    if (!compact(ix.rw_t_final, false)) throw std::runtime_error("COZK_RW_FUSED: t_final is not a public U32 column");
    uint64_t gw[4], tw[4];
    fe_to_u64x4(gamma, gw);
    fe_to_u64x4(tau, tw);
    rc_check(cozk_rw_memory_shared_leaves(w.env.ctx, a, vr, tr, vw, 4, gw, tw, w.env.mode, w.env.party, rw.a.h, rw.b.h, 0), w.env.ctx, "rw_memory_shared_leaves");
    rc_check(cozk_rw_memory_shared_init_final_leaves(w.env.ctx, w.P(ix.rw_v_init), w.P(ix.rw_v_final), w.CV(ix.rw_t_final), gw, tw, w.env.mode, w.env.party, inf.a.h, inf.b.h, 0),
             w.env.ctx, "rw_memory_shared_init_final_leaves");
}

// ---- 4a. read-write memory (read_write_memory/worker.rs:196-344): the shared leaves over the committed polynomials
void flow_rw_memory_worker(FlowWorker& w) {
    const FlowIdx& ix = w.h->ix;
    const size_t N = w.h->N, MEM = w.h->MEM;
    std::vector<fe> g, r_rw, r_if;
    fe tau;
    w.gammas(2, g, tau);
    // rs1, rs2, rd, ram as {a, v_read, v_write, index of t_read}: the read timestamps are committed in the order rd, rs1, rs2, ram
    static const int regs[4][4] = {{jolt::V_BC_RS1, jolt::V_RS1, jolt::V_RS1, 1}, {jolt::V_BC_RS2, jolt::V_RS2, jolt::V_RS2, 2}, {jolt::V_BC_RD, jolt::V_RD_READ, jolt::V_RD_WRITE, 0},
                                   {jolt::V_RAM_ADDR, jolt::V_RAM_READ, jolt::V_RAM_WRITE, 3}};
    std::vector<RwSlotLeaves> slots;
    for (const int* r : regs) slots.push_back({w.T(r[0]), w.T(r[1]), w.T(r[2]), w.T(ix.rw_t_read + r[3])});
    LeafBuf rw = mc_leaf_alloc(w.env, 8 * N), inf = mc_leaf_alloc(w.env, 2 * MEM);
    if (flow_rw_fused_enabled()) flow_rw_leaves_fused(w, regs, g[1], tau, rw, inf);
    else rw_memory_leaves_composed(w.env, slots, w.T(ix.rw_v_init), w.T(ix.rw_v_final), w.T(ix.rw_t_final), w.TC(w.ps.iota), w.TC(w.ps.iota), N, MEM, g[1], tau, rw, inf);
    mc_memory_checking(w.env, mc_leaves_to_layer(w.env, rw), 8, ToggleH(), mc_leaves_to_layer(w.env, inf), 2, r_rw, r_if);
    std::vector<cozk_poly*> rwp = {w.P(jolt::V_RAM_ADDR), w.P(jolt::V_RD_READ), w.P(jolt::V_RS1), w.P(jolt::V_RS2), w.P(jolt::V_RAM_READ), w.P(jolt::V_RD_WRITE), w.P(jolt::V_RAM_WRITE)};
    for (int k = 0; k < 4; k++) rwp.push_back(w.P(ix.rw_t_read + k));
    rwp.push_back(w.P(jolt::V_BC_RD));
    rwp.push_back(w.P(jolt::V_BC_RS1));
    rwp.push_back(w.P(jolt::V_BC_RS2));
    w.open(rwp, r_rw);
    w.open({w.P(ix.rw_v_final), w.P(ix.rw_t_final)}, r_if);
}

// ---- 4b. prove_outputs (read_write_memory/worker.rs:109-180), then v_final opened at the sumcheck's point
void flow_outputs_worker(FlowWorker& w) {
    const int v_final = w.h->ix.rw_v_final;
    const std::vector<fe> r_eq = mc_receive_point(w.env.star);
    w.open({w.P(v_final)}, prove_outputs_dense_worker(w.env, w.P(v_final), w.ps.io_range, w.ps.v_io, w.h->cfg.log_mem, r_eq));
}

void flow_worker_main(cozk_flow* h, FlowParty& ps, StarNetWorker* star, RingNet* ring) {
    FlowWorker w(h, ps, star, ring);
    const double t0 = now_ms();
    flow_commit_worker(w);
    const double t1 = now_ms();
    flow_bytecode_worker(w);
    const double t2 = now_ms();
    flow_primary_worker(w);
    const double t3 = now_ms();
    flow_lookups_worker(w);
    const double t4 = now_ms();
    flow_rw_memory_worker(w);
    flow_outputs_worker(w);
    const double t5 = now_ms();
    // ---- 5. Spartan
    ps.sp_times = SpartanTimes();
    prove_spartan_worker(w.env, h->sys, w.Ps(0, jolt::NUM_INPUTS), h->N, w.acc, &ps.sp_times);
    const double t6 = now_ms();
    // ---- 6. one reduce_and_prove over everything
    w.acc.reduce_and_prove_worker(w.env, *ps.setup);
    const double t7 = now_ms();
    ps.t_commit = t1 - t0, ps.t_bytecode = t2 - t1, ps.t_primary = t3 - t2, ps.t_lookups_gp = t4 - t3;
    ps.t_rw = t5 - t4, ps.t_spartan = t6 - t5, ps.t_open = t7 - t6, ps.t_total = t7 - t0;
    ps.record_net(star, ring);
}

// ------------------------------------------------------------------------------------------------ coordinator
void flow_coordinate(cozk_flow* h, StarNetCoordinator& net, FlowProof& proof) {
    const cozk_flow_config& c = h->cfg;
    Transcript tr("cozk-jolt");
    {
        std::vector<Bytes> msgs = net.receive_responses();
        std::vector<Reader> rds;
        for (auto& m : msgs) rds.emplace_back(m);
        proof.commitments = combine_commitments_from_parties(rds, h->nparties);
        for (auto& cm : proof.commitments) tr.append_point(cm.g_product);
    }
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.bytecode, (size_t)c.log_n, false, (size_t)c.log_b);
    {
        std::vector<fe> r_primary;
        (void)broadcast_challenge_vector(net, tr, (size_t)c.log_n);
        proof.primary = coordinate_primary_sumcheck(net, tr, c.log_n, r_primary, h->nparties, 0);
        proof.primary_claims = Rep3ProverOpeningAccumulator::receive_claims(net, tr);
    }
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.lookups, (size_t)c.log_n + 1, true, (size_t)c.log_m);
    mc_broadcast_gamma_tau(net, tr);
    mc_coordinate_memory_checking(net, tr, proof.rw, (size_t)c.log_n, false, (size_t)c.log_mem);
    coordinate_outputs(net, tr, c.log_mem, proof.outputs, proof.outputs_claims);
    proof.spartan = coordinate_spartan(net, tr, h->sys, h->N);
    std::vector<fe> r_red;
    fe rho, gamma;
    proof.reduced = Rep3ProverOpeningAccumulator::reduce_and_prove(net, tr, r_red, rho, gamma);
}

// ------------------------------------------------------------------------------------------------ plain verifier
// The verifier across the phases: a phase replays its part of the transcript vt, leaves its openings in opens and names the first
// check that fails in why; nothing else passes from phase to phase.
struct FlowVerifier {
    cozk_flow* h;
    const FlowProof& proof;
    Transcript vt;
    VerifierOpenings opens;
    std::string& why;
    FlowVerifier(cozk_flow* h_, const FlowProof& p, std::string& w) : h(h_), proof(p), vt("cozk-jolt"), opens(vt), why(w) {}
    void gammas(int k, std::vector<fe>& g, fe& tau) {  // (gamma, tau) off the transcript; g[j] = gamma^j
        fe gamma = vt.challenge_scalar();
        tau = vt.challenge_scalar();
        g.assign(1, Fr::one());
        for (int j = 0; j < k; j++) g.push_back(Fr::mul(g.back(), gamma));
    }
};

// ---- 2. bytecode
bool flow_verify_bytecode(FlowVerifier& v) {
    cozk_flow* h = v.h;
    const FlowIdx& ix = h->ix;
    const MemCheckProof& mp = v.proof.bytecode;
    std::vector<fe> g;
    fe tau;
    v.gammas(7, g, tau);
    MemCheckPoints p;
    if (!mc_verify_grand_products(mp, false, 2, 2, (size_t)h->cfg.log_n, (size_t)h->cfg.log_b, v.vt, p)) {
        v.why = "bytecode: grand products";
        return false;
    }
    std::vector<int> rwp = {jolt::V_BYTECODE_A, jolt::V_ELF, jolt::V_BITFLAGS, jolt::V_BC_RD, jolt::V_BC_RS1, jolt::V_BC_RS2, jolt::V_IMM, ix.bc_t_read};
    if (!v.opens.take(rwp, p.lo, mp.rw_claims) || !v.opens.take(std::vector<int>{ix.bc_t_final}, p.lo2, mp.if_claims)) {
        v.why = "bytecode: claims";
        return false;
    }
    const std::vector<fe>& cl = mp.rw_claims;
    fe read = Fr::sub(cl[6], tau);
    for (int k = 0; k < 6; k++) read = Fr::add(read, Fr::mul(g[(size_t)(1 + k)], cl[(size_t)k]));
    read = Fr::add(read, Fr::mul(g[7], cl[7]));
    if (!Fr::eq(mc_batch_eval({read, Fr::add(read, g[7])}, p.hi, Fr::zero()), p.rw_claim)) {
        v.why = "bytecode: read / write fingerprints != the GKR claim";
        return false;
    }
    std::vector<fe> initv(h->B);
    for (size_t i = 0; i < h->B; i++) {
        fe x = Fr::sub(Fr::add(Fr::from_u64(h->bc_table_clear[5][i]), Fr::mul(g[1], Fr::from_u64(i))), tau);
        for (int k = 0; k < 5; k++) x = Fr::add(x, Fr::mul(g[(size_t)(2 + k)], Fr::from_u64(h->bc_table_clear[(size_t)k][i])));
        initv[i] = x;
    }
    fe init = mc_mle_host(initv, p.lo2);
    if (!Fr::eq(mc_batch_eval({init, Fr::add(init, Fr::mul(g[7], mp.if_claims[0]))}, p.hi2, Fr::zero()), p.if_claim)) {
        v.why = "bytecode: init / final fingerprints != the GKR claim";
        return false;
    }
    return true;
}

// ---- 3a. instruction lookups, the primary sumcheck
bool flow_verify_primary(FlowVerifier& v) {
    cozk_flow* h = v.h;
    const cozk_flow_config& c = h->cfg;
    std::vector<fe> r_eq = v.vt.challenge_vector((size_t)c.log_n), rs;
    const int degree = primary_sumcheck_degree(h->instrs);
    if (!verify_primary_sumcheck(v.proof.primary, h->instrs, (size_t)c.n_mem, degree, r_eq, v.vt, rs)) {
        v.why = "primary sumcheck";
        return false;
    }
    if (!mc_vec_eq(v.proof.primary_claims, v.proof.primary.openings)) {
        v.why = "primary sumcheck: openings != the accumulator's claims";
        return false;
    }
    std::vector<int> pp;
    for (int m = 0; m < c.n_mem; m++) pp.push_back(h->ix.E + m);
    for (int i = 0; i < jolt::N_INSTR; i++) pp.push_back(jolt::V_INSTR + i);
    pp.push_back(h->ix.lasso_out);
    v.opens.take(pp, std::vector<fe>(rs.rbegin(), rs.rend()), v.proof.primary_claims);
    return true;
}

// check_multiset_equality (lasso/memory_checking/worker.rs:40-127): init * writes == reads * finals per memory.  The one check of a
// CONSISTENT witness: it holds for the counters of cfg.lookups_witness, not for seeded streams.
bool flow_lookups_multiset_holds(const cozk_flow_config& c, const MemCheckProof& mp) {
    const std::vector<fe>& rwh = mp.rw_hashes;
    const std::vector<fe>& ifh = mp.if_hashes;
    std::vector<size_t> init_at((size_t)c.n_subtables), final_at((size_t)c.n_mem);
    size_t at = 0;
    for (int s = 0; s < c.n_subtables; s++) {  // if_hashes per subtable: the init, then the finals of its memories
        init_at[(size_t)s] = at++;
        for (int m = 0; m < c.n_mem; m++)
            if (m % c.n_subtables == s) final_at[(size_t)m] = at++;
    }
    for (int m = 0; m < c.n_mem; m++) {
        const fe reads_finals = Fr::mul(rwh[(size_t)(2 * m)], ifh[final_at[(size_t)m]]);
        const fe writes_init = Fr::mul(rwh[(size_t)(2 * m + 1)], ifh[init_at[(size_t)(m % c.n_subtables)]]);
        if (!Fr::eq(reads_finals, writes_init)) return false;
    }
    return true;
}

// ---- 3b. instruction lookups, memory checking
bool flow_verify_lookups(FlowVerifier& v) {
    cozk_flow* h = v.h;
    const cozk_flow_config& c = h->cfg;
    const FlowIdx& ix = h->ix;
    const MemCheckProof& mp = v.proof.lookups;
    std::vector<fe> g;
    fe tau;
    v.gammas(2, g, tau);
    const size_t rw_batch = 2 * (size_t)c.n_mem, if_batch = (size_t)(c.n_subtables + c.n_mem);
    MemCheckPoints p;
    if (!mc_verify_grand_products(mp, true, rw_batch, if_batch, (size_t)c.log_n + 1, (size_t)c.log_m, v.vt, p)) {
        v.why = "lookups: grand products";
        return false;
    }
    std::vector<int> rwp, fcp;
    for (int i = 0; i < 4; i++) rwp.push_back(jolt::V_QUERY + i);
    for (int m = 0; m < c.n_mem; m++) rwp.push_back(ix.read_cts + m);
    for (int m = 0; m < c.n_mem; m++) rwp.push_back(ix.E + m);
    for (int i = 0; i < jolt::N_INSTR; i++) rwp.push_back(jolt::V_INSTR + i);
    rwp.push_back(ix.lasso_out);
    for (int m = 0; m < c.n_mem; m++) fcp.push_back(ix.final_cts + m);
    if (!v.opens.take(rwp, p.lo, mp.rw_claims) || !v.opens.take(fcp, p.lo2, mp.if_claims)) {
        v.why = "lookups: claims";
        return false;
    }
    const std::vector<fe>& cl = mp.rw_claims;
    const size_t o_rc = 4, o_E = 4 + (size_t)c.n_mem, o_fl = 4 + 2 * (size_t)c.n_mem;
    std::vector<fe> fps, fls;
    for (int m = 0; m < c.n_mem; m++) {
        fe read = Fr::sub(Fr::add(Fr::add(Fr::mul(g[2], cl[o_rc + (size_t)m]), Fr::mul(g[1], cl[o_E + (size_t)m])), cl[(size_t)(m % 4)]), tau);
        fps.push_back(read);
        fps.push_back(Fr::add(read, g[2]));
        fe fl = Fr::zero();  // the memory's flag = sum of the (one-hot) instruction flags that use it
        for (int i = 0; i < jolt::N_INSTR; i++) {
            const cozk_primary_instr& in = h->instrs[(size_t)i];
            bool uses = false;
            for (int j = 0; j < in.n_mems; j++) uses |= in.mems[j] == m;
            if (uses) fl = Fr::add(fl, cl[o_fl + (size_t)i]);
        }
        fls.push_back(fl);
        fls.push_back(fl);
    }
    if (!Fr::eq(mc_batch_eval(fls, p.hi, Fr::one()), p.flag_claim) || !Fr::eq(mc_batch_eval(fps, p.hi, Fr::zero()), p.rw_claim)) {
        v.why = "lookups: toggle layer's flag / fingerprint claims != the opened values";
        return false;
    }
    std::vector<fe> leaves;
    fe io = mc_iota_eval(p.lo2);
    for (int s = 0; s < c.n_subtables; s++) {
        std::vector<fe> sv(h->M);
        for (size_t i = 0; i < h->M; i++) sv[i] = Fr::from_u64(h->subtables_clear[(size_t)s][i]);
        fe init = Fr::sub(Fr::add(Fr::mul(g[1], mc_mle_host(sv, p.lo2)), io), tau);
        leaves.push_back(init);
        for (int m = 0; m < c.n_mem; m++)
            if (m % c.n_subtables == s) leaves.push_back(Fr::add(init, Fr::mul(g[2], mp.if_claims[(size_t)m])));
    }
    if (!Fr::eq(mc_batch_eval(leaves, p.hi2, Fr::zero()), p.if_claim)) {
        v.why = "lookups: init / final fingerprints != the GKR claim";
        return false;
    }
    if (c.lookups_witness && !flow_lookups_multiset_holds(c, mp)) {
        v.why = "lookups: multiset equality of the memory-checking hashes";
        return false;
    }
    return true;
}

// ---- 4a. read-write memory: the verifier of rw_memory_proof.hpp's memory check, minus the multiset check (seeded counters)
bool flow_verify_rw_memory(FlowVerifier& v) {
    cozk_flow* h = v.h;
    const FlowIdx& ix = h->ix;
    const MemCheckProof& mp = v.proof.rw;
    std::vector<fe> g;
    fe tau;
    v.gammas(2, g, tau);
    MemCheckPoints p;
    if (!mc_verify_grand_products(mp, false, 8, 2, (size_t)h->cfg.log_n, (size_t)h->cfg.log_mem, v.vt, p)) {
        v.why = "read-write memory: grand products";
        return false;
    }
    std::vector<int> rwp = {jolt::V_RAM_ADDR, jolt::V_RD_READ, jolt::V_RS1, jolt::V_RS2, jolt::V_RAM_READ, jolt::V_RD_WRITE, jolt::V_RAM_WRITE,
                            ix.rw_t_read, ix.rw_t_read + 1, ix.rw_t_read + 2, ix.rw_t_read + 3, jolt::V_BC_RD, jolt::V_BC_RS1, jolt::V_BC_RS2};
    if (!v.opens.take(rwp, p.lo, mp.rw_claims) || !v.opens.take(std::vector<int>{ix.rw_v_final, ix.rw_t_final}, p.lo2, mp.if_claims)) {
        v.why = "read-write memory: claims";
        return false;
    }
    // claims: a_ram 0, v_read_rd 1, v_read_rs1 2, v_read_rs2 3, v_read_ram 4, v_write_rd 5, v_write_ram 6, t_read rd 7 rs1 8 rs2 9 ram 10, a_rd 11, a_rs1 12, a_rs2 13
    static const std::vector<RwSlotClaims> regs = {{12, 2, 2, 8}, {13, 3, 3, 9}, {11, 1, 5, 7}, {0, 4, 6, 10}};
    fe rw_claim, if_claim;  // VerifierComputedOpening of v_init
    rw_memory_verify_leaves(mp.rw_claims, mp.if_claims, regs, mc_mle_host(h->clear[(size_t)ix.rw_v_init], p.lo2), g[1], tau, p, rw_claim, if_claim);
    if (!Fr::eq(rw_claim, p.rw_claim)) {
        v.why = "read-write memory: read / write fingerprints != the GKR claim";
        return false;
    }
    if (!Fr::eq(if_claim, p.if_claim)) {
        v.why = "read-write memory: init / final fingerprints != the GKR claim";
        return false;
    }
    return true;
}

// ---- 4b. the output check, io_range and v_io evaluated over all of memory
bool flow_verify_outputs(FlowVerifier& v) {
    cozk_flow* h = v.h;
    std::vector<fe> r_eq, r_out;
    fe claim;
    if (!verify_outputs(v.vt, h->cfg.log_mem, v.proof.outputs, v.proof.outputs_claims, r_eq, r_out, claim)) {
        v.why = "output check: shape";
        return false;
    }
    if (!outputs_final_holds(r_eq, r_out, mc_mle_host(h->io_range_clear, r_out), mc_mle_host(h->v_io_clear, r_out), v.proof.outputs_claims[0], claim)) {
        v.why = "output check: final claim";
        return false;
    }
    v.opens.take(std::vector<int>{h->ix.rw_v_final}, r_out, v.proof.outputs_claims);
    return true;
}

// ---- 5. Spartan
bool flow_verify_spartan(FlowVerifier& v) {
    std::vector<fe> rx_step, shift_r;
    fe rho[2];
    if (!verify_spartan(v.proof.spartan, v.h->sys, v.h->N, v.vt, rx_step, shift_r, rho, v.why)) return false;
    std::vector<int> cols;
    for (int i = 0; i < jolt::NUM_INPUTS; i++) cols.push_back(i);
    v.opens.take(cols, rx_step, v.proof.spartan.witness_evals, &rho[0]);
    v.opens.take(cols, shift_r, v.proof.spartan.shift_witness_evals, &rho[1]);
    return true;
}

// The phases in the transcript's order, then 6. the batched opening (opening_proof.rs:181-235 + the verifier's reduce_and_verify, out of
// tree): the reduction sumcheck over all openings and ONE PST13 check of the joint polynomial (pairing-free, trapdoor known)
bool flow_verify(cozk_flow* h, const FlowProof& proof, std::string& why) {
    FlowVerifier v(h, proof, why);
    if ((int)proof.commitments.size() != h->ix.count) {
        why = "commitment count";
        return false;
    }
    for (auto& cm : proof.commitments) v.vt.append_point(cm.g_product);
    return flow_verify_bytecode(v) && flow_verify_primary(v) && flow_verify_lookups(v) && flow_verify_rw_memory(v) && flow_verify_outputs(v) && flow_verify_spartan(v) &&
           verify_reduced_opening(v.opens.list, proof.commitments, v.vt, proof.reduced, *h->parties[0].setup, "opening reduction: shape", "opening reduction: final check", why);
}

}  // namespace

extern "C" {

int cozk_flow_create(const cozk_flow_config* cfg, cozk_flow** out) {
    return harness_create(cfg, out, [&](cozk_flow* h) {
        COZK_REQUIRE(cfg->mode == COZK_MODE_PLAIN || cfg->mode == COZK_MODE_REP3, "flow: mode");
        COZK_REQUIRE(cfg->log_n >= 1 && cfg->log_n <= 22, "flow: log_n in 1..22");
        COZK_REQUIRE(cfg->log_m >= 1 && cfg->log_m <= cfg->log_n && cfg->log_b >= 1 && cfg->log_b <= cfg->log_n && cfg->log_mem >= 2 && cfg->log_mem <= cfg->log_n,
                     "flow: log_m, log_b in 1..log_n, log_mem in 2..log_n");
        COZK_REQUIRE(cfg->n_mem >= 1 && cfg->n_mem <= 128 && cfg->n_subtables >= 1 && cfg->n_subtables <= cfg->n_mem, "flow: n_mem in 1..128, n_subtables in 1..n_mem");
        h->nparties = cfg->mode == COZK_MODE_REP3 ? 3 : 1;
        h->N = (size_t)1 << cfg->log_n;
        h->M = (size_t)1 << cfg->log_m;
        h->B = (size_t)1 << cfg->log_b;
        h->MEM = (size_t)1 << cfg->log_mem;
        COZK_REQUIRE(!cfg->lookups_witness || cfg->log_m == 16,
                     "flow: lookups_witness needs log_m == 16 (the addresses are the committed 16-bit query chunks), hence log_n >= 16");
        COZK_REQUIRE(cfg->lookups_tamper >= 0 && (cfg->lookups_tamper == 0 || (cfg->lookups_witness && (size_t)cfg->lookups_tamper <= h->M)),
                     "flow: lookups_tamper in 0..2^log_m, with lookups_witness");
        h->ix = FlowIdx(cfg->n_mem);
        jolt::build_system(h->sys);
        h->parties.resize((size_t)h->nparties);
        const char* no_ctx = "flow: cannot create a context (no HIP device?)";
        if (cfg->lookups_witness) h->parties[0].open_ctx(cfg->devices[0], no_ctx);  // the dealer's counting pass runs on party 0's device
        flow_build_clear(h);
        for (int p = 0; p < h->nparties; p++) {
            FlowParty& ps = h->parties[(size_t)p];
            ps.party = p;
            if (!ps.ctx) ps.open_ctx(cfg->devices[p], no_ctx);
            cozk_ctx_set_resident_rounds(ps.ctx, h->nparties > 1 ? 0 : 1);
            flow_setup_party(h, ps);
        }
    });
}

const char* cozk_flow_error(const cozk_flow* h) { return harness_error(h); }

int cozk_flow_destroy(cozk_flow* h) {
    if (!h) return COZK_OK;
    release_parties(h->parties, [](FlowParty& ps) {
        ps.polys.clear();
        ps.commit_vecs.clear();
        ps.msm_vecs.clear();
        ps.setup.reset();
        ps.iota = VecH();
        ps.bc_table.clear();
        ps.subtables.clear();
        ps.mem_flags.clear();
        ps.io_range = VecH();
        ps.v_io = VecH();
    });
    delete h;
    return COZK_OK;
}

size_t cozk_flow_num_polys(const cozk_flow* h) { return h ? (size_t)h->ix.count : 0; }

cozk_ctx* cozk_flow_ctx(cozk_flow* h, int party) { return h ? party_ctx(h->parties, party) : nullptr; }

int cozk_flow_prove(cozk_flow* h, int verify, cozk_flow_result* res) {
    if (!harness_prove_begin(h, res)) return COZK_ERR_INVALID_ARG;
    const int np = h->nparties;
    InProcNets nets(np, np == 3);
    std::vector<Participant> parts;
    add_participants(parts, "party", h->parties, [&](FlowParty& ps, int p) { flow_worker_main(h, ps, nets.worker(p), nets.ring(p)); });
    FlowProof proof;
    double wall_ms = 0;
    int rc = run_in_process(nets, parts, [&] {
        InProcStarCoordinator coord(&nets.star);
        flow_coordinate(h, coord, proof);
    }, h->error, wall_ms);
    if (rc != COZK_OK) return rc;
    res->wall_ms = wall_ms;  // the verifier below is outside the clock
    if (verify) harness_verify(h, res, h->parties[0].ctx->device, [&](std::string& why) { return flow_verify(h, proof, why); });
    for (const FlowParty& ps : h->parties) {
        res->t_commit_ms = std::max(res->t_commit_ms, ps.t_commit);
        res->t_bytecode_ms = std::max(res->t_bytecode_ms, ps.t_bytecode);
        res->t_primary_ms = std::max(res->t_primary_ms, ps.t_primary);
        res->t_lookups_gp_ms = std::max(res->t_lookups_gp_ms, ps.t_lookups_gp);
        res->t_rw_ms = std::max(res->t_rw_ms, ps.t_rw);
        res->t_spartan_ms = std::max(res->t_spartan_ms, ps.t_spartan);
        res->t_open_ms = std::max(res->t_open_ms, ps.t_open);
        res->t_worker_ms = std::max(res->t_worker_ms, ps.t_total);
        res->t_spartan_build_ms = std::max(res->t_spartan_build_ms, ps.sp_times.t_build);
        res->bytes_star_up += ps.star_up;
        res->bytes_star_down += ps.star_down;
        res->bytes_ring += ps.ring_bytes;
        res->star_messages += ps.star_msgs;
    }
    res->n_polys = (uint64_t)h->ix.count;
    res->n_openings = 10;
    finish_proof(h, proof.serialize(), res);
    return COZK_OK;
}

int cozk_flow_proof_bytes(const cozk_flow* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

}  // extern "C"
