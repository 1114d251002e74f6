// Lasso's primary sumcheck of the instruction lookups (prove_primary_sumcheck, jolt/vm/instruction_lookups/worker.rs:180-452; the
// lookups harness's primary phase) proved by n Shamir parties, all driven from the one thread that owns their contexts and plays the
// coordinator, as the Spartan workers are (shamir_jolt_spartan.hpp).  The reference has no Shamir prover; tests/shamir_primary_ref.py
// restates this file in big integers.  Included by harness.hip behind lookups_harness.hpp (the instance, the verifier's view) and
// shamir_harness.hpp (the handle base, the keys and the dealing, ShamirProve: the openings, the masks).
//
// Why the PLAIN kernels serve.  csrc/primary_sumcheck.inc compiles every multiplicative collation into slots that are sums of products
// of TWO affine forms, with a last step that stays local.  A party that runs the PLAIN program on degree-t shares therefore holds a
// point of a degree-2t sharing of every slot of a level -- and would hold degree 4t one level later.  So between the levels, where Rep3
// reshares over the ring, the 2t + 1 senders reduce the degree (GRR): every sender re-deals its slot values with a fresh degree-t
// polynomial, every sender combines what it was dealt with lagrange(1..2t + 1).  Public constants are added to every party's value
// (COZK_MODE_PLAIN does that): the constant sharing.  The last step multiplies two degree-t values and eq, the flags are public: the
// round message is a degree-2t sharing of the plain prover's, opened from senders 0..2t behind a degree-2t zero mask.  The coordinator's
// arithmetic is coordinate_primary_sumcheck's (primary_coordinator_round, prover.hpp).  So the proof is the plain prover's, byte for
// byte (LookupsHarness(mode = plain, primary = 1) up to proof_len; oracle/pyprimary.prove), accepted by verify_primary_sumcheck.
//
//   witness   flags and eq public.  E_m and lookup_outputs dealt by cozk_shamir_share_vec's rule, column v at share_counter + v 2^log_n,
//             lookup_outputs = column n_mem; the share keys are shamir_harness_keys'.  Only the senders keep their shares.
//   exchange  e-th exchange with n_elems > 0, in the order they happen: counter mul_counter + sum of the earlier exchanges' n_elems;
//             sender p's mul key c = the harness key (seed ^ 0x4D554C54, 64 p + c), c < t.
//   masks     M = D log_n openings of degree 2t (ShamirProve::deal_masks at rand_counter), m = D round + k.
//   finals    E_m(r), lookup_outputs(r): degree t, opened from parties 0..t, unmasked; flags(r) public.
//   grouped   senders' contexts on one device and shamir_gp_grouped (COZK_SHAMIR_GP_GROUP=0 switches it off, read on every prove): ONE
//             cozk_primary_group on sender 0's context: a level call per exchange, a grouped finish per round.  Otherwise per sender
//             cozk_primary_level, cozk_shamir_scatter of its level buffer to the senders (the dealing launch + peer copies), per
//             receiver cozk_shamir_combine_vec, copied into its level buffer.  Same keys, counters and positions: same bytes.
//
// The KING construct (cozk_shamir_primary_prep + cozk_shamir_primary_prove_king; tests/shamir_primary_king_ref.py) moves everything that
// needs fresh randomness in front of the witness.  Which (index, instruction) items are live in a round depends on the public flags
// alone, so the sizes of all exchanges are known beforehand (cozk_primary_plan) and ONE double-random pair of their sum serves them,
// exchange e at the element offset = the sum of the earlier exchanges' n_elems:
//   prep      (A) the M opening masks at rand_counter, pair 0 -- the masks prove deals; (B) one cozk_shamir_rand_inproc-rule dealing of
//             `total` elements at rand_counter + M, pair 0 only, both halves for parties 0..2t only (receivers are the senders).
//   exchange  sender m sends z_m + r_2t,m[off + pos] to the king, who opens zed = slot + r with lagrange(1..2t + 1); receiver q keeps
//             zed - r_t,q[off + pos].  Grouped: one cozk_primary_group_level_king on a keyless group.  Otherwise cozk_primary_level per
//             sender, cozk_vec_binop adds the r_2t slice, the king's context runs cozk_shamir_king_finish for the senders of its device
//             and each result is copied into that sender's level buffer; a sender on another device gets zed by peer copy and
//             subtracts its slice on its own stream.  Same values, same offsets: same bytes.
//   check     before a level launches anything its size is compared with the plan's (a bound flag that is zero would change it).
// Transcript, masks, openings, finals and verifier are those of the resharing prover: the same proof bytes.
// Semi-honest.  Not built: the other n - t - 1 pairs of the prep's dealing (one pair is extracted: `total` elements are dealt per
// party for `total` pair elements), one party per process, groups over several GPUs, one item list shared by the senders, worker
// sub-nets (log_workers), the primary inside a chained Shamir flow.
#pragma once

// msgs: [D round + k][p <= 2t]; finals: E_0 .. E_{n_mem - 1}, lookup_outputs
struct cozk_shamir_primary : cozk::ShamirHarness {
    cozk_shamir_primary_config cfg;
    cozk_lookups inst;  // the lookups harness's instance of (seed, log_n, n_pairs = n_mem, mix) and the verifier's view; it has no parties here
    std::vector<cozk::HarnessParty> parties;
    std::vector<std::vector<cozk::VecH>> flags;  // [p <= 2t][instruction]: the public 0/1 columns on the sender's context
    std::vector<std::vector<cozk::PolyH>> E;     // [p <= 2t][m]: the sender's share of E_m, PLAIN
    std::vector<cozk::PolyH> outputs;            // [p <= 2t]
    std::vector<std::vector<uint8_t>> mul_keys;  // [p][t]: the keys of sender p's re-deals
    // what cozk_shamir_primary_prep made, consumed by cozk_shamir_primary_prove_king
    struct Prep {
        bool made = false, used = false;
        std::vector<uint64_t> plan;  // [round][COZK_PRIMARY_MAX_LEVELS]: cozk_primary_plan
        uint64_t total = 0, n_exchanges = 0;
        double t_offline_ms = 0;
        std::vector<std::vector<fe>> zero;  // [p <= 2t][m < M]
        std::vector<cozk_vec*> rt, r2t;     // [p <= 2t]: the halves of the exchanges' pair, `total` elements each
    } prep;
};

namespace {

typedef Handle<cozk_primary_group, cozk_primary_group_free> PrimaryGroupH;

// frees the pair of a prep: every vector with its party's device current
static void shamir_primary_release_pairs(cozk_shamir_primary* h) {
    for (size_t p = 0; p < h->prep.rt.size(); p++) {
        (void)hipSetDevice(h->pcs[p]->device);
        cozk_vec_free(h->prep.rt[p]);
        cozk_vec_free(h->prep.r2t[p]);
    }
    h->prep.rt.clear();
    h->prep.r2t.clear();
}

static cozk_vec shamir_primary_view(cozk_ctx* c, const void* d, size_t n) {
    cozk_vec v{};
    v.ctx = c;
    v.n = n;
    v.kind = COZK_SCALAR_FR;
    v.d = const_cast<void*>(d);
    v.bytes = n * sizeof(fe);
    v.owned = false;
    return v;
}

// One king exchange composed of the existing calls: buf[p] = sender p's level buffer holding its n_el unmasked slot values, replaced by
// its share of the reduced sharing.  Pair elements off .. off + n_el.
static void shamir_primary_king_exchange(const ShamirProve& sp, cozk_shamir_primary* h, const std::vector<const void*>& buf, size_t n_el, size_t off,
                                         int king) {
    const int t = sp.t, senders = sp.senders;
    const std::vector<cozk_ctx*>& pcs = sp.pcs;
    cozk_ctx* const kc = pcs[(size_t)king];
    const size_t bytes = n_el * sizeof(fe);
    std::vector<VecH> masked((size_t)senders);  // m_p = z_p + r_2t,p on the king's device
    for (int p = 0; p < senders; p++) {
        cozk_ctx* c = pcs[(size_t)p];
        sp.set_dev(p);
        const cozk_vec zv = shamir_primary_view(c, buf[(size_t)p], n_el), rv = shamir_primary_view(c, (const fe*)h->prep.r2t[(size_t)p]->d + off, n_el);
        cozk_vec* m = nullptr;
        rc_check(cozk_vec_alloc(c, n_el, COZK_SCALAR_FR, &m), c, "vec_alloc");
        VecH mh(m);
        rc_check(cozk_vec_binop(c, COZK_OP_ADD, 0, &zv, &rv, m), c, "vec_binop(mask)");
        if (c->device == kc->device) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            masked[(size_t)p] = std::move(mh);
            continue;
        }
        cozk_vec* km = nullptr;
        sp.set_dev(king);
        rc_check(cozk_vec_alloc(kc, n_el, COZK_SCALAR_FR, &km), kc, "vec_alloc");
        masked[(size_t)p] = VecH(km);
        sp.set_dev(p);
        HIP_TRY(hipMemcpyPeerAsync(km->d, kc->device, m->d, c->device, bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // the king opens zed and unmasks for the senders of its device in one launch; zed itself is kept only for senders elsewhere
    std::vector<int> local, remote;
    for (int q = 0; q < senders; q++) (pcs[(size_t)q]->device == kc->device ? local : remote).push_back(q);
    std::vector<const cozk_vec*> mv, rt;
    for (int p = 0; p < senders; p++) mv.push_back(masked[(size_t)p].h);
    for (int q : local) rt.push_back(h->prep.rt[(size_t)q]);
    sp.set_dev(king);
    std::vector<cozk_vec*> out(local.size(), nullptr);
    cozk_vec* z = nullptr;
    if (!local.empty()) {
        rc_check(cozk_shamir_king_finish(kc, mv.data(), t, rt.data(), off, (int)local.size(), out.data(), remote.empty() ? nullptr : &z), kc, "shamir_king_finish(level)");
    } else {  // the king shares its device with no sender: the open alone
        std::vector<uint32_t> pts((size_t)senders);
        for (int p = 0; p < senders; p++) pts[(size_t)p] = (uint32_t)p + 1;
        rc_check(cozk_shamir_combine_vec(kc, mv.data(), pts.data(), (size_t)senders, 2 * t, &z), kc, "shamir_combine_vec(level)");
    }
    VecH zh(z);
    std::vector<VecH> outs;
    for (cozk_vec* o : out) outs.emplace_back(o);
    for (size_t i = 0; i < local.size(); i++)
        HIP_TRY(hipMemcpyAsync(const_cast<void*>(buf[(size_t)local[i]]), cozk_vec_device_ptr(outs[i].h), bytes, hipMemcpyDeviceToDevice, kc->stream));
    HIP_TRY(hipStreamSynchronize(kc->stream));
    for (int q : remote) {
        cozk_ctx* c = pcs[(size_t)q];
        cozk_vec* zq = nullptr;
        sp.set_dev(q);
        rc_check(cozk_vec_alloc(c, n_el, COZK_SCALAR_FR, &zq), c, "vec_alloc");
        VecH zqh(zq);
        sp.set_dev(king);
        HIP_TRY(hipMemcpyPeerAsync(zq->d, c->device, z->d, kc->device, bytes, kc->stream));
        HIP_TRY(hipStreamSynchronize(kc->stream));
        sp.set_dev(q);
        const cozk_vec rv = shamir_primary_view(c, (const fe*)h->prep.rt[(size_t)q]->d + off, n_el);
        cozk_vec ov = shamir_primary_view(c, buf[(size_t)q], n_el);
        rc_check(cozk_vec_binop(c, COZK_OP_SUB, 0, zq, &rv, &ov), c, "vec_binop(unmask)");
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    sp.set_dev(king);  // the king's vectors go back to the king's pool
    masked.clear();
    outs.clear();
    zh = VecH();
}

// king < 0: the resharing construct; otherwise the king construct on the prep's pair
static void shamir_primary_prove(cozk_shamir_primary* h, bool verify, cozk_shamir_primary_result* res, int king = -1) {
    const bool kingly = king >= 0;
    ShamirProve sp(h, verify);
    const int t = sp.t, senders = sp.senders, openers = sp.openers, log_n = h->cfg.log_n;
    const size_t n_mem = (size_t)h->cfg.n_mem, n_instr = h->inst.instrs.size();
    const std::vector<cozk_ctx*>& pcs = sp.pcs;
    cozk_ctx* const c0 = sp.c0;
    const bool grouped = sp.grouped;
    auto set_dev = [&](int p) { sp.set_dev(p); };
    PrimarySumcheckProof pf;
    sp.sync_all();
    const double t0 = now_ms();
    Transcript tr("cozk-lookups");
    const std::vector<fe> r_eq = tr.challenge_vector((size_t)log_n);
    // ---- a PLAIN cozk_primary per sender over its shares
    std::vector<PrimaryH> prims((size_t)senders);
    {
        const std::vector<uint64_t> w = to_abi(r_eq);
        for (int p = 0; p < senders; p++) {
            cozk_ctx* c = pcs[(size_t)p];
            set_dev(p);
            VecH eq;
            rc_check(cozk_eq_evals(c, w.data(), log_n, &eq.h), c, "eq_evals");
            std::vector<const cozk_vec*> fl;
            for (const VecH& f : h->flags[(size_t)p]) fl.push_back(f.h);
            std::vector<const cozk_poly*> Ep;
            for (const PolyH& e : h->E[(size_t)p]) Ep.push_back(e.h);
            rc_check(cozk_primary_create(c, COZK_MODE_PLAIN, 0, h->inst.instrs.data(), n_instr, fl.data(), Ep.data(), n_mem, h->outputs[(size_t)p].h, eq.h,
                                         &prims[(size_t)p].h),
                     c, "primary_create");
        }
    }
    const int D = cozk_primary_degree(prims[0].h);
    sp.sync_all();
    const double t1 = now_ms();
    // ---- masks
    const size_t M = (size_t)D * (size_t)log_n;
    if (kingly) {
        COZK_REQUIRE(h->prep.zero.size() == (size_t)senders && h->prep.zero[0].size() == M, "shamir_primary_prove_king: the preprocessing holds other masks");
        sp.zero = h->prep.zero;
    } else {
        sp.deal_masks(h->cfg.rand_counter, M);
    }
    const double t2 = now_ms();
    // ---- rounds
    PrimaryGroupH g;
    if (grouped) {
        std::vector<cozk_primary*> members;
        std::vector<uint8_t> keys;
        for (int p = 0; p < senders; p++) {
            members.push_back(prims[(size_t)p].h);
            keys.insert(keys.end(), h->mul_keys[(size_t)p].begin(), h->mul_keys[(size_t)p].end());
        }
        set_dev(0);
        if (kingly) rc_check(cozk_primary_group_create_king(c0, members.data(), senders, &g.h), c0, "primary_group_create_king");
        else rc_check(cozk_primary_group_create(c0, members.data(), senders, keys.data(), &g.h), c0, "primary_group_create");
    }
    std::vector<const cozk_vec*> k_rt(h->prep.rt.begin(), h->prep.rt.end()), k_r2t(h->prep.r2t.begin(), h->prep.r2t.end());
    std::vector<uint32_t> pts((size_t)senders);
    for (int p = 0; p < senders; p++) pts[(size_t)p] = (uint32_t)p + 1;
    uint64_t ctr = h->cfg.mul_counter, rr[4];
    uint64_t n_exchanged = 0, n_exchanges = 0;
    fe claim = Fr::zero();
    std::vector<fe> rs;
    for (int round = 0; round < log_n; round++) {
        size_t n_items = 0;
        int n_levels = 0;
        for (int p = 0; p < senders; p++) {
            size_t ni = 0;
            int nl = 0;
            set_dev(p);
            rc_check(cozk_primary_round_begin(pcs[(size_t)p], prims[(size_t)p].h, round ? rr : nullptr, &ni, &nl), pcs[(size_t)p], "primary_round_begin");
            if (p == 0) {
                n_items = ni;
                n_levels = nl;
            }
            COZK_REQUIRE(ni == n_items && nl == n_levels, "shamir_primary: the senders' item lists differ (the flags are public)");
        }
        for (int level = 1; level <= n_levels; level++) {
            size_t n_el = 0;
            if (kingly) {  // the plan, before the level launches anything: exchange e lives at the offset the earlier ones' sizes give
                const uint64_t have = cozk_primary_level_elems(prims[0].h, level), want = h->prep.plan[(size_t)COZK_PRIMARY_MAX_LEVELS * round + level - 1];
                COZK_REQUIRE(have == want && n_exchanged + have <= h->prep.total,
                             "shamir_primary_prove_king: round " + std::to_string(round) + " level " + std::to_string(level) + " holds " + std::to_string(have) +
                                 " elements, the plan says " + std::to_string(want) + " (a bound flag is zero?)");
            }
            if (grouped && kingly) {
                set_dev(0);
                rc_check(cozk_primary_group_level_king(g.h, level, k_rt.data(), k_r2t.data(), (size_t)n_exchanged, &n_el), c0, "primary_group_level_king");
                if (n_el) h->stats.group_rounds++;
            } else if (grouped) {
                set_dev(0);
                rc_check(cozk_primary_group_level(g.h, level, ctr, &n_el), c0, "primary_group_level");
                if (n_el) h->stats.group_rounds++;
            } else {
                std::vector<const void*> buf((size_t)senders, nullptr);
                for (int p = 0; p < senders; p++) {
                    size_t ne = 0;
                    set_dev(p);
                    rc_check(cozk_primary_level(pcs[(size_t)p], prims[(size_t)p].h, level, nullptr, nullptr, 0, &buf[(size_t)p], nullptr, &ne), pcs[(size_t)p],
                             "primary_level");
                    h->stats.single_rounds++;
                    if (p == 0) n_el = ne;
                    COZK_REQUIRE(ne == n_el, "shamir_primary: the senders' level sizes differ (the flags are public)");
                }
                if (n_el && kingly) {
                    shamir_primary_king_exchange(sp, h, buf, n_el, (size_t)n_exchanged, king);
                } else if (n_el) {
                    // the degree reduction, composed: every sender deals its level buffer to the senders, every sender combines
                    std::vector<std::vector<VecH>> dealt((size_t)senders);  // [dealer][receiver], the receiver's vector
                    for (int m = 0; m < senders; m++) {
                        cozk_vec view{};
                        view.ctx = pcs[(size_t)m];
                        view.n = n_el;
                        view.kind = COZK_SCALAR_FR;
                        view.d = const_cast<void*>(buf[(size_t)m]);
                        view.bytes = n_el * sizeof(fe);
                        view.owned = false;
                        std::vector<cozk_vec*> out((size_t)senders, nullptr);
                        set_dev(m);
                        rc_check(cozk_shamir_scatter(pcs[(size_t)m], &view, h->mul_keys[(size_t)m].data(), t, senders, ctr, pcs.data(), out.data()), pcs[(size_t)m],
                                 "shamir_scatter(level)");
                        for (int q = 0; q < senders; q++) dealt[(size_t)m].emplace_back(out[(size_t)q]);
                    }
                    for (int q = 0; q < senders; q++) {
                        cozk_ctx* c = pcs[(size_t)q];
                        std::vector<const cozk_vec*> recv;
                        for (int m = 0; m < senders; m++) recv.push_back(dealt[(size_t)m][(size_t)q].h);
                        VecH comb;
                        set_dev(q);
                        rc_check(cozk_shamir_combine_vec(c, recv.data(), pts.data(), (size_t)senders, 2 * t, &comb.h), c, "shamir_combine_vec(level)");
                        HIP_TRY(hipMemcpyAsync(const_cast<void*>(buf[(size_t)q]), cozk_vec_device_ptr(comb.h), n_el * sizeof(fe), hipMemcpyDeviceToDevice, c->stream));
                        HIP_TRY(hipStreamSynchronize(c->stream));
                    }
                    for (int q = 0; q < senders; q++) {
                        set_dev(q);  // a receiver's vectors go back to the receiver's pool
                        for (int m = 0; m < senders; m++) dealt[(size_t)m][(size_t)q] = VecH();
                    }
                }
            }
            if (n_el) {  // n_el == 0: nothing to exchange at this level (public knowledge): the counter stays
                ctr += n_el;
                n_exchanged += n_el;
                n_exchanges++;
            }
        }
        std::vector<uint64_t> ev((size_t)4 * D * senders);
        if (grouped) {
            set_dev(0);
            rc_check(cozk_primary_group_round_finish(g.h, ev.data()), c0, "primary_group_round_finish");
            h->stats.group_rounds++;
        } else {
            for (int p = 0; p < senders; p++) {
                set_dev(p);
                rc_check(cozk_primary_round_finish(pcs[(size_t)p], prims[(size_t)p].h, ev.data() + (size_t)4 * D * p), pcs[(size_t)p], "primary_round_finish");
                h->stats.single_rounds++;
            }
        }
        std::vector<fe> opened((size_t)D);
        for (int k = 0; k < D; k++) opened[(size_t)k] = sp.open_2t(ev.data() + 4 * k, (size_t)4 * D, (size_t)(D * round + k));
        const fe r_j = primary_coordinator_round(opened, claim, tr, pf);
        rs.push_back(r_j);
        fe_to_u64x4(r_j, rr);
    }
    g = PrimaryGroupH();
    sp.sync_all();
    if (kingly) shamir_primary_release_pairs(h);  // consumed: every stream has drained behind the last exchange
    const double t3 = now_ms();
    // ---- the final claims: E(r) and lookup_outputs(r) from the openers, flags(r) public
    {
        std::vector<std::vector<uint64_t>> Ee((size_t)openers, std::vector<uint64_t>(8 * n_mem)), oe((size_t)openers, std::vector<uint64_t>(8));
        std::vector<uint64_t> Fe(4 * n_instr), scratch(4 * n_instr);
        for (int p = 0; p < openers; p++) {
            uint64_t qe[4];
            set_dev(p);
            rc_check(cozk_primary_final_evals(pcs[(size_t)p], prims[(size_t)p].h, rr, Ee[(size_t)p].data(), p ? scratch.data() : Fe.data(), oe[(size_t)p].data(), qe),
                     pcs[(size_t)p], "primary_final_evals");
        }
        const size_t tamper = h->cfg.tamper_final > 0 ? (size_t)h->cfg.tamper_final - 1 : (size_t)-1;
        auto open_t = [&](fe* sh) {  // tamper_final: one opener's share of one value is off by one, in `finals` and in the opening
            for (int p = 0; p < openers; p++)
                if (h->finals.size() + (size_t)p == tamper) sh[p] = Fr::add(sh[p], Fr::one());
            return sp.open_t(sh);
        };
        for (size_t m = 0; m <= n_mem; m++) {
            fe sh[COZK_SHAMIR_MAX_PARTIES];
            for (int p = 0; p < openers; p++) sh[p] = fe_from_u64x4(m < n_mem ? Ee[(size_t)p].data() + 8 * m : oe[(size_t)p].data());
            const fe v = open_t(sh);
            if (m < n_mem) pf.openings.push_back(v);
            else {
                for (size_t i = 0; i < n_instr; i++) pf.openings.push_back(fe_from_u64x4(Fe.data() + 4 * i));
                pf.openings.push_back(v);
            }
        }
        tr.append_scalars(pf.openings);
    }
    sp.release(prims);
    sp.sync_all();
    const double t4 = now_ms();
    res->verified = -1;
    if (verify) {
        std::string why;
        bool ok = true;
        Transcript vt("cozk-lookups");
        const std::vector<fe> vr_eq = vt.challenge_vector((size_t)log_n);
        std::vector<fe> vrs;
        if (!verify_primary_sumcheck(pf, h->inst.instrs, n_mem, primary_sumcheck_degree(h->inst.instrs), vr_eq, vt, vrs)) {
            ok = false;
            why = "primary sumcheck: a round or the final claim does not hold";
        } else {
            // the opened evaluations against the dealer's clear columns (stand-in for the PCS opening), as the lookups harness checks them
            cozk_lookups& in = h->inst;
            if (!in.vctx) {
                int rc = cozk_ctx_create(h->cfg.devices[0], &in.vctx);
                if (rc != COZK_OK) throw CozkError(rc, "shamir_primary: cannot create the verifier's context");
                HIP_TRY(hipSetDevice(in.vctx->device));
                lookups_setup_primary_verifier(&in);
            }
            HIP_TRY(hipSetDevice(in.vctx->device));
            const std::vector<fe> pt(vrs.rbegin(), vrs.rend());
            const std::vector<uint64_t> w = to_abi(pt);
            VecH chi;
            rc_check(cozk_eq_evals(in.vctx, w.data(), (int)pt.size(), &chi.h), in.vctx, "eq_evals");
            std::vector<const cozk_poly*> ps;
            for (auto& e : in.v_E) ps.push_back(e.h);
            for (auto& f : in.v_iflags) ps.push_back(f.h);
            ps.push_back(in.v_outputs.h);
            std::vector<uint64_t> out(4 * ps.size());
            rc_check(cozk_poly_batch_evaluate_at_chi(in.vctx, ps.data(), ps.size(), chi.h, out.data()), in.vctx, "batch_evaluate");
            for (size_t i = 0; i < ps.size() && ok; i++)
                if (!Fr::eq(fe_from_u64x4(out.data() + 4 * i), pf.openings[i])) {
                    ok = false;
                    why = "primary sumcheck: opening " + std::to_string(i) + " != polynomial(r)";
                }
        }
        res->verified = ok ? 1 : 0;
        if (!ok) h->error = "verification failed: " + why;
    }
    res->grouped = grouped ? 1 : 0;
    res->degree = D;
    res->n_opened = M;
    res->n_exchanges = n_exchanges;
    res->n_exchanged = n_exchanged;
    res->wall_ms = t4 - t0;
    res->t_build_ms = t1 - t0;
    res->t_masks_ms = t2 - t1;
    res->t_rounds_ms = t3 - t2;
    res->t_finals_ms = t4 - t3;
    Writer w;
    pf.write(w);
    finish_proof(h, w.b, res);
}

// create went through
static bool shamir_primary_built(const cozk_shamir_primary* x) {
    return x->E.size() == (size_t)(2 * x->t + 1) && x->E.back().size() == (size_t)x->cfg.n_mem && x->outputs.back().h != nullptr;
}

// The preprocessing of one king prove: the plan from the public flags, (A) the opening masks, (B) the exchanges' pair.  Refused on a
// handle that has been preprocessed: (rand_keys, rand_counter .. rand_counter + M + total) must never be used again.
static void shamir_primary_prep(cozk_shamir_primary* h) {
    const int t = h->t, n = h->n, senders = 2 * t + 1, log_n = h->cfg.log_n;
    const std::vector<cozk_ctx*>& pcs = h->pcs;
    COZK_REQUIRE(!h->prep.made, "shamir_primary_prep: the harness has been preprocessed (its key and counter range must never be used again)");
    const ShamirGpArgs a{pcs.data(), nullptr, 0, t, n, nullptr, false};
    cozk_shamir_primary::Prep pr;
    shamir_gp_sync_all(a);
    const double t0 = now_ms();
    HIP_TRY(hipSetDevice(pcs[0]->device));
    std::vector<const cozk_vec*> fl;
    for (const VecH& f : h->flags[0]) fl.push_back(f.h);
    pr.plan.assign((size_t)COZK_PRIMARY_MAX_LEVELS * log_n, 0);
    rc_check(cozk_primary_plan(pcs[0], h->inst.instrs.data(), h->inst.instrs.size(), fl.data(), log_n, pr.plan.data(), &pr.total), pcs[0], "primary_plan");
    for (uint64_t e : pr.plan) pr.n_exchanges += e ? 1 : 0;
    const size_t M = (size_t)primary_sumcheck_degree(h->inst.instrs) * (size_t)log_n;
    std::vector<const uint8_t*> rk((size_t)n);
    for (int p = 0; p < n; p++) rk[(size_t)p] = h->rand_keys[(size_t)p].data();
    pr.zero = shamir_gp_zero_masks(a, rk.data(), h->cfg.rand_counter, M);
    if (pr.total) {
        pr.rt.assign((size_t)senders, nullptr);
        pr.r2t.assign((size_t)senders, nullptr);
        rc_check(shamir_rand_pairs_inproc(pcs.data(), rk.data(), (size_t)pr.total, t, n, h->cfg.rand_counter + M, 1, senders, pr.rt.data(), pr.r2t.data()), pcs[0],
                 "shamir_rand_pairs_inproc");
    }
    shamir_gp_sync_all(a);
    pr.t_offline_ms = now_ms() - t0;
    pr.made = true;
    h->prep = std::move(pr);
}

static void shamir_primary_release(cozk_shamir_primary* h) {
    shamir_primary_release_pairs(h);
    for (size_t p = 0; p < h->parties.size(); p++) {
        if (h->parties[p].ctx) (void)hipSetDevice(h->parties[p].ctx->device);
        if (p < h->flags.size()) h->flags[p].clear();
        if (p < h->E.size()) h->E[p].clear();
        if (p < h->outputs.size()) h->outputs[p] = PolyH();
    }
    release_parties(h->parties, [](HarnessParty&) {});
    if (h->inst.vctx) {
        (void)hipSetDevice(h->inst.vctx->device);
        h->inst.v_E.clear();
        h->inst.v_iflags.clear();
        h->inst.v_outputs = PolyH();
        cozk_ctx_destroy(h->inst.vctx);
        h->inst.vctx = nullptr;
    }
}

}  // namespace

extern "C" {

int cozk_shamir_primary_create(const cozk_shamir_primary_config* cfg, cozk_shamir_primary** out) {
    return harness_create(cfg, out, [&](cozk_shamir_primary* h) {
        const std::string w = "shamir_primary";
        shamir_gp_require_parties(w, cfg->degree, cfg->num_parties);
        COZK_REQUIRE(cfg->log_n >= 1 && cfg->log_n <= 24, w + ": log_n out of range (1..24)");
        COZK_REQUIRE(cfg->n_mem >= 1 && cfg->n_mem <= 128, w + ": n_mem out of range (1..128)");
        COZK_REQUIRE(cfg->mix == 0 || cfg->mix == 1, w + ": mix is 0 (uniform) or 1 (sha2-shaped)");
        const int t = h->t = cfg->degree, n = h->n = cfg->num_parties, senders = 2 * t + 1;
        // the lookups harness's own instance
        cozk_lookups& in = h->inst;
        memset(&in.cfg, 0, sizeof in.cfg);
        in.cfg.mode = COZK_MODE_PLAIN;
        in.cfg.log_n = cfg->log_n;
        in.cfg.n_pairs = cfg->n_mem;
        in.cfg.devices[0] = cfg->devices[0];
        in.cfg.seed = cfg->seed;
        in.cfg.primary = 1;
        in.cfg.mix = cfg->mix;
        in.N = (size_t)1 << cfg->log_n;
        lookups_setup_primary_clear(&in);
        const size_t N = in.N;
        h->parties.resize((size_t)n);
        for (int p = 0; p < n; p++) {
            h->parties[(size_t)p].party = p;
            h->parties[(size_t)p].open_ctx(cfg->devices[p], "shamir_primary: cannot create a context (no HIP device?)");
            h->pcs.push_back(h->parties[(size_t)p].ctx);
        }
        const std::vector<cozk_ctx*>& pcs = h->pcs;
        const std::vector<uint8_t> skeys = shamir_harness_keys(h, cfg->seed);
        h->mul_keys.assign((size_t)n, std::vector<uint8_t>((size_t)t * COZK_PRF_KEY_BYTES));
        for (int p = 0; p < n; p++)
            for (int c = 0; c < t; c++)
                harness_prf_key(cfg->seed ^ 0x4D554C54ull, (uint64_t)(64 * p + c), h->mul_keys[(size_t)p].data() + (size_t)c * COZK_PRF_KEY_BYTES);
        // the public flags, on every sender's context
        h->flags.resize((size_t)senders);
        h->E.resize((size_t)senders);
        h->outputs.resize((size_t)senders);
        {
            std::vector<uint8_t> col(N);
            for (size_t i = 0; i < in.instrs.size(); i++) {
                for (size_t x = 0; x < N; x++) col[x] = in.which[x] == i ? 1 : 0;
                for (int p = 0; p < senders; p++) {
                    HIP_TRY(hipSetDevice(pcs[(size_t)p]->device));
                    h->flags[(size_t)p].push_back(upload_vec(pcs[(size_t)p], col.data(), N, COZK_SCALAR_U8, "vec_upload(instruction flags)"));
                }
            }
        }
        // the witness: E_m = column m, lookup_outputs = column n_mem, dealt once each; a party above 2t runs no program and drops its share
        for (int v = 0; v <= cfg->n_mem; v++) {
            HIP_TRY(hipSetDevice(pcs[0]->device));
            VecH cv = v < cfg->n_mem ? make_vec_random(pcs[0], N, COZK_SCALAR_FR, cfg->seed + 9000ull * (uint64_t)(v + 1), 0)
                                     : upload_vec(pcs[0], in.outputs_plain.data(), N, COZK_SCALAR_FR, "vec_upload(outputs)");
            std::vector<PolyH> dealt = shamir_deal_column(h, cv, skeys, cfg->share_counter + (uint64_t)v * (uint64_t)N, senders);
            for (int p = 0; p < senders; p++) {
                if (v < cfg->n_mem) h->E[(size_t)p].push_back(std::move(dealt[(size_t)p]));
                else h->outputs[(size_t)p] = std::move(dealt[(size_t)p]);
            }
        }
    });
}

const char* cozk_shamir_primary_error(const cozk_shamir_primary* h) { return harness_error(h); }

int cozk_shamir_primary_destroy(cozk_shamir_primary* h) {
    if (!h) return COZK_OK;
    shamir_primary_release(h);
    delete h;
    return COZK_OK;
}

int cozk_shamir_primary_prove(cozk_shamir_primary* h, int verify, cozk_shamir_primary_result* res) {
    return shamir_harness_prove(h, res, "shamir_primary", shamir_primary_built,
                                [&](cozk_shamir_primary* x, cozk_shamir_primary_result* r) { shamir_primary_prove(x, verify != 0, r); });
}

int cozk_shamir_primary_prep_get_result(const cozk_shamir_primary* h, cozk_shamir_primary_prep_result* res) {
    if (!h || !res) return COZK_ERR_INVALID_ARG;
    memset(res, 0, sizeof *res);
    if (!h->prep.made) return COZK_OK;
    res->n_openings = h->prep.zero.empty() ? 0 : h->prep.zero[0].size();
    res->pair_elems = h->prep.total;
    res->n_exchanges = h->prep.n_exchanges;
    res->used = h->prep.used ? 1 : 0;
    res->t_offline_ms = h->prep.t_offline_ms;
    return COZK_OK;
}

int cozk_shamir_primary_prep(cozk_shamir_primary* h, cozk_shamir_primary_prep_result* res) {
    if (!h || !res) return COZK_ERR_INVALID_ARG;
    memset(res, 0, sizeof *res);
    if (h->n == 0 || h->pcs.size() != (size_t)h->n || !shamir_primary_built(h)) {
        h->error = "shamir_primary_prep: the harness was not built";
        return COZK_ERR_INVALID_ARG;
    }
    h->error.clear();
    try {
        shamir_primary_prep(h);
    } catch (const CozkError& e) {
        h->error = e.what();
        for (cozk_ctx* c : h->pcs) (void)hipStreamSynchronize(c->stream);
        return e.code;
    } catch (const std::exception& e) {
        h->error = e.what();
        return COZK_ERR_INTERNAL;
    }
    return cozk_shamir_primary_prep_get_result(h, res);
}

int cozk_shamir_primary_prove_king(cozk_shamir_primary* h, int king, int verify, cozk_shamir_primary_result* res) {
    return shamir_harness_prove(h, res, "shamir_primary_king", shamir_primary_built, [&](cozk_shamir_primary* x, cozk_shamir_primary_result* r) {
        // everything is refused before the first launch; the prep is marked used before it
        COZK_REQUIRE(king >= 0 && king < x->n, "shamir_primary_prove_king: 0 <= king < num_parties");
        COZK_REQUIRE(x->prep.made, "shamir_primary_prove_king: no preprocessing (cozk_shamir_primary_prep)");
        COZK_REQUIRE(!x->prep.used, "shamir_primary_prove_king: the preprocessing has been used (a pair must never be used twice)");
        x->prep.used = true;
        shamir_primary_prove(x, verify != 0, r, king);
    });
}

int cozk_shamir_primary_proof_bytes(const cozk_shamir_primary* h, uint8_t* out, size_t cap) { return harness_proof_bytes(h, out, cap); }

size_t cozk_shamir_primary_msgs_len(const cozk_shamir_primary* h) { return h ? h->msgs.size() : 0; }
size_t cozk_shamir_primary_finals_len(const cozk_shamir_primary* h) { return h ? h->finals.size() : 0; }

int cozk_shamir_primary_msgs(const cozk_shamir_primary* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->msgs : nullptr, out, cap); }
int cozk_shamir_primary_finals(const cozk_shamir_primary* h, uint64_t* out, size_t cap) { return fe_copy_out(h ? &h->finals : nullptr, out, cap); }
int cozk_shamir_primary_get_stats(const cozk_shamir_primary* h, cozk_shamir_gp_stats* stats) { return shamir_harness_stats(h, stats); }

}  // extern "C"
