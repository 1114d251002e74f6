// What every in-process harness shares: the party and handle bases, the in-process channels of one proof, the runner that
// drives the participants on threads of their own and the coordinator on the calling thread, and the create / error /
// proof-bytes plumbing of the C ABI.  Included by harness.hip ahead of the harnesses.
#pragma once
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>

#include "net.hpp"

namespace cozk {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// one participant of an in-process harness: its context, its net counters of the last prove, its error of the last prove
struct HarnessParty {
    cozk_ctx* ctx = nullptr;
    bool own_ctx = false;
    int party = 0;
    uint64_t star_up = 0, star_down = 0, star_msgs = 0, ring_bytes = 0;
    std::string error;
    // a context of its own on `device`, current on this thread
    void open_ctx(int device, const char* fail_msg) {
        int rc = cozk_ctx_create(device, &ctx);
        if (rc != COZK_OK) throw CozkError(rc, fail_msg);
        own_ctx = true;
        HIP_TRY(hipSetDevice(ctx->device));
    }
    void record_net(const StarNetWorker* star, const RingNet* ring = nullptr) {
        star_up = star->bytes_up;
        star_down = star->bytes_down;
        star_msgs = star->n_msgs;
        ring_bytes = ring ? ring->bytes_sent : 0;
    }
};

// destroy time: release(party) frees the party's device handles with its device current, then its context goes
template <class P, class F>
void release_parties(std::vector<P>& parties, F release) {
    for (auto& ps : parties) {
        if (ps.ctx) (void)hipSetDevice(ps.ctx->device);
        release(ps);
        if (ps.own_ctx && ps.ctx) cozk_ctx_destroy(ps.ctx);
    }
}

template <class P>
cozk_ctx* party_ctx(std::vector<P>& parties, int party) {
    if (party < 0 || party >= (int)parties.size()) return nullptr;
    return parties[(size_t)party].ctx;
}

// the part of every harness handle the C ABI reads back
struct HarnessHandle {
    std::string error;
    Bytes last_proof;
};

// *_create: a new harness holding *cfg, then setup(h) validates and builds it.  On failure the harness is returned all the
// same: the caller reads its error, then destroys it
template <class H, class C, class F>
int harness_create(const C* cfg, H** out, F setup) {
    if (!cfg || !out) return COZK_ERR_INVALID_ARG;
    H* h = new H();
    h->cfg = *cfg;
    *out = h;
    try {
        setup(h);
    } catch (const CozkError& e) {
        h->error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        h->error = e.what();
        return COZK_ERR_INTERNAL;
    }
    return COZK_OK;
}

inline const char* harness_error(const HarnessHandle* h) { return h ? h->error.c_str() : "null harness"; }

inline int harness_proof_bytes(const HarnessHandle* h, uint8_t* out, size_t cap) {
    if (!h || !out || cap < h->last_proof.size()) return COZK_ERR_INVALID_ARG;
    memcpy(out, h->last_proof.data(), h->last_proof.size());
    return COZK_OK;
}

// the start of every prove: false on a null argument, else a zeroed result with verified = -1 (not verified)
template <class H, class R>
bool harness_prove_begin(const H* h, R* res) {
    if (!h || !res) return false;
    memset(res, 0, sizeof *res);
    res->verified = -1;
    return true;
}

// The plain verifier after a prove, outside its clock: f(why) -> bool runs with `device` current.  A refusal, or an exception in f,
// sets verified = 0 and leaves "verification failed: <why>" as the harness's error.
template <class R, class F>
void harness_verify(HarnessHandle* h, R* res, int device, F f) {
    std::string why;
    try {
        HIP_TRY(hipSetDevice(device));
        res->verified = f(why) ? 1 : 0;
    } catch (const std::exception& e) {
        why = e.what();
        res->verified = 0;
    }
    if (res->verified == 0) h->error = "verification failed: " + why;
}

// the end of every prove: keep the serialized proof for *_proof_bytes, report its length and SHA-256
template <class R>
void finish_proof(HarnessHandle* h, Bytes proof, R* res) {
    h->last_proof = std::move(proof);
    res->proof_len = h->last_proof.size();
    Sha256 s;
    s.update(h->last_proof.data(), h->last_proof.size());
    s.final(res->proof_digest);
}

// The in-process channels of one proof.  `star`: one worker end per participant.  ring3: participant p is party p % 3 of
// ring p / 3 (one ring per three consecutive participants).  n_sub > 0: a second star of n_sub ends (worker sub-nets,
// public workers).  Every channel aborts with star.abort.
struct InProcNets {
    InProcStar star;
    std::unique_ptr<InProcStar> sub;
    std::vector<std::unique_ptr<InProcRing>> rings;
    std::vector<std::unique_ptr<InProcStarWorker>> star_ends, sub_ends;
    std::vector<std::unique_ptr<InProcRingNet>> ring_ends;
    explicit InProcNets(int n, bool ring3 = false, int n_sub = 0) : star(n) {
        for (int p = 0; p < n; p++) {
            if (ring3 && p % 3 == 0) rings.emplace_back(new InProcRing(&star.abort));
            star_ends.emplace_back(new InProcStarWorker(&star, p));
            ring_ends.emplace_back(ring3 ? new InProcRingNet(rings.back().get(), p % 3) : nullptr);
        }
        if (n_sub <= 0) return;
        sub.reset(new InProcStar(n_sub));
        for (auto& c : sub->up) c.abort = &star.abort;
        for (auto& c : sub->down) c.abort = &star.abort;
        for (int i = 0; i < n_sub; i++) sub_ends.emplace_back(new InProcStarWorker(sub.get(), i));
    }
    StarNetWorker* worker(int p) { return star_ends[(size_t)p].get(); }
    RingNet* ring(int p) { return ring_ends[(size_t)p].get(); }
    StarNetWorker* sub_worker(int i) { return sub_ends[(size_t)i].get(); }
};

// one participant thread: body() runs it; a failure lands in ps->error as "<role> <index>: ..."
struct Participant {
    const char* role;
    int index;
    HarnessParty* ps;
    std::function<void()> body;
};

// every party of `parties` as a participant: body(party struct, index)
template <class P, class F>
void add_participants(std::vector<Participant>& out, const char* role, std::vector<P>& parties, F body) {
    for (int i = 0; i < (int)parties.size(); i++) {
        P* ps = &parties[(size_t)i];
        out.push_back(Participant{role, i, ps, [ps, i, body] { body(*ps, i); }});
    }
}

// One in-process proof over `nets`: every participant on a thread of its own, coordinator() on the calling thread.  An
// exception in any of them is recorded and aborts every channel, so that the others unblock.  After the joins `error` names
// the failure (a participant's over the coordinator's, the last participant's over earlier ones).  wall_ms spans the first
// thread start to the last join.  Returns COZK_OK or COZK_ERR_INTERNAL.
inline int run_in_process(InProcNets& nets, std::vector<Participant>& parts, const std::function<void()>& coordinator, std::string& error, double& wall_ms) {
    Abort& abort = nets.star.abort;
    for (auto& pt : parts) pt.ps->error.clear();
    std::vector<std::thread> threads;
    double t0 = now_ms();
    for (auto& pt : parts) {
        threads.emplace_back([&abort, &pt] {
            try {
                pt.body();
            } catch (const std::exception& e) {
                pt.ps->error = e.what();
                abort.flag.store(true);
            }
        });
    }
    int rc = COZK_OK;
    try {
        coordinator();
    } catch (const std::exception& e) {
        error = std::string("coordinator: ") + e.what();
        abort.flag.store(true);
        rc = COZK_ERR_INTERNAL;
    }
    for (auto& t : threads) t.join();
    wall_ms = now_ms() - t0;
    for (auto& pt : parts) {
        if (!pt.ps->error.empty()) {
            error = std::string(pt.role) + " " + std::to_string(pt.index) + ": " + pt.ps->error;
            rc = COZK_ERR_INTERNAL;
        }
    }
    return rc;
}

// One proof by party 0 alone over a star of one end: worker(party, its end) on a thread of its own, coordinate(net) on the calling
// thread; then res->wall_ms and, with `verify`, verifier(why) on the party's device, outside the clock.  Returns run_in_process's
// code, and on a failure leaves res as harness_prove_begin made it.
template <class P, class R, class W, class C, class V>
int prove_by_one_party(HarnessHandle* h, std::vector<P>& parties, int verify, R* res, W worker, C coordinate, V verifier) {
    InProcNets nets(1);
    std::vector<Participant> parts;
    add_participants(parts, "party", parties, [&](P& ps, int) { worker(ps, nets.worker(0)); });
    double wall_ms = 0;
    int rc = run_in_process(nets, parts, [&] {
        InProcStarCoordinator coord(&nets.star);
        coordinate(coord);
    }, h->error, wall_ms);
    if (rc != COZK_OK) return rc;
    res->wall_ms = wall_ms;
    if (verify) harness_verify(h, res, parties[0].ctx->device, verifier);
    return COZK_OK;
}

}  // namespace cozk
