// Stand-alone host program around the host tail of the dense layer rounds (co-zkvms_amd/csrc/host/layer_tail.hpp): no device code
// runs and no GPU is needed.  Built by co-zkvms_amd/build.py (build_host_program) and driven by tests/test_layer_tail_host.py.
//
//   layer_tail_check            cases on stdin, results on stdout (both binary, little-endian):
//       in : u64 ncases; per case u64 {NC, len, E1_len, E2_len, have_r, nrounds}, then Montgomery elements of 32 bytes:
//            layer a [len], layer b [len] (NC = 2), E1 [E1_len], E2 [E2_len], the pending challenge (have_r), nrounds challenges
//       out: per case nrounds x 3 sums g(0), g(2), g(3); 4 final claims; u64 {len, E1_len, E2_len, binds}; E1 [E1_len]; E2 [E2_len]
//   layer_tail_check --time-mul  nanoseconds per Fr::mul on this host, in a dependent chain and in four independent ones
#include <chrono>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../co-zkvms_amd/csrc/host/layer_tail.hpp"

static bool get(void* p, size_t bytes) { return fread(p, 1, bytes, stdin) == bytes; }
static void put(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }

template <int NC>
static bool run_case(const uint64_t h[6]) {
    const size_t len = h[1], E1_len = h[2], E2_len = h[3];
    const bool have_r = h[4] != 0;
    const int nrounds = (int)h[5];
    std::vector<fe> area(layer_tail_entries(NC, len, E1_len, E2_len) + 1), rs((size_t)nrounds + 1);
    fe r0 = Fr::zero();
    if (!get(area.data(), (area.size() - 1) * sizeof(fe))) return false;
    if (have_r && !get(&r0, sizeof(fe))) return false;
    if (nrounds && !get(rs.data(), (size_t)nrounds * sizeof(fe))) return false;
    LayerTailView t = layer_tail_view(area.data(), NC, len, E1_len, E2_len);
    fe fin[4];
    const int binds = layer_tail_rounds<NC>(
        t, have_r, r0, nrounds,
        [&](int j, const fe s[3]) {
            put(s, 3 * sizeof(fe));
            return rs[(size_t)j];
        },
        fin);
    put(fin, sizeof fin);
    const uint64_t shape[4] = {t.len, t.E1_len, t.E2_len, (uint64_t)binds};
    put(shape, sizeof shape);
    put(t.E1, t.E1_len * sizeof(fe));
    put(t.E2, t.E2_len * sizeof(fe));
    return true;
}

static int time_mul() {
    using clk = std::chrono::steady_clock;
    const int n = 4000000;
    fe x = Fr::from_u64(0x1234567u), y = Fr::from_u64(0x9e3779b9u);
    fe a = x, b = y, c = Fr::add(x, y), d = Fr::dbl(y);
    auto t0 = clk::now();
    for (int i = 0; i < n; i++) a = Fr::mul(a, y);
    auto t1 = clk::now();
    for (int i = 0; i < n / 4; i++) {
        a = Fr::mul(a, y);
        b = Fr::mul(b, y);
        c = Fr::mul(c, y);
        d = Fr::mul(d, y);
    }
    auto t2 = clk::now();
    const fe keep = Fr::add(Fr::add(a, b), Fr::add(c, d));
    printf("{\"fr_mul_dependent_ns\": %.1f, \"fr_mul_independent_ns\": %.1f, \"check\": %u}\n",
           std::chrono::duration<double, std::nano>(t1 - t0).count() / n, std::chrono::duration<double, std::nano>(t2 - t1).count() / n, keep.l[0] & 1u);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--time-mul")) return time_mul();
    uint64_t ncases = 0;
    if (!get(&ncases, sizeof ncases)) return 2;
    for (uint64_t k = 0; k < ncases; k++) {
        uint64_t h[6];
        if (!get(h, sizeof h)) return 2;
        if (h[0] != 1 && h[0] != 2) return 3;
        if (!(h[0] == 2 ? run_case<2>(h) : run_case<1>(h))) return 2;
    }
    return fflush(stdout) == 0 ? 0 : 4;
}
