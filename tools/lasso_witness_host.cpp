// The sequential walk of the Lasso lookup witness (co-jolt/src/jolt/vm/instruction_lookups/witness.rs:85-150) as a plain host loop, one
// thread per memory and at most `n_threads` at a time: what a dealer does without cozk_lasso_witness.  Built by
// tools/run_lasso_witness.py (g++ -O2 -shared -fPIC -pthread) as the baseline beside the device call, and as a full-size cross-check.
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

extern "C" int lasso_witness_host(const uint32_t* dims, size_t n, const uint32_t* subtables, size_t M, const uint8_t* flags, const int* mem_dim, const int* mem_subtable,
                                  size_t n_mem, int n_threads, uint32_t* read_cts, uint32_t* E, uint32_t* final_cts) {
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&] {
        for (size_t m = next++; m < n_mem; m = next++) {
            const uint32_t* addr = dims + (size_t)mem_dim[m] * n;
            const uint32_t* sub = subtables + (size_t)mem_subtable[m] * M;
            const uint8_t* fl = flags + m * n;
            uint32_t *rc = read_cts + m * n, *e = E + m * n, *fc = final_cts + m * M;
            memset(fc, 0, M * sizeof(uint32_t));
            for (size_t j = 0; j < n; j++) {
                if (!fl[j]) {
                    rc[j] = e[j] = 0;
                    continue;
                }
                const uint32_t a = addr[j];
                if (a >= M) {
                    bad = 1;
                    rc[j] = e[j] = 0;
                    continue;
                }
                rc[j] = fc[a]++;
                e[j] = sub[a];
            }
        }
    };
    std::vector<std::thread> ts;
    for (int t = 0; t < n_threads; t++) ts.emplace_back(work);
    for (auto& t : ts) t.join();
    return bad.load();
}
