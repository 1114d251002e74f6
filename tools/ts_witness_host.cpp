// The walk of the timestamp range-check witness (jolt-core's TimestampRangeCheckPolynomials::generate_witness) as a plain host loop:
// per slot two columns of Lasso counters over an identity table of M entries, key = t_read[s][j] and key = j - t_read[s][j].  One
// thread, as the dealer's walk is written.  What a dealer does without cozk_timestamp_range_witness.  Built by
// tools/run_ts_witness.py (g++ -O2 -shared -fPIC) as the baseline beside the device call, and as a full-size cross-check.
#include <cstddef>
#include <cstdint>
#include <cstring>

// Returns the number of steps with t_read[s][j] > j (those steps are skipped).
extern "C" size_t ts_witness_host(const uint32_t* const* t_read, size_t n_slots, size_t n, size_t M, uint32_t* const* rc_rt, uint32_t* const* rc_gmr,
                                  uint32_t* const* fc_rt, uint32_t* const* fc_gmr) {
    size_t bad = 0;
    for (size_t s = 0; s < n_slots; s++) {
        memset(fc_rt[s], 0, M * sizeof(uint32_t));
        memset(fc_gmr[s], 0, M * sizeof(uint32_t));
        for (size_t j = 0; j < n; j++) {
            const uint32_t t = t_read[s][j];
            if (t > j) {
                bad++;
                continue;
            }
            rc_rt[s][j] = fc_rt[s][t]++;
            rc_gmr[s][j] = fc_gmr[s][(uint32_t)j - t]++;
        }
    }
    return bad;
}
