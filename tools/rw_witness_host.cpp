// The sequential walk of the read-write memory witness (jolt-core's ReadWriteMemoryPolynomials::generate_witness) as a plain host loop:
// the n * n_slots operations in (step, slot) order against one table of MEM words and one of MEM timestamps.  One thread: every
// operation depends on the one before it, so the walk cannot be split.  What a dealer does without cozk_rw_memory_witness.  Built by
// tools/run_rw_witness.py (g++ -O2 -shared -fPIC) as the baseline beside the device call, and as a full-size cross-check.
#include <cstddef>
#include <cstdint>
#include <cstring>

// v_write[s] null: the slot only reads; is_write[s] null: every step writes; v_written[s] may be null.  Returns the number of
// addresses >= MEM (those operations are skipped).
extern "C" size_t rw_witness_host(const uint32_t* const* addr, const uint32_t* const* v_write, const uint8_t* const* is_write, size_t n_slots, size_t n,
                                  const uint32_t* v_init, size_t MEM, uint32_t* const* v_read, uint32_t* const* t_read, uint32_t* const* v_written, uint32_t* v_final,
                                  uint32_t* t_final) {
    memcpy(v_final, v_init, MEM * sizeof(uint32_t));
    memset(t_final, 0, MEM * sizeof(uint32_t));
    size_t bad = 0;
    for (size_t j = 0; j < n; j++)
        for (size_t s = 0; s < n_slots; s++) {
            const uint32_t a = addr[s][j];
            if (a >= MEM) {
                bad++;
                continue;
            }
            const uint32_t v = v_final[a];
            v_read[s][j] = v;
            t_read[s][j] = t_final[a];
            const uint32_t w = v_write[s] && (!is_write[s] || is_write[s][j]) ? v_write[s][j] : v;
            v_final[a] = w;
            t_final[a] = (uint32_t)j;
            if (v_written[s]) v_written[s][j] = w;
        }
    return bad;
}
