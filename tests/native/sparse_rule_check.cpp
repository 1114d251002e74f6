// Stand-alone CPU check of the storage rule and the hand-over decision of the sparse pair layers
// (co-zkvms_amd/csrc/host/sparse_rule.hpp): built and run by tests/test_sparse_rule_host.py.  Exit status 0 = every check held.
#include <stdio.h>
#include "../../co-zkvms_amd/csrc/host/sparse_rule.hpp"

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #c);     \
            failures++;                                       \
        }                                                     \
    } while (0)

int main() {
    // the rule: at most half of the n / 2 pairs stored, i.e. sparse bytes cnt * (64 NC + 4) below dense bytes n * 32 NC
    CHECK(sparse_rule_keeps(0, 2));
    CHECK(sparse_rule_keeps(4, 16) && !sparse_rule_keeps(5, 16));
    CHECK(sparse_rule_keeps(1, 4) && !sparse_rule_keeps(2, 4) && !sparse_rule_keeps(1, 2));
    for (size_t n = 2; n <= 4096; n += 2)
        for (size_t cnt = 0; cnt <= n / 2; cnt++) {
            const bool keep = sparse_rule_keeps(cnt, n);
            CHECK(keep == (2 * cnt <= n / 2));
            for (size_t nc = 1; nc <= 2; nc++)
                if (keep) CHECK(cnt * (64 * nc + 4) <= n * 32 * nc);
        }
    // construct: nothing at or below the coalesce point (one pair per circuit) is stored sparse, however empty
    CHECK(!sparse_construct_keeps(0, 2 * 6, 6) && !sparse_construct_keeps(0, 6, 6) && sparse_construct_keeps(0, 4 * 6, 6));
    CHECK(sparse_construct_keeps(6, 4 * 6, 6) && !sparse_construct_keeps(7, 4 * 6, 6) && !sparse_construct_keeps(0, 16, 0));
    // prove: whatever the counts, a layer of `batch` circuits of per >= 4 entries hands over after at least one round and with at
    // least one dense round left: rounds = log2(next_pow2(n / 2)), sparse rounds <= log2(per) - 1
    for (size_t batch = 2; batch <= 40; batch += 2)
        for (size_t per = 4; per <= 1024; per *= 2) {
            size_t n = batch * per, sparse_rounds = 0, rounds = 0;
            for (size_t p = 1; p < n / 2; p *= 2) rounds++;
            for (;;) {
                sparse_rounds++;                                   // the round runs, its challenge arrives
                if (sparse_handover_after_bind(0, n, batch)) break;  // nothing stored: only the coalesce point stops it
                n /= 2;
                CHECK(n % 4 == 0);                                 // the lengths a sparse layer binds and sums at
            }
            CHECK(sparse_rounds >= 1 && sparse_rounds < rounds);
            CHECK(n / 2 == 2 * batch);  // handed over with one pair per circuit left after the bind
        }
    CHECK(sparse_handover_after_bind(5, 32, 2) && !sparse_handover_after_bind(4, 32, 2));  // the bind breaks the rule / keeps it
    CHECK(sparse_handover_after_bind(0, 8, 2) && sparse_handover_after_bind(0, 64, 0));
    if (!failures) printf("sparse_rule_check: ok\n");
    return failures ? 1 : 0;
}
