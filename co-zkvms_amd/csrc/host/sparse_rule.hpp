// The storage rule of the sparse pair layers (csrc/sparse_layer.inc) and the prover's hand-over decision.  Host-only and free of
// any other header of the project, so that a small CPU program can test it (tests/native/sparse_rule_check.cpp).
#pragma once
#include <stddef.h>

// THE one rule, used at construct and after every bind: a layer of dense length n stays sparse while 2 * cnt <= n / 2, i.e. while
// it stores at most half of its n / 2 pairs.  A storage rule -- the sparse bytes cnt * (64 NC + 4) then stay below the dense bytes
// n * 32 NC -- not one tuned for time.
static inline bool sparse_rule_keeps(size_t cnt, size_t n) { return 2 * cnt <= n / 2; }

// Construct: a layer of `batch` circuits is stored sparse if the rule keeps it and it is above the reference's coalesce point (one
// pair per circuit, sparse_interleaved_poly.rs:57-67), where the reference's own layer is dense.
static inline bool sparse_construct_keeps(size_t cnt, size_t n, size_t batch) { return batch > 0 && n / batch >= 4 && sparse_rule_keeps(cnt, n); }

// Prove: after the challenge of a round, hand over to a dense layer if the bind -- to next_cnt stored pairs of a layer of n / 2 --
// breaks the rule or leaves one pair per circuit.  It always happens: the length halves per round and n / 2 / batch reaches 2.
static inline bool sparse_handover_after_bind(size_t next_cnt, size_t n, size_t batch) {
    const size_t next_n = n / 2;
    return batch == 0 || next_n / batch <= 2 || !sparse_rule_keeps(next_cnt, next_n);
}
