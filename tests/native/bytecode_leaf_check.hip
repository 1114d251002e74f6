// Stand-alone host program around csrc/bytecode_arith.hip.hpp (tests/test_bytecode_leaf_host.py): the word arithmetic of the bytecode
// leaf kernels on a CPU, no GPU and no project library.  stdin: a u64 case count, then per case 19 u64 words: gamma[4], tau[4] (Montgomery),
// the row number, the seven entries, a bit mask of the entries with a high half (U64 / I64 columns), imm_signed, one word unused.
// stdout per case three 32-byte Montgomery words: bc_read_public(entries), and bc_init_final(row, entries)'s init and final.
#include <stdio.h>
#include <vector>
#include "../../co-zkvms_amd/csrc/bytecode_arith.hip.hpp"

int main() {
    uint64_t n = 0;
    if (fread(&n, 8, 1, stdin) != 1) return 2;
    std::vector<fe> out;
    for (uint64_t c = 0; c < n; c++) {
        uint64_t w[19];
        if (fread(w, 8, 19, stdin) != 19) return 2;
        const BcCoeffs cf = bc_coeffs(w, w + 4);
        auto entry = [&](int k) { return BcEntry{w[9 + k], ((w[16] >> k) & 1) != 0}; };
        fe init, fin;
        bc_init_final(cf, (uint32_t)w[8], entry, w[17] != 0, init, fin);
        out.push_back(bc_read_public(cf, entry));
        out.push_back(init);
        out.push_back(fin);
    }
    return fwrite(out.data(), sizeof(fe), out.size(), stdout) == out.size() ? 0 : 3;
}
