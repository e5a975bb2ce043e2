// twin_main -- TEST INFRASTRUCTURE: what the twins' own main programs (the -D..._TWIN_MAIN builds that run under the sanitizers)
// share: the seeded generator rnd, CHECK, heap blocks of exactly a vector's size, and the random reads strand_twin and
// readpos_twin draw.  Define TWIN_NAME, the program's name in CHECK's message, before the include.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_strand.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {      // xorshift64*, [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) { printf(TWIN_NAME ": check failed at line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

template <class T> static T *exact(const std::vector<T> &v) {      // a heap block of exactly the vector's size
    T *p = (T *)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// One seeded batch of reads on a reference of G bases, its arrays in exact blocks: regular and arbitrary CIGAR words, reads in
// front of, inside and behind the reference, l_seq that disagrees with the CIGAR, QUAL '*', reads with a status.
struct TwinReads {
    int32_t G, mq;
    int64_t n;
    int32_t *pos; uint16_t *flag; uint32_t *lseq, *coff, *cig, *soff; uint8_t *seq, *qual, *status;
    void draw(int round) {
        using namespace amp;
        static const uint32_t codes[5] = {1, 2, 4, 8, 15};
        G = 1 + (int32_t)rnd(round % 5 == 0 ? 4 : 3000);
        n = rnd(round % 3 == 0 ? 700 : 40);
        mq = (int32_t)rnd(50);
        std::vector<int32_t> v_pos;
        std::vector<uint16_t> v_flag;
        std::vector<uint32_t> v_lseq, v_coff(1, 0u), words, v_soff(1, 0u);
        std::vector<uint8_t> v_seq, v_qual, v_status;
        int32_t pile = (int32_t)rnd((uint32_t)G);
        for (int64_t i = 0; i < n; ++i) {
            std::vector<uint32_t> ops;
            uint32_t L = 0;
            const uint32_t kind = rnd(10);
            if (kind < 6) {                       // regular: clips, a core of up to 9 ops, clips
                if (rnd(4) == 0) ops.push_back((rnd(5) << 4) | ST_OP_H);
                if (rnd(3) == 0) ops.push_back((rnd(9) << 4) | ST_OP_S);
                const uint32_t core = 1 + rnd(kind == 0 ? 9 : 3);
                for (uint32_t k = 0; k < core; ++k) {
                    static const uint32_t pick[7] = {ST_OP_M, ST_OP_M, ST_OP_EQ, ST_OP_X, ST_OP_I, ST_OP_D, ST_OP_N};
                    ops.push_back((rnd(k % 2 ? 6 : 90) << 4) | pick[rnd(k == 0 ? 4 : 7)]);
                }
                if (rnd(3) == 0) ops.push_back((rnd(9) << 4) | ST_OP_S);
                if (rnd(4) == 0) ops.push_back((rnd(5) << 4) | ST_OP_H);
            } else {                              // anything
                const uint32_t k = rnd(8) == 0 ? 40 + rnd(10) : rnd(6);
                for (uint32_t j = 0; j < k; ++j) ops.push_back((rnd(30) << 4) | rnd(10));
            }
            for (uint32_t v : ops) { const uint32_t op = v & 15u; if (op == ST_OP_M || op == ST_OP_I || op == ST_OP_S || op == ST_OP_EQ || op == ST_OP_X) L += v >> 4; }
            if (rnd(12) == 0) L = rnd(2) ? L + 1 + rnd(5) : (L > 3 ? L - 1 - rnd(3) : 0);      // l_seq and the CIGAR disagree
            for (uint32_t v : ops) words.push_back(v);
            v_coff.push_back((uint32_t)words.size());
            // a pile, a wide spread, and reads in front of and behind the reference
            const uint32_t where = rnd(10);
            v_pos.push_back(where < 6 ? pile + (int32_t)rnd(40) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1));
            v_flag.push_back((uint16_t)((rnd(2) ? 0x10u : 0u) | (rnd(2) ? 0x1u : 0u)));
            v_lseq.push_back(L);
            v_status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = v_qual.size();
            for (uint32_t k = 0; k < padded; ++k) v_qual.push_back((uint8_t)rnd(60));
            if (L && rnd(30) == 0) v_qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) v_seq.push_back((uint8_t)((codes[rnd(5)] << 4) | codes[rnd(5)]));
            v_soff.push_back((uint32_t)(v_qual.size() / 8));
        }
        pos = exact(v_pos); flag = exact(v_flag); lseq = exact(v_lseq); coff = exact(v_coff); cig = exact(words); soff = exact(v_soff);
        seq = exact(v_seq); qual = exact(v_qual); status = exact(v_status);
    }
    void release() { free(pos); free(flag); free(lseq); free(coff); free(cig); free(soff); free(seq); free(qual); free(status); }
};
