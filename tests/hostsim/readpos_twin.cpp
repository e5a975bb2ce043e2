// readpos_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_readpos.hpp that k_readpos calls per read and per
// base, looped over arrays on the CPU in the kernel's own order of steps: tiles of RP_BLOCK reads, their shapes, the window
// rule, the segment list, one add per (segment, position) into the window's 16-bit halves, the serial walk of the other reads,
// the flush (when the window moves, every RP_MAX_TILES_PER_FLUSH tiles, at the end).  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libreadpos_twin.so readpos_twin.cpp   (tests/test_readpos_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DREADPOS_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o readpos_twin readpos_twin.cpp && ./readpos_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_readpos.hpp"

using namespace amp;

extern "C" {

int twin_window() { return RP_W; }
int twin_slots() { return RP_SLOTS; }
int twin_flush_period() { return RP_MAX_TILES_PER_FLUSH; }
int twin_rp_bin(int32_t d) { return (int)rp_bin(d); }

// The reads are given as they are walked (with do_trim: the trimmed pos and CIGAR).  hist: uint32[ref_len][6][7], added to.
// info[0..4]: reads that took the window, reads that walked serially, flushes that found a non-zero word, adds the serial reads
// made inside the window, the largest 16-bit half a flush met.  force_serial: every read walks (the window stays empty).
// Returns non-zero when a step left its bounds (a word outside the window, a segment past the list, a position past the
// table, a negative distance, a half that carried).
int twin_readpos(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                 const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                 int32_t force_serial, uint32_t *hist, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    std::vector<uint32_t> cell((size_t)RP_W * RP_WORDS, 0u);
    std::vector<uint32_t> shadow((size_t)RP_W * RP_CELLS, 0u);       // the same adds, a u32 per cell: a carry between halves shows
    std::vector<ReadposSeg> segs((size_t)RP_BLOCK * RP_SLOTS);
    int bad = 0;
    int32_t anchor = 0;
    int since = 0;
    for (int k = 0; k < 5; ++k) info[k] = 0;
    auto add = [&](int32_t w, int c) {
        if (w < 0 || w >= RP_W || c < 0 || c >= RP_CELLS) { bad |= 1; return; }
        cell[(size_t)rp_word(w, c)] += rp_one(c);
        shadow[(size_t)w * RP_CELLS + c] += 1u;
    };
    auto flush = [&]() {
        bool any = false;
        for (int k = 0; k < RP_W * RP_WORDS; ++k) {
            const uint32_t v = cell[(size_t)k];
            if (!v) continue;
            any = true;
            cell[(size_t)k] = 0u;
            const int64_t p = (int64_t)anchor + k / RP_WORDS;
            const int c = 2 * (k % RP_WORDS);
            if (p < 0 || p >= ref_len) { bad |= 2; continue; }
            const uint32_t half[2] = {v & 0xFFFFu, v >> 16};
            for (int h = 0; h < 2; ++h) {
                if (half[h] != shadow[(size_t)(k / RP_WORDS) * RP_CELLS + c + h]) bad |= 32;
                if ((int64_t)half[h] > info[4]) info[4] = half[h];
                hist[(size_t)p * RP_CELLS + c + h] += half[h];
            }
        }
        std::fill(shadow.begin(), shadow.end(), 0u);
        if (any) ++info[2];
    };
    for (int64_t base = 0; base < n; base += RP_BLOCK) {
        const int m = (int)(n - base < RP_BLOCK ? n - base : RP_BLOCK);
        StrandRead R[RP_BLOCK];
        StrandShape sh[RP_BLOCK];
        bool live[RP_BLOCK];
        uint32_t qual0[RP_BLOCK];
        int32_t lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            live[t] = !status || status[i] == 0;
            R[t] = StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], (flag[i] & 0x10u) ? 1u : 0u, (uint64_t)seq_off8[i] * 8ull};
            qual0[t] = R[t].lseq > 0 ? qual[R[t].base] : 0xFFu;
            sh[t] = StrandShape{false, 0, 0};
            if (!live[t]) continue;
            sh[t] = readpos_segments(R[t], P, qual0[t], [](const ReadposSeg &) {});
            if (force_serial) sh[t].regular = false;
            if (sh[t].regular) { lo = R[t].pos < lo ? R[t].pos : lo; hi = sh[t].ref_end > hi ? sh[t].ref_end : hi; }
        }
        if (!readpos_window_keeps(anchor, lo, hi) || since >= RP_MAX_TILES_PER_FLUSH) {
            flush();
            if (lo <= hi) anchor = lo;
            since = 0;
        }
        ++since;
        size_t ns = 0;
        bool win[RP_BLOCK];
        for (int t = 0; t < m; ++t) {
            win[t] = live[t] && readpos_read_windowed(sh[t], R[t].pos, anchor);
            if (!win[t]) continue;
            ++info[0];
            readpos_segments(R[t], P, qual0[t], [&](const ReadposSeg &s) {
                if (ns < segs.size()) segs[ns++] = s; else bad |= 4;
            });
        }
        for (size_t s = 0; s < ns; ++s) {
            const ReadposSeg g = segs[s];
            const int32_t a0 = g.r0 - anchor, a1 = a0 + rp_seg_len(g);
            if (a0 < 0 || a1 > RP_W) { bad |= 8; continue; }
            for (int32_t p = a0; p < a1; ++p) {
                uint32_t col = 5u;
                if (!rp_seg_del(g) && !readpos_base(seq, qual, g.q0 + (uint64_t)(p - a0), min_quality, col)) continue;
                const int32_t d = rp_seg_d(g, p - a0);
                if (d < 0) { bad |= 64; continue; }
                add(p, rp_cell(col, rp_bin(d)));
            }
        }
        for (int t = 0; t < m; ++t) {
            if (!live[t] || win[t]) continue;
            ++info[1];
            readpos_walk(R[t], P, seq, qual, [&](int32_t r, uint32_t col, int32_t d) {
                if (r < 0 || r >= ref_len || col > 5u) { bad |= 16; return; }
                if (d < 0) { bad |= 64; return; }
                const int c = rp_cell(col, rp_bin(d));
                const int64_t w = (int64_t)r - (int64_t)anchor;
                if (w >= 0 && w < RP_W) { ++info[3]; add((int32_t)w, c); }
                else hist[(size_t)r * RP_CELLS + c] += 1u;
            });
        }
    }
    flush();
    return bad;
}

}  // extern "C"

#ifdef READPOS_TWIN_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {      // xorshift64*, [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) { printf("readpos_twin: check failed at line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

template <class T> static T *exact(const std::vector<T> &v) {      // a heap block of exactly the vector's size
    T *p = (T *)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int main() {
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    int64_t windowed = 0, serial = 0;
    for (int32_t d = 0; d < 300; ++d) {
        const uint32_t want = d < 2 ? 0u : d < 4 ? 1u : d < 8 ? 2u : d < 16 ? 3u : d < 32 ? 4u : d < 64 ? 5u : 6u;
        CHECK(rp_bin(d) == want);
    }
    CHECK(rp_bin(0x7FFFFFFF) == 6u);
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 1 + (int32_t)rnd(round % 5 == 0 ? 4 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 700 : 40);
        const int32_t mq = (int32_t)rnd(50);
        std::vector<int32_t> pos;
        std::vector<uint16_t> flag;
        std::vector<uint32_t> lseq, coff(1, 0u), words, soff(1, 0u);
        std::vector<uint8_t> seq, qual, status;
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
            coff.push_back((uint32_t)words.size());
            // a pile, a wide spread, and reads in front of and behind the reference
            const uint32_t where = rnd(10);
            pos.push_back(where < 6 ? pile + (int32_t)rnd(40) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1));
            flag.push_back((uint16_t)((rnd(2) ? 0x10u : 0u) | (rnd(2) ? 0x1u : 0u)));
            lseq.push_back(L);
            status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = qual.size();
            for (uint32_t k = 0; k < padded; ++k) qual.push_back((uint8_t)rnd(60));
            if (L && rnd(30) == 0) qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) seq.push_back((uint8_t)((codes[rnd(5)] << 4) | codes[rnd(5)]));
            soff.push_back((uint32_t)(qual.size() / 8));
        }
        int32_t *p_pos = exact(pos); uint16_t *p_flag = exact(flag); uint32_t *p_lseq = exact(lseq), *p_coff = exact(coff), *p_cig = exact(words), *p_soff = exact(soff);
        uint8_t *p_seq = exact(seq), *p_qual = exact(qual), *p_st = exact(status);
        const size_t nh = (size_t)G * RP_CELLS;
        uint32_t *hist[2];
        int64_t info[2][5];
        for (int mode = 0; mode < 2; ++mode) {
            hist[mode] = (uint32_t *)calloc(nh, 4);
            CHECK(twin_readpos(n, p_pos, p_flag, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, p_st, G, mq, mode, hist[mode], info[mode]) == 0);
        }
        // the window and the walk agree on every read, and the all-serial run never touches the segments
        CHECK(memcmp(hist[0], hist[1], nh * 4) == 0);
        CHECK(info[1][0] == 0 && info[0][0] + info[0][1] == info[1][1]);
        windowed += info[0][0]; serial += info[0][1];
        free(p_pos); free(p_flag); free(p_lseq); free(p_coff); free(p_cig); free(p_soff); free(p_seq); free(p_qual); free(p_st);
        for (int mode = 0; mode < 2; ++mode) free(hist[mode]);
    }
    CHECK(windowed > 1000 && serial > 1000);
    printf("readpos_twin ok\n");
    return 0;
}
#endif
