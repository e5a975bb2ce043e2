// codon_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_codon.hpp that k_codon calls per read and per codon,
// looped over arrays on the CPU in the kernel's own order of steps: tiles of CD_BLOCK reads, their shapes, the window rule, the
// list of entries, one add per (entry, slot of the window) into the window's cells, the serial path of the other reads, the
// flush.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fPIC -shared -I amplipy_amd/csrc -o libcodon_twin.so codon_twin.cpp   (tests/test_codon_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DCODON_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o codon_twin codon_twin.cpp && ./codon_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_codon.hpp"

using namespace amp;

extern "C" {

int twin_window() { return CD_W; }
int twin_slots() { return CD_SLOTS; }
int twin_block() { return CD_BLOCK; }

// The reads are given as they are counted (with do_trim: the trimmed pos and CIGAR).  codon: uint32[n_slots][65], reads:
// uint64[2], both added to.  info[0..3]: reads that took the window, regular reads that went serially, flushes that found a
// non-zero cell, adds the serial reads made inside the window.  force_serial: every regular read goes serially (the list stays
// empty).  Returns non-zero when a step left its bounds (a cell outside the window, an entry past the list, a slot past the table).
int twin_codon(int64_t n, const int32_t *pos, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8,
               const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality, int32_t n_slots,
               const int32_t *starts, int32_t force_serial, uint32_t *codon, uint64_t *reads, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    std::vector<uint32_t> cell((size_t)CD_W * CD_CELLS, 0u);
    std::vector<StrandSeg> segs((size_t)CD_BLOCK * CD_SLOTS);
    int bad = 0;
    CodonWindow w = codon_window_none();
    int since = 0;
    for (int k = 0; k < 4; ++k) info[k] = 0;
    auto flush = [&]() {
        bool any = false;
        for (int k = 0; k < CD_W * CD_CELLS; ++k) {
            const uint32_t v = cell[(size_t)k];
            if (!v) continue;
            any = true;
            cell[(size_t)k] = 0u;
            const int64_t slot = (int64_t)w.a0 + k / CD_CELLS;
            if (slot < 0 || slot >= n_slots) { bad |= 1; continue; }
            codon[(size_t)w.a0 * CD_CELLS + (size_t)k] += v;
        }
        if (any) ++info[2];
    };
    for (int64_t base = 0; base < n; base += CD_BLOCK) {
        const int m = (int)(n - base < CD_BLOCK ? n - base : CD_BLOCK);
        StrandRead R[CD_BLOCK];
        CodonShape sh[CD_BLOCK];
        bool live[CD_BLOCK];
        uint32_t qual0[CD_BLOCK];
        int32_t lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            live[t] = !status || status[i] == 0;
            R[t] = StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], 0u, (uint64_t)seq_off8[i] * 8ull};
            qual0[t] = R[t].lseq > 0 ? qual[R[t].base] : 0xFFu;
            sh[t] = CodonShape{false, 0, 0};
            if (!live[t]) continue;
            sh[t] = codon_segments(R[t], P, qual0[t], [](const StrandSeg &) {});
            ++reads[sh[t].regular ? 0 : 1];
            if (sh[t].regular) { lo = R[t].pos < lo ? R[t].pos : lo; hi = sh[t].ref_end > hi ? sh[t].ref_end : hi; }
        }
        if (!codon_window_keeps(w, lo, hi) || since >= CD_MAX_TILES_PER_FLUSH) {
            flush();
            if (lo <= hi) w = codon_window_at(starts, n_slots, lo);
            since = 0;
        }
        ++since;
        size_t ns = 0;
        bool win[CD_BLOCK];
        for (int t = 0; t < m; ++t) {
            win[t] = live[t] && !force_serial && codon_read_windowed(sh[t], R[t].pos, w);
            if (!win[t]) continue;
            ++info[0];
            codon_segments(R[t], P, qual0[t], [&](const StrandSeg &s) {
                if (ns < segs.size()) segs[ns++] = s; else bad |= 2;
            });
        }
        // phase B, slot-major: the slot at start p takes every entry whose range holds p
        for (int k = 0; k < CD_W; ++k) {
            const int64_t slot = (int64_t)w.a0 + k;
            if (slot >= n_slots) break;
            const int32_t p = starts[slot];
            for (size_t s = 0; s < ns; ++s) {
                const StrandSeg g = segs[s];
                if (p < g.r0 || (int64_t)p >= (int64_t)g.r0 + st_seg_len(g)) continue;
                uint32_t c;
                if (codon_entry_cell(g, p, seq, qual, min_quality, c)) {
                    if (c >= (uint32_t)CD_CELLS) { bad |= 4; continue; }
                    cell[(size_t)k * CD_CELLS + c] += 1u;
                }
            }
        }
        // ... and no entry reaches a slot outside the window (it would be lost)
        for (size_t s = 0; s < ns; ++s) {
            const StrandSeg g = segs[s];
            const int32_t f = codon_lower_bound(starts, n_slots, g.r0), l = codon_lower_bound(starts, n_slots, (int64_t)g.r0 + st_seg_len(g));
            if (f < l && (f < w.a0 || (int64_t)l > (int64_t)w.a0 + CD_W)) bad |= 16;
        }
        for (int t = 0; t < m; ++t) {
            if (!live[t] || win[t] || !sh[t].regular) continue;
            ++info[1];
            codon_read(R[t], P, seq, qual, qual0[t], starts, n_slots, [&](int32_t s, uint32_t c) {
                if (s < 0 || s >= n_slots || c >= (uint32_t)CD_CELLS) { bad |= 8; return; }
                const int64_t k = (int64_t)s - (int64_t)w.a0;
                if (k >= 0 && k < CD_W) { ++info[3]; cell[(size_t)k * CD_CELLS + c] += 1u; }
                else codon[(size_t)s * CD_CELLS + c] += 1u;
            });
        }
    }
    flush();
    return bad;
}

}  // extern "C"

#ifdef CODON_TWIN_MAIN
#define TWIN_NAME "codon_twin"
#include "twin_main.hpp"

int main() {
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    int64_t windowed = 0, serial = 0, broken = 0, triplets = 0;
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 3 + (int32_t)rnd(round % 5 == 0 ? 6 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 700 : 40);
        const int32_t mq = (int32_t)rnd(50);
        // slots: every position, one frame, or a sparse draw
        std::vector<int32_t> starts;
        const uint32_t mode_s = rnd(3);
        for (int32_t p = (int32_t)rnd(3); p + 3 <= G; p += mode_s == 0 ? 1 : mode_s == 1 ? 3 : 1 + (int32_t)rnd(40)) starts.push_back(p);
        if (starts.empty()) starts.push_back(0);
        std::vector<int32_t> pos;
        std::vector<uint32_t> lseq, coff(1, 0u), words, soff(1, 0u);
        std::vector<uint8_t> seq, qual, status;
        int32_t pile = (int32_t)rnd((uint32_t)G);
        for (int64_t i = 0; i < n; ++i) {
            std::vector<uint32_t> ops;
            uint32_t L = 0;
            const uint32_t kind = rnd(10);
            if (kind < 7) {                       // regular: clips, a core of up to 9 ops, clips
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
            lseq.push_back(L);
            status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = qual.size();
            for (uint32_t k = 0; k < padded; ++k) qual.push_back((uint8_t)rnd(60));
            if (L && rnd(30) == 0) qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) seq.push_back((uint8_t)((codes[rnd(rnd(4) ? 4 : 5)] << 4) | codes[rnd(rnd(4) ? 4 : 5)]));
            soff.push_back((uint32_t)(qual.size() / 8));
        }
        int32_t *p_pos = exact(pos), *p_st = exact(starts); uint32_t *p_lseq = exact(lseq), *p_coff = exact(coff), *p_cig = exact(words), *p_soff = exact(soff);
        uint8_t *p_seq = exact(seq), *p_qual = exact(qual), *p_status = exact(status);
        const size_t nc = starts.size() * CD_CELLS;
        uint32_t *tab[2];
        uint64_t rd[2][2] = {{0, 0}, {0, 0}};
        int64_t info[2][4];
        for (int mode = 0; mode < 2; ++mode) {
            tab[mode] = (uint32_t *)calloc(nc, 4);
            CHECK(twin_codon(n, p_pos, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, p_status, G, mq, (int32_t)starts.size(), p_st, mode, tab[mode], rd[mode], info[mode]) == 0);
        }
        // the window and the serial path agree on every read, and the all-serial run never touches the list
        CHECK(memcmp(tab[0], tab[1], nc * 4) == 0 && rd[0][0] == rd[1][0] && rd[0][1] == rd[1][1]);
        CHECK(info[1][0] == 0 && info[0][0] + info[0][1] == info[1][1] && info[1][1] == (int64_t)rd[0][0]);
        int64_t live = 0;
        for (uint8_t s : status) live += s == 0;
        CHECK((int64_t)(rd[0][0] + rd[0][1]) == live);
        windowed += info[0][0]; serial += info[0][1];
        for (size_t k = 0; k < nc; ++k) { if (k % CD_CELLS == (size_t)CD_BROKEN) broken += tab[0][k]; else triplets += tab[0][k]; }
        free(p_pos); free(p_st); free(p_lseq); free(p_coff); free(p_cig); free(p_soff); free(p_seq); free(p_qual); free(p_status);
        for (int mode = 0; mode < 2; ++mode) free(tab[mode]);
    }
    CHECK(windowed > 1000 && serial > 1000 && broken > 1000 && triplets > 1000);
    printf("codon_twin ok\n");
    return 0;
}
#endif
