// cooc_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_cooc.hpp that k_cooc calls per read and per set,
// looped over arrays on the CPU in the kernel's own order of steps: tiles of CO_BLOCK reads, their shapes, the window rule, per
// read the walk over its candidate sets, each key into the window's cells or past the window into the table, the flush.  Built
// with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fPIC -shared -I amplipy_amd/csrc -o libcooc_twin.so cooc_twin.cpp   (tests/test_cooc_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DCOOC_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o cooc_twin cooc_twin.cpp
//   ./cooc_twin [cases.bin]
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python.  With
// a file (written by tests/test_cooc_twin.py: the crafted cases with the tables the restatement expects) it runs every case from
// heap blocks of exactly the needed size and compares; without one it runs seeded batches of regular and arbitrary CIGARs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_cooc.hpp"

using namespace amp;

extern "C" {

int twin_window() { return CO_W; }
int twin_sites() { return CO_SITES; }
int twin_block() { return CO_BLOCK; }

// The reads are given as they are counted (with do_trim: the trimmed pos and CIGAR).  cooc: uint32[n_sets][65], reads:
// uint64[2], both added to.  first[s] = site_pos[set_off[s]]; max_span as amp_cooc_enable computes it.  info[0..2]: adds into
// the window, adds past it, flushes that found a non-zero cell.  Returns non-zero when a step left its bounds.
int twin_cooc(int64_t n, const int32_t *pos, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8,
              const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality, int32_t n_sets,
              const int32_t *first, const int32_t *set_off, const int32_t *site_pos, const int32_t *site_len, const int32_t *site_sym, int32_t max_span,
              uint32_t *cooc, uint64_t *reads, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    const CoocSets S{n_sets, first, set_off, site_pos, site_len, site_sym, max_span};
    std::vector<uint32_t> cell((size_t)CO_W * CO_CELLS, 0u);
    int bad = 0;
    CoocWindow w = cooc_window_none();
    int since = 0;
    for (int k = 0; k < 3; ++k) info[k] = 0;
    auto flush = [&]() {
        bool any = false;
        for (int k = 0; k < CO_W * CO_CELLS; ++k) {
            const uint32_t v = cell[(size_t)k];
            if (!v) continue;
            any = true;
            cell[(size_t)k] = 0u;
            const int64_t set = (int64_t)w.a0 + k / CO_CELLS;
            if (set < 0 || set >= n_sets) { bad |= 1; continue; }
            cooc[(size_t)w.a0 * CO_CELLS + (size_t)k] += v;
        }
        if (any) ++info[2];
    };
    for (int64_t base = 0; base < n; base += CO_BLOCK) {
        const int m = (int)(n - base < CO_BLOCK ? n - base : CO_BLOCK);
        StrandRead R[CO_BLOCK];
        StrandShape sh[CO_BLOCK];
        uint32_t qual0[CO_BLOCK];
        int32_t lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            R[t] = StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], 0u, (uint64_t)seq_off8[i] * 8ull};
            qual0[t] = R[t].lseq > 0 ? qual[R[t].base] : 0xFFu;
            sh[t].regular = false; sh[t].n_seg = 0; sh[t].ref_end = 0;
            if (status && status[i] != 0) continue;
            sh[t] = regular_scan(R[t], P, qual0[t], [](int32_t, uint64_t, uint32_t, bool) {});
            ++reads[sh[t].regular ? 0 : 1];
            if (sh[t].regular) { lo = R[t].pos < lo ? R[t].pos : lo; hi = sh[t].ref_end > hi ? sh[t].ref_end : hi; }
        }
        if (!cooc_window_keeps(w, S, lo, hi) || since >= CO_MAX_TILES_PER_FLUSH) {
            flush();
            if (lo <= hi) w = cooc_window_at(S, lo);
            since = 0;
        }
        ++since;
        for (int t = 0; t < m; ++t) {
            if (!sh[t].regular) continue;
            for (int32_t s = cooc_first_candidate(S, R[t].pos); cooc_is_candidate(S, s, sh[t].ref_end); ++s) {
                uint32_t c;
                if (s < 0 || s >= n_sets) { bad |= 2; break; }
                if (!cooc_read_set(R[t], P, qual0[t], sh[t].ref_end, seq, qual, S, s, c)) continue;
                if (c >= (uint32_t)CO_CELLS) { bad |= 4; continue; }
                const int32_t key = s * CO_CELLS + (int32_t)c;
                const int32_t k = cooc_window_cell(w, key);
                if (k >= CO_W * CO_CELLS) { bad |= 8; continue; }
                if (k >= 0) { ++info[0]; cell[(size_t)k] += 1u; }
                else { ++info[1]; cooc[(size_t)key] += 1u; }
            }
        }
    }
    flush();
    return bad;
}

// One read through cooc_read, the form without a window: the same adds.
int twin_cooc_plain(int64_t n, const int32_t *pos, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8,
                    const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality, int32_t n_sets,
                    const int32_t *first, const int32_t *set_off, const int32_t *site_pos, const int32_t *site_len, const int32_t *site_sym, int32_t max_span,
                    uint32_t *cooc, uint64_t *reads) {
    const StrandParams P{ref_len, min_quality};
    const CoocSets S{n_sets, first, set_off, site_pos, site_len, site_sym, max_span};
    int bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (status && status[i] != 0) continue;
        const StrandRead R{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], 0u, (uint64_t)seq_off8[i] * 8ull};
        const uint32_t q0 = R.lseq > 0 ? qual[R.base] : 0xFFu;
        const bool regular = cooc_read(R, P, seq, qual, q0, S, [&](int32_t s, uint32_t c) {
            if (s < 0 || s >= n_sets || c >= (uint32_t)CO_CELLS) { bad |= 1; return; }
            cooc[(size_t)s * CO_CELLS + c] += 1u;
        });
        ++reads[regular ? 0 : 1];
    }
    return bad;
}

}  // extern "C"

#ifdef COOC_TWIN_MAIN
#define TWIN_NAME "cooc_twin"
#include "twin_main.hpp"

struct Sets {
    std::vector<int32_t> first, off, pos, len, sym;
    int32_t max_span = 0;
    void finish() {
        first.clear(); max_span = 0;
        for (size_t s = 0; s + 1 < off.size(); ++s) {
            first.push_back(pos[(size_t)off[s]]);
            const int32_t span = pos[(size_t)off[s + 1] - 1] - pos[(size_t)off[s]];
            if (span > max_span) max_span = span;
        }
    }
};

struct Batch {
    std::vector<int32_t> pos;
    std::vector<uint32_t> lseq, coff, words, soff;
    std::vector<uint8_t> seq, qual, status;
};

// window and plain must agree; -> 0, or the line of what failed
static int run(const Batch &b, const Sets &S, int32_t G, int32_t mq, std::vector<uint32_t> &tab, uint64_t rd[2], int64_t info[3]) {
    const int64_t n = (int64_t)b.pos.size();
    int32_t *p_pos = exact(b.pos), *p_first = exact(S.first), *p_off = exact(S.off), *p_sp = exact(S.pos), *p_sl = exact(S.len), *p_ss = exact(S.sym);
    uint32_t *p_lseq = exact(b.lseq), *p_coff = exact(b.coff), *p_cig = exact(b.words), *p_soff = exact(b.soff);
    uint8_t *p_seq = exact(b.seq), *p_qual = exact(b.qual), *p_status = exact(b.status);
    const int32_t ns = (int32_t)S.first.size();
    const size_t nc = (size_t)ns * CO_CELLS;
    tab.assign(nc, 0u);
    std::vector<uint32_t> plain(nc, 0u);
    uint64_t rd2[2] = {0, 0};
    rd[0] = rd[1] = 0;
    uint32_t *t0 = exact(tab), *t1 = exact(plain);
    const int bad0 = twin_cooc(n, p_pos, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, b.status.empty() ? nullptr : p_status, G, mq, ns, p_first, p_off, p_sp, p_sl, p_ss,
                               S.max_span, t0, rd, info);
    const int bad1 = twin_cooc_plain(n, p_pos, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, b.status.empty() ? nullptr : p_status, G, mq, ns, p_first, p_off, p_sp, p_sl,
                                     p_ss, S.max_span, t1, rd2);
    const bool same = memcmp(t0, t1, nc * 4) == 0 && rd[0] == rd2[0] && rd[1] == rd2[1];
    if (nc) memcpy(tab.data(), t0, nc * 4);
    free(p_pos); free(p_first); free(p_off); free(p_sp); free(p_sl); free(p_ss); free(p_lseq); free(p_coff); free(p_cig); free(p_soff);
    free(p_seq); free(p_qual); free(p_status); free(t0); free(t1);
    CHECK(bad0 == 0 && bad1 == 0);
    CHECK(same);
    return 0;
}

template <class T> static bool rd_vec(FILE *f, std::vector<T> &v) {
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0 || n > (1 << 26)) return false;
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

// the file: int32 n_cases; per case int32 G, mq; then the vectors (int64 count, elements): pos, lseq, cig_off, cig, seq_off8,
// seq, qual, set_off, site_pos, site_len, site_sym (int32), the expected cooc (uint32) and reads (uint64[2])
static int run_file(const char *fn) {
    FILE *f = fopen(fn, "rb");
    CHECK(f != nullptr);
    int32_t n_cases = 0;
    CHECK(fread(&n_cases, 4, 1, f) == 1);
    for (int32_t k = 0; k < n_cases; ++k) {
        int32_t hdr[2];
        CHECK(fread(hdr, 4, 2, f) == 2);
        Batch b; Sets S;
        std::vector<uint32_t> want, got;
        std::vector<uint64_t> want_rd;
        CHECK(rd_vec(f, b.pos) && rd_vec(f, b.lseq) && rd_vec(f, b.coff) && rd_vec(f, b.words) && rd_vec(f, b.soff) && rd_vec(f, b.seq) && rd_vec(f, b.qual));
        CHECK(rd_vec(f, S.off) && rd_vec(f, S.pos) && rd_vec(f, S.len) && rd_vec(f, S.sym) && rd_vec(f, want) && rd_vec(f, want_rd));
        CHECK(S.off.size() >= 2 && want_rd.size() == 2);
        S.finish();
        uint64_t rd[2];
        int64_t info[3];
        CHECK(run(b, S, hdr[0], hdr[1], got, rd, info) == 0);
        if (got != want || rd[0] != want_rd[0] || rd[1] != want_rd[1]) { printf("cooc_twin: case %d differs from the expected tables\n", k); fclose(f); return 1; }
    }
    fclose(f);
    printf("cooc_twin ok: %d cases\n", n_cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_file(argv[1]);
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    int64_t in_window = 0, past = 0, partial = 0, complete = 0, skipped = 0;
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 3 + (int32_t)rnd(round % 5 == 0 ? 6 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 700 : 40);
        const int32_t mq = (int32_t)rnd(50);
        // sets: sparse, dense, or more than a window holds; sorted by first site as they are made
        Sets S;
        S.off.push_back(0);
        const uint32_t mode_s = rnd(3);
        for (int32_t p = (int32_t)rnd(3); p < G; p += mode_s == 0 ? 1 + (int32_t)rnd(60) : mode_s == 1 ? (int32_t)rnd(2) : 1 + (int32_t)rnd(4)) {
            const uint32_t sites = 1 + rnd(CO_SITES);
            int32_t at = p;
            for (uint32_t j = 0; j < sites && at < G; ++j) {
                const int32_t len = rnd(3) == 0 ? 1 + (int32_t)rnd(6) : 0;
                if (at + (len ? len : 1) > G) break;
                S.pos.push_back(at); S.len.push_back(len); S.sym.push_back(len ? 0 : (int32_t)rnd(4));
                at += (len ? len : 1) + (int32_t)rnd(rnd(4) ? 8 : 200);
            }
            if ((int32_t)S.pos.size() > S.off.back()) S.off.push_back((int32_t)S.pos.size());
        }
        if (S.off.size() < 2) { S.pos.push_back(0); S.len.push_back(0); S.sym.push_back(0); S.off.push_back(1); }
        S.finish();
        Batch b;
        b.coff.push_back(0u); b.soff.push_back(0u);
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
            for (uint32_t v : ops) b.words.push_back(v);
            b.coff.push_back((uint32_t)b.words.size());
            const uint32_t where = rnd(10);       // a pile, a wide spread, and reads in front of and behind the reference
            b.pos.push_back(where < 6 ? pile + (int32_t)rnd(40) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1));
            b.lseq.push_back(L);
            b.status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = b.qual.size();
            for (uint32_t k = 0; k < padded; ++k) b.qual.push_back((uint8_t)rnd(60));
            if (L && rnd(30) == 0) b.qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) b.seq.push_back((uint8_t)((codes[rnd(rnd(4) ? 4 : 5)] << 4) | codes[rnd(rnd(4) ? 4 : 5)]));
            b.soff.push_back((uint32_t)(b.qual.size() / 8));
        }
        std::vector<uint32_t> tab;
        uint64_t rd[2];
        int64_t info[3];
        CHECK(run(b, S, G, mq, tab, rd, info) == 0);
        int64_t live = 0;
        for (uint8_t s : b.status) live += s == 0;
        CHECK((int64_t)(rd[0] + rd[1]) == live);
        in_window += info[0]; past += info[1]; skipped += (int64_t)rd[1];
        for (size_t k = 0; k < tab.size(); ++k) { if (k % CO_CELLS == (size_t)CO_PARTIAL) partial += tab[k]; else complete += tab[k]; }
    }
    CHECK(in_window > 1000 && past > 1000 && partial > 1000 && complete > 1000 && skipped > 100);
    printf("cooc_twin ok\n");
    return 0;
}
#endif
