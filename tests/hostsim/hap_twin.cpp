// hap_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_hap.hpp that k_hap calls, looped over arrays on the CPU
// in the kernel's own order of steps: tiles of HP_BLOCK reads, waves of 64 lanes that walk their candidate regions in step, per
// step the tallies combined by region and the keys combined by equality, one insert per distinct key through hap_probe with a
// compare-and-swap on a plain array.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fPIC -shared -I amplipy_amd/csrc -o libhap_twin.so hap_twin.cpp   (tests/test_hap_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DHAP_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o hap_twin hap_twin.cpp
//   ./hap_twin [cases.bin]
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python.  With
// a file (written by tests/test_hap_twin.py: the crafted cases with the tables the restatement expects) it runs every case from
// heap blocks of exactly the needed size and compares; without one it sweeps the 16-at-once compare over every nibble phase
// and runs seeded batches of regular and arbitrary CIGARs, with the 16-at-once compare and with the one-base one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amp_hap.hpp"

using namespace amp;

extern "C" {

// MAX_DIFFS, MAX_REGION, TALLY_COLS, KEY_WORDS, GLOBAL_PROBES, LOG2_DEFAULT, BLOCK, KIND_N, KIND_DEL, EMPTY (low 31 bits)
void twin_constants(int32_t *out) {
    const int32_t v[10] = {HP_MAX_DIFFS, HP_MAX_REGION, HP_TALLY_COLS, HP_KEY_WORDS, HP_GLOBAL_PROBES, HP_LOG2_DEFAULT, HP_BLOCK, HP_KIND_N, HP_KIND_DEL,
                           (int32_t)(HP_EMPTY & 0x7FFFFFFFu)};
    for (int k = 0; k < 10; ++k) out[k] = v[k];
}

uint64_t twin_hash(const uint32_t *key) { return hap_hash(key); }
uint32_t twin_slot(const uint32_t *key, uint32_t log2_capacity) { return hap_slot_global(hap_hash(key), log2_capacity); }

// The n bases from read base k0 against the reference from p0, by the 16-at-once compare and by the one-base function: -> the
// number of differences of good quality when both hand out the same (position, code) list and the same low-quality flag
// (*lowq), -1 otherwise.  diffs: room for n pairs (position, code).
int32_t twin_match_both(const uint8_t *seq, const uint8_t *qual, uint64_t k0, const uint8_t *ref_ascii, int32_t ref_len, int32_t p0, int32_t n, int32_t min_quality,
                        int32_t *diffs, int32_t *lowq) {
    const size_t rb = ((size_t)ref_len + 1) / 2;
    std::vector<uint8_t> code4(rb, 0), mask4(rb, 0);
    hap_pack_ref(ref_ascii, ref_len, code4.data(), mask4.data());
    const HapRef F{code4.data(), mask4.data()};
    std::vector<int32_t> a, b;
    const bool la = hap_match16(seq, qual, k0, F, p0, n, min_quality, [&](int32_t p, uint32_t c) { a.push_back(p); a.push_back((int32_t)c); });
    const bool lb = hap_match1(seq, qual, k0, F, p0, n, min_quality, [&](int32_t p, uint32_t c) { b.push_back(p); b.push_back((int32_t)c); });
    if (a != b || la != lb) return -1;
    for (size_t k = 0; k < b.size(); ++k) diffs[k] = b[k];
    *lowq = lb ? 1 : 0;
    return (int32_t)(b.size() / 2);
}

// The reads are given as they are counted (with do_trim: the trimmed pos and CIGAR).  entries: room for cap of them, *n_entries
// the used slots, ordered by the key words; info[0..2]: used, capacity, lost; info[3]: inserts made (after the combine);
// tally: uint64[n_regions][6], reads: uint64[2], both added to.  fast: the 16-at-once compare.  Returns non-zero when a step
// left its bounds.
int twin_hap(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8,
             const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality, int32_t n_regions, const int32_t *start,
             const int32_t *end, const uint8_t *ref_ascii, int32_t log2_capacity, int32_t fast, amp_hap_entry *entries, int64_t cap, int64_t *n_entries,
             uint64_t *info, uint64_t *tally, uint64_t *reads) {
    const StrandParams P{ref_len, min_quality};
    const HapRegions G{n_regions, start, end};
    const size_t rb = ((size_t)ref_len + 1) / 2;
    std::vector<uint8_t> code4(rb, 0), mask4(rb, 0);
    hap_pack_ref(ref_ascii, ref_len, code4.data(), mask4.data());
    const HapRef F{code4.data(), mask4.data()};
    const size_t slots = (size_t)1 << log2_capacity;
    std::vector<uint32_t> keys(slots * HP_KEY_WORDS, HP_EMPTY), cnt(slots * 2, 0u);
    uint64_t used = 0, lost = 0, inserts = 0;
    int bad = 0;
    auto insert = [&](const uint32_t *key, uint32_t count, uint32_t rev) {
        bool fresh;
        ++inserts;
        const int64_t s = hap_probe(key, hap_slot_global(hap_hash(key), (uint32_t)log2_capacity), (uint32_t)(slots - 1), hap_probes_global((uint32_t)log2_capacity),
                                    [&](uint32_t slot, int w, uint32_t v) {
                                        if (slot >= slots || w < 0 || w >= HP_KEY_WORDS) { bad |= 1; return 0u; }
                                        uint32_t &cell = keys[(size_t)slot * HP_KEY_WORDS + (size_t)w];
                                        const uint32_t prev = cell;
                                        if (prev == HP_EMPTY) cell = v;
                                        return prev;
                                    }, fresh);
        if (s < 0) { lost += count; return; }
        if (fresh) ++used;
        cnt[2 * (size_t)s] += count; cnt[2 * (size_t)s + 1] += rev;
    };
    for (int64_t base = 0; base < n; base += HP_BLOCK) {
        const int m = (int)(n - base < HP_BLOCK ? n - base : HP_BLOCK);
        for (int w0 = 0; w0 < m; w0 += 64) {               // a wave
            const int lanes = m - w0 < 64 ? m - w0 : 64;
            StrandRead R[64];
            StrandShape sh[64];
            uint32_t qual0[64], key[64][HP_KEY_WORDS];
            int32_t r[64];
            bool more[64], live[64], covered[64];
            for (int t = 0; t < lanes; ++t) {
                const int64_t i = base + w0 + t;
                R[t] = StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], (flag[i] & 0x10u) ? 1u : 0u, (uint64_t)seq_off8[i] * 8ull};
                qual0[t] = R[t].lseq > 0 ? qual[R[t].base] : 0xFFu;
                sh[t].regular = false; sh[t].n_seg = 0; sh[t].ref_end = 0;
                live[t] = !(status && status[i] != 0);
                covered[t] = false;
                if (live[t]) sh[t] = regular_scan(R[t], P, qual0[t], [](int32_t, uint64_t, uint32_t, bool) {});
                r[t] = sh[t].regular ? hap_first_candidate(G, R[t].pos) : G.n;
                more[t] = sh[t].regular && hap_is_candidate(G, r[t], sh[t].ref_end);
            }
            for (;;) {                                      // a step of the walk
                bool any = false;
                for (int t = 0; t < lanes; ++t) any = any || more[t];
                if (!any) break;
                int32_t reg[64];
                int out[64];
                for (int t = 0; t < lanes; ++t) {
                    reg[t] = -1; out[t] = HP_OUT_NONE;
                    if (!more[t]) continue;
                    if (r[t] < 0 || r[t] >= n_regions) { bad |= 2; more[t] = false; continue; }
                    if (hap_covers(G, r[t], sh[t].ref_end)) {
                        if (start[r[t]] < R[t].pos) bad |= 4;
                        reg[t] = r[t];
                        out[t] = fast ? hap_judge<true>(R[t], P, qual0[t], seq, qual, F, r[t], start[r[t]], end[r[t]], key[t])
                                      : hap_judge<false>(R[t], P, qual0[t], seq, qual, F, r[t], start[r[t]], end[r[t]], key[t]);
                        covered[t] = true;
                    }
                    ++r[t];
                    more[t] = hap_is_candidate(G, r[t], sh[t].ref_end);
                }
                bool done[64] = {false};
                for (int s = 0; s < lanes; ++s) {           // the tallies, a leader per distinct region
                    if (reg[s] < 0 || done[s]) continue;
                    uint64_t col[HP_TALLY_COLS] = {0, 0, 0, 0, 0, 0};
                    for (int t = s; t < lanes; ++t) {
                        if (reg[t] != reg[s]) continue;
                        done[t] = true;
                        ++col[HP_COVER];
                        if (out[t] == HP_OUT_REF) { ++col[HP_REF]; if (R[t].rev) ++col[HP_REF_REV]; }
                        if (out[t] == HP_OUT_LOWQ) ++col[HP_LOWQ];
                        if (out[t] == HP_OUT_OVERFLOW) ++col[HP_OVERFLOW];
                        if (out[t] == HP_OUT_EDGE) ++col[HP_EDGE];
                    }
                    for (int c = 0; c < HP_TALLY_COLS; ++c) tally[(size_t)reg[s] * HP_TALLY_COLS + (size_t)c] += col[c];
                }
                for (int t = 0; t < lanes; ++t) done[t] = false;
                for (int s = 0; s < lanes; ++s) {           // the keys, a leader per distinct key
                    if (out[s] != HP_OUT_KEY || done[s]) continue;
                    uint32_t count = 0, rev = 0;
                    for (int t = s; t < lanes; ++t) {
                        if (out[t] != HP_OUT_KEY || done[t] || hap_hash(key[t]) != hap_hash(key[s]) || !hap_key_equal(key[t], key[s])) continue;
                        done[t] = true;
                        ++count; rev += R[t].rev;
                    }
                    if ((key[s][0] & 0xFFFFu) != (uint32_t)reg[s] || (key[s][0] >> 16) < 1u || (key[s][0] >> 16) > (uint32_t)HP_MAX_DIFFS) bad |= 8;
                    insert(key[s], count, rev);
                }
            }
            for (int t = 0; t < lanes; ++t)
                if (live[t]) ++reads[covered[t] ? 0 : 1];
        }
    }
    info[0] = used; info[1] = slots; info[2] = lost; info[3] = inserts;
    int64_t at = 0;
    for (size_t s = 0; s < slots; ++s) {
        const uint32_t *k = &keys[s * HP_KEY_WORDS];
        if (k[0] == HP_EMPTY) continue;
        if (k[HP_KEY_WORDS - 1] == HP_EMPTY) { bad |= 16; continue; }
        if (at < cap) {
            amp_hap_entry e;
            e.head = k[0];
            for (int w = 1; w < HP_KEY_WORDS; ++w) e.diff[w - 1] = k[w];
            e.count = cnt[2 * s]; e.rev = cnt[2 * s + 1];
            entries[at] = e;
        }
        ++at;
    }
    *n_entries = at;
    if ((uint64_t)at != used) bad |= 32;
    std::sort(entries, entries + (at < cap ? at : cap), [](const amp_hap_entry &x, const amp_hap_entry &y) { return hap_key_less(&x.head, &y.head); });
    return bad;
}

}  // extern "C"

#ifdef HAP_TWIN_MAIN
#define TWIN_NAME "hap_twin"
#include "twin_main.hpp"

struct Batch {
    std::vector<int32_t> pos;
    std::vector<uint16_t> flag;
    std::vector<uint32_t> lseq, coff, words, soff;
    std::vector<uint8_t> seq, qual, status;
};

struct Result {
    std::vector<amp_hap_entry> entries;
    std::vector<uint64_t> tally;
    uint64_t reads[2], info[4];
};

static bool same_result(const Result &a, const Result &b) {
    return a.entries.size() == b.entries.size() && (a.entries.empty() || memcmp(a.entries.data(), b.entries.data(), a.entries.size() * sizeof(amp_hap_entry)) == 0) &&
           a.tally == b.tally && a.reads[0] == b.reads[0] && a.reads[1] == b.reads[1] && a.info[0] == b.info[0] && a.info[2] == b.info[2];
}

static int run(const Batch &b, const std::vector<int32_t> &start, const std::vector<int32_t> &end, const std::vector<uint8_t> &ref, int32_t mq, int32_t log2_capacity,
               int fast, Result &res) {
    const int64_t n = (int64_t)b.pos.size();
    int32_t *p_pos = exact(b.pos), *p_start = exact(start), *p_end = exact(end);
    uint16_t *p_flag = exact(b.flag);
    uint32_t *p_lseq = exact(b.lseq), *p_coff = exact(b.coff), *p_cig = exact(b.words), *p_soff = exact(b.soff);
    uint8_t *p_seq = exact(b.seq), *p_qual = exact(b.qual), *p_status = exact(b.status), *p_ref = exact(ref);
    const size_t cap = (size_t)1 << log2_capacity;
    std::vector<amp_hap_entry> ent(cap);
    res.tally.assign(start.size() * HP_TALLY_COLS, 0);
    uint64_t *p_tally = exact(res.tally);
    res.reads[0] = res.reads[1] = 0;
    int64_t ne = 0;
    const int bad = twin_hap(n, p_pos, p_flag, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, b.status.empty() ? nullptr : p_status, (int32_t)ref.size(), mq,
                             (int32_t)start.size(), p_start, p_end, p_ref, log2_capacity, fast, ent.data(), (int64_t)cap, &ne, res.info, p_tally, res.reads);
    if (!res.tally.empty()) memcpy(res.tally.data(), p_tally, res.tally.size() * 8);
    res.entries.assign(ent.begin(), ent.begin() + ne);
    free(p_pos); free(p_start); free(p_end); free(p_flag); free(p_lseq); free(p_coff); free(p_cig); free(p_soff); free(p_seq); free(p_qual); free(p_status);
    free(p_ref); free(p_tally);
    CHECK(bad == 0);
    // the invariant, summed over the regions (the lost reads are known for the table only)
    uint64_t cover = 0, rest = 0;
    for (size_t r = 0; r < start.size(); ++r) {
        const uint64_t *t = &res.tally[r * HP_TALLY_COLS];
        cover += t[HP_COVER]; rest += t[HP_REF] + t[HP_LOWQ] + t[HP_OVERFLOW] + t[HP_EDGE];
        CHECK(t[HP_REF_REV] <= t[HP_REF]);
    }
    for (const amp_hap_entry &e : res.entries) { rest += e.count; CHECK(e.rev <= e.count); }
    CHECK(cover == rest + res.info[2]);
    return 0;
}

template <class T> static bool rd_vec(FILE *f, std::vector<T> &v) {
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0 || n > (1 << 26)) return false;
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

// the file: int32 n_cases; per case int32 mq; then the vectors (int64 count, elements): pos, flag, lseq, cig_off, cig, seq_off8,
// seq, qual, start, end, ref (letters), the expected entries (16 uint32 each), tally (uint64) and reads (uint64[2])
static int run_file(const char *fn) {
    FILE *f = fopen(fn, "rb");
    CHECK(f != nullptr);
    int32_t n_cases = 0;
    CHECK(fread(&n_cases, 4, 1, f) == 1);
    for (int32_t k = 0; k < n_cases; ++k) {
        int32_t mq;
        CHECK(fread(&mq, 4, 1, f) == 1);
        Batch b;
        std::vector<int32_t> start, end;
        std::vector<uint8_t> ref;
        std::vector<uint32_t> want;
        std::vector<uint64_t> want_tally, want_rd;
        CHECK(rd_vec(f, b.pos) && rd_vec(f, b.flag) && rd_vec(f, b.lseq) && rd_vec(f, b.coff) && rd_vec(f, b.words) && rd_vec(f, b.soff) && rd_vec(f, b.seq) && rd_vec(f, b.qual));
        CHECK(rd_vec(f, start) && rd_vec(f, end) && rd_vec(f, ref) && rd_vec(f, want) && rd_vec(f, want_tally) && rd_vec(f, want_rd));
        CHECK(want_rd.size() == 2 && want.size() % 16 == 0);
        for (int fast = 0; fast < 2; ++fast) {
            Result res;
            CHECK(run(b, start, end, ref, mq, 10, fast, res) == 0);
            const bool ok = res.entries.size() * 16 == want.size() && (want.empty() || memcmp(res.entries.data(), want.data(), want.size() * 4) == 0) &&
                            res.tally == want_tally && res.reads[0] == want_rd[0] && res.reads[1] == want_rd[1] && res.info[2] == 0;
            if (!ok) { printf("hap_twin: case %d (fast %d) differs from the expected tables\n", k, fast); fclose(f); return 1; }
        }
    }
    fclose(f);
    printf("hap_twin ok: %d cases\n", n_cases);
    return 0;
}

// every nibble phase of the read offset crossed with every phase of the reference offset, lengths round 16 and across a word
// boundary, from heap blocks of exactly the bytes that hold the bases
static int sweep() {
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    static const char letters[8] = {'A', 'C', 'G', 'T', 'N', 'a', 'c', 't'};
    int64_t diffs = 0, lows = 0;
    for (uint32_t kq = 0; kq < 16; ++kq)
        for (uint32_t kr = 0; kr < 16; ++kr)
            for (int32_t n : {1, 2, 15, 16, 17, 31, 32, 33, 40}) {
                const size_t L = kq + (size_t)n, G = kr + (size_t)n;
                std::vector<uint8_t> seq((L + 1) / 2), qual(L), ref(G);
                for (size_t p = 0; p < G; ++p) ref[p] = (uint8_t)letters[rnd(8)];
                for (uint8_t &q : qual) q = (uint8_t)(rnd(8) ? 30 + rnd(10) : rnd(20));
                for (size_t k = 0; k < L; ++k) {
                    uint32_t c = codes[rnd(rnd(6) ? 4 : 5)];
                    if (k >= kq && rnd(4)) c = hap_ref_code(ref[kr + (k - kq)]) == 15u ? c : hap_ref_code(ref[kr + (k - kq)]);      // mostly the reference
                    seq[k >> 1] = (uint8_t)(seq[k >> 1] | (c << ((k & 1) ? 0 : 4)));
                }
                uint8_t *p_seq = exact(seq), *p_qual = exact(qual), *p_ref = exact(ref);
                std::vector<int32_t> out(2 * (size_t)n);
                int32_t lowq = 0;
                const int32_t nd = twin_match_both(p_seq, p_qual, kq, p_ref, (int32_t)G, (int32_t)kr, n, 20, out.data(), &lowq);
                free(p_seq); free(p_qual); free(p_ref);
                CHECK(nd >= 0);
                diffs += nd; lows += lowq;
            }
    CHECK(diffs > 1000 && lows > 100);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_file(argv[1]);
    CHECK(sweep() == 0);
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    static const char letters[6] = {'A', 'C', 'G', 'T', 'N', 'g'};
    uint64_t keyed = 0, refs = 0, lowq = 0, over = 0, edge = 0, other = 0, lost = 0, combined = 0;
    for (int round = 0; round < 200; ++round) {
        const int32_t G = 3 + (int32_t)rnd(round % 5 == 0 ? 6 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 700 : 40);
        const int32_t mq = (int32_t)rnd(40);
        std::vector<uint8_t> ref((size_t)G);
        for (uint8_t &c : ref) c = (uint8_t)letters[rnd(rnd(10) ? 4 : 6)];
        std::vector<int32_t> start, end;
        for (int32_t p = (int32_t)rnd(3); p < G; p += (int32_t)rnd(round % 2 ? 40 : 3)) {
            const int32_t len = 1 + (int32_t)rnd(rnd(5) ? 30 : 200);
            if (p + len > G) continue;
            start.push_back(p); end.push_back(p + len);
        }
        if (start.empty()) { start.push_back(0); end.push_back(1); }
        Batch b;
        b.coff.push_back(0u); b.soff.push_back(0u);
        const int32_t pile = (int32_t)rnd((uint32_t)G);
        std::vector<int32_t> rpos;
        std::vector<std::vector<uint32_t>> rops;
        for (int64_t i = 0; i < n; ++i) {
            std::vector<uint32_t> ops;
            uint32_t L = 0;
            const uint32_t kind = rnd(10);
            if (kind < 8) {                       // regular: clips, a core of up to 9 ops, clips
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
            const int32_t p0 = where < 6 ? pile + (int32_t)rnd(4) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1);
            b.pos.push_back(p0);
            b.flag.push_back((uint16_t)(rnd(2) ? 0x10 : 0));
            b.lseq.push_back(L);
            b.status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = b.qual.size();
            for (uint32_t k = 0; k < padded; ++k) b.qual.push_back((uint8_t)(rnd(10) ? 25 + rnd(15) : rnd(40)));
            if (L && rnd(30) == 0) b.qual[q0] = 0xFF;
            // bases: the reference under the match ops (as far as the CIGAR can be followed), a few of them changed
            std::vector<uint32_t> bases(padded, 1u);
            const uint32_t noise = rnd(8) == 0 ? 3u : 50u;      // one read in eight is far from the reference
            {
                int64_t q = 0, r = p0;
                for (uint32_t v : ops) {
                    const uint32_t op = v & 15u, len = v >> 4;
                    if (op == ST_OP_M || op == ST_OP_EQ || op == ST_OP_X) {
                        for (uint32_t k = 0; k < len; ++k)
                            if (q + k < padded && r + k >= 0 && r + k < G) bases[(size_t)(q + k)] = rnd(noise) ? hap_ref_code(ref[(size_t)(r + k)]) : codes[rnd(5)];
                        q += len; r += len;
                    } else if (op == ST_OP_I || op == ST_OP_S) q += len;
                    else if (op == ST_OP_D || op == ST_OP_N) r += len;
                }
            }
            for (uint32_t k = 0; k < padded / 2; ++k) b.seq.push_back((uint8_t)((bases[2 * k] << 4) | bases[2 * k + 1]));
            b.soff.push_back((uint32_t)(b.qual.size() / 8));
        }
        Result fast, slow, tiny;
        CHECK(run(b, start, end, ref, mq, 12, 1, fast) == 0);
        CHECK(run(b, start, end, ref, mq, 12, 0, slow) == 0);
        CHECK(same_result(fast, slow) && fast.info[2] == 0);
        CHECK(run(b, start, end, ref, mq, 4, 1, tiny) == 0);           // 16 slots: what does not fit is lost, never merged
        CHECK(tiny.tally == fast.tally && tiny.info[0] <= 16 && tiny.info[0] == tiny.entries.size());
        for (const amp_hap_entry &e : tiny.entries) {
            bool found = false;
            for (const amp_hap_entry &g : fast.entries) found = found || memcmp(&e, &g, sizeof(e)) == 0;
            CHECK(found);
        }
        int64_t live = 0;
        for (uint8_t s : b.status) live += s == 0;
        CHECK((int64_t)(fast.reads[0] + fast.reads[1]) == live);
        other += fast.reads[1]; lost += tiny.info[2];
        for (size_t r = 0; r < start.size(); ++r) {
            const uint64_t *t = &fast.tally[r * HP_TALLY_COLS];
            refs += t[HP_REF]; lowq += t[HP_LOWQ]; over += t[HP_OVERFLOW]; edge += t[HP_EDGE];
        }
        uint64_t in_round = 0;
        for (const amp_hap_entry &e : fast.entries) in_round += e.count;
        keyed += in_round;
        combined += in_round > fast.info[3] ? 1 : 0;
    }
    CHECK(keyed > 1000 && refs > 1000 && lowq > 100 && over > 10 && edge > 100 && other > 100 && lost > 100 && combined > 0);
    printf("hap_twin ok\n");
    return 0;
}
#endif
