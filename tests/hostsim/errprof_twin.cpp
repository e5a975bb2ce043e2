// errprof_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_errprof.hpp that k_errprof calls, looped over
// arrays on the CPU in the kernel's own order of steps: tiles of EP_BLOCK reads; per read the scan, then its segments onto the
// tile's list or the serial walk; per list entry 64 lanes at a time on consecutive bases, each lane's own cycle cell, the
// clamped lanes and the quality and substitution keys combined per distinct key; the flush of the block's u32 cells into the
// u64 tables.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fPIC -shared -I amplipy_amd/csrc -o liberrprof_twin.so errprof_twin.cpp   (tests/test_errprof_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DERRPROF_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o errprof_twin errprof_twin.cpp
//   ./errprof_twin [cases.bin]
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python.  With
// a file (written by tests/test_errprof_twin.py: the crafted cases with the tables the restatement expects) it runs every case
// from heap blocks of exactly the needed size and compares; without one it runs seeded batches of regular and arbitrary CIGARs,
// on which the segment path and an all-serial walk must agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_errprof.hpp"

using namespace amp;

extern "C" {

int twin_cells() { return EP_CELLS; }
int twin_slots() { return EP_SLOTS; }
int twin_block() { return EP_BLOCK; }
int twin_lds_lseq() { return EP_LDS_LSEQ; }
int twin_cycles() { return EP_CYCLES; }
int twin_quals() { return EP_QUALS; }

void twin_ref_codes(const uint8_t *ref_ascii, const uint32_t *mask_bits, int32_t ref_len, uint8_t *code) { errprof_ref_codes(ref_ascii, mask_bits, ref_len, code); }

static StrandRead read_of(int64_t i, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                          const uint32_t *seq_off8) {
    return StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], (flag[i] & 0x10u) ? 1u : 0u, (uint64_t)seq_off8[i] * 8ull};
}

// The reads are given as they are counted (with do_trim: the trimmed pos and CIGAR).  cells: uint64[EP_CELLS + 2] -- cyc, qualt,
// sub in the ABI's layout, then reads[2] -- added to.  info[0..4]: list entries, reads walked serially into the block's cells,
// reads walked into the tables, trips of the combine loops, flushes.  Returns non-zero when a step left its bounds or two lanes
// of a step met on one cell.
int twin_errprof(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                 const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                 const uint8_t *code, uint64_t *cells, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    std::vector<uint32_t> cell((size_t)EP_CELLS, 0u);
    std::vector<EpSeg> list;
    int bad = 0, since = 0;
    for (int k = 0; k < 5; ++k) info[k] = 0;
    auto flush = [&]() {
        ++info[4];
        for (int k = 0; k < EP_CELLS; ++k) {
            const int g = ep_block_to_global(k);
            if (g < 0 || g >= EP_CELLS) { bad |= 1; continue; }
            cells[g] += cell[(size_t)k];
            cell[(size_t)k] = 0u;
        }
    };
    auto block_add = [&](int k, uint32_t v) {
        if (k < 0 || k >= EP_CELLS) { bad |= 2; return; }
        if ((uint64_t)cell[(size_t)k] + v > 0xFFFFFFFFull) bad |= 4;
        cell[(size_t)k] += v;
    };
    // the lanes with have[l] and equal key[l]: one add of their number per distinct key, all of them different cells
    auto combine = [&](const bool *have, const int *key) {
        bool done[64] = {false};
        for (int l = 0; l < 64; ++l) {
            if (!have[l] || done[l]) continue;
            uint32_t cnt = 0;
            for (int o = l; o < 64; ++o) if (have[o] && key[o] == key[l]) { done[o] = true; ++cnt; }
            ++info[3];
            block_add(key[l], cnt);
        }
    };
    for (int64_t base = 0; base < n; base += EP_BLOCK) {
        const int m = (int)(n - base < EP_BLOCK ? n - base : EP_BLOCK);
        if (since >= EP_MAX_TILES_PER_FLUSH) { flush(); since = 0; }
        ++since;
        list.clear();
        // ---- phase A
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            if (status && status[i] != 0) continue;
            const StrandRead R = read_of(i, pos, flag, lseq, cig_off, cig, seq_off8);
            const uint32_t qual0 = R.lseq > 0 ? qual[R.base] : 0xFFu;
            const uint32_t mate = (flag[i] & 0x80u) ? 1u : 0u;
            const StrandShape sh = errprof_segments(R, P, qual0, mate, [](const EpSeg &) {});
            if (!sh.regular) { ++cells[EP_CELLS + 1]; continue; }
            ++cells[EP_CELLS];
            if (ep_read_listed(sh, R.lseq)) {
                if (sh.n_seg > EP_SLOTS) bad |= 8;
                errprof_segments(R, P, qual0, mate, [&](const EpSeg &g) { list.push_back(g); });
                continue;
            }
            const bool in_block = ep_read_in_block(R.lseq);
            ++info[in_block ? 1 : 2];
            errprof_segments(R, P, qual0, mate, [&](const EpSeg &g) {
                if ((int64_t)g.r0 < 0 || (int64_t)g.r0 + g.len > ref_len || g.q0 < R.base || g.q0 + g.len > R.base + (uint64_t)R.lseq) { bad |= 16; return; }
                errprof_seg_walk(g, seq, qual, code, min_quality, [&](int kc, int kq, int ks) {
                    if (in_block) { block_add(kc, 1u); block_add(kq, 1u); block_add(ks, 1u); }
                    else { cells[ep_block_to_global(kc)] += 1; cells[kq] += 1; cells[ks] += 1; }
                });
            });
        }
        if (list.size() > (size_t)EP_BLOCK * EP_SLOTS) bad |= 32;
        // ---- phase B
        info[0] += (int64_t)list.size();
        for (const EpSeg &g : list) {
            if ((int64_t)g.r0 < 0 || (int64_t)g.r0 + g.len > ref_len) { bad |= 64; continue; }
            for (uint32_t j0 = 0; j0 < g.len; j0 += 64u) {
                bool part[64], open_end[64];
                int kc[64], kq[64], ks[64];
                for (int l = 0; l < 64; ++l) {
                    const uint32_t j = j0 + (uint32_t)l;
                    part[l] = false; kc[l] = kq[l] = ks[l] = 0;
                    int32_t c = 0;
                    if (j < g.len) {
                        const uint64_t k = g.q0 + j;
                        c = ep_seg_cycle(g, j);
                        if (c < 0) bad |= 128;
                        part[l] = errprof_base(st_base_code(seq, k), code[(int64_t)g.r0 + j], qual[k], ep_seg_mate(g), ep_seg_rev(g), c, min_quality, kc[l], kq[l], ks[l]);
                    }
                    open_end[l] = part[l] && c >= EP_CYCLES - 1;
                }
                for (int l = 0; l < 64; ++l) {
                    if (!part[l] || open_end[l]) continue;
                    for (int o = 0; o < l; ++o) if (part[o] && !open_end[o] && kc[o] == kc[l]) bad |= 256;     // each lane its own cell
                    block_add(kc[l], 1u);
                }
                combine(open_end, kc);
                combine(part, kq);
                combine(part, ks);
            }
        }
    }
    flush();
    return bad;
}

// Every regular read base by base, straight into the tables: the same adds.
int twin_errprof_serial(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                        const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                        const uint8_t *code, uint64_t *cells) {
    const StrandParams P{ref_len, min_quality};
    int bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (status && status[i] != 0) continue;
        const StrandRead R = read_of(i, pos, flag, lseq, cig_off, cig, seq_off8);
        const uint32_t qual0 = R.lseq > 0 ? qual[R.base] : 0xFFu;
        const uint32_t mate = (flag[i] & 0x80u) ? 1u : 0u;
        const StrandShape sh = errprof_segments(R, P, qual0, mate, [](const EpSeg &) {});
        ++cells[EP_CELLS + (sh.regular ? 0 : 1)];
        if (!sh.regular) continue;
        errprof_segments(R, P, qual0, mate, [&](const EpSeg &g) {
            errprof_seg_walk(g, seq, qual, code, min_quality, [&](int kc, int kq, int ks) {
                const int gc = ep_block_to_global(kc);
                if (gc < 0 || gc >= EP_CYC_CELLS || kq < EP_QUAL_AT || kq >= EP_SUB_AT || ks < EP_SUB_AT || ks >= EP_CELLS) { bad |= 1; return; }
                cells[gc] += 1; cells[kq] += 1; cells[ks] += 1;
            });
        });
    }
    return bad;
}

}  // extern "C"

#ifdef ERRPROF_TWIN_MAIN
#define TWIN_NAME "errprof_twin"
#include "twin_main.hpp"

struct Batch {
    std::vector<int32_t> pos;
    std::vector<uint16_t> flag;
    std::vector<uint32_t> lseq, coff, words, soff;
    std::vector<uint8_t> seq, qual, status;
};

// the segment path and the all-serial walk must agree; -> 0, or the line of what failed
static int run(const Batch &b, const std::vector<uint8_t> &ref, const std::vector<uint32_t> &mask, int32_t mq, std::vector<uint64_t> &tab, int64_t info[5]) {
    const int64_t n = (int64_t)b.pos.size();
    const int32_t G = (int32_t)ref.size();
    int32_t *p_pos = exact(b.pos);
    uint16_t *p_flag = exact(b.flag);
    uint32_t *p_lseq = exact(b.lseq), *p_coff = exact(b.coff), *p_cig = exact(b.words), *p_soff = exact(b.soff), *p_mask = exact(mask);
    uint8_t *p_seq = exact(b.seq), *p_qual = exact(b.qual), *p_status = exact(b.status), *p_ref = exact(ref);
    std::vector<uint8_t> code_v((size_t)G, 0);
    uint8_t *p_code = exact(code_v);
    twin_ref_codes(p_ref, mask.empty() ? nullptr : p_mask, G, p_code);
    tab.assign((size_t)EP_CELLS + 2, 0ull);
    uint64_t *t0 = exact(tab), *t1 = exact(tab);
    const int bad0 = twin_errprof(n, p_pos, p_flag, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, b.status.empty() ? nullptr : p_status, G, mq, p_code, t0, info);
    const int bad1 = twin_errprof_serial(n, p_pos, p_flag, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, b.status.empty() ? nullptr : p_status, G, mq, p_code, t1);
    const bool same = memcmp(t0, t1, tab.size() * 8) == 0;
    memcpy(tab.data(), t0, tab.size() * 8);
    free(p_pos); free(p_flag); free(p_lseq); free(p_coff); free(p_cig); free(p_soff); free(p_mask); free(p_seq); free(p_qual); free(p_status); free(p_ref);
    free(p_code); free(t0); free(t1);
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

// the file: int32 n_cases; per case int32 mq; then the vectors (int64 count, elements): pos, flag, lseq, cig_off, cig, seq_off8,
// seq, qual, the reference letters, the mask words (none: no mask), the expected cells (uint64[EP_CELLS + 2])
static int run_file(const char *fn) {
    FILE *f = fopen(fn, "rb");
    CHECK(f != nullptr);
    int32_t n_cases = 0;
    CHECK(fread(&n_cases, 4, 1, f) == 1);
    for (int32_t k = 0; k < n_cases; ++k) {
        int32_t mq;
        CHECK(fread(&mq, 4, 1, f) == 1);
        Batch b;
        std::vector<uint8_t> ref;
        std::vector<uint32_t> mask;
        std::vector<uint64_t> want, got;
        CHECK(rd_vec(f, b.pos) && rd_vec(f, b.flag) && rd_vec(f, b.lseq) && rd_vec(f, b.coff) && rd_vec(f, b.words) && rd_vec(f, b.soff) && rd_vec(f, b.seq) && rd_vec(f, b.qual));
        CHECK(rd_vec(f, ref) && rd_vec(f, mask) && rd_vec(f, want));
        CHECK(want.size() == (size_t)EP_CELLS + 2 && (mask.empty() || mask.size() == (ref.size() + 31) / 32));
        int64_t info[5];
        CHECK(run(b, ref, mask, mq, got, info) == 0);
        if (got != want) { printf("errprof_twin: case %d differs from the expected tables\n", k); fclose(f); return 1; }
    }
    fclose(f);
    printf("errprof_twin ok: %d cases\n", n_cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_file(argv[1]);
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    static const char letters[] = "ACGTacgtNnRY";
    int64_t listed = 0, serial = 0, skipped = 0, open_bin = 0, mism = 0;
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 1 + (int32_t)rnd(round % 5 == 0 ? 6 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 700 : 40);
        const int32_t mq = (int32_t)rnd(50);
        std::vector<uint8_t> ref((size_t)G);
        for (auto &c : ref) c = (uint8_t)letters[rnd(rnd(6) ? 4 : 12)];
        std::vector<uint32_t> mask;
        if (rnd(2)) { mask.assign(((size_t)G + 31) / 32, 0u); for (uint32_t k = rnd(20); k--;) { const uint32_t p = rnd((uint32_t)G); mask[p >> 5] |= 1u << (p & 31); } }
        Batch b;
        b.coff.push_back(0u); b.soff.push_back(0u);
        int32_t pile = (int32_t)rnd((uint32_t)G);
        for (int64_t i = 0; i < n; ++i) {
            std::vector<uint32_t> ops;
            uint32_t L = 0;
            const uint32_t kind = rnd(10);
            if (kind < 7) {                       // regular: clips, a core of up to 13 ops, clips
                if (rnd(4) == 0) ops.push_back((rnd(5) << 4) | ST_OP_H);
                if (rnd(3) == 0) ops.push_back((rnd(9) << 4) | ST_OP_S);
                const uint32_t core = 1 + rnd(kind == 0 ? 13 : 3);
                for (uint32_t k = 0; k < core; ++k) {
                    static const uint32_t pick[7] = {ST_OP_M, ST_OP_M, ST_OP_EQ, ST_OP_X, ST_OP_I, ST_OP_D, ST_OP_N};
                    ops.push_back((rnd(k % 2 ? 6 : (kind == 1 ? 700 : 90)) << 4) | pick[rnd(k == 0 ? 4 : 7)]);
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
            b.flag.push_back((uint16_t)((rnd(2) ? 0x10u : 0u) | (rnd(3) == 0 ? 0x80u : 0u) | (rnd(2) ? 0x1u : 0u)));
            b.lseq.push_back(L);
            b.status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = b.qual.size();
            const uint32_t qmode = rnd(3);        // one quality, a few bins, anything
            const uint8_t q1 = (uint8_t)rnd(255);
            for (uint32_t k = 0; k < padded; ++k) b.qual.push_back(qmode == 0 ? q1 : qmode == 1 ? (uint8_t)(2 + 12 * rnd(4)) : (uint8_t)rnd(255));
            if (L && rnd(30) == 0) b.qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) b.seq.push_back((uint8_t)((codes[rnd(rnd(4) ? 4 : 5)] << 4) | codes[rnd(rnd(4) ? 4 : 5)]));
            b.soff.push_back((uint32_t)(b.qual.size() / 8));
        }
        std::vector<uint64_t> tab;
        int64_t info[5];
        CHECK(run(b, ref, mask, mq, tab, info) == 0);
        int64_t live = 0;
        for (uint8_t s : b.status) live += s == 0;
        CHECK((int64_t)(tab[EP_CELLS] + tab[EP_CELLS + 1]) == live);
        for (int m = 0; m < 2; ++m) {            // the three tables hold the same bases per mate
            uint64_t sc = 0, sq = 0, ss = 0;
            for (int k = 0; k < EP_CYC_CELLS / 2; ++k) sc += tab[(size_t)(m * (EP_CYC_CELLS / 2) + k)];
            for (int k = 0; k < EP_QUAL_CELLS / 2; ++k) sq += tab[(size_t)(EP_QUAL_AT + m * (EP_QUAL_CELLS / 2) + k)];
            for (int k = 0; k < EP_SUB_CELLS / 2; ++k) ss += tab[(size_t)(EP_SUB_AT + m * (EP_SUB_CELLS / 2) + k)];
            CHECK(sc == sq && sq == ss);
        }
        listed += info[0]; serial += info[1]; skipped += (int64_t)tab[EP_CELLS + 1];
        for (int m = 0; m < 2; ++m) for (int e = 0; e < 2; ++e) open_bin += (int64_t)tab[(size_t)ep_cyc_cell((uint32_t)m, EP_CYCLES - 1, (uint32_t)e)];
        for (int k = 1; k < EP_CYC_CELLS; k += 2) mism += (int64_t)tab[(size_t)k];
    }
    CHECK(listed > 1000 && serial > 20 && skipped > 100 && open_bin > 100 && mism > 1000);
    printf("errprof_twin ok\n");
    return 0;
}
#endif
