// del_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_del.hpp that k_del calls, looped over arrays on the
// CPU in the kernel's own order of steps: tiles of DL_BLOCK reads, a read's shape and events (from the CIGAR words when it is
// regular, the walk otherwise), the tile's list, equal keys of 64 list entries combined, the leaders into the block's table
// with the real hash and probe rule, the three-quarters flush at the tile boundary, the straight-to-global paths, the global
// table with its bounded probe count and its `lost` counter.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libdel_twin.so del_twin.cpp   (tests/test_del_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DDEL_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o del_twin del_twin.cpp && ./del_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_del.hpp"

using namespace amp;

extern "C" {

int twin_del_constant(int which) {
    static const int v[] = {DL_BLOCK, DL_LIST, DL_LDS_SLOTS, DL_LDS_PROBES, DL_LDS_FLUSH_AT, DL_GLOBAL_PROBES, DL_LOG2_DEFAULT, DL_LOG2_MIN, DL_LOG2_MAX, ST_SLOTS};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
uint64_t twin_del_key(int32_t start, int32_t len) { return del_key(start, len); }
uint32_t twin_del_slot_lds(uint64_t key) { return del_slot_lds(key); }
uint32_t twin_del_slot_global(uint64_t key, uint32_t log2_capacity) { return del_slot_global(key, log2_capacity); }
uint32_t twin_del_probes_global(uint32_t log2_capacity) { return del_probes_global(log2_capacity); }

enum { I_REGULAR, I_WALKED, I_LIST_FULL, I_LDS_PAST, I_FLUSH_FULL, I_COMBINED, I_USED, I_LOST, I_QUAL_READS, I_LDS_INSERTS, N_INFO };

// The reads are given as they are walked (with do_trim: the trimmed pos and CIGAR).  keys: uint64[2^log2_capacity] (DL_EMPTY:
// free), cnt: uint32[2^log2_capacity][2]; both are added to, so that a second call is a second batch.  info[N_INFO]: reads whose
// events came from the CIGAR words, reads that walked, events the list had no room for, inserts that went past the block's
// table, flushes at a tile boundary, list entries a leader took along, slots claimed in the global table, reads lost, first
// quality bytes looked at on behalf of regular reads, inserts into the block's table.  force_serial: every read walks.
// Returns non-zero when a step left its bounds.
int twin_del(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
             const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
             uint32_t log2_capacity, int32_t force_serial, uint64_t *keys, uint32_t *cnt, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    std::vector<uint64_t> s_key((size_t)DL_LDS_SLOTS, DL_EMPTY), s_list((size_t)DL_LIST);
    std::vector<uint32_t> s_cnt((size_t)DL_LDS_SLOTS * 2, 0u);
    uint32_t s_used = 0;
    int bad = 0;
    for (int k = 0; k < N_INFO; ++k) info[k] = 0;
    const uint32_t mask = (1u << log2_capacity) - 1u;
    auto global_insert = [&](uint64_t key, uint32_t count, uint32_t rev) {
        if (key == DL_EMPTY || del_key_len(key) < 1 || del_key_start(key) < 0 || (int64_t)del_key_start(key) + del_key_len(key) > ref_len) bad |= 1;
        const int64_t s = del_probe(key, del_slot_global(key, log2_capacity), mask, del_probes_global(log2_capacity), [&](uint32_t slot) {
            if (slot > mask) { bad |= 2; return key; }
            const uint64_t prev = keys[slot];
            if (prev == DL_EMPTY) { keys[slot] = key; ++info[I_USED]; }
            return prev;
        });
        if (s < 0) { info[I_LOST] += count; return; }
        cnt[2 * s] += count; cnt[2 * s + 1] += rev;
    };
    auto lds_insert = [&](uint64_t key, uint32_t count, uint32_t rev) {
        const int64_t s = del_probe(key, del_slot_lds(key), (uint32_t)(DL_LDS_SLOTS - 1), (uint32_t)DL_LDS_PROBES, [&](uint32_t slot) {
            if (slot >= (uint32_t)DL_LDS_SLOTS) { bad |= 4; return key; }
            const uint64_t prev = s_key[slot];
            if (prev == DL_EMPTY) { s_key[slot] = key; ++s_used; }
            return prev;
        });
        if (s < 0) { ++info[I_LDS_PAST]; global_insert(key, count, rev); return; }
        ++info[I_LDS_INSERTS];
        s_cnt[2 * (size_t)s] += count; s_cnt[2 * (size_t)s + 1] += rev;
    };
    auto flush = [&]() {
        for (int k = 0; k < DL_LDS_SLOTS; ++k) {
            if (s_key[(size_t)k] == DL_EMPTY) continue;
            global_insert(s_key[(size_t)k], s_cnt[2 * (size_t)k], s_cnt[2 * (size_t)k + 1]);
            s_key[(size_t)k] = DL_EMPTY; s_cnt[2 * (size_t)k] = 0u; s_cnt[2 * (size_t)k + 1] = 0u;
        }
        s_used = 0;
    };
    for (int64_t base = 0; base < n; base += DL_BLOCK) {
        const int m = (int)(n - base < DL_BLOCK ? n - base : DL_BLOCK);
        // ---- phase A
        uint32_t s_n = 0;
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            if (status && status[i] != 0) continue;
            const StrandRead R{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], (flag[i] & 0x10u) ? 1u : 0u, (uint64_t)seq_off8[i] * 8ull};
            auto put = [&](int32_t start, int32_t len) {
                const uint64_t key = del_key(start, len);
                const uint32_t slot = s_n++;
                if (slot < (uint32_t)DL_LIST) s_list[slot] = key | (R.rev ? DL_REV_BIT : 0ull);
                else { ++info[I_LIST_FULL]; global_insert(key, 1u, R.rev); }
            };
            int32_t n_ev = 0;
            StrandShape sh = del_events_regular(R, P, [&](int32_t, int32_t) { ++n_ev; });
            if (del_qual_needed(sh, n_ev)) { ++info[I_QUAL_READS]; if (qual[R.base] == 0xFFu) sh.regular = false; }
            if (force_serial) sh.regular = false;
            if (!sh.regular) { ++info[I_WALKED]; del_events_walk(R, P, seq, qual, put); }
            else { ++info[I_REGULAR]; if (n_ev > 0) del_events_regular(R, P, put); }
        }
        // ---- phase B
        const uint32_t ns = s_n < (uint32_t)DL_LIST ? s_n : (uint32_t)DL_LIST;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {
            const uint32_t lanes = ns - s0 < 64u ? ns - s0 : 64u;
            uint64_t pending = lanes == 64u ? ~0ull : ((1ull << lanes) - 1ull);
            while (pending) {
                const int src = __builtin_ctzll(pending);
                const uint64_t lk = s_list[s0 + (uint32_t)src] & ~DL_REV_BIT;
                uint64_t same = 0ull, revs = 0ull;
                for (uint32_t l = 0; l < lanes; ++l) {
                    const uint64_t e = s_list[s0 + l];
                    if ((e & ~DL_REV_BIT) == lk) { same |= 1ull << l; if (e & DL_REV_BIT) revs |= 1ull << l; }
                }
                if ((same & pending) != same) bad |= 8;
                lds_insert(lk, (uint32_t)__builtin_popcountll(same), (uint32_t)__builtin_popcountll(revs));
                info[I_COMBINED] += __builtin_popcountll(same) - 1;
                pending &= ~same;
            }
        }
        // ---- the tile boundary
        if (s_used > (uint32_t)DL_LDS_FLUSH_AT) { ++info[I_FLUSH_FULL]; flush(); }
    }
    flush();
    return bad;
}

}  // extern "C"

#ifdef DEL_TWIN_MAIN
#define TWIN_NAME "del_twin"
#include "twin_main.hpp"

int main() {
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    int64_t regular = 0, walked = 0, combined = 0, lost_runs = 0, past = 0;
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 1 + (int32_t)rnd(round % 5 == 0 ? 4 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 900 : 40);
        const int32_t mq = (int32_t)rnd(50);
        const uint32_t log2cap = round % 4 == 0 ? 4u : 12u;
        std::vector<int32_t> pos;
        std::vector<uint16_t> flag;
        std::vector<uint32_t> lseq, coff(1, 0u), words, soff(1, 0u);
        std::vector<uint8_t> seq, qual, status;
        int32_t pile = (int32_t)rnd((uint32_t)G);
        for (int64_t i = 0; i < n; ++i) {
            std::vector<uint32_t> ops;
            uint32_t L = 0;
            const uint32_t kind = rnd(10);
            if (kind < 3) {                       // a pile's own deletion: many reads, one key
                ops.push_back((20u << 4) | ST_OP_M); ops.push_back((3u << 4) | ST_OP_D); ops.push_back((20u << 4) | ST_OP_M);
            } else if (kind < 7) {                // regular: clips, a core of up to 9 ops, clips
                if (rnd(4) == 0) ops.push_back((rnd(5) << 4) | ST_OP_H);
                if (rnd(3) == 0) ops.push_back((rnd(9) << 4) | ST_OP_S);
                const uint32_t core = 1 + rnd(kind == 3 ? 9 : 3);
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
            const uint32_t where = rnd(10);
            pos.push_back(kind < 3 ? pile : where < 6 ? pile + (int32_t)rnd(40) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1));
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
        const size_t cap = (size_t)1 << log2cap;
        uint64_t *keys[2]; uint32_t *cnt[2];
        int64_t info[2][N_INFO];
        std::vector<uint32_t> dash[2], rev[2];
        for (int mode = 0; mode < 2; ++mode) {
            keys[mode] = (uint64_t *)malloc(cap * 8); memset(keys[mode], 0xFF, cap * 8);
            cnt[mode] = (uint32_t *)calloc(cap * 2, 4);
            CHECK(twin_del(n, p_pos, p_flag, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, p_st, G, mq, log2cap, mode, keys[mode], cnt[mode], info[mode]) == 0);
            // what the table holds, per position
            dash[mode].assign((size_t)G, 0u); rev[mode].assign((size_t)G, 0u);
            int64_t used = 0;
            for (size_t s = 0; s < cap; ++s) {
                if (keys[mode][s] == DL_EMPTY) { CHECK(cnt[mode][2 * s] == 0 && cnt[mode][2 * s + 1] == 0); continue; }
                ++used;
                CHECK(cnt[mode][2 * s] > 0 && cnt[mode][2 * s + 1] <= cnt[mode][2 * s]);
                for (int32_t p = del_key_start(keys[mode][s]); p < del_key_start(keys[mode][s]) + del_key_len(keys[mode][s]); ++p) {
                    dash[mode][(size_t)p] += cnt[mode][2 * s]; rev[mode][(size_t)p] += cnt[mode][2 * s + 1];
                }
            }
            CHECK(used == info[mode][I_USED]);
        }
        // the CIGAR words and the walk agree on every read, and the all-serial run never takes the regular path
        CHECK(info[1][I_REGULAR] == 0 && info[0][I_REGULAR] + info[0][I_WALKED] == info[1][I_WALKED]);
        if (info[0][I_LOST] == 0 && info[1][I_LOST] == 0) {
            CHECK(dash[0] == dash[1] && rev[0] == rev[1]);
            // ... and the per-position sums are the '-' column of the strand walk
            std::vector<uint32_t> want((size_t)G, 0u);
            const StrandParams P{G, mq};
            for (int64_t i = 0; i < n; ++i) {
                if (p_st[i]) continue;
                const StrandRead R{p_pos[i], p_cig + p_coff[i], p_coff[i + 1] - p_coff[i], (int32_t)p_lseq[i], 0u, (uint64_t)p_soff[i] * 8ull};
                strand_walk(R, P, p_seq, p_qual, [&](int32_t r, uint32_t col, uint32_t) { if (col == 5u) ++want[(size_t)r]; });
            }
            CHECK(dash[0] == want);
        } else {
            CHECK(info[0][I_USED] == (int64_t)cap || log2cap > 4u);
            ++lost_runs;
        }
        regular += info[0][I_REGULAR]; walked += info[0][I_WALKED]; combined += info[0][I_COMBINED]; past += info[0][I_LDS_PAST];
        free(p_pos); free(p_flag); free(p_lseq); free(p_coff); free(p_cig); free(p_soff); free(p_seq); free(p_qual); free(p_st);
        for (int mode = 0; mode < 2; ++mode) { free(keys[mode]); free(cnt[mode]); }
    }
    CHECK(regular > 1000 && walked > 1000 && combined > 1000 && lost_runs > 0);
    (void)past;
    printf("del_twin ok\n");
    return 0;
}
#endif
