// amplicon_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_amplicon.hpp that k_amplicon calls per read,
// per tile and per base, looped over arrays on the CPU in the kernel's own order of steps: tiles of AM_BLOCK reads, the
// assignment from the original coordinates, the reads per amplicon by runs inside a wave, the waves' requests, the slots
// (resolve, flush, commit), the segment list, one add per (segment, position) into the slot's cells, the serial walk of the
// other reads, the last flush.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libamplicon_twin.so amplicon_twin.cpp   (tests/test_amplicon_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DAMPLICON_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o amplicon_twin amplicon_twin.cpp && ./amplicon_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_amplicon.hpp"

using namespace amp;

extern "C" {

int twin_window() { return AM_W; }
int twin_slots() { return AM_SLOTS; }
int twin_seg_slots() { return AM_SEG_SLOTS; }

// pos / cig_off / cig: the reads as they came in; new_pos / new_ncig / new_cig (read i's words at cig_off[i] + 3 i) and status:
// what the read pass made of them (read with do_trim; status may be null).  counts: uint32[cells][6], reads: uint64[n_amp + 1],
// both added to.  info[0..5]: reads that took a window, reads that walked serially, flushes that found a non-zero cell, adds the
// serial reads made inside a window, reads that belong to no amplicon, serial reads whose amplicon had no slot.  force_serial:
// every read walks (the windows stay empty).  Returns non-zero when a step left its bounds.
int twin_amplicon(int64_t n, const int32_t *pos, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8,
                  const uint8_t *seq, const uint8_t *qual, const uint8_t *status, const int32_t *new_pos, const uint32_t *new_ncig,
                  const uint32_t *new_cig, int32_t do_trim, int32_t ref_len, int32_t min_quality, int32_t n_amp, const int32_t *lo,
                  const int32_t *hi, const int32_t *amp_start, const int32_t *amp_end, int32_t force_serial, uint32_t *counts,
                  uint64_t *reads, int64_t *info) {
    const StrandParams P{ref_len, min_quality};
    std::vector<uint32_t> off((size_t)n_amp + 1, 0u);
    for (int32_t k = 0; k < n_amp; ++k) off[(size_t)k + 1] = off[(size_t)k] + (uint32_t)(hi[k] - lo[k]);
    const int64_t cells = off[(size_t)n_amp];
    const AmpliconTables T{ref_len, n_amp, lo, hi, off.data(), amp_start, amp_end};
    std::vector<uint32_t> cell((size_t)AM_SLOTS * AM_SLOT_WORDS, 0u);
    std::vector<AmSeg> segs((size_t)AM_BLOCK * AM_SEG_SLOTS);
    AmSlots S;
    amplicon_slots_init(S);
    int bad = 0;
    for (int k = 0; k < 6; ++k) info[k] = 0;
    auto add_global = [&](int32_t a, int64_t r, uint32_t col, uint32_t v) {
        if (a < 0 || a >= n_amp || r < lo[a] || r >= hi[a] || col >= (uint32_t)AM_COLS) { bad |= 1; return; }
        const int64_t row = (int64_t)off[(size_t)a] + (r - lo[a]);
        if (row < 0 || row >= cells) { bad |= 1; return; }
        counts[(size_t)row * AM_COLS + col] += v;
    };
    auto flush = [&](uint32_t mask) {
        for (int k = 0; k < AM_SLOTS; ++k) {
            if (!((mask >> k) & 1u)) continue;
            bool any = false;
            for (int i = 0; i < AM_SLOT_WORDS; ++i) {
                uint32_t &v = cell[(size_t)k * AM_SLOT_WORDS + (size_t)i];
                if (!v) continue;
                any = true;
                if (S.amp[k] < 0 || i % AM_STRIDE >= AM_COLS) bad |= 2;      // a free slot and the padding hold nothing
                else add_global(S.amp[k], (int64_t)S.anchor[k] + i / AM_STRIDE, (uint32_t)(i % AM_STRIDE), v);
                v = 0u;
            }
            if (any) ++info[2];
        }
    };
    for (int64_t base = 0; base < n; base += AM_BLOCK) {
        const int m = (int)(n - base < AM_BLOCK ? n - base : AM_BLOCK);
        StrandRead R[AM_BLOCK];
        StrandShape sh[AM_BLOCK];
        bool live[AM_BLOCK];
        uint32_t qual0[AM_BLOCK];
        int32_t amp[AM_BLOCK], lo_a[AM_BLOCK], hi_a[AM_BLOCK];
        for (int t = 0; t < AM_BLOCK; ++t) {
            live[t] = false; amp[t] = -1; lo_a[t] = hi_a[t] = 0; qual0[t] = 0xFFu;
            sh[t] = StrandShape{false, 0, 0};
            R[t] = StrandRead{0, cig, 0u, 0, 0u, 0ull};
            if (t >= m) continue;
            const int64_t i = base + t;
            if (status && status[i] != 0) continue;
            live[t] = true;
            const uint32_t c0 = cig_off[i];
            amp[t] = amplicon_assign(pos[i], (int64_t)pos[i] + am_cigar_ref_len(cig + c0, cig_off[i + 1] - c0), T);
            if (amp[t] < 0) { ++info[4]; continue; }
            lo_a[t] = lo[amp[t]]; hi_a[t] = hi[amp[t]];
            if (do_trim) R[t] = StrandRead{new_pos[i], new_cig + (size_t)c0 + 3 * (size_t)i, new_ncig[i], (int32_t)lseq[i], 0u, (uint64_t)seq_off8[i] * 8ull};
            else R[t] = StrandRead{pos[i], cig + c0, cig_off[i + 1] - c0, (int32_t)lseq[i], 0u, (uint64_t)seq_off8[i] * 8ull};
            if (R[t].lseq > 0) qual0[t] = qual[R[t].base];
            sh[t] = amplicon_segments(R[t], P, qual0[t], 0, [](const AmSeg &) {});
            if (force_serial) sh[t].regular = false;
        }
        // reads per amplicon: runs of equal keys inside a wave, the run's first lane adds its length
        for (int w = 0; w < AM_BLOCK / 64; ++w) {
            int l = 0;
            while (l < 64) {
                const int t = w * 64 + l;
                const int32_t key = live[t] ? (amp[t] >= 0 ? amp[t] : n_amp) : -1;
                int len = 1;
                while (l + len < 64) {
                    const int u = t + len;
                    if ((live[u] ? (amp[u] >= 0 ? amp[u] : n_amp) : -1) != key) break;
                    ++len;
                }
                if (key >= 0) reads[key] += (uint64_t)len;
                l += len;
            }
        }
        // the waves' requests
        AmReq req[AM_REQS];
        int nreq = 0;
        for (int w = 0; w < AM_BLOCK / 64; ++w) {
            bool pending[64];
            for (int l = 0; l < 64; ++l) {
                const int t = w * 64 + l;
                pending[l] = live[t] && amplicon_wants_slot(amp[t], sh[t], R[t].pos, lo_a[t], hi_a[t]);
            }
            int mine = 0;
            for (int l = 0; l < 64; ++l) {
                if (!pending[l]) continue;
                const int t = w * 64 + l;
                AmReq q{amp[t], 0x7FFFFFFF, -0x7FFFFFFF - 1, lo_a[t]};
                for (int u = l; u < 64; ++u) {
                    if (!pending[u] || amp[w * 64 + u] != q.amp) continue;
                    pending[u] = false;
                    if (R[w * 64 + u].pos < q.lo) q.lo = R[w * 64 + u].pos;
                    if (sh[w * 64 + u].ref_end > q.hi) q.hi = sh[w * 64 + u].ref_end;
                }
                if (mine < AM_REQ_PER_WAVE) { req[nreq++] = q; ++mine; }
            }
        }
        amplicon_resolve(S, req, nreq);
        if (S.flush) flush(S.flush);
        amplicon_commit(S);
        for (int k = 0; k < AM_SLOTS; ++k)
            if (S.amp[k] >= n_amp || (S.amp[k] >= 0 && (S.anchor[k] < lo[S.amp[k]] || S.anchor[k] >= hi[S.amp[k]]))) bad |= 4;
        size_t ns = 0;
        int slot[AM_BLOCK];
        for (int t = 0; t < AM_BLOCK; ++t) {
            slot[t] = live[t] ? amplicon_read_slot(S, amp[t], sh[t], R[t].pos, lo_a[t], hi_a[t]) : -1;
            if (slot[t] < 0) continue;
            ++info[0];
            amplicon_segments(R[t], P, qual0[t], slot[t], [&](const AmSeg &s) {
                if (ns < segs.size()) segs[ns++] = s; else bad |= 8;
            });
        }
        for (size_t s = 0; s < ns; ++s) {
            const AmSeg g = segs[s];
            const int k = am_seg_slot(g);
            if (k >= AM_SLOTS || !((S.used >> k) & 1u)) { bad |= 16; continue; }
            const int32_t a0 = g.r0 - S.anchor[k], a1 = a0 + am_seg_len(g);
            if (a0 < 0 || a1 > AM_W) { bad |= 32; continue; }
            for (int32_t p = a0; p < a1; ++p) {
                if (am_seg_del(g)) {
                    cell[(size_t)am_cell(k, p, 5u)] += 1u;
                } else {
                    uint32_t col, qv;
                    if (strand_base(seq, qual, g.q0 + (uint64_t)(p - a0), min_quality, col, qv)) cell[(size_t)am_cell(k, p, col)] += 1u;
                }
            }
        }
        for (int t = 0; t < AM_BLOCK; ++t) {
            if (!live[t] || amp[t] < 0 || slot[t] >= 0 || (sh[t].regular && sh[t].n_seg == 0)) continue;
            ++info[1];
            const int k = amplicon_slot_of(S, amp[t]);
            if (k < 0) ++info[5];
            const int32_t anchor = k >= 0 ? S.anchor[k] : 0;
            amplicon_walk(R[t], P, seq, qual, lo_a[t], hi_a[t], [&](int32_t r, uint32_t col) {
                const int64_t w = (int64_t)r - (int64_t)anchor;
                if (k >= 0 && w >= 0 && w < AM_W) { ++info[3]; cell[(size_t)am_cell(k, (int32_t)w, col)] += 1u; }
                else add_global(amp[t], r, col, 1u);
            });
        }
    }
    flush((1u << AM_SLOTS) - 1u);
    return bad;
}

}  // extern "C"

#ifdef AMPLICON_TWIN_MAIN
#define TWIN_NAME "amplicon_twin"
#include "twin_main.hpp"

int main() {
    static const uint32_t codes[5] = {1, 2, 4, 8, 15};
    int64_t windowed = 0, serial = 0, none = 0, no_slot = 0;
    for (int round = 0; round < 300; ++round) {
        const int32_t G = 1 + (int32_t)rnd(round % 5 == 0 ? 4 : 3000);
        const int64_t n = rnd(round % 3 == 0 ? 900 : 40);
        const int32_t mq = (int32_t)rnd(50);
        // amplicons: spans anywhere, overlapping, nested, some longer than a window; owner tables drawn from the amplicons
        // whose span covers the position (and now and then from any amplicon: the assignment must still hold the read to the span)
        const int32_t A = 1 + (int32_t)rnd(round % 4 == 0 ? 9 : 3);
        std::vector<int32_t> lo, hi, ast((size_t)G, -1), aen((size_t)G, -1);
        for (int32_t a = 0; a < A; ++a) {
            const int32_t l = (int32_t)rnd((uint32_t)G);
            const int32_t len = 1 + (int32_t)rnd(rnd(4) == 0 ? 1400u : 300u);
            lo.push_back(l); hi.push_back(l + len > G ? G : l + len);
        }
        for (int32_t p = 0; p < G; ++p) {
            for (int32_t a = 0; a < A; ++a) {
                if (p >= lo[(size_t)a] && p < lo[(size_t)a] + 25 && rnd(3)) ast[(size_t)p] = a;
                if (p < hi[(size_t)a] && p >= hi[(size_t)a] - 25 && rnd(3)) aen[(size_t)p] = a;
            }
            if (rnd(40) == 0) ast[(size_t)p] = (int32_t)rnd((uint32_t)A);
            if (rnd(40) == 0) aen[(size_t)p] = (int32_t)rnd((uint32_t)A);
        }
        std::vector<int32_t> pos, npos;
        std::vector<uint32_t> lseq, coff(1, 0u), words, soff(1, 0u), nncig, nwords;
        std::vector<uint8_t> seq, qual, status;
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
            // at an amplicon's start, anywhere, and in front of and behind the reference
            const uint32_t where = rnd(10);
            const int32_t a = (int32_t)rnd((uint32_t)A);
            const int32_t p = where < 7 ? lo[(size_t)a] + (int32_t)rnd(12) : where < 9 ? (int32_t)rnd((uint32_t)G + 30) - 15 : (int32_t)rnd(2) * (G - 1);
            pos.push_back(p);
            for (uint32_t v : ops) words.push_back(v);
            // the "trimmed" alignment: the same read, or (a first op of M and some length) that op cut down from the left, the
            // position moved along -- it lies inside the original one; the words sit at cig_off + 3 i, garbage between the slots
            const size_t slot0 = coff.back() + 3 * (size_t)i;
            nwords.resize(slot0 + ops.size() + 3, 0xFFFFFFFFu);
            uint32_t cut = 0;
            if (!ops.empty() && (ops[0] & 15u) == ST_OP_M && (ops[0] >> 4) > 2 && rnd(2)) cut = 1 + rnd((ops[0] >> 4) - 1);
            for (size_t k = 0; k < ops.size(); ++k) nwords[slot0 + k + (cut ? 1 : 0)] = k == 0 && cut ? (((ops[0] >> 4) - cut) << 4) | ST_OP_M : ops[k];
            if (cut) nwords[slot0] = (cut << 4) | ST_OP_S;
            nncig.push_back((uint32_t)ops.size() + (cut ? 1u : 0u));
            npos.push_back(p + (int32_t)cut);
            coff.push_back((uint32_t)words.size());
            lseq.push_back(L);
            status.push_back(rnd(25) == 0 ? (uint8_t)(1 + rnd(9)) : (uint8_t)0);
            const uint32_t padded = (L + 7u) & ~7u;
            const size_t q0 = qual.size();
            for (uint32_t k = 0; k < padded; ++k) qual.push_back((uint8_t)rnd(60));
            if (L && rnd(30) == 0) qual[q0] = 0xFF;
            for (uint32_t k = 0; k < padded / 2; ++k) seq.push_back((uint8_t)((codes[rnd(5)] << 4) | codes[rnd(5)]));
            soff.push_back((uint32_t)(qual.size() / 8));
        }
        nwords.resize((size_t)coff.back() + 3 * (size_t)n, 0xFFFFFFFFu);
        int32_t *p_pos = exact(pos), *p_npos = exact(npos), *p_lo = exact(lo), *p_hi = exact(hi), *p_ast = exact(ast), *p_aen = exact(aen);
        uint32_t *p_lseq = exact(lseq), *p_coff = exact(coff), *p_cig = exact(words), *p_soff = exact(soff), *p_nncig = exact(nncig), *p_ncig = exact(nwords);
        uint8_t *p_seq = exact(seq), *p_qual = exact(qual), *p_st = exact(status);
        int64_t cells = 0;
        for (int32_t a = 0; a < A; ++a) cells += hi[(size_t)a] - lo[(size_t)a];
        for (int trim = 0; trim < 2; ++trim) {
            uint32_t *cnt[2]; uint64_t *rd[2];
            int64_t info[2][6];
            for (int mode = 0; mode < 2; ++mode) {
                cnt[mode] = (uint32_t *)calloc((size_t)cells * AM_COLS, 4); rd[mode] = (uint64_t *)calloc((size_t)A + 1, 8);
                CHECK(twin_amplicon(n, p_pos, p_lseq, p_coff, p_cig, p_soff, p_seq, p_qual, p_st, p_npos, p_nncig, p_ncig, trim, G, mq, A, p_lo, p_hi, p_ast,
                                    p_aen, mode, cnt[mode], rd[mode], info[mode]) == 0);
            }
            // the windows and the walk agree on every read, and the all-serial run never touches the segments
            CHECK(memcmp(cnt[0], cnt[1], (size_t)cells * AM_COLS * 4) == 0 && memcmp(rd[0], rd[1], ((size_t)A + 1) * 8) == 0);
            CHECK(info[1][0] == 0 && info[0][4] == info[1][4]);
            uint64_t total = 0, live = 0;
            for (int32_t a = 0; a <= A; ++a) total += rd[0][a];
            for (int64_t i = 0; i < n; ++i) live += status[(size_t)i] == 0;
            CHECK(total == live && rd[0][A] == (uint64_t)info[0][4]);
            windowed += info[0][0]; serial += info[0][1]; none += info[0][4]; no_slot += info[0][5];
            for (int mode = 0; mode < 2; ++mode) { free(cnt[mode]); free(rd[mode]); }
        }
        free(p_pos); free(p_npos); free(p_lo); free(p_hi); free(p_ast); free(p_aen); free(p_lseq); free(p_coff); free(p_cig); free(p_soff);
        free(p_nncig); free(p_ncig); free(p_seq); free(p_qual); free(p_st);
    }
    CHECK(windowed > 1000 && serial > 1000 && none > 1000 && no_slot > 0);
    printf("amplicon_twin ok\n");
    return 0;
}
#endif
