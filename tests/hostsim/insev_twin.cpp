// insev_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_insev.hpp that k_insev calls, looped over arrays on
// the CPU in the kernel's own order of steps: this batch's slots of the eight shard regions between cursor and counter, 64 of
// them at a time, the guards, a used event's key and cells, equal keys of the 64 combined, the leader's ONE insert with the real
// hash and the word-by-word probe rule, the bounded probe count and the `lost` counter.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libinsev_twin.so insev_twin.cpp   (tests/test_insev_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DINSEV_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o insev_twin insev_twin.cpp && ./insev_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amp_insev.hpp"

using namespace amp;

extern "C" {

int twin_insev_constant(int which) {
    static const int v[] = {IE_BLOCK, IE_GRID, IE_BINS, IE_LOG2_DEFAULT, IE_LOG2_MIN, IE_LOG2_MAX, (int)sizeof(InsevSide), (int)sizeof(amp_insev_entry), AMP_INSEV_STRIDE};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
// the allele hash of n base codes, a byte each
uint64_t twin_insev_allele_hash(const uint8_t *codes, int32_t n) {
    uint64_t h = ins_hash_seed();
    for (int32_t k = 0; k < n; ++k) h = ins_hash_step(h, codes[k]);
    return ins_hash_final(h);
}
int32_t twin_insev_d(int32_t q_from, int32_t q_to, int32_t qs, int32_t qe) { return insev_d(q_from, q_to, qs, qe); }
uint32_t twin_insev_bin(int32_t d) { return rp_bin(d); }
uint32_t twin_insev_slot(uint64_t k0, uint64_t k1, uint32_t log2_capacity) {
    const uint64_t key[2] = {k0, k1};
    return keyed_slot(insev_hash(key), log2_capacity);
}

enum { I_SLOTS, I_UNUSED, I_GUARDED, I_EVENTS, I_INSERTS, I_COMBINED, I_USED, I_LOST, N_INFO };

// The reads are given as they were counted (with do_trim: the trimmed CIGAR); status may be null.  ev: the list's eight regions of
// `cap` entries, shard_n / cursor: uint64[8].  keys: uint64[2^log2_capacity][2] (IE_EMPTY: free), cnt: uint32[..][2], side:
// InsevSide[..]; all are added to, so that a second call is a second batch.  info[N_INFO]: slots visited, of them unused,
// dropped by a guard, tallied; inserts made, entries a leader took along, slots claimed, events lost.  Non-zero when a step
// left its bounds.
int twin_insev(int64_t n, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig, const uint32_t *seq_off8, const uint8_t *seq,
               const uint8_t *qual, const uint8_t *status, uint64_t read_base, const amp_ins_event *ev, long long cap, const unsigned long long *shard_n,
               const unsigned long long *cursor, uint32_t log2_capacity, uint64_t *keys, uint32_t *cnt, InsevSide *side, int64_t *info) {
    int bad = 0;
    for (int k = 0; k < N_INFO; ++k) info[k] = 0;
    const uint32_t mask = (1u << log2_capacity) - 1u;
    const InsevSpan M = insev_span(cap, cursor, shard_n);
    const int64_t total = M.start[8];
    struct Lane { bool have; uint64_t key[2]; InsevCells c; };
    for (int64_t j0 = 0; j0 < total; j0 += 64) {
        Lane L[64];
        const int lanes = (int)(total - j0 < 64 ? total - j0 : 64);
        for (int l = 0; l < 64; ++l) {
            L[l].have = false;
            if (l >= lanes) continue;
            ++info[I_SLOTS];
            const size_t at = insev_span_at(M, j0 + l);
            if (at >= (size_t)8 * (size_t)cap) { bad |= 1; continue; }
            const amp_ins_event e = ev[at];
            if (ins_unused(e)) { ++info[I_UNUSED]; continue; }
            const int64_t i = ins_read_row(e.read, read_base);
            if (!(i < n && (!status || status[i] == 0) && e.q_from >= 0 && e.q_from <= e.q_to && e.q_to <= (int32_t)lseq[i])) { ++info[I_GUARDED]; continue; }
            L[l].have = true;
            ++info[I_EVENTS];
            insev_key(seq, seq_off8, read_base, e, L[l].key);
            L[l].c = insev_cells(e, cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], flag[i], qual, (uint64_t)seq_off8[i] * 8ull);
            if (L[l].c.bin >= (uint32_t)IE_BINS) bad |= 2;
        }
        uint64_t pending = 0;
        for (int l = 0; l < 64; ++l) if (L[l].have) pending |= 1ull << l;
        while (pending) {
            const int src = __builtin_ctzll(pending);
            uint64_t same = 0;
            uint32_t count = 0, rev = 0, noqual = 0, bin[IE_BINS] = {0, 0, 0, 0, 0, 0, 0};
            uint64_t qsum = 0;
            for (int l = 0; l < 64; ++l) {
                if (!L[l].have || L[l].key[0] != L[src].key[0] || L[l].key[1] != L[src].key[1]) continue;
                same |= 1ull << l;
                ++count; rev += L[l].c.rev; noqual += L[l].c.noqual; qsum += L[l].c.qsum; ++bin[L[l].c.bin];
            }
            if ((same & pending) != same) bad |= 4;
            pending &= ~same;
            ++info[I_INSERTS];
            info[I_COMBINED] += count - 1;
            bool fresh;
            const int64_t s = insev_probe(L[src].key, keyed_slot(insev_hash(L[src].key), log2_capacity), mask, keyed_probes(log2_capacity),
                                          [&](uint32_t slot, int w, uint64_t v) {
                                              if (slot > mask) { bad |= 8; return v; }
                                              uint64_t &word = keys[(size_t)slot * 2 + (size_t)w];
                                              const uint64_t prev = word;
                                              if (prev == IE_EMPTY) word = v;
                                              return prev;
                                          }, fresh);
            if (s < 0) { info[I_LOST] += count; continue; }
            if (fresh) ++info[I_USED];
            cnt[2 * s] += count; cnt[2 * s + 1] += rev;
            side[s].noqual += noqual; side[s].qsum += qsum;
            for (int b = 0; b < IE_BINS; ++b) side[s].bin[b] += bin[b];
        }
    }
    return bad;
}

}  // extern "C"

#ifdef INSEV_TWIN_MAIN
#define TWIN_NAME "insev_twin"
#include "twin_main.hpp"

// Seeded batches (twin_main.hpp's reads) with an event list drawn over them -- real intervals, unused slots, entries of rows
// outside the batch and intervals that leave their read -- in exact heap blocks; the table against a plain map of the events.
int main() {
    int64_t events = 0, guarded = 0, combined = 0, lost_runs = 0;
    for (int round = 0; round < 200; ++round) {
        TwinReads B;
        B.draw(round);
        const uint64_t read_base = round % 4 == 0 ? 0xFFFFFFF0ull : (uint64_t)rnd(1000);
        const long long cap = 1 + (long long)rnd(200);
        std::vector<amp_ins_event> list((size_t)8 * (size_t)cap, amp_ins_event{-1, 0u, 0, 0});
        unsigned long long shard_n[8], cursor[8];
        for (int s = 0; s < 8; ++s) {
            shard_n[s] = rnd(6) == 0 ? (unsigned long long)cap + rnd(5) : rnd((uint32_t)cap + 1);
            cursor[s] = rnd(3) == 0 ? rnd((uint32_t)cap + 3) : 0;
            for (long long k = 0; k < cap; ++k) {
                amp_ins_event &e = list[(size_t)s * (size_t)cap + (size_t)k];
                const uint32_t kind = rnd(10);
                if (kind == 0 || B.n == 0) continue;                                     // unused
                const int64_t i = rnd(3) == 0 ? 0 : rnd((uint32_t)B.n);                // (a pile on row 0)
                const int32_t L = (int32_t)B.lseq[i];
                e.ref_pos = (int32_t)rnd(50);
                e.read = (uint32_t)((uint64_t)(kind == 1 ? B.n + rnd(5) : i) + read_base);
                e.q_from = L ? (int32_t)rnd((uint32_t)L + 1) : 0;
                e.q_to = kind == 2 ? e.q_from + L + 1 : e.q_from + (L - e.q_from ? (int32_t)rnd((uint32_t)(L - e.q_from) + 1) % 5 : 0);
                if (rnd(4) == 0) { e.q_from = 0; e.q_to = L < 3 ? L : 3; }             // (the pile's allele)
            }
        }
        amp_ins_event *p_ev = exact(list);
        const uint32_t log2cap = round % 5 == 0 ? 4u : 11u;
        const size_t slots = (size_t)1 << log2cap;
        uint64_t *keys = (uint64_t *)malloc(slots * 16); memset(keys, 0xFF, slots * 16);
        uint32_t *cnt = (uint32_t *)calloc(slots * 2, 4);
        InsevSide *side = (InsevSide *)calloc(slots, sizeof(InsevSide));
        int64_t info[N_INFO];
        CHECK(twin_insev(B.n, B.flag, B.lseq, B.coff, B.cig, B.soff, B.seq, B.qual, B.status, read_base, p_ev, cap, shard_n, cursor, log2cap, keys, cnt, side, info) == 0);
        // every slot's cells add up, and over the table they account for every tallied event
        int64_t used = 0, total = 0;
        for (size_t s = 0; s < slots; ++s) {
            if (keys[2 * s + 1] == IE_EMPTY) { CHECK(keys[2 * s] == IE_EMPTY && cnt[2 * s] == 0); continue; }
            ++used;
            uint32_t b = 0;
            for (int k = 0; k < IE_BINS; ++k) b += side[s].bin[k];
            CHECK(b == cnt[2 * s] && cnt[2 * s + 1] <= cnt[2 * s] && side[s].noqual <= cnt[2 * s]);
            total += cnt[2 * s];
        }
        CHECK(used == info[I_USED] && total + info[I_LOST] == info[I_EVENTS]);
        CHECK(info[I_SLOTS] == info[I_UNUSED] + info[I_GUARDED] + info[I_EVENTS]);
        if (info[I_LOST]) { CHECK(used == (int64_t)slots || log2cap > 4u); ++lost_runs; }
        events += info[I_EVENTS]; guarded += info[I_GUARDED]; combined += info[I_COMBINED];
        free(p_ev); free(keys); free(cnt); free(side);
        B.release();
    }
    CHECK(events > 1000 && guarded > 100 && combined > 100 && lost_runs > 0);
    printf("insev_twin ok\n");
    return 0;
}
#endif
