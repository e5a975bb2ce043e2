// ins_twin -- TEST INFRASTRUCTURE: the per-event functions of amplipy_amd/csrc/amp_ins.hpp that the kernels of amp_ins.hip call,
// looped over host arrays in the order of steps of ins_aggregate: hash key per slot (k_ins_hash), a stable sort by it, the
// position key in that order (k_ins_poskey), a stable sort by it, heads by neighbour comparison (k_ins_heads), their exclusive
// sum, runs and counts (k_ins_runs, the last event writing the number of runs).  hash_mask is the twin's own: it is applied to
// the shared function's key of every used slot, so that alleles collide and interleave (the device always sorts the full key).
// Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fPIC -shared -I amplipy_amd/csrc -o libins_twin.so ins_twin.cpp     (tests/test_ins_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DINS_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o ins_twin ins_twin.cpp && ./ins_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded lists in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "amp_ins.hpp"

using namespace amp;

extern "C" {

int64_t twin_read_row(uint32_t read, uint64_t read_base) { return ins_read_row(read, read_base); }

// ev: the eight shard regions of `cap` slots each, shard_n[8] slots in use per region (unused slots among them carry
// ref_pos = -1); seq_off8 / seq: the packed batch the read ids refer to, read_base as the events were recorded with.
// runs: room for one record per slot in use, zeroed here.  run_of_slot: per slot in use (concatenated regions), the run
// its event went to, 0xFFFFFFFF for an unused slot.  Returns non-zero when a step left its bounds.
int twin_ins_aggregate(const amp_ins_event *ev, long long cap, const unsigned long long *shard_n, const uint32_t *seq_off8, const uint8_t *seq,
                       uint64_t read_base, uint64_t hash_mask, amp_ins_run *runs, uint32_t *run_of_slot, int64_t *n_events, int64_t *n_runs) {
    const ShardMap M = ins_shard_map(ev, cap, shard_n);
    const int64_t n = M.start[8];
    *n_events = 0; *n_runs = 0;
    if (n == 0) return 0;
    for (int k = 0; k < 8; ++k) if ((long long)shard_n[k] > cap) return 1;
    memset(runs, 0, (size_t)n * sizeof(amp_ins_run));
    std::vector<uint64_t> key((size_t)n);
    std::vector<uint32_t> idx((size_t)n), tmp((size_t)n);
    uint64_t nvalid = 0, nruns = 0;
    // k_ins_hash
    for (int64_t j = 0; j < n; ++j) {
        const amp_ins_event e = slot_event(M, j);
        idx[(size_t)j] = (uint32_t)j;
        uint64_t k = ins_hash_key(seq, seq_off8, read_base, e);
        if (k != INS_KEY_UNUSED) { k &= hash_mask; ++nvalid; }
        key[(size_t)j] = k;
        run_of_slot[j] = 0xFFFFFFFFu;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    // k_ins_poskey: the key of the events in hash order
    for (int64_t j = 0; j < n; ++j) key[(size_t)j] = ins_pos_key(slot_event(M, (int64_t)idx[(size_t)j]));
    std::iota(tmp.begin(), tmp.end(), 0u);
    std::stable_sort(tmp.begin(), tmp.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    std::vector<uint64_t> skey((size_t)n);
    std::vector<uint32_t> sidx((size_t)n);
    for (int64_t j = 0; j < n; ++j) { skey[(size_t)j] = key[tmp[(size_t)j]]; sidx[(size_t)j] = idx[tmp[(size_t)j]]; }
    // k_ins_heads
    std::vector<uint32_t> head((size_t)n, 0u), rid((size_t)n, 0u);
    for (int64_t j = 0; j < (int64_t)nvalid; ++j) {
        uint32_t h = 1u;
        if (j > 0 && skey[(size_t)j] == skey[(size_t)j - 1])
            h = ins_same_allele(seq, seq_off8, read_base, slot_event(M, (int64_t)sidx[(size_t)j]), slot_event(M, (int64_t)sidx[(size_t)j - 1])) ? 0u : 1u;
        head[(size_t)j] = h;
    }
    // the exclusive sum
    uint32_t acc = 0;
    for (int64_t j = 0; j < n; ++j) { rid[(size_t)j] = acc; acc += head[(size_t)j]; }
    // k_ins_runs
    int bad = 0;
    for (int64_t j = 0; j < (int64_t)nvalid; ++j) {
        const uint32_t r = ins_run_of(rid[(size_t)j], head[(size_t)j]);
        if ((int64_t)r >= n) { bad |= 2; continue; }
        if (head[(size_t)j]) runs[r].first = slot_event(M, (int64_t)sidx[(size_t)j]);
        runs[r].count += 1u;
        run_of_slot[sidx[(size_t)j]] = r;
        if (j == (int64_t)nvalid - 1) nruns = (uint64_t)r + 1u;
    }
    *n_events = (int64_t)nvalid;
    *n_runs = nvalid ? (int64_t)nruns : 0;
    return bad;
}

}  // extern "C"

#ifdef INS_TWIN_MAIN
#define TWIN_NAME "ins_twin"
#include "twin_main.hpp"

int main() {
    static const uint64_t masks[4] = {0ull, 1ull, 15ull, ~0ull};
    int64_t split_rounds = 0, unused_seen = 0, events_seen = 0;
    for (int round = 0; round < 400; ++round) {
        // a batch: reads of 0..40 bases over few letters (so that alleles repeat), ids wrapping in some rounds
        const uint32_t n_reads = 1 + rnd(round % 7 == 0 ? 300 : 12);
        const uint64_t read_base = round % 3 == 0 ? 0ull : round % 3 == 1 ? 7ull + rnd(1000) : 0x100000000ull - 1 - rnd(n_reads);
        std::vector<uint32_t> lseq, soff(1, 0u);
        std::vector<uint8_t> seq;
        const uint32_t letters = 1 + rnd(3);
        for (uint32_t i = 0; i < n_reads; ++i) {
            const uint32_t L = rnd(41), padded = (L + 7u) & ~7u;
            lseq.push_back(L);
            for (uint32_t k = 0; k < padded / 2; ++k) seq.push_back((uint8_t)(((1u << rnd(letters)) << 4) | (1u << rnd(letters))));
            soff.push_back((uint32_t)(seq.size() / 4));
        }
        // a list: cap, fills of the eight shards (some empty), events at few positions, unused slots among them
        const long long cap = 1 + rnd(round % 5 == 0 ? 600 : 40);
        unsigned long long shard_n[8];
        int64_t n_slots = 0;
        for (int s = 0; s < 8; ++s) { shard_n[s] = rnd(3) == 0 ? 0ull : rnd((uint32_t)cap + 1); n_slots += (int64_t)shard_n[s]; }
        std::vector<amp_ins_event> ev((size_t)(8 * cap), amp_ins_event{-1, 0u, 0, 0});
        for (size_t k = 0; k < ev.size(); ++k) ev[k] = amp_ins_event{(int32_t)rnd(3), 0xDEADu, 1000000, 2000000};     // beyond the fill: never to be read
        int64_t want_events = 0;
        for (int s = 0; s < 8; ++s)
            for (unsigned long long k = 0; k < shard_n[s]; ++k) {
                amp_ins_event e{-1, 0u, 0, 0};
                if (rnd(5) != 0) {
                    const uint32_t i = rnd(n_reads), a = rnd(lseq[i] + 1), b = a + rnd(std::min<uint32_t>(lseq[i] - a, 4u) + 1);
                    e = amp_ins_event{(int32_t)rnd(4), (uint32_t)(read_base + i), (int32_t)a, (int32_t)b};
                    ++want_events;
                } else {
                    ++unused_seen;
                }
                ev[(size_t)s * (size_t)cap + (size_t)k] = e;
            }
        amp_ins_event *p_ev = exact(ev);
        uint32_t *p_soff = exact(soff);
        uint8_t *p_seq = exact(seq);
        // the plain tally: text per event
        auto text_of = [&](const amp_ins_event &e) {
            std::string t;
            const int64_t row = (int64_t)(((uint64_t)e.read - read_base) & 0xFFFFFFFFull);
            for (int32_t q = e.q_from; q < e.q_to; ++q) {
                const uint64_t k = (uint64_t)soff[(size_t)row] * 8u + (uint64_t)q;
                t.push_back("=ACMGRSVTWYHKDBN"[(k & 1) ? (seq[k >> 1] & 15) : (seq[k >> 1] >> 4)]);
            }
            return t;
        };
        std::map<std::pair<int32_t, std::string>, int64_t> want;
        std::vector<amp_ins_event> flat;
        for (int s = 0; s < 8; ++s)
            for (unsigned long long k = 0; k < shard_n[s]; ++k) flat.push_back(ev[(size_t)s * (size_t)cap + (size_t)k]);
        for (const amp_ins_event &e : flat) if (e.ref_pos >= 0) ++want[{e.ref_pos, text_of(e)}];
        for (int m = 0; m < 4; ++m) {
            std::vector<amp_ins_run> runs((size_t)std::max<int64_t>(n_slots, 1));
            std::vector<uint32_t> ros((size_t)std::max<int64_t>(n_slots, 1));
            amp_ins_run *p_runs = exact(runs);
            uint32_t *p_ros = exact(ros);
            int64_t ne = -1, nr = -1;
            CHECK(twin_ins_aggregate(p_ev, cap, shard_n, p_soff, p_seq, read_base, masks[m], p_runs, p_ros, &ne, &nr) == 0);
            CHECK(ne == want_events && nr <= ne && (ne == 0) == (nr == 0));
            std::map<std::pair<int32_t, std::string>, int64_t> got;
            int64_t total = 0;
            uint64_t last = 0;
            for (int64_t r = 0; r < nr; ++r) {
                const amp_ins_run &R = p_runs[r];
                CHECK(R.count > 0 && R.reserved == 0 && R.first.ref_pos >= 0);
                got[{R.first.ref_pos, text_of(R.first)}] += R.count;
                total += R.count;
                const uint64_t pk = ((uint64_t)(uint32_t)R.first.ref_pos << 32) | (uint32_t)(R.first.q_to - R.first.q_from);
                CHECK(pk >= last);
                last = pk;
            }
            CHECK(total == ne && got == want);
            // every event sits in a run of its own text, and the representative is one of the run's events
            std::vector<uint32_t> members((size_t)std::max<int64_t>(nr, 1), 0u), rep((size_t)std::max<int64_t>(nr, 1), 0u);
            for (int64_t j = 0; j < n_slots; ++j) {
                const amp_ins_event &e = flat[(size_t)j];
                if (e.ref_pos < 0) { CHECK(p_ros[j] == 0xFFFFFFFFu); continue; }
                const uint32_t r = p_ros[j];
                CHECK((int64_t)r < nr);
                CHECK(e.ref_pos == p_runs[r].first.ref_pos && text_of(e) == text_of(p_runs[r].first));
                ++members[r];
                if (memcmp(&e, &p_runs[r].first, sizeof(e)) == 0) ++rep[r];
            }
            for (int64_t r = 0; r < nr; ++r) CHECK(members[(size_t)r] == p_runs[r].count && rep[(size_t)r] >= 1u);
            if (m == 3) CHECK(nr == (int64_t)want.size());
            else { CHECK(nr >= (int64_t)want.size()); if (nr > (int64_t)want.size()) ++split_rounds; }
            free(p_runs); free(p_ros);
        }
        events_seen += want_events;
        free(p_ev); free(p_soff); free(p_seq);
    }
    CHECK(split_rounds > 100 && unused_seen > 1000 && events_seen > 10000);
    printf("ins_twin ok\n");
    return 0;
}
#endif
