// amp_insev.hpp -- insertion alleles: strand, quality and read-position evidence.  The read pass leaves
// every insertion event of a batch on the event list in HBM (amp_ins_event {ref_pos, read, q_from, q_to}: the allele is
// SEQ[q_from:q_to] of the read, anchor base and all); k_insev (amp_insev.hip) reads the entries the batch's pass appended and
// tallies them per allele.  It walks no CIGAR for the events themselves -- every path of the read pass has already encoded the
// reference's rules -- only a read's leading and trailing clips for the query span.  What ONE event contributes is written
// here as plain functions: k_insev calls them on the device; tests/hostsim/insev_twin.cpp loops the same functions over host
// arrays, built with plain g++, against the restatement in tests/insev_util.py.
//
// The key of an event is two 64-bit words: ins_pos_key (ref_pos << 32 | length) and ins_hash_key (the 63-bit allele hash) of
// amp_ins.hpp -- the two values amp_aggregate_ins_events sorts by.  Per key: count, rev (FLAG 0x10), noqual (reads with QUAL
// '*'), qsum (the allele's quality bytes, 64-bit, over the reads that have some) and seven bins of rp_bin(d)
// (amp_readpos.hpp), d = max(0, min(q_from - qs, qe - q_to)): the kept query bases between the allele and the nearer end of
// the counted alignment's query span [qs, qe) -- soft clips and trimmed primers do not count, inserted bases do.
#pragma once

#include <stdint.h>

#include "amp_ins.hpp"
#include "amp_keyed.hpp"
#include "amp_readpos.hpp"

namespace amp {

constexpr int IE_BLOCK = 256;                // lanes of a k_insev block: an event per lane and trip
constexpr int IE_GRID = 512;                 // its blocks, whatever the batch: the number of events is known on the device only
constexpr int IE_BINS = RP_BINS;
constexpr int IE_LOG2_DEFAULT = 20, IE_LOG2_MIN = 4, IE_LOG2_MAX = 28;      // the table's slots (64 bytes each): amp_del_enable's range rule
constexpr uint64_t IE_EMPTY = ~0ull;         // a free key word: a position is below 2^31, a hash below 2^63
static_assert(IE_BLOCK * IE_GRID == AMP_INSEV_STRIDE, "the stride the ABI names");
static_assert(IE_BINS == 7, "amp_insev_entry::bin");

// What the table keeps per slot beside the keyed table's (count, rev)
struct InsevSide {
    unsigned long long qsum;
    uint32_t noqual;
    uint32_t bin[IE_BINS];
};
static_assert(sizeof(InsevSide) == 40, "64 bytes a slot: two key words, two counts, this");

// One event's contribution
struct InsevCells {
    uint32_t rev, noqual, bin;
    uint64_t qsum;
};

// [qs, qe) of a CIGAR as the count walk takes them (query_alignment_start / _end: hard clips skipped, the soft clips at
// either end; element 0 is never examined from the back)
AMP_ST_HD void insev_query_span(const uint32_t *cig, uint32_t n_ops, int32_t lseq, int32_t &qs, int32_t &qe) {
    int32_t off = 0;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const uint32_t v = cig[i], op = v & 15u;
        if (op == ST_OP_H) continue;
        if (op != ST_OP_S) break;
        off += (int32_t)(v >> 4);
    }
    int32_t end = lseq;
    for (int64_t k = (int64_t)n_ops - 1; k >= 1; --k) {
        const uint32_t v = cig[k], op = v & 15u;
        if (op == ST_OP_H) continue;
        if (op != ST_OP_S) break;
        end -= (int32_t)(v >> 4);
    }
    qs = off; qe = end;
}

// The distance of the interval [q_from, q_to) from the nearer end of [qs, qe): an allele whose anchor base lies in a clip, or
// that ends behind the span, is at distance 0
AMP_ST_HD int32_t insev_d(int32_t q_from, int32_t q_to, int32_t qs, int32_t qe) {
    const int32_t m = rp_min(q_from - qs, qe - q_to);
    return m > 0 ? m : 0;
}

// The read has no qualities: QUAL '*' (first byte 0xFF), or no bases at all
AMP_ST_HD bool insev_noqual(const uint8_t *qual, uint64_t base, int32_t lseq) { return lseq <= 0 || qual[base] == 0xFFu; }

AMP_ST_HD uint64_t insev_qsum(const uint8_t *qual, uint64_t base, int32_t q_from, int32_t q_to) {
    uint64_t s = 0;
    for (int32_t q = q_from; q < q_to; ++q) s += qual[base + (uint64_t)q];
    return s;
}

// The cells of event e of the read in row `row`, whose counted CIGAR is cig[0 .. n_ops)
AMP_ST_HD InsevCells insev_cells(const amp_ins_event &e, const uint32_t *cig, uint32_t n_ops, int32_t lseq, uint32_t flag, const uint8_t *qual, uint64_t base) {
    InsevCells c;
    int32_t qs, qe;
    insev_query_span(cig, n_ops, lseq, qs, qe);
    c.rev = (flag & 0x10u) ? 1u : 0u;
    c.noqual = insev_noqual(qual, base, lseq) ? 1u : 0u;
    c.qsum = c.noqual ? 0ull : insev_qsum(qual, base, e.q_from, e.q_to);
    c.bin = rp_bin(insev_d(e.q_from, e.q_to, qs, qe));
    return c;
}

// The key of a used event
AMP_ST_HD void insev_key(const uint8_t *seq, const uint32_t *seq_off8, uint64_t read_base, const amp_ins_event &e, uint64_t *key) {
    key[0] = ins_pos_key(e);
    key[1] = ins_hash_key(seq, seq_off8, read_base, e);
}
AMP_ST_HD int32_t insev_key_pos(const uint64_t *key) { return (int32_t)(uint32_t)(key[0] >> 32); }
AMP_ST_HD int32_t insev_key_len(const uint64_t *key) { return (int32_t)(uint32_t)key[0]; }

// Where a key starts in the table: the 64-bit finaliser of MurmurHash3 over both words
AMP_ST_HD uint64_t insev_hash(const uint64_t *key) {
    uint64_t x = key[0] * 0x9E3779B97F4A7C15ull ^ key[1];
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// The probe rule (hap_probe's, for two 64-bit words).  No compare-and-swap is 128 bits wide, so a slot is claimed ONE WORD AT A
// TIME in fixed order: cas(slot, w, value) puts value into word w of the slot when that word is IE_EMPTY and says what it
// held before.  An inserter that meets a word that is neither empty nor its own leaves the slot for the next one; an inserter
// that gets through both words has matched both, whoever wrote which: the slot holds exactly its key.  Progress: a word once
// written never changes until a reset, so a slot ends up with one key and a key that left a slot leaves it every time -- all
// inserts of one key end in one slot; whoever writes word 0 goes straight on to word 1, so no slot stays half a key; nothing
// here waits for another inserter, and the loop is bounded by `probes`.  -> the key's slot (fresh: this call wrote its last
// word), or -1 when none of the slots tried took the key.
template <class Cas>
AMP_ST_HD int64_t insev_probe(const uint64_t *key, uint32_t first, uint32_t mask, uint32_t probes, Cas cas, bool &fresh) {
    fresh = false;
    for (uint32_t k = 0; k < probes; ++k) {
        const uint32_t s = (first + k) & mask;
        const uint64_t p0 = cas(s, 0, key[0]);
        if (p0 != IE_EMPTY && p0 != key[0]) continue;
        const uint64_t p1 = cas(s, 1, key[1]);
        if (p1 != IE_EMPTY && p1 != key[1]) continue;
        fresh = p1 == IE_EMPTY;
        return (int64_t)s;
    }
    return -1;
}

// Slot j of this batch's part of the list -- the slots [from[s], to[s]) of every shard s, one shard behind the other -> its
// index in the list's array (shard regions of `cap` entries); start[s]: the slots in front of shard s, start[8]: all of them
struct InsevSpan { long long cap; long long from[8]; long long start[9]; };
AMP_ST_HD InsevSpan insev_span(long long cap, const unsigned long long *cursor, const unsigned long long *shard_n) {
    InsevSpan M;
    M.cap = cap;
    long long tot = 0;
    for (int s = 0; s < 8; ++s) {
        const long long to = (long long)shard_n[s] < cap ? (long long)shard_n[s] : cap;      // (a counter past the capacity: dropped events)
        const long long from = (long long)cursor[s] < to ? (long long)cursor[s] : to;
        M.from[s] = from; M.start[s] = tot;
        tot += to - from;
    }
    M.start[8] = tot;
    return M;
}
AMP_ST_HD size_t insev_span_at(const InsevSpan &M, int64_t j) {
    int s = 0;
    for (int k = 1; k < 8; ++k) s += j >= M.start[k] ? 1 : 0;
    return (size_t)s * (size_t)M.cap + (size_t)(M.from[s] + (j - M.start[s]));
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is insev_hook of amp_insev.hip, declared in amp_hook.hpp)
