// amp_del.hpp -- deletion events.  The count table records a deleted base as one more '-' at one
// position (update_base_counts, A:713-715); that one read skipped positions 21765 to 21770 TOGETHER is lost there.  An event
// is, for one counted read, a maximal run of consecutive reference positions each of which that read's count walk adds to the
// '-' column: key (start, len), 0-based, len >= 1.  D and N ops are alike (st_is_del); neighbouring D / N ops, and D / N ops
// with only an insertion between them, are one event; a deletion that runs past the reference end is cut where the walk stops.
// Per key the table holds count (reads) and rev (those with FLAG 0x10), so that for every position p the counts of the events
// with start <= p < start + len add up to counts[p]['-'] and their rev to the strand tallies' rev[p][5].
//
// What one read gives and where a key goes is written here as plain functions: k_del (amp_del.hip) calls them on the device;
// tests/hostsim/del_twin.cpp loops the same functions on the CPU, built with plain g++, against the restatement in
// tests/del_util.py.  A read with a regular CIGAR (regular_scan, amp_strand.hpp) gives its events from the CIGAR words alone;
// every other read walks (strand_walk) and groups the consecutive column-5 sinks.  The tables are keyed, not positional: a
// small open-addressed table per block in LDS in front of one in HBM, the same hash, linear probing, a bounded probe count.
#pragma once

#include <stdint.h>

#include "amp_keyed.hpp"
#include "amp_strand.hpp"

namespace amp {

constexpr int DL_BLOCK = 256;                // lanes of a k_del block = reads of a tile
constexpr int DL_LIST = 1024;                // events a tile's list holds; an event past it goes straight to the global table
constexpr int DL_LDS_LOG2 = 10;
constexpr int DL_LDS_SLOTS = 1 << DL_LDS_LOG2;           // slots of a block's table: a u64 key and two u32 counts each, 16 KB
constexpr int DL_LDS_PROBES = 16;            // slots an insert into the block's table tries; then it goes straight to the global table
constexpr int DL_LDS_FLUSH_AT = DL_LDS_SLOTS / 4 * 3;    // more used slots than this at a tile boundary: the block's table goes to the global one
constexpr int DL_GLOBAL_PROBES = 4096;       // slots an insert into the global table tries (keyed_probes); then the event is lost
constexpr int DL_TILES_PER_BLOCK = 2;        // a block takes at least this many tiles before another block is added ...
constexpr int DL_BLOCKS_PER_CU = 6;          // ... and the grid stops growing here: six blocks' LDS (24.6 KB each) fit a CU
constexpr int DL_MAX_TILES_PER_FLUSH = 1 << 23;          // a key takes at most one add per read: 2^23 tiles of 256 stay below 2^32
constexpr int DL_LOG2_DEFAULT = 20, DL_LOG2_MIN = 4, DL_LOG2_MAX = 28;      // the global table's slots (16 bytes each)
constexpr uint64_t DL_EMPTY = ~0ull;         // no key: a start is below 2^31
constexpr uint64_t DL_REV_BIT = 1ull << 63;  // a list entry: the key, and this bit for a reverse read
static_assert(DL_LDS_FLUSH_AT * 4 == DL_LDS_SLOTS * 3, "three quarters");
static_assert(DL_GLOBAL_PROBES == KEYED_PROBES, "one probe rule (amp_keyed.hpp)");
static_assert((uint64_t)DL_MAX_TILES_PER_FLUSH * DL_BLOCK < (1ull << 32), "a count of the block's table cannot overflow before its flush");

// The key of an event: start in the high word, len in the low one -- keys order as (start, len) does.
AMP_ST_HD uint64_t del_key(int32_t start, int32_t len) { return ((uint64_t)(uint32_t)start << 32) | (uint64_t)(uint32_t)len; }
AMP_ST_HD int32_t del_key_start(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }
AMP_ST_HD int32_t del_key_len(uint64_t key) { return (int32_t)(uint32_t)key; }

// The hash both tables use (the 64-bit finaliser of MurmurHash3): the block's table takes its low bits, the global table the
// bits from 32 up, so that keys which meet in one need not meet in the other.
AMP_ST_HD uint64_t del_hash(uint64_t key) {
    uint64_t x = key;
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
AMP_ST_HD uint32_t del_slot_lds(uint64_t key) { return (uint32_t)del_hash(key) & (uint32_t)(DL_LDS_SLOTS - 1); }
AMP_ST_HD uint32_t del_slot_global(uint64_t key, uint32_t log2_capacity) { return keyed_slot(del_hash(key), log2_capacity); }
AMP_ST_HD uint32_t del_probes_global(uint32_t log2_capacity) { return keyed_probes(log2_capacity); }

// The probe rule of both tables: slots first, first + 1, ... (wrapping at the table's end), at most `probes` of them;
// claim(slot) puts the key into an empty slot and says what the slot held before (DL_EMPTY: the key is new there).  -> the
// key's slot, or -1 when none of the slots tried is empty or the key's own: the loop ends either way.
template <class Claim>
AMP_ST_HD int64_t del_probe(uint64_t key, uint32_t first, uint32_t mask, uint32_t probes, Claim claim) {
    for (uint32_t k = 0; k < probes; ++k) {
        const uint32_t s = (first + k) & mask;
        const uint64_t prev = claim(s);
        if (prev == DL_EMPTY || prev == key) return (int64_t)s;
    }
    return -1;
}

// Neighbouring deletions into one event: add(r0, len) per deleted stretch in walk order, cut() where something else is
// known to lie between two stretches and once more at the end; emit(start, len) per event.
template <class Emit>
struct DelRun {
    int32_t start = 0, len = 0;
    Emit emit;
    AMP_ST_HD explicit DelRun(Emit e) : emit(e) {}
    AMP_ST_HD void cut() { if (len) emit(start, len); len = 0; }
    AMP_ST_HD void add(int32_t r0, int32_t n) {
        if (len && start + len == r0) { len += n; return; }
        cut();
        start = r0; len = n;
    }
};

// The events of a read with a regular CIGAR, from its CIGAR words alone: the deletion segments of regular_scan, neighbours
// merged (an insertion puts nothing between them; a match segment does).  The scan is told that QUAL is there: it reads no
// byte of the read.  Only when the shape is regular are the events the read's; the caller looks twice -- once to learn the
// shape and the number of events, once to take them -- and asks del_qual_needed in between.
template <class Emit>
AMP_ST_HD StrandShape del_events_regular(const StrandRead &R, const StrandParams &P, Emit emit) {
    DelRun<Emit> run(emit);
    const StrandShape sh = regular_scan(R, P, 0u, [&](int32_t r0, uint64_t, uint32_t len, bool del) {
        if (del) run.add(r0, (int32_t)len);
        else run.cut();
    });
    run.cut();
    return sh;
}

// A read without QUAL is not regular, but the scan above was not told.  Without an event that changes nothing (such a read's
// walk hands out deleted positions in front of its first base only, and every one of them lies in a D or N op); with events
// the read's first quality byte decides.
AMP_ST_HD bool del_qual_needed(const StrandShape &sh, int32_t n_events) { return sh.regular && n_events > 0; }

// The events of every other read: the exact walk, its column-5 sinks grouped where their positions are consecutive.
template <class Emit>
AMP_ST_HD void del_events_walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Emit emit) {
    DelRun<Emit> run(emit);
    strand_walk(R, P, seq, qual, [&](int32_t r, uint32_t col, uint32_t) {
        if (col == 5u) run.add(r, 1);
    });
    run.cut();
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is del_hook of amp_del.hip, declared in amp_hook.hpp)
