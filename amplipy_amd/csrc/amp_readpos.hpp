// amp_readpos.hpp -- read-position tallies per allele: for every increment update_base_counts (A:690-753)
// makes to one of the six fixed keys A C G T N '-' of a position, hist[r][c][rp_bin(d)] += 1, where d says how far from the
// nearer end of the read's kept query span [query_alignment_start, query_alignment_end) the base sits.  What one read and one
// base add is written here as plain functions on top of amp_strand.hpp: k_readpos (amp_readpos.hip) calls them on the device;
// tests/hostsim/readpos_twin.cpp loops the same functions over arrays on the CPU, built with plain g++, against the
// restatement in tests/readpos_util.py.
//
// The distance.  A match base at query index q, qs <= q < qe: d = min(q - qs, qe - 1 - q), the kept query bases between it and
// the nearer end.  A deleted position (D or N): d = max(0, min(q_next - qs, qe - q_next) - 1), the smaller distance of the two
// flanking bases, q_next being the query index the next pair with a query index takes.  rp_bin(d) = min(6, bit_length(d >> 1)):
// d < 2, 2-3, 4-7, 8-15, 16-31, 32-63, >= 64.
//
// Two views of a read, as in amp_strand.hpp: readpos_segments on regular_scan for a read with a regular CIGAR -- a segment
// carries the distances dl, dr of its first base from the two ends, so that the lane of offset p has d = min(dl + p, dr - p) --
// and readpos_walk, the pair walk for every other read (six_key_walk with the distances worked out here).  ReadposTally, at the
// end: what k_readpos's loop (tally_poswin, amp_tally.hpp) and the twin's (poswin_twin.hpp) are told about this tally; the
// window rule is poswin_keeps / poswin_read_windowed of amp_strand.hpp on RP_W and RP_SLOTS.
//
// The window.  RP_W positions x 42 cells, two cells to a u32 word as 16-bit halves: RP_WORDS = 21 words per position, an odd
// stride.  A read adds at most 1 to a cell of a position per tile (its reference positions only advance), a tile has RP_BLOCK
// reads, so RP_MAX_TILES_PER_FLUSH tiles keep a half below 2^16 and no add ever carries into the upper half's neighbour.
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

namespace amp {

constexpr int RP_BLOCK = 256;            // lanes of a k_readpos block = reads of a tile
constexpr int RP_SLOTS = 4;              // segment slots per read; a read that needs more walks serially
constexpr int RP_CHUNK = 64;             // positions a wave takes at a time, one per lane
constexpr int RP_W = 512;                // reference positions of a block's window
constexpr int RP_BINS = AMP_RP_BINS;     // distance bins
constexpr int RP_COLS = AMP_NSYM;        // A C G T N '-'
constexpr int RP_CELLS = RP_COLS * RP_BINS;        // 16-bit cells of a window position = u32 cells of a table position
constexpr int RP_WORDS = (RP_CELLS + 1) / 2;       // u32 words of a window position
constexpr int RP_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int RP_BLOCKS_PER_CU = 2;      // ... and the grid stops growing here (the window and the list: two blocks to a CU)
constexpr int RP_MAX_TILES_PER_FLUSH = 255;        // a half takes at most 256 adds of 1 per tile
static_assert(RP_BINS == 7 && RP_CELLS == 42, "six columns of seven bins");

AMP_ST_HD uint32_t rp_bin(int32_t d) {
    uint32_t v = (uint32_t)d >> 1, b = 0;
    while (v && b < (uint32_t)RP_BINS - 1u) { v >>= 1; ++b; }
    return b;
}
AMP_ST_HD int32_t rp_min(int32_t a, int32_t b) { return a < b ? a : b; }
// a match base at query index q
AMP_ST_HD int32_t rp_match_d(int32_t q, int32_t qs, int32_t qe) { return rp_min(q - qs, qe - 1 - q); }
// a deleted position in front of query index q_next
AMP_ST_HD int32_t rp_del_d(int32_t q_next, int32_t qs, int32_t qe) {
    const int32_t m = rp_min(q_next - qs, qe - q_next) - 1;
    return m > 0 ? m : 0;
}

// A segment of a regular read: StrandSeg (the strand bit unused: deletions of both strands are kept) and the distances of
// its first base from the two ends of the kept span.  A deletion segment has one distance for all its positions, in dl.
struct ReadposSeg : StrandSeg {
    int32_t dl, dr;
};
// the distance of the segment's position at offset p
AMP_ST_HD int32_t rp_seg_d(const ReadposSeg &s, int32_t p) { return st_seg_del(s) ? s.dl : rp_min(s.dl + p, s.dr - p); }

// The segments of a regular read to put(seg): the scan's, every one of them.  qs and qe come from the CIGAR words the scan
// reads (st_query_bounds); a read whose bounds raise is not regular.
template <class Put>
AMP_ST_HD StrandShape readpos_segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) {
    int32_t qs = 0, qe = 0;
    const bool bounds = st_query_bounds(R, qs, qe);
    StrandShape sh = regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t len, bool del) {
        const int32_t q = (int32_t)(q0 - R.base);
        ReadposSeg s;
        s.r0 = r0; s.len_kind = (len << 2) | (del ? 2u : 0u); s.q0 = q0;
        if (del) { s.dl = rp_del_d(q, qs, qe); s.dr = s.dl; }
        else { s.dl = q - qs; s.dr = qe - 1 - q; }
        put(s);
    });
    sh.regular = sh.regular && bounds;
    return sh;
}

// What one base of a match segment adds: col < 5 when it is counted.
AMP_ST_HD bool readpos_base(const uint8_t *seq, const uint8_t *qual, uint64_t k, int32_t min_quality, uint32_t &col) {
    col = st_code_to_col(st_base_code(seq, k));
    return (int32_t)qual[k] >= min_quality && col < 5u;
}

// The cell (col, bin) of a table position, the window word that holds it and what an add of 1 adds to that word
AMP_ST_HD int rp_cell(uint32_t col, uint32_t bin) { return (int)col * RP_BINS + (int)bin; }
AMP_ST_HD int rp_word(int32_t wpos, int cell) { return wpos * RP_WORDS + (cell >> 1); }
AMP_ST_HD uint32_t rp_one(int cell) { return (cell & 1) ? 0x10000u : 1u; }

// The segment fields and the window rule under the read-position tallies' own names, for callers that name them: one-line forwards
AMP_ST_HD int32_t rp_seg_len(const ReadposSeg &s) { return st_seg_len(s); }
AMP_ST_HD bool rp_seg_del(const ReadposSeg &s) { return st_seg_del(s); }
AMP_ST_HD bool readpos_window_keeps(int32_t anchor, int32_t lo, int32_t hi) { return poswin_keeps<RP_W>(anchor, lo, hi); }
AMP_ST_HD bool readpos_read_windowed(const StrandShape &sh, int32_t pos, int32_t anchor) { return poswin_read_windowed<RP_W, RP_SLOTS>(sh, pos, anchor); }

// The six-key walk for one read (six_key_walk, amp_strand.hpp) with the distance in place of the query index: sink(ref_pos,
// col, d) for every increment (col 5: a deleted position).  Every position handed out lies inside [0, ref_len), every d is >= 0.
template <class Sink>
AMP_ST_HD void readpos_walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Sink sink) {
    six_key_walk(R, P, seq, qual, [&](int32_t r, uint32_t col, int32_t q, int32_t qs, int32_t qe) {
        sink(r, col, col == 5u ? rp_del_d(q, qs, qe) : rp_match_d(q, qs, qe));
    });
}

// The read-position tallies as tally_poswin (amp_tally.hpp) and its CPU twin (tests/hostsim/poswin_twin.hpp) take them.  A
// window position has 42 cells in WORDS = 21 u32 words; an add is always 1.  "add(c, v)": cell c of the position at hand gets v.
struct ReadposTally {
    static constexpr int BLOCK = RP_BLOCK, SLOTS = RP_SLOTS, CHUNK = RP_CHUNK, W = RP_W, WORDS = RP_WORDS, MAX_TILES_PER_FLUSH = RP_MAX_TILES_PER_FLUSH;
    using Seg = ReadposSeg;
    struct Out {
        uint32_t *hist;                  // [ref_len][6][7]
    };
    template <class Put>
    static AMP_ST_HD StrandShape segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) { return readpos_segments(R, P, qual0, put); }
    // what a segment adds at offset k of its span (a deletion loads no base)
    template <class Add>
    static AMP_ST_HD void seg_adds(const Seg &g, int32_t k, const uint8_t *seq, const uint8_t *qual, int32_t min_quality, Add add) {
        uint32_t col = 5u;
        if (st_seg_del(g) || readpos_base(seq, qual, g.q0 + (uint64_t)k, min_quality, col)) add(rp_cell(col, rp_bin(rp_seg_d(g, k))), 1u);
    }
    // the serial walk, sink(ref_pos, col, d), and what one of its increments adds
    template <class Sink>
    static AMP_ST_HD void walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Sink sink) { readpos_walk(R, P, seq, qual, sink); }
    template <class Add>
    static AMP_ST_HD void walk_adds(const StrandRead &, uint32_t col, int32_t d, Add add) { add(rp_cell(col, rp_bin(d)), 1u); }
    // the window word of cell c of window position w, and what an add of v = 1 adds to it
    static AMP_ST_HD int word(int32_t w, int c) { return rp_word(w, c); }
    static AMP_ST_HD uint32_t inc(int c, uint32_t) { return rp_one(c); }
    // cell c of table position p gets v, by plus(address, v); word k of a flushed window position is cells 2k and 2k + 1
    template <class Plus>
    static AMP_ST_HD void to_table(const Out &o, size_t p, int c, uint32_t v, Plus plus) { plus(&o.hist[p * RP_CELLS + c], v); }
    template <class Plus>
    static AMP_ST_HD void flush_word(const Out &o, size_t p, int k, uint32_t v, Plus plus) {
        if (v & 0xFFFFu) to_table(o, p, 2 * k, v & 0xFFFFu, plus);
        if (v >> 16) to_table(o, p, 2 * k + 1, v >> 16, plus);
    }
};
static_assert(ReadposTally::WORDS == 21 && (ReadposTally::WORDS & 1), "an odd stride: lanes on the same cell of neighbouring positions hit different banks");
static_assert((uint64_t)ReadposTally::MAX_TILES_PER_FLUSH * ReadposTally::BLOCK < (1ull << 16), "a 16-bit half cannot overflow before its flush");

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is readpos_hook of amp_readpos.hip, declared in amp_hook.hpp)
