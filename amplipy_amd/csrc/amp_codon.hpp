// amp_codon.hpp -- codon tallies within single reads.  The slots are the codon start positions of the
// CDS rows, starts[n_slots], strictly increasing; the table is codon[n_slots][65].  A REGULAR read (regular_scan,
// amp_strand.hpp) adds, for the slot at start p:
//   a triplet: [p, p + 3) lies inside one match segment -- a maximal run of M = X ops with no inserted, deleted or skipped
//     base inside it -- and all three bases are among A C G T with quality >= min_quality: cell 16 b0 + 4 b1 + b2 += 1;
//   broken: [p, p + 3) lies inside [pos, ref_end) but inside no match segment (a deletion or skip overlaps the codon, or an
//     insertion sits between two of its positions): cell 64 += 1, once per read and slot, no quality test.
// Every other read with status 0 adds nothing and is counted as skipped.  What one read and one codon add is written here as
// plain functions: k_codon (amp_codon.hip) calls them on the device; tests/hostsim/codon_twin.cpp loops the same functions over
// arrays on the CPU, built with plain g++, against the restatement in tests/codon_util.py.
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

namespace amp {

constexpr int CD_BLOCK = 256;            // lanes of a k_codon block = reads of a tile
constexpr int CD_SLOTS = 6;              // list entries per read: a read with two indels has five; a read that needs more goes serial
constexpr int CD_CHUNK = 64;             // codon slots a wave takes at a time, one per lane
constexpr int CD_UNROLL = 4;             // entries a wave of k_codon has in flight in phase B: their loads are issued before the first add
constexpr int CD_W = 192;                // codon slots of a block's window: 576 positions of a single-frame CDS, 192 of three frames
constexpr int CD_CELLS = 65;             // u32 cells of a slot: the 64 triplets, then broken
constexpr int CD_BROKEN = 64;
constexpr int CD_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int CD_BLOCKS_PER_CU = 2;      // ... and the grid stops growing here (74.5 KB of LDS: two blocks share a CU)
constexpr int CD_MAX_TILES_PER_FLUSH = 1 << 23;     // a cell takes at most one add per read: 256 per tile
constexpr int64_t CD_MAX_SLOTS = 1 << 20;
static_assert(CD_W % CD_CHUNK == 0, "the window is whole chunks");
static_assert(CD_CELLS & 1, "an odd stride: the lanes of a wave hit 64 different banks");
static_assert((uint64_t)CD_MAX_TILES_PER_FLUSH * CD_BLOCK < (1ull << 32), "a window cell cannot overflow before its flush");
static_assert(CD_W * 3 >= 512, "a window of at least 512 positions on a single-frame CDS");

struct CodonShape {
    bool regular;          // regular_scan's word on the read
    int32_t n_seg;         // list entries codon_segments hands out
    int32_t ref_end;
};

// An entry of a regular read's list, as a StrandSeg: the codon starts [r0, r0 + length) it speaks for.  Match (bit 1 clear):
// a codon at start p in that range lies inside the match segment, its first base at index q0 + (p - r0) of qual / seq.
// Break (bit 1 set): the read breaks the codon at every start in the range.
AMP_ST_HD bool cd_seg_break(const StrandSeg &s) { return st_seg_del(s); }

// BAM 4-bit code -> 0..3 for A C G T, 0xFF otherwise
AMP_ST_HD uint32_t cd_code_to_base(uint32_t code) { return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 0xFFu; }

// The per-base step, three times, in two halves so that a caller can have the loads of several codons in flight before it
// looks at the first: the three quality bytes and the three 4-bit codes of the codon whose first base is at index k ...
AMP_ST_HD uint32_t codon_load_quals(const uint8_t *qual, uint64_t k) {
    return (uint32_t)qual[k] | ((uint32_t)qual[k + 1] << 8) | ((uint32_t)qual[k + 2] << 16);
}
AMP_ST_HD uint32_t codon_load_codes(const uint8_t *seq, uint64_t k) {
    return (st_base_code(seq, k) << 8) | (st_base_code(seq, k + 1) << 4) | st_base_code(seq, k + 2);
}
// ... and the triplet's cell, or nothing when a base is not A C G T or its quality is low.
AMP_ST_HD bool codon_cell_of(uint32_t quals, uint32_t codes, int32_t min_quality, uint32_t &cell) {
    uint32_t c = 0u;
    bool ok = true;
    for (int j = 0; j < 3; ++j) {
        const uint32_t b = cd_code_to_base((codes >> (4 * (2 - j))) & 15u);
        ok = ok && b < 4u && (int32_t)((quals >> (8 * j)) & 255u) >= min_quality;
        c = (c << 2) | (b & 3u);
    }
    cell = c;
    return ok;
}
AMP_ST_HD bool codon_cell(const uint8_t *seq, const uint8_t *qual, uint64_t k, int32_t min_quality, uint32_t &cell) {
    return codon_cell_of(codon_load_quals(qual, k), codon_load_codes(seq, k), min_quality, cell);
}

// The list of a read, to put(entry): the match segments of at least 3 bases (as the codon starts they hold) and the intervals
// of codon starts the read breaks -- [r - 2, r + len - 1] for a deletion or skip of [r, r + len), [r - 2, r - 1] for an insertion
// in front of r -- merged in CIGAR order so that no start is handed out twice (two deletions that touch one codon; an
// insertion next to a deletion), and cut to the codons that lie inside [pos, ref_end).  An interval is handed out when a later
// one no longer touches it -- that one begins at some r' - 2 with r' <= ref_end, so the finished one ends below ref_end - 3 and
// needs no cut -- and the last one is cut when the CIGAR ends.  Adjacent match ops (5M 5M; = X =; a zero-length op between
// them) are one match segment.  The entries of a read that turns out not to be regular are to be thrown away.
template <class Put>
AMP_ST_HD CodonShape codon_segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) {
    int32_t n = 0;
    bool have_m = false, have_b = false;
    int64_t m_r0 = 0, m_r1 = 0, b0 = 0, b1 = 0;      // the match segment [m_r0, m_r1) and the break starts [b0, b1] being built
    uint64_t m_q0 = 0;
    auto emit = [&](int64_t s0, int64_t cnt, bool brk, uint64_t q0) {
        if (cnt <= 0) return;
        StrandSeg s;
        s.r0 = (int32_t)s0;
        s.len_kind = ((uint32_t)cnt << 2) | (brk ? 2u : 0u);
        s.q0 = q0;
        put(s);
        ++n;
    };
    auto add_break = [&](int64_t s0, int64_t s1) {      // starts [s0, s1]
        if (s0 < (int64_t)R.pos) s0 = R.pos;
        if (s1 < s0) return;
        if (have_b && s0 <= b1 + 1) { if (s1 > b1) b1 = s1; return; }
        if (have_b) emit(b0, b1 - b0 + 1, true, 0ull);
        have_b = true; b0 = s0; b1 = s1;
    };
    const StrandShape sh = regular_scan(R, P, qual0, [&](int32_t seg_r0, uint64_t q0, uint32_t seg_len, bool del) {
        const int64_t r0 = seg_r0, len = seg_len;
        if (del) {
            if (have_m) { emit(m_r0, m_r1 - m_r0 - 2, false, m_q0); have_m = false; }
            add_break(r0 - 2, r0 + len - 1);
        } else if (have_m && q0 == m_q0 + (uint64_t)(m_r1 - m_r0)) {
            m_r1 += len;                 // the same run goes on (r0 == m_r1: nothing but match ops since)
        } else {
            if (have_m) {                // an insertion between two match segments
                emit(m_r0, m_r1 - m_r0 - 2, false, m_q0);
                add_break(r0 - 2, r0 - 1);
            }
            have_m = true; m_r0 = r0; m_r1 = r0 + len; m_q0 = q0;
        }
    });
    if (have_m) emit(m_r0, m_r1 - m_r0 - 2, false, m_q0);
    if (have_b) {
        if (b1 > (int64_t)sh.ref_end - 3) b1 = (int64_t)sh.ref_end - 3;
        emit(b0, b1 - b0 + 1, true, 0ull);
    }
    CodonShape out;
    out.regular = sh.regular; out.n_seg = n; out.ref_end = sh.ref_end;
    return out;
}

// The first slot whose start is >= key (n_slots: none)
AMP_ST_HD int32_t codon_lower_bound(const int32_t *starts, int32_t n_slots, int64_t key) {
    int32_t lo = 0, hi = n_slots;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)starts[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A block's window: the slots [a0, a0 + CD_W).  Every slot whose start lies in [wlo, whi) is one of them.
struct CodonWindow {
    int32_t a0;
    int64_t wlo, whi;
};
// The window for a tile whose regular reads begin at lo: anchored at the first slot whose start is >= lo - 2.
AMP_ST_HD CodonWindow codon_window_at(const int32_t *starts, int32_t n_slots, int32_t lo) {
    CodonWindow w;
    w.wlo = (int64_t)lo - 2;
    w.a0 = codon_lower_bound(starts, n_slots, w.wlo);
    w.whi = (int64_t)w.a0 + CD_W < (int64_t)n_slots ? (int64_t)starts[w.a0 + CD_W] : ((int64_t)1 << 40);
    return w;
}
AMP_ST_HD CodonWindow codon_window_none() {      // before the first tile: no start lies in it
    CodonWindow w;
    w.a0 = 0; w.wlo = 0; w.whi = 0;
    return w;
}
// A tile whose regular reads span [lo, hi) stays on the window when every codon start it can reach, [lo, hi - 3], lies in it;
// otherwise the window is flushed and anchored again.  (No regular read: lo > hi, nothing moves.)
AMP_ST_HD bool codon_window_keeps(const CodonWindow &w, int32_t lo, int32_t hi) {
    return lo > hi || ((int64_t)lo >= w.wlo && (int64_t)hi - 3 < w.whi);
}
// A read takes the window when it is regular, fits its list entries and reaches no start outside the window.
AMP_ST_HD bool codon_read_windowed(const CodonShape &sh, int32_t pos, const CodonWindow &w) {
    return sh.regular && sh.n_seg <= CD_SLOTS && (int64_t)pos >= w.wlo && (int64_t)sh.ref_end - 3 < w.whi;
}

// What an entry adds at the slot with start p (p inside the entry's range): the cell, or nothing.
AMP_ST_HD bool codon_entry_cell(const StrandSeg &g, int32_t p, const uint8_t *seq, const uint8_t *qual, int32_t min_quality, uint32_t &cell) {
    if (cd_seg_break(g)) { cell = (uint32_t)CD_BROKEN; return true; }
    return codon_cell(seq, qual, g.q0 + (uint64_t)(p - g.r0), min_quality, cell);
}

// One read without the window: sink(slot, cell) for every add.  -> whether the read is regular (tallied); a read that is not
// adds nothing.  Every slot handed out lies inside [0, n_slots), every byte read inside the read's l_seq bases.
template <class Sink>
AMP_ST_HD bool codon_read(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, uint32_t qual0,
                          const int32_t *starts, int32_t n_slots, Sink sink) {
    const CodonShape sh = codon_segments(R, P, qual0, [](const StrandSeg &) {});
    if (!sh.regular) return false;
    codon_segments(R, P, qual0, [&](const StrandSeg &g) {
        const int64_t end = (int64_t)g.r0 + st_seg_len(g);
        for (int32_t s = codon_lower_bound(starts, n_slots, g.r0); s < n_slots && (int64_t)starts[s] < end; ++s) {
            uint32_t cell;
            if (codon_entry_cell(g, starts[s], seq, qual, P.min_quality, cell)) sink(s, cell);
        }
    });
    return true;
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is codon_hook of amp_codon.hip, declared in amp_hook.hpp)
