// amp_strand.hpp -- per-allele strand and base-quality tallies: for every increment update_base_counts
// (A:690-753) makes to one of the six fixed keys A C G T N '-' of a position, rev[r][c] += 1 when the read is on the reverse
// strand and qsum[r][c] += the base's quality (the five base columns; a deleted position has none).  What one read and one
// base add is written here as plain functions: k_strand (amp_strand.hip) calls them on the device;
// tests/hostsim/strand_twin.cpp loops the same functions over arrays on the CPU, built with plain g++ (no HIP headers: the
// two attributes are defined away), against the restatement in tests/strand_util.py.
//
// Two views of a read's alignment.  regular_scan (under strand_segments, and under amplicon_segments and codon_segments of
// amp_amplicon.hpp and amp_codon.hpp): a read with a REGULAR CIGAR -- hard clips, then soft clips, then a core
// of M = X I D N ops, then soft clips, then hard clips, its query bases adding up to l_seq -- is a list of segments: a match
// segment (reference start, query start, length) per M = X op and a deletion segment (reference start, length) per D N op.
// On such a read every pair of a match op lies inside [query_alignment_start, query_alignment_end), the pairs the insertion
// scan (A:730-748) swallows are inserted or clipped bases, and no pair follows the break of A:726 that could count: the
// counted set is every deleted position and every match base whose quality reaches min_quality.  six_key_walk: the six-key
// part of the exact walk (count_read_walk, amp_read.hpp) for every other read, pair by pair, with the quality test in front
// of the soft-clip tests, the break at the first good base at or past query_alignment_end, and the insertion scan's pairs;
// strand_walk and readpos_walk (amp_readpos.hpp) are its two adapters.  StrandTally, at the end: what k_strand's loop
// (tally_poswin, amp_tally.hpp) and the twin's (poswin_twin.hpp) are told about this tally.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/amplihip.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#define AMP_ST_HD __host__ __device__ inline

namespace amp {

constexpr int ST_BLOCK = 256;            // lanes of a k_strand block = reads of a tile
constexpr int ST_SLOTS = 4;              // segment slots per read: a tile's list holds ST_BLOCK * ST_SLOTS segments, a read that needs more walks serially
constexpr int ST_CHUNK = 64;             // positions a wave takes at a time, one per lane
constexpr int ST_W = 512;                // reference positions of a block's window
constexpr int ST_REV_COLS = AMP_NSYM;    // columns of rev: A C G T N '-'
constexpr int ST_QSUM_COLS = 5;          // columns of qsum: A C G T N
constexpr int ST_CELLS = ST_REV_COLS + ST_QSUM_COLS;      // u32 cells of a window position: rev, then qsum
constexpr int ST_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int ST_BLOCKS_PER_CU = 4;      // ... and the grid stops growing here
constexpr int ST_MAX_TILES_PER_FLUSH = 32768;      // a cell takes at most 256 adds of at most 255 per tile: 32768 tiles stay below 2^32

constexpr uint32_t ST_OP_M = 0, ST_OP_I = 1, ST_OP_D = 2, ST_OP_N = 3, ST_OP_S = 4, ST_OP_H = 5, ST_OP_P = 6, ST_OP_EQ = 7, ST_OP_X = 8;
AMP_ST_HD bool st_is_match(uint32_t op) { return op == ST_OP_M || op == ST_OP_EQ || op == ST_OP_X; }
AMP_ST_HD bool st_is_del(uint32_t op) { return op == ST_OP_D || op == ST_OP_N; }

struct StrandParams {
    int32_t ref_len;
    int32_t min_quality;
};

// One read as the tallies see it: the alignment that was counted (the trimmed one with do_trim), and where its bytes lie.
struct StrandRead {
    int32_t pos;
    const uint32_t *cig;
    uint32_t n_ops;
    int32_t lseq;
    uint32_t rev;          // FLAG & 0x10
    uint64_t base;         // index of the read's first base in qual (bytes) and seq (nibbles)
};

// A segment of a regular read.  len_kind = length << 2 | deletion << 1 | reverse strand; q0: the index in qual / seq of the
// segment's first base (match segments).
struct StrandSeg {
    int32_t r0;
    uint32_t len_kind;
    uint64_t q0;
};
AMP_ST_HD int32_t st_seg_len(const StrandSeg &s) { return (int32_t)(s.len_kind >> 2); }
AMP_ST_HD bool st_seg_del(const StrandSeg &s) { return (s.len_kind & 2u) != 0u; }
AMP_ST_HD bool st_seg_rev(const StrandSeg &s) { return (s.len_kind & 1u) != 0u; }

// BAM 4-bit code -> column, 0xFF: none of A C G T N
AMP_ST_HD uint32_t st_code_to_col(uint32_t code) {
    return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : code == 15 ? 4u : 0xFFu;
}
AMP_ST_HD uint32_t st_base_code(const uint8_t *seq, uint64_t k) {
    const uint32_t b = seq[k >> 1];
    return (k & 1) ? (b & 15u) : (b >> 4);
}

struct StrandShape {
    bool regular;          // the segments are the read's whole counted set, and all of it lies inside the reference
    int32_t n_seg;         // segments handed out
    int32_t ref_end;       // pos + the reference bases of the CIGAR (regular reads)
};
constexpr StrandShape ST_NO_READ = {false, 0, 0};         // what a lane without a live read carries

// The scan of a read's CIGAR, the one place where "regular" is decided: put(r0, q_index, len, is_del) for every non-empty
// match and deletion segment in CIGAR order (q_index: the index in qual / seq of a match segment's first base), n_seg of
// them; the shape says whether they may be used.  qual0: the read's first quality byte (0xFF: QUAL '*').
template <class Put>
AMP_ST_HD StrandShape regular_scan(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) {
    StrandShape sh;
    sh.regular = false; sh.n_seg = 0; sh.ref_end = R.pos;
    int phase = 0;                       // 0 leading H, 1 leading S, 2 core, 3 trailing S, 4 trailing H
    int64_t q = 0, r = R.pos;
    bool ok = R.lseq > 0 && qual0 != 0xFFu && R.pos >= 0;
    for (uint32_t k = 0; ok && k < R.n_ops; ++k) {
        const uint32_t v = R.cig[k], op = v & 15u;
        const int64_t len = (int64_t)(v >> 4);
        if (op == ST_OP_H) {
            if (phase == 1) ok = false;
            else if (phase >= 2) phase = 4;
        } else if (op == ST_OP_S) {
            if (phase <= 1) phase = 1;
            else if (phase <= 3) phase = 3;
            else ok = false;
            q += len;
        } else if (st_is_match(op) || op == ST_OP_I || st_is_del(op)) {
            if (phase > 2) { ok = false; break; }
            phase = 2;
            if (op == ST_OP_I) { q += len; continue; }
            const bool del = st_is_del(op);
            if (r + len > (int64_t)P.ref_len || (!del && q + len > (int64_t)R.lseq)) { ok = false; break; }
            if (len > 0) {
                put((int32_t)r, R.base + (uint64_t)q, (uint32_t)len, del);
                ++sh.n_seg;
            }
            if (!del) q += len;
            r += len;
        } else {
            ok = false;                  // P, and op codes the format does not have
        }
    }
    sh.regular = ok && phase >= 2 && q == (int64_t)R.lseq;
    sh.ref_end = (int32_t)r;
    return sh;
}

// The segments the strand tallies use, to put(seg): the scan's, without a forward read's deletions (they add nothing; n_seg
// leaves them out).
template <class Put>
AMP_ST_HD StrandShape strand_segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) {
    int32_t n = 0;
    StrandShape sh = regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t len, bool del) {
        if (del && !R.rev) return;
        put(StrandSeg{r0, (len << 2) | (del ? 2u : 0u) | (R.rev ? 1u : 0u), q0});
        ++n;
    });
    sh.n_seg = n;
    return sh;
}

// What one base of a match segment adds: col < 5 and its quality when it is counted.
AMP_ST_HD bool strand_base(const uint8_t *seq, const uint8_t *qual, uint64_t k, int32_t min_quality, uint32_t &col, uint32_t &qv) {
    qv = qual[k];
    col = st_code_to_col(st_base_code(seq, k));
    return (int32_t)qv >= min_quality && col < (uint32_t)ST_QSUM_COLS;
}

// The window rule of the position-window tallies (k_strand, k_readpos), on W positions and SLOTS segment slots per read.  A
// tile whose regular reads span [lo, hi) stays on a window anchored at `anchor` when all of them fit it; otherwise the window
// is flushed and anchored again at lo.  (No regular read: lo > hi, nothing moves.)
template <int W>
AMP_ST_HD bool poswin_keeps(int32_t anchor, int32_t lo, int32_t hi) {
    return lo > hi || (lo >= anchor && (int64_t)hi <= (int64_t)anchor + W);
}
// A read takes the window when it is regular, fits its slots and lies inside the window.
template <int W, int SLOTS>
AMP_ST_HD bool poswin_read_windowed(const StrandShape &sh, int32_t pos, int32_t anchor) {
    return sh.regular && sh.n_seg <= SLOTS && pos >= anchor && (int64_t)sh.ref_end <= (int64_t)anchor + W;
}
// The rule and the window cells of column c under the strand tallies' own names, for callers that name them: one-line forwards
AMP_ST_HD bool strand_window_keeps(int32_t anchor, int32_t lo, int32_t hi) { return poswin_keeps<ST_W>(anchor, lo, hi); }
AMP_ST_HD bool strand_read_windowed(const StrandShape &sh, int32_t pos, int32_t anchor) { return poswin_read_windowed<ST_W, ST_SLOTS>(sh, pos, anchor); }
AMP_ST_HD int st_cell_rev(int32_t wpos, uint32_t col) { return wpos * ST_CELLS + (int)col; }
AMP_ST_HD int st_cell_qsum(int32_t wpos, uint32_t col) { return st_cell_rev(wpos, col) + ST_REV_COLS; }

// query_alignment_start / _end of pysam as count_read_walk reads them (hard clips skipped; a hard clip inside the soft clip
// raises: such a read has a status and adds nothing).
AMP_ST_HD bool st_query_bounds(const StrandRead &R, int32_t &qs, int32_t &qe) {
    int32_t off = 0;
    for (uint32_t i = 0; i < R.n_ops; ++i) {
        const uint32_t v = R.cig[i], op = v & 15u;
        if (op == ST_OP_H) { if (off != 0 && off != R.lseq) return false; }
        else if (op == ST_OP_S) off += (int32_t)(v >> 4);
        else break;
    }
    qs = off;
    int32_t end = R.lseq;
    for (int64_t k = (int64_t)R.n_ops - 1; k >= 1; --k) {      // element 0 is never examined
        const uint32_t v = R.cig[k], op = v & 15u;
        if (op == ST_OP_H) { if (end != R.lseq) return false; }
        else if (op == ST_OP_S) end -= (int32_t)(v >> 4);
        else break;
    }
    qe = end;
    return true;
}

// The aligned pairs of a CIGAR one at a time (q or r -1: None); zero-length ops, hard clips and op codes >= 9 have none, a
// padding op gives (q, None) like an insertion.
struct StrandPairs {
    const uint32_t *cig;
    uint32_t n, k;
    int32_t j, len, q, r;
    uint32_t op;
    AMP_ST_HD void init(const StrandRead &R) { cig = R.cig; n = R.n_ops; k = 0; j = 0; len = 0; q = 0; r = R.pos; op = ST_OP_H; }
    AMP_ST_HD bool next(int32_t &pq, int32_t &pr) {
        while (j >= len) {
            if (k >= n) return false;
            const uint32_t v = cig[k++];
            op = v & 15u; j = 0;
            len = (op == ST_OP_H || op >= 9u) ? 0 : (int32_t)(v >> 4);
        }
        ++j;
        if (st_is_match(op)) { pq = q++; pr = r++; }
        else if (st_is_del(op)) { pq = -1; pr = r++; }
        else { pq = q++; pr = -1; }
        return true;
    }
};

// The six-key part of the exact walk for one read, the one copy of it: sink(ref_pos, col, q, qs, qe) for every increment, with
// the read's query bounds [qs, qe).  A match base: col < 5 and q its query index.  A deleted position: col 5 and q the query
// index the next pair with one takes.  Where the reference raises the read has a status and its adds are unspecified: the walk
// ends there.  Every position handed out lies inside [0, ref_len), every byte read and every q of a match base inside the
// read's l_seq bases.
template <class Sink>
AMP_ST_HD void six_key_walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Sink sink) {
    int32_t qs, qe;
    if (!st_query_bounds(R, qs, qe) || R.lseq <= 0) return;
    const bool have_qual = qual[R.base] != 0xFFu;
    StrandPairs it;
    it.init(R);
    int32_t q, r;
    bool pending = false;
    int32_t pend_q = 0, pend_r = 0;
    for (;;) {
        if (pending) { q = pend_q; r = pend_r; pending = false; }
        else if (!it.next(q, r)) break;
        if (q < 0) {                                                                       // A:714-715
            if ((uint32_t)r >= (uint32_t)P.ref_len) return;
            sink(r, 5u, it.q, qs, qe);                                                     // (it.q: the next pair's query index)
            continue;
        }
        if (!have_qual || q >= R.lseq) return;
        if ((int32_t)qual[R.base + (uint64_t)q] < P.min_quality) continue;                 // A:718
        if (q < qs) continue;                                                              // A:722
        if (q >= qe) break;                                                                // A:726
        if (r < 0) {                                                                       // A:730-748: the scan takes pairs with it
            bool q_none = false;
            while (r < 0 && !q_none && q < qe) {
                if (q >= R.lseq) return;
                if ((int32_t)qual[R.base + (uint64_t)q] < P.min_quality) break;
                if (!it.next(q, r)) return;                                                // A:734
                if (q < 0) q_none = true;
            }
            if (r >= 0) { pending = true; pend_q = q; pend_r = r; }                        // A:742-743
            continue;
        }
        if ((uint32_t)r >= (uint32_t)P.ref_len) return;                                    // A:751-753
        const uint32_t col = st_code_to_col(st_base_code(seq, R.base + (uint64_t)q));
        if (col == 0xFFu) return;
        sink(r, col, q, qs, qe);
    }
}

// The walk as the strand tallies, amplicon_walk and del_events_walk take it: sink(ref_pos, col, quality) (col 5: quality 0)
template <class Sink>
AMP_ST_HD void strand_walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Sink sink) {
    six_key_walk(R, P, seq, qual, [&](int32_t r, uint32_t col, int32_t q, int32_t, int32_t) {
        sink(r, col, col == 5u ? 0u : (uint32_t)qual[R.base + (uint64_t)q]);
    });
}

// The strand tallies as tally_poswin (amp_tally.hpp) and its CPU twin (tests/hostsim/poswin_twin.hpp) take them.  A window
// position has WORDS = 11 u32 words, one per cell: six reverse counts, then five quality sums.  "add(c, v)": cell c of the
// position at hand gets v.
struct StrandTally {
    static constexpr int BLOCK = ST_BLOCK, SLOTS = ST_SLOTS, CHUNK = ST_CHUNK, W = ST_W, WORDS = ST_CELLS, MAX_TILES_PER_FLUSH = ST_MAX_TILES_PER_FLUSH;
    using Seg = StrandSeg;
    struct Out {
        uint32_t *rev;                   // [ref_len][6]
        unsigned long long *qsum;        // [ref_len][5]
    };
    template <class Put>
    static AMP_ST_HD StrandShape segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, Put put) { return strand_segments(R, P, qual0, put); }
    // what a segment adds at offset k of its span (a forward read's deletions are not in the list)
    template <class Add>
    static AMP_ST_HD void seg_adds(const Seg &g, int32_t k, const uint8_t *seq, const uint8_t *qual, int32_t min_quality, Add add) {
        if (st_seg_del(g)) {
            add(5, 1u);
        } else {
            uint32_t col, qv;
            if (strand_base(seq, qual, g.q0 + (uint64_t)k, min_quality, col, qv)) {
                add(ST_REV_COLS + (int)col, qv);
                if (st_seg_rev(g)) add((int)col, 1u);
            }
        }
    }
    // the serial walk, sink(ref_pos, col, quality), and what one of its increments adds
    template <class Sink>
    static AMP_ST_HD void walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, Sink sink) { strand_walk(R, P, seq, qual, sink); }
    template <class Add>
    static AMP_ST_HD void walk_adds(const StrandRead &R, uint32_t col, uint32_t qv, Add add) {
        if (R.rev) add((int)col, 1u);
        if (col < (uint32_t)ST_QSUM_COLS) add(ST_REV_COLS + (int)col, qv);
    }
    // the window word of cell c of window position w, and what an add of v adds to it
    static AMP_ST_HD int word(int32_t w, int c) { return w * ST_CELLS + c; }
    static AMP_ST_HD uint32_t inc(int, uint32_t v) { return v; }
    // cell c of table position p gets v, by plus(address, v); word k of a flushed window position is cell k
    template <class Plus>
    static AMP_ST_HD void to_table(const Out &o, size_t p, int c, uint32_t v, Plus plus) {
        if (c < ST_REV_COLS) plus(&o.rev[p * ST_REV_COLS + c], v);
        else plus(&o.qsum[p * ST_QSUM_COLS + (c - ST_REV_COLS)], (unsigned long long)v);
    }
    template <class Plus>
    static AMP_ST_HD void flush_word(const Out &o, size_t p, int k, uint32_t v, Plus plus) { to_table(o, p, k, v, plus); }
};
static_assert(StrandTally::WORDS == 11 && (StrandTally::WORDS & 1), "an odd stride: the lanes of a wave hit 64 different banks");
static_assert((uint64_t)StrandTally::MAX_TILES_PER_FLUSH * StrandTally::BLOCK * 255u < (1ull << 32), "a window cell cannot overflow before its flush");
}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is strand_hook of amp_strand.hip, declared in amp_hook.hpp)
