// amp_amplicon.hpp -- per-amplicon allele counts: which amplicon the evidence at a position comes from.
// A read with status 0 is assigned to one amplicon by its ORIGINAL coordinates (amplicon_assign); every increment
// update_base_counts (A:690-753) makes to one of the six fixed keys A C G T N '-' at position r for a read assigned to a adds
// one to amp_counts[cell_off[a] + r - lo_a][c].  What one read asks for and adds is written here as plain functions:
// k_amplicon (amp_amplicon.hip) calls them on the device; tests/hostsim/amplicon_twin.cpp loops the same functions over
// arrays on the CPU, built with plain g++ (no HIP headers: the two attributes are defined away), against the restatement in
// tests/amplicon_util.py.
//
// The two views of a read's alignment are section 16's (amp_strand.hpp): a REGULAR read is a list of segments -- here every
// deletion is handed out, on either strand, and a segment carries the LDS slot of its amplicon in place of the strand -- and
// every other read walks pair by pair through strand_walk, whose positions are bounded to the amplicon's span here.
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

#define AMP_AM_HD __host__ __device__ inline

namespace amp {

constexpr int AM_BLOCK = 256;            // lanes of a k_amplicon block = reads of a tile
constexpr int AM_W = 512;                // reference positions of one slot's window
constexpr int AM_SLOTS = 4;              // windows a block keeps in LDS, each bound to (amplicon, anchor)
constexpr int AM_SEG_SLOTS = 4;          // segment slots per read: a tile's list holds AM_BLOCK * AM_SEG_SLOTS segments, a read that needs more walks serially
constexpr int AM_CHUNK = 64;             // positions a wave takes at a time, one per lane
constexpr int AM_COLS = AMP_NSYM;        // columns of the table: A C G T N '-'
constexpr int AM_STRIDE = 7;             // u32 words of a window position: the six columns and one of padding
constexpr int AM_SLOT_WORDS = AM_W * AM_STRIDE;
constexpr int AM_REQ_PER_WAVE = 8;       // distinct amplicons a wave may ask a slot for in one tile; the others walk serially
constexpr int AM_REQS = AM_REQ_PER_WAVE * (AM_BLOCK / 64);
constexpr int AM_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int AM_BLOCKS_PER_CU = 2;      // ... and the grid stops growing here (the LDS of a block: two fit a CU)
constexpr int AM_MAX_TILES_PER_FLUSH = 1 << 23;      // a cell takes at most 256 adds of one per tile
constexpr int64_t AM_MAX_CELLS = 1ll << 22;          // positions of all spans together (96 MB of table)
static_assert(AM_W % (AM_CHUNK * (AM_BLOCK / 64)) == 0, "every wave owns the same number of chunks of a window");
static_assert(AM_STRIDE > AM_COLS && (AM_STRIDE & 1), "an odd stride: the lanes of a wave hit 64 different banks");
static_assert(AM_SLOTS >= 1 && AM_SLOTS <= 8, "a segment keeps its slot in three bits");
static_assert((uint64_t)AM_MAX_TILES_PER_FLUSH * 256u < (1ull << 32), "a window cell cannot overflow before its flush");

// The amplicon set as the device sees it.
struct AmpliconTables {
    int32_t ref_len;
    int32_t n_amp;
    const int32_t *lo, *hi;              // [n_amp] spans, half-open, 0 <= lo < hi <= ref_len
    const uint32_t *cell_off;            // [n_amp] first row of the amplicon in amp_counts
    const int32_t *amp_start, *amp_end;  // [ref_len] owner tables, -1: none
};

// Reference length of a CIGAR (BAM words len << 4 | op): ops M D N = X consume the reference.
AMP_AM_HD int64_t am_cigar_ref_len(const uint32_t *cig, uint32_t n_ops) {
    int64_t r = 0;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t v = cig[k], op = v & 15u;
        if (op == ST_OP_M || op == ST_OP_D || op == ST_OP_N || op == ST_OP_EQ || op == ST_OP_X) r += (int64_t)(v >> 4);
    }
    return r;
}

// The amplicon of a read that came in at [p, e): the first of amp_start[p], amp_end[e - 1] whose span contains the read,
// -1: none.  An owner entry outside [0, n_amp) is no candidate.
AMP_AM_HD int32_t amplicon_assign(int32_t p, int64_t e, const AmpliconTables &T) {
    if (p >= 0 && p < T.ref_len) {
        const int32_t a = T.amp_start[p];
        if (a >= 0 && a < T.n_amp && T.lo[a] <= p && e <= (int64_t)T.hi[a]) return a;
    }
    if (e > 0 && e <= (int64_t)T.ref_len) {
        const int32_t a = T.amp_end[e - 1];
        if (a >= 0 && a < T.n_amp && T.lo[a] <= p && e <= (int64_t)T.hi[a]) return a;
    }
    return -1;
}

// A segment of a regular read: a StrandSeg with len_kind = length << 4 | slot << 1 | deletion.
using AmSeg = StrandSeg;
AMP_AM_HD int32_t am_seg_len(const AmSeg &s) { return (int32_t)(s.len_kind >> 4); }
AMP_AM_HD int am_seg_slot(const AmSeg &s) { return (int)((s.len_kind >> 1) & 7u); }
AMP_AM_HD bool am_seg_del(const AmSeg &s) { return (s.len_kind & 1u) != 0u; }

// The segments of a read, in CIGAR order, to put(seg): every segment of the scan (regular_scan, amp_strand.hpp), deletions on
// either strand, with the slot in place of the strand.
template <class Put>
AMP_AM_HD StrandShape amplicon_segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, int slot, Put put) {
    return regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t len, bool del) {
        put(AmSeg{r0, (len << 4) | ((uint32_t)slot << 1) | (del ? 1u : 0u), q0});
    });
}

// The bounded pair-by-pair walk: sink(ref_pos, col) for every increment of the read inside [lo, hi).  A position outside
// the span cannot come from a read with status 0 -- the counted alignment lies inside the original one, and the original one
// inside the span it was assigned to -- and is dropped here all the same, so that no caller indexes past an amplicon's rows.
template <class Sink>
AMP_AM_HD void amplicon_walk(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, int32_t lo, int32_t hi, Sink sink) {
    strand_walk(R, P, seq, qual, [&](int32_t r, uint32_t col, uint32_t) {
        if (r >= lo && r < hi && col < (uint32_t)AM_COLS) sink(r, col);
    });
}

// The LDS cell of column c at window position wpos of slot k
AMP_AM_HD int am_cell(int slot, int32_t wpos, uint32_t col) { return (slot * AM_W + wpos) * AM_STRIDE + (int)col; }

// ---- slots ----------------------------------------------------------------------------------------------------------------
// A block's windows and what they are bound to.  amp / anchor: the binding the cells were added under (amp -1: free);
// new_amp / new_anchor: the binding from this tile on, written by amplicon_resolve and taken over by amplicon_commit once the
// slots in `flush` have gone to the table under the old one.
struct AmSlots {
    int32_t amp[AM_SLOTS], anchor[AM_SLOTS];
    int32_t new_amp[AM_SLOTS], new_anchor[AM_SLOTS];
    uint32_t flush;                      // bit k: slot k goes to the table before the commit
    uint32_t used;                       // bit k: a read of this tile asked for slot k's amplicon
    uint32_t victim;                     // where the search for a slot to give away starts
};

// What a tile asks: a window for amplicon amp (whose span starts at span_lo) that holds [lo, hi).
struct AmReq {
    int32_t amp, lo, hi, span_lo;
};
// Where a window that must hold the request is anchored: at the start of the span when the request fits from there (a span
// of up to AM_W positions never moves again, whatever the order of the reads), else at the request's first position.
AMP_AM_HD int32_t am_anchor_for(const AmReq &q) { return (int64_t)q.hi - (int64_t)q.span_lo <= (int64_t)AM_W ? q.span_lo : q.lo; }

AMP_AM_HD void amplicon_slots_init(AmSlots &S) {
    for (int k = 0; k < AM_SLOTS; ++k) { S.amp[k] = S.new_amp[k] = -1; S.anchor[k] = S.new_anchor[k] = 0; }
    S.flush = 0u; S.used = 0u; S.victim = 0u;
}

// A read asks for a window when its segments are its whole counted set, fit the list and lie inside its amplicon's span.
AMP_AM_HD bool amplicon_wants_slot(int32_t a, const StrandShape &sh, int32_t pos, int32_t lo_a, int32_t hi_a) {
    return a >= 0 && sh.regular && sh.n_seg > 0 && sh.n_seg <= AM_SEG_SLOTS && pos >= lo_a && sh.ref_end <= hi_a;
}

// One tile's requests (any order, an amplicon may come more than once: req is merged in place) against the slots.  An
// amplicon that has a slot keeps it; its anchor moves (am_anchor_for) when the tile does not fit the window as it
// stands (an amplicon longer than AM_W moves along this way).  The others take a free slot, then a slot no request of this
// tile names, starting at `victim`; when every slot is named, they get none and their reads walk serially.  One caller.
AMP_AM_HD void amplicon_resolve(AmSlots &S, AmReq *req, int n) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        int j = 0;
        while (j < m && req[j].amp != req[i].amp) ++j;
        if (j == m) { req[m++] = req[i]; continue; }
        if (req[i].lo < req[j].lo) req[j].lo = req[i].lo;
        if (req[i].hi > req[j].hi) req[j].hi = req[i].hi;
    }
    uint32_t used = 0u, flush = 0u;
    for (int k = 0; k < AM_SLOTS; ++k) { S.new_amp[k] = S.amp[k]; S.new_anchor[k] = S.anchor[k]; }
    for (int j = 0; j < m; ++j) {
        for (int k = 0; k < AM_SLOTS; ++k) {
            if (S.amp[k] != req[j].amp) continue;
            used |= 1u << k;
            if (!(req[j].lo >= S.anchor[k] && (int64_t)req[j].hi <= (int64_t)S.anchor[k] + AM_W)) { flush |= 1u << k; S.new_anchor[k] = am_anchor_for(req[j]); }
            req[j].amp = -1 - req[j].amp;            // placed
            break;
        }
    }
    for (int j = 0; j < m; ++j) {
        if (req[j].amp < 0) continue;
        int k = -1;
        for (int t = 0; t < AM_SLOTS && k < 0; ++t) {
            const int kk = (int)((S.victim + (uint32_t)t) % (uint32_t)AM_SLOTS);
            if (!((used >> kk) & 1u) && S.amp[kk] < 0) k = kk;
        }
        for (int t = 0; t < AM_SLOTS && k < 0; ++t) {
            const int kk = (int)((S.victim + (uint32_t)t) % (uint32_t)AM_SLOTS);
            if (!((used >> kk) & 1u)) k = kk;
        }
        if (k < 0) continue;
        if (S.amp[k] >= 0) flush |= 1u << k;
        S.new_amp[k] = req[j].amp; S.new_anchor[k] = am_anchor_for(req[j]);
        used |= 1u << k;
        S.victim = (uint32_t)(k + 1) % (uint32_t)AM_SLOTS;
    }
    S.flush = flush; S.used = used;
}

AMP_AM_HD void amplicon_commit(AmSlots &S) {
    for (int k = 0; k < AM_SLOTS; ++k) { S.amp[k] = S.new_amp[k]; S.anchor[k] = S.new_anchor[k]; }
    S.flush = 0u;
}

// The slot bound to amplicon a, -1: none
AMP_AM_HD int amplicon_slot_of(const AmSlots &S, int32_t a) {
    if (a < 0) return -1;
    for (int k = 0; k < AM_SLOTS; ++k)
        if (S.amp[k] == a) return k;
    return -1;
}

// The slot a read's segments go to, -1: the read walks serially.  Only a slot that a request of this tile named takes
// segments (phase B visits those): a read whose wave had more distinct amplicons than requests walks, slot or no slot.
AMP_AM_HD int amplicon_read_slot(const AmSlots &S, int32_t a, const StrandShape &sh, int32_t pos, int32_t lo_a, int32_t hi_a) {
    if (!amplicon_wants_slot(a, sh, pos, lo_a, hi_a)) return -1;
    const int k = amplicon_slot_of(S, a);
    if (k < 0 || !((S.used >> k) & 1u)) return -1;
    return (pos >= S.anchor[k] && (int64_t)sh.ref_end <= (int64_t)S.anchor[k] + AM_W) ? k : -1;
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is amplicon_hook of amp_amplicon.hip, declared in amp_hook.hpp)
