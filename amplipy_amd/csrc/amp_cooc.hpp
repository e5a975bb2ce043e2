// amp_cooc.hpp -- co-occurrence of listed mutations on single reads.  A SET is 1 to CO_SITES sites in
// strictly increasing position that do not overlap; a site is a substitution (p, b), b one of A C G T, or a deletion (p, len),
// len >= 1; positions are 0-based.  The sets are sorted by the position of their first site.  A REGULAR read (regular_scan,
// amp_strand.hpp) whose counted alignment is [pos, ref_end) gives every site of a set one of three states ("deleted": inside
// a D or N op):
//   substitution (p, b): p is a match position whose base is among A C G T with quality >= min_quality: MUT when the base is
//     b, NOT otherwise; p is deleted: NOT; anything else (p outside [pos, ref_end), base N, low quality): NONE;
//   deletion (p, len): NONE unless p - 1 and p + len both lie in [pos, ref_end); then MUT when every position of
//     [p, p + len) is deleted and neither p - 1 nor p + len is, NOT otherwise.  No quality test; the rule is about positions,
//     not ops (3D2D is one run of five deleted positions).
// and adds to the set: all sites MUT or NOT: cooc[set][sum of 2^j over the sites j that are MUT] += 1; at least one but not all:
// cooc[set][64] += 1 (partial); none: nothing.  Every other read with status 0 adds nothing and is counted as skipped.
// Insertions are not sites.  What one read adds to one set is written here as plain functions: k_cooc (amp_cooc.hip) calls
// them on the device; tests/hostsim/cooc_twin.cpp loops the same functions over arrays on the CPU, built with plain g++,
// against the restatement in tests/cooc_util.py.
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

namespace amp {

constexpr int CO_BLOCK = 256;            // lanes of a k_cooc block = reads of a tile
constexpr int CO_SITES = 6;              // sites of a set at most: 2^6 patterns
constexpr int CO_CELLS = 65;             // u32 cells of a set: the 64 patterns (site 0 is bit 0), then partial
constexpr int CO_PARTIAL = 64;
constexpr int CO_W = 192;                // sets of a block's window
constexpr int CO_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int CO_BLOCKS_PER_CU = 3;      // ... and the grid stops growing here (49.9 KB of LDS: three blocks share a CU)
constexpr int CO_MAX_TILES_PER_FLUSH = 1 << 23;     // a cell takes at most one add per read: 256 per tile
constexpr int32_t CO_MAX_SETS = 1 << 16;
constexpr int32_t CO_MAX_SPAN = 1 << 16;            // last site's position minus the first site's, at most
static_assert((1 << CO_SITES) == CO_PARTIAL && CO_CELLS == CO_PARTIAL + 1, "one cell per pattern, then partial");
static_assert(CO_CELLS & 1, "an odd stride: the cells of neighbouring sets lie in different banks");
static_assert((uint64_t)CO_MAX_TILES_PER_FLUSH * CO_BLOCK < (1ull << 32), "a window cell cannot overflow before its flush");
static_assert((int64_t)CO_MAX_SETS * CO_CELLS < (1ll << 31), "a key, set * 65 + cell, is a positive int32");
static_assert((size_t)CO_W * CO_CELLS * 4 <= 50 * 1024, "the window leaves room for three blocks in a CU's 160 KB of LDS");

// The sets as a kernel or the twin is handed them: set s has the sites [off[s], off[s + 1]); first[s] = pos[off[s]],
// non-decreasing; len 0: a substitution to sym (0..3 for A C G T); max_span: the greatest pos[off[s + 1] - 1] - first[s].
struct CoocSets {
    int32_t n_sets;
    const int32_t *first, *off, *pos, *len, *sym;
    int32_t max_span;
};

// BAM 4-bit code -> 0..3 for A C G T, 0xFF otherwise
AMP_ST_HD uint32_t co_code_to_base(uint32_t code) { return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 0xFFu; }

// The first set whose first site is >= key (n_sets: none)
AMP_ST_HD int32_t cooc_lower_bound(const int32_t *first, int32_t n_sets, int64_t key) {
    int32_t lo = 0, hi = n_sets;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)first[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The sets that can have an informative site on a read over [pos, ref_end) are among [cooc_first_candidate, the first set
// whose first site is >= ref_end): a set in front of them has its last site below pos, a set behind them its first site at
// or past ref_end -- and a deletion site there would need p + len < ref_end.
AMP_ST_HD int32_t cooc_first_candidate(const CoocSets &S, int32_t pos) { return cooc_lower_bound(S.first, S.n_sets, (int64_t)pos - S.max_span); }
AMP_ST_HD bool cooc_is_candidate(const CoocSets &S, int32_t s, int32_t ref_end) { return s < S.n_sets && S.first[s] < ref_end; }

// What a regular read over [R.pos, ref_end) adds to set s: the cell, or nothing when no site is informative.  One scan of the
// CIGAR; per substitution site one nibble and one quality byte at most, inside the read's l_seq bases.  Bit j of `inf`: site j is
// MUT or NOT; of `mut`: it is MUT.  For a deletion site, `ov`: a match segment overlaps [p, p + len); `fl` / `fr`: a match
// segment holds p - 1 / p + len.  (Inside [pos, ref_end) a position is a match position or deleted.)
AMP_ST_HD bool cooc_read_set(const StrandRead &R, const StrandParams &P, uint32_t qual0, int32_t ref_end, const uint8_t *seq, const uint8_t *qual,
                             const CoocSets &S, int32_t s, uint32_t &cell) {
    const int32_t o = S.off[s];
    const int n = (int)(S.off[s + 1] - o);
    int32_t sp[CO_SITES], sl[CO_SITES];
    uint32_t sb[CO_SITES];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CO_SITES; ++j) {
        const bool have = j < n;
        sp[j] = have ? S.pos[o + j] : 0; sl[j] = have ? S.len[o + j] : 0; sb[j] = have ? (uint32_t)S.sym[o + j] : 0u;
    }
    uint32_t inf = 0u, mut = 0u, ov = 0u, fl = 0u, fr = 0u;
    regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t seg_len, bool del) {
        const int64_t a = r0, b = (int64_t)r0 + seg_len;      // the segment is [a, b)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < CO_SITES; ++j) {
            if (j >= n) continue;
            const int64_t p = sp[j], e = p + sl[j];
            if (sl[j] == 0) {
                if (p < a || p >= b) continue;
                if (del) { inf |= 1u << j; continue; }
                const uint64_t k = q0 + (uint64_t)(p - a);
                const uint32_t base = co_code_to_base(st_base_code(seq, k));
                if (base < 4u && (int32_t)qual[k] >= P.min_quality) {
                    inf |= 1u << j;
                    if (base == sb[j]) mut |= 1u << j;
                }
            } else if (!del) {
                if (a < e && b > p) ov |= 1u << j;
                if (p - 1 >= a && p - 1 < b) fl |= 1u << j;
                if (e >= a && e < b) fr |= 1u << j;
            }
        }
    });
    for (int j = 0; j < CO_SITES; ++j) {
        if (j >= n || sl[j] == 0) continue;
        if ((int64_t)sp[j] - 1 < (int64_t)R.pos || (int64_t)sp[j] + sl[j] >= (int64_t)ref_end) continue;
        inf |= 1u << j;
        if (!((ov >> j) & 1u) && ((fl >> j) & 1u) && ((fr >> j) & 1u)) mut |= 1u << j;
    }
    if (!inf) return false;
    cell = inf == (1u << n) - 1u ? mut : (uint32_t)CO_PARTIAL;
    return true;
}

// One read: sink(set, cell) for every add.  -> whether the read is regular (tallied); a read that is not adds nothing.  Every
// set handed out lies inside [0, n_sets), every cell inside [0, 65).
template <class Sink>
AMP_ST_HD bool cooc_read(const StrandRead &R, const StrandParams &P, const uint8_t *seq, const uint8_t *qual, uint32_t qual0, const CoocSets &S, Sink sink) {
    const StrandShape sh = regular_scan(R, P, qual0, [](int32_t, uint64_t, uint32_t, bool) {});
    if (!sh.regular) return false;
    for (int32_t s = cooc_first_candidate(S, R.pos); cooc_is_candidate(S, s, sh.ref_end); ++s) {
        uint32_t cell;
        if (cooc_read_set(R, P, qual0, sh.ref_end, seq, qual, S, s, cell)) sink(s, cell);
    }
    return true;
}

// A block's window: the sets [a0, a0 + CO_W).  Every set whose first site lies in [wlo, whi) is one of them.  A key outside it
// goes to the global table, so the window decides cost, never the result.
struct CoocWindow {
    int32_t a0;
    int64_t wlo, whi;
};
// The window for a tile whose regular reads begin at lo: anchored at the first candidate of a read at lo.  A set list that
// fits the window whole never moves.
AMP_ST_HD CoocWindow cooc_window_at(const CoocSets &S, int32_t lo) {
    CoocWindow w;
    if (S.n_sets <= CO_W) { w.a0 = 0; w.wlo = -((int64_t)1 << 40); w.whi = (int64_t)1 << 40; return w; }
    w.wlo = (int64_t)lo - S.max_span;
    w.a0 = cooc_lower_bound(S.first, S.n_sets, w.wlo);
    w.whi = (int64_t)w.a0 + CO_W < (int64_t)S.n_sets ? (int64_t)S.first[w.a0 + CO_W] : ((int64_t)1 << 40);
    return w;
}
AMP_ST_HD CoocWindow cooc_window_none() {      // before the first tile: no set lies in it
    CoocWindow w;
    w.a0 = 0; w.wlo = 0; w.whi = 0;
    return w;
}
// A tile whose regular reads span [lo, hi) stays on the window when every candidate of its reads -- first site in
// [lo - max_span, hi) -- lies in it; otherwise the window is flushed and anchored again.  (No regular read: lo > hi.)
AMP_ST_HD bool cooc_window_keeps(const CoocWindow &w, const CoocSets &S, int32_t lo, int32_t hi) {
    return lo > hi || ((int64_t)lo - S.max_span >= w.wlo && (int64_t)hi <= w.whi);
}
// The window cell of a key, or -1 when its set lies outside
AMP_ST_HD int32_t cooc_window_cell(const CoocWindow &w, int32_t key) {
    const int64_t k = (int64_t)key - (int64_t)w.a0 * CO_CELLS;
    return k >= 0 && k < (int64_t)CO_W * CO_CELLS ? (int32_t)k : -1;
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is cooc_hook of amp_cooc.hip, declared in amp_hook.hpp)
