// amp_hap.hpp -- read haplotypes per region: the distinct sets of differences from the reference that single reads carry over a
// stretch, and how many reads carry each.
//
// REGIONS.  A region is [start, end), 0-based, of 1 to HP_MAX_REGION = 4096 positions; at most 2^16 of them, sorted by start;
// they may overlap.
// WHICH READS.  Only reads with status 0 take part, as they were counted (the trimmed alignment [pos, ref_end) with do_trim), and
// only those with a regular CIGAR (regular_scan, amp_strand.hpp, as for k_cooc).  Every other status-0 read adds reads[1] += 1
// and nothing else; so does a regular read that covers no region.  Every read that covers at least one region adds
// reads[0] += 1.  A read is tried against every region with pos <= start and end <= ref_end; inside such a region every
// position is a match position or a deleted one (inside a D or N op).
// HOW A REGION IS JUDGED.  Each trial adds tally[region][COVER] += 1 and then exactly one of, tested in this order:
//   1 EDGE      the region's first or last position is deleted (the run may go on outside: it cannot be named);
//   2 LOWQ      some match position has a reference letter among A C G T (either case), a read base that differs from it, and
//               a quality below min_quality (a quality byte of 0xFF counts as below);
//   3 OVERFLOW  the read's differences are more than HP_MAX_DIFFS = 13;
//   4 REF       there is none: tally[region][REF] += 1, and [REF_REV] += 1 when the FLAG has 0x10;
//   5           the key (region, differences) goes to the table: count += 1, and rev += 1 when reverse.
// A DIFFERENCE, collected in ascending offset: a maximal run of deleted positions is one difference of kind 5 with its length
// (after the EDGE test both its flanks are match positions inside the region; 3D2D, and D ops with only an insertion between
// them, are one run); a match position whose reference letter is among A C G T, whose read base differs from it and whose
// quality is at or above min_quality is one difference of kind 0..3 for a read base A C G T and 4 for any other (N).  A
// position whose reference letter is not A C G T is never a difference; a low-quality base that equals the reference is none
// and does not disqualify the read.  INSERTIONS ARE NOT DIFFERENCES, exactly as they are not sites of k_cooc: two reads that
// differ only by an insertion fall together (the insertion alleles are in the VCF).
// THE DIFFERENCE WORD: bits 0-11 the offset in the region, 12-14 the kind, 15-27 the deletion length (0: a substitution), the
// rest zero.  THE KEY: 14 words: head = region | n_diffs << 16, then 13 difference words, the unused ones zero.
// THE INVARIANT, per region, asserted wherever a table is read:
//   COVER == REF + LOWQ + OVERFLOW + EDGE + the counts of the region's entries + the lost reads of that region.
//
// What one read gives one region, the 16-bases-at-once compare, the hash and the word-by-word claim of a slot are written here
// as plain functions: k_hap (amp_hap.hip) calls them on the device; tests/hostsim/hap_twin.cpp loops the same functions over
// arrays on the CPU, built with plain g++, against the restatement in tests/hap_util.py -- and holds the 16-at-once compare to
// the one-base-at-a-time one.
#pragma once

#include <stdint.h>

#include "amp_keyed.hpp"
#include "amp_strand.hpp"

namespace amp {

constexpr int HP_BLOCK = 256;                // lanes of a k_hap block = reads of a tile
constexpr int HP_MAX_DIFFS = 13;
constexpr int HP_KEY_WORDS = 14;             // head, then the difference words
constexpr int HP_KEY_STRIDE = 15;            // words between two lanes' keys in LDS (odd: neighbouring lanes in different banks)
constexpr int HP_MAX_REGION = 4096;
constexpr int32_t HP_MAX_REGIONS = 1 << 16;
constexpr int HP_TALLY_COLS = 6;
constexpr int HP_COVER = 0, HP_REF = 1, HP_REF_REV = 2, HP_LOWQ = 3, HP_OVERFLOW = 4, HP_EDGE = 5;       // the columns of tally
constexpr int HP_KIND_N = 4, HP_KIND_DEL = 5;
constexpr int HP_GLOBAL_PROBES = 4096;       // slots an insert tries (keyed_probes); then the reads are lost
constexpr int HP_LOG2_DEFAULT = 20, HP_LOG2_MIN = 4, HP_LOG2_MAX = 28;      // the table's slots (64 bytes each)
constexpr int HP_TILES_PER_BLOCK = 2;        // a block takes at least this many tiles before another block is added ...
constexpr int HP_BLOCKS_PER_CU = 4;          // ... and the grid stops growing here (15 KB of LDS a block)
constexpr uint32_t HP_EMPTY = 0xFFFFFFFFu;   // no key word: a head has n_diffs <= 13 in its high half, a difference word four zero bits on top
// what a trial comes to
constexpr int HP_OUT_NONE = -1, HP_OUT_REF = 0, HP_OUT_LOWQ = 1, HP_OUT_OVERFLOW = 2, HP_OUT_EDGE = 3, HP_OUT_KEY = 4;
static_assert(HP_MAX_DIFFS == AMP_HAP_MAX_DIFFS && HP_MAX_REGION == AMP_HAP_MAX_REGION && HP_TALLY_COLS == AMP_HAP_TALLY_COLS, "amplihip.h");
static_assert(HP_GLOBAL_PROBES == KEYED_PROBES, "one probe rule (amp_keyed.hpp)");
static_assert(HP_KEY_WORDS == HP_MAX_DIFFS + 1 && sizeof(amp_hap_entry) == 64 && (HP_KEY_STRIDE & 1), "a key is the first 14 words of an entry");
static_assert(HP_MAX_REGION <= (1 << 12) && HP_MAX_REGION < (1 << 13), "offset and deletion length fit their bits");

AMP_ST_HD uint32_t hap_head(int32_t region, int n_diffs) { return (uint32_t)region | ((uint32_t)n_diffs << 16); }
AMP_ST_HD uint32_t hap_diff_word(int32_t offset, uint32_t kind, int32_t del_len) { return (uint32_t)offset | (kind << 12) | ((uint32_t)del_len << 15); }

// A reference letter as enable packs it: the BAM 4-bit code (A C G T either case: 1 2 4 8; anything else 15) and whether it
// is among A C G T
AMP_ST_HD bool hap_ref_acgt(uint8_t ch) {
    const uint8_t u = ch & 0xDFu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
AMP_ST_HD uint32_t hap_ref_code(uint8_t ch) {
    const uint8_t u = ch & 0xDFu;
    return u == 'A' ? 1u : u == 'C' ? 2u : u == 'G' ? 4u : u == 'T' ? 8u : 15u;
}
// BAM 4-bit code of a read base -> kind: 0..3 for A C G T, 4 (N) for anything else
AMP_ST_HD uint32_t hap_kind(uint32_t code) { return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : (uint32_t)HP_KIND_N; }

// The packed reference: codes and mask as nibbles, packed like a read's SEQ (base k in byte k >> 1, the high nibble when k is
// even); a mask nibble is 15 where the letter is among A C G T, 0 elsewhere.
struct HapRef {
    const uint8_t *code4, *mask4;
};
// ... as enable packs it: code4 and mask4 take (ref_len + 1) / 2 bytes each, zero on entry
AMP_ST_HD void hap_pack_ref(const uint8_t *ref_ascii, int32_t ref_len, uint8_t *code4, uint8_t *mask4) {
    for (int32_t p = 0; p < ref_len; ++p) {
        const int sh = (p & 1) ? 0 : 4;
        code4[p >> 1] = (uint8_t)(code4[p >> 1] | (hap_ref_code(ref_ascii[p]) << sh));
        if (hap_ref_acgt(ref_ascii[p])) mask4[p >> 1] = (uint8_t)(mask4[p >> 1] | (15u << sh));
    }
}
struct HapRegions {
    int32_t n;
    const int32_t *start, *end;
};

AMP_ST_HD bool hap_low(uint32_t q, int32_t min_quality) { return q == 0xFFu || (int32_t)q < min_quality; }

// ---- one base at a time: the definition
AMP_ST_HD bool hap_base_differs(uint32_t read_code, uint32_t ref_code, uint32_t mask_nibble) { return mask_nibble != 0u && read_code != ref_code; }

// The n bases of a match stretch, read base index k0 against reference position p0: sink(p, read code) per difference of good
// quality, in ascending p.  -> whether one of low quality was met.
template <class Sink>
AMP_ST_HD bool hap_match1(const uint8_t *seq, const uint8_t *qual, uint64_t k0, const HapRef &F, int32_t p0, int32_t n, int32_t min_quality, Sink sink) {
    bool lowq = false;
    for (int32_t d = 0; d < n; ++d) {
        const uint32_t code = st_base_code(seq, k0 + (uint64_t)d);
        if (!hap_base_differs(code, st_base_code(F.code4, (uint64_t)(p0 + d)), st_base_code(F.mask4, (uint64_t)(p0 + d)))) continue;
        if (hap_low(qual[k0 + (uint64_t)d], min_quality)) lowq = true;
        else sink(p0 + d, code);
    }
    return lowq;
}

// ---- sixteen at a time: the shortcut, held to the above by the twin
// The nibbles [k, k + n) of a, 1 <= n <= 16, as one word: nibble k + j in bits 60 - 4 j .. 63 - 4 j, the rest zero.  Only the
// bytes that hold those nibbles are read.
AMP_ST_HD uint64_t hap_nib16(const uint8_t *a, uint64_t k, int n) {
    const uint64_t b0 = k >> 1, b1 = (k + (uint64_t)n - 1u) >> 1;
    uint64_t v = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) v = (v << 8) | (b0 + (uint64_t)i <= b1 ? (uint64_t)a[b0 + (uint64_t)i] : 0ull);
    if (k & 1u) {
        const uint64_t tail = b0 + 8u <= b1 ? (uint64_t)a[b0 + 8u] : 0ull;
        v = (v << 4) | (tail >> 4);
    }
    return n < 16 ? v & ~(~0ull >> (4 * n)) : v;
}

template <class Sink>
AMP_ST_HD bool hap_match16(const uint8_t *seq, const uint8_t *qual, uint64_t k0, const HapRef &F, int32_t p0, int32_t n, int32_t min_quality, Sink sink) {
    bool lowq = false;
    for (int32_t d = 0; d < n; d += 16) {
        const int m = n - d < 16 ? (int)(n - d) : 16;
        const uint64_t rw = hap_nib16(seq, k0 + (uint64_t)d, m);
        uint64_t x = (rw ^ hap_nib16(F.code4, (uint64_t)(p0 + d), m)) & hap_nib16(F.mask4, (uint64_t)(p0 + d), m);
        while (x) {                          // most words are zero: most of a region equals the reference
            const int j = __builtin_clzll(x) >> 2;
            const int sh = 60 - 4 * j;
            if (hap_low(qual[k0 + (uint64_t)(d + j)], min_quality)) lowq = true;
            else sink(p0 + d + j, (uint32_t)(rw >> sh) & 15u);
            x &= ~(15ull << sh);
        }
    }
    return lowq;
}

// ---- the regions a read is tried against: those with pos <= start and end <= ref_end.  They lie among [hap_first_candidate,
// the first region whose start is >= ref_end).
AMP_ST_HD int32_t hap_first_candidate(const HapRegions &G, int32_t pos) {
    int32_t lo = 0, hi = G.n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (G.start[mid] < pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}
AMP_ST_HD bool hap_is_candidate(const HapRegions &G, int32_t r, int32_t ref_end) { return r < G.n && G.start[r] < ref_end; }
AMP_ST_HD bool hap_covers(const HapRegions &G, int32_t r, int32_t ref_end) { return G.end[r] <= ref_end; }

// What a regular read over [R.pos, ref_end) comes to on region `region` = [rs, re), which it covers: one of HP_OUT_*; with
// HP_OUT_KEY the 14 words of key are the key.  One scan of the CIGAR; only bases of the read inside the region are looked at.
// FAST: the 16-at-once compare.
template <bool FAST>
AMP_ST_HD int hap_judge(const StrandRead &R, const StrandParams &P, uint32_t qual0, const uint8_t *seq, const uint8_t *qual, const HapRef &F, int32_t region,
                        int32_t rs, int32_t re, uint32_t *key) {
    bool edge = false, lowq = false;
    int n = 0;                               // differences met, HP_MAX_DIFFS + 1 at most
    int32_t run_start = 0, run_len = 0;      // the run of deleted positions that is open
    auto put = [&](uint32_t word) {
        if (n < HP_MAX_DIFFS) key[1 + n] = word;
        if (n <= HP_MAX_DIFFS) ++n;
    };
    auto cut = [&]() {
        if (run_len) put(hap_diff_word(run_start - rs, (uint32_t)HP_KIND_DEL, run_len));
        run_len = 0;
    };
    regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t len, bool del) {
        const int64_t a64 = r0 > rs ? r0 : rs, b64 = (int64_t)r0 + len < (int64_t)re ? (int64_t)r0 + len : (int64_t)re;
        if (a64 >= b64) return;
        const int32_t a = (int32_t)a64, b = (int32_t)b64;      // the segment inside the region: [a, b)
        if (del) {
            if (a == rs || b == re) edge = true;
            if (run_len && run_start + run_len == a) { run_len += b - a; return; }
            cut();
            run_start = a; run_len = b - a;
            return;
        }
        cut();
        if (edge) return;
        auto sink = [&](int32_t p, uint32_t code) { put(hap_diff_word(p - rs, hap_kind(code), 0)); };
        const uint64_t k0 = q0 + (uint64_t)(a - r0);
        const bool low = FAST ? hap_match16(seq, qual, k0, F, a, b - a, P.min_quality, sink) : hap_match1(seq, qual, k0, F, a, b - a, P.min_quality, sink);
        lowq = lowq || low;
    });
    cut();
    if (edge) return HP_OUT_EDGE;
    if (lowq) return HP_OUT_LOWQ;
    if (n > HP_MAX_DIFFS) return HP_OUT_OVERFLOW;
    if (n == 0) return HP_OUT_REF;
    key[0] = hap_head(region, n);
    for (int k = n; k < HP_MAX_DIFFS; ++k) key[1 + k] = 0u;
    return HP_OUT_KEY;
}

// ---- the table: open addressing, linear probing, a bounded probe count
AMP_ST_HD uint64_t hap_hash(const uint32_t *key) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int w = 0; w < HP_KEY_WORDS; ++w) {
        h = (h ^ (uint64_t)key[w]) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
AMP_ST_HD uint32_t hap_slot_global(uint64_t hash, uint32_t log2_capacity) { return keyed_slot(hash, log2_capacity); }
AMP_ST_HD uint32_t hap_probes_global(uint32_t log2_capacity) { return keyed_probes(log2_capacity); }
AMP_ST_HD bool hap_key_equal(const uint32_t *x, const uint32_t *y) {
    bool same = true;
    for (int w = 0; w < HP_KEY_WORDS; ++w) same = same && x[w] == y[w];
    return same;
}
AMP_ST_HD bool hap_key_less(const uint32_t *x, const uint32_t *y) {
    for (int w = 0; w < HP_KEY_WORDS; ++w)
        if (x[w] != y[w]) return x[w] < y[w];
    return false;
}

// The probe rule.  A key is fourteen words and no compare-and-swap is that wide, so a slot is claimed ONE WORD AT A TIME in
// fixed order: cas(slot, w, value) puts value into word w of the slot when that word is HP_EMPTY and says what it held before.
// An inserter that meets a word that is neither empty nor its own leaves the slot for the next one; an inserter that gets
// through all fourteen has matched every word, whoever wrote which: the slot holds exactly its key.  Words once written never
// change, so a slot ends up with one key, and a key that left a slot leaves it every time.  Nothing here waits for another
// inserter: both loops are bounded by constants.  -> the key's slot (fresh: this call wrote its last word), or -1 when none
// of the slots tried took the key.
template <class Cas>
AMP_ST_HD int64_t hap_probe(const uint32_t *key, uint32_t first, uint32_t mask, uint32_t probes, Cas cas, bool &fresh) {
    fresh = false;
    for (uint32_t k = 0; k < probes; ++k) {
        const uint32_t s = (first + k) & mask;
        bool mine = true;
        uint32_t prev = 0u;
        for (int w = 0; w < HP_KEY_WORDS; ++w) {
            prev = cas(s, w, key[w]);
            if (prev != HP_EMPTY && prev != key[w]) { mine = false; break; }
        }
        if (mine) { fresh = prev == HP_EMPTY; return (int64_t)s; }
    }
    return -1;
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is hap_hook of amp_hap.hip, declared in amp_hook.hpp)
