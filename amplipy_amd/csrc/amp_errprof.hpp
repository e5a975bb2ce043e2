// amp_errprof.hpp -- the error profile: how often a base differs from the reference, by sequencing
// cycle, by reported quality and by substitution class.  What one read and one base add is written here as plain functions:
// k_errprof (amp_errprof.hip) calls them on the device; tests/hostsim/errprof_twin.cpp loops the same functions over arrays on
// the CPU, built with plain g++, against the restatement in tests/errprof_util.py.
//
// A read takes part when it has status 0 and its counted alignment (the trimmed one with do_trim) is REGULAR -- regular_scan's
// rule (amp_strand.hpp), so QUAL '*', pos < 0, irregular CIGARs and anything outside the reference are out.  Every base of every
// match op (M = X) of such a read -- query index q, reference position r, whatever its quality -- with
//   b  the read base, one of A C G T (BAM codes 1 2 4 8; anything else takes no part),
//   x  the reference letter at r, upper-cased, one of A C G T and r not masked (else the base takes no part),
//   m  FLAG & 0x80 (mate; unpaired reads are mate 0),   s  FLAG & 0x10 (strand),
//   c  min(s ? l_seq - 1 - q : q, EP_CYCLES - 1): the cycle counted from the 5' end of the stored SEQ (hard clips do not count),
//   v  min(qual[q], EP_QUALS - 1),   e  b != x,   g  qual[q] >= min_quality
// adds 1 to three uint64 cells: cyc[m][c][e], qualt[m][v][e], sub[m][s][g][x][b].  reads[0] += 1 per regular read with status
// 0, reads[1] += 1 per other read with status 0 (which adds nothing to the tables); a read with a status touches nothing.
//
// Invariants (exact): for each m, the sums of cyc[m], qualt[m] and sub[m] are equal.  With no mask, on a batch whose status-0
// reads are all regular, for every reference letter X and base b: the sum over m, s of sub[m][s][1][X][b] equals the sum of
// counts[p][b] of the count table over the positions p with upper(ref[p]) == X -- the counted set of a regular read is exactly
// its match bases at or above min_quality (amp_strand.hpp).
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

namespace amp {

constexpr int EP_CYCLES = 512;           // cycles of cyc; the last bin is open-ended
constexpr int EP_QUALS = 94;             // qualities of qualt; the last bin is open-ended (Phred+33 in printable ASCII ends at 93)
constexpr int EP_CYC_CELLS = 2 * EP_CYCLES * 2;          // cyc[m][c][e]
constexpr int EP_QUAL_CELLS = 2 * EP_QUALS * 2;          // qualt[m][v][e]
constexpr int EP_SUB_CELLS = 2 * 2 * 2 * 4 * 4;          // sub[m][s][g][x][b]
constexpr int EP_QUAL_AT = EP_CYC_CELLS, EP_SUB_AT = EP_QUAL_AT + EP_QUAL_CELLS;
constexpr int EP_CELLS = EP_SUB_AT + EP_SUB_CELLS;       // the three tables as one array, in this order
constexpr uint8_t EP_NO_CODE = 0xFFu;    // a reference position that takes no part

constexpr int EP_BLOCK = 256;            // lanes of a k_errprof block = reads of a tile
constexpr int EP_SLOTS = 4;              // match-segment slots per read on the tile's list; a read that needs more walks serially
constexpr int EP_TILES_PER_BLOCK = 4;    // a block takes at least this many tiles before another block is added
constexpr int EP_BLOCKS_PER_CU = 4;      // ... and the grid stops growing here
// One base adds 1 to one cell of each table, so a block cell takes at most the bases of the tiles since its flush.  A read
// adds to the block's u32 cells only up to EP_LDS_LSEQ bases (a longer one walks serially into the u64 tables), a tile has
// EP_BLOCK reads:
constexpr int32_t EP_LDS_LSEQ = 65535;
constexpr int EP_MAX_TILES_PER_FLUSH = 256;
static_assert((uint64_t)EP_MAX_TILES_PER_FLUSH * EP_BLOCK * (uint64_t)EP_LDS_LSEQ < (1ull << 32), "a block cell cannot overflow before its flush");
static_assert(EP_CYCLES % 64 == 0, "the two e halves of a mate's cycles start on the same bank: lanes on consecutive cycles hit 64 different banks");

// ---- the cells as the ABI lays them out (each table on its own)
AMP_ST_HD int ep_cyc_cell(uint32_t m, uint32_t c, uint32_t e) { return (int)((m * EP_CYCLES + c) * 2u + e); }
AMP_ST_HD int ep_qual_cell(uint32_t m, uint32_t v, uint32_t e) { return (int)((m * EP_QUALS + v) * 2u + e); }
AMP_ST_HD int ep_sub_cell(uint32_t m, uint32_t s, uint32_t g, uint32_t x, uint32_t b) { return (int)(((((m * 2u + s) * 2u + g) * 4u) + x) * 4u + b); }

// ---- the cells as a block keeps them: one array of EP_CELLS words, qualt and sub as above behind cyc, cyc itself as
// [m][e][c] -- the 64 lanes of a wave hold 64 consecutive cycles of one mate, and with c innermost they hit 64 different banks
// whatever their e.  ep_block_to_global: the index of block cell k in the three tables laid end to end in the ABI's order.
AMP_ST_HD int ep_block_cyc(uint32_t m, uint32_t c, uint32_t e) { return (int)((m * 2u + e) * EP_CYCLES + c); }
AMP_ST_HD int ep_block_to_global(int k) {
    if (k >= EP_CYC_CELLS) return k;
    const uint32_t c = (uint32_t)k % EP_CYCLES, e = ((uint32_t)k / EP_CYCLES) & 1u, m = (uint32_t)k / (2 * EP_CYCLES);
    return ep_cyc_cell(m, c, e);
}

// ---- the reference as the kernel reads it: 0..3 for A C G T (either case), EP_NO_CODE for every other letter and for a masked
// position (mask_bits: bit p & 31 of word p >> 5; null: none) -- the mask costs the kernel nothing.
AMP_ST_HD uint8_t ep_ref_code(uint8_t ascii) {
    const uint8_t u = (uint8_t)(ascii & 0xDFu);          // upper case for letters
    const bool letter = (ascii >= 'A' && ascii <= 'Z') || (ascii >= 'a' && ascii <= 'z');
    if (!letter) return EP_NO_CODE;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : EP_NO_CODE;
}
inline void errprof_ref_codes(const uint8_t *ref_ascii, const uint32_t *mask_bits, int32_t ref_len, uint8_t *code) {
    for (int32_t p = 0; p < ref_len; ++p) {
        const bool masked = mask_bits && ((mask_bits[p >> 5] >> (p & 31)) & 1u);
        code[p] = masked ? EP_NO_CODE : ep_ref_code(ref_ascii[p]);
    }
}

// ---- one base: whether it takes part, and its three block cells.  bam_code: the read's 4-bit base; x: the reference code at
// its position; qv: its quality byte; m, s: mate and strand of its read; c: its cycle before the clamp (>= 0).
AMP_ST_HD bool errprof_base(uint32_t bam_code, uint32_t x, uint32_t qv, uint32_t m, uint32_t s, int32_t c, int32_t min_quality, int &kc, int &kq, int &ks) {
    const uint32_t b = st_code_to_col(bam_code);
    if (b > 3u || x > 3u) return false;
    const uint32_t e = b != x ? 1u : 0u, g = (int32_t)qv >= min_quality ? 1u : 0u;
    const uint32_t cc = c < EP_CYCLES - 1 ? (uint32_t)c : (uint32_t)(EP_CYCLES - 1);
    const uint32_t v = qv < (uint32_t)(EP_QUALS - 1) ? qv : (uint32_t)(EP_QUALS - 1);
    kc = ep_block_cyc(m, cc, e);
    kq = EP_QUAL_AT + ep_qual_cell(m, v, e);
    ks = EP_SUB_AT + ep_sub_cell(m, s, g, x, b);
    return true;
}

// ---- a match segment of a regular read: base j of it has the query byte q0 + j (index in qual / seq), the reference position
// r0 + j and the cycle c0 + j on a forward read, c0 - j on a reverse one.  kind = mate << 1 | reverse strand.
struct EpSeg {
    uint64_t q0;
    int32_t r0;
    uint32_t len;
    int32_t c0;
    uint32_t kind;
};
AMP_ST_HD uint32_t ep_seg_mate(const EpSeg &g) { return (g.kind >> 1) & 1u; }
AMP_ST_HD uint32_t ep_seg_rev(const EpSeg &g) { return g.kind & 1u; }
AMP_ST_HD int32_t ep_seg_cycle(const EpSeg &g, uint32_t j) { return ep_seg_rev(g) ? g.c0 - (int32_t)j : g.c0 + (int32_t)j; }

// The match segments of a read, to put(seg), in CIGAR order; n_seg counts them alone.  They may be used when the shape says
// regular (regular_scan decides, nothing here).
template <class Put>
AMP_ST_HD StrandShape errprof_segments(const StrandRead &R, const StrandParams &P, uint32_t qual0, uint32_t mate, Put put) {
    int32_t n = 0;
    StrandShape sh = regular_scan(R, P, qual0, [&](int32_t r0, uint64_t q0, uint32_t len, bool del) {
        if (del) return;
        const int32_t q = (int32_t)(q0 - R.base);
        put(EpSeg{q0, r0, len, R.rev ? R.lseq - 1 - q : q, (mate << 1) | (R.rev ? 1u : 0u)});
        ++n;
    });
    sh.n_seg = n;
    return sh;
}

// A regular read puts its segments on the tile's list when they fit its slots and it is short enough for the block's u32 cells;
// every other regular read walks serially (errprof_seg_walk per segment) -- into the block's cells when ep_read_in_block, else
// straight into the u64 tables.
AMP_ST_HD bool ep_read_in_block(int32_t lseq) { return lseq <= EP_LDS_LSEQ; }
AMP_ST_HD bool ep_read_listed(const StrandShape &sh, int32_t lseq) { return sh.regular && sh.n_seg <= EP_SLOTS && ep_read_in_block(lseq); }

// One segment base by base: sink(kc, kq, ks) per base that takes part.  code: the reference codes.
template <class Sink>
AMP_ST_HD void errprof_seg_walk(const EpSeg &g, const uint8_t *seq, const uint8_t *qual, const uint8_t *code, int32_t min_quality, Sink sink) {
    for (uint32_t j = 0; j < g.len; ++j) {
        int kc, kq, ks;
        const uint64_t k = g.q0 + j;
        if (errprof_base(st_base_code(seq, k), code[(int64_t)g.r0 + j], qual[k], ep_seg_mate(g), ep_seg_rev(g), ep_seg_cycle(g, j), min_quality, kc, kq, ks))
            sink(kc, kq, ks);
    }
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is errprof_hook of amp_errprof.hip, declared in amp_hook.hpp)
