// amp_clip.hpp -- soft-clip sites of the QC report: what ONE read adds to the clip table, as plain
// functions.  A large deletion leaves no gap in an alignment: the aligner aligns one side and soft-clips the rest, so the only
// trace of the event is a pile of reads that all stop at one reference position, and whose clipped bases match the reference
// somewhere else.  k_qc_clips (amp_qc.hip) tallies per reference position and side how many reads are clipped there and what
// their first CL_K clipped bases are; the host (amplipy_amd/clips.py) builds a consensus per site and places it.  k_qc_clips
// calls these functions on the device; tests/hostsim/clip_twin.cpp loops them over arrays on the CPU, built with plain g++,
// against the restatement in tests/clip_util.py.
//
// A read is its ORIGINAL pos, CIGAR, l_seq, FLAG and SEQ, never the trimmed alignment.  There is no quality test.
#pragma once

#include <stdint.h>

#include "amp_qc.hpp"

namespace amp {

constexpr int CL_K = 16;                     // clipped bases kept per site, nearest the junction first
constexpr int CL_COLS = 5;                   // A C G T other
constexpr int CL_CELLS = 2 + CL_K * CL_COLS; // u32 cells per (position, side): reads, rev, comp[j][c]
constexpr int CL_LEFT = 0, CL_RIGHT = 1;     // the clip lies in front of / behind the aligned bases
constexpr int CL_MIN_MAX = 64;               // the largest clip_min
enum { CL_SCANNED = 0, CL_SKIPPED, CL_N_LEFT, CL_N_RIGHT, CL_N_SCALARS };      // the u64 scalars behind the table
constexpr uint32_t CL_NO_COL = 7u;           // a field of clip_cols without a base
static_assert(CL_K == AMP_CLIP_K && CL_COLS == AMP_CLIP_COLS && CL_CELLS == AMP_CLIP_CELLS && CL_N_SCALARS == AMP_CLIP_SCALARS, "the sizes the ABI names");
static_assert(CL_CELLS == 82 && CL_K * 3 <= 64, "a site's columns travel as 3-bit fields of one 64-bit word");

// u32 words of the table of a reference of ref_len bases -- [(ref_len + 1)][2][CL_CELLS], position-major: a RIGHT site may
// lie at ref_len -- and the first word of a site
AMP_QC_HD size_t clip_table_words(int32_t ref_len) { return ((size_t)ref_len + 1) * 2 * CL_CELLS; }
AMP_QC_HD size_t clip_site_word(int32_t p, int side) { return ((size_t)p * 2 + (size_t)side) * CL_CELLS; }

struct ClipRead {
    int32_t skipped;        // the read adds to `skipped` and to nothing else
    int32_t L[2];           // clipped bases in front and behind (S ops summed; H ops skipped)
    int32_t p[2];           // the site of either side, -1: none (the clip is shorter than clip_min)
};

// The clips of one read.  The CIGAR is walked from the front -- leading H ops skipped, S ops summed, up to the first other op --
// and from the back down to element 1 (element 0 is never examined from the back, as in insev_query_span).
AMP_QC_HD ClipRead clip_scan(int32_t pos, const uint32_t *cig, uint32_t n_ops, int32_t lseq, int32_t ref_len, int32_t clip_min) {
    ClipRead r;
    r.skipped = 1; r.L[0] = r.L[1] = 0; r.p[0] = r.p[1] = -1;
    int64_t left = 0, right = 0;
    uint32_t k = 0;
    for (; k < n_ops; ++k) {
        const uint32_t v = cig[k], op = v & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        left += v >> 4;
    }
    if (k == n_ops || lseq <= 0 || pos < 0) return r;       // (no op other than H / S; SEQ '*'; in front of the reference)
    for (int64_t b = (int64_t)n_ops - 1; b >= 1; --b) {
        const uint32_t v = cig[b], op = v & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        right += v >> 4;
    }
    const uint64_t ref = qc_cigar_ref_len(cig, n_ops);
    if (left + right > (int64_t)lseq || (uint64_t)pos + ref > (uint64_t)ref_len) return r;
    r.skipped = 0;
    r.L[CL_LEFT] = (int32_t)left; r.L[CL_RIGHT] = (int32_t)right;
    if (left >= clip_min) r.p[CL_LEFT] = pos;
    if (right >= clip_min) r.p[CL_RIGHT] = pos + (int32_t)ref;
    return r;
}

// Column of a BAM base code: A C G T are 1 2 4 8, anything else ('=', N, the IUPAC codes) is `other`
AMP_QC_HD uint32_t clip_col(uint32_t code) { return code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : 4u; }

// Query base q of the read whose bases start at `base` (a multiple of 8): nibbles, high first
AMP_QC_HD uint32_t clip_code(const uint8_t *seq, uint64_t base, int32_t q) {
    const uint64_t at = base + (uint64_t)q;
    const uint32_t b = seq[at >> 1];
    return (at & 1u) ? (b & 15u) : (b >> 4);
}

// The columns of a site's clipped bases as CL_K fields of 3 bits, offset j in bits [3j, 3j + 3); CL_NO_COL from min(L, CL_K) on.
// LEFT: offset j is query base L_left - 1 - j; RIGHT: query base lseq - L_right + j.  (clip_scan saw to L_left + L_right <= lseq.)
AMP_QC_HD uint64_t clip_cols(const uint8_t *seq, uint64_t base, int32_t lseq, int side, int32_t L) {
    uint64_t w = 0;
    const int32_t m = L < CL_K ? L : CL_K;
    for (int j = 0; j < CL_K; ++j) {
        uint32_t f = CL_NO_COL;
        if (j < m) f = clip_col(clip_code(seq, base, side == CL_LEFT ? L - 1 - j : lseq - L + j));
        w |= (uint64_t)f << (3 * j);
    }
    return w;
}
AMP_QC_HD uint32_t clip_field(uint64_t cols, int j) { return (uint32_t)(cols >> (3 * j)) & 7u; }

}  // namespace amp
