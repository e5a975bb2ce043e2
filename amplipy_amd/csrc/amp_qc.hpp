// amp_qc.hpp -- the amplicon QC report: what one read adds to the per-read tallies and the per-primer
// read counts, and what one position adds to a region's depth figures, as plain functions.  k_qc_reads / k_qc_regions
// (amp_qc.hip) call them on the device; tests/hostsim/qc_twin.cpp loops the same functions over arrays on the CPU, built
// with plain g++ (no HIP headers: the two attributes are defined away), against the restatement in tests/qc_util.py.
#pragma once

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
#define AMP_QC_HD __host__ __device__ inline

namespace amp {

// Counters a block keeps in LDS for the per-primer histogram (u32, start counts then end counts): primer sets of up to
// QC_LDS_COUNTERS / 2 rows take the LDS path, larger ones add their aggregated runs straight to the global u64 arrays.
constexpr int QC_LDS_COUNTERS = 8192;
constexpr int QC_BLOCK = 256;            // lanes of a k_qc_reads / k_qc_regions block
constexpr int QC_TILES_PER_BLOCK = 4;    // k_qc_reads: a block takes at least this many 256-read tiles before another block is added
constexpr int QC_BLOCKS_PER_CU = 4;      // ... and the grid stops growing here

// The scalar tallies in the order of amp_qc_reads.  The first QC_N_FLAGS are counts of reads (one bit each in QcRead::bits),
// the last two are sums.
enum {
    QC_ROWS = 0, QC_ERRORS, QC_PRIMER_START, QC_PRIMER_END, QC_PRIMER_BOTH, QC_PRIMER_NONE, QC_QUALITY, QC_KEPT, QC_DROPPED_SHORT,
    QC_DROPPED_NO_PRIMER, QC_N_FLAGS, QC_REF_BASES_IN = QC_N_FLAGS, QC_REF_BASES_OUT, QC_N_TALLIES
};
static_assert(sizeof(amp_qc_reads) == QC_N_TALLIES * sizeof(uint64_t), "amp_qc_reads is the tallies in enum order");

struct QcReadParams {
    int32_t ref_len;
    int32_t do_trim;
    int32_t min_length;
    int32_t include_no_primer;
};

struct QcRead {
    uint32_t bits;          // bit k: the read adds one to tally k (k < QC_N_FLAGS)
    uint64_t ref_in;        // reference bases of the original CIGAR
    uint64_t ref_out;       // ... of the trimmed one (ref_len), 0 without trimming
    int64_t orig_end;       // pos + ref_in
    int32_t owner_start;    // primer that takes the read's start trim, -1: none
    int32_t owner_end;      // ... its end trim
};

// Reference length of a CIGAR (BAM words len << 4 | op): ops M D N = X consume the reference.
AMP_QC_HD uint64_t qc_cigar_ref_len(const uint32_t *cig, uint32_t n_ops) {
    uint64_t r = 0;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t v = cig[k], op = v & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) r += v >> 4;
    }
    return r;
}

// One read.  pos / cig / n_ops: the read as it came in; ref_len_out / trim_flags / status: what the read pass made of it
// (read only with do_trim, status always).  The keep rule is A:910; the primer look-ups use the ORIGINAL pos and end, as
// trim_read's own do (A:450-451), and do nothing on a coordinate outside the reference or on a position no primer covers.
AMP_QC_HD QcRead qc_classify(int32_t pos, const uint32_t *cig, uint32_t n_ops, int32_t ref_len_out, uint32_t trim_flags, uint32_t status,
                             const QcReadParams &P, const int32_t *left_owner, const int32_t *right_owner) {
    QcRead r;
    r.bits = 1u << QC_ROWS;
    r.ref_in = 0; r.ref_out = 0; r.orig_end = pos; r.owner_start = -1; r.owner_end = -1;
    if (status != 0u) { r.bits |= 1u << QC_ERRORS; return r; }
    r.ref_in = qc_cigar_ref_len(cig, n_ops);
    r.orig_end = (int64_t)pos + (int64_t)r.ref_in;
    if (!P.do_trim) return r;
    const bool ps = (trim_flags & AMP_TRIM_PRIMER_START) != 0u, pe = (trim_flags & AMP_TRIM_PRIMER_END) != 0u;
    if (ps) r.bits |= 1u << QC_PRIMER_START;
    if (pe) r.bits |= 1u << QC_PRIMER_END;
    if (ps && pe) r.bits |= 1u << QC_PRIMER_BOTH;
    if (!ps && !pe) r.bits |= 1u << QC_PRIMER_NONE;
    if (trim_flags & AMP_TRIM_QUALITY) r.bits |= 1u << QC_QUALITY;
    r.ref_out = (uint64_t)(int64_t)ref_len_out;
    if (ref_len_out < P.min_length) r.bits |= 1u << QC_DROPPED_SHORT;
    else if (!ps && !pe && !P.include_no_primer) r.bits |= 1u << QC_DROPPED_NO_PRIMER;
    else r.bits |= 1u << QC_KEPT;
    if (ps && pos >= 0 && pos < P.ref_len) r.owner_start = left_owner[pos];
    const int64_t last = r.orig_end - 1;
    if (pe && last >= 0 && last < (int64_t)P.ref_len) r.owner_end = right_owner[last];
    return r;
}

// depth of a position: A C G T N and '-' of its row of the count table (the insertion tally is not part of it)
AMP_QC_HD uint32_t qc_depth_of(const uint32_t *row) {
    return row[0] + row[1] + row[2] + row[3] + row[4] + row[5];
}

// A region's figures while positions are added to them, and the merge of two partial figures.
struct QcRegionAcc {
    uint64_t sum;
    uint32_t mn, mx;
    uint32_t covered[AMP_QC_MAX_DEPTHS];
};

AMP_QC_HD QcRegionAcc qc_region_empty() {
    QcRegionAcc a;
    a.sum = 0; a.mn = 0xFFFFFFFFu; a.mx = 0;
    for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) a.covered[k] = 0;
    return a;
}

AMP_QC_HD void qc_region_add(QcRegionAcc &a, uint32_t depth, int32_t n_depths, const uint32_t *depths) {
    a.sum += depth;
    a.mn = depth < a.mn ? depth : a.mn;
    a.mx = depth > a.mx ? depth : a.mx;
    for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) a.covered[k] += (k < n_depths && depth >= depths[k]) ? 1u : 0u;
}

AMP_QC_HD void qc_region_merge(QcRegionAcc &a, const QcRegionAcc &b) {
    a.sum += b.sum;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) a.covered[k] += b.covered[k];
}

// A region clamped to the reference: start and end in [0, ref_len], end = start when nothing is left.
AMP_QC_HD void qc_region_clamp(int32_t ref_len, int32_t &start, int32_t &end) {
    start = start < 0 ? 0 : (start > ref_len ? ref_len : start);
    end = end < 0 ? 0 : (end > ref_len ? ref_len : end);
    if (end < start) end = start;
}

AMP_QC_HD amp_qc_region qc_region_result(int32_t start, int32_t end, const QcRegionAcc &a) {
    amp_qc_region r;
    r.start = start; r.end = end;
    r.depth_sum = a.sum;
    r.depth_min = end > start ? a.mn : 0u;
    r.depth_max = a.mx;
    for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) r.covered[k] = a.covered[k];
    return r;
}

}  // namespace amp
// (the hook amplihip.hip runs behind the read pass is qc_hook of amp_qc.hip, declared in amp_hook.hpp)
