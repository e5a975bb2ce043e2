// amp_call.hpp -- the per-position decision of calling (A:756-771 alleles_from_counts + A:917-952), as one
// function: everything between the loads of k_call (six base counts, the position's insertion-event count, the
// reference byte) and its stores.  __host__ __device__ only so that tests/hostsim can run the same code on the CPU
// against a plain restatement of the reference's loop; the shipped library never executes it on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/amplihip.h"

#ifndef AMP_HD
#define AMP_HD __host__ __device__ __forceinline__
#endif

namespace amp {

// Everything that does not depend on the TEXT of an insertion allele: total depth, the six base symbols ranked
// like sorted(..., reverse=True) (count descending, ties by symbol descending: 'T' > 'N' > 'G' > 'C' > 'A' > '-'),
// consensus symbol, variant record.  ``cnt``: the position's counts in column order A C G T N -; ``ins``: its
// insertion events; ``ref_sym``: where its reference byte is (read only when run_variants: a context without a
// reference may still call the consensus).  ``relevant`` comes back true when an
// insertion string could out-rank the best base symbol or reach the variant frequency threshold; the record then
// carries AMP_CALL_INS_RELEVANT and the host finishes the position from the event list.
AMP_HD amp_pos_call call_position(const uint32_t (&cnt)[6], uint32_t ins, const uint8_t *ref_sym, const amp_call_params &pr, bool &relevant) {
    const int desc[6] = {3, 4, 2, 1, 0, 5};            // T N G C A -
    const char sym_of[6] = {'A', 'C', 'G', 'T', 'N', '-'};
    uint32_t c[6], idx[6];
    uint64_t total = ins;
    for (int k = 0; k < 6; ++k) { idx[k] = desc[k]; c[k] = cnt[desc[k]]; total += c[k]; }
    for (int a = 1; a < 6; ++a) {                      // stable: ties keep the symbol order
        uint32_t cv = c[a], iv = idx[a];
        int b = a - 1;
        while (b >= 0 && c[b] < cv) { c[b + 1] = c[b]; idx[b + 1] = idx[b]; --b; }
        c[b + 1] = cv; idx[b + 1] = iv;
    }
    uint32_t order = 0, nnz = 0;
    for (int k = 0; k < 6; ++k) { order |= idx[k] << (3 * k); nnz += c[k] != 0; }
    amp_pos_call o;
    o.total_depth = (uint32_t)total;
    o.order = order | (nnz << 18);
    o.consensus_sym = -1;
    o.flags = 0; o.alt_mask = 0; o.ref_count = 0;
    const double dtot = (double)total;
    relevant = false;
    if (ins) {
        relevant = pr.full_ranking != 0 || ins >= c[0];
        if (pr.run_variants && (double)ins / dtot >= pr.min_freq_variants) relevant = true;
    }
    if (pr.run_consensus && nnz && (int64_t)c[0] >= (int64_t)pr.min_depth_consensus &&
        (double)c[0] / dtot >= pr.min_freq_consensus) o.consensus_sym = (int8_t)idx[0];       // A:928-929
    if (pr.run_variants) {                                                                     // A:933-951
        const char rs = (char)*ref_sym;
        uint32_t rc = 0; double rf = 0.0; uint32_t n_alt = 0, altm = 0;
        for (int k = 0; k < 6; ++k) {
            if (!c[k]) continue;
            double f = (double)c[k] / dtot;
            if (sym_of[idx[k]] == rs) { rc = c[k]; rf = f; }
            else if (f >= pr.min_freq_variants) { altm |= 1u << k; ++n_alt; }
        }
        o.ref_count = rc; o.alt_mask = (uint8_t)altm;
        if ((int64_t)total >= (int64_t)pr.min_depth_variants && n_alt) o.flags |= AMP_CALL_VARIANT;
        if ((int64_t)rc >= (int64_t)pr.min_depth_variants && rf >= pr.min_freq_variants) o.flags |= AMP_CALL_GT_HAS_REF;
    }
    if (relevant) o.flags |= AMP_CALL_INS_RELEVANT;
    return o;
}

}  // namespace amp
