// qc_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_qc.hpp that k_qc_reads, k_qc_depth and k_qc_regions
// call per read and per position, looped over arrays on the CPU.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libqc_twin.so qc_twin.cpp          (tests/test_qc_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DQC_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o qc_twin qc_twin.cpp && ./qc_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches and tables in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "amp_qc.hpp"

using namespace amp;

extern "C" {

// k_qc_reads without the reductions: every tally summed read after read
int twin_read_tallies(int64_t n, const int32_t *pos, const uint32_t *cig_off, const uint32_t *cig, const int32_t *ref_len_out,
                      const uint8_t *trim_flags, const uint8_t *status, int32_t ref_len, int32_t do_trim, int32_t min_length,
                      int32_t include_no_primer, const int32_t *left_owner, const int32_t *right_owner, int32_t n_primers,
                      uint64_t *tallies, uint64_t *reads_start, uint64_t *reads_end) {
    const QcReadParams P{ref_len, do_trim, min_length, include_no_primer};
    for (int k = 0; k < QC_N_TALLIES; ++k) tallies[k] = 0;
    for (int32_t k = 0; k < n_primers; ++k) reads_start[k] = reads_end[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const QcRead r = qc_classify(pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], do_trim ? ref_len_out[i] : 0,
                                     do_trim ? trim_flags[i] : 0u, status ? status[i] : 0u, P, left_owner, right_owner);
        for (int k = 0; k < QC_N_FLAGS; ++k) tallies[k] += (r.bits >> k) & 1u;
        tallies[QC_REF_BASES_IN] += r.ref_in;
        tallies[QC_REF_BASES_OUT] += r.ref_out;
        if (r.owner_start >= n_primers || r.owner_end >= n_primers) return -1;
        if (r.owner_start >= 0) ++reads_start[r.owner_start];
        if (r.owner_end >= 0) ++reads_end[r.owner_end];
    }
    return 0;
}

void twin_depth(const uint32_t *counts, int32_t ref_len, uint32_t *depth) {
    for (int32_t p = 0; p < ref_len; ++p) depth[p] = qc_depth_of(counts + (size_t)p * AMP_NSYM);
}

// k_qc_regions with its lanes run one after the other: QC_BLOCK partial figures per region, lanes striding it, merged in
// the kernel's order (64 lanes of a wave by halving distances, then the waves)
void twin_regions(const uint32_t *depth, int32_t ref_len, int32_t n_regions, const int32_t *rstart, const int32_t *rend, int32_t n_depths,
                  const uint32_t *depths, amp_qc_region *out) {
    for (int32_t r = 0; r < n_regions; ++r) {
        int32_t s = rstart[r], e = rend[r];
        qc_region_clamp(ref_len, s, e);
        QcRegionAcc lane[QC_BLOCK];
        for (int t = 0; t < QC_BLOCK; ++t) {
            lane[t] = qc_region_empty();
            for (int64_t p = (int64_t)s + t; p < e; p += QC_BLOCK) qc_region_add(lane[t], depth[p], n_depths, depths);
        }
        for (int w = 0; w < QC_BLOCK / 64; ++w)
            for (int d = 32; d >= 1; d >>= 1)
                for (int l = 0; l < d; ++l) qc_region_merge(lane[w * 64 + l], lane[w * 64 + l + d]);
        for (int w = 1; w < QC_BLOCK / 64; ++w) qc_region_merge(lane[0], lane[w * 64]);
        out[r] = qc_region_result(s, e, lane[0]);
    }
}

}  // extern "C"

#ifdef QC_TWIN_MAIN
#define TWIN_NAME "qc_twin"
#include "twin_main.hpp"

int main() {
    for (int round = 0; round < 200; ++round) {
        const int32_t G = 1 + (int32_t)rnd(round % 4 == 0 ? 3 : 900);
        const int32_t np = (int32_t)rnd(12);
        // owners as any table may hold them: -1 or a primer
        int32_t *lo = (int32_t *)malloc((size_t)G * 4), *ro = (int32_t *)malloc((size_t)G * 4);
        for (int32_t p = 0; p < G; ++p) { lo[p] = np ? (int32_t)rnd((uint32_t)np + 1) - 1 : -1; ro[p] = np ? (int32_t)rnd((uint32_t)np + 1) - 1 : -1; }
        const int64_t n = rnd(300);
        std::vector<uint32_t> off((size_t)n + 1, 0), words;
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t ops = rnd(8) == 0 ? 40 + rnd(30) : rnd(4);       // (also reads without an op)
            for (uint32_t k = 0; k < ops; ++k) words.push_back((rnd(200) << 4) | rnd(10));
            off[(size_t)i + 1] = (uint32_t)words.size();
        }
        int32_t *pos = (int32_t *)malloc((size_t)(n ? n : 1) * 4), *rl = (int32_t *)malloc((size_t)(n ? n : 1) * 4);
        uint8_t *tf = (uint8_t *)malloc((size_t)(n ? n : 1)), *st = (uint8_t *)malloc((size_t)(n ? n : 1));
        uint32_t *cig = (uint32_t *)malloc((words.size() ? words.size() : 1) * 4), *coff = (uint32_t *)malloc(((size_t)n + 1) * 4);
        for (size_t k = 0; k < words.size(); ++k) cig[k] = words[k];
        for (int64_t i = 0; i <= n; ++i) coff[i] = off[(size_t)i];
        for (int64_t i = 0; i < n; ++i) {
            pos[i] = (int32_t)rnd((uint32_t)G + 40) - 20;                    // in front of, inside and behind the reference
            if (rnd(50) == 0) pos[i] = rnd(2) ? 0x7FFFFFFF : -0x7FFFFFFF - 1;
            rl[i] = (int32_t)rnd(300); tf[i] = (uint8_t)rnd(8); st[i] = rnd(20) == 0 ? (uint8_t)(1 + rnd(9)) : 0;
        }
        uint64_t t[QC_N_TALLIES];
        uint64_t *ps = (uint64_t *)malloc((size_t)(np ? np : 1) * 8), *pe = (uint64_t *)malloc((size_t)(np ? np : 1) * 8);
        for (int do_trim = 0; do_trim < 2; ++do_trim) {
            CHECK(twin_read_tallies(n, pos, coff, cig, rl, tf, st, G, do_trim, (int32_t)rnd(200), (int32_t)rnd(2), lo, ro, np, t, ps, pe) == 0);
            CHECK(t[QC_ROWS] == (uint64_t)n);
            uint64_t s_sum = 0, e_sum = 0;
            for (int32_t k = 0; k < np; ++k) { s_sum += ps[k]; e_sum += pe[k]; }
            if (do_trim) {
                CHECK(t[QC_KEPT] + t[QC_DROPPED_SHORT] + t[QC_DROPPED_NO_PRIMER] == t[QC_ROWS] - t[QC_ERRORS]);
                CHECK(t[QC_PRIMER_NONE] + t[QC_PRIMER_START] + t[QC_PRIMER_END] - t[QC_PRIMER_BOTH] == t[QC_ROWS] - t[QC_ERRORS]);
                CHECK(s_sum <= t[QC_PRIMER_START] && e_sum <= t[QC_PRIMER_END]);
            } else {
                for (int k = QC_PRIMER_START; k < QC_N_FLAGS; ++k) CHECK(t[k] == 0);
                CHECK(t[QC_REF_BASES_OUT] == 0 && s_sum == 0 && e_sum == 0);
            }
        }
        // depth and regions: the whole reference against two halves of it
        uint32_t *counts = (uint32_t *)malloc((size_t)G * AMP_NSYM * 4), *depth = (uint32_t *)malloc((size_t)G * 4);
        for (size_t k = 0; k < (size_t)G * AMP_NSYM; ++k) counts[k] = rnd(4) == 0 ? 0u : rnd(round % 7 == 0 ? 600000000u : 300u);
        twin_depth(counts, G, depth);
        const int32_t cut = (int32_t)rnd((uint32_t)G + 1);
        const int32_t rs[5] = {0, 0, cut, -7, G + 3}, re[5] = {G, cut, G, G + 9, G + 8};
        const int32_t nd = (int32_t)rnd(AMP_QC_MAX_DEPTHS + 1);
        uint32_t *dp = (uint32_t *)malloc((size_t)(nd ? nd : 1) * 4);
        for (int32_t k = 0; k < nd; ++k) dp[k] = rnd(3) == 0 ? 0xFFFFFFFFu : rnd(400);
        amp_qc_region *reg = (amp_qc_region *)malloc(5 * sizeof(amp_qc_region));
        twin_regions(depth, G, 5, rs, re, nd, dp, reg);
        CHECK(reg[0].depth_sum == reg[1].depth_sum + reg[2].depth_sum);
        CHECK(reg[3].start == 0 && reg[3].end == G && reg[3].depth_sum == reg[0].depth_sum && reg[3].depth_min == reg[0].depth_min);
        CHECK(reg[4].start == G && reg[4].end == G && reg[4].depth_sum == 0 && reg[4].depth_min == 0 && reg[4].depth_max == 0);
        for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) {
            CHECK(reg[0].covered[k] == reg[1].covered[k] + reg[2].covered[k]);
            CHECK(k < nd || reg[0].covered[k] == 0);
            CHECK(reg[0].covered[k] <= (uint32_t)G);
        }
        free(lo); free(ro); free(pos); free(rl); free(tf); free(st); free(cig); free(coff); free(ps); free(pe);
        free(counts); free(depth); free(dp); free(reg);
    }
    printf("qc_twin ok\n");
    return 0;
}
#endif
