// plan_shim.cpp -- C entry points over amplipy_amd/csrc/amp_plan.hpp for tests/test_read_plan.py.  Built with g++ and nothing
// of HIP: that it compiles is the proof that the plan header is plain C++.  Built twice: as shipped and with -DAMP_DEV.
#include "../../amplipy_amd/csrc/amp_plan.hpp"

using namespace amp;

enum { IN_COLS = 11, HEAD_COLS = 17, N_REGIONS = 15, OUT_COLS = HEAD_COLS + 2 * N_REGIONS };

extern "C" int plan_in_cols(void) { return IN_COLS; }
extern "C" int plan_out_cols(void) { return OUT_COLS; }
#ifdef AMP_DEV
extern "C" int plan_dev(void) { return 1; }
#else
extern "C" int plan_dev(void) { return 0; }
#endif

// F_WAVES, F6_WAVES, F7_WAVES, F_EVGRAN, L_WAVES, L_EVCAP, GL_MAXSEG, DEFER_INDEX_MASK, TILE, T_WAVES
extern "C" void plan_constants(int64_t *out) {
    const int64_t v[] = {F_WAVES, F6_WAVES, F7_WAVES, F_EVGRAN, L_WAVES, L_EVCAP, GL_MAXSEG, DEFER_INDEX_MASK, TILE, T_WAVES};
    for (size_t k = 0; k < sizeof(v) / sizeof(v[0]); ++k) out[k] = v[k];
}

// in[r]: n_reads, n_cig, n_bases_padded, window, min_quality, requested_variant, n_cu, cu_share, caller gives new_pos, new_ncig, new_cig
// out[r]: ok, kv, variant, f5.waves, f5.qrun, fg.grid, fg.rpb, fast_waves, tg.grid, tg.tpb, gen_grid, heavy_grid, long_kernel, direct,
//         ev_fixed, total_words, fast_path_active, then (off, words) of the regions in the order of ReadPlan
extern "C" void plan_rows(long rows, const int64_t *in, int64_t *out) {
    for (long r = 0; r < rows; ++r) {
        const int64_t *a = in + (size_t)r * IN_COLS;
        int64_t *o = out + (size_t)r * OUT_COLS;
        const PlanIn pi{a[0], a[1], a[2], (int32_t)a[3], (int32_t)a[4], (int)a[5], (int)a[6], (int)a[7], a[8] != 0, a[9] != 0, a[10] != 0};
        ReadPlan p;
        for (int k = 0; k < OUT_COLS; ++k) o[k] = -1;
        o[16] = fast_path_active(pi.requested_variant, pi.window, pi.min_quality) ? 1 : 0;
        o[0] = plan_reads(pi, p) ? 1 : 0;
        if (!o[0]) continue;
        const int64_t head[] = {p.kv, p.variant, p.f5.waves, p.f5.qrun, p.fg.grid, p.fg.rpb, p.fast_waves, p.tg.grid, p.tg.tpb, p.gen_grid,
                                p.heavy_grid, p.long_kernel, p.direct, p.ev_fixed, (int64_t)p.total_words};
        for (int k = 0; k < 15; ++k) o[1 + k] = head[k];
        const Region *const reg[N_REGIONS] = {&p.pingpong, &p.dlist, &p.dcnt, &p.split, &p.new_pos, &p.new_ncig, &p.new_cig, &p.glist, &p.gcnt,
                                              &p.gdense, &p.geo, &p.segfirst, &p.llist, &p.lpos, &p.clist};
        for (int k = 0; k < N_REGIONS; ++k) { o[HEAD_COLS + 2 * k] = (int64_t)reg[k]->off; o[HEAD_COLS + 2 * k + 1] = (int64_t)reg[k]->words; }
    }
}
