// plan_history_shim.cpp -- C entry point over amplipy_amd/csrc/amp_plan.hpp for tests/test_read_plan_history.py: the blocks the
// two kernels behind a fast kernel are launched with, from the lists of the engine's previous pass.  Built with g++, nothing of HIP.
#include "../../amplipy_amd/csrc/amp_plan.hpp"

using namespace amp;

// in: n_reads, n_cu, cu_share, prev_list, prev_heavy (negative: no history); 150-base reads with one CIGAR op, default parameters
// out: ok, kv, gen_grid, heavy_grid, gen_blocks, heavy_blocks, total_words
extern "C" void plan_history(const int64_t *in, int64_t *out) {
    PlanIn pi{in[0], in[0], in[0] * 152, 4, 20, 0, (int)in[1], (int)in[2], true, true, true};
    pi.prev_list = in[3];
    pi.prev_heavy = in[4];
    ReadPlan p;
    out[0] = plan_reads(pi, p) ? 1 : 0;
    if (!out[0]) return;
    out[1] = p.kv; out[2] = p.gen_grid; out[3] = p.heavy_grid; out[4] = p.gen_blocks; out[5] = p.heavy_blocks; out[6] = (int64_t)p.total_words;
}
