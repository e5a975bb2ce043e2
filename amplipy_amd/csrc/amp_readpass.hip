// amp_readpass.hip -- the read pass of libamplihip.so: every kernel that trims and counts reads, and launch_reads, which plans a
// batch (amp_plan.hpp) and launches them on the ctx stream.  A unit of its own beside amplihip.hip (the C ABI): these kernels
// are most of the library's compile time, and the host code that changes most often is not here.
//
// k_coordinate_helpers lives here too: it instantiates the same amp_read.hpp templates as the read kernels.
#include <hip/hip_runtime.h>

#include <stdio.h>

#include <algorithm>

#include "../../include/amplihip.h"
#include "amp_ctx.hpp"
#include "amp_plan.hpp"
#include "amp_read.hpp"
#include "amp_tile.hpp"
#include "amp_fast.hpp"
#include "amp_fast5.hpp"
#include "amp_fast6.hpp"
#include "amp_fast7.hpp"
#include "amp_wave.hpp"
#include "amp_heavy.hpp"

using namespace amp;

// Launches the read kernels for a device-resident batch on the ctx stream: plan (amp_plan.hpp: which kernels, their grids,
// the scratch layout), reserve events, size the scratch buffer, turn the plan's offsets into pointers, launch.
int amp::launch_reads(amp_ctx *c, const amp_dev_reads *rd, uint64_t read_base, const amp_trim_out *o) {
    if (c->do_trim && !c->have_primers) return AMP_ESTATE;
    const int64_t n = rd->n_reads;
    c->timed = false;
    c->call_pending = false;       // (calls begun earlier are for the table as it was)
    if (n == 0) return AMP_OK;
    DevOut out{o ? o->new_pos : nullptr, o ? o->new_ncig : nullptr, o ? o->new_cig : nullptr, o ? o->ref_len : nullptr,
               o ? o->trim_flags : nullptr, o ? o->status : nullptr};
    ReadPlan pl;
    PlanIn pin{n, rd->n_cig, rd->n_bases_padded, c->window, c->min_quality, c->kernel_variant, c->n_cu, c->cu_share,
               out.new_pos != nullptr, out.new_ncig != nullptr, out.new_cig != nullptr};
    {   // The lists of the engine's last FINISHED pass (amp_ctx::h_hist): both words of one pass, and of one behind the last setter
        // and behind the last pass of another variant.  The words are read as they stand, without waiting for the pass before: a
        // caller that launches the next pass before that one has finished gets the history of the pass before it, or none -- so
        // the two grids, and with them traces and timings, depend on when the host arrives here.  The results do not.
        const unsigned long long w0 = __atomic_load_n(&c->h_hist[0], __ATOMIC_RELAXED), w1 = __atomic_load_n(&c->h_hist[1], __ATOMIC_RELAXED);
        const uint32_t e = (uint32_t)(w0 >> 32);
        if (e == (uint32_t)(w1 >> 32) && (int32_t)(e - c->hist_from) >= 0 && (int32_t)(c->epoch - e) >= 0) {
            pin.prev_heavy = (int64_t)(uint32_t)w0; pin.prev_list = (int64_t)(uint32_t)w1;
        }
    }
    if (!plan_reads(pin, pl)) {
        snprintf(c->err, sizeof(c->err), "a batch holds at most %u reads", DEFER_INDEX_MASK); return AMP_EINVAL;
    }
    if (c->force_gen_blocks > 0) pl.gen_blocks = std::min<int64_t>(c->force_gen_blocks, pl.gen_grid);
    if (c->force_heavy_blocks > 0) pl.heavy_blocks = std::min<int64_t>(c->force_heavy_blocks, pl.heavy_grid);
    const int kv = pl.kv, variant = pl.variant;
    const TileGrid &tg = pl.tg;
    const FastGrid &fg = pl.fg;
    // event capacity
    if (c->do_count && !c->ev_reserved) {
        unsigned long long h[CTR_WORDS];
        HIPCHK(c, hipMemsetAsync(&c->d_ctr[CTR_EVENT_BOUND], 0, sizeof(unsigned long long), c->stream));
        k_event_bound<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(n, rd->cig_off32, rd->cig, c->d_ctr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h, c->d_ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        unsigned long long mx = 0;
        for (int s = 0; s < EV_SHARDS; ++s) mx = std::max(mx, h[CTR_EV_SHARD0 + s]);
        // what the fullest shard holds + twice the batch's bound + the granules its waves leave open (ReadPlan::ev_fixed)
        const int64_t need = (int64_t)(mx + 2 * h[CTR_EVENT_BOUND]) + pl.ev_fixed;
        if (need > c->ev_cap) HIPCHK(c, grow_events(c, std::max<int64_t>(need, c->ev_cap + c->ev_cap / 2)));
    }
    KParams P{c->min_quality, c->window, c->do_trim, c->do_count, c->ref_len, c->max_primer_len, c->d_min_start, c->d_max_end, ++c->epoch};
    HIPCHK(c, c->scratch.ensure(pl.total_words * 4));
    uint32_t *const scr = c->scratch.as<uint32_t>();
    const auto at = [scr](const Region &r) { return scr + r.off; };
    uint32_t *const dlist = at(pl.dlist), *const dcnt = at(pl.dcnt);
    c->dbg_dcnt = dcnt; c->dbg_grid = (int)tg.grid;
#ifdef AMP_DEV
    if (c->phases & 0x100u) HIPCHK(c, hipMemsetAsync(dcnt, 0, ((size_t)tg.grid * 5 + 64) * 4, c->stream));
#endif
    if (!out.new_pos) out.new_pos = (int32_t *)at(pl.new_pos);
    if (!out.new_ncig) out.new_ncig = at(pl.new_ncig);
    if (!out.new_cig) out.new_cig = at(pl.new_cig);
    const EventBuf eb{c->events.as<amp_ins_event>(), c->d_ctr, c->d_ins_at, (long long)c->ev_cap};
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (variant == 1) {
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        k_reads_lane<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(P, *rd, read_base, out, at(pl.pingpong), c->d_counts, eb);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev2, c->stream));
    } else if (variant == 4) {
        // fast pass over the simple reads, then the general tile kernel over the list of the others
        const SplitDesc none{nullptr, nullptr, nullptr, nullptr};
        uint32_t *const glist = at(pl.glist), *const gcnt = at(pl.gcnt), *const gdense = at(pl.gdense), *const clist = at(pl.clist);
        uint32_t *const segfirst = at(pl.segfirst), *const llist = at(pl.llist), *const lpos = at(pl.lpos);
        GenGeo *const geo = (GenGeo *)at(pl.geo);
        const bool long_kernel = pl.long_kernel, direct = pl.direct;
        if (c->split_timing) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        if ((kv == 7 ? fast7_launch(P, *rd, read_base, out, c->d_counts, eb, glist, gcnt, clist, fg, c->stream)
             : kv == 6 ? fast6_launch(P, *rd, read_base, out, c->d_counts, eb, glist, gcnt, clist, fg, c->stream)
             : kv == 5 ? fast5_launch(P, *rd, read_base, out, c->d_counts, eb, glist, gcnt, fg, pl.f5, c->stream)
                     : fast_launch(P, *rd, read_base, out, c->d_counts, eb, glist, gcnt, fg, c->stream, dcnt + tg.grid + 64)) != 0) {
            snprintf(c->err, sizeof(c->err), "fast kernel launch failed"); return AMP_EHIP;
        }
        if (c->split_timing) HIPCHK(c, hipEventRecord(c->ev2, c->stream));
        const ListSrc ls{direct ? glist : nullptr, direct ? gcnt : nullptr, (int)fg.grid, (int)fg.rpb, (uint32_t)pl.gen_grid, segfirst, geo};
        // (ctr[CTR_LONG_N], [CTR_LONG_TICKET], [CTR_GEN_LEFT] are zeroed by the fast kernel)
        if (!direct) {
            k_gcompact<<<(unsigned)fg.grid, 256, 0, c->stream>>>(glist, gcnt, (int)fg.rpb, n, gdense, geo, (uint32_t)pl.gen_grid, c->d_ctr,
                                                                  rd->cig_off32, llist, lpos, long_kernel ? L_MAXOPS - 4 : 0);
            HIPCHK(c, hipGetLastError());
        }
        if (long_kernel) {
            k_long<<<2u * (unsigned)c->n_cu, L_WAVES * 64, 0, c->stream>>>(P, *rd, read_base, out, c->d_counts, eb, llist, lpos, gdense);
            HIPCHK(c, hipGetLastError());
        }
#ifdef AMP_DEV
        if (c->phases & 0x100u) {           // stamps of the general pass alone: the fast kernel's are dropped
            HIPCHK(c, hipMemsetAsync(&c->d_ctr[CTR_STAMP0], 0, (CTR_EV_SHARD0 - CTR_STAMP0) * sizeof(unsigned long long), c->stream));
            k_tile<true, false, true><<<(unsigned)pl.gen_blocks, T_WAVES * 64, 0, c->stream>>>(P, *rd, read_base, out, c->d_counts, eb, dlist, dcnt, 0, none,
                                                                                       direct ? nullptr : gdense, geo, (uint32_t)tg.grid, ls AMP_PHASES_ARG(c->phases));
        } else
#endif
        k_tile<false, false, true><<<(unsigned)pl.gen_blocks, T_WAVES * 64, 0, c->stream>>>(P, *rd, read_base, out, c->d_counts, eb, dlist, dcnt, 0, none,
                                                                                    direct ? nullptr : gdense, geo, (uint32_t)tg.grid, ls AMP_PHASES_ARG(c->phases));
        HIPCHK(c, hipGetLastError());
        // (the tile kernel does the indels of regular reads itself and raises the heavy pass's flag)
        HIPCHK(c, (hipError_t)heavy_launch(P, *rd, read_base, out, at(pl.pingpong), c->d_counts, eb, dlist, dcnt, pl.heavy_blocks, tg, geo, segfirst, c->stream, c->h_hist));
        c->last_gen_blocks = (int)pl.gen_blocks; c->last_heavy_blocks = (int)pl.heavy_blocks;
    } else {
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        uint32_t *const sp = at(pl.split);      // variant 3 hand-over arrays
        const SplitDesc sd{(int32_t *)sp, sp + n, sp + 2 * n, sp + 3 * n};
        int rc = variant == 3
                     ? split_launch(P, *rd, read_base, out, c->d_counts, eb, dlist, dcnt, c->n_cu, c->phases, sd, c->stream)
                     : tile_launch(P, *rd, read_base, out, c->d_counts, eb, dlist, dcnt, c->n_cu, c->phases, c->stream);
        if (rc != 0) { snprintf(c->err, sizeof(c->err), "tile kernel launch failed: %s", hipGetErrorString((hipError_t)rc)); return AMP_EHIP; }
        HIPCHK(c, hipEventRecord(c->ev2, c->stream));
        HIPCHK(c, (hipError_t)heavy_launch(P, *rd, read_base, out, at(pl.pingpong), c->d_counts, eb, dlist, dcnt, pl.heavy_grid, tg, nullptr, nullptr, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev3, c->stream));
    c->timed = true;
    c->last_split = variant != 4 || c->split_timing;
    c->last_kv = kv;
    if (variant != 4) c->hist_from = c->epoch + 1;      // no k_deferred_heavy behind a fast kernel wrote the lists of this pass: the next one has no history
    return AMP_OK;
}

extern "C" {

// The reference's coordinate helpers on the device, one lane per case: get_pos_on_query (A:389-412), get_pos_on_ref
// (A:363-386) and fix_cigar (A:415-423) -- the very device functions the kernels use (amp_read.hpp), driven directly.
__global__ void __launch_bounds__(256)
k_coordinate_helpers(int64_t n, const uint32_t *__restrict__ cig_off, uint32_t *cig, const int32_t *__restrict__ ref_start,
                     const int32_t *__restrict__ ref_pos, const int32_t *__restrict__ query_pos, int32_t *out_q, int32_t *out_r,
                     uint32_t *fixed, uint32_t *fixed_n, uint8_t *status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c0 = cig_off[i];
    const int nops = (int)(cig_off[i + 1] - c0);
    const CigBuf<1> c{cig + c0};
    int e1 = 0, e2 = 0;
    out_q[i] = pos_on_query(c, nops, ref_pos[i], ref_start[i], e1);
    out_r[i] = pos_on_ref(c, nops, query_pos[i], ref_start[i], e2);
    Emitter<CigBuf<1>> e{CigBuf<1>{fixed + c0}};
    for (int k = 0; k < nops; ++k) { const uint32_t v = c.get(k); e.push(v & 15u, v >> 4); }
    fixed_n[i] = (uint32_t)e.finish();
    status[i] = (uint8_t)((e1 & 15) | ((e2 & 15) << 4));      // one nibble per helper: the reference's get_pos_on_query returns before it touches later ops
}

int amp_coordinate_helpers(amp_ctx *c, int64_t n, const uint32_t *cig_off, const uint32_t *cig, const int32_t *ref_start,
                           const int32_t *ref_pos, const int32_t *query_pos, int32_t *pos_on_query_out, int32_t *pos_on_ref_out,
                           uint32_t *fixed_cig, uint32_t *fixed_n, uint8_t *status) {
    if (!c || n < 0) return AMP_EINVAL;
    if (n == 0) return AMP_OK;
    if (!cig_off || !ref_start || !ref_pos || !query_pos || !pos_on_query_out || !pos_on_ref_out || !fixed_cig || !fixed_n || !status)
        return AMP_EINVAL;
    const size_t nc = cig_off[n];
    if (nc && !cig) return AMP_EINVAL;
    Guard g(c->device);
    // one scratch image: offsets | ops | starts | ref positions | query positions | the two results | fixed ops | their counts | status
    const size_t words = ((size_t)n + 1) + nc + 3 * (size_t)n + 2 * (size_t)n + nc + (size_t)n + ((size_t)n + 3) / 4 + 16;
    HIPCHK(c, c->call_buf.ensure(words * 4));
    uint32_t *d = c->call_buf.as<uint32_t>();
    uint32_t *d_off = d, *d_cig = d_off + n + 1;
    int32_t *d_rs = (int32_t *)(d_cig + nc), *d_rp = d_rs + n, *d_qp = d_rp + n, *d_oq = d_qp + n, *d_or = d_oq + n;
    uint32_t *d_fx = (uint32_t *)(d_or + n), *d_fn = d_fx + nc;
    uint8_t *d_st = (uint8_t *)(d_fn + n);
    HIPCHK(c, hipMemcpyAsync(d_off, cig_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (nc) HIPCHK(c, hipMemcpyAsync(d_cig, cig, nc * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rs, ref_start, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rp, ref_pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_qp, query_pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    k_coordinate_helpers<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(n, d_off, d_cig, d_rs, d_rp, d_qp, d_oq, d_or, d_fx, d_fn, d_st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pos_on_query_out, d_oq, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pos_on_ref_out, d_or, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (nc) HIPCHK(c, hipMemcpyAsync(fixed_cig, d_fx, nc * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fixed_n, d_fn, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, d_st, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

}  // extern "C"
