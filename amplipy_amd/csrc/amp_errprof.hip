// amp_errprof.hip -- the error profile by cycle, quality and substitution, tallied on the device (C ABI:
// the amp_errprof_* entry points of amplihip.h; semantics in amp_errprof.hpp).
//
// k_errprof runs behind the read pass of every batch while the hook is on, last of the hooks.  It has the tally skeleton's
// outer shape (amp_tally.hpp: 256-lane blocks over contiguous runs of 256-read tiles, one lane per read in phase A), but its
// table is not positional: a keyed histogram of EP_CELLS (2,552) cells into which EVERY match base of a pile lands, so what
// has to be designed is the contention, not the walk.  Phase A puts each regular read's match segments on the tile's list in
// LDS.  Phase B: a wave takes the list an entry at a time, its lanes on 64 CONSECUTIVE BASES OF ONE SEGMENT -- qual, seq and
// reference-code loads are consecutive bytes, mate and strand are wave-uniform, and the 64 lanes hold 64 different cycles.
// The three adds of a base reach the block's u32 cells like this:
//   cyc    each lane adds 1 to its own cell (64 different cycles: 64 different addresses, and with the block's [m][e][c]
//          layout 64 different banks); only lanes clamped into the open-ended last bin share a cell, and those are combined;
//   qualt  the lanes' keys are combined: the leader of each group of equal keys gets the group's popcount by a ballot loop
//   sub    (one trip per DISTINCT key of the 64 lanes: 4 to 8 with binned qualities, a handful of classes), and when the loop
//          is over all leaders add at once -- different keys, different addresses.
// So no instruction has two lanes of a wave on one address, and nothing per base goes to HBM.  (Lanes of different waves may
// meet on a cell; that is what the LDS atomic is for.)  The block's non-zero cells go to the u64 tables when the block ends
// and every EP_MAX_TILES_PER_FLUSH tiles, one atomic each.  Reads with more segments than slots walk serially in their lane
// with LDS atomics, reads longer than EP_LDS_LSEQ bases serially into the u64 tables: slow and correct.  No step relies on
// the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "amp_errprof.hpp"
#include "amp_hook.hpp"
#include "amp_strand.hpp"
#include "amp_tally.hpp"

namespace amp {

struct ErrprofState : HookState {
    unsigned long long *d_cells = nullptr;     // [EP_CELLS]: cyc, qualt, sub in the ABI's layout, then reads[2]
    uint8_t *d_code = nullptr;                 // [ref_len]: the reference codes
};

struct ErrprofArgs {
    TallyReads in;
    const uint8_t *code;
    unsigned long long *cells;                 // [EP_CELLS + 2]
};

// cells[key] += the number of lanes with `have` and this key, one add per distinct key of the wave: the leaders' counts by a
// ballot loop, then every leader's add in one instruction.  Whole waves call it.
__device__ __forceinline__ void ep_combine_add(uint32_t *cells, bool have, int key, int lane) {
    uint32_t mine = 0u;
    const auto same_key = [&](int src) {
        const int lk = __shfl(key, src);
        return have && key == lk;
    };
    wave_each_distinct(have, same_key, [&](int src, unsigned long long same) { if (lane == src) mine = (uint32_t)__popcll(same); });
    if (mine) atomicAdd(&cells[key], mine);
}

// DO_TRIM: in.do_trim as a constant of the kernel -- each of the two kernels carries one alignment's pointers, not both
template <bool DO_TRIM>
__global__ void __launch_bounds__(EP_BLOCK)
k_errprof(ErrprofArgs a) {
    __shared__ uint32_t s_cell[EP_CELLS];
    __shared__ EpSeg s_seg[EP_BLOCK * EP_SLOTS];
    __shared__ uint32_t s_n[2];                // segments on the list, by the tile's parity (the other one is zeroed meanwhile)
    TallyReads in = a.in;
    in.do_trim = DO_TRIM ? 1 : 0;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < EP_CELLS; k += EP_BLOCK) s_cell[k] = 0u;
    if (tid == 0) { s_n[0] = 0u; s_n[1] = 0u; }
    int64_t t0, t1;
    tally_tile_range(in.n, EP_BLOCK, t0, t1);
    int since = 0;                             // tiles since the last flush
    uint32_t n_profiled = 0u, n_skipped = 0u;
    auto flush = [&]() { tally_flush<EP_BLOCK>(s_cell, EP_CELLS, [&](int k, uint32_t v) { atomicAdd(&a.cells[ep_block_to_global(k)], (unsigned long long)v); }); };
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        const int par = (int)((t - t0) & 1);
        if (since >= EP_MAX_TILES_PER_FLUSH) {                             // (the same for every lane)
            flush();
            since = 0;
            __syncthreads();
        }
        ++since;
        // ---- phase A: one lane per read; its match segments onto the tile's list
        const int64_t i = t * EP_BLOCK + tid;
        if (tally_live(in, i)) {
            StrandRead R;
            uint32_t qual0 = 0xFFu;
            tally_counted_read(in, i, R, qual0);
            const uint32_t mate = (in.flag[i] & 0x80u) ? 1u : 0u;
            const StrandShape sh = errprof_segments(R, in.P, qual0, mate, [](const EpSeg &) {});
            if (!sh.regular) {
                ++n_skipped;
            } else if (ep_read_listed(sh, R.lseq)) {
                ++n_profiled;
                if (sh.n_seg > 0) {
                    uint32_t slot = atomicAdd(&s_n[par], (uint32_t)sh.n_seg);      // (at most EP_SLOTS per read: the list cannot overflow)
                    errprof_segments(R, in.P, qual0, mate, [&](const EpSeg &g) { s_seg[slot++] = g; });
                }
            } else {                                                       // the serial path
                ++n_profiled;
                const bool in_block = ep_read_in_block(R.lseq);
                errprof_segments(R, in.P, qual0, mate, [&](const EpSeg &g) {
                    errprof_seg_walk(g, in.seq, in.qual, a.code, in.P.min_quality, [&](int kc, int kq, int ks) {
                        if (in_block) {
                            atomicAdd(&s_cell[kc], 1u); atomicAdd(&s_cell[kq], 1u); atomicAdd(&s_cell[ks], 1u);
                        } else {
                            atomicAdd(&a.cells[ep_block_to_global(kc)], 1ull); atomicAdd(&a.cells[kq], 1ull); atomicAdd(&a.cells[ks], 1ull);
                        }
                    });
                });
            }
        }
        __syncthreads();
        // ---- phase B: a wave per list entry, its lanes on consecutive bases of the segment
        if (tid == 0) s_n[par ^ 1] = 0u;
        const uint32_t ns = s_n[par];
        for (uint32_t s = (uint32_t)wave; s < ns; s += (uint32_t)(EP_BLOCK / 64)) {          // (wave-uniform: whole waves at the ballots)
            const EpSeg g = s_seg[s];
            const uint32_t m = ep_seg_mate(g), rev = ep_seg_rev(g);
            for (uint32_t j0 = 0u; j0 < g.len; j0 += 64u) {
                const uint32_t j = j0 + (uint32_t)lane;
                bool part = false;
                int kc = 0, kq = 0, ks = 0;
                int32_t c = 0;
                if (j < g.len) {
                    const uint64_t k = g.q0 + j;
                    c = ep_seg_cycle(g, j);
                    part = errprof_base(st_base_code(in.seq, k), a.code[(int64_t)g.r0 + j], in.qual[k], m, rev, c, in.P.min_quality, kc, kq, ks);
                }
                const bool open_end = part && c >= EP_CYCLES - 1;          // the clamped lanes share the last bin's two cells
                if (part && !open_end) atomicAdd(&s_cell[kc], 1u);
                if (__ballot(open_end)) ep_combine_add(s_cell, open_end, kc, lane);
                ep_combine_add(s_cell, part, kq, lane);
                ep_combine_add(s_cell, part, ks, lane);
            }
        }
        __syncthreads();
    }
    flush();
    tally_wave_add2(a.cells + EP_CELLS, n_profiled, n_skipped);        // the block's reads
}

static ErrprofState *errprof_state(amp_ctx *c) { return hook_state<ErrprofState>(c, HOOK_ERRPROF); }

static int errprof_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    ErrprofState *s = errprof_state(c);
    return hook_launch(q, s, errprof_hook, rd->n_reads, o, EP_BLOCK, EP_TILES_PER_BLOCK, EP_BLOCKS_PER_CU, [&](unsigned grid) {
        const ErrprofArgs a = {tally_reads(q, rd, o), s->d_code, s->d_cells};
        if (a.in.do_trim) k_errprof<true><<<grid, EP_BLOCK, 0, q.stream>>>(a);
        else k_errprof<false><<<grid, EP_BLOCK, 0, q.stream>>>(a);
    });
}

HookOps errprof_hook = {"the error profile needs", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, errprof_enqueue, hook_free<ErrprofState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_errprof_enable(amp_ctx *c, int on, const uint8_t *ref_ascii, const uint32_t *mask_bits) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_ERRPROF);
    if (!on) { slot.on = false; return AMP_OK; }
    if (!ref_ascii) {
        snprintf(q.err, q.err_cap, "the error profile needs the reference's letters");
        return AMP_EINVAL;
    }
    std::vector<uint8_t> code((size_t)std::max(q.ref_len, 1), EP_NO_CODE);
    errprof_ref_codes(ref_ascii, mask_bits, q.ref_len, code.data());
    Guard g(q.device);
    ErrprofState *s = errprof_state(c);
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, errprof_hook, s, [&](ErrprofState &f) -> int {
            HOOKTRY(hook_alloc(q, f, &f.d_cells, (size_t)(EP_CELLS + 2) * 8, (size_t)(EP_CELLS + 2) * 8));
            HOOKTRY(hook_alloc(q, f, &f.d_code, code.size()));
            hook_table(f, f.d_cells, EP_CYC_CELLS);
            hook_table(f, f.d_cells + EP_QUAL_AT, EP_QUAL_CELLS);
            hook_table(f, f.d_cells + EP_SUB_AT, EP_SUB_CELLS);
            hook_table(f, f.d_cells + EP_CELLS, 2);
            return AMP_OK;
        }));
    }
    slot.on = false;
    HOOKCHK(q, hipStreamSynchronize(q.stream));            // (a kernel on the codes of the call before may still be in flight)
    HOOKCHK(q, hipMemcpyAsync(s->d_code, code.data(), code.size(), hipMemcpyHostToDevice, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_errprof_get(amp_ctx *c, uint64_t *cyc, uint64_t *qualt, uint64_t *sub, uint64_t *reads) { return hook_get(c, HOOK_ERRPROF, {cyc, qualt, sub, reads}); }

int amp_errprof_add(amp_ctx *c, const uint64_t *cyc, const uint64_t *qualt, const uint64_t *sub, const uint64_t *reads) {
    return hook_add_tables(c, HOOK_ERRPROF, {cyc, qualt, sub, reads});
}

int amp_errprof_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_ERRPROF, ms); }

}  // extern "C"
