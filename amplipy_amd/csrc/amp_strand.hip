// amp_strand.hip -- per-allele strand and base-quality tallies on the device (C ABI: the amp_strand_*
// entry points of amplihip.h).
//
// k_strand runs behind the read pass of every batch while the tallies are on and touches every counted base a second time.
// The normal input is a coordinate-sorted pile of thousands of reads on one amplicon, so lanes that walked neighbouring reads
// base by base would add onto the same few addresses in lock-step.  The kernel turns the work round instead, in the shape of
// amp_tally.hpp: segments per read in phase A (strand_segments, amp_strand.hpp), position-major adds in phase B.  Its own
// part: the block keeps a window of ST_W reference positions x 11 u32 cells in LDS; each wave owns every fourth 64-position
// chunk of it and each lane one position of the chunk; the wave loops over the tile's segments that overlap its chunk, and
// lane p loads qual[q0 + p - r0] and the base nibble -- consecutive lanes, consecutive bytes -- and adds into its OWN cells.
// The window stays where it is while the block's next tile fits it (in a sorted batch it mostly does).  Reads the segments
// do not cover -- more segments than slots, an irregular CIGAR, a read outside the window (a tile wider than the window, an
// unsorted batch) -- walk serially (strand_walk): slow and correct.  No step relies on the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "amp_hook.hpp"
#include "amp_strand.hpp"
#include "amp_tally.hpp"

namespace amp {

struct StrandState : HookState {
    unsigned long long *d_qsum = nullptr;      // [ref_len][5]; one allocation of 64 bytes per position with ...
    uint32_t *d_rev = nullptr;                 // ... [ref_len][6] behind it
};

struct StrandArgs {
    TallyReads in;
    uint32_t *rev;
    unsigned long long *qsum;
};

// the window to the global tables
__device__ __forceinline__ void strand_flush(uint32_t *s_cell, int32_t anchor, const StrandArgs &a) {
    tally_flush<ST_BLOCK>(s_cell, ST_W * ST_CELLS, [&](int k, uint32_t v) {
        const size_t p = (size_t)anchor + (size_t)(k / ST_CELLS);
        const int c = k % ST_CELLS;
        if (c < ST_REV_COLS) atomicAdd(&a.rev[p * ST_REV_COLS + c], v);
        else atomicAdd(&a.qsum[p * ST_QSUM_COLS + (c - ST_REV_COLS)], (unsigned long long)v);
    });
}

__global__ void __launch_bounds__(ST_BLOCK)
k_strand(StrandArgs a) {
    __shared__ uint32_t s_cell[ST_W * ST_CELLS];
    __shared__ StrandSeg s_seg[ST_BLOCK * ST_SLOTS];
    __shared__ int32_t s_lo[ST_BLOCK / 64], s_hi[ST_BLOCK / 64];
    __shared__ uint32_t s_nseg;
    const TallyReads &in = a.in;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < ST_W * ST_CELLS; k += ST_BLOCK) s_cell[k] = 0u;
    if (tid == 0) s_nseg = 0u;
    int64_t t0, t1;
    tally_tile_range(in.n, ST_BLOCK, t0, t1);
    int32_t anchor = 0;
    int since = 0;                             // tiles since the last flush
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * ST_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = {false, 0, 0};
        const bool live = tally_live(in, i);
        if (live) {
            tally_counted_read(in, i, R, qual0);
            sh = strand_segments(R, in.P, qual0, [](const StrandSeg &) {});
        }
        int32_t lo = sh.regular ? R.pos : SPAN_NO_LO, hi = sh.regular ? sh.ref_end : SPAN_NO_HI;
        block_span<ST_BLOCK>(lo, hi, s_lo, s_hi);
        if (!strand_window_keeps(anchor, lo, hi) || since >= ST_MAX_TILES_PER_FLUSH) {       // (the same for every lane)
            strand_flush(s_cell, anchor, a);
            if (lo <= hi) anchor = lo;
            since = 0;
            __syncthreads();
        }
        ++since;
        const bool win = live && strand_read_windowed(sh, R.pos, anchor);
        if (win && sh.n_seg > 0) {
            uint32_t slot = atomicAdd(&s_nseg, (uint32_t)sh.n_seg);        // (at most ST_SLOTS per read: the list cannot overflow)
            strand_segments(R, in.P, qual0, [&](const StrandSeg &s) { s_seg[slot++] = s; });
        }
        __syncthreads();
        // ---- phase B: position-major over the tile's segments; lane `lane` of the wave owns position c * 64 + lane of chunk c
        // A segment touches three or four of the eight chunks, so most of the list is no work for a given chunk and costs a
        // sixty-fourth of a trip here.
        const uint32_t ns = s_nseg;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                        // (ns is block-uniform: whole waves at the ballots)
            bool have;
            const StrandSeg mine = seg_take(s_seg, s0, ns, lane, have);
            const int32_t m0 = mine.r0 - anchor, m1 = m0 + st_seg_len(mine);
            for (int c = wave; c < ST_W / ST_CHUNK; c += ST_BLOCK / 64) {
                const int32_t c0 = c * ST_CHUNK;
                unsigned long long hits = __ballot(have && m1 > c0 && m0 < c0 + ST_CHUNK);
                const int32_t p = c0 + lane;
                while (hits) {
                    const int src = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    const StrandSeg g = seg_from(mine, src);
                    const int32_t a0 = g.r0 - anchor, a1 = a0 + st_seg_len(g);
                    if (p < a0 || p >= a1) {
                        // (not this lane's position; every lane is back for the next segment's shuffles)
                    } else if (st_seg_del(g)) {
                        s_cell[st_cell_rev(p, 5u)] += 1u;                  // (a forward read's deletions are not in the list)
                    } else {
                        uint32_t col, qv;
                        if (strand_base(in.seq, in.qual, g.q0 + (uint64_t)(p - a0), in.P.min_quality, col, qv)) {
                            s_cell[st_cell_qsum(p, col)] += qv;
                            if (st_seg_rev(g)) s_cell[st_cell_rev(p, col)] += 1u;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_nseg = 0u;
        // ---- the serial path: reads the window did not take
        if (live && !win) {
            const uint32_t rev = R.rev;
            strand_walk(R, in.P, in.seq, in.qual, [&](int32_t r, uint32_t col, uint32_t qv) {
                const int64_t w = (int64_t)r - (int64_t)anchor;
                if (w >= 0 && w < ST_W) {
                    if (rev) atomicAdd(&s_cell[st_cell_rev((int32_t)w, col)], 1u);
                    if (col < (uint32_t)ST_QSUM_COLS) atomicAdd(&s_cell[st_cell_qsum((int32_t)w, col)], qv);
                } else {
                    if (rev) atomicAdd(&a.rev[(size_t)r * ST_REV_COLS + col], 1u);
                    if (col < (uint32_t)ST_QSUM_COLS) atomicAdd(&a.qsum[(size_t)r * ST_QSUM_COLS + col], (unsigned long long)qv);
                }
            });
        }
        __syncthreads();
    }
    strand_flush(s_cell, anchor, a);
}

static size_t strand_bytes(int32_t ref_len) { return (size_t)ref_len * 64; }

static StrandState *strand_state(amp_ctx *c) { return hook_state<StrandState>(c, HOOK_STRAND); }

static void strand_free(void *state) {
    StrandState *s = hook_state_of<StrandState>(state);
    if (!s) return;
    if (s->d_qsum) (void)hipFree(s->d_qsum);
    s->timer.destroy();
    delete s;
}

static int strand_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    StrandState *s = strand_state(c);
    // (a block's window is flushed when it moves, not per tile)
    return hook_launch(q, s, strand_hook, rd->n_reads, o, ST_BLOCK, ST_TILES_PER_BLOCK, ST_BLOCKS_PER_CU, [&](unsigned grid) {
        k_strand<<<grid, ST_BLOCK, 0, q.stream>>>(StrandArgs{tally_reads(q, rd, o), s->d_rev, s->d_qsum});
    });
}

static int strand_reset(amp_ctx *c) {
    const HookCtx q = ctx_hook(c);
    HOOKCHK(q, hipMemsetAsync(strand_state(c)->d_qsum, 0, strand_bytes(q.ref_len), q.stream));
    return AMP_OK;
}

HookOps strand_hook = {"the strand tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, strand_enqueue, strand_reset, strand_free};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_strand_enable(amp_ctx *c, int on) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_STRAND);
    if (!on) { slot.on = false; return AMP_OK; }
    Guard g(q.device);
    StrandState *s = strand_state(c);
    if (!s) {
        const int rc = hook_new_state(q, slot, strand_hook, s, [&](StrandState &f) -> int {
            HOOKCHK(q, hipMalloc((void **)&f.d_qsum, std::max<size_t>(strand_bytes(q.ref_len), 64)));
            f.d_rev = (uint32_t *)(f.d_qsum + (size_t)q.ref_len * ST_QSUM_COLS);
            return AMP_OK;
        });
        if (rc != AMP_OK) return rc;
    }
    HOOKCHK(q, hipMemsetAsync(s->d_qsum, 0, strand_bytes(q.ref_len), q.stream));
    slot.on = true;
    return AMP_OK;
}

int amp_strand_get(amp_ctx *c, uint32_t *rev, uint64_t *qsum) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    StrandState *s = strand_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    const size_t G = (size_t)q.ref_len;
    if (rev && G) HOOKCHK(q, hipMemcpyAsync(rev, s->d_rev, G * ST_REV_COLS * 4, hipMemcpyDeviceToHost, q.stream));
    if (qsum && G) HOOKCHK(q, hipMemcpyAsync(qsum, s->d_qsum, G * ST_QSUM_COLS * 8, hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

int amp_strand_add(amp_ctx *c, const uint32_t *rev, const uint64_t *qsum) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    StrandState *s = strand_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    const size_t G = (size_t)q.ref_len;
    const int rc = hook_add(q, s->d_rev, rev, G * ST_REV_COLS);
    return rc != AMP_OK ? rc : hook_add(q, (uint64_t *)s->d_qsum, qsum, G * ST_QSUM_COLS);
}

int amp_strand_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_STRAND, ms); }

}  // extern "C"
