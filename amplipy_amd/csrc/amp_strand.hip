// amp_strand.hip -- per-allele strand and base-quality tallies on the device (C ABI: the amp_strand_*
// entry points of amplihip.h).
//
// k_strand runs behind the read pass of every batch while the tallies are on and touches every counted base a second time.
// The normal input is a coordinate-sorted pile of thousands of reads on one amplicon, so lanes that walked neighbouring reads
// base by base would add onto the same few addresses in lock-step.  The kernel turns the work round instead.  A block takes
// 256 neighbouring reads.  Phase A, one lane per read: the read's CIGAR becomes a few segments in LDS (strand_segments,
// amp_strand.hpp).  Phase B, position-major: the block keeps a window of ST_W reference positions x 11 u32 cells in LDS;
// each wave owns every fourth 64-position chunk of it and each lane one position of the chunk; the wave loops over the tile's
// segments that overlap its chunk (wave-uniform: found 64 at a time by a ballot), and lane p loads qual[q0 + p - r0] and the base nibble
// -- consecutive lanes, consecutive bytes -- and adds into its OWN cells with a plain LDS add: no two lanes share an address.
// The window stays where it is while the block's next tile fits it (a block takes a contiguous run of tiles, so in a sorted
// batch it mostly does); when it moves and when the block ends, the non-zero cells go to the global tables, one atomic each.
// Reads the segments do not cover -- more segments than slots, an irregular CIGAR, a read outside the window (a tile wider
// than the window, an unsorted batch) -- walk serially, one lane per read (strand_walk), with LDS atomics inside the window
// and global atomics outside: slow and correct.  No step relies on the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "amp_hook.hpp"
#include "amp_strand.hpp"

namespace amp {

struct StrandState {
    unsigned long long *d_qsum = nullptr;      // [ref_len][5]; one allocation of 64 bytes per position with ...
    uint32_t *d_rev = nullptr;                 // ... [ref_len][6] behind it
    HookTimer timer;
};

struct StrandArgs {
    int64_t n;
    const int32_t *pos;
    const uint16_t *flag;
    const uint32_t *lseq, *cig_off32, *cig, *seq_off8;
    const uint8_t *seq, *qual;
    const int32_t *new_pos;                    // the trimmed alignment (do_trim)
    const uint32_t *new_ncig, *new_cig;
    const uint8_t *status;                     // may be null without do_trim
    int32_t do_trim;
    StrandParams P;
    uint32_t *rev;
    unsigned long long *qsum;
};

// the non-zero cells of the window to the global tables, one atomic each; the window is all zero afterwards
__device__ __forceinline__ void strand_flush(uint32_t *s_cell, int32_t anchor, const StrandArgs &a) {
    for (int k = (int)threadIdx.x; k < ST_W * ST_CELLS; k += ST_BLOCK) {
        const uint32_t v = s_cell[k];
        if (!v) continue;
        s_cell[k] = 0u;
        const size_t p = (size_t)anchor + (size_t)(k / ST_CELLS);
        const int c = k % ST_CELLS;
        if (c < ST_REV_COLS) atomicAdd(&a.rev[p * ST_REV_COLS + c], v);
        else atomicAdd(&a.qsum[p * ST_QSUM_COLS + (c - ST_REV_COLS)], (unsigned long long)v);
    }
}

__global__ void __launch_bounds__(ST_BLOCK)
k_strand(StrandArgs a) {
    __shared__ uint32_t s_cell[ST_W * ST_CELLS];
    __shared__ StrandSeg s_seg[ST_BLOCK * ST_SLOTS];
    __shared__ int32_t s_lo[ST_BLOCK / 64], s_hi[ST_BLOCK / 64];
    __shared__ uint32_t s_nseg;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < ST_W * ST_CELLS; k += ST_BLOCK) s_cell[k] = 0u;
    if (tid == 0) s_nseg = 0u;
    // the block's contiguous run of tiles (the bounds are the same for every lane: the barriers below see whole blocks)
    const int64_t tiles = (a.n + ST_BLOCK - 1) / ST_BLOCK;
    const int64_t t0 = tiles * (int64_t)blockIdx.x / (int64_t)gridDim.x, t1 = tiles * ((int64_t)blockIdx.x + 1) / (int64_t)gridDim.x;
    int32_t anchor = 0;
    int since = 0;                             // tiles since the last flush
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * ST_BLOCK + tid;
        StrandRead R;
        R.pos = 0; R.cig = a.cig; R.n_ops = 0u; R.lseq = 0; R.rev = 0u; R.base = 0ull;
        StrandShape sh;
        sh.regular = false; sh.n_seg = 0; sh.ref_end = 0;
        bool live = false;
        uint32_t qual0 = 0xFFu;
        if (i < a.n && (a.status ? a.status[i] == 0 : true)) {
            live = true;
            const uint32_t c0 = a.cig_off32[i];
            if (a.do_trim) {
                R.pos = a.new_pos[i]; R.cig = a.new_cig + (size_t)c0 + 3 * (size_t)i; R.n_ops = a.new_ncig[i];
            } else {
                R.pos = a.pos[i]; R.cig = a.cig + c0; R.n_ops = a.cig_off32[i + 1] - c0;
            }
            R.lseq = (int32_t)a.lseq[i];
            R.rev = (a.flag[i] & 0x10u) ? 1u : 0u;
            R.base = (uint64_t)a.seq_off8[i] * 8ull;
            if (R.lseq > 0) qual0 = a.qual[R.base];
            sh = strand_segments(R, a.P, qual0, [](const StrandSeg &) {});
        }
        int32_t lo = sh.regular ? R.pos : 0x7FFFFFFF, hi = sh.regular ? sh.ref_end : -0x7FFFFFFF - 1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d));
            hi = max(hi, __shfl_xor(hi, d));
        }
        if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < ST_BLOCK / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
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
            strand_segments(R, a.P, qual0, [&](const StrandSeg &s) { s_seg[slot++] = s; });
        }
        __syncthreads();
        // ---- phase B: position-major over the tile's segments; lane `lane` of the wave owns position c * 64 + lane of chunk c
        // The wave takes the list 64 segments at a time, a segment per lane, ballots which of them overlap the chunk, and
        // visits only those (their fields broadcast by shuffle): a segment touches three or four of the eight chunks, so most
        // of the list is no work for a given chunk and costs a sixty-fourth of a trip here.
        const uint32_t ns = s_nseg;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                        // (ns is block-uniform: whole waves at the ballots)
            const bool have = s0 + (uint32_t)lane < ns;
            StrandSeg mine;
            mine.r0 = 0; mine.len_kind = 0u; mine.q0 = 0ull;
            if (have) mine = s_seg[s0 + (uint32_t)lane];
            const int32_t m0 = mine.r0 - anchor, m1 = m0 + st_seg_len(mine);
            for (int c = wave; c < ST_W / ST_CHUNK; c += ST_BLOCK / 64) {
                const int32_t c0 = c * ST_CHUNK;
                unsigned long long hits = __ballot(have && m1 > c0 && m0 < c0 + ST_CHUNK);
                const int32_t p = c0 + lane;
                while (hits) {
                    const int src = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    StrandSeg g;
                    g.r0 = __shfl(mine.r0, src);
                    g.len_kind = __shfl(mine.len_kind, src);
                    g.q0 = __shfl((unsigned long long)mine.q0, src);
                    const int32_t a0 = g.r0 - anchor, a1 = a0 + st_seg_len(g);
                    if (p < a0 || p >= a1) {
                        // (not this lane's position; every lane is back for the next segment's shuffles)
                    } else if (st_seg_del(g)) {
                        s_cell[st_cell_rev(p, 5u)] += 1u;                  // (a forward read's deletions are not in the list)
                    } else {
                        uint32_t col, qv;
                        if (strand_base(a.seq, a.qual, g.q0 + (uint64_t)(p - a0), a.P.min_quality, col, qv)) {
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
            strand_walk(R, a.P, a.seq, a.qual, [&](int32_t r, uint32_t col, uint32_t qv) {
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

static StrandState *strand_state(amp_ctx *c) { return (StrandState *)hook_slot(c, HOOK_STRAND).state; }

static void strand_free(void *state) {
    StrandState *s = (StrandState *)state;
    if (!s) return;
    if (s->d_qsum) (void)hipFree(s->d_qsum);
    s->timer.destroy();
    delete s;
}

static int strand_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    StrandState *s = strand_state(c);
    s->timer.timed = false;
    const int64_t n = rd->n_reads;
    if (n <= 0) return AMP_OK;
    const int rc = hook_check_out(q, o, strand_hook);
    if (rc != AMP_OK) return rc;
    StrandArgs a;
    a.n = n; a.pos = rd->pos; a.flag = rd->flag; a.lseq = rd->lseq; a.cig_off32 = rd->cig_off32; a.cig = rd->cig; a.seq_off8 = rd->seq_off8;
    a.seq = rd->seq; a.qual = rd->qual;
    a.new_pos = o ? o->new_pos : nullptr; a.new_ncig = o ? o->new_ncig : nullptr; a.new_cig = o ? o->new_cig : nullptr;
    a.status = o ? o->status : nullptr;
    a.do_trim = q.do_trim ? 1 : 0;
    a.P = StrandParams{q.ref_len, q.min_quality};
    a.rev = s->d_rev; a.qsum = s->d_qsum;
    HOOKCHK(q, s->timer.begin(q.stream));           // (below: a block's window is flushed when it moves, not per tile)
    k_strand<<<hook_grid(n, ST_BLOCK, ST_TILES_PER_BLOCK, ST_BLOCKS_PER_CU, q.n_cu), ST_BLOCK, 0, q.stream>>>(a);
    HOOKCHK(q, hipGetLastError());
    HOOKCHK(q, s->timer.end(q.stream));
    return AMP_OK;
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
        s = new (std::nothrow) StrandState();
        if (!s) return AMP_ENOMEM;
        HookDrop drop{strand_hook, s};
        HOOKCHK(q, hipMalloc((void **)&s->d_qsum, std::max<size_t>(strand_bytes(q.ref_len), 64)));
        s->d_rev = (uint32_t *)(s->d_qsum + (size_t)q.ref_len * ST_QSUM_COLS);
        HOOKCHK(q, s->timer.create());
        drop.state = nullptr;
        slot.state = s;
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

int amp_strand_last_ms(amp_ctx *c, float *ms) {
    if (!c) return AMP_EINVAL;
    StrandState *s = strand_state(c);
    return s ? s->timer.last_ms(ctx_hook(c), ms) : AMP_ESTATE;
}

}  // extern "C"
