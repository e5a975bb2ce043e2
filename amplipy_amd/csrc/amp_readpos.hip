// amp_readpos.hip -- read-position tallies per allele on the device (C ABI: the amp_readpos_* entry
// points of amplihip.h).
//
// k_readpos runs behind the read pass of every batch while the tallies are on and touches every counted base once more, in the
// shape of amp_tally.hpp and of k_strand: segments per read in phase A (readpos_segments, amp_readpos.hpp), position-major adds
// in phase B.  Its own part: a window position has 42 cells (six columns of seven distance bins), kept two to a word as 16-bit
// halves, 21 words a position, so that the window stays RP_W = 512 positions wide at 42 KB; a segment carries the distances of
// its first base from the two ends of the read's kept span, and lane p of a chunk turns its offset into the bin with two adds
// and a min.  Deletion segments of both strands are on the list.  The halves bound the flush period: the window goes to the
// global table every RP_MAX_TILES_PER_FLUSH tiles at the latest.  Reads the segments do not cover -- more segments than slots,
// an irregular CIGAR, a read outside the window -- walk serially (readpos_walk).  No step relies on the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "amp_hook.hpp"
#include "amp_readpos.hpp"
#include "amp_tally.hpp"

namespace amp {

struct ReadposState : HookState {
    uint32_t *d_hist = nullptr;                // [ref_len][6][7]
};

struct ReadposArgs {
    TallyReads in;
    uint32_t *hist;
};

// Entry s0 + lane of the list (seg_take of amp_tally.hpp for a ReadposSeg), and lane src's entry in every lane (seg_from)
__device__ __forceinline__ ReadposSeg rp_seg_take(const ReadposSeg *list, uint32_t s0, uint32_t ns, int lane, bool &have) {
    ReadposSeg mine;
    mine.r0 = 0; mine.len_kind = 0u; mine.q0 = 0ull; mine.dl = 0; mine.dr = 0;
    have = s0 + (uint32_t)lane < ns;
    if (have) mine = list[s0 + (uint32_t)lane];
    return mine;
}
__device__ __forceinline__ ReadposSeg rp_seg_from(const ReadposSeg &mine, int src) {
    ReadposSeg g;
    g.r0 = __shfl(mine.r0, src);
    g.len_kind = __shfl(mine.len_kind, src);
    g.q0 = __shfl((unsigned long long)mine.q0, src);
    g.dl = __shfl(mine.dl, src);
    g.dr = __shfl(mine.dr, src);
    return g;
}

// the window to the global table: a word is two cells
__device__ __forceinline__ void readpos_flush(uint32_t *s_cell, int32_t anchor, const ReadposArgs &a) {
    tally_flush<RP_BLOCK>(s_cell, RP_W * RP_WORDS, [&](int k, uint32_t v) {
        uint32_t *row = a.hist + ((size_t)anchor + (size_t)(k / RP_WORDS)) * RP_CELLS + 2 * (k % RP_WORDS);
        if (v & 0xFFFFu) atomicAdd(&row[0], v & 0xFFFFu);
        if (v >> 16) atomicAdd(&row[1], v >> 16);
    });
}

__global__ void __launch_bounds__(RP_BLOCK)
k_readpos(ReadposArgs a) {
    __shared__ uint32_t s_cell[RP_W * RP_WORDS];
    __shared__ ReadposSeg s_seg[RP_BLOCK * RP_SLOTS];
    __shared__ int32_t s_lo[RP_BLOCK / 64], s_hi[RP_BLOCK / 64];
    __shared__ uint32_t s_nseg;
    const TallyReads &in = a.in;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < RP_W * RP_WORDS; k += RP_BLOCK) s_cell[k] = 0u;
    if (tid == 0) s_nseg = 0u;
    int64_t t0, t1;
    tally_tile_range(in.n, RP_BLOCK, t0, t1);
    int32_t anchor = 0;
    int since = 0;                             // tiles since the last flush
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * RP_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = {false, 0, 0};
        const bool live = tally_live(in, i);
        if (live) {
            tally_counted_read(in, i, R, qual0);
            sh = readpos_segments(R, in.P, qual0, [](const ReadposSeg &) {});
        }
        int32_t lo = sh.regular ? R.pos : SPAN_NO_LO, hi = sh.regular ? sh.ref_end : SPAN_NO_HI;
        block_span<RP_BLOCK>(lo, hi, s_lo, s_hi);
        if (!readpos_window_keeps(anchor, lo, hi) || since >= RP_MAX_TILES_PER_FLUSH) {      // (the same for every lane)
            readpos_flush(s_cell, anchor, a);
            if (lo <= hi) anchor = lo;
            since = 0;
            __syncthreads();
        }
        ++since;
        const bool win = live && readpos_read_windowed(sh, R.pos, anchor);
        if (win && sh.n_seg > 0) {
            uint32_t slot = atomicAdd(&s_nseg, (uint32_t)sh.n_seg);        // (at most RP_SLOTS per read: the list cannot overflow)
            readpos_segments(R, in.P, qual0, [&](const ReadposSeg &s) { s_seg[slot++] = s; });
        }
        __syncthreads();
        // ---- phase B: position-major over the tile's segments; lane `lane` of the wave owns position c * 64 + lane of chunk c,
        // so no two lanes of a wave add to the same word
        const uint32_t ns = s_nseg;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                        // (ns is block-uniform: whole waves at the ballots)
            bool have;
            const ReadposSeg mine = rp_seg_take(s_seg, s0, ns, lane, have);
            const int32_t m0 = mine.r0 - anchor, m1 = m0 + rp_seg_len(mine);
            for (int c = wave; c < RP_W / RP_CHUNK; c += RP_BLOCK / 64) {
                const int32_t c0 = c * RP_CHUNK;
                unsigned long long hits = __ballot(have && m1 > c0 && m0 < c0 + RP_CHUNK);
                const int32_t p = c0 + lane;
                while (hits) {
                    const int src = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    const ReadposSeg g = rp_seg_from(mine, src);
                    const int32_t a0 = g.r0 - anchor, a1 = a0 + rp_seg_len(g);
                    if (p >= a0 && p < a1) {                               // (else not this lane's position; every lane is back for the next segment's shuffles)
                        uint32_t col = 5u;
                        if (rp_seg_del(g) || readpos_base(in.seq, in.qual, g.q0 + (uint64_t)(p - a0), in.P.min_quality, col)) {
                            const int cell = rp_cell(col, rp_bin(rp_seg_d(g, p - a0)));
                            s_cell[rp_word(p, cell)] += rp_one(cell);
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_nseg = 0u;
        // ---- the serial path: reads the window did not take
        if (live && !win) {
            readpos_walk(R, in.P, in.seq, in.qual, [&](int32_t r, uint32_t col, int32_t d) {
                const int cell = rp_cell(col, rp_bin(d));
                const int64_t w = (int64_t)r - (int64_t)anchor;
                if (w >= 0 && w < RP_W) atomicAdd(&s_cell[rp_word((int32_t)w, cell)], rp_one(cell));
                else atomicAdd(&a.hist[(size_t)r * RP_CELLS + cell], 1u);
            });
        }
        __syncthreads();
    }
    readpos_flush(s_cell, anchor, a);
}

static size_t readpos_bytes(int32_t ref_len) { return (size_t)ref_len * RP_CELLS * sizeof(uint32_t); }

static ReadposState *readpos_state(amp_ctx *c) { return hook_state<ReadposState>(c, HOOK_READPOS); }

static void readpos_free(void *state) {
    ReadposState *s = hook_state_of<ReadposState>(state);
    if (!s) return;
    if (s->d_hist) (void)hipFree(s->d_hist);
    s->timer.destroy();
    delete s;
}

static int readpos_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    ReadposState *s = readpos_state(c);
    return hook_launch(q, s, readpos_hook, rd->n_reads, o, RP_BLOCK, RP_TILES_PER_BLOCK, RP_BLOCKS_PER_CU, [&](unsigned grid) {
        k_readpos<<<grid, RP_BLOCK, 0, q.stream>>>(ReadposArgs{tally_reads(q, rd, o), s->d_hist});
    });
}

static int readpos_reset(amp_ctx *c) {
    const HookCtx q = ctx_hook(c);
    HOOKCHK(q, hipMemsetAsync(readpos_state(c)->d_hist, 0, readpos_bytes(q.ref_len), q.stream));
    return AMP_OK;
}

HookOps readpos_hook = {"the read-position tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, readpos_enqueue, readpos_reset, readpos_free};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_readpos_enable(amp_ctx *c, int on) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_READPOS);
    if (!on) { slot.on = false; return AMP_OK; }
    Guard g(q.device);
    ReadposState *s = readpos_state(c);
    if (!s) {
        const int rc = hook_new_state(q, slot, readpos_hook, s, [&](ReadposState &f) -> int {
            HOOKCHK(q, hipMalloc((void **)&f.d_hist, std::max<size_t>(readpos_bytes(q.ref_len), 64)));
            return AMP_OK;
        });
        if (rc != AMP_OK) return rc;
    }
    HOOKCHK(q, hipMemsetAsync(s->d_hist, 0, readpos_bytes(q.ref_len), q.stream));
    slot.on = true;
    return AMP_OK;
}

int amp_readpos_get(amp_ctx *c, uint32_t *hist) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    ReadposState *s = readpos_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    if (hist && q.ref_len) HOOKCHK(q, hipMemcpyAsync(hist, s->d_hist, readpos_bytes(q.ref_len), hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

int amp_readpos_add(amp_ctx *c, const uint32_t *hist) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    ReadposState *s = readpos_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    return hook_add(q, s->d_hist, hist, (size_t)q.ref_len * RP_CELLS);
}

int amp_readpos_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_READPOS, ms); }

}  // extern "C"
