// amp_codon.hip -- codon tallies within single reads on the device (C ABI: the amp_codon_* entry points
// of amplihip.h).
//
// k_codon runs behind the read pass of every batch while the hook is on, last of the hooks, in the shape of amp_tally.hpp
// with lanes owning codon slots instead of positions; what follows is its own part.  Phase A: the read's CIGAR becomes a
// few list entries in LDS (codon_segments, amp_codon.hpp) -- match segments as the codon starts they hold, and the intervals
// of codon starts the read breaks.  Phase B, slot-major: the block keeps a window of CD_W consecutive slots x 65 u32 cells in
// LDS; a wave owns a 64-slot chunk of it and each lane one slot; the wave visits the entries that overlap its chunk's range of
// starts, and the lane of slot s tests whether its codon start lies in the entry: for a match segment it loads three quality
// bytes and three nibbles and adds to its triplet's cell, for a break interval it adds to cell 64.  The window stays while the
// block's next tile fits it.  Reads the list does not cover -- more entries than CD_SLOTS, a read outside the window -- go
// serially (codon_read), with LDS atomics inside the window and global atomics outside.  No step relies on the reads being
// sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "amp_hook.hpp"
#include "amp_codon.hpp"
#include "amp_tally.hpp"

namespace amp {

struct CodonState : HookState {
    int32_t n_slots = 0;
    std::vector<int32_t> starts;               // the host's copy: the set is laid out again only when it changed
    int32_t *d_starts = nullptr;               // [n_slots]
    uint32_t *d_codon = nullptr;               // [n_slots][65]
    unsigned long long *d_reads = nullptr;     // [2]: tallied, skipped
};

struct CodonArgs {
    TallyReads in;
    int32_t n_slots;
    const int32_t *starts;
    uint32_t *codon;
    unsigned long long *reads;
};

// the window to the global table.  (Only slots below n_slots are ever added to: a0 + k / 65 is inside the table for every
// non-zero cell.)
__device__ __forceinline__ void codon_flush(uint32_t *s_cell, int32_t a0, const CodonArgs &a) {
    tally_flush<CD_BLOCK>(s_cell, CD_W * CD_CELLS, [&](int k, uint32_t v) { atomicAdd(&a.codon[(size_t)a0 * CD_CELLS + (size_t)k], v); });
}

__global__ void __launch_bounds__(CD_BLOCK)
k_codon(CodonArgs a) {
    __shared__ uint32_t s_cell[CD_W * CD_CELLS];
    __shared__ StrandSeg s_seg[CD_BLOCK * CD_SLOTS];
    __shared__ int32_t s_lo[CD_BLOCK / 64], s_hi[CD_BLOCK / 64];
    __shared__ uint32_t s_nseg;
    const TallyReads &in = a.in;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < CD_W * CD_CELLS; k += CD_BLOCK) s_cell[k] = 0u;
    if (tid == 0) s_nseg = 0u;
    int64_t t0, t1;
    tally_tile_range(in.n, CD_BLOCK, t0, t1);
    CodonWindow win_at = codon_window_none();
    int since = 0;                             // tiles since the last flush
    uint32_t n_tallied = 0u, n_skipped = 0u;   // this lane's reads
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * CD_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        CodonShape sh = {false, 0, 0};
        const bool live = tally_live(in, i);
        if (live) {
            tally_counted_read(in, i, R, qual0);
            sh = codon_segments(R, in.P, qual0, [](const StrandSeg &) {});
            if (sh.regular) ++n_tallied; else ++n_skipped;
        }
        int32_t lo = sh.regular ? R.pos : SPAN_NO_LO, hi = sh.regular ? sh.ref_end : SPAN_NO_HI;
        block_span<CD_BLOCK>(lo, hi, s_lo, s_hi);
        if (!codon_window_keeps(win_at, lo, hi) || since >= CD_MAX_TILES_PER_FLUSH) {         // (the same for every lane)
            codon_flush(s_cell, win_at.a0, a);
            if (lo <= hi) win_at = codon_window_at(a.starts, a.n_slots, lo);                  // (every lane searches: the same loads)
            since = 0;
            __syncthreads();
        }
        ++since;
        const bool win = live && codon_read_windowed(sh, R.pos, win_at);
        if (win && sh.n_seg > 0) {
            uint32_t slot = atomicAdd(&s_nseg, (uint32_t)sh.n_seg);        // (at most CD_SLOTS per read: the list cannot overflow)
            codon_segments(R, in.P, qual0, [&](const StrandSeg &s) { s_seg[slot++] = s; });
        }
        __syncthreads();
        // ---- phase B: slot-major over the tile's list; lane `lane` of the wave owns slot a0 + c * 64 + lane of chunk c
        const uint32_t ns = s_nseg;
        for (int c = wave; c < CD_W / CD_CHUNK; c += CD_BLOCK / 64) {
            const int64_t first = (int64_t)win_at.a0 + c * CD_CHUNK;       // (wave-uniform)
            if (ns == 0u || first >= (int64_t)a.n_slots) continue;
            const int32_t mine_slot = (int32_t)first + lane;
            const bool owns = mine_slot < a.n_slots;
            const int32_t p = owns ? a.starts[mine_slot] : 0x7FFFFFFF;
            const int32_t c_lo = a.starts[first];
            const int32_t c_hi = a.starts[min((int64_t)a.n_slots - 1, first + CD_CHUNK - 1)];      // the chunk's starts lie in [c_lo, c_hi]
            uint32_t *my = s_cell + (size_t)(c * CD_CHUNK + lane) * CD_CELLS;
            for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                    // (ns is block-uniform: whole waves at the ballots)
                bool have;
                const StrandSeg mine = seg_take(s_seg, s0, ns, lane, have);
                unsigned long long hits = __ballot(have && (int64_t)mine.r0 <= (int64_t)c_hi && (int64_t)mine.r0 + st_seg_len(mine) > (int64_t)c_lo);
                // CD_UNROLL entries at a time: first the loads of all of them (a hit costs one trip to memory, and the trips
                // of one group overlap), then the adds
                while (hits) {
                    uint32_t what[CD_UNROLL], quals[CD_UNROLL], codes[CD_UNROLL];         // what: 0 nothing, 1 broken, 2 a triplet
#pragma unroll
                    for (int u = 0; u < CD_UNROLL; ++u) {
                        what[u] = 0u; quals[u] = 0u; codes[u] = 0u;
                        if (!hits) continue;                                   // (wave-uniform)
                        const int src = __ffsll((long long)hits) - 1;
                        hits &= hits - 1ull;
                        const StrandSeg g = seg_from(mine, src);
                        if (owns && p >= g.r0 && (int64_t)p < (int64_t)g.r0 + st_seg_len(g)) {
                            if (cd_seg_break(g)) {
                                what[u] = 1u;
                            } else {
                                const uint64_t k = g.q0 + (uint64_t)(p - g.r0);
                                what[u] = 2u; quals[u] = codon_load_quals(in.qual, k); codes[u] = codon_load_codes(in.seq, k);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < CD_UNROLL; ++u) {
                        uint32_t cell = (uint32_t)CD_BROKEN;
                        if (what[u] == 1u || (what[u] == 2u && codon_cell_of(quals[u], codes[u], in.P.min_quality, cell))) my[cell] += 1u;
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_nseg = 0u;
        // ---- the serial path: reads the window did not take
        if (live && !win && sh.regular) {
            const int32_t a0 = win_at.a0;
            codon_read(R, in.P, in.seq, in.qual, qual0, a.starts, a.n_slots, [&](int32_t s, uint32_t cell) {
                const int64_t w = (int64_t)s - (int64_t)a0;
                if (w >= 0 && w < CD_W) atomicAdd(&s_cell[(size_t)w * CD_CELLS + cell], 1u);
                else atomicAdd(&a.codon[(size_t)s * CD_CELLS + cell], 1u);
            });
        }
        __syncthreads();
    }
    codon_flush(s_cell, win_at.a0, a);
    tally_wave_add2(a.reads, n_tallied, n_skipped);            // the block's reads
}

static CodonState *codon_state(amp_ctx *c) { return hook_state<CodonState>(c, HOOK_CODON); }

static int codon_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    CodonState *s = codon_state(c);
    // (a block's window is flushed when it moves, not per tile)
    return hook_launch(q, s, codon_hook, rd->n_reads, o, CD_BLOCK, CD_TILES_PER_BLOCK, CD_BLOCKS_PER_CU, [&](unsigned grid) {
        k_codon<<<grid, CD_BLOCK, 0, q.stream>>>(CodonArgs{tally_reads(q, rd, o), s->n_slots, s->d_starts, s->d_codon, s->d_reads});
    });
}

HookOps codon_hook = {"the codon tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, codon_enqueue, hook_free<CodonState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_codon_enable(amp_ctx *c, int32_t n_slots, const int32_t *starts) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_CODON);
    if (n_slots == 0 || !starts) { slot.on = false; return AMP_OK; }
    if (n_slots < 0 || (int64_t)n_slots > CD_MAX_SLOTS) {
        snprintf(q.err, q.err_cap, "the codon slots: %d, not in [1, %lld]", n_slots, (long long)CD_MAX_SLOTS);
        return AMP_EINVAL;
    }
    const size_t N = (size_t)n_slots;
    for (size_t k = 0; k < N; ++k) {
        if (starts[k] < 0 || (int64_t)starts[k] + 3 > (int64_t)q.ref_len || (k && starts[k] <= starts[k - 1])) {
            snprintf(q.err, q.err_cap, "codon slot %zu: start %d is not above the one before it, or the codon reaches past the reference", k, starts[k]);
            return AMP_EINVAL;
        }
    }
    Guard g(q.device);
    CodonState *s = codon_state(c);
    if (s && (s->n_slots != n_slots || memcmp(s->starts.data(), starts, N * 4) != 0)) {
        // another set: the tables are laid out again (a kernel of the old one may still be in flight)
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        hook_free<CodonState>(s);
        s = nullptr; slot.state = nullptr; slot.on = false;
    }
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, codon_hook, s, [&](CodonState &f) -> int {
            f.n_slots = n_slots;
            f.starts.assign(starts, starts + N);
            HOOKTRY(hook_alloc(q, f, &f.d_starts, N * 4));
            HOOKTRY(hook_alloc(q, f, &f.d_codon, N * CD_CELLS * 4, N * CD_CELLS * 4));
            HOOKTRY(hook_alloc(q, f, &f.d_reads, 16, 16));
            hook_table(f, f.d_codon, N * CD_CELLS);
            hook_table(f, f.d_reads, 2);
            HOOKCHK(q, hipMemcpyAsync(f.d_starts, f.starts.data(), N * 4, hipMemcpyHostToDevice, q.stream));
            HOOKCHK(q, hipStreamSynchronize(q.stream));
            return AMP_OK;
        }));
    }
    slot.on = false;
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_codon_get(amp_ctx *c, uint32_t *codon, uint64_t *reads) { return hook_get(c, HOOK_CODON, {codon, reads}); }

int amp_codon_add(amp_ctx *c, const uint32_t *codon, const uint64_t *reads) { return hook_add_tables(c, HOOK_CODON, {codon, reads}); }

int amp_codon_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_CODON, ms); }

}  // extern "C"
