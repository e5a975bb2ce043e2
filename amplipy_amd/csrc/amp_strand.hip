// amp_strand.hip -- per-allele strand and base-quality tallies on the device (C ABI: the amp_strand_*
// entry points of amplihip.h).
//
// k_strand runs behind the read pass of every batch while the tallies are on and touches every counted base a second time.
// The normal input is a coordinate-sorted pile of thousands of reads on one amplicon, so lanes that walked neighbouring reads
// base by base would add onto the same few addresses in lock-step.  The kernel turns the work round instead, in the shape of
// amp_tally.hpp: segments per read in phase A (strand_segments, amp_strand.hpp), position-major adds in phase B.  The loop is
// tally_poswin of amp_tally.hpp, shared with k_readpos, on StrandTally of amp_strand.hpp: the block keeps a window of ST_W reference positions x 11 u32 cells in LDS; each wave owns every fourth 64-position
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
    StrandTally::Out out;
};

__global__ void __launch_bounds__(ST_BLOCK)
k_strand(StrandArgs a) { tally_poswin<StrandTally>(a.in, a.out); }

static StrandState *strand_state(amp_ctx *c) { return hook_state<StrandState>(c, HOOK_STRAND); }

static int strand_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    StrandState *s = strand_state(c);
    // (a block's window is flushed when it moves, not per tile)
    return hook_launch(q, s, strand_hook, rd->n_reads, o, ST_BLOCK, ST_TILES_PER_BLOCK, ST_BLOCKS_PER_CU, [&](unsigned grid) {
        k_strand<<<grid, ST_BLOCK, 0, q.stream>>>(StrandArgs{tally_reads(q, rd, o), {s->d_rev, s->d_qsum}});
    });
}

HookOps strand_hook = {"the strand tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, strand_enqueue, hook_free<StrandState>};

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
        HOOKTRY(hook_new_state(q, slot, strand_hook, s, [&](StrandState &f) -> int {
            const size_t G = (size_t)q.ref_len;
            HOOKTRY(hook_alloc(q, f, &f.d_qsum, std::max<size_t>(G * 64, 64), G * 64));
            f.d_rev = (uint32_t *)(f.d_qsum + G * ST_QSUM_COLS);
            hook_table(f, f.d_rev, G * ST_REV_COLS);
            hook_table(f, f.d_qsum, G * ST_QSUM_COLS);
            return AMP_OK;
        }));
    }
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_strand_get(amp_ctx *c, uint32_t *rev, uint64_t *qsum) { return hook_get(c, HOOK_STRAND, {rev, qsum}); }

int amp_strand_add(amp_ctx *c, const uint32_t *rev, const uint64_t *qsum) { return hook_add_tables(c, HOOK_STRAND, {rev, qsum}); }

int amp_strand_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_STRAND, ms); }

}  // extern "C"
