// amp_readpos.hip -- read-position tallies per allele on the device (C ABI: the amp_readpos_* entry
// points of amplihip.h).
//
// k_readpos runs behind the read pass of every batch while the tallies are on and touches every counted base once more, in the
// shape of amp_tally.hpp and of k_strand: segments per read in phase A (readpos_segments, amp_readpos.hpp), position-major adds
// in phase B.  The loop is k_strand's, tally_poswin of amp_tally.hpp, on ReadposTally of amp_readpos.hpp: a window position has 42 cells (six columns of seven distance bins), kept two to a word as 16-bit
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
    ReadposTally::Out out;
};

__global__ void __launch_bounds__(RP_BLOCK)
k_readpos(ReadposArgs a) { tally_poswin<ReadposTally>(a.in, a.out); }

static ReadposState *readpos_state(amp_ctx *c) { return hook_state<ReadposState>(c, HOOK_READPOS); }

static int readpos_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    ReadposState *s = readpos_state(c);
    return hook_launch(q, s, readpos_hook, rd->n_reads, o, RP_BLOCK, RP_TILES_PER_BLOCK, RP_BLOCKS_PER_CU, [&](unsigned grid) {
        k_readpos<<<grid, RP_BLOCK, 0, q.stream>>>(ReadposArgs{tally_reads(q, rd, o), {s->d_hist}});
    });
}

HookOps readpos_hook = {"the read-position tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, readpos_enqueue, hook_free<ReadposState>};

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
        HOOKTRY(hook_new_state(q, slot, readpos_hook, s, [&](ReadposState &f) -> int {
            const size_t cells = (size_t)q.ref_len * RP_CELLS;
            HOOKTRY(hook_alloc(q, f, &f.d_hist, std::max<size_t>(cells * 4, 64), cells * 4));
            hook_table(f, f.d_hist, cells);
            return AMP_OK;
        }));
    }
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_readpos_get(amp_ctx *c, uint32_t *hist) { return hook_get(c, HOOK_READPOS, {hist}); }

int amp_readpos_add(amp_ctx *c, const uint32_t *hist) { return hook_add_tables(c, HOOK_READPOS, {hist}); }

int amp_readpos_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_READPOS, ms); }

}  // extern "C"
