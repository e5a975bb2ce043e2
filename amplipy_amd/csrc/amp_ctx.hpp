// amp_ctx.hpp -- the context behind the C ABI (include/amplihip.h), private to the two units that see inside it:
// amplihip.hip (create, destroy, setters, everything but the read pass) and amp_readpass.hip (launch_reads and the read
// kernels).  Every other unit goes through the accessors ctx_stream / ctx_device (amp_codec.hpp) and ctx_hook / hook_slot
// (amp_hook.hpp) and does not include this header.  -DAMP_DEV changes the struct: both units are built with the same defines.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/amplihip.h"
#include "amp_read.hpp"      // CTR_*, EV_SHARDS, KParams
#include "amp_hook.hpp"      // HookSlot, Guard, AMP_HIPCHK

// A device buffer that grows and is released with its owner.
struct DBuf {
    void *p = nullptr;
    size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    ~DBuf() { release(); }      // (the owner makes the device current: amp_ctx_destroy)
    hipError_t ensure(size_t bytes, bool keep = false, hipStream_t s = nullptr) {
        if (bytes <= cap) return hipSuccess;
        size_t ncap = std::max(bytes, cap + cap / 2);
        void *np = nullptr;
        hipError_t e = hipMalloc(&np, ncap);
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        if (p) (void)hipFree(p);
        p = np; cap = ncap;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

struct amp_ctx {
    int device = 0;
    int32_t ref_len = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t *d_counts = nullptr;
    bool own_counts = false;
    int32_t *d_min_start = nullptr, *d_max_end = nullptr;
    int32_t max_primer_len = 0;
    bool have_primers = false;
    int32_t min_quality = 20, window = 4, do_trim = 1, do_count = 1;
    // insertion events
    DBuf events;                  // amp_ins_event[EV_SHARDS][ev_cap]
    int64_t ev_cap = 0;           // per shard
    bool ev_reserved = false;     // caller sized the buffer: skip the bound pre-pass
    unsigned long long *d_ctr = nullptr;  // [CTR_WORDS] device counters (the enum next to EventBuf, amp_read.hpp)
    uint32_t *d_ins_at = nullptr;         // [ref_len] insertion events per reference position
    uint8_t *d_ref = nullptr;             // [ref_len] reference sequence, ASCII (amp_set_reference)
    bool have_ref = false;
    // staging for the host-pointer path
    DBuf s_pos, s_flag, s_tlen, s_lseq, s_cigoff, s_cig, s_seqoff, s_seq, s_qual;
    int64_t staged_n = -1, staged_ncig = 0, staged_nbases = 0;     // the batch of the last amp_process_batch, still in the buffers above
    DBuf o_pos, o_ncig, o_cig, o_reflen, o_flags, o_status;
    DBuf scratch;                 // CIGAR scratch for reads whose ops do not fit the LDS slots
    DBuf call_buf;
    DBuf call_sync;                // k_call_fused's ticket and flags (zero between launches)
    DBuf agg_buf;                  // amp_aggregate_ins_events: run records + the sort's scratch
    void *h_pin = nullptr; size_t h_pin_cap = 0;   // pinned staging for call results (amp_call_compact_begin: written by the kernel itself)
    std::vector<uint8_t> h_img; bool img_pinned = false;   // ... and the pageable image of a view that was not begun (one copy)
    bool call_pending = false;     // amp_call_compact_begin has enqueued the calling kernels; amp_call_compact_view picks them up
    amp_call_params call_pending_params{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr, ev_call = nullptr;
    bool timed = false;
    bool last_split = false;      // the last launch recorded ev1 / ev2
    int last_kv = 0;              // kernel variant the last batch took (amp_last_kernel_variant)
    bool split_timing = false;    // also time the first kernel of a pass alone (amp_set_timing): costs an idle gap behind it
    int n_cu = 256;
    int cu_share = 1;              // the fast kernels of this ctx are sized for n_cu / cu_share CUs (amp_set_cu_share)
    uint32_t epoch = 0;            // launches of the read kernels so far (KParams::epoch)
    // What the last finished pass of variant 4 left for its second kernels, written by k_deferred_heavy into pinned host memory
    // (no copy, no wait): [0] = epoch << 32 | heavy entries, [1] = epoch << 32 | reads on the general list.  launch_reads sizes
    // the next pass's second kernels by it (ReadPlan::gen_blocks / heavy_blocks) when both words carry one epoch, not older than
    // hist_from (the setters of the plan's inputs and every pass of another variant move it past the passes launched so far).
    unsigned long long *h_hist = nullptr;
    uint32_t hist_from = 1;
    int force_gen_blocks = 0, force_heavy_blocks = 0;      // amp_debug_second_grids: 0 = by the plan
    int last_gen_blocks = 0, last_heavy_blocks = 0;        // what the last pass of variant 4 was launched with (amp_debug_last_second_grids)
    // amp_set_kernel_variant: 0 = by the batch (route_variant, amp_plan.hpp), 1 = one lane per read (the reference kernel),
    // 2 = fused tile kernel, 3 = split pipeline (k_trim + k_scan + k_tile<SPLIT>), 4 / 5 / 6 / 7 = a fast kernel (k_fast, k_fast5,
    // k_fast6, k_fast7: the four generations) + the general pass (k_tile<LIST> over the other reads)
    int kernel_variant = 0;
    uint32_t *dbg_dcnt = nullptr; int dbg_grid = 0;
    amp::HookSlot hooks[amp::N_HOOKS] = {};  // the opt-in kernels behind the read pass (amp_hook.hpp): a hook that is on costs one more kernel per batch
    uint32_t phases = 0xFFu;       // always 0xFF in the shipped library; -DAMP_DEV builds can mask phases of the tile kernel (AMPLIHIP_PHASES)
    char err[320] = {0};
};

#define HIPCHK(ctx, call) AMP_HIPCHK((ctx)->err, sizeof((ctx)->err), #call, call)

// The batch of the last amp_process_batch call: its device copy is still in the ctx's staging buffers.
inline amp_dev_reads staged_reads(const amp_ctx *c) {
    return amp_dev_reads{c->staged_n, c->s_pos.as<int32_t>(), c->s_flag.as<uint16_t>(), c->s_tlen.as<int32_t>(), c->s_lseq.as<uint32_t>(),
                         c->s_cigoff.as<uint32_t>(), c->s_cig.as<uint32_t>(), c->s_seqoff.as<uint32_t>(), c->s_seq.as<uint8_t>(),
                         c->s_qual.as<uint8_t>(), c->staged_ncig, c->staged_nbases};
}

// what crosses the boundary between the two units
namespace amp {
// amplihip.hip: re-lays the event list's shard regions out for a larger capacity per shard
hipError_t grow_events(amp_ctx *c, int64_t ncap);
// amp_readpass.hip: the read kernels for a device-resident batch, on the ctx stream
int launch_reads(amp_ctx *c, const amp_dev_reads *rd, uint64_t read_base, const amp_trim_out *o);
}  // namespace amp
