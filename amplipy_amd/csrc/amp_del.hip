// amp_del.hip -- deletion events tallied on the device (C ABI: the amp_del_* entry points of amplihip.h).
//
// k_del runs behind the read pass of every batch while the hook is on.  It has the tally skeleton's outer shape (amp_tally.hpp:
// 256-lane blocks over contiguous runs of 256-read tiles, one lane per read in phase A) but its table is keyed, not positional:
// most reads have no event, and the usual case is a pile of thousands of reads that all carry the SAME event -- the worst case
// for an atomic per event.  So: phase A puts each read's events (del_events_regular: CIGAR words alone, no base or quality
// byte unless the read has an event, then one; every other read walks, del_events_walk) on the tile's list in LDS.  Phase B: a
// wave takes the list 64 entries at a time, an entry per lane, and combines equal keys by a ballot loop -- the leader's key
// is broadcast, the lanes that hold it are balloted, the leader adds both popcounts -- into the block's open-addressed table
// in LDS (64-bit key claimed by compare-and-swap, two u32 counts).  The block's table goes to the global table in HBM when
// the block ends and, at a tile boundary, once it is more than three quarters full; an insert that finds no slot within
// DL_LDS_PROBES goes straight to the global table, as does an event the list has no room for.  The global table persists
// across batches: nothing per read or per batch comes down.  Every probe loop is bounded (del_probe); an event that finds no
// slot in the global table adds its reads to `lost` and is dropped, never merged into another key.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "amp_del.hpp"
#include "amp_hook.hpp"
#include "amp_strand.hpp"
#include "amp_tally.hpp"

namespace amp {

struct DelTable {                               // the global table as a kernel is handed it
    unsigned long long *keys;                   // [capacity], DL_EMPTY: free
    uint32_t *cnt;                              // [capacity][2]: count, rev
    unsigned long long *info;                   // [2]: used slots, lost reads
    uint32_t log2_capacity;
};

struct DelState : HookState {
    DelTable t = {nullptr, nullptr, nullptr, 0u};      // keys, cnt and info are one allocation
};

struct DelArgs {
    TallyReads in;
    DelTable t;
};

// (key, count, rev) into the global table: 64-bit compare-and-swap on the key, then the adds (agent scope: HIP's default)
__device__ __forceinline__ void del_global_insert(const DelTable &t, uint64_t key, uint32_t count, uint32_t rev) {
    const int64_t s = del_probe(key, del_slot_global(key, t.log2_capacity), (1u << t.log2_capacity) - 1u, del_probes_global(t.log2_capacity), [&](uint32_t slot) {
        const uint64_t prev = atomicCAS(&t.keys[slot], (unsigned long long)DL_EMPTY, (unsigned long long)key);
        if (prev == DL_EMPTY) atomicAdd(&t.info[0], 1ull);
        return prev;
    });
    if (s < 0) { atomicAdd(&t.info[1], (unsigned long long)count); return; }
    atomicAdd(&t.cnt[2 * (size_t)s], count);
    if (rev) atomicAdd(&t.cnt[2 * (size_t)s + 1], rev);
}

// ... into the block's table, or past it when it has no slot within its probe count
__device__ __forceinline__ void del_lds_insert(unsigned long long *s_key, uint32_t *s_cnt, uint32_t *s_used, const DelTable &t, uint64_t key, uint32_t count,
                                               uint32_t rev) {
    const int64_t s = del_probe(key, del_slot_lds(key), (uint32_t)(DL_LDS_SLOTS - 1), (uint32_t)DL_LDS_PROBES, [&](uint32_t slot) {
        const uint64_t prev = atomicCAS(&s_key[slot], (unsigned long long)DL_EMPTY, (unsigned long long)key);
        if (prev == DL_EMPTY) atomicAdd(s_used, 1u);
        return prev;
    });
    if (s < 0) { del_global_insert(t, key, count, rev); return; }
    atomicAdd(&s_cnt[2 * s], count);
    if (rev) atomicAdd(&s_cnt[2 * s + 1], rev);
}

// the block's table to the global one; its slots are free afterwards
__device__ __forceinline__ void del_flush(unsigned long long *s_key, uint32_t *s_cnt, const DelTable &t) {
    for (int k = (int)threadIdx.x; k < DL_LDS_SLOTS; k += DL_BLOCK) {
        const uint64_t key = s_key[k];
        if (key == DL_EMPTY) continue;
        del_global_insert(t, key, s_cnt[2 * k], s_cnt[2 * k + 1]);
        s_key[k] = DL_EMPTY; s_cnt[2 * k] = 0u; s_cnt[2 * k + 1] = 0u;
    }
}

// The counted alignment of live read i, as tally_counted_read gives it, without its quality byte
__device__ __forceinline__ void del_counted_read(const TallyReads &in, int64_t i, StrandRead &R) {
    const uint32_t c0 = in.cig_off32[i];
    if (in.do_trim) {
        R.pos = in.new_pos[i]; R.cig = in.new_cig + (size_t)c0 + 3 * (size_t)i; R.n_ops = in.new_ncig[i];
    } else {
        R.pos = in.pos[i]; R.cig = in.cig + c0; R.n_ops = in.cig_off32[i + 1] - c0;
    }
    R.lseq = (int32_t)in.lseq[i];
    R.rev = (in.flag[i] & 0x10u) ? 1u : 0u;
    R.base = (uint64_t)in.seq_off8[i] * 8ull;
}

__global__ void __launch_bounds__(DL_BLOCK)
k_del(DelArgs a) {
    __shared__ unsigned long long s_key[DL_LDS_SLOTS];
    __shared__ uint32_t s_cnt[DL_LDS_SLOTS * 2];
    __shared__ unsigned long long s_list[DL_LIST];
    __shared__ uint32_t s_n[2];                 // entries asked for on the list, by the tile's parity (the other one is zeroed meanwhile)
    __shared__ uint32_t s_used;
    const TallyReads &in = a.in;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < DL_LDS_SLOTS; k += DL_BLOCK) { s_key[k] = DL_EMPTY; s_cnt[2 * k] = 0u; s_cnt[2 * k + 1] = 0u; }
    if (tid == 0) { s_n[0] = 0u; s_n[1] = 0u; s_used = 0u; }
    int64_t t0, t1;
    tally_tile_range(in.n, DL_BLOCK, t0, t1);
    int since = 0;                              // tiles since the last flush
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        const int par = (int)((t - t0) & 1);
        // ---- phase A: one lane per read; its events onto the tile's list
        const int64_t i = t * DL_BLOCK + tid;
        if (tally_live(in, i)) {
            StrandRead R;
            del_counted_read(in, i, R);
            auto put = [&](int32_t start, int32_t len) {
                const uint64_t key = del_key(start, len);
                const uint32_t slot = atomicAdd(&s_n[par], 1u);
                if (slot < (uint32_t)DL_LIST) s_list[slot] = key | (R.rev ? DL_REV_BIT : 0ull);
                else del_global_insert(a.t, key, 1u, R.rev);
            };
            int32_t n_ev = 0;
            StrandShape sh = del_events_regular(R, in.P, [&](int32_t, int32_t) { ++n_ev; });
            if (del_qual_needed(sh, n_ev) && in.qual[R.base] == 0xFFu) sh.regular = false;
            if (!sh.regular) del_events_walk(R, in.P, in.seq, in.qual, put);       // the serial path: irregular reads walk in their lane
            else if (n_ev > 0) del_events_regular(R, in.P, put);
        }
        __syncthreads();
        // ---- phase B: equal keys of a wave's 64 entries combined, the leaders into the block's table
        if (tid == 0) s_n[par ^ 1] = 0u;
        const uint32_t ns = min(s_n[par], (uint32_t)DL_LIST);
        for (uint32_t s0 = (uint32_t)wave * 64u; s0 < ns; s0 += (uint32_t)DL_BLOCK) {      // (wave-uniform: whole waves at the ballots)
            const bool have = s0 + (uint32_t)lane < ns;
            const uint64_t e = have ? (uint64_t)s_list[s0 + (uint32_t)lane] : 0ull;
            const uint64_t key = e & ~DL_REV_BIT;
            const unsigned long long revs = __ballot(have && (e & DL_REV_BIT) != 0ull);
            unsigned long long pending = __ballot(have);
            while (pending) {
                const int src = __ffsll((long long)pending) - 1;
                const uint64_t lk = (uint64_t)__shfl((unsigned long long)key, src);
                const unsigned long long same = __ballot(have && key == lk);
                if (lane == src) del_lds_insert(s_key, s_cnt, &s_used, a.t, lk, (uint32_t)__popcll(same), (uint32_t)__popcll(same & revs));
                pending &= ~same;
            }
        }
        __syncthreads();
        // ---- the tile boundary (s_used changes in phase B and below only: every lane reads the same value here)
        ++since;
        if (s_used > (uint32_t)DL_LDS_FLUSH_AT || since >= DL_MAX_TILES_PER_FLUSH) {
            del_flush(s_key, s_cnt, a.t);
            since = 0;
            __syncthreads();
            if (tid == 0) s_used = 0u;          // (behind the barrier: every lane has read it; the next change is behind the next one)
        }
    }
    del_flush(s_key, s_cnt, a.t);
}

// host entries through the same insert path
__global__ void k_del_add(DelTable t, const amp_del_event *ev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const amp_del_event e = ev[i];
    del_global_insert(t, del_key(e.start, e.len), e.count, e.rev);
}

// the used slots, in no order
__global__ void k_del_compact(DelTable t, amp_del_event *out, unsigned long long *n_out, uint64_t cap_out) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1ull << t.log2_capacity)) return;
    const uint64_t key = t.keys[s];
    if (key == DL_EMPTY) return;
    const uint64_t at = atomicAdd(n_out, 1ull);
    if (at < cap_out) out[at] = amp_del_event{del_key_start(key), del_key_len(key), t.cnt[2 * s], t.cnt[2 * s + 1]};
}

static size_t del_bytes(uint32_t log2_capacity) { return ((size_t)16 << log2_capacity) + 64; }      // keys, counts, info (and the compaction's counter)

static DelState *del_state(amp_ctx *c) { return hook_state<DelState>(c, HOOK_DEL); }

static void del_free(void *state) {
    DelState *s = hook_state_of<DelState>(state);
    if (!s) return;
    if (s->t.keys) (void)hipFree(s->t.keys);
    s->timer.destroy();
    delete s;
}

static int del_layout(const HookCtx &q, DelTable &t, uint32_t log2_capacity) {
    if (t.keys) (void)hipFree(t.keys);
    t = DelTable{nullptr, nullptr, nullptr, 0u};
    void *p = nullptr;
    HOOKCHK(q, hipMalloc(&p, del_bytes(log2_capacity)));
    const size_t cap = (size_t)1 << log2_capacity;
    t.keys = (unsigned long long *)p;
    t.cnt = (uint32_t *)(t.keys + cap);
    t.info = t.keys + 2 * cap;
    t.log2_capacity = log2_capacity;
    return AMP_OK;
}

static int del_zero(const HookCtx &q, const DelTable &t) {
    const size_t cap = (size_t)1 << t.log2_capacity;
    HOOKCHK(q, hipMemsetAsync(t.keys, 0xFF, cap * 8, q.stream));
    HOOKCHK(q, hipMemsetAsync(t.cnt, 0, cap * 8 + 64, q.stream));
    return AMP_OK;
}

static int del_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    DelState *s = del_state(c);
    return hook_launch(q, s, del_hook, rd->n_reads, o, DL_BLOCK, DL_TILES_PER_BLOCK, DL_BLOCKS_PER_CU, [&](unsigned grid) {
        k_del<<<grid, DL_BLOCK, 0, q.stream>>>(DelArgs{tally_reads(q, rd, o), s->t});
    });
}

static int del_reset(amp_ctx *c) { return del_state(c)->t.keys ? del_zero(ctx_hook(c), del_state(c)->t) : AMP_OK; }

HookOps del_hook = {"the deletion events need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, del_enqueue, del_reset, del_free};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_del_enable(amp_ctx *c, int on, int log2_capacity) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_DEL);
    if (!on) { slot.on = false; return AMP_OK; }
    if (log2_capacity == 0) log2_capacity = DL_LOG2_DEFAULT;
    if (log2_capacity < DL_LOG2_MIN || log2_capacity > DL_LOG2_MAX) {
        snprintf(q.err, q.err_cap, "the deletion events' table takes 2^%d to 2^%d slots (0: the default, 2^%d)", DL_LOG2_MIN, DL_LOG2_MAX, DL_LOG2_DEFAULT);
        return AMP_EINVAL;
    }
    Guard g(q.device);
    DelState *s = del_state(c);
    if (!s) {
        const int rc = hook_new_state(q, slot, del_hook, s, [&](DelState &f) -> int { return del_layout(q, f.t, (uint32_t)log2_capacity); });
        if (rc != AMP_OK) return rc;
    } else if (s->t.log2_capacity != (uint32_t)log2_capacity) {
        slot.on = false;
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        const int rc = del_layout(q, s->t, (uint32_t)log2_capacity);
        if (rc != AMP_OK) return rc;
    }
    const int rc = del_zero(q, s->t);
    if (rc != AMP_OK) return rc;
    slot.on = true;
    return AMP_OK;
}

int amp_del_get(amp_ctx *c, amp_del_event *entries, int64_t cap, int64_t *n, amp_del_info *info) {
    if (!c || cap < 0) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    DelState *s = del_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    Guard g(q.device);
    unsigned long long h[2] = {0ull, 0ull};
    HOOKCHK(q, hipMemcpyAsync(h, s->t.info, sizeof(h), hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    if (info) { info->used = h[0]; info->capacity = 1ull << s->t.log2_capacity; info->lost = h[1]; }
    if (n) *n = (int64_t)h[0];
    if ((uint64_t)cap < h[0] || (h[0] && !entries)) {
        snprintf(q.err, q.err_cap, "the deletion events' table holds %llu entries, the array given %lld", h[0], (long long)cap);
        return AMP_EINVAL;
    }
    if (!h[0]) return AMP_OK;
    amp_del_event *d_out = nullptr;
    HOOKCHK(q, hipMalloc((void **)&d_out, (size_t)h[0] * sizeof(amp_del_event)));
    unsigned long long *d_n = s->t.info + 2;                       // (inside the allocation's last 64 bytes)
    const int rc = [&]() -> int {
        HOOKCHK(q, hipMemsetAsync(d_n, 0, 8, q.stream));
        const uint64_t slots = 1ull << s->t.log2_capacity;
        k_del_compact<<<(unsigned)((slots + 255) / 256), 256, 0, q.stream>>>(s->t, d_out, d_n, h[0]);
        HOOKCHK(q, hipGetLastError());
        HOOKCHK(q, hipMemcpyAsync(entries, d_out, (size_t)h[0] * sizeof(amp_del_event), hipMemcpyDeviceToHost, q.stream));
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        return AMP_OK;
    }();
    (void)hipFree(d_out);
    if (rc != AMP_OK) return rc;
    std::sort(entries, entries + h[0], [](const amp_del_event &x, const amp_del_event &y) { return x.start != y.start ? x.start < y.start : x.len < y.len; });
    return AMP_OK;
}

int amp_del_add(amp_ctx *c, const amp_del_event *entries, int64_t n) {
    if (!c || n < 0 || (n && !entries)) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    DelState *s = del_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    if (!n) return AMP_OK;
    for (int64_t k = 0; k < n; ++k) {
        if (entries[k].start < 0 || entries[k].len < 1) {
            snprintf(q.err, q.err_cap, "deletion event %lld: start %d, length %d", (long long)k, entries[k].start, entries[k].len);
            return AMP_EINVAL;
        }
    }
    Guard g(q.device);
    amp_del_event *d_in = nullptr;
    HOOKCHK(q, hipMalloc((void **)&d_in, (size_t)n * sizeof(amp_del_event)));
    const int rc = [&]() -> int {
        HOOKCHK(q, hipMemcpyAsync(d_in, entries, (size_t)n * sizeof(amp_del_event), hipMemcpyHostToDevice, q.stream));
        k_del_add<<<(unsigned)((n + 255) / 256), 256, 0, q.stream>>>(s->t, d_in, n);
        HOOKCHK(q, hipGetLastError());
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        return AMP_OK;
    }();
    (void)hipFree(d_in);
    return rc;
}

int amp_del_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_DEL, ms); }

}  // extern "C"
