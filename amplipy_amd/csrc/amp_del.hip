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
#include <stdio.h>

#include "amp_del.hpp"
#include "amp_hook.hpp"
#include "amp_strand.hpp"
#include "amp_tally.hpp"

namespace amp {

using DelTable = KeyedTable<unsigned long long, 1>;     // the global table (amp_keyed.hpp): a key is one word, DL_EMPTY: free

struct DelState : HookState {
    DelTable t = {nullptr, nullptr, nullptr, 0u};
};

struct DelArgs {
    TallyReads in;
    DelTable t;
};

// (key, count, rev) into the global table: 64-bit compare-and-swap on the key, then the adds (agent scope: HIP's default)
__device__ __forceinline__ void del_global_insert(const DelTable &t, uint64_t key, uint32_t count, uint32_t rev) {
    bool fresh = false;
    const int64_t s = del_probe(key, del_slot_global(key, t.log2_capacity), (1u << t.log2_capacity) - 1u, del_probes_global(t.log2_capacity), [&](uint32_t slot) {
        const uint64_t prev = atomicCAS(&t.keys[slot], (unsigned long long)DL_EMPTY, (unsigned long long)key);
        fresh = prev == DL_EMPTY;
        return prev;
    });
    keyed_tally(t, s, fresh, count, rev);
}

// What amp_keyed.hpp is told about the table
struct DelKeys {
    using Word = unsigned long long;
    using Entry = amp_del_event;
    using Table = DelTable;
    static constexpr int WORDS = 1, LOG2_MIN = DL_LOG2_MIN, LOG2_MAX = DL_LOG2_MAX, LOG2_DEFAULT = DL_LOG2_DEFAULT;
    static constexpr const char *NOUN = "the deletion events' table";
    static __device__ void insert(const Table &t, const Entry &e) { del_global_insert(t, del_key(e.start, e.len), e.count, e.rev); }
    static __device__ void to_entry(const Table &t, uint64_t s, Entry &e) { e = Entry{del_key_start(t.keys[s]), del_key_len(t.keys[s]), t.cnt[2 * s], t.cnt[2 * s + 1]}; }
    static __host__ __device__ bool whole(const Word *key) { return key[0] != DL_EMPTY; }
    static bool less(const Entry &x, const Entry &y) { return x.start != y.start ? x.start < y.start : x.len < y.len; }
    static bool check(const Entry &e, long long k, char *err, size_t cap) {
        if (e.start >= 0 && e.len >= 1) return true;
        snprintf(err, cap, "deletion event %lld: start %d, length %d", k, e.start, e.len);
        return false;
    }
};

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
            uint64_t lk = 0ull;                 // the leader's key, in every lane
            const auto same_key = [&](int src) {
                lk = (uint64_t)__shfl((unsigned long long)key, src);
                return have && key == lk;
            };
            wave_each_distinct(have, same_key, [&](int src, unsigned long long same) {
                if (lane == src) del_lds_insert(s_key, s_cnt, &s_used, a.t, lk, (uint32_t)__popcll(same), (uint32_t)__popcll(same & revs));
            });
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

static DelState *del_state(amp_ctx *c) { return hook_state<DelState>(c, HOOK_DEL); }

static int del_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    DelState *s = del_state(c);
    return hook_launch(q, s, del_hook, rd->n_reads, o, DL_BLOCK, DL_TILES_PER_BLOCK, DL_BLOCKS_PER_CU, [&](unsigned grid) {
        k_del<<<grid, DL_BLOCK, 0, q.stream>>>(DelArgs{tally_reads(q, rd, o), s->t});
    });
}

HookOps del_hook = {"the deletion events need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, del_enqueue, hook_free<DelState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_del_enable(amp_ctx *c, int on, int log2_capacity) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_DEL);
    if (!on) { slot.on = false; return AMP_OK; }
    HOOKTRY(keyed_capacity<DelKeys>(q, log2_capacity));
    Guard g(q.device);
    DelState *s = del_state(c);
    const auto layout = [&](DelState &f) -> int { return keyed_layout(q, f, f.t, (uint32_t)log2_capacity); };
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, del_hook, s, layout));
    } else if (s->t.log2_capacity != (uint32_t)log2_capacity) {
        HOOKTRY(keyed_relayout(q, slot, *s, layout));
    }
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_del_get(amp_ctx *c, amp_del_event *entries, int64_t cap, int64_t *n, amp_del_info *info) {
    if (!c || cap < 0) return AMP_EINVAL;
    DelState *s = del_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    return keyed_get<DelKeys>(ctx_hook(c), s->t, entries, cap, n, info);
}

int amp_del_add(amp_ctx *c, const amp_del_event *entries, int64_t n) {
    if (!c || n < 0 || (n && !entries)) return AMP_EINVAL;
    DelState *s = del_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    return keyed_add(ctx_hook(c), s->t, DelKeys{}, entries, n);
}

int amp_del_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_DEL, ms); }

}  // extern "C"
