// amp_keyed.hpp -- the keyed table in HBM that the deletion events (amp_del.hip), the insertion evidence (amp_insev.hip) and the
// read haplotypes (amp_hap.hip) tally into: open addressing, linear probing, a bounded probe count.  One
// allocation: keys[capacity] of N words of type W (all ones: free), then cnt[capacity][2] (count, rev), then info[2] (used slots,
// lost reads), then the rest of a 64-byte tail, where the compaction keeps its counter.  Which slot a hash starts at and how
// many slots an insert tries are plain functions (the hostsim twins call them); the table, its layout, the two helper kernels,
// the host side of get and add and the way to another capacity are written once over a unit's traits type T:
//   Word, WORDS, Entry (of the ABI)     Table: what the kernels are handed -- KeyedTable<Word, WORDS>, or a struct that derives from
//   it and adds what a slot carries beside (count, rev)                          whole(key): the slot holds all of a key
//   insert(table, entry): the unit's device insert of a host entry     to_entry(table, slot, entry): a used slot into a zeroed entry
//   less(entry, entry): the order get returns       check(entry, k, err, cap): a host entry of add, false with its message
//   NOUN, LOG2_MIN, LOG2_MAX, LOG2_DEFAULT
// The probe loops stay with their units: del_probe claims a key with one 64-bit compare-and-swap, hap_probe and insev_probe
// word by word.
#pragma once

#include <stdint.h>

#include "amp_strand.hpp"

namespace amp {

constexpr int KEYED_PROBES = 4096;           // slots an insert tries (all of a smaller table); then its reads are lost
AMP_ST_HD uint32_t keyed_slot(uint64_t hash, uint32_t log2_capacity) { return (uint32_t)(hash >> 32) & ((1u << log2_capacity) - 1u); }
AMP_ST_HD uint32_t keyed_probes(uint32_t log2_capacity) { return log2_capacity < 12u ? (1u << log2_capacity) : (uint32_t)KEYED_PROBES; }

}  // namespace amp

#ifdef __HIPCC__
#include <algorithm>

#include "amp_hook.hpp"

namespace amp {

template <class W, int N>
struct KeyedTable {                             // the table as a kernel is handed it
    W *keys;                                    // [capacity][N]
    uint32_t *cnt;                              // [capacity][2]: count, rev
    unsigned long long *info;                   // [2]: used slots, lost reads
    uint32_t log2_capacity;
};

// The end of an insert into the table: s is the key's slot (fresh: this insert took it), or negative when it found none
template <class W, int N>
__device__ __forceinline__ void keyed_tally(const KeyedTable<W, N> &t, int64_t s, bool fresh, uint32_t count, uint32_t rev) {
    if (s < 0) { atomicAdd(&t.info[1], (unsigned long long)count); return; }
    if (fresh) atomicAdd(&t.info[0], 1ull);
    atomicAdd(&t.cnt[2 * (size_t)s], count);
    if (rev) atomicAdd(&t.cnt[2 * (size_t)s + 1], rev);
}

// host entries through the unit's insert path
template <class T>
__global__ void k_keyed_add(typename T::Table t, const typename T::Entry *ev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) T::insert(t, ev[i]);
}

// the used slots, in no order, into a zeroed array (the unit fills an entry field by field: its padding stays zero)
template <class T>
__global__ void k_keyed_compact(typename T::Table t, typename T::Entry *out, unsigned long long *n_out, uint64_t cap_out) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1ull << t.log2_capacity)) return;
    if (!T::whole(t.keys + (size_t)s * T::WORDS)) return;
    const uint64_t at = atomicAdd(n_out, 1ull);
    if (at < cap_out) T::to_entry(t, s, out[at]);
}

// log2_capacity as enable was given it: 0 is the default; outside the range the refusal is in q.err
template <class T>
int keyed_capacity(const HookCtx &q, int &log2_capacity) {
    if (log2_capacity == 0) log2_capacity = T::LOG2_DEFAULT;
    if (log2_capacity >= T::LOG2_MIN && log2_capacity <= T::LOG2_MAX) return AMP_OK;
    snprintf(q.err, q.err_cap, "%s takes 2^%d to 2^%d slots (0: the default, 2^%d)", T::NOUN, T::LOG2_MIN, T::LOG2_MAX, T::LOG2_DEFAULT);
    return AMP_EINVAL;
}

// A table of 2^log2_capacity slots that the state owns; a reset (hook_zero) frees the keys and zeroes the rest
template <class W, int N>
int keyed_layout(const HookCtx &q, HookState &s, KeyedTable<W, N> &t, uint32_t log2_capacity) {
    const size_t cap = (size_t)1 << log2_capacity, key_bytes = cap * N * sizeof(W);
    t = KeyedTable<W, N>{nullptr, nullptr, nullptr, 0u};
    HOOKTRY(hook_alloc(q, s, &t.keys, key_bytes + cap * 8 + 64, cap * 8 + 64, key_bytes));
    t.cnt = (uint32_t *)(t.keys + cap * N);
    t.info = (unsigned long long *)(t.cnt + cap * 2);
    t.log2_capacity = log2_capacity;
    return AMP_OK;
}

// amp_*_enable at another capacity than the state's: the hook is switched off, what is in flight on the old tables ends, they
// go back, and layout(s) -- the unit's, as at its first enable -- lays them out again
template <class S, class Layout>
int keyed_relayout(const HookCtx &q, HookSlot &slot, S &s, Layout layout) {
    slot.on = false;
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    hook_release(s);
    return layout(s);
}

// amp_*_get's entries: info and n as the table stands, then -- when the caller's array holds them -- the used slots,
// compacted on the device and sorted here
template <class T, class Info>
int keyed_get(const HookCtx &q, const typename T::Table &t, typename T::Entry *entries, int64_t cap, int64_t *n, Info *info) {
    using Entry = typename T::Entry;
    Guard g(q.device);
    unsigned long long h[2] = {0ull, 0ull};
    HOOKCHK(q, hipMemcpyAsync(h, t.info, sizeof(h), hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    if (info) { info->used = h[0]; info->capacity = 1ull << t.log2_capacity; info->lost = h[1]; }
    if (n) *n = (int64_t)h[0];
    if ((uint64_t)cap < h[0] || (h[0] && !entries)) {
        snprintf(q.err, q.err_cap, "%s holds %llu entries, the array given %lld", T::NOUN, h[0], (long long)cap);
        return AMP_EINVAL;
    }
    if (!h[0]) return AMP_OK;
    Entry *d_out = nullptr;
    HOOKCHK(q, hipMalloc((void **)&d_out, (size_t)h[0] * sizeof(Entry)));
    unsigned long long *d_n = t.info + 2;                          // (inside the allocation's last 64 bytes)
    const int rc = [&]() -> int {
        HOOKCHK(q, hipMemsetAsync(d_out, 0, (size_t)h[0] * sizeof(Entry), q.stream));      // (the entries' padding, too)
        HOOKCHK(q, hipMemsetAsync(d_n, 0, 8, q.stream));
        const uint64_t slots = 1ull << t.log2_capacity;
        k_keyed_compact<T><<<(unsigned)((slots + 255) / 256), 256, 0, q.stream>>>(t, d_out, d_n, h[0]);
        HOOKCHK(q, hipGetLastError());
        HOOKCHK(q, hipMemcpyAsync(entries, d_out, (size_t)h[0] * sizeof(Entry), hipMemcpyDeviceToHost, q.stream));
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        return AMP_OK;
    }();
    (void)hipFree(d_out);
    if (rc == AMP_OK) std::sort(entries, entries + h[0], T::less);
    return rc;
}

// amp_*_add's entries: each checked by `traits`, then all of them through k_keyed_add
template <class T>
int keyed_add(const HookCtx &q, const typename T::Table &t, const T &traits, const typename T::Entry *entries, int64_t n) {
    using Entry = typename T::Entry;
    for (int64_t k = 0; k < n; ++k)
        if (!traits.check(entries[k], (long long)k, q.err, q.err_cap)) return AMP_EINVAL;
    if (!n) return AMP_OK;
    Guard g(q.device);
    Entry *d_in = nullptr;
    HOOKCHK(q, hipMalloc((void **)&d_in, (size_t)n * sizeof(Entry)));
    const int rc = [&]() -> int {
        HOOKCHK(q, hipMemcpyAsync(d_in, entries, (size_t)n * sizeof(Entry), hipMemcpyHostToDevice, q.stream));
        k_keyed_add<T><<<(unsigned)((n + 255) / 256), 256, 0, q.stream>>>(t, d_in, n);
        HOOKCHK(q, hipGetLastError());
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        return AMP_OK;
    }();
    (void)hipFree(d_in);
    return rc;
}

}  // namespace amp
#endif
