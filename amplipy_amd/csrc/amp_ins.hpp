// amp_ins.hpp -- on-device aggregation of insertion events: the internal interface of amp_ins.hip and
// what it does to ONE event, written as plain functions.  The kernels of amp_ins.hip (k_ins_hash, k_ins_poskey, k_ins_heads,
// k_ins_runs) and k_event_strings (amplihip.hip) call them on the device; tests/hostsim/ins_twin.cpp loops the same functions
// over host arrays in the kernels' order of steps, built with plain g++ (no HIP headers: the two attributes are defined away).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/amplihip.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#define AMP_INS_HD __host__ __device__ inline

namespace amp {

// 4-bit base code q of the read whose bases start at base `boff` of the packed array (high nibble first)
AMP_INS_HD uint32_t ins_code(const uint8_t *seq, int64_t boff, int32_t q) {
    const int64_t k = boff + q;
    const uint32_t b = seq[k >> 1];
    return (k & 1) ? (b & 15u) : (b >> 4);
}

// Row of the batch an event's read id refers to: ids are 32-bit and relative to the batch's read_base modulo 2^32.
AMP_INS_HD int64_t ins_read_row(uint32_t read, uint64_t read_base) { return (int64_t)(((uint64_t)read - read_base) & 0xFFFFFFFFull); }

AMP_INS_HD bool ins_unused(const amp_ins_event &e) { return e.ref_pos < 0; }      // a slot that was reserved and not used

// The hash of an allele's base codes: seed, one step per code, and the last shift that keeps the top bit for the unused slots.
constexpr uint64_t INS_KEY_UNUSED = ~0ull;
AMP_INS_HD uint64_t ins_hash_seed() { return 0x9E3779B97F4A7C15ull; }
AMP_INS_HD uint64_t ins_hash_step(uint64_t h, uint32_t code) {
    h ^= (uint64_t)code + 1ull;
    h *= 0xFF51AFD7ED558CCDull;
    return h ^ (h >> 29);
}
AMP_INS_HD uint64_t ins_hash_final(uint64_t h) { return h >> 1; }

// the low sort key of a slot: unused slots sort behind everything, and no used slot has their key (the top bit of a hash is clear)
AMP_INS_HD uint64_t ins_hash_key(const uint8_t *seq, const uint32_t *seq_off8, uint64_t read_base, const amp_ins_event &e) {
    if (ins_unused(e)) return INS_KEY_UNUSED;
    const int64_t boff = (int64_t)seq_off8[ins_read_row(e.read, read_base)] * 8;
    uint64_t h = ins_hash_seed();
    for (int32_t q = e.q_from; q < e.q_to; ++q) h = ins_hash_step(h, ins_code(seq, boff, q));
    return ins_hash_final(h);
}

// the high sort key of a slot: ref_pos << 32 | length
AMP_INS_HD uint64_t ins_pos_key(const amp_ins_event &e) {
    return ins_unused(e) ? INS_KEY_UNUSED : ((uint64_t)(uint32_t)e.ref_pos << 32) | (uint64_t)(uint32_t)(e.q_to - e.q_from);
}

// Two events carry the same allele at the same position: position, length and every base code agree.
AMP_INS_HD bool ins_same_allele(const uint8_t *seq, const uint32_t *seq_off8, uint64_t read_base, const amp_ins_event &a, const amp_ins_event &b) {
    if (ins_pos_key(a) != ins_pos_key(b)) return false;
    const int64_t oa = (int64_t)seq_off8[ins_read_row(a.read, read_base)] * 8, ob = (int64_t)seq_off8[ins_read_row(b.read, read_base)] * 8;
    const int32_t len = a.q_to - a.q_from;
    bool same = true;
    for (int32_t q = 0; q < len && same; ++q) same = ins_code(seq, oa, a.q_from + q) == ins_code(seq, ob, b.q_from + q);
    return same;
}

// slot j of the concatenated shard regions -> its event
struct ShardMap { const amp_ins_event *ev; long long cap; long long start[9]; };      // start[s] = slots in front of shard s
AMP_INS_HD ShardMap ins_shard_map(const amp_ins_event *ev, long long cap, const unsigned long long *shard_n) {
    ShardMap M;
    M.ev = ev; M.cap = cap;
    long long tot = 0;
    for (int k = 0; k < 8; ++k) { M.start[k] = tot; tot += (long long)shard_n[k]; }
    M.start[8] = tot;
    return M;
}
AMP_INS_HD const amp_ins_event &slot_event(const ShardMap &M, int64_t j) {
    int s = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 1; k < 8; ++k) s += j >= M.start[k] ? 1 : 0;
    return M.ev[(size_t)s * (size_t)M.cap + (size_t)(j - M.start[s])];
}

// rid = exclusive sum of head over the sorted events: the run of an event
AMP_INS_HD uint32_t ins_run_of(uint32_t rid, uint32_t head) { return rid + head - 1u; }

#ifdef __HIPCC__
// bytes of device scratch ins_aggregate needs for n_slots event-list slots
size_t ins_scratch_bytes(int64_t n_slots);

// Sorts and run-length encodes the events held in the 8 shard regions of `ev` (region s: shard_n[s] slots of `cap`; slots
// reserved and not used carry ref_pos = -1).  d_runs: room for one record per slot.  Returns 0 or a hipError_t / -1;
// *n_events = real events, *n_runs = records written (device memory d_runs[0 .. *n_runs)).  Synchronises the stream.
int ins_aggregate(hipStream_t s, const amp_dev_reads &rd, uint64_t read_base, const amp_ins_event *ev, long long cap, const unsigned long long *shard_n,
                  void *scratch, amp_ins_run *d_runs, int64_t *n_events, int64_t *n_runs);
#endif

}  // namespace amp
