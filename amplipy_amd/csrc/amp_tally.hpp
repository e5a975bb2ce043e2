// amp_tally.hpp -- the skeleton of the windowed tally kernels behind the read pass: k_strand
// (amp_strand.hip), k_readpos (amp_readpos.hip), k_amplicon (amp_amplicon.hip), k_codon (amp_codon.hip).  HIP only.  The four kernels have one shape.  A
// block of 256 lanes takes a contiguous run of tiles of 256 neighbouring reads (tally_tile_range).  Phase A, one lane per read:
// the read is live when it exists and has status 0 (tally_live), its counted alignment is the trimmed one with do_trim
// (tally_counted_read), its CIGAR becomes a few segments (regular_scan, amp_strand.hpp), and the span of the tile's regular reads
// (wave_span, block_span) says whether the block's window in LDS stays where it is.  Reads the window takes put their segments
// on a list in LDS.  Phase B: lanes own cells of the window; a wave takes the list 64 entries at a time, an entry per lane
// (seg_take), ballots the entries that concern its chunk and visits those, their fields broadcast by shuffle (seg_from); each
// lane adds into its OWN cells with plain LDS adds.  Reads the window did not take walk serially, one lane per read, with LDS
// atomics inside the window and global atomics outside.  When the window moves and when the block ends its non-zero cells go
// to the global table, one atomic each (tally_flush).  The rules of the read pass -- where a read's arrays lie -- and the wave
// and block idioms are written here once.  k_strand and k_readpos, whose windows are both keyed by reference position, are
// one body as well: tally_poswin, at the end, over a policy that names the tally's segments, cells and tables.  The loop nests
// of phase B, the window rules and the serial paths of k_amplicon and k_codon are the kernels' own.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "amp_hook.hpp"
#include "amp_strand.hpp"

namespace amp {

// The reads of a batch and the results of its trimming pass, as a tally kernel is handed them.
struct TallyReads {
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
};

inline TallyReads tally_reads(const HookCtx &q, const amp_dev_reads *rd, const amp_trim_out *o) {
    TallyReads in;
    in.n = rd->n_reads; in.pos = rd->pos; in.flag = rd->flag; in.lseq = rd->lseq; in.cig_off32 = rd->cig_off32; in.cig = rd->cig;
    in.seq_off8 = rd->seq_off8; in.seq = rd->seq; in.qual = rd->qual;
    in.new_pos = o ? o->new_pos : nullptr; in.new_ncig = o ? o->new_ncig : nullptr; in.new_cig = o ? o->new_cig : nullptr;
    in.status = o ? o->status : nullptr;
    in.do_trim = q.do_trim ? 1 : 0;
    in.P = StrandParams{q.ref_len, q.min_quality};
    return in;
}

// The block's contiguous run of tiles [t0, t1) of `block` reads (the bounds are the same for every lane: barriers inside the
// loop over them see whole blocks)
__device__ __forceinline__ void tally_tile_range(int64_t n, int block, int64_t &t0, int64_t &t1) {
    const int64_t tiles = (n + block - 1) / block;
    t0 = tiles * (int64_t)blockIdx.x / (int64_t)gridDim.x;
    t1 = tiles * ((int64_t)blockIdx.x + 1) / (int64_t)gridDim.x;
}

// Lane i's read exists and has status 0.  Nothing of read i is touched unless this holds.
__device__ __forceinline__ bool tally_live(const TallyReads &in, int64_t i) { return i < in.n && (in.status ? in.status[i] == 0 : true); }

// No read: what a lane past n, or with a read that has a status, carries through the tile
__device__ __forceinline__ void tally_no_read(const TallyReads &in, StrandRead &R, uint32_t &qual0) {
    R.pos = 0; R.cig = in.cig; R.n_ops = 0u; R.lseq = 0; R.rev = 0u; R.base = 0ull;
    qual0 = 0xFFu;
}

// The counted alignment of live read i -- the trimmed one with do_trim: its CIGAR lies in new_cig at the original offset plus
// three words per read in front -- and its first quality byte.
__device__ __forceinline__ void tally_counted_read(const TallyReads &in, int64_t i, StrandRead &R, uint32_t &qual0) {
    const uint32_t c0 = in.cig_off32[i];
    if (in.do_trim) {
        R.pos = in.new_pos[i]; R.cig = in.new_cig + (size_t)c0 + 3 * (size_t)i; R.n_ops = in.new_ncig[i];
    } else {
        R.pos = in.pos[i]; R.cig = in.cig + c0; R.n_ops = in.cig_off32[i + 1] - c0;
    }
    R.lseq = (int32_t)in.lseq[i];
    R.rev = (in.flag[i] & 0x10u) ? 1u : 0u;
    R.base = (uint64_t)in.seq_off8[i] * 8ull;
    if (R.lseq > 0) qual0 = in.qual[R.base];
}

// [lo, hi) of a lane that has nothing to span
constexpr int32_t SPAN_NO_LO = 0x7FFFFFFF, SPAN_NO_HI = -0x7FFFFFFF - 1;

// The wave's span: the least lo and the greatest hi of its lanes, in every lane
__device__ __forceinline__ void wave_span(int32_t &lo, int32_t &hi) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
}

// The block's span, in every lane, through s_lo / s_hi[BLOCK / 64].  One barrier, between the waves' stores and the loads.
template <int BLOCK>
__device__ __forceinline__ void block_span(int32_t &lo, int32_t &hi, int32_t *s_lo, int32_t *s_hi) {
    wave_span(lo, hi);
    if ((threadIdx.x & 63u) == 0u) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
}

// The wave's lanes with `have` fall into groups that hold the same key; body(src, same) once per group, wave-uniformly: src is
// the group's lowest lane, `same` the ballot of its lanes.  same_as(src) -- does this lane hold lane src's key -- is evaluated
// by EVERY lane (its shuffles need them all) and is false in a lane without a key.  Whole waves call this; a body that wants
// one actor tests lane == src itself, and one that wants the leader's key lets same_as leave it in a variable of the caller (a
// scalar then, where the lane's own copy is a vector register).  (src is among `same`: the loop ends.)
template <class Same, class Body>
__device__ __forceinline__ void wave_each_distinct(bool have, Same same_as, Body body) {
    unsigned long long pending = __ballot(have);
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        const unsigned long long same = __ballot(same_as(src));
        body(src, same);
        pending &= ~same;
    }
}

// Two per-lane read counters summed over the wave, one atomic each onto reads[0] and reads[1]
__device__ __forceinline__ void tally_wave_add2(unsigned long long *reads, uint32_t a, uint32_t b) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (a) atomicAdd(&reads[0], (unsigned long long)a);
        if (b) atomicAdd(&reads[1], (unsigned long long)b);
    }
}

// Entry s0 + lane of a list of ns segments of type S; `have`: there is one (an all-zero entry otherwise)
template <class S>
__device__ __forceinline__ S seg_take(const S *list, uint32_t s0, uint32_t ns, int lane, bool &have) {
    S mine = {};
    have = s0 + (uint32_t)lane < ns;
    if (have) mine = list[s0 + (uint32_t)lane];
    return mine;
}
// Lane src's entry, in every lane of the wave: a shuffle per 32 bits of S (the copies are of constant size: registers)
template <class S>
__device__ __forceinline__ S seg_from(const S &mine, int src) {
    static_assert(std::is_trivially_copyable<S>::value && sizeof(S) % 4 == 0, "a segment travels by 32-bit shuffles");
    uint32_t w[sizeof(S) / 4];
    __builtin_memcpy(w, &mine, sizeof(S));
#pragma unroll
    for (size_t k = 0; k < sizeof(S) / 4; ++k) w[k] = __shfl(w[k], src);
    S g;
    __builtin_memcpy(&g, w, sizeof(S));
    return g;
}

// The non-zero cells of a window to fn(k, v) -- the kernel's atomic onto its table; the cells are all zero afterwards.
template <int BLOCK, class Fn>
__device__ __forceinline__ void tally_flush(uint32_t *cells, int n_words, Fn fn) {
    for (int k = (int)threadIdx.x; k < n_words; k += BLOCK) {
        const uint32_t v = cells[k];
        if (!v) continue;
        cells[k] = 0u;
        fn(k, v);
    }
}


// The body of a position-window kernel, k_strand and k_readpos: the block keeps a window of T::W reference positions x
// T::WORDS u32 words in LDS; each wave owns every (BLOCK / 64)-th T::CHUNK-position chunk of it and each lane one position of
// the chunk.  T (StrandTally of amp_strand.hpp, ReadposTally of amp_readpos.hpp) says what the tally's segments are, what a
// (segment, position) and a walked increment add to which cell, which window word holds a cell and how a word reaches the
// tables `out`.  The window stays where it is while the block's next tile fits it, for T::MAX_TILES_PER_FLUSH tiles at most.
template <class T>
__device__ __forceinline__ void tally_poswin(const TallyReads &in, const typename T::Out &out) {
    static_assert(T::CHUNK == 64 && T::W % (T::CHUNK * (T::BLOCK / 64)) == 0, "every wave owns the same number of chunks of the window, a lane per position");
    using Seg = typename T::Seg;
    __shared__ uint32_t s_cell[T::W * T::WORDS];
    __shared__ Seg s_seg[T::BLOCK * T::SLOTS];
    __shared__ int32_t s_lo[T::BLOCK / 64], s_hi[T::BLOCK / 64];
    __shared__ uint32_t s_nseg;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto atomic = [](auto *p, auto v) { atomicAdd(p, v); };
    int32_t anchor = 0;
    const auto flush = [&]() {                 // the window to the global tables
        tally_flush<T::BLOCK>(s_cell, T::W * T::WORDS, [&](int k, uint32_t v) { T::flush_word(out, (size_t)anchor + (size_t)(k / T::WORDS), k % T::WORDS, v, atomic); });
    };
    for (int k = tid; k < T::W * T::WORDS; k += T::BLOCK) s_cell[k] = 0u;
    if (tid == 0) s_nseg = 0u;
    int64_t t0, t1;
    tally_tile_range(in.n, T::BLOCK, t0, t1);
    int since = 0;                             // tiles since the last flush
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * T::BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = ST_NO_READ;
        const bool live = tally_live(in, i);
        if (live) {
            tally_counted_read(in, i, R, qual0);
            sh = T::segments(R, in.P, qual0, [](const Seg &) {});
        }
        int32_t lo = sh.regular ? R.pos : SPAN_NO_LO, hi = sh.regular ? sh.ref_end : SPAN_NO_HI;
        block_span<T::BLOCK>(lo, hi, s_lo, s_hi);
        if (!poswin_keeps<T::W>(anchor, lo, hi) || since >= T::MAX_TILES_PER_FLUSH) {        // (the same for every lane)
            flush();
            if (lo <= hi) anchor = lo;
            since = 0;
            __syncthreads();
        }
        ++since;
        const bool win = live && poswin_read_windowed<T::W, T::SLOTS>(sh, R.pos, anchor);
        if (win && sh.n_seg > 0) {
            uint32_t slot = atomicAdd(&s_nseg, (uint32_t)sh.n_seg);        // (at most T::SLOTS per read: the list cannot overflow)
            T::segments(R, in.P, qual0, [&](const Seg &s) { s_seg[slot++] = s; });
        }
        __syncthreads();
        // ---- phase B: position-major over the tile's segments; lane `lane` of the wave owns position c * 64 + lane of chunk c,
        // so no two lanes of a wave add to the same word.  A segment touches three or four of the eight chunks, so most of the
        // list is no work for a given chunk and costs a sixty-fourth of a trip here.
        const uint32_t ns = s_nseg;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                        // (ns is block-uniform: whole waves at the ballots)
            bool have;
            const Seg mine = seg_take(s_seg, s0, ns, lane, have);
            const int32_t m0 = mine.r0 - anchor, m1 = m0 + st_seg_len(mine);
            for (int c = wave; c < T::W / T::CHUNK; c += T::BLOCK / 64) {
                const int32_t c0 = c * T::CHUNK;
                unsigned long long hits = __ballot(have && m1 > c0 && m0 < c0 + T::CHUNK);
                const int32_t p = c0 + lane;
                while (hits) {
                    const int src = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    const Seg g = seg_from(mine, src);
                    const int32_t a0 = g.r0 - anchor, a1 = a0 + st_seg_len(g);
                    if (p >= a0 && p < a1)     // (else not this lane's position; every lane is back for the next segment's shuffles)
                        T::seg_adds(g, p - a0, in.seq, in.qual, in.P.min_quality, [&](int cell, uint32_t v) { s_cell[T::word(p, cell)] += T::inc(cell, v); });
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_nseg = 0u;
        // ---- the serial path: reads the window did not take, LDS atomics inside the window and global atomics outside
        if (live && !win) {
            T::walk(R, in.P, in.seq, in.qual, [&](int32_t r, uint32_t col, auto x) {
                const int64_t w = (int64_t)r - (int64_t)anchor;
                T::walk_adds(R, col, x, [&](int cell, uint32_t v) {
                    if (w >= 0 && w < T::W) atomicAdd(&s_cell[T::word((int32_t)w, cell)], T::inc(cell, v));
                    else T::to_table(out, (size_t)r, cell, v, atomic);
                });
            });
        }
        __syncthreads();
    }
    flush();
}

}  // namespace amp
