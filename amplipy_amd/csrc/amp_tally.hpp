// amp_tally.hpp -- the skeleton of the windowed tally kernels behind the read pass: k_strand
// (amp_strand.hip), k_amplicon (amp_amplicon.hip), k_codon (amp_codon.hip).  HIP only.  The three kernels have one shape.  A
// block of 256 lanes takes a contiguous run of tiles of 256 neighbouring reads (tally_tile_range).  Phase A, one lane per read:
// the read is live when it exists and has status 0 (tally_live), its counted alignment is the trimmed one with do_trim
// (tally_counted_read), its CIGAR becomes a few segments (regular_scan, amp_strand.hpp), and the span of the tile's regular reads
// (wave_span, block_span) says whether the block's window in LDS stays where it is.  Reads the window takes put their segments
// on a list in LDS.  Phase B: lanes own cells of the window; a wave takes the list 64 entries at a time, an entry per lane
// (seg_take), ballots the entries that concern its chunk and visits those, their fields broadcast by shuffle (seg_from); each
// lane adds into its OWN cells with plain LDS adds.  Reads the window did not take walk serially, one lane per read, with LDS
// atomics inside the window and global atomics outside.  When the window moves and when the block ends its non-zero cells go
// to the global table, one atomic each (tally_flush).  The rules of the read pass -- where a read's arrays lie -- and the wave
// and block idioms are written here once; the loop nests of phase B, the window rules and the serial paths are the kernels' own.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

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

// Entry s0 + lane of a list of ns; `have`: there is one (an empty entry otherwise)
__device__ __forceinline__ StrandSeg seg_take(const StrandSeg *list, uint32_t s0, uint32_t ns, int lane, bool &have) {
    StrandSeg mine;
    mine.r0 = 0; mine.len_kind = 0u; mine.q0 = 0ull;
    have = s0 + (uint32_t)lane < ns;
    if (have) mine = list[s0 + (uint32_t)lane];
    return mine;
}
// Lane src's entry, in every lane of the wave
__device__ __forceinline__ StrandSeg seg_from(const StrandSeg &mine, int src) {
    StrandSeg g;
    g.r0 = __shfl(mine.r0, src);
    g.len_kind = __shfl(mine.len_kind, src);
    g.q0 = __shfl((unsigned long long)mine.q0, src);
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

}  // namespace amp
