// amp_fast7.hpp -- the fast kernel for batches of MIXED read lengths (variant 7): the second generation's tile loop
// (f5_tiles, amp_fast5.hpp) driven by per-block lists of reads binned by length, so that a tile's piece loops run to the
// length of ITS reads and no lane is spent on a read that goes to the general pass.  CDNA4 / gfx950.
//
// What k_fast5 does on BASELINE config 5 (75-300 bp reads, 40 % of them for the general pass): a tile is 64 CONSECUTIVE
// reads, its loops run to the longest of them (300 bases in practically every tile) and 43 % of its lanes hold reads it
// hands over: 36 % of the lane-slots do work.  Here a block first walks the headers of its reads once and
// writes four lists into its segment of `clist` (scratch): reads of up to 80 / 144 / 224 / 304 bases whose CIGAR can have
// the closed-form shape (at most five ops, soft clips where a five- or four-op shape needs them); everything else goes on
// the general list at once.  Tiles are then cut from the lists, longest bin first:
//   bins 0 and 1: 64 reads, lane = read, 6 / 10 piece slots
//   bins 2 and 3: 32 reads, TWO lanes per read (lane 2r takes the first 8 / 10 pieces of read r, lane 2r + 1 the others):
//     the rows of 64 reads of 304 bases do not fit a wave's share of the LDS next to six other waves, the rows of 32 do,
//     and the piece loops are half as long.  Both lanes compute the read's trims (same inputs, same result); the first
//     failing window is the minimum over the pair; results, indel extras and hand-overs are lane 2r's.
// A tile's rows are gathered by LDS-DMA into a row-major image with a stride per bin (a multiple of 16 bytes: lane l of
// instruction s moves image bytes [1024 s + 16 l, + 16), which lie in ONE row).  This file holds that tile source, F7Lists;
// everything behind the staging buffers is the shared tile loop, which sees a lane's first piece (`pbase') and whether it
// stores its read's results (`mine').
#pragma once

#include "amp_fast5.hpp"

namespace amp {

#ifndef AMP_F7_ABL
#define AMP_F7_ABL 0      // development builds: bit 2 no gather, bit 4 no tiles (the lists only); results are wrong on purpose
#endif
#ifndef AMP_F7_REPS
#define AMP_F7_REPS 4
#endif
// Waves per block, replicas and width of a wave's packed window: the LDS holds 8 waves with 2 replicas, 7 with 4 or 6 with 5.  The
// counting adds are bound by LDS bank conflicts (14.5 LDS cycles per instruction with two replicas, 12 of them conflicts), so
// replicas buy more than the eighth wave: config 5 takes 1.69 ms with 8 x 2, 1.34 with 7 x 4, 1.43 / 1.42 with 6 x 4 / 6 x 5, 1.52
// with 5 x 8 (profiles/r04_config5_ablations.txt).  (AMP_F7_NWAVES / F7_WAVES are defined in amp_plan.hpp: the host sizes the grid with them.)
#ifndef AMP_F7_PWIN
#define AMP_F7_PWIN 400                   // a read of 304 bases + 16 positions in front + the spread of a tile's starts
#endif
constexpr int F7_QCAP = 9728;             // bytes of a tile's quality image (64 x 144, 32 x 304)
constexpr int F7_SCAP = 5120;             // ... of its packed-base image (64 x 80, 32 x 160)
constexpr uint32_t F7_B2MAX = 224u, F7_PAIRBIN = 2u, F7_B2MAGIC = 19173962u;      // bin 2: reads of up to so many bases; bins from here on hold two lanes per read; ceil(2^32 / F7_B2MAX)
constexpr int F7_REP = AMP_F7_REPS, F7_PW = AMP_F7_PWIN;    // packed window: replicas, positions
constexpr int F7_NBIN = 4;
constexpr int F7_SLOTS = 10;              // pieces of a LANE at most (a read of more than 144 bases has two lanes)

// one of four 16-bit / 32-bit constants by a bin number (shifts of packed words: a chain of selects becomes a table in scratch
// memory, and every load from it makes the wave wait for all of its loads in flight)
__device__ __forceinline__ uint32_t f7_pick16(uint32_t b, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    const uint64_t w = (uint64_t)v0 | ((uint64_t)v1 << 16) | ((uint64_t)v2 << 32) | ((uint64_t)v3 << 48);
    return (uint32_t)(w >> (16u * b)) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t f7_pick32(uint32_t b, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    const uint64_t lo = (uint64_t)v0 | ((uint64_t)v1 << 32), hi = (uint64_t)v2 | ((uint64_t)v3 << 32);
    return (uint32_t)(((b & 2u) ? hi : lo) >> (32u * (b & 1u)));
}
__device__ __forceinline__ uint32_t f7_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// k_fast7's tile source (see the head of the file).  A key is a lane's list entry: its read, 0xFFFFFFFF for none.
struct F7Lists {
    static constexpr int WAVES = F7_WAVES, QCAP = F7_QCAP, SCAP = F7_SCAP;
    static constexpr int SLOTS = F7_SLOTS, AHEAD = F7_SLOTS;
    static constexpr bool SORTED = false;       // (a list is not strictly in the order of the batch)
    // row = offset of the lane's row in the quality image (the packed bases' image has rows at brow), np = pieces of the LANE,
    // first = its first piece, half = the second lane of a pair
    struct Geo { uint32_t np, first, row, brow, bin; bool half, fastq;
        __device__ uint32_t pbase() const { return first; }
        __device__ uint32_t srow() const { return brow; }
        __device__ bool mine() const { return !half; }
        __device__ bool pair() const { return bin >= F7_PAIRBIN; }
        __device__ uint32_t past() const { return 4096u; } };      // (np lies on the partner's pieces)
    uint32_t *clist;                          // 2 * grid * rpb words of scratch (the blocks' lists)
    lds_u32 *nb;                              // the lengths of the block's four lists
    F5Blk b;
    uint32_t *seg;
    uint32_t q_tot8, nb0, nb1, nb2, nb3, t1, t2, t3, n_tb;
    uint32_t tk0, tk1, tk2, tk3, tk4;         // (tickets run four tiles ahead: the list entries of tile t + 4 are asked for while
    uint32_t k0, k1, kR, kN;                  //  tile t is computed, the headers of t + 3)
    __device__ void clear() const { nb[0] = 0; nb[1] = 0; nb[2] = 0; nb[3] = 0; }
    __device__ void prologue(const F5Blk &blk, uint32_t *glist, lds_u32 *gcur) {
        b = blk;
        const int64_t rb = b.rb, re = b.re;
        const int lane = b.lane;
        q_tot8 = b.rd.seq_off8[b.rd.n_reads];      // rows end here (units of 8 bases): 16 bytes of slack behind
        // ---- bins: the block's reads by length (A:426-753 do not care about the order of reads).  The block's segment of clist is
        // two stretches of reads_per_block entries: bins 0 / 1 fill the first from its front / back, bins 2 / 3 the second; reads
        // that cannot have the closed-form shape go on the general list at once.  (The order inside a list is the order in which
        // the waves' groups of 64 reads arrive: a tile does not rely on it.)
        seg = clist + 2 * rb;
        {
            constexpr int R = 4;                                       // groups of 64 reads whose loads are in flight together
            for (int64_t g0 = rb + (int64_t)b.wave * 64; g0 < re; g0 += (int64_t)R * F7_WAVES * 64) {
                uint32_t c0[R], c1[R], ls[R], wf[R], wl[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int64_t i = g0 + (int64_t)r * F7_WAVES * 64 + lane;
                    const int64_t ic = i < re ? i : rb;
                    c0[r] = b.rd.cig_off32[ic]; c1[r] = b.rd.cig_off32[ic + 1]; ls[r] = b.rd.lseq[ic];
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {      // first and last CIGAR word of the reads with four or five ops: such a shape needs soft clips
                    const uint32_t nops = c1[r] - c0[r];
                    const bool want = nops == 4u || nops == 5u;
                    wf[r] = want ? b.rd.cig[c0[r]] : 4u; wl[r] = want ? b.rd.cig[c1[r] - 1u] : 4u;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int64_t i = g0 + (int64_t)r * F7_WAVES * 64 + lane;
                    const bool valid = i < re;
                    const uint32_t nops = c1[r] - c0[r];
                    const bool sf = (wf[r] & 15u) == OP_S, sl = (wl[r] & 15u) == OP_S;
                    const bool cand = ls[r] >= 1u && ls[r] <= (uint32_t)F5_MAXLEN && nops >= 1u && nops <= 5u && (nops < 4u || (nops == 4u ? (sf | sl) : (sf & sl)));
                    const uint32_t cls = !valid ? 5u : !cand ? 4u : ls[r] <= 80u ? 0u : ls[r] <= 144u ? 1u : ls[r] <= F7_B2MAX ? 2u : 3u;
#pragma unroll
                    for (uint32_t c = 0; c < 5u; ++c) {
                        const unsigned long long m = __ballot(cls == c);
                        if (!m) continue;
                        uint32_t base = 0;
                        if (lane == 0) base = __hip_atomic_fetch_add(c == 4u ? gcur : &nb[c], (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        if (cls == c) {
                            if (c == 4u) glist[(size_t)rb + at] = (uint32_t)i;
                            else seg[(c >> 1) * (uint32_t)b.rpb + ((c & 1u) ? (uint32_t)b.rpb - 1u - at : at)] = (uint32_t)i;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // tiles, longest bin first: tiles [0, t3) of bin 3, [t3, t2) of bin 2 (32 reads each), [t2, t1) of bin 1, [t1, n_tb) of bin 0
        nb0 = nb[0]; nb1 = nb[1]; nb2 = nb[2]; nb3 = nb[3];
        t3 = (nb3 + 31u) >> 5; t2 = t3 + ((nb2 + 31u) >> 5); t1 = t2 + ((nb1 + 63u) >> 6); n_tb = (AMP_F7_ABL & 4) ? 0u : t1 + ((nb0 + 63u) >> 6);
    }
    // tile tk: its bin, and the list entry of the lane.  Tiles of bins 2 and 3 hold 32 reads, two lanes each.
    __device__ uint32_t bin_of(uint32_t tk) const { return 3u - (tk >= t3 ? 1u : 0u) - (tk >= t2 ? 1u : 0u) - (tk >= t1 ? 1u : 0u); }
    __device__ uint32_t entry_of(uint32_t tk) const {
        const uint32_t b_ = bin_of(tk);
        const uint32_t first = f7_pick32(b_, t1, t2, t3, 0u), cnt = f7_pick32(b_, nb0, nb1, nb2, nb3);      // (by value: a select between captured variables is a select between their addresses, and puts them in scratch memory)
        const uint32_t ln = f7_lane();
        const uint32_t j = b_ >= F7_PAIRBIN ? (tk - first) * 32u + (ln >> 1) : (tk - first) * 64u + ln;
        const bool valid = tk < n_tb && j < cnt;
        const uint32_t at = (b_ >> 1) * (uint32_t)b.rpb + ((b_ & 1u) ? (uint32_t)b.rpb - 1u - j : j);
        const uint32_t e = seg[valid ? at : 0u];
        return valid ? e : 0xFFFFFFFFu;
    }
    template <class T> __device__ void start(T ticket) {
        tk0 = ticket(); tk1 = ticket(); tk2 = ticket(); tk3 = ticket();
        k0 = entry_of(tk0); k1 = entry_of(tk1);
        kR = entry_of(tk2); kN = entry_of(tk3);
    }
    template <class T> __device__ void take(T ticket) { tk4 = ticket(); }
    __device__ F5Hdr next_hdr() {
        const F5Hdr h = load_hdr(kN);           // (kN arrived before the wait at the top of this turn)
        kR = kN;
        kN = entry_of(tk4);
        return h;
    }
    __device__ void rotate() { tk0 = tk1; tk1 = tk2; tk2 = tk3; tk3 = tk4; }
    __device__ void touch() const { asm volatile("" : : "v"(kN), "v"(kR)); }
    __device__ bool valid(uint32_t ent) const { return ent != 0xFFFFFFFFu; }
    __device__ uint32_t idx(uint32_t ent) const { return valid(ent) ? ent : (uint32_t)b.rb; }      // (a lane without a read points at the block's first)
    __device__ int64_t index(const F5HdrP &h) const { return (int64_t)h.idx; }
    __device__ F5Hdr load_hdr(uint32_t ent) const {
        const int64_t i = ent == 0xFFFFFFFFu ? b.rb : (int64_t)ent;
        F5Hdr h;
        h.pos = b.rd.pos[i]; h.flag = b.rd.flag[i]; h.tlen = b.rd.tlen[i]; h.lseq = b.rd.lseq[i];
        h.c0 = b.rd.cig_off32[i]; h.c1 = b.rd.cig_off32[i + 1]; h.o8 = b.rd.seq_off8[i];
        return h;
    }
    __device__ Geo geometry(const F5HdrP &h, uint32_t tk, uint32_t phi_lane) const {
        Geo g;
        g.bin = bin_of(tk);
        const bool pair = g.bin >= F7_PAIRBIN;
        const uint32_t qs = f7_pick16(g.bin, 80u, 144u, F7_B2MAX, 304u);
        const uint32_t ss = f7_pick16(g.bin, 48u, 80u, 112u, 160u);
        const uint32_t na = 8u + (g.bin & 1u) * 2u;                 // pieces of a pair's first lane (bin 2: 8, bin 3: 10)
        const uint32_t r = pair ? (uint32_t)b.lane >> 1 : (uint32_t)b.lane;
        g.half = pair && (b.lane & 1);
        g.fastq = h.valid();
        const uint32_t npt = (h.lseq() + phi_lane + 15u) >> 4;    // pieces of the read (bins 2 / 3: more than na, by their lengths)
        g.np = !g.fastq ? 1u : !pair ? npt : g.half ? npt - na : na;
        g.first = g.half && g.fastq ? na : 0u;
        g.row = g.fastq ? r * qs : 0u;
        g.brow = g.fastq ? r * ss : 0u;
        return g;
    }
    // LDS-DMA of a tile's rows: lane l of instruction s moves bytes [1024 s + 16 l, + 16) of the row-major image; they belong
    // to ONE row (strides are multiples of 16), whose address comes from the lane that holds the row.  unit = bytes per 8
    // bases (8: qualities, 4: packed bases).  Bytes of a row behind the end of the batch's buffer are fetched from its end
    // (16 bytes of slack); they lie behind the read's own bytes.
    __device__ void stage(const F5HdrP &h, const Geo &g, bool bases, lds_u8 *stage) const {
        const uint8_t *const base = bases ? b.rd.seq : b.rd.qual;
        const uint32_t unit = bases ? 4u : 8u, bin = g.bin;
        const bool pair = bin >= F7_PAIRBIN;
        const uint32_t stride = bases ? f7_pick16(bin, 48u, 80u, 112u, 160u) : f7_pick16(bin, 80u, 144u, F7_B2MAX, 304u);
        const uint32_t magic = bases ? f7_pick32(bin, 89478486u, 53687092u, 38347923u, 26843546u)
                                     : f7_pick32(bin, 53687092u, 29826162u, F7_B2MAGIC, 14128182u);      // ceil(2^32 / stride)
        const uint32_t ln16 = f7_lane() * 16u;
        const uint32_t nbytes = (pair ? 32u : 64u) * stride;
        const int ninst = (AMP_F7_ABL & 2) ? 0 : (int)((nbytes + 1023u) >> 10);
        // the rows' addresses of ALL instructions first (one wait for the ten permutes instead of one each), then the instructions
        constexpr int MAXI = (F7_QCAP + 1023) / 1024;
        uint32_t o8v[MAXI], wv[MAXI];
#pragma unroll
        for (int sl = 0; sl < MAXI; ++sl) {
            if (bases && sl >= (F7_SCAP + 1023) / 1024) break;       // (`bases` is a constant at both call sites)
            const uint32_t off0 = (uint32_t)(sl * 1024) + ln16, off = off0 < nbytes ? off0 : nbytes - 16u;
            const uint32_t row = __umulhi(off, magic);
            wv[sl] = off - row * stride;
            o8v[sl] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((pair ? row * 2u : row) * 4u), (int)h.o8);      // (all lanes take part: a lane that is switched off hands out nothing)
        }
#pragma unroll
        for (int sl = 0; sl < MAXI; ++sl) {
            if (sl >= ninst || (bases && sl >= (F7_SCAP + 1023) / 1024)) break;      // (uniform)
            const uint32_t off0 = (uint32_t)(sl * 1024) + ln16;
            const uint32_t lim = (q_tot8 - o8v[sl]) * unit;
            if (off0 < nbytes) dma16(base + (int64_t)o8v[sl] * unit + (wv[sl] < lim ? wv[sl] : lim), stage + sl * 1024);      // (lanes past the image: the staging buffer ends there)
        }
    }
    // the 128-byte lines of the lane's row (a pair shares them out)
    __device__ void prefetch(const F5HdrP &h1, const Geo &g1, uint32_t &pfA, uint32_t &pfB) const {
        const uint32_t lim = (q_tot8 - h1.o8) * 4u;
        const uint32_t off = g1.half ? 128u : 0u;
        const uint8_t *sb = b.rd.seq + (int64_t)h1.o8 * 4;
        pfA = *(const uint32_t *)(sb + (off < lim ? off : 0u));
        pfB = *(const uint32_t *)(sb + (off + 64u < lim ? off + 64u : 0u));
    }
};

template <int W>
__global__ void __launch_bounds__(F7_WAVES * 64, 2)
k_fast7(F_ARGS, int32_t pad19, uint32_t *clist) {      // (individual arguments, like k_fast: see the note at F_ARGS)
    __shared__ uint32_t s_nb[F7_NBIN];
    f5_tiles<W, F7_REP, F7_PW>(F7Lists{clist, (lds_u32 *)s_nb}, F_ARGS_FWD);
}

// clist: 2 * grid * rpb words of scratch (the blocks' bin lists)
static inline int fast7_launch(const KParams &P, const amp_dev_reads &rd, uint64_t read_base, const DevOut &out, uint32_t *counts,
                               const EventBuf &eb, uint32_t *glist, uint32_t *gcnt, uint32_t *clist, const FastGrid &fg, hipStream_t stream) {
    const unsigned g = (unsigned)fg.grid;
    const int rpb = (int)fg.rpb;
#define AMP_F7_GO(w) k_fast7<w><<<g, F7_WAVES * 64, 0, stream>>>(F_ARGS_PASS(P, rd, out, eb, rpb), 0, clist)
    switch (P.window) {
        case 1: AMP_F7_GO(1); break;
        case 2: AMP_F7_GO(2); break;
        case 3: AMP_F7_GO(3); break;
        case 4: AMP_F7_GO(4); break;
        case 5: AMP_F7_GO(5); break;
        case 6: AMP_F7_GO(6); break;
        case 7: AMP_F7_GO(7); break;
        default: AMP_F7_GO(8); break;
    }
#undef AMP_F7_GO
    return (int)hipGetLastError();
}

}  // namespace amp
