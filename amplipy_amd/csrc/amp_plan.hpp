// amp_plan.hpp -- the host's plan for one batch of reads: which kernels it takes, how large their grids are and where
// each of them finds its piece of the scratch buffer.  Plain C++ (no HIP): the kernel headers include it for the
// geometry constants and grid functions they share with the host, launch_reads (amp_readpass.hip) turns a ReadPlan into
// pointers and launches, and tests/test_read_plan.py checks it on a machine without a GPU.
//
// The plan is a pure function of PlanIn.  Two of its inputs are history: the lengths of the general list and of the heavy list
// of the engine's previous pass (launch_reads reads them from two words the heavy kernel leaves in pinned host memory; negative =
// unknown).  They decide nothing but how many BLOCKS the two kernels behind a fast kernel are launched with (gen_blocks,
// heavy_blocks): twice what the previous pass would have kept busy, between PREDICT_MIN and the full grid for the engine's share
// of the CUs.  The SEGMENTS the lists are cut into (gen_grid, heavy_grid), every other grid and the scratch layout do not depend
// on them, and a block walks as many segments as it has to: a batch unlike the one before runs correctly on the wrong number of
// blocks, only slower, and the pass after it is sized by what it found (tests/test_read_plan_history.py).  "Previous" is the last
// pass that had FINISHED when the host planned this one (the words are read without a wait, so the two block counts depend on
// the host's timing; nothing else does), and only a pass behind a fast kernel leaves history: after a pass of another variant,
// as after a setter that changes a plan input, the next pass has none and takes the full grids.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace amp {

// ---- geometry the host and the kernels share ------------------------------------------------------------------
constexpr int TILE = 64;          // reads per wave tile
constexpr int T_WAVES = 8;        // waves per block of the tile kernel (two blocks per CU)
constexpr int T_MAXOPS = 18;      // CIGAR ops per read held in LDS as 16-bit words (input ops <= T_MAXOPS-3, lengths sum < 4096)
constexpr uint32_t DEFER_INDEX_MASK = 0x3FFFFFFFu;   // read index of a deferred-list entry (the two bits above are its kind: amp_tile.hpp)
// Where k_tile<LIST> finds its list when k_gcompact has not packed it (the common case: one launch less per batch).  The fast
// kernel leaves one list segment per block (entries [b * rpb, b * rpb + gcnt[b]) of glist); a block of the tile kernel sums
// the counts itself (a KB from L2), derives the geometry k_gcompact would have written, and finds entry li of the virtual
// dense list by a binary search over the prefix sums.
constexpr int GL_MAXSEG = 256;
constexpr int GEN_MAXGRID = 1024;     // blocks of the general pass at most = the words of segfirst, one per block

#ifndef AMP_F_WAVES
#define AMP_F_WAVES 8
#endif
constexpr int F_WAVES = AMP_F_WAVES;  // waves per block of k_fast (one block per CU: LDS)
constexpr uint32_t F_EVGRAN = 64;     // event-list slots a wave of a fast kernel reserves at a time
// k_fast's stamps of -DAMP_DEV builds (F_STAMP_OUT, amp_fast.hpp; tools/run_scan.py reads them through amp_debug_blocks): eight words
// per block, then from word F_DBG_WAVE0 on six per wave, written behind the light counts of dcnt
constexpr int F_DBG_WAVE0 = 2048, F_DBG_WAVEWORDS = 6;
static inline size_t fast_stamp_words(int64_t grid) { return F_DBG_WAVE0 + (size_t)grid * F_WAVES * F_DBG_WAVEWORDS; }
constexpr int F6_WAVES = 8;
#ifndef AMP_F7_NWAVES
#define AMP_F7_NWAVES 7               // (why seven: amp_fast7.hpp)
#endif
constexpr int F7_WAVES = AMP_F7_NWAVES;
constexpr int L_WAVES = 12;          // k_long (amp_wave.hpp): waves per block, two blocks per CU
constexpr int L_MAXOPS = 160;        // words per CIGAR row: reads of up to L_MAXOPS - 4 ops (more: the heavy pass's wave path, 508)
constexpr int L_EVCAP = 64;          // events staged per wave

// Geometry shared by the tile kernel and the second pass: block b owns tiles [b*tpb, (b+1)*tpb).
struct TileGrid { int64_t grid, tpb; };
static inline TileGrid tile_grid(int64_t n_reads, int n_cu) {
    const int64_t n_tiles = (n_reads + TILE - 1) / TILE;
    // 32 blocks per CU: two are resident, the rest are handed out as CUs free up, which evens out the
    // (measured) speed differences between blocks and XCDs.  Measured on 19.9 M reads: 8 blocks per CU
    // 3.45 ms, 16: 3.20, 32: 3.15, 64: 3.13, one tile per wave (the minimum): 3.34.
    int64_t tpb = (n_tiles + 32 * (int64_t)n_cu - 1) / (32 * (int64_t)n_cu);
    tpb = ((tpb + T_WAVES - 1) / T_WAVES) * T_WAVES;   // whole super-tiles per block
    if (tpb < T_WAVES) tpb = T_WAVES;
    return TileGrid{(n_tiles + tpb - 1) / tpb, tpb};
}

// Grid of a fast kernel with so many waves per block, `bpc` blocks per CU (one is resident): a block owns a contiguous
// range of whole tiles of 64 reads, which its waves take one by one (at least two tiles per wave).
struct FastGrid { int64_t grid, rpb; };
static inline FastGrid fast_grid_of(int64_t n_reads, int n_cu, int waves, int bpc) {
    int64_t rpb = (n_reads + bpc * (int64_t)n_cu - 1) / (bpc * (int64_t)n_cu);
    rpb = ((rpb + 63) / 64) * 64;
    if (rpb < 2 * waves * 64) rpb = 2 * waves * 64;
    return FastGrid{(n_reads + rpb - 1) / rpb, rpb};
}
#ifndef AMP_F_BPC
#define AMP_F_BPC 1
#endif
static inline FastGrid fast_grid(int64_t n_reads, int n_cu) { return fast_grid_of(n_reads, n_cu, F_WAVES, AMP_F_BPC); }            // k_fast
static inline FastGrid fast5_grid(int64_t n_reads, int n_cu, int waves) { return fast_grid_of(n_reads, n_cu, waves, 1); }      // k_fast5 / k_fast7
static inline FastGrid fast6_grid(int64_t n_reads, int n_cu) { return fast_grid_of(n_reads, n_cu, F6_WAVES, 1); }

struct Fast5Cfg { int waves, qrun; };
// which build of k_fast5: by the mean padded read length of the batch (bases, a multiple of 8 per read)
static inline Fast5Cfg fast5_cfg(int64_t n_reads, int64_t n_bases_padded, int window) {
    const int64_t mean_pad = n_reads > 0 ? (n_bases_padded + n_reads - 1) / n_reads : 0;
    if (mean_pad <= 152 || window != 4) return Fast5Cfg{8, 9728};          // (the other two are built for the default window only)
    if (mean_pad <= 192) return Fast5Cfg{6, 13312};
    return Fast5Cfg{4, 19456};
}

// ---- routing --------------------------------------------------------------------------------------------------
// Windows wider than a chunk take the serial scan of the general kernel, and the fast kernels' byte-parallel quality
// test is written for min_quality <= 128: no fast pass for such runs (amp_fast_path_active).
static inline bool fast_path_active(int requested_variant, int window, int min_quality) {
    return (requested_variant == 0 || requested_variant >= 4) && window <= 8 && min_quality <= 128;
}

// The variant a batch takes (amp_last_kernel_variant; the public statement of the rule is at amp_set_kernel_variant).
// The fast kernel by the batch: its first generation (amp_fast.hpp) keeps a read in registers and is the quicker one for
// reads of up to 152 bases; the second (amp_fast5.hpp) consumes reads from LDS and takes them up to 304 bases (200 and
// 250 bp runs: 1.5 x and 1.3 x the first generation, which hands such reads to the general pass).
// (A window of 8 makes the first-generation kernel spill 39 registers: 0.354 ms on the bench batch against 0.296 for the second;
//  windows 5-7 are its own: 0.253 / 0.269 ms at windows of 6 / 7 against 0.277 / 0.280 -- a window of 7 spills 15 registers since the
//  64-bit adds took four fixed ones, and is still the quicker of the two.)
// (Batches of long reads with many CIGAR ops -- three a read and more: soft clips and indels everywhere, BASELINE config 5 --
//  take the list-driven build of the second generation, amp_fast7.hpp: its tiles hold reads of one length class and none of
//  the reads that go to the general pass; on batches of uniform long reads it is the slower one, 0.49 against 0.37 ms at 250 bp.)
static inline int route_variant(int requested_variant, int64_t n_reads, int64_t n_cig, const Fast5Cfg &f5, int window, int min_quality) {
    const bool mixed = f5.waves != 8 && n_cig >= 3 * n_reads;
    const int kv0 = requested_variant == 0 ? (mixed ? 7 : (f5.waves == 8 && window != 8) ? 4 : 5) : requested_variant;
    const int kv1 = (kv0 >= 4 && !fast_path_active(kv0, window, min_quality)) ? 2 : kv0;
    return (kv1 == 6 && min_quality < 1) ? 4 : kv1;      // (the third generation tells a masked base by its zeroed code: with min_quality 0 the pad bases of a row would count as kept)
}

// ---- the blocks of the second kernels ---------------------------------------------------------------------------
// Segments (blocks' shares) a list of n_list reads is cut into for a general pass of gen_grid segments at most: k_tile<LIST> and
// k_gcompact derive the same on the device (tiles per segment: whole super-tiles, at least one).
static inline int64_t gen_segments(int64_t n_list, int64_t gen_grid) {
    const int64_t tiles = (n_list + TILE - 1) / TILE;
    int64_t tpb = (tiles + gen_grid - 1) / gen_grid;
    tpb = std::max<int64_t>(((tpb + T_WAVES - 1) / T_WAVES) * T_WAVES, T_WAVES);
    return (tiles + tpb - 1) / tpb;
}
constexpr int64_t PREDICT_MIN = 8;      // blocks of a launch that is expected to find nothing (about one per XCD)
static inline int64_t predicted_blocks(int64_t units_before, int64_t cap) {
    return std::min<int64_t>(std::max<int64_t>(2 * units_before, std::min<int64_t>(PREDICT_MIN, cap)), cap);
}

// ---- the plan -------------------------------------------------------------------------------------------------
struct PlanIn {
    int64_t n_reads, n_cig, n_bases_padded;      // amp_dev_reads
    int32_t window, min_quality;
    int requested_variant, n_cu, cu_share;       // amp_set_kernel_variant, the device's CUs, amp_set_cu_share
    bool caller_gives_new_pos, caller_gives_new_ncig, caller_gives_new_cig;      // outputs the caller has buffers for
    // what the previous pass of this engine left for its second kernels: reads on the general list, entries on the heavy
    // (deferred) list.  Negative: no history -- the engine's first pass, or one behind a setter that changed the plan's inputs.
    int64_t prev_list = -1, prev_heavy = -1;
};

struct Region { size_t off, words; };      // a piece of the scratch buffer, in 32-bit words (arrays of such words: nothing asks for more than their alignment)
struct ReadPlan {
    int kv, variant;      // what amp_last_kernel_variant reports; the launch sequence (5, 6 and 7 differ from 4 in the fast kernel only)
    Fast5Cfg f5;
    FastGrid fg;          // grid of the fast kernel of `kv` (variants 1-3 launch none)
    int fast_waves;       // ... and its waves per block (0: none)
    TileGrid tg;
    int64_t gen_grid, heavy_grid;      // list segments of k_tile<LIST> (the general pass of variant 4); the most blocks k_deferred_heavy is given on the whole chip
    int64_t gen_blocks, heavy_blocks;  // blocks the two are launched with (variant 4): predicted from the engine's previous pass, see plan_reads
    bool long_kernel;     // k_long (amp_wave.hpp) takes the reads with many CIGAR ops
    bool direct;          // k_tile<LIST> indexes the fast kernel's per-block segments itself: no k_gcompact
    int64_t ev_fixed;     // event-list slots to reserve on top of the bound of the batch's events
    size_t total_words;   // scratch the batch needs
    // scratch, in this order.  Regions no kernel of the variant touches have no words.
    Region pingpong;      // CIGAR slots the serial trims ping-pong with (the other buffer is the read's output slot)
    Region dlist;         // deferred list: one segment of tpb * 64 entries per tile-kernel block
    Region dcnt;          // [grid] light counts | 64 | [4 * grid] debug words | [grid] heavy counts (-DAMP_DEV: at least fast_stamp_words behind the 64)
    Region split;         // variant 3: the four hand-over arrays of SplitDesc, n words each
    Region new_pos, new_ncig, new_cig;      // stand-ins for outputs the caller did not give and the second pass reads (no words otherwise)
    Region glist, gcnt;   // variant 4: the fast kernel's hand-over list, one segment of rpb entries per block, and the entries used in each
                          // (gcnt has F_WAVES words per block; the kernels write and read the first `grid` of them)
    Region gdense, geo;   // ... the dense list k_gcompact packs them into, GenGeo
    Region segfirst;      // ... first read of every block of the general pass
    Region llist, lpos;   // long_kernel: k_long's reads and their places in gdense
    Region clist;         // variants 6 / 7: the blocks' class / bin lists
};

// The plan of a batch of n_reads >= 1.  false: no plan -- the batch is empty, or too large for the 30-bit read index of the
// list entries; nothing of `p` is valid then.  A handful of integer operations: it runs once per batch on the host's critical path.
static inline bool plan_reads(const PlanIn &in, ReadPlan &p) {
    const int64_t n = in.n_reads;
    if (n < 1 || n > (int64_t)DEFER_INDEX_MASK) return false;
    p.f5 = fast5_cfg(n, in.n_bases_padded, in.window);
    p.kv = route_variant(in.requested_variant, n, in.n_cig, p.f5, in.window, in.min_quality);
    p.variant = p.kv >= 5 ? 4 : p.kv;
    p.tg = tile_grid(n, in.n_cu);
    const int fast_cus = std::max(1, in.n_cu / in.cu_share);
    p.fast_waves = p.kv == 7 ? F7_WAVES : p.kv == 6 ? F6_WAVES : p.kv == 5 ? p.f5.waves : p.kv == 4 ? F_WAVES : 0;
    p.fg = p.kv == 6 ? fast6_grid(n, fast_cus) : p.kv >= 5 ? fast5_grid(n, fast_cus, p.fast_waves) : fast_grid(n, fast_cus);
    // general pass of variant 4: at most four blocks per CU (its list is usually a tenth of the batch; blocks without
    // tiles would still have to be placed on a CU one after the other), tiles per block decided on the device
    p.gen_grid = std::min<int64_t>(std::min<int64_t>(p.tg.grid, 4 * (int64_t)in.n_cu), GEN_MAXGRID);
    p.heavy_grid = std::min<int64_t>(p.tg.grid, 2 * (int64_t)in.n_cu);
    // ... and how many blocks walk those segments.  Blocks of a launch with nothing to do still have to be placed, each on a CU
    // that no block of a fast kernel holds (a k_fast block takes its CU whole), so the launch is sized for the work the engine's
    // previous pass had: twice the segments its list would fill today, and twice the rounds of 256 entries its heavy list was,
    // between PREDICT_MIN and the full grid for this engine's share of the CUs.  A block walks segments b, b + blocks, ...: a
    // wrong prediction costs time, never the result, and the next pass is sized by what this one finds.
    {
        const int64_t gen_cap = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.tg.grid, 4 * (int64_t)fast_cus), GEN_MAXGRID));
        const int64_t heavy_cap = std::max<int64_t>(1, std::min<int64_t>(p.tg.grid, 2 * (int64_t)fast_cus));
        p.gen_blocks = in.prev_list < 0 ? gen_cap : predicted_blocks(gen_segments(in.prev_list, p.gen_grid), gen_cap);
        p.heavy_blocks = in.prev_heavy < 0 ? heavy_cap : predicted_blocks((in.prev_heavy + 255) / 256, heavy_cap);
    }
    // a batch of reads with many CIGAR ops (eight a read on average: Nanopore-like) gets k_long (amp_wave.hpp) for them; the
    // results do not depend on this choice
    p.long_kernel = p.variant == 4 && in.n_cig >= 8 * n;
    // the list stays in the fast kernel's per-block segments and the tile kernel indexes them itself -- one launch less --
    // unless k_long needs the dense list (to flag its reads in) or the fast kernel ran more blocks than the tile kernel's table holds
    // (a fast grid never has more blocks than CUs: on a 256-CU part only long_kernel switches this off, and the plan's side of
    //  fg.grid > GL_MAXSEG is covered by the n_cu = 304 rows of tests/test_read_plan.py)
    p.direct = !p.long_kernel && p.fg.grid <= GL_MAXSEG;      // (read by variant 4 only)
    // Any shard may receive every new event, so each is sized for the batch's bound plus: one open granule per wave of the fast
    // kernel (it reserves list slots a granule at a time; a refill leaves fewer slots unused than the tile that caused it needs)
    // and of k_long.  The fast kernel's term is the larger of k_fast's waves for this batch -- what was reserved before the
    // chosen kernel was known here, kept so that no reservation shrinks -- and the waves of the kernel that runs (k_fast7's
    // seven-wave blocks are smaller: 897 reads are two blocks, 14 waves, where k_fast has 8).
    p.ev_fixed = std::max((p.kv <= 4 ? p.fg : fast_grid(n, fast_cus)).grid * F_WAVES, p.fg.grid * p.fast_waves) * (int64_t)F_EVGRAN + 2 * (int64_t)in.n_cu * L_WAVES * L_EVCAP;
    // the scratch buffer
    const size_t un = (size_t)n, slots = (size_t)in.n_cig + 3 * un;      // a read's CIGAR slot: its ops + 3 (what the trims can add)
    const size_t n_tiles = (un + TILE - 1) / TILE;
    const size_t gen_tpb_max = (((n_tiles + (size_t)p.gen_grid - 1) / (size_t)p.gen_grid + T_WAVES - 1) / T_WAVES) * T_WAVES;
    const bool v4 = p.variant == 4;
    const size_t fast_list = v4 ? (size_t)p.fg.grid * (size_t)p.fg.rpb : 0;
    size_t at = 0;
    const auto take = [&at](size_t words) { const Region r{at, words}; at += words; return r; };
    p.pingpong = take(slots);
    p.dlist = take(std::max(((size_t)p.tg.grid + 1) * (size_t)p.tg.tpb, n_tiles + gen_tpb_max + T_WAVES) * TILE);
    size_t dcnt_words = (size_t)p.tg.grid * 6 + 64;
#ifdef AMP_DEV      // k_fast stamps over the debug words and past them: on a small batch further than dcnt reaches otherwise
    if (p.kv == 4) dcnt_words = std::max(dcnt_words, (size_t)p.tg.grid + 64 + fast_stamp_words(p.fg.grid));
#endif
    p.dcnt = take(dcnt_words);
    p.split = take(p.variant == 3 ? 4 * un : 0);
    p.new_pos = take(in.caller_gives_new_pos ? 0 : un);
    p.new_ncig = take(in.caller_gives_new_ncig ? 0 : un);
    p.new_cig = take(in.caller_gives_new_cig ? 0 : slots);
    p.glist = take(fast_list);
    p.gcnt = take(v4 ? (size_t)p.fg.grid * F_WAVES : 0);
    p.gdense = take(v4 ? (un + 3) & ~(size_t)3 : 0);
    p.geo = take(v4 ? 4 : 0);
    p.segfirst = take(v4 ? GEN_MAXGRID : 0);
    p.llist = take(p.long_kernel ? un : 0);
    p.lpos = take(p.long_kernel ? un : 0);
    p.clist = take(p.kv == 6 ? fast_list : p.kv == 7 ? 2 * fast_list : 0);
    p.total_words = at;      // (the carver's position: size and placement cannot disagree)
    return true;
}

}  // namespace amp
