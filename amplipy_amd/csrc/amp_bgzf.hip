// amp_bgzf.hip -- the opt-in device codec for BAM input.
//
// The reference reads BAM through pysam (AmpliPy.py:296-324, :896) and skips records by A:902; the host codec does that in
// libampbam (ampbam_open_range_at: BGZF inflate, CRC check and record index on host threads; ampbam_decode: the packed batch),
// and the decoded batch is then copied to the device.  Here the COMPRESSED bytes of a piece of the file (whole BGZF blocks) go
// up, and everything else happens in HBM:
//   inflate  one wave per BGZF block (k_bgzf_inflate): the block's raw DEFLATE stream into its place in the piece's image
//            [carry | inflated blocks]; the decoder's tables lie in LDS
//   crc      one wave per block (k_bgzf_crc): 64 slices folded and combined, compared with the block's trailer
//   walk     lane = stretch of BAM_STRETCH image bytes: a first record start (known for the stretch of the first record, else the
//            first offset from which a chain of 64 plausible records runs and from which the stretch can be walked), the number of
//            records that start in the stretch, where the chain leaves it
//   rounds   link / jump x K / settle: pointer jumping over `stretch -> stretch of its exit offset` marks the stretches the TRUE
//            chain passes through (a link holds only where the chain arrives exactly at the next stretch's entry); the stretch
//            where it breaks is walked again from the true arrival and the round repeats.  A settled index makes later rounds
//            leave at once, so rounds are launched blind
//   emit     lane = stretch on the chain: record offsets, the row predicate of A:902, CIGAR words and 8-base slots per record;
//            exclusive sums (hipcub) give row, CIGAR-word and slot offsets
//   rows     lane = record: the row's scalars, its CIGAR words, src_index
//   pack     lane = one 8-base slot of the batch: 4 bytes of nibbles, 8 quality bytes (pads, spare nibble zero)
// One wait per piece: counts and verdicts come down together.  A block the device refuses (decoder or CRC) is named to the
// caller, who inflates it on the host and patches it in (amp_bam_patch_block, amp_bam_reindex).
//
// The lane functions compile for the host as well (-DAMPBGZF_HOSTSIM: any C++ compiler, sanitizers included) and a driver runs
// them lane after lane: the twin the CPU tests check against libampbam.
// What surrounds the stages -- stream, copies, scan, events, the batch's way into the read pass -- is the shell of amp_codec.hpp.
#include <utility>
#include <vector>

#include "amp_codec.hpp"
#define BGZ_HD AMP_HD
#include "amp_bamtail.hpp"
#include "amp_bamtext.hpp"

namespace ampbgzf {

enum { CTL_REFUSED = 0, CTL_SETTLED, CTL_BAD, CTL_ROUNDS, CTL_CARRY, CTL_NREC, CTL_NROWS, CTL_NCIG, CTL_NBASES, CTL_NSLOTS,
       CTL_WORDS = 16 };
enum { BAM_STRETCH = 4096, WAVE = 64, CHAIN = 64, BLIND_ROUNDS = 2 };
enum { ST_RUN = 0, ST_END = 1, ST_BAD = 2 };
static const uint32_t NONE = 0xFFFFFFFFu;
static const int64_t IMAGE_LIMIT = AMP_BAM_IMAGE_LIMIT;

struct DevBlock { uint32_t in_off, in_len, out_off, out_len, crc; };

// Every pointer of a piece: device memory in the library, host memory in the twin.  Buf is a kernel argument and its layout the
// kernels' view of it: blocks, image and index, then the batch (amp_dev_reads: the shell's struct), then the counters.
struct BufIndex {
    const uint8_t *comp; const DevBlock *blocks; uint8_t *verdict; int64_t n_blocks, force_refuse;
    uint8_t *img; int64_t n_img, carry_len, o0, t0, n_stretch, rec_cap, rec_base; int32_t n_ref;
    uint32_t *entry, *exit_, *cnt, *s_cnt, *ja, *jb; uint8_t *st, *reach;
    uint32_t *rec_off, *s_row, *s_ncig, *s_slots;
};
struct Buf : BufIndex, ampcodec::Batch {
    uint32_t *row_seq;
    unsigned long long *ctl;
    uint64_t spare;            // (the kernels' other arguments stay where they were when a pointer lay here)
    ampbamout::Out o;          // the re-encoder of trimmed records (amp_bamout.hip)
    ampbamtext::Text x;        // trimmed records as SAM text (amp_bamtext.hip)
};

// ---- inflate / crc: one wave per block ----------------------------------------------------------------------------------------
BGZ_HD void lane_inflate(const Buf &b, int64_t k, Tables &T) {
    const DevBlock blk = b.blocks[k];
    const bool ok = inflate_block(b.comp + blk.in_off, blk.in_len, b.img + b.carry_len + blk.out_off, blk.out_len, T);
    b.verdict[k] = ok ? 0 : 1;
}
// `reg` = XOR of crc_lane over the 64 lanes
BGZ_HD void lane_crc_verdict(const Buf &b, int64_t k, uint32_t reg) {
    if (b.verdict[k] == 0 && ((~reg) != b.blocks[k].crc || k == b.force_refuse)) b.verdict[k] = 2;
    if (b.verdict[k]) AMP_ADD64(&b.ctl[CTL_REFUSED], 1);
}

// ---- the record index -----------------------------------------------------------------------------------------------------------
struct Walk { uint32_t exit_, cnt, st; };
BGZ_HD Walk walk_from(const Buf &b, uint64_t o, uint64_t hi) {
    Walk w{0, 0, ST_RUN};
    while (o < hi) {
        uint64_t nx = 0;
        const int s = record_step(b.img, (uint64_t)b.n_img, o, &nx);
        if (s == STEP_STOP) { w.st = ST_END; break; }
        if (s == STEP_BAD) { w.st = ST_BAD; break; }
        ++w.cnt; o = nx;
    }
    if (w.st == ST_RUN && o + 36 > (uint64_t)b.n_img) w.st = ST_END;      // (what the walk of the next stretch would find)
    w.exit_ = (uint32_t)o;
    return w;
}
BGZ_HD bool idx_skip(const Buf &b) { return b.ctl[CTL_REFUSED] != 0; }
BGZ_HD void put_walk(const Buf &b, int64_t t, uint32_t entry, const Walk &w) { b.entry[t] = entry; b.exit_[t] = w.exit_; b.cnt[t] = w.cnt; b.st[t] = (uint8_t)w.st; }

BGZ_HD void lane_walk(const Buf &b, int64_t t) {
    if (idx_skip(b)) return;
    const uint64_t n = (uint64_t)b.n_img, lo = (uint64_t)t * BAM_STRETCH, hi = lo + BAM_STRETCH < n ? lo + BAM_STRETCH : n;
    Walk none{0, 0, ST_RUN};
    if (t < b.t0) { put_walk(b, t, NONE, none); return; }
    if (t == b.t0) { put_walk(b, t, (uint32_t)b.o0, walk_from(b, (uint64_t)b.o0, hi)); return; }      // the known first record: no guess
    for (uint64_t cand = lo; cand < hi; ++cand) {
        uint64_t at = cand, nx = 0;
        int chain = 0;
        while (chain < CHAIN && at + 36 <= n && record_plausible(b.img, n, at, b.n_ref, &nx)) { at = nx; ++chain; }
        if (!(chain >= CHAIN || (chain >= 1 && at + 36 > n))) continue;
        const Walk w = walk_from(b, cand, hi);
        if (w.st == ST_BAD) continue;
        put_walk(b, t, (uint32_t)cand, w);
        return;
    }
    put_walk(b, t, NONE, none);
}

// the chain that enters stretch t at entry[t] ends here: the image's end, a bad record, or a next stretch that was entered elsewhere
BGZ_HD bool terminal(const Buf &b, int64_t t) {
    if (b.entry[t] == NONE || b.st[t] != ST_RUN) return true;
    return b.entry[b.exit_[t] / BAM_STRETCH] != b.exit_[t];
}
BGZ_HD void lane_link(const Buf &b, int64_t t) {
    if (idx_skip(b) || b.ctl[CTL_SETTLED]) return;
    b.reach[t] = t == b.t0 ? 1 : 0;
    b.ja[t] = terminal(b, t) ? (uint32_t)t : b.exit_[t] / BAM_STRETCH;
}
BGZ_HD void lane_jump(const Buf &b, int64_t t) {
    if (idx_skip(b) || b.ctl[CTL_SETTLED]) return;
    const uint32_t j = b.ja[t];
    if (b.reach[t]) b.reach[j] = 1;
    b.jb[t] = b.ja[j];
}
BGZ_HD void lane_settle(const Buf &b, int64_t t) {
    if (idx_skip(b) || b.ctl[CTL_SETTLED]) return;
    if (!b.reach[t] || !terminal(b, t)) return;            // (exactly one stretch passes: the last one on the true chain)
    b.ctl[CTL_ROUNDS] += 1;
    if (b.st[t] == ST_END) { b.ctl[CTL_CARRY] = b.exit_[t]; b.ctl[CTL_SETTLED] = 1; return; }
    if (b.st[t] == ST_BAD) { b.ctl[CTL_BAD] = 1; b.ctl[CTL_CARRY] = b.exit_[t]; b.ctl[CTL_SETTLED] = 1; return; }
    // the true chain arrives at exit[t], the stretch there was entered elsewhere (or nowhere): walk it from the arrival
    const uint64_t o = b.exit_[t], nt = o / BAM_STRETCH, n = (uint64_t)b.n_img;
    const uint64_t hi = (nt + 1) * BAM_STRETCH < n ? (nt + 1) * BAM_STRETCH : n;
    put_walk(b, (int64_t)nt, (uint32_t)o, walk_from(b, o, hi));
}

// ---- decode -----------------------------------------------------------------------------------------------------------------------
BGZ_HD bool dec_skip(const Buf &b) { return b.ctl[CTL_REFUSED] != 0 || b.ctl[CTL_SETTLED] == 0 || b.ctl[CTL_BAD] != 0; }
BGZ_HD void lane_counts(const Buf &b, int64_t t) { b.s_cnt[t] = (!dec_skip(b) && b.reach[t]) ? b.cnt[t] : 0u; }

BGZ_HD void lane_emit(const Buf &b, int64_t t) {
    if (dec_skip(b) || !b.reach[t]) return;
    const uint64_t n = (uint64_t)b.n_img, hi = (uint64_t)(t + 1) * BAM_STRETCH < n ? (uint64_t)(t + 1) * BAM_STRETCH : n;
    uint64_t o = b.entry[t];
    uint64_t i = b.s_cnt[t];
    while (o < hi) {
        uint64_t nx = 0;
        if (record_step(b.img, n, o, &nx) != STEP_OK) break;
        if (i < (uint64_t)b.rec_cap) {
            const uint8_t *c = b.img + o + 4;
            const uint32_t n_cig = rd16(c + 12), flag = rd16(c + 14), l_seq = rd32(c + 16);
            const bool row = !(flag & 4u) && n_cig > 0;                      // A:902
            b.rec_off[i] = (uint32_t)o;
            b.s_row[i] = row ? 1u : 0u; b.s_ncig[i] = row ? n_cig : 0u; b.s_slots[i] = row ? (uint32_t)(((uint64_t)l_seq + 7) >> 3) : 0u;
        }
        ++i; o = nx;
    }
    if (terminal(b, t)) b.ctl[CTL_NREC] = i < (uint64_t)b.rec_cap ? i : (uint64_t)b.rec_cap;
}

BGZ_HD void lane_rows(const Buf &b, int64_t i) {
    if (dec_skip(b)) return;
    const uint32_t o = b.rec_off[i];
    const uint8_t *c = b.img + o + 4;
    const uint32_t l_name = c[8], n_cig = rd16(c + 12), flag = rd16(c + 14), l_seq = rd32(c + 16);
    const bool row = !(flag & 4u) && n_cig > 0;
    if (row) {
        const uint32_t r = b.s_row[i], c0 = b.s_ncig[i];
        b.pos[r] = (int32_t)rd32(c + 4); b.flag[r] = (uint16_t)flag; b.tlen[r] = (int32_t)rd32(c + 28); b.lseq[r] = l_seq;
        b.cig_off32[r] = c0; b.seq_off8[r] = b.s_slots[i];
        const uint8_t *v = c + 32 + l_name;
        for (uint32_t k = 0; k < n_cig; ++k) b.cig[c0 + k] = rd32(v + 4 * k);
        b.row_seq[r] = o + 4u + 32u + l_name + 4u * n_cig;
        b.src_index[r] = b.rec_base + i;
        AMP_ADD64(&b.ctl[CTL_NBASES], l_seq);
    }
    if (i == (int64_t)b.ctl[CTL_NREC] - 1) {
        const uint32_t nr = b.s_row[i] + (row ? 1u : 0u);
        b.cig_off32[nr] = b.s_ncig[i] + (row ? n_cig : 0u);
        b.seq_off8[nr] = b.s_slots[i] + (row ? (uint32_t)(((uint64_t)l_seq + 7) >> 3) : 0u);
        b.ctl[CTL_NROWS] = nr; b.ctl[CTL_NCIG] = b.cig_off32[nr]; b.ctl[CTL_NSLOTS] = b.seq_off8[nr];
    }
}

BGZ_HD void lane_pack(const Buf &b, int64_t s) {
    if (dec_skip(b)) return;
    const uint32_t n = (uint32_t)b.ctl[CTL_NROWS];
    uint32_t lo = 0, hi = n;                                  // the last row r with seq_off8[r] <= s (rows without bases own no slot)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (b.seq_off8[mid] <= (uint32_t)s) lo = mid; else hi = mid; }
    const uint32_t r = lo, k = (uint32_t)s - b.seq_off8[r], L = b.lseq[r];
    const uint32_t nb = L - 8u * k >= 8u ? 8u : L - 8u * k;
    const uint8_t *sq = b.img + b.row_seq[r];
    uint32_t w;
    __builtin_memcpy(&w, sq + 4u * k, 4);                     // (the image carries 64 zeroed bytes behind its end)
    const uint32_t nbytes = (nb + 1u) >> 1;
    if (nbytes < 4u) w &= (1u << (8u * nbytes)) - 1u;
    if (nb & 1u) w &= ~(0x0Fu << (8u * (nbytes - 1u)));       // the spare nibble of an odd l_seq
    __builtin_memcpy(b.seq + 4 * (size_t)s, &w, 4);
    uint64_t q;
    __builtin_memcpy(&q, sq + ((L + 1u) >> 1) + 8u * k, 8);
    if (nb < 8u) q &= (1ull << (8u * nb)) - 1ull;
    __builtin_memcpy(b.qual + 8 * (size_t)s, &q, 8);
}

BGZ_HD void lane_slack(const Buf &b, int64_t) {               // 16 zeroed bytes behind cig, seq and qual
    if (dec_skip(b)) return;
    const size_t nc = (size_t)b.ctl[CTL_NCIG], ns = (size_t)b.ctl[CTL_NSLOTS];
    for (int k = 0; k < 4; ++k) b.cig[nc + k] = 0;
    for (int k = 0; k < 16; ++k) { b.seq[4 * ns + k] = 0; b.qual[8 * ns + k] = 0; }
}

// ---- layout -----------------------------------------------------------------------------------------------------------------------
static inline int64_t rec_cap_for(int64_t n_img) { return n_img / 37 + 2; }       // a record is 4 + 32 + a name of one byte at least
// Carves `base` (NULL: sizes only) for images of up to cap bytes and n_blocks blocks; returns the bytes needed.
static size_t carve(Buf &b, uint8_t *base, int64_t cap, int64_t cap_blocks) {
    const size_t n = (size_t)cap, S = n / BAM_STRETCH + 2, R = (size_t)rec_cap_for(cap);
    ampcodec::Carver take{base};
    b.blocks = (const DevBlock *)take((size_t)cap_blocks * sizeof(DevBlock)); b.verdict = take((size_t)cap_blocks);
    uint32_t **per_stretch[] = {&b.entry, &b.exit_, &b.cnt, &b.s_cnt, &b.ja, &b.jb};
    for (uint32_t **p : per_stretch) *p = (uint32_t *)take(S * 4);
    b.st = take(S); b.reach = take(S);
    uint32_t **per_rec[] = {&b.rec_off, &b.s_row, &b.s_ncig, &b.s_slots};
    for (uint32_t **p : per_rec) *p = (uint32_t *)take(R * 4);
    b.pos = (int32_t *)take((R + 1) * 4); b.flag = (uint16_t *)take((R + 1) * 2); b.tlen = (int32_t *)take((R + 1) * 4);
    b.lseq = (uint32_t *)take((R + 1) * 4); b.cig_off32 = (uint32_t *)take((R + 1) * 4); b.seq_off8 = (uint32_t *)take((R + 1) * 4);
    b.row_seq = (uint32_t *)take((R + 1) * 4); b.src_index = (int64_t *)take((R + 1) * 8);
    // a row's CIGAR words, packed bases and qualities all lie in its record: 4 bytes per word, and a row of L bases has
    // (L + 1) / 2 + L bytes of them, so its ceil(L / 8) slots are at most L / 8 + 1
    b.cig = (uint32_t *)take((n / 4 + 8) * 4); b.seq = take((n / 8 + R) * 4 + 64); b.qual = take((n / 8 + R) * 8 + 64);
    b.ctl = (unsigned long long *)take(CTL_WORDS * 8);
    return take.o;
}

}  // namespace ampbgzf

using namespace ampbgzf;
using namespace ampcodec;

CODEC_FIRST_BAD_KERNEL(k_bam_first_bad)
#ifndef AMPBGZF_HOSTSIM
CODEC_KERNEL(k_bam_walk, lane_walk)
CODEC_KERNEL(k_bam_link, lane_link)
CODEC_KERNEL(k_bam_jump, lane_jump)
CODEC_KERNEL(k_bam_settle, lane_settle)
CODEC_KERNEL(k_bam_counts, lane_counts)
CODEC_KERNEL(k_bam_emit, lane_emit)
CODEC_KERNEL(k_bam_rows, lane_rows)
CODEC_KERNEL(k_bam_pack, lane_pack)
CODEC_KERNEL(k_bam_slack, lane_slack)

// One wave per BGZF block, its decoder's tables in LDS.  The decode of a stream is serial in its bit position: lane 0 runs it
// (the branch is wave-uniform per instruction: the other lanes are masked off, not diverged into another path).
__global__ void __launch_bounds__(64) k_bgzf_inflate(Buf b) {
    __shared__ Tables T;
    for (int64_t k = blockIdx.x; k < b.n_blocks; k += gridDim.x) {
        if (threadIdx.x == 0) lane_inflate(b, k, T);
        __syncthreads();
    }
}
// Four waves per workgroup, one block each; the byte table of the CRC in LDS.
__global__ void __launch_bounds__(256) k_bgzf_crc(Buf b) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < b.n_blocks; k += (int64_t)gridDim.x * 4) {
        const DevBlock blk = b.blocks[k];
        uint32_t reg = b.verdict[k] ? 0u : crc_lane(b.img + b.carry_len + blk.out_off, blk.out_len, lane, tab);
        for (int d = 32; d >= 1; d >>= 1) reg ^= __shfl_xor(reg, d, 64);
        if (lane == 0) lane_crc_verdict(b, k, reg);
    }
}
#endif

struct amp_bam {
    Shell sh;
    Buf b{};
    size_t cap_img = 0, cap_comp = 0, cap_carry = 0, cap_arena = 0;
    int64_t arena_img = 0, arena_blocks = 0;
    uint8_t *arena = nullptr, *img = nullptr, *comp = nullptr, *carry = nullptr;
    int64_t carry_len = 0;                            // bytes of the last image behind its last complete record, kept in `carry`
    Trim trim{};                                      // results of the read pass
    std::vector<DevBlock> h_blocks;
    std::vector<uint8_t> h_verdict;
    amp_bam_info info{};
    bool fed = false;
    int64_t refused_left = 0, force_refuse = -1;
    unsigned long long h_ctl[CTL_WORDS];
    // the re-encoder of trimmed records (amp_bamout.hip)
    bool processed = false, encoded = false;          // of the last feed: results are there; its rows were encoded
    int64_t good_rows = 0;                            // rows in front of the first failing one
    ampbamout::Tail tail;                             // the encoder's buffers, carry and counters (amp_bamtail.hpp)
    ampbamtext::State text;                           // trimmed records as SAM text: name table, sizes, the text (amp_bamtext.hip)
};

#ifndef AMPBGZF_HOSTSIM
static int bam_inflate_crc(amp_bam *s) {
    const int64_t nb = s->b.n_blocks;
    if (nb <= 0) return AMP_OK;
    // twelve decoders fit a CU's LDS: 256 x 12 workgroups are resident at once, a larger piece's blocks queue behind them
    k_bgzf_inflate<<<(unsigned)(nb < 3072 ? nb : 3072), 64, 0, s->sh.stream>>>(s->b);
    if (hipGetLastError() != hipSuccess) return AMP_EHIP;
    codec_mark(s->sh, 2);
    k_bgzf_crc<<<(unsigned)((nb + 3) / 4 < 4096 ? (nb + 3) / 4 : 4096), 256, 0, s->sh.stream>>>(s->b);
    return hipGetLastError() == hipSuccess ? AMP_OK : AMP_EHIP;
}
#else
static int bam_inflate_crc(amp_bam *s) {
    static Tables T;
    static uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i);
    for (int64_t k = 0; k < s->b.n_blocks; ++k) lane_inflate(s->b, k, T);
    for (int64_t k = 0; k < s->b.n_blocks; ++k) {
        const DevBlock blk = s->b.blocks[k];
        uint32_t reg = 0;
        if (!s->b.verdict[k]) for (uint32_t lane = 0; lane < WAVE; ++lane) reg ^= crc_lane(s->b.img + s->b.carry_len + blk.out_off, blk.out_len, lane, tab);
        lane_crc_verdict(s->b, k, reg);
    }
    return AMP_OK;
}
#endif

static int bam_ensure(amp_bam *s, int64_t n_img, int64_t n_blocks, int64_t n_comp) {
    CODEC_OK(codec_grow(s->sh, &s->img, &s->cap_img, (size_t)n_img + 64));
    CODEC_OK(codec_grow(s->sh, &s->comp, &s->cap_comp, (size_t)n_comp + 64));
    if (!s->arena || n_img > s->arena_img || n_blocks > s->arena_blocks) {      // pieces of a run have one size: grown once, then reused
        const int64_t ci = n_img > s->arena_img ? n_img + n_img / 8 + 4096 : s->arena_img;
        const int64_t cb = n_blocks > s->arena_blocks ? n_blocks + n_blocks / 8 + 64 : s->arena_blocks;
        Buf probe = s->b;
        const size_t need = carve(probe, nullptr, ci, cb);
        CODEC_OK(codec_grow(s->sh, &s->arena, &s->cap_arena, need));
        (void)carve(s->b, s->arena, ci, cb);
        s->arena_img = ci; s->arena_blocks = cb;
    }
    s->b.img = s->img; s->b.comp = s->comp;
    return AMP_OK;
}

// walk, blind rounds, decode, the counters' way down: everything behind the CRC verdicts, enqueued without waiting
static int bam_index_decode(amp_bam *s) {
    Buf &b = s->b;
    const int64_t S = b.n_stretch, R = b.rec_cap;
    CODEC_OK(codec_zero(s->sh, &b.ctl[CTL_SETTLED], 0, (CTL_WORDS - CTL_SETTLED) * 8));
    CODEC_OK(codec_zero(s->sh, b.cig_off32, 0, 4));
    CODEC_OK(codec_zero(s->sh, b.seq_off8, 0, 4));
    CODEC_OK(codec_zero(s->sh, b.s_row, 0, (size_t)R * 4));
    CODEC_OK(codec_zero(s->sh, b.s_ncig, 0, (size_t)R * 4));
    CODEC_OK(codec_zero(s->sh, b.s_slots, 0, (size_t)R * 4));
    if (S > 0) CODEC_RUN(s, k_bam_walk, lane_walk, S, -1);
    return AMP_OK;
}
static int bam_rounds(amp_bam *s, int rounds) {
    Buf &b = s->b;
    const int64_t S = b.n_stretch;
    if (S <= 0) return AMP_OK;
    int K = 1;
    while ((1ll << K) < S) ++K;
    for (int r = 0; r < rounds; ++r) {
        CODEC_RUN(s, k_bam_link, lane_link, S, -1);
        for (int k = 0; k <= K; ++k) {
            CODEC_RUN(s, k_bam_jump, lane_jump, S, -1);
            uint32_t *t = b.ja; b.ja = b.jb; b.jb = t;
        }
        CODEC_RUN(s, k_bam_settle, lane_settle, S, -1);
    }
    return AMP_OK;
}
static int bam_decode(amp_bam *s) {
    Buf &b = s->b;
    const int64_t S = b.n_stretch, R = b.rec_cap;
    if (S > 0) {
        CODEC_RUN(s, k_bam_counts, lane_counts, S, -1);
        CODEC_OK(codec_scan(s->sh, b.s_cnt, S));
        CODEC_RUN(s, k_bam_emit, lane_emit, S, -1);
        CODEC_OK(codec_scan(s->sh, b.s_row, R));
        CODEC_OK(codec_scan(s->sh, b.s_ncig, R));
        CODEC_OK(codec_scan(s->sh, b.s_slots, R));
        CODEC_RUN(s, k_bam_rows, lane_rows, R, CTL_NREC);
        CODEC_RUN(s, k_bam_pack, lane_pack, b.n_img / 8 + R, CTL_NSLOTS);
    }
    CODEC_RUN(s, k_bam_slack, lane_slack, 1, -1);
    return AMP_OK;
}

// waits for the piece (once on the ordinary path) and fills the info
static int bam_finish(amp_bam *s, amp_bam_info *info) {
    Buf &b = s->b;
    const unsigned long long *c = s->h_ctl;
    CODEC_OK(bam_rounds(s, BLIND_ROUNDS));
    codec_mark(s->sh, 4);
    CODEC_OK(bam_decode(s));
    codec_mark(s->sh, 5);
    for (;;) {
        CODEC_OK(codec_down(s->sh, s->h_ctl, b.ctl, CTL_WORDS * 8));
        CODEC_OK(codec_wait(s->sh));
        if (c[CTL_REFUSED] || c[CTL_SETTLED] || b.n_stretch <= 0) break;
        CODEC_OK(bam_rounds(s, BLIND_ROUNDS));                    // an index that has not settled: more rounds, another wait
        CODEC_OK(bam_decode(s));
    }
    amp_bam_info &I = s->info;
    I.n_refused = (int64_t)c[CTL_REFUSED]; I.index_rounds = (int64_t)c[CTL_ROUNDS]; I.waits = s->sh.waits;
    s->refused_left = I.n_refused;
    I.n_records = I.n_rows = I.n_cig = I.n_bases = I.n_bases_padded = 0; I.bad_record = 0;
    I.carry_out = 0; I.next_first = 0;
    if (!I.n_refused) {
        if (b.n_stretch <= 0) {                                  // the first record starts behind this image (a long header)
            I.next_first = b.o0 - b.n_img;
        } else {
            I.bad_record = c[CTL_BAD] ? 1 : 0;
            I.n_records = (int64_t)c[CTL_NREC]; I.n_rows = (int64_t)c[CTL_NROWS]; I.n_cig = (int64_t)c[CTL_NCIG];
            I.n_bases = (int64_t)c[CTL_NBASES]; I.n_bases_padded = (int64_t)c[CTL_NSLOTS] * 8;
            I.carry_out = b.n_img - (int64_t)c[CTL_CARRY];
            // the tail behind the last complete record opens the next image (a device-to-device copy of less than one record)
            CODEC_OK(codec_grow(s->sh, &s->carry, &s->cap_carry, (size_t)I.carry_out + 64));
            CODEC_OK(codec_d2d(s->sh, s->carry, b.img + (int64_t)c[CTL_CARRY], (size_t)I.carry_out));
        }
        s->carry_len = I.carry_out;
    }
    if (info) *info = I;
    return AMP_OK;
}

extern "C" {

// libampbam's reader of one run (ampbam_open_range_at + ampbam_decode; pysam's iteration at A:296-324, A:896, A:902)
int amp_bam_create(amp_ctx *ctx, amp_bam **out) { return codec_new(ctx, out, AMP_BAM_N_STAGES, k_bam_first_bad); }

void amp_bam_destroy(amp_bam *s) {
    if (!s) return;
    DevGuard guard(s->sh);
    (void)codec_wait(s->sh);
    codec_free(s->arena); codec_free(s->img); codec_free(s->comp); codec_free(s->carry); ampbamout::tail_free(s->tail);
    codec_free(s->text.names); codec_free(s->text.name_off); codec_free(s->text.arena); codec_free(s->text.out);
    codec_delete(s);
}

// ampbam_open_range_at for one piece of whole BGZF blocks: inflate, CRC, record index; and ampbam_decode of its records
int amp_bam_feed(amp_bam *s, const uint8_t *comp, int64_t n_comp, const amp_bam_block *blocks, int64_t n_blocks, int64_t first_off,
                 int32_t n_ref, int64_t rec_base, amp_bam_info *info) {
    if (!s || !info || n_comp < 0 || n_blocks < 0 || (n_comp && !comp) || (n_blocks && !blocks) || n_ref < 0 || n_comp >= (1ll << 31)) return AMP_EINVAL;
    DevGuard guard(s->sh);
    s->fed = s->processed = s->encoded = s->text.checked = false;
    const int64_t waits0 = s->sh.waits;
    int64_t isize = 0;
    try { s->h_blocks.resize((size_t)n_blocks); s->h_verdict.assign((size_t)n_blocks, 0); } catch (const std::bad_alloc &) { return AMP_ENOMEM; }
    for (int64_t k = 0; k < n_blocks; ++k) {
        const amp_bam_block &x = blocks[k];
        if ((int64_t)x.in_off + (int64_t)x.in_len > n_comp || x.out_len > 65536u) return AMP_EINVAL;
        if (isize + (int64_t)x.out_len > IMAGE_LIMIT) return AMP_EOVERFLOW;
        s->h_blocks[(size_t)k] = DevBlock{x.in_off, x.in_len, (uint32_t)isize, x.out_len, x.crc};
        isize += x.out_len;
    }
    const int64_t carry_len = first_off >= 0 ? 0 : s->carry_len;
    const int64_t n_img = carry_len + isize;
    if (n_img > IMAGE_LIMIT) return AMP_EOVERFLOW;
    CODEC_OK(bam_ensure(s, n_img > 0 ? n_img : 1, n_blocks > 0 ? n_blocks : 1, n_comp > 0 ? n_comp : 1));
    Buf &b = s->b;
    b.n_blocks = n_blocks; b.force_refuse = s->force_refuse; s->force_refuse = -1;
    b.n_img = n_img; b.carry_len = carry_len; b.o0 = first_off >= 0 ? first_off : 0; b.n_ref = n_ref; b.rec_base = rec_base;
    b.t0 = b.o0 / BAM_STRETCH; b.n_stretch = b.o0 < n_img ? (n_img + BAM_STRETCH - 1) / BAM_STRETCH : 0; b.rec_cap = rec_cap_for(n_img);
    amp_bam_info z{};
    z.n_blocks = n_blocks; z.n_inflated = isize; z.image_bytes = n_img; z.carry_in = carry_len;
    z.bytes_up = n_comp + n_blocks * (int64_t)sizeof(DevBlock);
    s->info = z;
    codec_mark(s->sh, 0);
    CODEC_OK(codec_up(s->sh, (void *)b.comp, comp, (size_t)n_comp));
    CODEC_OK(codec_up(s->sh, (void *)b.blocks, s->h_blocks.data(), (size_t)n_blocks * sizeof(DevBlock)));
    CODEC_OK(codec_d2d(s->sh, b.img, s->carry, (size_t)carry_len));
    CODEC_OK(codec_zero(s->sh, b.img + n_img, 0, 64));
    CODEC_OK(codec_zero(s->sh, b.ctl, 0, CTL_WORDS * 8));
    codec_mark(s->sh, 1);
    CODEC_OK(bam_inflate_crc(s));
    codec_mark(s->sh, 3);
    CODEC_OK(bam_index_decode(s));
    CODEC_OK(bam_finish(s, nullptr));
    s->info.waits = s->sh.waits - waits0;
    *info = s->info;
    s->fed = true;
    return AMP_OK;
}

// development aid: the next feed treats block k of its piece as refused although it inflates (the fallback's test)
int amp_bam_dev_refuse(amp_bam *s, int64_t k) {
    if (!s) return AMP_EINVAL;
    s->force_refuse = k;
    return AMP_OK;
}

// the numbers of the blocks the last feed refused (at most cap of them; *n = how many there are)
int amp_bam_refused(amp_bam *s, int64_t *idx, int64_t cap, int64_t *n) {
    if (!s || !n || cap < 0 || (cap && !idx)) return AMP_EINVAL;
    if (!s->fed) return AMP_ESTATE;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, s->h_verdict.data(), s->b.verdict, s->h_verdict.size()));
    CODEC_OK(codec_wait(s->sh));
    int64_t m = 0;
    for (size_t k = 0; k < s->h_verdict.size(); ++k) if (s->h_verdict[k]) { if (m < cap) idx[m] = (int64_t)k; ++m; }
    *n = m;
    return AMP_OK;
}

// why: one byte per block of the last feed as the kernels left it -- 0 accepted, 1 refused by the decoder, 2 by the CRC (tests)
int amp_bam_verdicts(amp_bam *s, uint8_t *verdict, int64_t cap) {
    if (!s || cap < 0 || (cap && !verdict)) return AMP_EINVAL;
    if (!s->fed) return AMP_ESTATE;
    if (cap < (int64_t)s->h_blocks.size()) return AMP_EOVERFLOW;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, verdict, s->b.verdict, s->h_blocks.size()));
    return codec_wait(s->sh);
}

// the bytes of block k as the host inflated them (ampbam_inflate_raw / zlib, CRC checked by the caller) into the image
int amp_bam_patch_block(amp_bam *s, int64_t k, const uint8_t *bytes, int64_t n_bytes) {
    if (!s || k < 0 || n_bytes < 0 || (n_bytes && !bytes)) return AMP_EINVAL;
    if (!s->fed || k >= (int64_t)s->h_blocks.size() || !s->h_verdict[(size_t)k]) return AMP_ESTATE;
    const DevBlock &blk = s->h_blocks[(size_t)k];
    if (n_bytes != (int64_t)blk.out_len) return AMP_EINVAL;
    DevGuard guard(s->sh);
    CODEC_OK(codec_up(s->sh, s->b.img + s->b.carry_len + blk.out_off, bytes, (size_t)n_bytes));
    CODEC_OK(codec_wait(s->sh));
    s->h_verdict[(size_t)k] = 0;
    --s->refused_left;
    return AMP_OK;
}

// record index and decode again, once every refused block has been patched
int amp_bam_reindex(amp_bam *s, amp_bam_info *info) {
    if (!s || !info) return AMP_EINVAL;
    if (!s->fed || s->refused_left != 0) return AMP_ESTATE;
    DevGuard guard(s->sh);
    s->text.checked = false;
    const int64_t waits0 = s->info.waits, w0 = s->sh.waits;
    CODEC_OK(codec_zero(s->sh, s->b.ctl, 0, CTL_WORDS * 8));
    CODEC_OK(bam_index_decode(s));
    CODEC_OK(bam_finish(s, nullptr));
    s->info.waits = waits0 + (s->sh.waits - w0);
    *info = s->info;
    return AMP_OK;
}

// the batch of the last feed as the read pass takes it
int amp_bam_reads(amp_bam *s, amp_dev_reads *out) {
    if (!s || !out) return AMP_EINVAL;
    if (!s->fed || s->info.n_refused) return AMP_ESTATE;
    *out = codec_reads(s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded);
    return AMP_OK;
}

// ampbam_decode's batch copied to the host, 16 bytes of slack behind cig, seq and qual included: tests and tools
int amp_bam_batch_to_host(amp_bam *s, const amp_reads *dst, int64_t *src_index) {
    if (!s || !dst) return AMP_EINVAL;
    if (!s->fed || s->info.n_refused) return AMP_ESTATE;
    return codec_batch_to_host(s->sh, s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, dst, src_index, 16);
}

// the image of the last feed ([carry | inflated blocks], image_bytes of them) and the offsets of its records: tests, tools, and
// what a device re-encoder of trimmed records would start from
int amp_bam_image_to_host(amp_bam *s, uint8_t *image, int64_t image_cap, uint32_t *rec_off, int64_t rec_cap) {
    if (!s || image_cap < 0 || rec_cap < 0) return AMP_EINVAL;
    if (!s->fed) return AMP_ESTATE;
    DevGuard guard(s->sh);
    if (image) { if (image_cap < s->b.n_img) return AMP_EOVERFLOW; CODEC_OK(codec_down(s->sh, image, s->b.img, (size_t)s->b.n_img)); }
    if (rec_off) { if (rec_cap < s->info.n_records) return AMP_EOVERFLOW; CODEC_OK(codec_down(s->sh, rec_off, s->b.rec_off, (size_t)s->info.n_records * 4)); }
    return codec_wait(s->sh);
}

#ifndef AMPBGZF_HOSTSIM
// A:896-915 for the rows of the piece: amp_process_batch_device on the batch where it lies, results kept in s
int amp_bam_process(amp_bam *s, uint64_t read_base, int64_t *first_bad_row, uint8_t *its_status) {
    if (!s) return AMP_EINVAL;
    if (!s->fed || s->info.n_refused || s->info.bad_record) return AMP_ESTATE;
    int64_t bad = -1;
    CODEC_OK(codec_process(s->sh, s->b, s->trim, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, read_base, 6, &bad, its_status));
    s->good_rows = bad >= 0 ? bad : s->info.n_rows;
    s->processed = true;
    if (first_bad_row) *first_bad_row = bad;
    return AMP_OK;
}

// milliseconds of the stages of the last feed / process / encode on the ctx stream (HIP events); on != 0 switches the events on
int amp_bam_stage_ms(amp_bam *s, int on, float *ms) { return s ? codec_stage_ms(s->sh, on, ms) : AMP_EINVAL; }
#endif

}  // extern "C"

#include "amp_bamout.hip"
#include "amp_bamtext.hip"
