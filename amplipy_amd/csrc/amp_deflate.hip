// amp_deflate.hip -- DEFLATE encoder for the BGZF blocks of the trimmed BAM (include/amplihip.h: amp_deflate_blocks).
//
// One workgroup per chunk of at most 0xFF00 bytes, the chunk resident in LDS.  The work is a fixed list of phases with a
// workgroup barrier between two phases and no other dependency between threads:
//
//   load      the chunk into LDS; match table, histograms cleared
//   insert    the chunk is cut into segments of SEG = 124 bytes.  Every segment owns ROW = 128 one-byte slots of the match
//             table: slot [hash of 4 bytes][segment] = offset in the segment of the LAST position with that hash.  One lane fills
//             one segment's slots in position order, so the table does not depend on scheduling: the streams are reproducible.
//   scout     lane k parses the last SCOUT = 32 bytes of segment k (greedy with one step of lazy evaluation) and notes where its
//             last token would end: E[k + 1], up to SEG - 1 bytes into the next segment
//   parse     lane k parses [E[k], E[k + 1]) for good: tokens to global scratch, literal/length and distance histograms in LDS.
//             A match candidate for position p is looked up in the slots of p's own segment and of the KWIN - 1 segments in front
//             of it (a window of 4 KiB), plus distance 1; every candidate is verified against the bytes in LDS.
//   codes     dynamic Huffman codes: symbols ranked by frequency in parallel, the two-queue merge by one lane per alphabet
//             (literal/length, distance; then the code-length alphabet), every leaf walks to its root for its depth; a tree
//             deeper than 15 / 15 / 7 is built again from halved frequencies; code lengths sent with the run codes 16 / 17 / 18
//   size      bits per lane, prefix sum; a stream that would not fit `room`, or is not smaller than a stored block, becomes a
//             stored block (or out_len = 0 when even that does not fit)
//   emit      every lane writes its tokens at its own bit offset into a zeroed LDS image (LDS atomic OR: neighbours share
//             words), one lane the block header, one the end-of-block code
//   store     the image, or the stored block, to global memory: never a byte beyond out + k * stride + room
//
// Every loop is bounded by the chunk length or a constant; workgroups do not wait for each other.
// The phase functions compile for the host as well (atomics become plain updates): run thread after thread, phase after phase
// (-DAMPDF_HOSTSIM: host_deflate), they produce the same streams, which is how the encoder was checked against zlib without a
// device.  The library itself has no host path: amp_deflate_blocks needs the GPU.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "../../include/amplihip.h"

namespace ampdf {

constexpr int BS_MAX = 0xFF00;                       // bytes of a chunk at most
constexpr int SEG = 124;                             // bytes of a segment (31 dwords: lanes that walk their segments in step hit different banks)
constexpr int NSEG_MAX = (BS_MAX + SEG - 1) / SEG;   // 527
constexpr int THREADS = 576;                         // nine waves; threads NSEG_MAX.. have no segment (two of them write header and end-of-block)
constexpr int ROW = 128;                             // table slots of a segment
constexpr int KWIN = 32;                             // segments searched: a window of 32 * 124 bytes
constexpr int TROW = KWIN + ((NSEG_MAX + 3) & ~3);   // bytes of a table row: one hash value's slots of all segments behind KWIN empty ones
constexpr int TOK_MAX = 256;                         // tokens of a lane at most (a lane covers at most 2 * SEG - 1 bytes)
constexpr int MIN_MATCH = 4, MAX_MATCH = 258;
constexpr int SCOUT = 32;                            // bytes at a segment's end that the scout parses (measured: 16 bytes lose 0.4 %
                                                     // of the stream size against the whole segment, 32 bytes 0.2 %, 48 bytes 0.1 %)
constexpr int NICE_MATCH = 64;                       // a match this long is taken without looking at the next position
constexpr int NL = 288, ND = 32, NC = 19;            // alphabet sizes (padded)
constexpr int T_HEADER = THREADS - 1, T_EOB = THREADS - 2, T_DIST = 64;
static_assert(NSEG_MAX <= THREADS - 2, "two threads without a segment are needed");
static_assert(2 * SEG - 1 <= TOK_MAX, "token slots of a lane");
static_assert(KWIN * SEG < 32768, "distances must fit DEFLATE's window");

enum { MODE_NONE = 0, MODE_STORED = 1, MODE_HUFF = 2 };

struct Shared {
    uint32_t data[(BS_MAX + 32) / 4];                // the chunk, at byte offset `skew` (the source's misalignment); match_len reads up to 22 bytes past it
    uint32_t tab[ROW * TROW / 4 + 2];                // match table (one byte per slot), [hash][segment]; later the image of the stream
    uint32_t hist_l[NL], hist_d[ND], hist_c[NC + 1];
    uint32_t code_l[NL], code_d[ND], code_c[NC + 1];  // bit-reversed code | length << 16
    uint32_t weight[2 * NL + 2 * ND];                // Huffman construction (literal/length nodes, then distance nodes)
    uint16_t parent[2 * NL + 2 * ND];
    uint16_t order_l[NL], order_d[ND], order_c[NC + 1];
    uint8_t depth[2 * NL + 2 * ND];
    uint8_t len_l[NL], len_d[ND], len_c[NC + 1];
    uint16_t clseq[NL + ND];                          // code-length symbols: symbol | extra bits' value << 8
    uint16_t seg_end[NSEG_MAX + 1];                   // E[]
    uint16_t ntok[THREADS];
    uint32_t lane_bits[THREADS];
    uint32_t lane_off[THREADS];
    uint32_t used_l, used_d, used_c, n_cl, hlit, hdist, hclen, overflow, deep_l, deep_d;
    uint32_t header_bits, body_bits, total_bytes, mode;
};
static_assert(sizeof(Shared) <= 160 * 1024, "LDS of a gfx950 compute unit");

struct Args {
    const uint8_t *in;
    int64_t n_bytes;
    int32_t block_bytes;
    uint8_t *out;
    int64_t stride;
    int32_t room;
    uint32_t *out_len;
    uint32_t *tokens;                                 // [gridDim.x][TOK_MAX][THREADS]
    const unsigned long long *n_dev;                  // not NULL: n_bytes is read from here by the kernel (at most the n_bytes above)
};

#define AMPDF_FN __host__ __device__ static inline

AMPDF_FN void add_u32(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
AMPDF_FN void or_u32(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// four bytes at any byte offset of a dword array (two aligned reads)
AMPDF_FN uint32_t rd4(const uint32_t *w, int at) {
    const uint32_t lo = w[at >> 2], hi = w[(at >> 2) + 1];
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (at & 3)));
}
AMPDF_FN uint32_t rd1(const uint32_t *w, int at) { return (w[at >> 2] >> (8 * (at & 3))) & 0xFFu; }
// eight hash bits of four bytes: seven choose the slot (ROW), the eighth is kept in the slot next to the position's offset
// in its segment (seven bits; 0xFF = empty) and spares half of the look-ups that would find other bytes
AMPDF_FN uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> 24; }
static_assert(ROW == 128 && SEG < 127 && KWIN == 32 && TROW % 4 == 0, "layout of a slot and of a row");

// bytes that agree at a and b (a < b), at most maxl: sixteen bytes a turn (the loads of a turn do not wait for each other; a
// turn costs one round trip to the LDS however wide it is)
AMPDF_FN int match_len(const uint32_t *d, int a, int b, int maxl) {
    int l = 0;
    while (l < maxl) {
        const uint32_t *pa = d + ((a + l) >> 2), *pb = d + ((b + l) >> 2);
        const int sa = 8 * ((a + l) & 3), sb = 8 * ((b + l) & 3);
        uint32_t wa[5], wb[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) { wa[i] = pa[i]; wb[i] = pb[i]; }
        int same = 16;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const uint32_t x = (uint32_t)(((((uint64_t)wa[i + 1]) << 32) | wa[i]) >> sa) ^ (uint32_t)(((((uint64_t)wb[i + 1]) << 32) | wb[i]) >> sb);
            if (x) same = 4 * i + (__builtin_ctz(x) >> 3);
        }
        l += same;
        if (same < 16) break;
    }
    return l < maxl ? l : maxl;
}

// the longest match for position p (chunk-relative) that ends at or before `lim`; 0 when there is none of MIN_MATCH bytes
AMPDF_FN int find_match(const Shared &sh, int skew, int n, int p, int lim, int *dist) {
    const int maxl = lim - p < MAX_MATCH ? lim - p : MAX_MATCH;
    if (maxl < MIN_MATCH || p + 4 > n) return 0;
    const uint32_t *d = sh.data;
    const uint32_t v = rd4(d, skew + p);
    const uint32_t hv = hash4(v), tag = (hv & 1) << 7;
    const int w = p / SEG;
    // the slots of segments w - 31 .. w for this hash value are 32 consecutive bytes of the table: all read at once, and the first
    // four bytes of every candidate too (loads that do not depend on each other), before any match is extended
    const int at = (int)(hv >> 1) * TROW + w + 1;
    const uint32_t *t = sh.tab + (at >> 2);
    const int sft = 8 * (at & 3);
    uint32_t hit = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t four = (uint32_t)(((((uint64_t)t[i + 1]) << 32) | t[i]) >> sft);
        // four slots at once: bit 7 of a byte of `bad` is set when the slot's tag differs or its offset is not below SEG (empty)
        const uint32_t bad = ((four ^ (tag * 0x01010101u)) | ((four & 0x7F7F7F7Fu) + (uint32_t)(128 - SEG) * 0x01010101u)) & 0x80808080u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * i + b;
            const int q = (w - (KWIN - 1) + j) * SEG + (int)((four >> (8 * b)) & 0x7Fu);
            bool ok = !(bad & (0x80u << (8 * b)));
            if (j == KWIN - 1) ok = ok && q < p;          // only the position's own segment holds later positions
            const uint32_t x = rd4(d, skew + (ok ? q : p));
            hit |= (uint32_t)(ok && x == v) << j;
        }
    }
    int best = 0, bd = 0;
    while (hit) {                                         // nearest segment first
        const int j = 31 - __builtin_clz(hit);
        hit &= ~(1u << j);
        const int q = (w - (KWIN - 1) + j) * SEG + (int)(rd1(sh.tab, at + j) & 0x7Fu);
        if (best >= MIN_MATCH && rd1(d, skew + q + best) != rd1(d, skew + p + best)) continue;      // cannot be longer
        const int l = 4 + match_len(d, skew + q + 4, skew + p + 4, maxl - 4);
        if (l > best) { best = l; bd = p - q; }
    }
    if (p > 0 && rd1(d, skew + p - 1) == (v & 0xFFu)) {                                             // a run
        const int l = match_len(d, skew + p - 1, skew + p, maxl);
        if (l > best || (l == best && l)) { best = l; bd = 1; }
    }
    *dist = bd;
    return best >= MIN_MATCH ? best : 0;
}

AMPDF_FN void len_symbol(int len, int *sym, int *ebits, int *eval) {
    const int l3 = len - 3;
    if (l3 < 8) { *sym = 257 + l3; *ebits = 0; *eval = 0; return; }
    if (len == MAX_MATCH) { *sym = 285; *ebits = 0; *eval = 0; return; }
    const int eb = (31 - __builtin_clz((unsigned)l3)) - 2;
    *sym = 257 + 4 * eb + 4 + ((l3 >> eb) & 3); *ebits = eb; *eval = l3 & ((1 << eb) - 1);
}
AMPDF_FN void dist_symbol(int dist, int *sym, int *ebits, int *eval) {
    const int d1 = dist - 1;
    if (d1 < 4) { *sym = d1; *ebits = 0; *eval = 0; return; }
    const int b = 31 - __builtin_clz((unsigned)d1);
    *sym = 2 * b + ((d1 >> (b - 1)) & 1); *ebits = b - 1; *eval = d1 & ((1 << (b - 1)) - 1);
}

// Greedy parse with one step of lazy evaluation of [p, stop): tokens start in front of `stop` and end at or before `lim`.
// KEEP: tokens go to tok[i * THREADS] and into the histograms.  Returns where the last token ended; *n_tok = tokens.
template <bool KEEP>
AMPDF_FN int parse(Shared &sh, int skew, int n, int p, int stop, int lim, uint32_t *tok, int *n_tok) {
    int nt = 0, len = 0, dist = 0;
    bool pending = false;                                 // a match (len, dist) at p waits for the look at p + 1
    // one look-up per turn of the loop, for every lane of the wave alike: at p, or at p + 1 behind a pending match
    while (p < stop) {
        int d2 = 0;
        const int l2 = find_match(sh, skew, n, pending ? p + 1 : p, lim, &d2);
        bool literal;
        if (!pending) {
            len = l2; dist = d2;
            if (len && len < NICE_MATCH && p + 1 < stop) { pending = true; continue; }
            literal = len == 0;
        } else {
            literal = l2 > len;
            if (literal) { len = l2; dist = d2; pending = len < NICE_MATCH && p + 2 < stop; }      // the better match, at p + 1, waits in its turn
            else pending = false;
        }
        if (literal) {
            if (KEEP) {
                const uint32_t b = rd1(sh.data, skew + p);
                if (nt < TOK_MAX) tok[(size_t)nt * THREADS] = b; else sh.overflow = 1;
                add_u32(&sh.hist_l[b], 1);
            }
            p += 1; ++nt;
            if (pending || len == 0) continue;
            // the match behind the literal is taken as it is
        }
        if (KEEP) {
            int s, eb, ev;
            if (nt < TOK_MAX) tok[(size_t)nt * THREADS] = 0x80000000u | ((uint32_t)len << 16) | (uint32_t)(dist - 1); else sh.overflow = 1;
            len_symbol(len, &s, &eb, &ev); add_u32(&sh.hist_l[s], 1);
            dist_symbol(dist, &s, &eb, &ev); add_u32(&sh.hist_d[s], 1);
        }
        p += len; ++nt; len = 0;
    }
    *n_tok = nt;
    return p;
}

// rank of symbol i among the used symbols of an alphabet by (frequency, symbol): order[rank] = i
AMPDF_FN void rank_symbol(const uint32_t *freq, int n, int i, uint16_t *order, uint32_t *weight, uint32_t *used) {
    const uint32_t f = freq[i];
    if (!f) return;
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const uint32_t g = freq[j];
        r += (g && (g < f || (g == f && j < i))) ? 1 : 0;
    }
    order[r] = (uint16_t)i; weight[r] = f;
    add_u32(used, 1);
}

// Huffman tree over the m >= 2 leaves weight[0..m) (ascending): the two-queue merge.  Node m + t is made by the t-th merge, the
// root is node 2m - 2; parent[] of every other node is set.  One lane; the heads of both queues are kept in registers.
AMPDF_FN void merge_tree(int m, uint32_t *weight, uint16_t *parent) {
    uint32_t wa = weight[0], wb = 0xFFFFFFFFu;
    int ia = 0, ib = m;                                   // next leaf, next internal node not yet merged
    for (int t = 0; t < m - 1; ++t) {
        const int node = m + t;
        uint32_t sum = 0;
        for (int two = 0; two < 2; ++two) {
            if (ia < m && (ib >= node || wa <= wb)) { sum += wa; parent[ia] = (uint16_t)node; ++ia; wa = ia < m ? weight[ia] : 0xFFFFFFFFu; }
            else { sum += wb; parent[ib] = (uint16_t)node; ++ib; wb = ib < node ? weight[ib] : 0xFFFFFFFFu; }
        }
        weight[node] = sum;
        if (ib == node) wb = sum;                         // the queue of internal nodes was empty: the new node is its head
    }
}

// depth of leaf i of that tree: the walk to the root (bounded: a tree over at most 2^17 counts is less than 32 deep)
AMPDF_FN int leaf_depth(int m, const uint16_t *parent, int i) {
    int x = i, dl = 0;
    const int root = 2 * m - 2;
    while (x != root && dl < 64) { x = parent[x]; ++dl; }
    return dl;
}

// Huffman code lengths of the m >= 2 used symbols order[0..m) (ascending frequency), no longer than max_bits, by one lane alone:
// a tree that is too deep is built again from halved frequencies (the halving keeps the order), starting with freq >> shift0.
AMPDF_FN void build_lengths(const uint32_t *freq, const uint16_t *order, int m, int max_bits, int shift0, uint32_t *weight, uint16_t *parent, uint8_t *depth, uint8_t *len) {
    for (int shift = shift0; shift < 32; ++shift) {
        for (int i = 0; i < m; ++i) { const uint32_t f = freq[order[i]] >> shift; weight[i] = f ? f : 1; }
        merge_tree(m, weight, parent);
        const int root = 2 * m - 2;
        depth[root] = 0;
        for (int i = root - 1; i >= m; --i) depth[i] = (uint8_t)(depth[parent[i]] + 1);
        int deepest = 0;
        for (int i = 0; i < m; ++i) { const int dl = depth[parent[i]] + 1; depth[i] = (uint8_t)dl; deepest = dl > deepest ? dl : deepest; }
        if (deepest <= max_bits) break;
    }
    for (int i = 0; i < m; ++i) len[order[i]] = depth[i];
}

// canonical code of symbol i (RFC 1951 3.2.2), bit-reversed for an LSB-first stream, with its length in bits 16..
AMPDF_FN uint32_t canonical(const uint8_t *len, int n, int i) {
    const int L = len[i];
    if (!L) return 0;
    uint32_t code = 0;
    for (int j = 0; j < n; ++j) {
        const int lj = len[j];
        if (lj && lj < L) code += 1u << (L - lj);
        else if (lj == L && j < i) code += 1;
    }
    return (__builtin_bitreverse32(code) >> (32 - L)) | ((uint32_t)L << 16);
}

struct BitWriter {                                       // into the zeroed LDS image; words are shared with the neighbours
    uint32_t *img; uint64_t acc; int nb; uint32_t word;
    __host__ __device__ void start(uint32_t *image, uint32_t bit) { img = image; acc = 0; nb = (int)(bit & 31); word = bit >> 5; }
    __host__ __device__ void put(uint32_t v, int bits) {  // bits <= 31
        acc |= (uint64_t)v << nb; nb += bits;
        if (nb >= 32) { or_u32(&img[word], (uint32_t)acc); ++word; acc >>= 32; nb -= 32; }
    }
    __host__ __device__ void code(uint32_t c) { put(c & 0xFFFFu, (int)(c >> 16)); }
    __host__ __device__ void finish() { if (nb) or_u32(&img[word], (uint32_t)acc); }
};

constexpr int N_PHASES = 17;
// the order in which the lengths of the code-length code are sent (RFC 1951 3.2.7), five bits an entry
constexpr uint64_t pack5(const int *v, int n) { uint64_t r = 0; for (int i = 0; i < n; ++i) r |= (uint64_t)v[i] << (5 * i); return r; }
constexpr int CLEN_A[12] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4}, CLEN_B[7] = {12, 3, 13, 2, 14, 1, 15};
constexpr uint64_t CLEN_LO = pack5(CLEN_A, 12), CLEN_HI = pack5(CLEN_B, 7);
AMPDF_FN int clen_order(int i) { return (int)(((i < 12 ? CLEN_LO >> (5 * i) : CLEN_HI >> (5 * (i - 12)))) & 31); }

// phase P of chunk `blk` for thread `tid` of workgroup `wg`
template <int P>
AMPDF_FN void phase(Shared &sh, const Args &a, int64_t blk, int wg, int tid) {
    const int64_t off = blk * (int64_t)a.block_bytes;
    const int n = (int)(a.n_bytes - off < a.block_bytes ? a.n_bytes - off : a.block_bytes);
    const uint8_t *src = a.in + off;
    const int skew = (int)((uintptr_t)src & 3);
    const int nseg = (n + SEG - 1) / SEG;
    uint32_t *tok = a.tokens + (size_t)wg * TOK_MAX * THREADS + tid;
    if constexpr (P == 0) {                               // ---- load ----
        const uint32_t *s4 = (const uint32_t *)(src - skew);      // aligned dwords that hold at least one byte of the chunk
        const int nw = (skew + n + 3) >> 2;
        for (int i = tid; i < nw; i += THREADS) sh.data[i] = s4[i];
        for (int i = nw + tid; i < (int)(sizeof(sh.data) / 4); i += THREADS) sh.data[i] = 0;
        for (int i = tid; i < (int)(sizeof(sh.tab) / 4); i += THREADS) sh.tab[i] = 0xFFFFFFFFu;
        for (int i = tid; i < NL; i += THREADS) { sh.hist_l[i] = 0; sh.len_l[i] = 0; }
        if (tid < ND) { sh.hist_d[tid] = 0; sh.len_d[tid] = 0; }
        if (tid < NC + 1) { sh.hist_c[tid] = 0; sh.len_c[tid] = 0; }
        if (tid == 0) { sh.used_l = sh.used_d = sh.used_c = 0; sh.overflow = 0; sh.deep_l = sh.deep_d = 0; sh.seg_end[0] = 0; sh.mode = MODE_NONE; }
        sh.ntok[tid] = 0; sh.lane_bits[tid] = 0;
    } else if constexpr (P == 1) {                        // ---- insert ----
        if (tid < nseg) {
            uint8_t *col = (uint8_t *)sh.tab + KWIN + tid;
            const int p0 = tid * SEG, p1 = (p0 + SEG < n - 3 ? p0 + SEG : n - 3);
            for (int p = p0; p < p1; ++p) {
                const uint32_t hv = hash4(rd4(sh.data, skew + p));
                col[(hv >> 1) * TROW] = (uint8_t)((p - p0) | ((hv & 1) << 7));
            }
        }
    } else if constexpr (P == 2) {                        // ---- scout ----
        if (tid < nseg) {
            const int b1 = (tid + 1) * SEG < n ? (tid + 1) * SEG : n;
            const int lim = b1 + SEG - 1 < n ? b1 + SEG - 1 : n;
            int nt;
            const int from = b1 - SCOUT > tid * SEG ? b1 - SCOUT : tid * SEG;
            const int e = parse<false>(sh, skew, n, from, b1, lim, nullptr, &nt);
            sh.seg_end[tid + 1] = (uint16_t)(tid == nseg - 1 ? n : e);
        }
    } else if constexpr (P == 3) {                        // ---- parse ----
        if (tid < nseg) {
            int nt;
            const int e0 = sh.seg_end[tid], e1 = sh.seg_end[tid + 1];
            parse<true>(sh, skew, n, e0, e1, e1, tok, &nt);
            sh.ntok[tid] = (uint16_t)(nt < TOK_MAX ? nt : TOK_MAX);
        }
        if (tid == T_EOB) add_u32(&sh.hist_l[256], 1);
    } else if constexpr (P == 4) {                        // ---- at least two distance codes (a complete code, as zlib sends it) ----
        if (tid == 0) {
            int used = 0;
            for (int i = 0; i < 30; ++i) used += sh.hist_d[i] ? 1 : 0;
            if (used < 2) { if (!sh.hist_d[0]) sh.hist_d[0] = 1; if (!sh.hist_d[1]) sh.hist_d[1] = 1; }
        }
    } else if constexpr (P == 5) {                        // ---- rank by frequency ----
        if (tid < 286) rank_symbol(sh.hist_l, 286, tid, sh.order_l, sh.weight, &sh.used_l);
        else if (tid >= NL && tid < NL + 30) rank_symbol(sh.hist_d, 30, tid - NL, sh.order_d, sh.weight + 2 * NL, &sh.used_d);
    } else if constexpr (P == 6) {                        // ---- the two trees ----
        if (tid == 0) merge_tree((int)sh.used_l, sh.weight, sh.parent);
        if (tid == T_DIST) merge_tree((int)sh.used_d, sh.weight + 2 * NL, sh.parent + 2 * NL);
    } else if constexpr (P == 7) {                        // ---- code lengths: every leaf walks to its root ----
        if (tid < (int)sh.used_l) {
            const int dl = leaf_depth((int)sh.used_l, sh.parent, tid);
            sh.len_l[sh.order_l[tid]] = (uint8_t)dl;
            if (dl > 15) sh.deep_l = 1;
        } else if (tid >= NL && tid < NL + (int)sh.used_d) {
            const int dl = leaf_depth((int)sh.used_d, sh.parent + 2 * NL, tid - NL);
            sh.len_d[sh.order_d[tid - NL]] = (uint8_t)dl;
            if (dl > 15) sh.deep_d = 1;
        }
    } else if constexpr (P == 8) {                        // ---- a tree deeper than 15 (rare): again, from halved frequencies ----
        if (tid == 0 && sh.deep_l) build_lengths(sh.hist_l, sh.order_l, (int)sh.used_l, 15, 1, sh.weight, sh.parent, sh.depth, sh.len_l);
        if (tid == T_DIST && sh.deep_d) build_lengths(sh.hist_d, sh.order_d, (int)sh.used_d, 15, 1, sh.weight + 2 * NL, sh.parent + 2 * NL, sh.depth + 2 * NL, sh.len_d);
    } else if constexpr (P == 9) {                        // ---- codes; the code lengths as run-length symbols ----
        if (tid < 286) sh.code_l[tid] = canonical(sh.len_l, 286, tid);
        else if (tid >= NL && tid < NL + 30) sh.code_d[tid - NL] = canonical(sh.len_d, 30, tid - NL);
        else if (tid == T_HEADER) {
            int hlit = 286, hdist = 30;
            while (hlit > 257 && !sh.len_l[hlit - 1]) --hlit;
            while (hdist > 1 && !sh.len_d[hdist - 1]) --hdist;
            const int total = hlit + hdist;
            int ncl = 0, i = 0;
            while (i < total) {
                const int v = i < hlit ? sh.len_l[i] : sh.len_d[i - hlit];
                int run = 1;
                while (i + run < total && (i + run < hlit ? sh.len_l[i + run] : sh.len_d[i + run - hlit]) == v) ++run;
                int left = run;
                if (v == 0) {
                    while (left >= 11) { const int r = left < 138 ? left : 138; sh.clseq[ncl++] = (uint16_t)(18 | ((r - 11) << 8)); sh.hist_c[18]++; left -= r; }
                    if (left >= 3) { sh.clseq[ncl++] = (uint16_t)(17 | ((left - 3) << 8)); sh.hist_c[17]++; left = 0; }
                } else {
                    sh.clseq[ncl++] = (uint16_t)v; sh.hist_c[v]++; --left;
                    while (left >= 3) { const int r = left < 6 ? left : 6; sh.clseq[ncl++] = (uint16_t)(16 | ((r - 3) << 8)); sh.hist_c[16]++; left -= r; }
                }
                for (; left > 0; --left) { sh.clseq[ncl++] = (uint16_t)v; sh.hist_c[v]++; }
                i += run;
            }
            int used = 0;
            for (int s = 0; s < NC; ++s) used += sh.hist_c[s] ? 1 : 0;
            if (used < 2) { if (!sh.hist_c[0]) sh.hist_c[0] = 1; if (!sh.hist_c[8]) sh.hist_c[8] = 1; }
            sh.n_cl = (uint32_t)ncl; sh.hlit = (uint32_t)hlit; sh.hdist = (uint32_t)hdist;
        }
    } else if constexpr (P == 10) {
        if (tid < NC) rank_symbol(sh.hist_c, NC, tid, sh.order_c, sh.weight, &sh.used_c);
    } else if constexpr (P == 11) {                        // ---- code-length code; bits of every lane ----
        if (tid == T_HEADER) build_lengths(sh.hist_c, sh.order_c, (int)sh.used_c, 7, 0, sh.weight, sh.parent, sh.depth, sh.len_c);
        if (tid < nseg) {
            uint32_t bits = 0;
            const int nt = sh.ntok[tid];
            for (int i = 0; i < nt; ++i) {
                const uint32_t t = tok[(size_t)i * THREADS];
                if (t >> 31) {
                    int s, eb, ev;
                    len_symbol((int)((t >> 16) & 0x1FF), &s, &eb, &ev); bits += sh.len_l[s] + eb;
                    dist_symbol((int)(t & 0xFFFF) + 1, &s, &eb, &ev); bits += sh.len_d[s] + eb;
                } else bits += sh.len_l[t];
            }
            sh.lane_bits[tid] = bits;
        }
    } else if constexpr (P == 12) {                       // ---- bit offsets ----
        if (tid < NC) sh.code_c[tid] = canonical(sh.len_c, NC, tid);
        uint32_t before = 0;
        for (int j = 0; j < nseg; ++j) before += j < tid ? sh.lane_bits[j] : 0;
        sh.lane_off[tid] = before;
        if (tid == T_EOB) sh.body_bits = before;          // T_EOB >= nseg: the sum of all lanes
    } else if constexpr (P == 13) {                       // ---- the block's size; how it is sent ----
        if (tid == 0) {
            int hclen = NC;
            while (hclen > 4 && !sh.len_c[clen_order(hclen - 1)]) --hclen;
            uint32_t hb = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
            for (uint32_t i = 0; i < sh.n_cl; ++i) {
                const int s = sh.clseq[i] & 0xFF;
                hb += sh.len_c[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            const uint32_t bits = hb + sh.body_bits + sh.len_l[256];
            const uint32_t bytes = (bits + 7) >> 3, stored = (uint32_t)n + 5;
            sh.hclen = (uint32_t)hclen; sh.header_bits = hb;
            if (!sh.overflow && bytes < stored && bytes <= (uint32_t)a.room && bytes <= sizeof(sh.tab) - 8) { sh.mode = MODE_HUFF; sh.total_bytes = bytes; }
            else if (stored <= (uint32_t)a.room) { sh.mode = MODE_STORED; sh.total_bytes = stored; }
            else { sh.mode = MODE_NONE; sh.total_bytes = 0; }
        }
    } else if constexpr (P == 14) {                       // ---- a zeroed image ----
        if (sh.mode == MODE_HUFF) for (int i = tid; i < (int)(sh.total_bytes + 11) / 4; i += THREADS) sh.tab[i] = 0;
    } else if constexpr (P == 15) {                       // ---- emit ----
        if (sh.mode != MODE_HUFF) return;
        BitWriter w;
        if (tid < nseg) {
            w.start(sh.tab, sh.header_bits + sh.lane_off[tid]);
            const int nt = sh.ntok[tid];
            for (int i = 0; i < nt; ++i) {
                const uint32_t t = tok[(size_t)i * THREADS];
                if (t >> 31) {
                    int s, eb, ev;
                    len_symbol((int)((t >> 16) & 0x1FF), &s, &eb, &ev); w.code(sh.code_l[s]); w.put((uint32_t)ev, eb);
                    dist_symbol((int)(t & 0xFFFF) + 1, &s, &eb, &ev); w.code(sh.code_d[s]); w.put((uint32_t)ev, eb);
                } else w.code(sh.code_l[t]);
            }
            w.finish();
        } else if (tid == T_EOB) {
            w.start(sh.tab, sh.header_bits + sh.body_bits);
            w.code(sh.code_l[256]);
            w.finish();
        } else if (tid == T_HEADER) {
            w.start(sh.tab, 0);
            w.put(1, 1); w.put(2, 2);                     // final block, dynamic codes
            w.put(sh.hlit - 257, 5); w.put(sh.hdist - 1, 5); w.put(sh.hclen - 4, 4);
            for (uint32_t i = 0; i < sh.hclen; ++i) w.put(sh.len_c[clen_order((int)i)], 3);
            for (uint32_t i = 0; i < sh.n_cl; ++i) {
                const int s = sh.clseq[i] & 0xFF, x = sh.clseq[i] >> 8;
                w.code(sh.code_c[s]);
                if (s >= 16) w.put((uint32_t)x, s == 16 ? 2 : s == 17 ? 3 : 7);
            }
            w.finish();
        }
    } else if constexpr (P == 16) {                       // ---- store ----
        uint8_t *dst = a.out + blk * a.stride;
        const uint32_t total = sh.total_bytes;            // <= room (phase 13)
        if (tid == 0) a.out_len[blk] = total;
        if (sh.mode == MODE_NONE) return;
        // byte i of the stream: image byte i, or (stored) 5 bytes of header and then chunk byte i - 5
        const uint32_t *img = sh.mode == MODE_HUFF ? sh.tab : sh.data;
        const int base = sh.mode == MODE_HUFF ? 0 : skew - 5;
        const uint32_t first = sh.mode == MODE_HUFF ? 0 : 5;
        if (sh.mode == MODE_STORED && tid < 5) {
            const uint32_t v = (uint32_t)n;
            dst[tid] = (uint8_t)(tid == 0 ? 1 : tid == 1 ? v : tid == 2 ? v >> 8 : tid == 3 ? ~v : (~v) >> 8);
        }
        uint32_t lead = (uint32_t)((4 - (((uintptr_t)dst + first) & 3)) & 3);     // bytes in front of the first aligned dword
        if (lead > total - first) lead = total - first;
        const uint32_t nw = (total - first - lead) >> 2, tail0 = first + lead + 4 * nw;
        if ((uint32_t)tid < lead) dst[first + tid] = (uint8_t)rd1(img, base + (int)first + tid);
        uint32_t *d4 = (uint32_t *)(dst + first + lead);
        for (uint32_t i = (uint32_t)tid; i < nw; i += THREADS) d4[i] = rd4(img, base + (int)(first + lead + 4 * i));
        if (tail0 + (uint32_t)tid < total) dst[tail0 + tid] = (uint8_t)rd1(img, base + (int)tail0 + tid);
    }
}

template <int P>
__device__ static inline void run_phases(Shared &sh, const Args &a, int64_t blk) {
    phase<P>(sh, a, blk, (int)blockIdx.x, (int)threadIdx.x);
    __syncthreads();
    if constexpr (P + 1 < N_PHASES) run_phases<P + 1>(sh, a, blk);
}

__global__ __launch_bounds__(THREADS) void k_deflate(Args a, int64_t n_blocks) {
    __shared__ Shared sh;
    if (a.n_dev) {                                        // a byte count that only the device knows: the launch was sized for the most it can be
        const int64_t n = (int64_t)*a.n_dev;
        if (n < a.n_bytes) a.n_bytes = n;
        n_blocks = (a.n_bytes + a.block_bytes - 1) / a.block_bytes;
    }
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) run_phases<0>(sh, a, blk);
}

// The streams of a launch moved together, each on a dword boundary, so that one copy takes them to the host: stream k goes to
// packed + sum of the rounded lengths in front of it.
__global__ __launch_bounds__(256) void k_pack(const uint8_t *out, int64_t stride, const uint32_t *out_len, uint32_t *packed) {
    __shared__ uint32_t before;
    const int k = (int)blockIdx.x;
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    uint32_t part = 0;
    for (int j = (int)threadIdx.x; j < k; j += 256) part += (out_len[j] + 3) >> 2;
    if (part) atomicAdd(&before, part);
    __syncthreads();
    const uint32_t *src = (const uint32_t *)(out + (int64_t)k * stride);      // stride is a multiple of 4
    const uint32_t nw = (out_len[k] + 3) >> 2;
    for (uint32_t i = threadIdx.x; i < nw; i += 256) packed[before + i] = src[i];
}

#ifdef AMPDF_HOSTSIM
template <int P>
static void host_phases(Shared &sh, const Args &a, int64_t blk) {
    for (int tid = 0; tid < THREADS; ++tid) phase<P>(sh, a, blk, 0, tid);
    if constexpr (P + 1 < N_PHASES) host_phases<P + 1>(sh, a, blk);
}
static void host_deflate(Args a, int64_t n_blocks) {
    static Shared sh;
    for (int64_t blk = 0; blk < n_blocks; ++blk) host_phases<0>(sh, a, blk);
}
}  // namespace ampdf
// what the kernel computes, on the host, one chunk after the other: for tests/test_gpu_deflate.py on a machine without a GPU
// (built there into a library of its own; never part of libamplihip.so)
extern "C" int ampdf_hostsim_blocks(const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride, int32_t out_room,
                                    uint32_t *out_len) {
    using namespace ampdf;
    if (n_bytes < 0 || block_bytes < 1 || block_bytes > BS_MAX || out_room < 0 || out_stride < out_room) return AMP_EINVAL;
    if (n_bytes == 0) return AMP_OK;
    static uint32_t tokens[(size_t)TOK_MAX * THREADS];
    host_deflate(Args{in, n_bytes, block_bytes, out, out_stride, out_room, out_len, tokens}, (n_bytes + block_bytes - 1) / block_bytes);
    return AMP_OK;
}
// the code lengths the phases give an alphabet of n symbols with these frequencies: max_bits 7 as phases 10 and 11 build the
// code-length code (build_lengths from the frequencies as they are), max_bits 15 as phases 5 to 8 build the other two (merge_tree,
// every leaf's walk, and build_lengths from halved frequencies only when a leaf is deeper than 15).  For tests/test_deflate_enc_craft.py:
// frequencies that no chunk gives reach the limits here.
extern "C" int ampdf_hostsim_lengths(const uint32_t *freq, int n, int max_bits, uint8_t *len) {
    using namespace ampdf;
    if (!freq || !len || n < 2 || n > 286 || (max_bits != 7 && max_bits != 15) || (max_bits == 7 && n > NC)) return AMP_EINVAL;
    static uint32_t weight[2 * NL];
    static uint16_t parent[2 * NL], order[NL];
    static uint8_t depth[2 * NL];
    uint32_t used = 0;
    for (int i = 0; i < n; ++i) len[i] = 0;
    for (int i = 0; i < n; ++i) rank_symbol(freq, n, i, order, weight, &used);
    if (used < 2) return AMP_EINVAL;
    if (max_bits == 7) { build_lengths(freq, order, (int)used, 7, 0, weight, parent, depth, len); return AMP_OK; }
    merge_tree((int)used, weight, parent);
    bool deep = false;
    for (int i = 0; i < (int)used; ++i) {
        const int dl = leaf_depth((int)used, parent, i);
        len[order[i]] = (uint8_t)dl;
        deep = deep || dl > 15;
    }
    if (deep) build_lengths(freq, order, (int)used, 15, 1, weight, parent, depth, len);
    return AMP_OK;
}
namespace ampdf {
#endif

// ---- host side: one state per device, kept between calls -------------------------------------------------------------------------
constexpr int MAX_DEV = 16;
constexpr int64_t PIECE_BLOCKS = 256;                     // chunks per launch of the host-pointer entry (16 MB of input)
constexpr int N_SLOTS = 2;                                // pieces in flight there

struct Slot {                                             // one piece of the host-pointer entry: its stream and buffers
    hipStream_t stream = nullptr;
    uint8_t *d_in = nullptr, *d_out = nullptr; size_t in_cap = 0, out_cap = 0;
    uint32_t *d_len = nullptr; size_t len_cap = 0;
    uint32_t *d_packed = nullptr; size_t packed_cap = 0;
    uint8_t *h_out = nullptr; size_t h_out_cap = 0;       // page-locked
    uint32_t *h_len = nullptr; size_t h_len_cap = 0;      // page-locked
};

struct DevState {
    std::mutex mu;
    bool init = false;
    int n_cu = 256;
    hipStream_t stream = nullptr;                         // what amp_deflate_blocks_device runs on when it is given none
    Slot slot[N_SLOTS];
    uint32_t *d_tokens = nullptr; int tok_grid = 0;       // token scratch of the encoder kernel: one launch at a time uses it
    hipEvent_t tokens_free = nullptr; bool tokens_used = false;
};
static DevState g_state[MAX_DEV];

static bool grow_dev(void **p, size_t *cap, size_t want) {
    if (*cap >= want) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, want) != hipSuccess) return false;
    *cap = want;
    return true;
}
static bool grow_pinned(void **p, size_t *cap, size_t want) {
    if (*cap >= want) return true;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) return false;
    *cap = want;
    return true;
}

static int grid_for(DevState &st, int64_t n_blocks) { return (int)(n_blocks < st.n_cu ? n_blocks : st.n_cu); }

static int ensure_tokens(DevState &st, int grid) {
    if (st.tok_grid >= grid) return AMP_OK;
    if (st.d_tokens) (void)hipFree(st.d_tokens);
    st.d_tokens = nullptr; st.tok_grid = 0;
    const int want = grid < st.n_cu ? st.n_cu : grid;     // one allocation for the process
    if (hipMalloc((void **)&st.d_tokens, (size_t)want * TOK_MAX * THREADS * sizeof(uint32_t)) != hipSuccess) return AMP_ENOMEM;
    st.tok_grid = want;
    return AMP_OK;
}

static int launch(DevState &st, const uint8_t *d_in, int64_t n_bytes, int32_t block_bytes, uint8_t *d_out, int64_t stride, int32_t room,
                  uint32_t *d_len, hipStream_t s, const unsigned long long *n_dev = nullptr) {
    const int64_t nb = (n_bytes + block_bytes - 1) / block_bytes;
    if (nb == 0) return AMP_OK;
    const int grid = grid_for(st, nb);
    const int rc = ensure_tokens(st, grid);
    if (rc) return rc;
    Args a{d_in, n_bytes, block_bytes, d_out, stride, room, d_len, st.d_tokens, n_dev};
    // launches share the token scratch: each waits for the one before it, on whatever stream that was
    if (st.tokens_used && hipStreamWaitEvent(s, st.tokens_free, 0) != hipSuccess) return AMP_EHIP;
    hipLaunchKernelGGL(k_deflate, dim3((unsigned)grid), dim3(THREADS), 0, s, a, nb);
    if (hipGetLastError() != hipSuccess) return AMP_EHIP;
    if (hipEventRecord(st.tokens_free, s) != hipSuccess) return AMP_EHIP;
    st.tokens_used = true;
    return AMP_OK;
}

static int state_for(int device, DevState **out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AMP_ENODEV;
    if (device < 0 || device >= n || device >= MAX_DEV) return AMP_EINVAL;
    *out = &g_state[device];
    return AMP_OK;
}

struct DeviceScope {                                      // the calling thread's device for the duration of a call
    int prev = -1; bool ok;
    explicit DeviceScope(int device) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; ok = hipSetDevice(device) == hipSuccess; }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

static int init_state(DevState &st, int device) {
    if (st.init) return AMP_OK;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return AMP_EHIP;
    if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) return AMP_ENODEV;
    st.n_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking) != hipSuccess) return AMP_EHIP;
    for (Slot &sl : st.slot)
        if (hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess) return AMP_EHIP;
    if (hipEventCreateWithFlags(&st.tokens_free, hipEventDisableTiming) != hipSuccess) return AMP_EHIP;
    st.init = true;
    return AMP_OK;
}

}  // namespace ampdf

extern "C" {

static int deflate_device(int device, const uint8_t *d_in, int64_t n_bytes, const unsigned long long *n_dev, int32_t block_bytes, uint8_t *d_out,
                          int64_t out_stride, int32_t out_room, uint32_t *d_out_len, void *stream) {
    using namespace ampdf;
    if (n_bytes < 0 || block_bytes < 1 || block_bytes > BS_MAX || out_room < 0 || out_stride < out_room) return AMP_EINVAL;
    if (n_bytes == 0) return AMP_OK;
    if (!d_in || !d_out || !d_out_len) return AMP_EINVAL;
    DevState *st;
    int rc = state_for(device, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(st->mu);
    DeviceScope scope(device);
    if (!scope.ok) return AMP_EHIP;
    rc = init_state(*st, device);
    if (rc) return rc;
    return launch(*st, d_in, n_bytes, block_bytes, d_out, out_stride, out_room, d_out_len, stream ? (hipStream_t)stream : st->stream, n_dev);
}

int amp_deflate_blocks_device(int device, const uint8_t *d_in, int64_t n_bytes, int32_t block_bytes, uint8_t *d_out, int64_t out_stride,
                              int32_t out_room, uint32_t *d_out_len, void *stream) {
    return deflate_device(device, d_in, n_bytes, nullptr, block_bytes, d_out, out_stride, out_room, d_out_len, stream);
}

int amp_deflate_blocks_device_counted(int device, const uint8_t *d_in, const uint64_t *d_n_bytes, int64_t max_bytes, int32_t block_bytes,
                                      uint8_t *d_out, int64_t out_stride, int32_t out_room, uint32_t *d_out_len, void *stream) {
    if (!d_n_bytes) return AMP_EINVAL;
    return deflate_device(device, d_in, max_bytes, (const unsigned long long *)d_n_bytes, block_bytes, d_out, out_stride, out_room, d_out_len, stream);
}

int amp_deflate_sync(int device) {
    using namespace ampdf;
    DevState *st;
    const int rc = state_for(device, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(st->mu);
    if (!st->init) return AMP_OK;
    return hipStreamSynchronize(st->stream) == hipSuccess ? AMP_OK : AMP_EHIP;
}

int amp_deflate_blocks(int device, const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride, int32_t out_room,
                       uint32_t *out_len) {
    using namespace ampdf;
    if (n_bytes < 0 || block_bytes < 1 || block_bytes > BS_MAX || out_room < 0 || out_stride < out_room) return AMP_EINVAL;
    if (n_bytes == 0) return AMP_OK;
    if (!in || !out || !out_len) return AMP_EINVAL;
    DevState *st;
    int rc = state_for(device, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(st->mu);
    DeviceScope scope(device);
    if (!scope.ok) return AMP_EHIP;
    rc = init_state(*st, device);
    if (rc) return rc;
    const int64_t nb = (n_bytes + block_bytes - 1) / block_bytes;
    // on the device a stream gets the room the caller gives it, rounded up to whole dwords between streams
    const int64_t d_stride = ((int64_t)out_room + 3) & ~(int64_t)3;
    const int64_t piece = nb < PIECE_BLOCKS ? nb : PIECE_BLOCKS, n_pieces = (nb + piece - 1) / piece;
    for (int i = 0; i < N_SLOTS && i < n_pieces; ++i) {
        Slot &sl = st->slot[i];
        if (!grow_dev((void **)&sl.d_in, &sl.in_cap, (size_t)piece * (size_t)block_bytes + 16) ||
            !grow_dev((void **)&sl.d_out, &sl.out_cap, (size_t)piece * (size_t)d_stride + 16) ||
            !grow_dev((void **)&sl.d_len, &sl.len_cap, (size_t)piece * 4) ||
            !grow_dev((void **)&sl.d_packed, &sl.packed_cap, (size_t)piece * (size_t)d_stride + 16) ||
            !grow_pinned((void **)&sl.h_out, &sl.h_out_cap, (size_t)piece * (size_t)d_stride + 16) ||
            !grow_pinned((void **)&sl.h_len, &sl.h_len_cap, (size_t)piece * 4)) return AMP_ENOMEM;
    }
    // Two pieces in flight: while the device encodes piece i, the host stages piece i + 1 (a copy from pageable memory keeps the
    // calling thread busy) and then moves the streams of piece i to where the caller wants them.
    auto count = [&](int64_t i) { return nb - i * piece < piece ? nb - i * piece : piece; };
    auto issue = [&](int64_t i) -> int {
        Slot &sl = st->slot[i % N_SLOTS];
        const int64_t cnt = count(i), off = i * piece * block_bytes;
        const int64_t bytes = n_bytes - off < cnt * block_bytes ? n_bytes - off : cnt * block_bytes;
        if (hipMemcpyAsync(sl.d_in, in + off, (size_t)bytes, hipMemcpyHostToDevice, sl.stream) != hipSuccess) return AMP_EHIP;
        const int lrc = launch(*st, sl.d_in, bytes, block_bytes, sl.d_out, d_stride, out_room, sl.d_len, sl.stream);
        if (lrc) return lrc;
        hipLaunchKernelGGL(k_pack, dim3((unsigned)cnt), dim3(256), 0, sl.stream, sl.d_out, d_stride, sl.d_len, sl.d_packed);
        if (hipGetLastError() != hipSuccess) return AMP_EHIP;
        if (hipMemcpyAsync(sl.h_len, sl.d_len, (size_t)cnt * 4, hipMemcpyDeviceToHost, sl.stream) != hipSuccess) return AMP_EHIP;
        return AMP_OK;
    };
    auto finish = [&](int64_t i) -> int {
        Slot &sl = st->slot[i % N_SLOTS];
        const int64_t cnt = count(i), b0 = i * piece;
        if (hipStreamSynchronize(sl.stream) != hipSuccess) return AMP_EHIP;
        // the streams are a fraction of their room: only the bytes that were written travel
        uint32_t words = 0;
        for (int64_t k = 0; k < cnt; ++k) {
            if (sl.h_len[k] > (uint32_t)out_room) return AMP_EHIP;
            words += (sl.h_len[k] + 3) >> 2;
        }
        if (words && hipMemcpyAsync(sl.h_out, sl.d_packed, (size_t)words * 4, hipMemcpyDeviceToHost, sl.stream) != hipSuccess) return AMP_EHIP;
        if (hipStreamSynchronize(sl.stream) != hipSuccess) return AMP_EHIP;
        size_t at = 0;
        for (int64_t k = 0; k < cnt; ++k) {
            const uint32_t len = sl.h_len[k];
            out_len[b0 + k] = len;
            if (len) memcpy(out + (b0 + k) * out_stride, sl.h_out + at, len);
            at += (size_t)((len + 3) >> 2) * 4;
        }
        return AMP_OK;
    };
    rc = issue(0);
    for (int64_t i = 0; i < n_pieces && rc == AMP_OK; ++i) {
        if (i + 1 < n_pieces) rc = issue(i + 1);
        if (rc == AMP_OK) rc = finish(i);
    }
    if (rc != AMP_OK)                                      // nothing of this call stays in flight behind an error
        for (Slot &sl : st->slot) (void)hipStreamSynchronize(sl.stream);
    return rc;
}

int amp_deflate_blocks_cb(void *user, const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride, int32_t out_room,
                          uint32_t *out_len) {
    if (!user) return AMP_EINVAL;
    return amp_deflate_blocks(*(const int32_t *)user, in, n_bytes, block_bytes, out, out_stride, out_room, out_len);
}

}  // extern "C"
