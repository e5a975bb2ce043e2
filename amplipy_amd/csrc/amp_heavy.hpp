// amp_heavy.hpp -- the second pass behind the tile kernel: k_deferred_heavy, written for CDNA4 / gfx950; with it the bound on a
// batch's insertion events (k_event_bound) and variant 1's lane-per-read kernel (k_reads_lane), which share its serial code.
//
// What reaches this pass: the "heavy" entries of the deferred list (amp_tile.hpp), few in a usual batch -- reads the tile kernel
// could not take at all (more CIGAR ops than its LDS column, 64 k bases or more, a trimmed CIGAR that is not regular, no room in
// the tile's segment table) and reads it counted and whose exact status is still missing (DEFER_STATUS_ONLY: a chunk lane or
// the indel walk met an error).  The tile kernel raises ctr[CTR_HEAVY_FLAG] when it defers anything; without the flag a block
// of this kernel returns at once.  (The tile kernel walks the indels of regular reads itself and writes no DEFER_INDELS entry
// any more; the pass still knows what to do with one: process_read_indels.)
//
// A read gets one of four treatments, chosen by the number of ops of its INPUT CIGAR:
//   * up to D_MAXOPS - 3 ops: lane = read, the serial trim of amp_read.hpp with both CIGAR buffers in LDS columns
//     (process_read<true>); a regular result leaves only its indels on the lane (the skip-ahead walk) and hands its match
//     bases to a group of D_GROUP lanes (count_match_coop);
//   * up to WV_MAXOPS - 4 ops: wave = read, the closed forms of amp_wave.hpp on CIGAR rows that alias the columns;
//   * more than that (or a many-op read that needs only its status): lane = read again, the CIGAR ping-pongs between the read's
//     output slot and its scratch slot in global memory, and the read's events go into a slice of the list reserved once, of
//     ins_event_bound slots (SliceSink);
//   * the exact serial walk (process_read<false>) for what the wave path declines, and inside process_read for every read
//     whose trimmed CIGAR is not regular.
// Counts of all four go through one block-wide LDS window of D_WIN positions (WinSink), events through a block-wide stage.
//
// Work items: the deferred list has one segment per block of the tile kernel, and a block here takes a UNIT of D_UNIT
// consecutive segments -- neighbours on the reference of a sorted batch, so they share one window.  heavy_pass<SPARSE = true>
// takes the units that hold at most one round (256) of entries in all and runs each as one round; heavy_pass<false> takes the
// segments of the other units one by one, so that a batch made of heavy reads keeps one block per segment.  A small
// persistent grid (ReadPlan::heavy_grid) looks at the counts of 64 work items per wave-load and enters those with entries.
//
// The kernels stay in the global namespace, where they were before they had a header: their symbols are what profiles name.
#pragma once

#include <type_traits>

#include "amp_tile.hpp"
#include "amp_wave.hpp"

using namespace amp;

// ---------------------------------------------------------------------------------------
// kernels shared by both variants
// ---------------------------------------------------------------------------------------

// Upper bound on the insertion events a read can record: every event starts on its own
// (q, None) aligned pair inside [query_alignment_start, query_alignment_end), i.e. on a base
// of an I / P / inner-S op of the INPUT CIGAR, ops [c0, c1) of cig.  Trimming only turns such bases into clips,
// never creates them.  The event list is reserved by this bound and the heavy pass cuts a read's slice of it by the same.
__device__ __forceinline__ unsigned long long ins_event_bound(const uint32_t *__restrict__ cig, uint32_t c0, uint32_t c1) {
    unsigned long long lead = 0, all = 0, trail = 0;
    bool in_lead = true;
    for (uint32_t k = c0; k < c1; ++k) {
        uint32_t v = cig[k], op = v & 15u, len = v >> 4;
        if (op == OP_H) continue;
        if (op == OP_S) { all += len; trail += len; if (in_lead) lead += len; }
        else { in_lead = false; trail = 0; if (op == OP_I || op == OP_P) all += len; }
    }
    return all - lead - (in_lead ? 0 : trail);
}

// ... of a batch, added to ctr[CTR_EVENT_BOUND]
__global__ void k_event_bound(int64_t n, const uint32_t *__restrict__ cig_off, const uint32_t *__restrict__ cig,
                              unsigned long long *ctr) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long b = 0;
    if (i < n) b = ins_event_bound(cig, cig_off[i], cig_off[i + 1]);
    for (int o = 32; o > 0; o >>= 1) b += __shfl_down(b, o);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[CTR_EVENT_BOUND], b);
}

struct DevSink {
    uint32_t *counts;
    const EventBuf &eb;
    uint32_t read;
    __device__ void add(int32_t r, uint32_t col) { atomicAdd(&counts[(size_t)r * AMP_NSYM + col], 1u); }
    __device__ void event(int32_t pos, int32_t lo, int32_t hi) { eb.record(pos, read, lo, hi); }
};


// Second-pass sink: the reads of one list segment come from one contiguous range of the sorted batch,
// so their counts are privatised in a block-wide LDS window (device-scope atomics on distinct
// addresses run at ~23 G/s chip-wide on MI355X: they, not the walk, bound a lane-per-read pass).
// Positions outside the window go straight to the global table.
constexpr uint32_t D_WIN = 1024;            // positions of the second pass's LDS window (with 512 the 400-base reads of a segment fell outside it half the time: global atomics)
constexpr uint32_t D_PLANES = AMP_NSYM + 1;   // six symbols + the insertion-event tally
constexpr uint32_t D_EVCAP = 512;             // events staged per round (the rest go out one by one)
struct WinSink {
    lds_u32 *win;
    int32_t base;
    uint32_t *counts;
    const EventBuf &eb;
    uint32_t read;
    lds_u32 *ev;      // [D_EVCAP][4] staged events
    lds_u32 *nev;     // staging cursor (keeps counting past D_EVCAP)
    __device__ void add(int32_t r, uint32_t col) {
        const uint32_t d = (uint32_t)(r - base);
        if (d < D_WIN) lds_add(win + col * D_WIN + d, 1u);
        else atomicAdd(&counts[(size_t)r * AMP_NSYM + col], 1u);
    }
    // One returning atomic per event on the list cursor serialises in L2 (~0.2 events/ns chip-wide,
    // measured): events are staged in LDS and the block reserves list space once per round.
    __device__ void event(int32_t pos, int32_t lo, int32_t hi) {
        const uint32_t k = atomicAdd((uint32_t *)nev, 1u);
        if (k < D_EVCAP) {
            ev[k * 4] = (uint32_t)pos; ev[k * 4 + 1] = read; ev[k * 4 + 2] = (uint32_t)lo; ev[k * 4 + 3] = (uint32_t)hi;
            const uint32_t d = (uint32_t)(pos - base);
            if (d < D_WIN) lds_add(win + AMP_NSYM * D_WIN + d, 1u);
            else atomicAdd(&eb.ins_at[pos], 1u);
        } else {
            eb.record(pos, read, lo, hi);
        }
    }
};

// Staged events -> the block's shard of the list, one reservation for all of them.  Block-wide.
__device__ void flush_staged_events(const EventBuf &eb, const uint32_t *s_ev, uint32_t *s_nev, unsigned long long *s_evbase) {
    __syncthreads();
    const uint32_t nev = *s_nev < D_EVCAP ? *s_nev : D_EVCAP;
    const unsigned shard = blockIdx.x & (EV_SHARDS - 1);
    if (threadIdx.x == 0 && nev) *s_evbase = atomicAdd(&eb.ctr[CTR_EV_SHARD0 + shard], (unsigned long long)nev);
    __syncthreads();
    if (nev) {
        const unsigned long long eb0 = *s_evbase;
        for (uint32_t k = threadIdx.x; k < nev; k += blockDim.x)
            if ((long long)(eb0 + k) < eb.cap)
                eb.ev[(size_t)shard * (size_t)eb.cap + eb0 + k] =
                    amp_ins_event{(int32_t)s_ev[k * 4], s_ev[k * 4 + 1], (int32_t)s_ev[k * 4 + 2], (int32_t)s_ev[k * 4 + 3]};
    }
    __syncthreads();
    if (threadIdx.x == 0) *s_nev = 0;
    __syncthreads();
}

// Sink of a read with a long CIGAR (tens of insertions): one reservation on the list cursor for the whole read
// (an upper bound of its events) instead of one per event; slots left over are marked invalid
// (ref_pos = -1) and dropped when the list is read out.  Counts go through the block's window.
struct SliceSink {
    WinSink &w;
    amp_ins_event *slice;
    uint32_t cap, used;
    __device__ void add(int32_t r, uint32_t col) { w.add(r, col); }
    __device__ void event(int32_t pos, int32_t lo, int32_t hi) {
        if (used < cap) {
            slice[used++] = amp_ins_event{pos, w.read, lo, hi};
            const uint32_t d = (uint32_t)(pos - w.base);
            if (d < D_WIN) lds_add(w.win + AMP_NSYM * D_WIN + d, 1u);
            else atomicAdd(&w.eb.ins_at[pos], 1u);
        } else {
            w.event(pos, lo, hi);
        }
    }
};

struct NullSink {   // dry run: only the status matters
    __device__ void add(int32_t, uint32_t) {}
    __device__ void event(int32_t, int32_t, int32_t) {}
};

// one CIGAR column in LDS for the second pass (stride = block size)
struct LdsCig256 {
    lds_u32 *p;
    __device__ __forceinline__ uint32_t get(int i) const { return p[i * 256]; }
    __device__ __forceinline__ void set(int i, uint32_t v) const { p[i * 256] = v; }
};

__device__ __forceinline__ bool is_home(const CigBuf<1> &b, const uint32_t *home) { return b.p == home; }
__device__ __forceinline__ bool is_home(const LdsCig256 &, const uint32_t *) { return false; }

// One read, start to finish, on one lane with the serial code of amp_read.hpp.  cur / tmp are the
// two CIGAR buffers the trims ping-pong between (global slots, or LDS columns when the read fits);
// the final CIGAR always lands in the read's output slot.  status_only: the tile kernel already
// counted this read and only needs to know which error comes first in pair order.
// COOP = false: the exact serial walk counts the read (returns false).
// COOP = true: the second-pass treatment of a read the tile kernel could not hold (more CIGAR ops than its LDS
// column): serial trim with both CIGAR buffers in LDS columns -- or, for CIGARs of more than D_MAXOPS - 3 ops
// (Nanopore-like reads), ping-pong between the read's output slot and the scratch slot in global memory --, then
//   * regular trimmed CIGAR (clips at the ends, body of M/=/X/I/D/N): deletions / insertion events by
//     the skip-ahead walk on this lane; the match bases are left to the block's waves (count_match_coop)
//     - returns true and leaves the final CIGAR in `cur`;
//   * anything else: the exact serial walk.
constexpr int D_MAXOPS = 19;      // (with the rest of HeavyLds this lets two blocks share a CU's 160 KB)
static_assert(4 * (3 * WV_MAXOPS + WV_STASH_WORDS) <= 2 * D_MAXOPS * 256 && 4 * WV_EVCAP <= 512 && WV_QSTASH <= 528, "the wave path's rows and event stages alias the columns / the block's stage");
template <bool COOP, class CB, class Sink>
__device__ bool process_read(const KParams &P, const amp_dev_reads &rd, int64_t i, const DevOut &out, Sink &sink,
                             const EventBuf &eb, bool status_only, CB &cur, CB &tmp, uint32_t c0, int n,
                             int &n_final, int32_t &pos_final) {
    uint32_t *const home = out.new_cig + (size_t)c0 + 3 * (size_t)i;
    for (int k = 0; k < n; ++k) cur.set(k, rd.cig[c0 + k]);
    const int32_t lseq = (int32_t)rd.lseq[i];
    const int64_t boff = (int64_t)rd.seq_off8[i] * 8;
    const uint8_t *qual = rd.qual + boff;
    const bool have_qual = lseq > 0 && qual[0] != 0xFF;
    TrimState st{rd.pos[i], n, 0u, 0};
    if (P.do_trim) trim_read_serial(P, st, rd.flag[i], rd.tlen[i], lseq, qual, have_qual, cur, tmp);
    if (!st.err && !is_home(cur, home))
        for (int k = 0; k < st.n; ++k) home[k] = cur.get(k);
    int err = st.err;
    bool coop = false;
    if (!err && P.do_count) {
        NullSink ns;
        if (status_only) {
            err = count_read_walk(P, cur, st.n, st.pos, lseq, ReadBytesCached{rd.seq, boff, qual}, have_qual, ns);
        } else if constexpr (!COOP) {
            err = count_read_walk(P, cur, st.n, st.pos, lseq, ReadBytesCached{rd.seq, boff, qual}, have_qual, sink);
        } else {
            bool regular, plain;
            int nseg, e1 = 0, e2 = 0;
            int32_t qs = 0, qe = 0;
            classify(cur, st.n, lseq, regular, plain, nseg);
            if (!have_qual || lseq <= 0) regular = false;
            if (regular) { qs = query_alignment_start(cur, st.n, lseq, e1); qe = query_alignment_end(cur, st.n, lseq, e2); }
            if (regular && !e1 && !e2) {
                if (!plain && count_regular_skip(P, cur, st.n, st.pos, lseq, qs, qe, QualAt{qual}, sink))
                    err = count_read_walk(P, cur, st.n, st.pos, lseq, ReadBytesCached{rd.seq, boff, qual}, have_qual, ns);
                coop = err == 0;
            } else {
                err = count_read_walk(P, cur, st.n, st.pos, lseq, ReadBytesCached{rd.seq, boff, qual}, have_qual, sink);
            }
        }
    }
    if (out.new_pos) out.new_pos[i] = st.pos;
    if (out.new_ncig) out.new_ncig[i] = st.err ? 0u : (uint32_t)st.n;
    if (out.ref_len) out.ref_len[i] = st.err ? 0 : reference_length(cur, st.n);
    if (out.trim_flags) out.trim_flags[i] = st.err ? (uint8_t)0 : (uint8_t)st.flags;
    if (out.status) out.status[i] = (uint8_t)err;
    if (err) atomicAdd(&eb.ctr[CTR_ERROR_READS], 1ull);
    n_final = st.n; pos_final = st.pos;
    return coop;
}

// Match bases of one regular read by a group of D_GROUP lanes: lane = base of the current match op
// (A:718, A:751-753); every op costs one memory round trip, so several reads per wave hide it.
// A base that cannot be counted (code outside ACGTN, position past the table) makes the group's
// first lane run the exact walk for the read's status, like the tile kernel's status-only deferral.
constexpr int D_GROUP = 16;
template <class CB, class Sink>
__device__ void count_match_coop(const KParams &P, const amp_dev_reads &rd, int64_t i, const DevOut &out, Sink &sink,
                                 const EventBuf &eb, const CB &cig, int n, int32_t pos, int lane) {
    const int32_t lseq = (int32_t)rd.lseq[i];
    const int64_t boff = (int64_t)rd.seq_off8[i] * 8;
    const uint8_t *qual = rd.qual + boff;
    const uint32_t G = (uint32_t)P.ref_len;
    int32_t q = 0, r = pos;
    bool bad = false;
    // the ops come D_GROUP at a time, one per lane, and are handed round with shuffles: a CIGAR that lives in global
    // memory (tens of ops) costs a round trip per sixteen ops instead of one per op
    // (a CIGAR in an LDS column is simply read op by op)
    constexpr bool in_lds = std::is_same<CB, LdsCig256>::value;
    const int lane0 = (int)(threadIdx.x & 63u) & ~(D_GROUP - 1);
    for (int k0 = 0; k0 < n; k0 += D_GROUP) {
        uint32_t mine = 0u;
        if (!in_lds) mine = k0 + lane < n ? cig.get(k0 + lane) : 0u;
        const int kn = n - k0 < D_GROUP ? n - k0 : D_GROUP;
        for (int k = 0; k < kn; ++k) {
            const uint32_t v = in_lds ? cig.get(k0 + k) : (uint32_t)__shfl((int)mine, lane0 + k), op = v & 15u;
            const int32_t len = (int32_t)(v >> 4);
            if (is_match_op(op)) {
                for (int32_t j = lane; j < len; j += D_GROUP) {
                    if ((int32_t)qual[q + j] < P.min_quality) continue;
                    const uint32_t col = code_to_col(base_code(rd.seq, boff, q + j));
                    if (col == 0xFFu || (uint32_t)(r + j) >= G) bad = true;
                    else sink.add(r + j, col);
                }
                q += len; r += len;
            } else if (op == OP_I || op == OP_S) q += len;
            else if (op == OP_D || op == OP_N) r += len;
        }
    }
    const uint64_t gmask = ((1ull << D_GROUP) - 1ull) << lane0;
    if ((__ballot(bad) & gmask) && lane == 0) {
        NullSink ns;
        const int err = count_read_walk(P, cig, n, pos, lseq, ReadBytesCached{rd.seq, boff, qual}, true, ns);
        if (out.status) out.status[i] = (uint8_t)err;
        if (err) atomicAdd(&eb.ctr[CTR_ERROR_READS], 1ull);
    }
}

// Variant 1: every read on its own lane.  Kept as the simple kernel the tile kernel is
// A/B-checked against on the GPU.
__global__ void __launch_bounds__(256)
k_reads_lane(KParams P, amp_dev_reads rd, uint64_t read_base, DevOut out, uint32_t *scratch, uint32_t *counts, EventBuf eb) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rd.n_reads) return;
    const uint32_t c0 = rd.cig_off32[i];
    const size_t slot = (size_t)c0 + 3 * (size_t)i;
    DevSink sink{counts, eb, (uint32_t)(read_base + (uint64_t)i)};
    CigBuf<1> cur{out.new_cig + slot}, tmp{scratch + slot};      // CIGAR ping-pong in global memory (any length)
    int nf; int32_t pf;
    process_read<false>(P, rd, i, out, sink, eb, false, cur, tmp, c0, (int)(rd.cig_off32[i + 1] - c0), nf, pf);
}

// Deletions / reference skips and insertion events of a read whose match bases the tile kernel
// already counted: the skip-ahead walk over the FINAL CIGAR the tile kernel wrote out (staged in an
// LDS column first: the walk re-reads ops many times).
template <class Sink>
__device__ int process_read_indels(const KParams &P, const amp_dev_reads &rd, int64_t i, const DevOut &out, Sink &sink, lds_u32 *col) {
    const size_t slot = (size_t)rd.cig_off32[i] + 3 * (size_t)i;
    const int n = (int)out.new_ncig[i];
    const int32_t lseq = (int32_t)rd.lseq[i];
    const int32_t pos = out.new_pos[i];
    const uint8_t *qual = rd.qual + (int64_t)rd.seq_off8[i] * 8;
    const QualAt qf{qual};
    int e1 = 0, e2 = 0;
    if (n <= T_MAXOPS) {
        const LdsCig256 cig{col};
        for (int k = 0; k < n; ++k) cig.set(k, out.new_cig[slot + k]);
        const int32_t qs = query_alignment_start(cig, n, lseq, e1), qe = query_alignment_end(cig, n, lseq, e2);
        return count_regular_skip(P, cig, n, pos, lseq, qs, qe, qf, sink);
    }
    const CigBuf<1> cig{out.new_cig + slot};
    const int32_t qs = query_alignment_start(cig, n, lseq, e1), qe = query_alignment_end(cig, n, lseq, e2);
    return count_regular_skip(P, cig, n, pos, lseq, qs, qe, qf, sink);
}


// Heavy half, off the back of the segment: reads the tile kernel could not take at all (more CIGAR ops
// than its LDS column, unusual CIGAR, no room in the tile's segment table) and reads that need
// their exact status.  Lane = read for trimming and indels, lane groups for match bases.
// The work item of a block is a UNIT of D_UNIT consecutive list segments (neighbours on the reference, so
// they can share one LDS window).  SPARSE = true takes the units with at most one round of entries in all and
// runs them as ONE round (a few heavy reads per segment are the common case, and a round per
// segment would be all latency); SPARSE = false takes the other units segment by segment, so that
// a batch made of heavy reads keeps one block per segment.
constexpr int D_UNIT = 8;
struct HeavyLds {
    uint32_t cig[2 * D_MAXOPS * 256];
    uint32_t win[D_PLANES * D_WIN];
    uint32_t coop[3 * 256];
    uint32_t ev[4 * D_EVCAP];
    uint32_t ucnt[D_UNIT + 1];
    uint32_t lng[256];              // reads of this round for the wave path (amp_wave.hpp)
    uint32_t nlong, nslow, wnev[4];
    uint32_t ncoop, nev;
    unsigned long long evbase, mask;
};

template <bool SPARSE>
__device__ __forceinline__ void heavy_pass(HeavyLds &L, const KParams &P, const amp_dev_reads &rd, uint64_t read_base, const DevOut &out,
                                           uint32_t *scratch, uint32_t *counts, const EventBuf &eb, const uint32_t *dlist,
                                           const uint32_t *dcnt, long long tiles_per_block, long long n_seg, long long dcnt_stride,
                                           const uint32_t *segfirst) {
    uint32_t *const s_cig = L.cig, *const s_win = L.win, *const s_coop = L.coop, *const s_ev = L.ev, *const s_ucnt = L.ucnt;
    uint32_t &s_ncoop = L.ncoop, &s_nev = L.nev;
    unsigned long long &s_evbase = L.evbase, &s_mask = L.mask;
    // Few reads are heavy: a small persistent grid looks at the counts of 64 work items per wave-load and only
    // enters those that have entries (a block per segment would cost more in empty launches).
    // work items: whole units (SPARSE) or single segments of the other units
    const int64_t n_item = SPARSE ? (n_seg + D_UNIT - 1) / D_UNIT : n_seg;
    for (int64_t u0 = blockIdx.x; u0 < n_item; u0 += (int64_t)gridDim.x * 64) {
    if (threadIdx.x < 64) {
        const int64_t it = u0 + (int64_t)threadIdx.x * gridDim.x;
        uint32_t tot = 0, own = 0;
        if (it < n_item) {
            const int64_t unit = SPARSE ? it : it / D_UNIT;
            for (int j = 0; j < D_UNIT; ++j) { const int64_t sbj = unit * D_UNIT + j; if (sbj < n_seg) tot += dcnt[5 * dcnt_stride + 64 + sbj]; }
            own = SPARSE ? tot : dcnt[5 * dcnt_stride + 64 + it];
        }
        const unsigned long long mk = __ballot(own != 0 && (tot <= 256u) == SPARSE);
        if (threadIdx.x == 0) s_mask = mk;
    }
    __syncthreads();
    unsigned long long todo = s_mask;
    __syncthreads();
    while (todo) {
    const int64_t item = u0 + (int64_t)(__ffsll((long long)todo) - 1) * gridDim.x;
    todo &= todo - 1;
    {
    const int64_t sb_first = SPARSE ? item * D_UNIT : item;
    __syncthreads();
    if (threadIdx.x == 0) {                      // exclusive prefix of the pass's segment counts
        uint32_t acc = 0;
        for (int j = 0; j < D_UNIT; ++j) {
            s_ucnt[j] = acc;
            const int64_t sbj = sb_first + j;
            if (sbj < n_seg && (SPARSE || j == 0)) acc += dcnt[5 * dcnt_stride + 64 + sbj];
        }
        s_ucnt[D_UNIT] = acc;
        s_ncoop = 0; s_nev = 0;
        L.nlong = 0; L.nslow = 0; L.wnev[0] = L.wnev[1] = L.wnev[2] = L.wnev[3] = 0;
    }
    for (uint32_t k = threadIdx.x; k < D_PLANES * D_WIN; k += blockDim.x) s_win[k] = 0;
    // sorted input: no read of this pass starts left of the first read of its first tile range
    const int64_t first_row = sb_first * tiles_per_block * TILE;
    int32_t base = rd.pos[segfirst ? (int64_t)segfirst[sb_first] : first_row];
    if (base < 0) base = 0;
    __syncthreads();
    const uint32_t cnt = s_ucnt[D_UNIT];
    uint32_t done = 0;   // cooperative entries of earlier rounds (the LDS cursor keeps counting)
    for (uint32_t k0 = 0; k0 < cnt; k0 += blockDim.x) {
        const uint32_t k = k0 + threadIdx.x;
        if (k < cnt) {
            int j = 0;
            if (SPARSE) {
#pragma unroll
                for (int jj = 1; jj < D_UNIT; ++jj) j += k >= s_ucnt[jj] ? 1 : 0;
            }
            const uint32_t *seg_end = dlist + ((size_t)(sb_first + j) + 1) * (size_t)tiles_per_block * TILE;
            const uint32_t e = seg_end[-1 - (int64_t)(k - s_ucnt[j])];
            const int64_t i = (int64_t)(e & DEFER_INDEX_MASK);
            bool status_only = (e & DEFER_STATUS_ONLY) != 0, more = true;
            WinSink sink{(lds_u32 *)s_win, base, counts, eb, (uint32_t)(read_base + (uint64_t)i), (lds_u32 *)s_ev, (lds_u32 *)&s_nev};
            if (e & DEFER_INDELS) {
                if (process_read_indels(P, rd, i, out, sink, (lds_u32 *)s_cig + threadIdx.x)) status_only = true;   // exact status below
                else if (!status_only) more = false;
            }
            if (more) {
                const uint32_t c0 = rd.cig_off32[i];
                const int n = (int)(rd.cig_off32[i + 1] - c0);
                if (n + 3 <= D_MAXOPS) {
                    LdsCig256 cur{(lds_u32 *)s_cig + threadIdx.x}, tmp{(lds_u32 *)s_cig + D_MAXOPS * 256 + threadIdx.x};
                    int nf; int32_t pf;
                    if (process_read<true>(P, rd, i, out, sink, eb, status_only, cur, tmp, c0, n, nf, pf)) {
                        // cooperative entry: read, final ops | column of the lane that trimmed it << 22 | buffer B << 30, start
                        const uint32_t slot = atomicAdd(&s_ncoop, 1u) - done;
                        const uint32_t in_b = cur.p != (lds_u32 *)s_cig + threadIdx.x;
                        s_coop[slot * 3] = (uint32_t)i;
                        s_coop[slot * 3 + 1] = (uint32_t)nf | (threadIdx.x << 22) | (in_b << 30);
                        s_coop[slot * 3 + 2] = (uint32_t)pf;
                    }
                } else if (!status_only && n <= WV_MAXOPS - 4) {
                    // tens to hundreds of ops: a wave per read, below
                    L.lng[atomicAdd(&L.nlong, 1u)] = (uint32_t)i;
                } else {
                    // longer CIGARs ping-pong in global memory; counts go through the block's window and the
                    // events into a slice of the list reserved once for the read, of ins_event_bound slots
                    const size_t slot = (size_t)c0 + 3 * (size_t)i;
                    uint32_t bound = 0;
                    if (!status_only && P.do_count) bound = (uint32_t)ins_event_bound(rd.cig, c0, c0 + (uint32_t)n);
                    const unsigned shard = blockIdx.x & (EV_SHARDS - 1);
                    unsigned long long base0 = 0;
                    if (bound) base0 = atomicAdd(&eb.ctr[CTR_EV_SHARD0 + shard], (unsigned long long)bound);
                    const bool fits = bound && (long long)(base0 + bound) <= eb.cap;
                    SliceSink ss{sink, eb.ev + (size_t)shard * (size_t)eb.cap + base0, fits ? bound : 0u, 0u};
                    // the trim runs on this lane; a regular result leaves only its indels here (skip-ahead walk) and
                    // hands the match bases to a group of lanes, which reads the final CIGAR from the output slot
                    CigBuf<1> cur{out.new_cig + slot}, tmp{scratch + slot};
                    int nf; int32_t pf;
                    if (process_read<true>(P, rd, i, out, ss, eb, status_only, cur, tmp, c0, n, nf, pf)) {
                        const uint32_t cslot = atomicAdd(&s_ncoop, 1u) - done;
                        s_coop[cslot * 3] = (uint32_t)i;
                        s_coop[cslot * 3 + 1] = ((uint32_t)nf & 0x3FFFFFu) | (1u << 31);      // bit 31: the CIGAR is in global memory
                        s_coop[cslot * 3 + 2] = (uint32_t)pf;
                    }
                    for (uint32_t k = ss.used; k < ss.cap; ++k) ss.slice[k] = amp_ins_event{-1, 0u, 0, 0};
                }
            }
        }
        __syncthreads();
        const uint32_t ncoop = s_ncoop - done;
        for (uint32_t c = threadIdx.x / D_GROUP; c < ncoop; c += blockDim.x / D_GROUP) {
            const int64_t i = (int64_t)s_coop[c * 3];
            const uint32_t w = s_coop[c * 3 + 1];
            WinSink sink{(lds_u32 *)s_win, base, counts, eb, (uint32_t)(read_base + (uint64_t)i), (lds_u32 *)s_ev, (lds_u32 *)&s_nev};
            if (w >> 31) {
                const CigBuf<1> cig{out.new_cig + (size_t)rd.cig_off32[i] + 3 * (size_t)i};
                count_match_coop(P, rd, i, out, sink, eb, cig, (int)(w & 0x3FFFFFu), (int32_t)s_coop[c * 3 + 2], (int)(threadIdx.x % D_GROUP));
            } else {
                const LdsCig256 cig{(lds_u32 *)s_cig + ((w >> 30) & 1u) * (D_MAXOPS * 256) + ((w >> 22) & 0xFFu)};
                count_match_coop(P, rd, i, out, sink, eb, cig, (int)(w & 0x3FFFFFu), (int32_t)s_coop[c * 3 + 2], (int)(threadIdx.x % D_GROUP));
            }
        }
        done += ncoop;
        flush_staged_events(eb, s_ev, &s_nev, &s_evbase);
        if (L.nlong) {
            // wave = read (amp_wave.hpp): three CIGAR rows per wave in the columns' space, events staged per wave
            const uint32_t nlong = L.nlong;
            const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
            lds_u32 *const row = (lds_u32 *)s_cig + wave * (3 * WV_MAXOPS);
            lds_u32 *const wev = (lds_u32 *)s_ev + wave * (WV_EVCAP * 4), *const wn = (lds_u32 *)&L.wnev[wave];
            lds_u8 *const wq = (lds_u8 *)((lds_u32 *)s_cig + 4 * 3 * WV_MAXOPS + wave * WV_STASH_WORDS);
            unsigned long long dummy_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; (void)dummy_acc;
            for (uint32_t c = (uint32_t)wave; c < nlong; c += 4u) {
                const int64_t i = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)L.lng[c]);
                WaveSink ws{(lds_u32 *)s_win, base, D_WIN, D_WIN, 31u, (uint32_t)AMP_NSYM, counts, eb, (uint32_t)(read_base + (uint64_t)i), wev, wn, (uint32_t)WV_EVCAP};
                if (!wave_read(P, rd, i, wv_header_load(rd, i, lane), out, ws, eb, row, row + WV_MAXOPS, row + 2 * WV_MAXOPS, wq, WV_MAXOPS - 4, lane, dummy_acc)) {
                    if (lane == 0) s_coop[atomicAdd(&L.nslow, 1u)] = (uint32_t)i;      // not a read for the closed forms
                }
                if (*wn > (uint32_t)WV_EVCAP / 2u) wv_flush_events(eb, wev, wn, (uint32_t)WV_EVCAP, lane);
            }
            wv_flush_events(eb, wev, wn, (uint32_t)WV_EVCAP, lane);
            __syncthreads();
            const uint32_t nslow = L.nslow;
            for (uint32_t k = threadIdx.x; k < nslow; k += blockDim.x) {
                // the exact serial code, CIGAR ping-pong between the output slot and the scratch slot
                const int64_t i = (int64_t)s_coop[k];
                const uint32_t c0 = rd.cig_off32[i];
                const size_t slot = (size_t)c0 + 3 * (size_t)i;
                WinSink sink{(lds_u32 *)s_win, base, counts, eb, (uint32_t)(read_base + (uint64_t)i), (lds_u32 *)s_ev, (lds_u32 *)&s_nev};
                CigBuf<1> cur{out.new_cig + slot}, tmp{scratch + slot};
                int nf; int32_t pf;
                process_read<false>(P, rd, i, out, sink, eb, false, cur, tmp, c0, (int)(rd.cig_off32[i + 1] - c0), nf, pf);
            }
            flush_staged_events(eb, s_ev, &s_nev, &s_evbase);
            if (threadIdx.x == 0) { L.nlong = 0; L.nslow = 0; }
            __syncthreads();
        }
    }
    for (uint32_t k = threadIdx.x; k < D_PLANES * D_WIN; k += blockDim.x) {
        const uint32_t v = s_win[k];
        if (!v) continue;
        const uint32_t plane = k / D_WIN, p = (uint32_t)base + k % D_WIN;
        if (plane < AMP_NSYM) atomicAdd(&counts[(size_t)p * AMP_NSYM + plane], v);
        else atomicAdd(&eb.ins_at[p], v);
    }
    __syncthreads();
    }
    }   // items of this round
    }   // rounds
}

// one launch for both kinds of work item: an empty launch is not free when the other step's scan
// kernel holds the LDS of every CU
__global__ void __launch_bounds__(256)
k_deferred_heavy(KParams P, amp_dev_reads rd, uint64_t read_base, DevOut out, uint32_t *scratch, uint32_t *counts,
                 EventBuf eb, const uint32_t *dlist, const uint32_t *dcnt, long long tiles_per_block, long long n_seg,
                 const GenGeo *geo, long long dcnt_stride, const uint32_t *segfirst, unsigned long long *hist) {
    __shared__ HeavyLds L;
    const bool any = __hip_atomic_load(&eb.ctr[CTR_HEAVY_FLAG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;   // set by the tile kernel
    if (geo) { tiles_per_block = (long long)geo->tpb; n_seg = (long long)geo->n_seg; }
    if (hist && blockIdx.x == 0) {
        // for the host's plan of the engine's next pass (amp_ctx::h_hist): the lengths of this pass's two lists, each in one
        // 8-byte word of pinned host memory with the pass's epoch
        if (threadIdx.x == 0) L.nev = 0;
        __syncthreads();
        uint32_t h = 0;
        if (any) for (long long s = threadIdx.x; s < n_seg; s += blockDim.x) h += dcnt[5 * dcnt_stride + 64 + s];
        if (h) atomicAdd(&L.nev, h);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long tag = (unsigned long long)P.epoch << 32;
            __hip_atomic_store(&hist[0], tag | L.nev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&hist[1], tag | (uint32_t)eb.ctr[CTR_GEN_LIST_N], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
    if (!any) return;
    heavy_pass<true>(L, P, rd, read_base, out, scratch, counts, eb, dlist, dcnt, tiles_per_block, n_seg, dcnt_stride, segfirst);
    __syncthreads();
    heavy_pass<false>(L, P, rd, read_base, out, scratch, counts, eb, dlist, dcnt, tiles_per_block, n_seg, dcnt_stride, segfirst);
}

// The second pass over the deferred list of a tile kernel that ran on the grid `tg`.  Behind k_tile<LIST> (geo and segfirst
// given) the list's geometry is decided on the device and read from geo; behind the other tile kernels it is tg's.
static inline int heavy_launch(const KParams &P, const amp_dev_reads &rd, uint64_t read_base, const DevOut &out, uint32_t *scratch,
                               uint32_t *counts, const EventBuf &eb, const uint32_t *dlist, const uint32_t *dcnt, int64_t grid,
                               const TileGrid &tg, const GenGeo *geo, const uint32_t *segfirst, hipStream_t stream,
                               unsigned long long *hist = nullptr) {
    k_deferred_heavy<<<(unsigned)grid, 256, 0, stream>>>(P, rd, read_base, out, scratch, counts, eb, dlist, dcnt, geo ? 0 : (long long)tg.tpb,
                                                         geo ? 0 : (long long)tg.grid, geo, (long long)tg.grid, segfirst, hist);
    return (int)hipGetLastError();
}
