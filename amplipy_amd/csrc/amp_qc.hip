// amp_qc.hip -- the amplicon QC report on the device (C ABI: the amp_qc_* entry points of amplihip.h).
//
// k_qc_reads runs behind the read pass of every batch while the report is on: one lane per read classifies it
// (qc_classify, amp_qc.hpp) from the batch and the pass's per-read results where they lie in HBM, and the block adds what
// its reads came to onto twelve 64-bit tallies and two per-primer read counts.  The normal input is a coordinate-sorted pile
// of thousands of reads on one primer, so nothing is added per lane: the scalar tallies are summed per wave (ballot and
// popcount for the counts, a shuffle sum for the two sums), then per block through LDS, and reach memory as one 64-bit add per
// tally and block; for the primer counts neighbouring lanes with the same owner form a run whose head adds the run's length
// -- to a histogram in LDS that the block flushes once when the primer set fits it, straight to the global arrays otherwise.
// No step relies on the reads being sorted: an unsorted batch only makes shorter runs.
// k_qc_depth and k_qc_regions turn the count table as it stands into depth per position and per-region figures, without
// atomics: the output does not depend on the order anything ran in.
// k_qc_clips (section 15b) is the report's second per-batch kernel, behind k_qc_reads while its own sub-switch is on: soft-clip
// sites per reference position and side, from the reads as they came in (amp_clip.hpp).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "amp_clip.hpp"
#include "amp_hook.hpp"
#include "amp_qc.hpp"
#include "amp_tally.hpp"

namespace amp {

struct QcState : HookState {
    amp_qc_params p{};                    // (its pointers are not kept: the arrays are copied below)
    int32_t *d_left = nullptr, *d_right = nullptr;        // [ref_len] owners
    unsigned long long *d_tally = nullptr;                // [QC_N_TALLIES + 2 * n_primers]: scalars, start counts, end counts
    int32_t *d_rstart = nullptr, *d_rend = nullptr;       // [n_regions], clamped
    amp_qc_region *d_regions = nullptr;                   // [n_regions]
    uint32_t *d_depth = nullptr;                          // [ref_len]
    // the clip sites (amp_qc_clips_enable): the table and, behind it in the same allocation, the CL_N_SCALARS 64-bit scalars
    uint32_t *d_clip = nullptr;
    int32_t clip_min = 0;                                 // 0: the sub-switch is off
    HookTimer clip_timer;                                 // k_qc_clips' own: `timer` stays k_qc_reads'
    size_t tally_words() const { return (size_t)QC_N_TALLIES + 2 * (size_t)p.n_primers; }
    ~QcState() { clip_timer.destroy(); }
};

struct QcReadsArgs {
    int64_t n;
    const int32_t *pos;
    const uint32_t *cig_off32, *cig;
    const int32_t *ref_len_out;
    const uint8_t *trim_flags, *status;
    const int32_t *left_owner, *right_owner;
    unsigned long long *tally;
    int32_t n_primers;
    QcReadParams P;
};

__device__ __forceinline__ int qc_lane() { return (int)(threadIdx.x & 63u); }

// Lanes of a wave that carry the same owner as their left neighbour form a run; the run's first lane adds its length.
// Every lane of the wave calls this (owner -1: nothing to add).
template <class Add>
__device__ __forceinline__ void qc_add_runs(int32_t owner, Add add) {
    const int lane = qc_lane();
    const int32_t prev = __shfl_up(owner, 1);
    const bool head = lane == 0 || prev != owner;
    const unsigned long long heads = __ballot(head);
    if (head && owner >= 0) {
        const unsigned long long behind = (heads >> lane) >> 1;       // run heads to the right of this lane
        add(owner, (uint32_t)(behind ? __ffsll((long long)behind) : 64 - lane));
    }
}

template <bool LDS_HIST>
__global__ void __launch_bounds__(QC_BLOCK)
k_qc_reads(QcReadsArgs a) {
    __shared__ uint32_t s_hist[LDS_HIST ? QC_LDS_COUNTERS : 1];
    __shared__ unsigned long long s_part[QC_BLOCK / 64][QC_N_TALLIES];
    const int tid = (int)threadIdx.x, lane = qc_lane(), wave = tid >> 6;
    const int n_hist = 2 * a.n_primers;
    if (LDS_HIST) {
        for (int k = tid; k < n_hist; k += QC_BLOCK) s_hist[k] = 0u;
        __syncthreads();
    }
    unsigned long long *const g_start = a.tally + QC_N_TALLIES, *const g_end = g_start + a.n_primers;
    uint32_t cnt[QC_N_FLAGS];                 // wave-uniform: reads of this wave with the bit set
#pragma unroll
    for (int k = 0; k < QC_N_FLAGS; ++k) cnt[k] = 0u;
    unsigned long long sum_in = 0ull, sum_out = 0ull;       // per lane
    // grid-stride over tiles of QC_BLOCK reads; the bound is the same for every lane of the block, so the shuffles and
    // ballots below always see whole waves
    for (int64_t base = (int64_t)blockIdx.x * QC_BLOCK; base < a.n; base += (int64_t)gridDim.x * QC_BLOCK) {
        const int64_t i = base + tid;
        uint32_t bits = 0u;
        int32_t own_s = -1, own_e = -1;
        if (i < a.n) {
            const uint32_t c0 = a.cig_off32[i], c1 = a.cig_off32[i + 1];
            const uint32_t st = a.status ? a.status[i] : 0u;
            const int32_t rl = a.P.do_trim ? a.ref_len_out[i] : 0;
            const uint32_t tf = a.P.do_trim ? a.trim_flags[i] : 0u;
            const QcRead r = qc_classify(a.pos[i], a.cig + c0, c1 - c0, rl, tf, st, a.P, a.left_owner, a.right_owner);
            bits = r.bits; own_s = r.owner_start; own_e = r.owner_end;
            sum_in += r.ref_in; sum_out += r.ref_out;
        }
#pragma unroll
        for (int k = 0; k < QC_N_FLAGS; ++k) cnt[k] += (uint32_t)__popcll(__ballot((bits >> k) & 1u));
        if (a.P.do_trim && a.n_primers > 0) {
            if (LDS_HIST) {
                qc_add_runs(own_s, [&](int32_t o, uint32_t len) { atomicAdd(&s_hist[o], len); });
                qc_add_runs(own_e, [&](int32_t o, uint32_t len) { atomicAdd(&s_hist[a.n_primers + o], len); });
            } else {
                qc_add_runs(own_s, [&](int32_t o, uint32_t len) { atomicAdd(&g_start[o], (unsigned long long)len); });
                qc_add_runs(own_e, [&](int32_t o, uint32_t len) { atomicAdd(&g_end[o], (unsigned long long)len); });
            }
        }
    }
    // the two sums over the wave, then everything over the block's waves, then one add per tally
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum_in += __shfl_down(sum_in, d);
        sum_out += __shfl_down(sum_out, d);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < QC_N_FLAGS; ++k) s_part[wave][k] = cnt[k];
        s_part[wave][QC_REF_BASES_IN] = sum_in;
        s_part[wave][QC_REF_BASES_OUT] = sum_out;
    }
    __syncthreads();
    if (tid < QC_N_TALLIES) {
        unsigned long long t = 0ull;
        for (int w = 0; w < QC_BLOCK / 64; ++w) t += s_part[w][tid];
        if (t) atomicAdd(&a.tally[tid], t);
    }
    if (LDS_HIST) {
        for (int k = tid; k < n_hist; k += QC_BLOCK) {
            const uint32_t v = s_hist[k];
            if (v) atomicAdd(&g_start[k], (unsigned long long)v);       // (the end counts lie behind the start counts here as there)
        }
    }
}

struct QcClipsArgs {
    int64_t n;
    const int32_t *pos;
    const uint16_t *flag;
    const uint32_t *lseq, *cig_off32, *cig, *seq_off8;
    const uint8_t *seq, *status;
    uint32_t *table;                    // [(ref_len + 1)][2][CL_CELLS]
    unsigned long long *scalars;        // [CL_N_SCALARS]
    int32_t ref_len, clip_min;
};

// What one read adds to its site, cell by cell (a lane whose site no other lane of the wave shares)
__device__ __forceinline__ void qc_clip_add_alone(uint32_t *cells, uint32_t rev, uint64_t cols) {
    atomicAdd(&cells[0], 1u);
    if (rev) atomicAdd(&cells[1], 1u);
    for (int j = 0; j < CL_K; ++j) {
        const uint32_t f = clip_field(cols, j);
        if (f == CL_NO_COL) break;
        atomicAdd(&cells[2 + j * CL_COLS + (int)f], 1u);
    }
}

// One lane per read.  The normal input is a pile -- thousands of neighbouring reads with one pos, hence one LEFT site; with
// pre-trimmed input nearly every read has a primer-length clip at one of a few hundred sites -- so nothing is added per read:
// per side the wave's lanes fall into groups with the same site (wave_each_distinct), a group's reads and reverse reads are
// popcounts of ballots, and per clipped-base offset five ballots give the group's count of every column, which lanes 0..4 add,
// one atomic each where the count is not zero.  The atomics a wave issues grow with its distinct sites, not with its reads.  A
// lane that is alone on its site is only noted in the loop and adds its own cells behind it, all such lanes at once.  A wave
// without a site of a side leaves that side at wave_each_distinct's first ballot.  Nothing relies on the batch being sorted.
__global__ void __launch_bounds__(QC_BLOCK)
k_qc_clips(QcClipsArgs a) {
    const int tid = (int)threadIdx.x, lane = qc_lane();
    uint32_t cnt[CL_N_SCALARS] = {0u, 0u, 0u, 0u};      // wave-uniform
    // (the bound is the same for every lane of the block: the ballots and shuffles below always see whole waves)
    for (int64_t base = (int64_t)blockIdx.x * QC_BLOCK; base < a.n; base += (int64_t)gridDim.x * QC_BLOCK) {
        const int64_t i = base + tid;
        const bool live = i < a.n && (a.status ? a.status[i] == 0 : true);
        ClipRead r;
        r.skipped = 0; r.L[0] = r.L[1] = 0; r.p[0] = r.p[1] = -1;
        int32_t lseq = 0;
        uint32_t rev = 0u;
        uint64_t sbase = 0ull;
        if (live) {
            const uint32_t c0 = a.cig_off32[i], c1 = a.cig_off32[i + 1];
            lseq = (int32_t)a.lseq[i];
            r = clip_scan(a.pos[i], a.cig + c0, c1 - c0, lseq, a.ref_len, a.clip_min);
            rev = (a.flag[i] & 0x10u) ? 1u : 0u;
            sbase = (uint64_t)a.seq_off8[i] * 8ull;
        }
        cnt[CL_SCANNED] += (uint32_t)__popcll(__ballot(live && !r.skipped));
        cnt[CL_SKIPPED] += (uint32_t)__popcll(__ballot(live && r.skipped));
        cnt[CL_N_LEFT] += (uint32_t)__popcll(__ballot(r.p[CL_LEFT] >= 0));
        cnt[CL_N_RIGHT] += (uint32_t)__popcll(__ballot(r.p[CL_RIGHT] >= 0));
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int32_t key = r.p[side];                // in [0, ref_len] (clip_scan), or -1
            const bool have = key >= 0;
            const uint64_t cols = have ? clip_cols(a.seq, sbase, lseq, side, r.L[side]) : ~0ull;
            bool alone = false;
            int32_t site = 0;                             // the group's key: a scalar
            wave_each_distinct(have, [&](int src) { site = __shfl(key, src); return have && key == site; },
                               [&](int src, unsigned long long same) {
                const uint32_t n_in = (uint32_t)__popcll(same);
                if (n_in == 1u) { alone = alone || lane == src; return; }
                const bool in = (same >> lane) & 1ull;
                uint32_t *const cells = a.table + clip_site_word(site, side);
                const uint32_t n_rev = (uint32_t)__popcll(__ballot(in && rev));
                if (lane == 0) atomicAdd(&cells[0], n_in);
                if (lane == 1 && n_rev) atomicAdd(&cells[1], n_rev);
                for (int j = 0; j < CL_K; ++j) {
                    const uint32_t f = in ? clip_field(cols, j) : CL_NO_COL;
                    if (!__ballot(f != CL_NO_COL)) break;      // (no read of the group is clipped this far)
                    uint32_t mine = 0u;
#pragma unroll
                    for (int c = 0; c < CL_COLS; ++c) {
                        const uint32_t v = (uint32_t)__popcll(__ballot(f == (uint32_t)c));
                        mine = lane == c ? v : mine;
                    }
                    if (lane < CL_COLS && mine) atomicAdd(&cells[2 + j * CL_COLS + lane], mine);
                }
            });
            if (alone) qc_clip_add_alone(a.table + clip_site_word(key, side), rev, cols);
        }
    }
    if (lane < CL_N_SCALARS) {
        uint32_t mine = 0u;
#pragma unroll
        for (int k = 0; k < CL_N_SCALARS; ++k) mine = lane == k ? cnt[k] : mine;
        if (mine) atomicAdd(&a.scalars[lane], (unsigned long long)mine);
    }
}

__global__ void __launch_bounds__(QC_BLOCK)
k_qc_depth(const uint32_t *__restrict__ counts, int32_t ref_len, uint32_t *__restrict__ depth) {
    for (int64_t p = (int64_t)blockIdx.x * QC_BLOCK + threadIdx.x; p < ref_len; p += (int64_t)gridDim.x * QC_BLOCK)
        depth[p] = qc_depth_of(counts + (size_t)p * AMP_NSYM);
}

__device__ __forceinline__ QcRegionAcc qc_shfl_down(const QcRegionAcc &a, int d) {
    QcRegionAcc b;
    b.sum = __shfl_down((unsigned long long)a.sum, d);
    b.mn = __shfl_down(a.mn, d);
    b.mx = __shfl_down(a.mx, d);
#pragma unroll
    for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) b.covered[k] = __shfl_down(a.covered[k], d);
    return b;
}

struct QcDepths { int32_t n; uint32_t d[AMP_QC_MAX_DEPTHS]; };

__global__ void __launch_bounds__(QC_BLOCK)
k_qc_regions(const uint32_t *__restrict__ depth, int32_t n_regions, const int32_t *__restrict__ rstart, const int32_t *__restrict__ rend,
             QcDepths dp, amp_qc_region *__restrict__ out) {
    __shared__ QcRegionAcc s_acc[QC_BLOCK / 64];
    const int tid = (int)threadIdx.x, lane = qc_lane(), wave = tid >> 6;
    for (int32_t r = (int32_t)blockIdx.x; r < n_regions; r += (int32_t)gridDim.x) {
        const int32_t s = rstart[r], e = rend[r];           // clamped by the host: 0 <= s <= e <= ref_len
        QcRegionAcc acc = qc_region_empty();
        for (int64_t p = (int64_t)s + tid; p < e; p += QC_BLOCK) qc_region_add(acc, depth[p], dp.n, dp.d);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const QcRegionAcc o = qc_shfl_down(acc, d);
            qc_region_merge(acc, o);
        }
        if (lane == 0) s_acc[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < QC_BLOCK / 64; ++w) qc_region_merge(acc, s_acc[w]);
            out[r] = qc_region_result(s, e, acc);
        }
        __syncthreads();
    }
}

static QcState *qc_state(amp_ctx *c) { return hook_state<QcState>(c, HOOK_QC); }

static int qc_enqueue_reads(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    QcState *s = qc_state(c);
    QcReadsArgs a;
    a.n = rd->n_reads; a.pos = rd->pos; a.cig_off32 = rd->cig_off32; a.cig = rd->cig;
    a.ref_len_out = o ? o->ref_len : nullptr; a.trim_flags = o ? o->trim_flags : nullptr; a.status = o ? o->status : nullptr;
    a.left_owner = s->d_left; a.right_owner = s->d_right;
    a.tally = s->d_tally; a.n_primers = s->p.n_primers;
    a.P = QcReadParams{q.ref_len, q.do_trim ? 1 : 0, s->p.min_length, s->p.include_no_primer};
    // (paid once per block: its LDS histogram and its twelve adds)
    HOOKTRY(hook_launch(q, s, qc_hook, a.n, o, QC_BLOCK, QC_TILES_PER_BLOCK, QC_BLOCKS_PER_CU, [&](unsigned grid) {
        if (2 * (int64_t)s->p.n_primers <= QC_LDS_COUNTERS) k_qc_reads<true><<<grid, QC_BLOCK, 0, q.stream>>>(a);
        else k_qc_reads<false><<<grid, QC_BLOCK, 0, q.stream>>>(a);
    }));
    if (s->clip_min <= 0 || !s->d_clip) return AMP_OK;
    // the clip sites, behind it on the same stream, between the events of a timer of their own
    s->clip_timer.timed = false;
    if (a.n <= 0) return AMP_OK;
    QcClipsArgs k;
    k.n = rd->n_reads; k.pos = rd->pos; k.flag = rd->flag; k.lseq = rd->lseq; k.cig_off32 = rd->cig_off32; k.cig = rd->cig;
    k.seq_off8 = rd->seq_off8; k.seq = rd->seq; k.status = a.status;
    k.table = s->d_clip; k.scalars = (unsigned long long *)(s->d_clip + clip_table_words(q.ref_len));
    k.ref_len = q.ref_len; k.clip_min = s->clip_min;
    HOOKCHK(q, s->clip_timer.begin(q.stream));
    k_qc_clips<<<hook_grid(k.n, QC_BLOCK, QC_TILES_PER_BLOCK, QC_BLOCKS_PER_CU, q.n_cu), QC_BLOCK, 0, q.stream>>>(k);
    HOOKCHK(q, hipGetLastError());
    HOOKCHK(q, s->clip_timer.end(q.stream));
    return AMP_OK;
}

HookOps qc_hook = {"the QC report needs", OUT_NEW_POS | OUT_REF_LEN | OUT_TRIM_FLAGS | OUT_STATUS, qc_enqueue_reads, hook_free<QcState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_qc_find_primer_owners(int32_t ref_len, int32_t n, const int32_t *starts, const int32_t *ends, int32_t off,
                              int32_t *left_owner, int32_t *right_owner) {
    if (ref_len < 0 || n < 0 || off < 0 || (n && (!starts || !ends)) || (ref_len && (!left_owner || !right_owner))) return AMP_EINVAL;
    // a sweep over the positions with the primers whose window has opened and whose index is not below that of the first
    // one still open, in index (= start) order; closed windows among them are skipped
    std::vector<int32_t> open((size_t)std::max(n, 1));
    int head = 0, tail = 0, next = 0;
    for (int32_t p = 0; p < ref_len; ++p) {
        while (next < n && (int64_t)p >= (int64_t)starts[next] - off) open[tail++] = next++;
        while (head != tail && (int64_t)p >= (int64_t)ends[open[head]] + off) ++head;
        int32_t lo = -1, ro = -1;
        for (int k = head; k < tail; ++k) {
            const int32_t i = open[k];
            if ((int64_t)p >= (int64_t)ends[i] + off) continue;
            if (lo < 0 || ends[i] > ends[lo]) lo = i;
            if (ro < 0 || starts[i] < starts[ro]) ro = i;
        }
        left_owner[p] = lo; right_owner[p] = ro;
    }
    return AMP_OK;
}

int amp_qc_enable(amp_ctx *c, const amp_qc_params *p) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_QC);
    if (!p) { slot.on = false; return AMP_OK; }
    if (p->n_primers < 0 || (p->n_primers && (!p->starts || !p->ends)) || p->primer_pos_offset < 0 || p->n_regions < 0 ||
        (p->n_regions && (!p->region_start || !p->region_end)) || p->n_depths < 0 || p->n_depths > AMP_QC_MAX_DEPTHS) return AMP_EINVAL;
    for (int32_t k = 1; k < p->n_primers; ++k)
        if (p->starts[k] < p->starts[k - 1] || (p->starts[k] == p->starts[k - 1] && p->ends[k] < p->ends[k - 1])) return AMP_EINVAL;
    if (q.do_trim && !q.have_primers) return AMP_ESTATE;
    Guard g(q.device);
    HOOKCHK(q, hipStreamSynchronize(q.stream));      // (a report that is replaced may still have a kernel in flight)
    hook_free<QcState>(slot.state);
    slot.state = nullptr; slot.on = false;
    QcState *made = nullptr;
    const int made_rc = hook_new_state(q, slot, qc_hook, made, [&](QcState &fresh) -> int {
        QcState *const s = &fresh;
        s->p = *p;
        s->p.starts = s->p.ends = s->p.region_start = s->p.region_end = nullptr;
        const size_t G = (size_t)q.ref_len, R = (size_t)p->n_regions;
        std::vector<int32_t> lo(G), ro(G), rs(R), re(R);
        int rc = amp_qc_find_primer_owners(q.ref_len, p->n_primers, p->starts, p->ends, p->primer_pos_offset, lo.data(), ro.data());
        if (rc != AMP_OK) return rc;
        for (size_t r = 0; r < R; ++r) {
            rs[r] = p->region_start[r]; re[r] = p->region_end[r];
            qc_region_clamp(q.ref_len, rs[r], re[r]);
        }
        HOOKTRY(hook_alloc(q, fresh, &s->d_left, G * 4));
        HOOKTRY(hook_alloc(q, fresh, &s->d_right, G * 4));
        HOOKTRY(hook_alloc(q, fresh, &s->d_depth, G * 4));
        HOOKTRY(hook_alloc(q, fresh, &s->d_tally, s->tally_words() * sizeof(unsigned long long), s->tally_words() * sizeof(unsigned long long)));
        if (R) {
            HOOKTRY(hook_alloc(q, fresh, &s->d_rstart, R * 4));
            HOOKTRY(hook_alloc(q, fresh, &s->d_rend, R * 4));
            HOOKTRY(hook_alloc(q, fresh, &s->d_regions, R * sizeof(amp_qc_region)));
            HOOKCHK(q, hipMemcpyAsync(s->d_rstart, rs.data(), R * 4, hipMemcpyHostToDevice, q.stream));
            HOOKCHK(q, hipMemcpyAsync(s->d_rend, re.data(), R * 4, hipMemcpyHostToDevice, q.stream));
        }
        HOOKCHK(q, hipMemcpyAsync(s->d_left, lo.data(), G * 4, hipMemcpyHostToDevice, q.stream));
        HOOKCHK(q, hipMemcpyAsync(s->d_right, ro.data(), G * 4, hipMemcpyHostToDevice, q.stream));
        HOOKCHK(q, hipMemsetAsync(s->d_tally, 0, s->tally_words() * sizeof(unsigned long long), q.stream));
        HOOKCHK(q, hipStreamSynchronize(q.stream));        // (the host vectors go away)
        return AMP_OK;
    });
    slot.on = made_rc == AMP_OK;
    return made_rc;
}

int amp_qc_read_tallies(amp_ctx *c, amp_qc_reads *out, uint64_t *primer_reads_start, uint64_t *primer_reads_end) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s = qc_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    const size_t np = (size_t)s->p.n_primers;
    if (out) HOOKCHK(q, hipMemcpyAsync(out, s->d_tally, sizeof(amp_qc_reads), hipMemcpyDeviceToHost, q.stream));
    if (primer_reads_start && np) HOOKCHK(q, hipMemcpyAsync(primer_reads_start, s->d_tally + QC_N_TALLIES, np * 8, hipMemcpyDeviceToHost, q.stream));
    if (primer_reads_end && np) HOOKCHK(q, hipMemcpyAsync(primer_reads_end, s->d_tally + QC_N_TALLIES + np, np * 8, hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

int amp_qc_depth(amp_ctx *c, uint32_t *depth, amp_qc_region *regions) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s = qc_state(c);
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    const int64_t blocks = ((int64_t)q.ref_len + QC_BLOCK - 1) / QC_BLOCK;
    k_qc_depth<<<(unsigned)std::min<int64_t>(blocks, (int64_t)QC_BLOCKS_PER_CU * q.n_cu), QC_BLOCK, 0, q.stream>>>(q.counts, q.ref_len, s->d_depth);
    HOOKCHK(q, hipGetLastError());
    if (depth) HOOKCHK(q, hipMemcpyAsync(depth, s->d_depth, (size_t)q.ref_len * 4, hipMemcpyDeviceToHost, q.stream));
    const int32_t R = s->p.n_regions;
    if (regions && R) {
        QcDepths dp;
        dp.n = s->p.n_depths;
        for (int k = 0; k < AMP_QC_MAX_DEPTHS; ++k) dp.d[k] = k < dp.n ? s->p.depths[k] : 0u;
        k_qc_regions<<<(unsigned)std::min<int64_t>(R, (int64_t)QC_BLOCKS_PER_CU * q.n_cu), QC_BLOCK, 0, q.stream>>>(s->d_depth, R, s->d_rstart, s->d_rend, dp, s->d_regions);
        HOOKCHK(q, hipGetLastError());
        HOOKCHK(q, hipMemcpyAsync(regions, s->d_regions, (size_t)R * sizeof(amp_qc_region), hipMemcpyDeviceToHost, q.stream));
    }
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

int amp_qc_last_ms(amp_ctx *c, float *reads_ms) { return hook_last_ms(c, HOOK_QC, reads_ms); }

// ---- clip sites: the sub-switch of the report ----
static size_t qc_clip_bytes(int32_t ref_len) { return clip_table_words(ref_len) * 4 + CL_N_SCALARS * sizeof(uint64_t); }

// The state with a clip table, or the refusal's code with its message in the ctx error text
static int qc_clip_state(amp_ctx *c, const HookCtx &q, const char *who, QcState *&s) {
    s = qc_state(c);
    if (s && s->d_clip) return AMP_OK;
    snprintf(q.err, q.err_cap, "%s: %s", who, s ? "the clip sites were not enabled since the last amp_qc_enable (amp_qc_clips_enable)" : "no QC report (amp_qc_enable)");
    return AMP_ESTATE;
}

int amp_qc_clips_enable(amp_ctx *c, int32_t clip_min) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s = qc_state(c);
    if (clip_min < 0 || clip_min > CL_MIN_MAX) {
        snprintf(q.err, q.err_cap, "amp_qc_clips_enable: clip_min %d is not in 0..%d", (int)clip_min, CL_MIN_MAX);
        return AMP_EINVAL;
    }
    if (!s) {
        snprintf(q.err, q.err_cap, "amp_qc_clips_enable: no QC report (amp_qc_enable)");
        return AMP_ESTATE;
    }
    if (clip_min == 0) { s->clip_min = 0; return AMP_OK; }       // off; a table read so far stays readable
    Guard g(q.device);
    const size_t bytes = qc_clip_bytes(q.ref_len);
    if (!s->d_clip) {
        HOOKCHK(q, s->clip_timer.create());
        HOOKTRY(hook_alloc(q, *s, &s->d_clip, bytes, bytes));     // (zeros: all of it, so amp_reset clears it)
    }
    HOOKCHK(q, hipStreamSynchronize(q.stream));      // (a kernel of the last setting may be in flight)
    HOOKCHK(q, hipMemsetAsync(s->d_clip, 0, bytes, q.stream));
    s->clip_min = clip_min;
    return AMP_OK;
}

int amp_qc_clips_get(amp_ctx *c, uint32_t *table, uint64_t *scalars) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s;
    HOOKTRY(qc_clip_state(c, q, "amp_qc_clips_get", s));
    Guard g(q.device);
    const size_t words = clip_table_words(q.ref_len);
    if (table) HOOKCHK(q, hipMemcpyAsync(table, s->d_clip, words * 4, hipMemcpyDeviceToHost, q.stream));
    if (scalars) HOOKCHK(q, hipMemcpyAsync(scalars, s->d_clip + words, CL_N_SCALARS * sizeof(uint64_t), hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

int amp_qc_clips_add(amp_ctx *c, const uint32_t *table, const uint64_t *scalars) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s;
    HOOKTRY(qc_clip_state(c, q, "amp_qc_clips_add", s));
    Guard g(q.device);
    const size_t words = clip_table_words(q.ref_len);
    HOOKTRY(hook_add(q, s->d_clip, table, words));
    return hook_add(q, (uint64_t *)(s->d_clip + words), scalars, (size_t)CL_N_SCALARS);
}

int amp_qc_clips_last_ms(amp_ctx *c, float *ms) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    QcState *s;
    HOOKTRY(qc_clip_state(c, q, "amp_qc_clips_last_ms", s));
    return s->clip_timer.last_ms(q, ms);
}

}  // extern "C"
