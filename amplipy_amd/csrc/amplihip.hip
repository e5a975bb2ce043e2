// amplihip.hip -- libamplihip.so: the C ABI (include/amplihip.h) for gfx950: the context, the calling kernels and the small ones.
//
// Replaces AmpliPy.py's per-read loop (A:896-915 = trim_read A:426-687 +
// update_base_counts A:690-753) and the integer part of calling (A:756-771, A:917-952)
// with batch kernels.  There is no host execution path for the read work: every entry point
// that touches reads launches kernels on the ctx's device.  The read kernels and launch_reads, which launches them, are a
// unit of their own (amp_readpass.hip): an edit of the host code here compiles none of them.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/amplihip.h"
#include "amp_ctx.hpp"
#include "amp_call.hpp"
#include "amp_ins.hpp"
#define AMP_CODEC_CTX_ONLY
#include "amp_codec.hpp"

using namespace amp;

hipError_t amp::grow_events(amp_ctx *c, int64_t ncap) {   // re-lays the shard regions out for a larger capacity
    if (ncap <= c->ev_cap) return hipSuccess;
    void *np = nullptr;
    hipError_t e = hipMalloc(&np, (size_t)EV_SHARDS * (size_t)ncap * sizeof(amp_ins_event));
    if (e != hipSuccess) return e;
    if (c->events.p && c->ev_cap) {
        for (int s = 0; s < EV_SHARDS && e == hipSuccess; ++s)
            e = hipMemcpyAsync((amp_ins_event *)np + (size_t)s * ncap, c->events.as<amp_ins_event>() + (size_t)s * c->ev_cap,
                               (size_t)c->ev_cap * sizeof(amp_ins_event), hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipFree(np); return e; }
    }
    c->events.release();
    c->events.p = np; c->events.cap = (size_t)EV_SHARDS * (size_t)ncap * sizeof(amp_ins_event);
    c->ev_cap = ncap;
    return hipSuccess;
}

// amp_reset: zeroes the device table and the counters.  A handful of blocks (RESET_BLOCKS) that store 16 bytes per lane in a
// grid-stride loop: while a pass of another engine runs, every block of this kernel has to wait for a CU that no block of a
// fast kernel holds, and the pass behind it on the stream waits with it.
constexpr unsigned RESET_BLOCKS = 8;
__global__ void __launch_bounds__(256)
k_reset(uint32_t *a, size_t na, uint32_t *b, size_t nb) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
    const size_t to16 = (size_t)((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) / 4;
    const size_t head = to16 < na ? to16 : na;      // words in front of the first 16-byte boundary
    const size_t nvec = (na - head) / 4, tail = na - head - nvec * 4;
    uint4 *const v = (uint4 *)(a + head);
    for (size_t i = t; i < nvec; i += nt) v[i] = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = t; i < head + tail + nb; i += nt) {
        if (i < head) a[i] = 0u;
        else if (i < head + tail) a[head + nvec * 4 + (i - head)] = 0u;
        else b[i - head - tail] = 0u;
    }
}

__global__ void k_add_u32(uint32_t *dst, const uint32_t *src, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// Calling (A:756-771 alleles_from_counts + A:917-952), one lane per reference position.
// Everything that does not depend on the TEXT of an insertion allele is decided here, by call_position (amp_call.hpp):
// total depth, the six base symbols ranked like sorted(..., reverse=True), consensus symbol, variant record.
// An insertion string can only matter when the position's insertion events could out-rank
// the best base symbol or reach the variant frequency threshold; such positions are flagged
// AMP_CALL_INS_RELEVANT and finished by the host from the event list.
__global__ void __launch_bounds__(256)
k_call(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ ins_at,
                       const uint8_t *__restrict__ ref, int32_t ref_len, amp_call_params pr, amp_pos_call *__restrict__ out,
                       unsigned long long *n_relevant, uint2 *__restrict__ blk) {
    __shared__ uint32_t sv[4], sr[4];
    int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < ref_len;
    if (!live) p = ref_len - 1;            // keep the whole block alive for the block-level counts
    uint32_t cnt[6];
    for (int k = 0; k < 6; ++k) cnt[k] = counts[(size_t)p * AMP_NSYM + k];
    bool relevant;
    const amp_pos_call o = call_position(cnt, ins_at[p], ref + p, pr, relevant);   // amp_call.hpp
    if (relevant && n_relevant && live) atomicAdd(n_relevant, 1ull);
    if (live) out[p] = o;
    if (blk) {   // records per 256-position block, for k_call_compact
        const bool isr = live && relevant, isv = live && !relevant && (o.flags & AMP_CALL_VARIANT);
        const unsigned long long bv = __ballot(isv), br = __ballot(isr);
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = (uint32_t)__popcll(bv); sr[threadIdx.x >> 6] = (uint32_t)__popcll(br); }
        __syncthreads();
        if (threadIdx.x == 0) blk[blockIdx.x] = make_uint2(sv[0] + sv[1] + sv[2] + sv[3], sr[0] + sr[1] + sr[2] + sr[3]);
    }
}

// Packs the outcome of k_call for the host: consensus column per position, the variant records in
// ascending position (insertion-relevant positions excluded: the host finishes those), and the list
// of insertion-relevant positions.  k_call leaves per-256-position-block record counts; each block
// here places its records behind the totals of the blocks before it.
__global__ void __launch_bounds__(256)
k_call_compact(const amp_pos_call *__restrict__ pc, const uint32_t *__restrict__ counts, int32_t ref_len, const uint2 *__restrict__ blk,
               int8_t *__restrict__ cons, amp_var_rec *__restrict__ vars, int32_t *__restrict__ rel, unsigned long long *n_out) {
    __shared__ uint32_t s_pv[4], s_pr[4], s_wv[4], s_wr[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // totals of the blocks before this one
    uint32_t pv = 0, prl = 0;
    for (int b = tid; b < (int)blockIdx.x; b += 256) { const uint2 c = blk[b]; pv += c.x; prl += c.y; }
    for (int o = 32; o > 0; o >>= 1) { pv += __shfl_down(pv, o); prl += __shfl_down(prl, o); }
    if (lane == 0) { s_pv[wave] = pv; s_pr[wave] = prl; }
    const int32_t p = blockIdx.x * 256 + tid;
    amp_pos_call c;
    c.flags = 0; c.consensus_sym = -1; c.alt_mask = 0; c.order = 0; c.total_depth = 0; c.ref_count = 0; c.pad = 0;
    if (p < ref_len) { c = pc[p]; cons[p] = c.consensus_sym; }
    const bool isr = (c.flags & AMP_CALL_INS_RELEVANT) != 0, isv = !isr && (c.flags & AMP_CALL_VARIANT);
    const unsigned long long bv = __ballot(isv), br = __ballot(isr);
    if (lane == 0) { s_wv[wave] = (uint32_t)__popcll(bv); s_wr[wave] = (uint32_t)__popcll(br); }
    __syncthreads();
    uint32_t ov = s_pv[0] + s_pv[1] + s_pv[2] + s_pv[3], orl = s_pr[0] + s_pr[1] + s_pr[2] + s_pr[3];
    for (int w = 0; w < wave; ++w) { ov += s_wv[w]; orl += s_wr[w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    ov += (uint32_t)__popcll(bv & below); orl += (uint32_t)__popcll(br & below);
    if (isr) rel[orl] = p;
    if (isv) {
        amp_var_rec v;
        v.pos = p; v.total_depth = c.total_depth; v.ref_count = c.ref_count;
        v.gt_has_ref = (c.flags & AMP_CALL_GT_HAS_REF) ? 1 : 0;
        // ALT slot j takes the j-th ranked symbol that is flagged (static slot indices: a dynamic one puts the record
        // into LDS, 11 KB per block, and the kernel could no longer run next to a block of the fast kernel)
        uint32_t m = c.alt_mask & 0x3Fu;
        uint8_t na = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (m) {
                const int k = __builtin_ctz(m);
                m &= m - 1u;
                const uint32_t col = (c.order >> (3 * k)) & 7u;
                v.alt_col[j] = (uint8_t)col; v.alt_count[j] = counts[(size_t)p * AMP_NSYM + col]; ++na;
            } else {
                v.alt_col[j] = 0xFF; v.alt_count[j] = 0;
            }
        }
        v.n_alt = na;
        vars[ov] = v;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 255) {   // last thread of the last block knows both totals
        n_out[0] = ov + (isv ? 1u : 0u);
        n_out[1] = orl + (isr ? 1u : 0u);
    }
}

// k_call and k_call_compact as ONE launch, for the pipelined callers (amp_call_compact_begin): a launch behind a pass costs its
// blocks' wait for free CUs and a place in the stream's queue, and nothing but the per-block record counts crosses from the one
// kernel to the other.  A block calls its 256 positions, keeps them in registers, publishes its two record counts and adds up
// those of the blocks in front of it (a look-back over their flags), then writes its part of the image.
// A block's number is the order of its arrival (a ticket), not blockIdx.x: every block with a smaller number has started, and
// a block publishes its counts before it waits for any, so the wait ends wherever the blocks are placed and however few of
// them are resident at a time.  sync: [0] ticket, [1] blocks that are through, [2] waits given up, [CALL_SYNC_FLAG0 + b] the flag
// of block b: bit 63 | relevant positions << 32 | variant records.  All zero before the launch; the last block through leaves
// them zero again.  A wait is given up after CALL_WAIT_TICKS of the 100 MHz clock (seconds: it cannot happen unless a block in
// front was lost); the image then says so in n_out[2] and the host refuses it.
constexpr int CALL_SYNC_FLAG0 = 4;
constexpr unsigned long long CALL_WAIT_TICKS = 400000000ull;
__global__ void __launch_bounds__(256)
k_call_fused(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ ins_at, const uint8_t *__restrict__ ref, int32_t ref_len,
             amp_call_params pr, int8_t *__restrict__ cons, amp_var_rec *__restrict__ vars, int32_t *__restrict__ rel,
             unsigned long long *n_out, unsigned long long *sync) {
    __shared__ uint32_t s_vb, s_last, s_pv[4], s_pr[4], s_wv[4], s_wr[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned long long *const flag = sync + CALL_SYNC_FLAG0;
    if (tid == 0) s_vb = (uint32_t)__hip_atomic_fetch_add(&sync[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t vb = s_vb;
    const int32_t p = (int32_t)(vb * 256u) + tid;
    const bool live = p < ref_len;
    const int32_t pp = live ? p : ref_len - 1;            // keep the whole block alive for the block-level counts
    uint32_t cnt[6];
    for (int k = 0; k < 6; ++k) cnt[k] = counts[(size_t)pp * AMP_NSYM + k];
    bool relevant;
    const amp_pos_call c = call_position(cnt, ins_at[pp], ref + pp, pr, relevant);   // amp_call.hpp
    if (live) cons[p] = c.consensus_sym;
    const bool isr = live && relevant, isv = live && !relevant && (c.flags & AMP_CALL_VARIANT);
    const unsigned long long bv = __ballot(isv), br = __ballot(isr);
    if (lane == 0) { s_wv[wave] = (uint32_t)__popcll(bv); s_wr[wave] = (uint32_t)__popcll(br); }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long tv = s_wv[0] + s_wv[1] + s_wv[2] + s_wv[3], tr = s_wr[0] + s_wr[1] + s_wr[2] + s_wr[3];
        __hip_atomic_store(&flag[vb], (1ull << 63) | (tr << 32) | tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // totals of the blocks in front of this one
    uint32_t pv = 0, prl = 0;
    bool gave_up = false;
    const unsigned long long t_wait0 = wall_clock64();
    for (uint32_t b = (uint32_t)tid; b < vb; b += 256u) {
        unsigned long long x = __hip_atomic_load(&flag[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (!(x >> 63)) {
            if (wall_clock64() - t_wait0 > CALL_WAIT_TICKS) { gave_up = true; break; }
            x = __hip_atomic_load(&flag[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        pv += (uint32_t)x; prl += (uint32_t)(x >> 32) & 0x7FFFFFFFu;
    }
    if (gave_up) __hip_atomic_fetch_add(&sync[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int o = 32; o > 0; o >>= 1) { pv += __shfl_down(pv, o); prl += __shfl_down(prl, o); }
    if (lane == 0) { s_pv[wave] = pv; s_pr[wave] = prl; }
    __syncthreads();
    uint32_t ov = s_pv[0] + s_pv[1] + s_pv[2] + s_pv[3], orl = s_pr[0] + s_pr[1] + s_pr[2] + s_pr[3];
    for (int w = 0; w < wave; ++w) { ov += s_wv[w]; orl += s_wr[w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    ov += (uint32_t)__popcll(bv & below); orl += (uint32_t)__popcll(br & below);
    // (offsets are sums of counts of distinct positions: inside the image whatever a given-up wait left out)
    if (isr) rel[orl] = p;
    if (isv) {
        amp_var_rec v;
        v.pos = p; v.total_depth = c.total_depth; v.ref_count = c.ref_count;
        v.gt_has_ref = (c.flags & AMP_CALL_GT_HAS_REF) ? 1 : 0;
        uint32_t m = c.alt_mask & 0x3Fu;      // (static slot indices: see k_call_compact)
        uint8_t na = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (m) {
                const int k = __builtin_ctz(m);
                m &= m - 1u;
                const uint32_t col = (c.order >> (3 * k)) & 7u;
                v.alt_col[j] = (uint8_t)col; v.alt_count[j] = counts[(size_t)p * AMP_NSYM + col]; ++na;
            } else {
                v.alt_col[j] = 0xFF; v.alt_count[j] = 0;
            }
        }
        v.n_alt = na;
        vars[ov] = v;
    }
    if (vb == gridDim.x - 1 && tid == 255) {   // last thread of the last block knows both totals
        n_out[0] = ov + (isv ? 1u : 0u);
        n_out[1] = orl + (isr ? 1u : 0u);
    }
    // The last block through tidies up for the next launch.  The count is a relaxed add: what it has to come after are this
    // block's loads of the flags, and their values were used in front of the barrier.  (As an agent-scope release it makes every
    // block wait for the write-back of its stores to the host image: profiles/small_launches_release_variant.json.)
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(&sync[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)gridDim.x - 1ull;
    __syncthreads();
    if (s_last) {
        if (tid == 0) {
            n_out[2] = __hip_atomic_load(&sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int k = 0; k < 3; ++k) __hip_atomic_store(&sync[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (uint32_t b = (uint32_t)tid; b < gridDim.x; b += 256u) __hip_atomic_store(&flag[b], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Copies the text of insertion events (SEQ[q_from:q_to], A:736-738, upper-cased like A:702)
// out of a device-resident batch: one lane per event.
__global__ void k_event_strings(amp_dev_reads rd, uint64_t read_base, int64_t n_ev, const amp_ins_event *__restrict__ ev,
                                const uint64_t *__restrict__ off, uint8_t *__restrict__ text) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ev) return;
    const char nt16[17] = "=ACMGRSVTWYHKDBN";
    const int64_t i = amp::ins_read_row(ev[e].read, read_base);      // read ids are relative to read_base modulo 2^32, as in k_ins_hash
    const int64_t boff = (int64_t)rd.seq_off8[i] * 8;
    uint8_t *dst = text + off[e];
    for (int32_t q = ev[e].q_from; q < ev[e].q_to; ++q) *dst++ = (uint8_t)nt16[amp::ins_code(rd.seq, boff, q)];
}

// what the device codecs (translation units of their own: amp_codec.hpp) need to know of a ctx
namespace amp {
hipStream_t ctx_stream(const amp_ctx *c) { return c->stream; }
int ctx_device(const amp_ctx *c) { return c->device; }
// ... and the hooks behind the read pass (amp_hook.hpp)
HookCtx ctx_hook(amp_ctx *c) {
    return HookCtx{c->device, c->ref_len, c->stream, c->d_counts, c->do_trim, c->have_primers ? 1 : 0, c->min_quality, c->n_cu, c->err, sizeof(c->err),
                   c->events.as<amp_ins_event>(), (long long)c->ev_cap, c->d_ctr + CTR_EV_SHARD0};
}
HookSlot &hook_slot(amp_ctx *c, int which) { return c->hooks[which]; }
}  // namespace amp

static const HookOps *const HOOKS[N_HOOKS] = {&qc_hook, &strand_hook, &amplicon_hook, &codon_hook, &del_hook, &insev_hook, &cooc_hook, &errprof_hook, &hap_hook, &readpos_hook};      // in the enum's order: the run order

// What the hooks that are on have to note in FRONT of the read pass (HookOps::before_pass, where a unit has one)
static int hooks_before_pass(amp_ctx *c, uint64_t read_base) {
    for (int k = 0; k < N_HOOKS; ++k) {
        if (!c->hooks[k].on || !HOOKS[k]->before_pass) continue;
        const int rc = HOOKS[k]->before_pass(c, read_base);
        if (rc != AMP_OK) return rc;
    }
    return AMP_OK;
}

// The kernels of the hooks that are on, behind the read pass on the ctx stream, until one fails.
static int enqueue_hooks(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *dev_out) {
    for (int k = 0; k < N_HOOKS; ++k) {
        if (!c->hooks[k].on) continue;
        if (!c->hooks[k].state) return AMP_ESTATE;
        const int rc = HOOKS[k]->enqueue(c, rd, dev_out);
        if (rc != AMP_OK) return rc;
    }
    return AMP_OK;
}

// ---------------------------------------------------------------------------------------
// library / context API
// ---------------------------------------------------------------------------------------
extern "C" {

int amp_version(void) { return AMP_ABI_VERSION; }

const char *amp_strerror(int rc) {
    switch (rc) {
        case AMP_OK: return "ok";
        case AMP_EINVAL: return "invalid argument";
        case AMP_ENOMEM: return "out of memory";
        case AMP_EHIP: return "HIP runtime error";
        case AMP_ENODEV: return "no usable GPU device";
        case AMP_ESTATE: return "call order violated";
        case AMP_EOVERFLOW: return "output buffer too small";
        case AMP_ERCCL: return "RCCL unavailable or collective failed";
        default: return "unknown error";
    }
}

const char *amp_last_error(const amp_ctx *ctx) { return ctx ? ctx->err : ""; }

const char *amp_read_status_exception(int status) {
    switch (status) {
        case AMP_RS_OK: return "";
        case AMP_RS_INDEX_REF: case AMP_RS_INDEX_PAIRS: case AMP_RS_INDEX_QUERY: case AMP_RS_CIGAR_OP: return "IndexError";
        case AMP_RS_KEY_BASE: return "KeyError";
        case AMP_RS_NO_SEQ: return "AttributeError";
        case AMP_RS_NO_QUAL: case AMP_RS_TYPE: return "TypeError";
        case AMP_RS_CLIP: return "ValueError";
        default: return "RuntimeError";
    }
}

int amp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// A:174-209.  The reference sweeps positions with a deque of the primers whose
// [start-off, end+off) window is open; stale entries never change min/max, so
// the result equals a plain interval cover.  Here: sweep with an explicit active set kept as
// a start-ordered ring, evaluating min/max over it like the reference does.
int amp_find_overlapping_primers(int32_t ref_len, int32_t n, const int32_t *starts, const int32_t *ends, int32_t off,
                                 int32_t *min_start, int32_t *max_end, int32_t *max_primer_len) {
    if (ref_len < 0 || n < 0 || off < 0 || (n && (!starts || !ends)) || (ref_len && (!min_start || !max_end))) return AMP_EINVAL;
    std::vector<int32_t> ring((size_t)std::max(n, 1));
    int head = 0, tail = 0, next = 0;
    for (int32_t p = 0; p < ref_len; ++p) {
        while (head != tail && p >= ends[ring[head]] + off) ++head;
        while (next < n && p >= starts[next] - off) ring[tail++] = next++;
        int32_t mn = -1, mx = -1;
        for (int k = head; k < tail; ++k) {
            int32_t s = starts[ring[k]], e = ends[ring[k]];
            if (k == head || s < mn) mn = s;
            if (k == head || e > mx) mx = e;
        }
        min_start[p] = mn; max_end[p] = mx;
    }
    if (max_primer_len) {
        int32_t m = 0;
        for (int k = 0; k < n; ++k) m = (k == 0) ? ends[k] - starts[k] : std::max(m, ends[k] - starts[k]);
        *max_primer_len = m;
    }
    return AMP_OK;
}

// Layout of the compact calling image (device and pinned host copy alike)
struct CallImage {
    unsigned nblk; size_t off_blk, off_img, img_cons, img_vars, img_rel, img_size;
    explicit CallImage(int32_t G) {
        nblk = (unsigned)((G + 255) / 256);
        off_blk = (size_t)G * sizeof(amp_pos_call);
        off_img = (off_blk + (size_t)nblk * sizeof(uint2) + 63) & ~(size_t)63;
        img_cons = 64; img_vars = img_cons + (((size_t)G + 63) & ~(size_t)63);
        img_rel = img_vars + (size_t)G * sizeof(amp_var_rec); img_size = img_rel + (size_t)G * 4;
    }
};

int amp_ctx_create(amp_ctx **out, int device, int32_t ref_len) {
    if (!out || ref_len <= 0) return AMP_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AMP_ENODEV;
    if (device < 0 || device >= n) return AMP_ENODEV;
    amp_ctx *c = new (std::nothrow) amp_ctx();
    if (!c) return AMP_ENOMEM;
    c->device = device; c->ref_len = ref_len;
    Guard g(c->device);
    if (!g.ok) { delete c; return AMP_ENODEV; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    auto fail = [&](int rc) { amp_ctx_destroy(c); return rc; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(AMP_EHIP);
    c->own_stream = true;
    size_t cb = (size_t)ref_len * AMP_DEV_COLS * sizeof(uint32_t);   // counts [G][6] followed by the insertion tally [G]
    if (hipMalloc((void **)&c->d_counts, cb) != hipSuccess) return fail(AMP_ENOMEM);
    c->own_counts = true;
    c->d_ins_at = c->d_counts + (size_t)ref_len * AMP_NSYM;
    if (hipMalloc((void **)&c->d_min_start, (size_t)ref_len * 4) != hipSuccess) return fail(AMP_ENOMEM);
    if (hipMalloc((void **)&c->d_max_end, (size_t)ref_len * 4) != hipSuccess) return fail(AMP_ENOMEM);
    if (hipMalloc((void **)&c->d_ctr, CTR_WORDS * sizeof(unsigned long long)) != hipSuccess) return fail(AMP_ENOMEM);
    if (hipMalloc((void **)&c->d_ref, (size_t)ref_len) != hipSuccess) return fail(AMP_ENOMEM);
    if (hipHostMalloc((void **)&c->h_hist, 64, hipHostMallocDefault) != hipSuccess) return fail(AMP_ENOMEM);
    memset(c->h_hist, 0, 64);
    if (hipMemsetAsync(c->d_counts, 0, cb, c->stream) != hipSuccess) return fail(AMP_EHIP);
    if (hipMemsetAsync(c->d_ctr, 0, CTR_WORDS * sizeof(unsigned long long), c->stream) != hipSuccess) return fail(AMP_EHIP);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->ev3) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_call, hipEventDisableTiming) != hipSuccess) return fail(AMP_EHIP);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(AMP_EHIP);
#ifdef AMP_DEV   // development builds only (tools/profile_phases.sh): the shipped library reads no debug switches
    const char *v = getenv("AMPLIHIP_KERNEL");
    if (v && v[0] >= '0' && v[0] <= '5') c->kernel_variant = v[0] - '0';
    v = getenv("AMPLIHIP_PHASES");
    if (v) c->phases = (uint32_t)strtoul(v, nullptr, 0);
#endif
    *out = c;
    return AMP_OK;
}

void amp_ctx_destroy(amp_ctx *c) {
    if (!c) return;
    Guard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int k = 0; k < N_HOOKS; ++k) {
        HOOKS[k]->free_state(c->hooks[k].state);
        c->hooks[k] = HookSlot{false, nullptr};
    }
    if (c->own_counts && c->d_counts) (void)hipFree(c->d_counts);
    if (c->d_min_start) (void)hipFree(c->d_min_start);
    if (c->d_max_end) (void)hipFree(c->d_max_end);
    if (c->d_ctr) (void)hipFree(c->d_ctr);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->h_hist) (void)hipHostFree(c->h_hist);
    if (c->d_ref) (void)hipFree(c->d_ref);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->ev3) (void)hipEventDestroy(c->ev3);
    if (c->ev_call) (void)hipEventDestroy(c->ev_call);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;      // (every DBuf releases its memory; g is still in scope)
}

int amp_ctx_set_stream(amp_ctx *c, void *s) {
    if (!c) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)s;
    c->own_stream = false;
    return AMP_OK;
}

int amp_ctx_bind_counts(amp_ctx *c, void *dev_counts) {
    if (!c || !dev_counts) return AMP_EINVAL;
    Guard g(c->device);
    size_t cb = (size_t)c->ref_len * AMP_DEV_COLS * sizeof(uint32_t);
    HIPCHK(c, hipMemcpyAsync(dev_counts, c->d_counts, cb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_counts) (void)hipFree(c->d_counts);
    c->d_counts = (uint32_t *)dev_counts;
    c->d_ins_at = c->d_counts + (size_t)c->ref_len * AMP_NSYM;
    c->own_counts = false;
    c->call_pending = false;       // (calls begun on the old table are not calls of this one)
    return AMP_OK;
}

int amp_set_primers(amp_ctx *c, const int32_t *mn, const int32_t *mx, int32_t max_primer_len) {
    if (!c || !mn || !mx || max_primer_len < 0) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipMemcpyAsync(c->d_min_start, mn, (size_t)c->ref_len * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_max_end, mx, (size_t)c->ref_len * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->max_primer_len = max_primer_len;
    c->have_primers = true;
    return AMP_OK;
}

int amp_set_params(amp_ctx *c, int32_t min_quality, int32_t window, int32_t do_trim, int32_t do_count) {
    if (!c || min_quality < 0 || window < 1) return AMP_EINVAL;  // A:841-844
    // (new values: the passes so far say nothing about the lists of the next one)
    if (c->min_quality != min_quality || c->window != window || c->do_trim != (do_trim != 0) || c->do_count != (do_count != 0)) c->hist_from = c->epoch + 1;
    c->min_quality = min_quality; c->window = window; c->do_trim = do_trim != 0; c->do_count = do_count != 0;
    return AMP_OK;
}

// 0 = by the batch, 1 = lane per read, 2 = fused tile kernel, 3 = split pipeline, 4 / 5 / 6 / 7 = a fast kernel (its four
// generations) + the general pass
int amp_set_kernel_variant(amp_ctx *c, int variant) {
    if (!c || variant < 0 || variant > 7) return AMP_EINVAL;
    if (c->kernel_variant != variant) c->hist_from = c->epoch + 1;
    c->kernel_variant = variant;
    return AMP_OK;
}

int amp_fast_path_active(amp_ctx *c) {
    if (!c) return AMP_EINVAL;
    return fast_path_active(c->kernel_variant, c->window, c->min_quality) ? 1 : 0;
}

int amp_last_kernel_variant(amp_ctx *c) {
    if (!c) return AMP_EINVAL;
    return c->last_kv;
}

int amp_set_cu_share(amp_ctx *c, int divisor) {
    if (!c || divisor < 1 || divisor > 16) return AMP_EINVAL;
    if (c->cu_share != divisor) c->hist_from = c->epoch + 1;
    c->cu_share = divisor;
    return AMP_OK;
}

int amp_debug_second_grids(amp_ctx *c, int gen_blocks, int heavy_blocks) {
    if (!c || gen_blocks < 0 || heavy_blocks < 0) return AMP_EINVAL;
    c->force_gen_blocks = gen_blocks; c->force_heavy_blocks = heavy_blocks;
    return AMP_OK;
}

int amp_debug_last_second_grids(amp_ctx *c, int *gen_blocks, int *heavy_blocks) {
    if (!c || !gen_blocks || !heavy_blocks) return AMP_EINVAL;
    *gen_blocks = c->last_gen_blocks; *heavy_blocks = c->last_heavy_blocks;
    return AMP_OK;
}

int amp_debug_event_capacity(amp_ctx *c, int64_t *per_shard) {
    if (!c || !per_shard) return AMP_EINVAL;
    *per_shard = c->ev_cap;
    return AMP_OK;
}

int amp_set_timing(amp_ctx *c, int split) {
    if (!c) return AMP_EINVAL;
    c->split_timing = split != 0;
    return AMP_OK;
}

int amp_reserve_events(amp_ctx *c, int64_t cap) {
    if (!c || cap < 0) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, grow_events(c, cap));
    c->ev_reserved = true;
    return AMP_OK;
}

int amp_sync(amp_ctx *c) {
    if (!c) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

int amp_process_batch_device(amp_ctx *c, const amp_dev_reads *rd, uint64_t read_base, const amp_trim_out *dev_out) {
    if (!c || !rd || rd->n_reads < 0) return AMP_EINVAL;
    if (rd->n_reads && (!rd->pos || !rd->flag || !rd->tlen || !rd->lseq || !rd->cig_off32 || !rd->cig || !rd->seq_off8 ||
                        !rd->seq || !rd->qual)) return AMP_EINVAL;
    Guard g(c->device);
    c->staged_n = -1;          // (amp_event_strings(reads = NULL) refers to the last HOST batch: there is none now)
    for (int k = 0; k < N_HOOKS && rd->n_reads; ++k) {      // in front of the pass: a refused call changes nothing
        if (!c->hooks[k].on) continue;
        const int rc = hook_check_out(ctx_hook(c), dev_out, *HOOKS[k]);
        if (rc != AMP_OK) return rc;
    }
    int rc = hooks_before_pass(c, read_base);
    if (rc == AMP_OK) rc = launch_reads(c, rd, read_base, dev_out);
    return rc != AMP_OK ? rc : enqueue_hooks(c, rd, dev_out);
}

int amp_process_batch(amp_ctx *c, const amp_reads *r, uint64_t read_base, const amp_trim_out *out) {
    if (!c || !r || r->n_reads < 0) return AMP_EINVAL;
    const int64_t n = r->n_reads;
    if (n == 0) return AMP_OK;
    if (!r->pos || !r->flag || !r->tlen || !r->lseq || !r->cig_off || !r->cig || !r->seq_off || !r->seq || !r->qual) return AMP_EINVAL;
    Guard g(c->device);
    const uint64_t n_cig = r->cig_off[n], n_bases = r->seq_off[n];
    if (n_cig > 0xFFFFFFF0ull || (n_bases >> 3) > 0xFFFFFFF0ull || (n_bases & 7)) return AMP_EINVAL;
    std::vector<uint32_t> co((size_t)n + 1), so((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) {
        if (r->seq_off[i] & 7) return AMP_EINVAL;
        if (i < n && (r->cig_off[i + 1] < r->cig_off[i] || r->seq_off[i + 1] < r->seq_off[i] + r->lseq[i])) return AMP_EINVAL;
        co[(size_t)i] = (uint32_t)r->cig_off[i];
        so[(size_t)i] = (uint32_t)(r->seq_off[i] >> 3);
    }
    hipStream_t s = c->stream;
    struct Up { DBuf *b; const void *src; size_t bytes; };
    Up ups[] = {{&c->s_pos, r->pos, (size_t)n * 4}, {&c->s_flag, r->flag, (size_t)n * 2}, {&c->s_tlen, r->tlen, (size_t)n * 4},
                {&c->s_lseq, r->lseq, (size_t)n * 4}, {&c->s_cigoff, co.data(), ((size_t)n + 1) * 4},
                {&c->s_cig, r->cig, (size_t)n_cig * 4}, {&c->s_seqoff, so.data(), ((size_t)n + 1) * 4},
                {&c->s_seq, r->seq, (size_t)(n_bases / 2)}, {&c->s_qual, r->qual, (size_t)n_bases}};
    for (Up &u : ups) {
        HIPCHK(c, u.b->ensure(u.bytes + 16));  // +16: tile loads may read one vector past the end
        if (u.bytes) HIPCHK(c, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const size_t slots = (size_t)n_cig + 3 * (size_t)n;
    HIPCHK(c, c->o_pos.ensure((size_t)n * 4)); HIPCHK(c, c->o_ncig.ensure((size_t)n * 4));
    HIPCHK(c, c->o_cig.ensure(slots * 4)); HIPCHK(c, c->o_reflen.ensure((size_t)n * 4));
    HIPCHK(c, c->o_flags.ensure((size_t)n)); HIPCHK(c, c->o_status.ensure((size_t)n));
    c->staged_n = n; c->staged_ncig = (int64_t)n_cig; c->staged_nbases = (int64_t)n_bases;
    const amp_dev_reads rd = staged_reads(c);
    amp_trim_out dout{c->o_pos.as<int32_t>(), c->o_ncig.as<uint32_t>(), c->o_cig.as<uint32_t>(), c->o_reflen.as<int32_t>(),
                      c->o_flags.as<uint8_t>(), c->o_status.as<uint8_t>()};
    int rc = hooks_before_pass(c, read_base);
    if (rc == AMP_OK) rc = launch_reads(c, &rd, read_base, &dout);
    if (rc != AMP_OK) return rc;
    rc = enqueue_hooks(c, &rd, &dout);         // (no check in front of the pass here: dout is always complete)
    if (rc != AMP_OK) return rc;
    if (out) {
        if (out->new_pos) HIPCHK(c, hipMemcpyAsync(out->new_pos, dout.new_pos, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (out->new_ncig) HIPCHK(c, hipMemcpyAsync(out->new_ncig, dout.new_ncig, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (out->new_cig) HIPCHK(c, hipMemcpyAsync(out->new_cig, dout.new_cig, slots * 4, hipMemcpyDeviceToHost, s));
        if (out->ref_len) HIPCHK(c, hipMemcpyAsync(out->ref_len, dout.ref_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (out->trim_flags) HIPCHK(c, hipMemcpyAsync(out->trim_flags, dout.trim_flags, (size_t)n, hipMemcpyDeviceToHost, s));
        if (out->status) HIPCHK(c, hipMemcpyAsync(out->status, dout.status, (size_t)n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return AMP_OK;
}

int amp_last_kernel_ms(amp_ctx *c, float *total_ms, float *scan_ms) {
    if (!c) return AMP_EINVAL;
    if (!c->timed) return AMP_ESTATE;
    Guard g(c->device);
    HIPCHK(c, hipEventSynchronize(c->ev3));
    float t = 0, s = 0;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev0, c->ev3));
    if (!c->last_split) s = t;     // (the first kernel was not timed separately)
    else HIPCHK(c, hipEventElapsedTime(&s, c->ev1, c->ev2));
    if (total_ms) *total_ms = t;
    if (scan_ms) *scan_ms = s;
    return AMP_OK;
}

int amp_get_counts(amp_ctx *c, uint32_t *counts) {
    if (!c || !counts) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipMemcpyAsync(counts, c->d_counts, (size_t)c->ref_len * AMP_NSYM * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

int amp_add_counts(amp_ctx *c, const uint32_t *counts) {
    if (!c || !counts) return AMP_EINVAL;
    Guard g(c->device);
    size_t n = (size_t)c->ref_len * AMP_NSYM;
    c->call_pending = false;       // the table changes: calls begun earlier are for the table as it was
    HIPCHK(c, c->call_buf.ensure(n * 4));
    HIPCHK(c, hipMemcpyAsync(c->call_buf.p, counts, n * 4, hipMemcpyHostToDevice, c->stream));
    k_add_u32<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->d_counts, c->call_buf.as<uint32_t>(), (int64_t)n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

void *amp_counts_device_ptr(amp_ctx *c) { return c ? c->d_counts : nullptr; }

int amp_get_ins_events(amp_ctx *c, int64_t *n, amp_ins_event *buf, int64_t cap) {
    if (!c || !n) return AMP_EINVAL;
    Guard g(c->device);
    unsigned long long h[EV_SHARDS];
    HIPCHK(c, hipMemcpyAsync(h, &c->d_ctr[CTR_EV_SHARD0], sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t total = 0;
    bool dropped = false;
    for (int s = 0; s < EV_SHARDS; ++s) { total += (int64_t)h[s]; if ((int64_t)h[s] > c->ev_cap) dropped = true; }
    *n = total;
    if (dropped) return AMP_EOVERFLOW;   // a reserved buffer was too small: events were dropped
    if (buf) {
        if (total > cap) return AMP_EOVERFLOW;
        int64_t o = 0;
        for (int s = 0; s < EV_SHARDS; ++s) {
            if (h[s]) HIPCHK(c, hipMemcpyAsync(buf + o, c->events.as<amp_ins_event>() + (size_t)s * c->ev_cap,
                                               (size_t)h[s] * sizeof(amp_ins_event), hipMemcpyDeviceToHost, c->stream));
            o += (int64_t)h[s];
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int64_t w = 0;                                   // slots a read reserved and did not use carry ref_pos = -1
        for (int64_t k = 0; k < total; ++k)
            if (buf[k].ref_pos >= 0) { if (w != k) buf[w] = buf[k]; ++w; }
        *n = w;
    }
    return AMP_OK;
}

int amp_drain_ins_events(amp_ctx *c, int64_t *n, amp_ins_event *buf, int64_t cap) {
    // amp_get_ins_events, then the list starts over (the per-position tally stays): a run of many batches reads every
    // event once instead of the whole accumulated list after each batch, and the device list stays one batch long
    const int rc = amp_get_ins_events(c, n, buf, cap);
    if (rc != AMP_OK || !buf) return rc;
    Guard g(c->device);
    HIPCHK(c, hipMemsetAsync(&c->d_ctr[CTR_EV_SHARD0], 0, EV_SHARDS * sizeof(unsigned long long), c->stream));
    return AMP_OK;
}

int amp_aggregate_ins_events(amp_ctx *c, const amp_dev_reads *rd, uint64_t read_base, int drain, int64_t *n_runs, amp_ins_run *buf, int64_t cap) {
    if (!c || !n_runs) return AMP_EINVAL;
    if (!rd && c->staged_n < 0) return AMP_ESTATE;       // no batch to read the alleles from: the size query says so, too
    Guard g(c->device);
    unsigned long long h[EV_SHARDS];
    HIPCHK(c, hipMemcpyAsync(h, &c->d_ctr[CTR_EV_SHARD0], sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t total = 0;
    for (int s = 0; s < EV_SHARDS; ++s) { if ((int64_t)h[s] > c->ev_cap) return AMP_EOVERFLOW; total += (int64_t)h[s]; }
    *n_runs = total;
    if (!buf) return AMP_OK;
    if (total > cap) return AMP_EOVERFLOW;
    amp_dev_reads staged;
    if (!rd) {
        staged = staged_reads(c);
        rd = &staged;
    }
    int64_t n_ev = 0, nr = 0;
    if (total) {
        const size_t sb = amp::ins_scratch_bytes(total), rb = (((size_t)total * sizeof(amp_ins_run)) + 255) & ~(size_t)255;
        HIPCHK(c, c->agg_buf.ensure(sb + rb));
        amp_ins_run *d_runs = (amp_ins_run *)c->agg_buf.p;
        const int rc = amp::ins_aggregate(c->stream, *rd, read_base, c->events.as<amp_ins_event>(), (long long)c->ev_cap, h,
                                          (uint8_t *)c->agg_buf.p + rb, d_runs, &n_ev, &nr);
        if (rc != 0) { snprintf(c->err, sizeof(c->err), "insertion-event aggregation failed: %d", rc); return AMP_EHIP; }
        if (nr) HIPCHK(c, hipMemcpyAsync(buf, d_runs, (size_t)nr * sizeof(amp_ins_run), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *n_runs = nr;
    if (drain) HIPCHK(c, hipMemsetAsync(&c->d_ctr[CTR_EV_SHARD0], 0, EV_SHARDS * sizeof(unsigned long long), c->stream));
    return AMP_OK;
}

int amp_debug_blocks(amp_ctx *c, uint32_t *out, int cap_blocks, int *n_blocks) {   // [block][dur, rebases, p2 chunks, p4 chunks]
    if (!c || !out || !n_blocks || !c->dbg_dcnt) return AMP_EINVAL;
    Guard g(c->device);
    int nb = c->dbg_grid < cap_blocks ? c->dbg_grid : cap_blocks;
    HIPCHK(c, hipMemcpyAsync(out, c->dbg_dcnt + c->dbg_grid + 64, (size_t)nb * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_blocks = nb;
    return AMP_OK;
}

int amp_debug_counters(amp_ctx *c, uint64_t *out16) {  // raw device counters (development aid)
    if (!c || !out16) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipMemcpyAsync(out16, c->d_ctr, CTR_DEBUG_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->kernel_variant != 1 && c->dbg_dcnt && c->dbg_grid > 0) {      // [3]: deferred reads of the LAST batch, from the per-block list counts
        std::vector<uint32_t> h((size_t)c->dbg_grid * 6 + 64);
        HIPCHK(c, hipMemcpyAsync(h.data(), c->dbg_dcnt, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint64_t tot = 0, heavy = 0;
        for (int b = 0; b < c->dbg_grid; ++b) { tot += h[(size_t)b]; heavy += h[(size_t)c->dbg_grid * 5 + 64 + (size_t)b]; }
        out16[3] = tot + heavy;
        out16[0] = heavy;                         // [0]: of which heavy entries (whole read / exact status)
    }
    return AMP_OK;
}

int amp_error_reads(amp_ctx *c, int64_t *n) {  // reads with a non-zero status since the last reset
    if (!c || !n) return AMP_EINVAL;
    Guard g(c->device);
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, &c->d_ctr[CTR_ERROR_READS], sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = (int64_t)h;
    return AMP_OK;
}

int amp_reset(amp_ctx *c) {
    if (!c) return AMP_EINVAL;
    Guard g(c->device);
    c->call_pending = false;
    // one small kernel for the table and the counters (two hipMemsetAsync calls are three fill kernels of 5 us each)
    const size_t words = (size_t)c->ref_len * AMP_DEV_COLS;
    constexpr size_t ctr_words = 2 * CTR_WORDS;      // the 64-bit counters as the 32-bit words k_reset writes
    k_reset<<<std::min<unsigned>(RESET_BLOCKS, (unsigned)((words + ctr_words + 1023) / 1024)), 256, 0, c->stream>>>(c->d_counts, words, (uint32_t *)c->d_ctr, ctr_words);
    HIPCHK(c, hipGetLastError());
    for (int k = 0; k < N_HOOKS; ++k) {        // (... and the tables of every hook that has some, on or off)
        if (!c->hooks[k].state) continue;
        const int rc = hook_zero(ctx_hook(c), *(const HookState *)c->hooks[k].state);
        if (rc != AMP_OK) return rc;
    }
    return AMP_OK;
}

// RCCL is resolved at run time so the library has no link-time dependency on it and uses
// whichever librccl the process (e.g. torch) already loaded.
typedef int (*nccl_reduce_fn)(const void *, void *, size_t, int, int, int, void *, hipStream_t);
typedef int (*nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
int amp_reduce(amp_ctx *c, void *comm, int root) {
    if (!c) return AMP_EINVAL;
    if (!comm) return AMP_OK;
    Guard g(c->device);
    c->call_pending = false;       // the table changes: calls begun earlier are for the un-reduced table
    void *h = dlopen(nullptr, RTLD_NOW);
    void *f_red = h ? dlsym(h, "ncclReduce") : nullptr;
    void *f_all = h ? dlsym(h, "ncclAllReduce") : nullptr;
    if (!f_red || !f_all) {
        void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (lib) { f_red = dlsym(lib, "ncclReduce"); f_all = dlsym(lib, "ncclAllReduce"); }
    }
    if (!f_red || !f_all) { snprintf(c->err, sizeof(c->err), "RCCL symbols not found"); return AMP_ERCCL; }
    const size_t cnt = (size_t)c->ref_len * AMP_DEV_COLS;
    const int nccl_uint32 = 3, nccl_sum = 0;
    int rc = root < 0 ? ((nccl_allreduce_fn)f_all)(c->d_counts, c->d_counts, cnt, nccl_uint32, nccl_sum, comm, c->stream)
                      : ((nccl_reduce_fn)f_red)(c->d_counts, c->d_counts, cnt, nccl_uint32, nccl_sum, root, comm, c->stream);
    if (rc != 0) { snprintf(c->err, sizeof(c->err), "RCCL reduce failed: %d", rc); return AMP_ERCCL; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

// ---------------------------------------------------------------------------------------
// calling (A:756-771, A:917-952)
// ---------------------------------------------------------------------------------------
int amp_set_reference(amp_ctx *c, const uint8_t *ref_ascii) {
    if (!c || !ref_ascii) return AMP_EINVAL;
    Guard g(c->device);
    HIPCHK(c, hipMemcpyAsync(c->d_ref, ref_ascii, (size_t)c->ref_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_ref = true;
    return AMP_OK;
}

int amp_call_positions(amp_ctx *c, const amp_call_params *pr, amp_pos_call *out, int64_t *n_relevant) {
    if (!c || !pr || !out) return AMP_EINVAL;
    if (pr->run_variants && !c->have_ref) return AMP_ESTATE;
    Guard g(c->device);
    const int32_t G = c->ref_len;
    HIPCHK(c, c->call_buf.ensure((size_t)G * sizeof(amp_pos_call)));
    HIPCHK(c, hipMemsetAsync(&c->d_ctr[CTR_CALL_RELEVANT], 0, sizeof(unsigned long long), c->stream));
    k_call<<<(unsigned)((G + 255) / 256), 256, 0, c->stream>>>(c->d_counts, c->d_ins_at, c->d_ref, G, *pr,
                                                              c->call_buf.as<amp_pos_call>(), &c->d_ctr[CTR_CALL_RELEVANT], nullptr);
    HIPCHK(c, hipGetLastError());
    unsigned long long nr = 0;
    HIPCHK(c, hipMemcpyAsync(out, c->call_buf.p, (size_t)G * sizeof(amp_pos_call), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nr, &c->d_ctr[CTR_CALL_RELEVANT], sizeof(nr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_relevant) *n_relevant = (int64_t)nr;
    return AMP_OK;
}

// Enqueues the calling kernels on the ctx stream; does not wait.  (The caller has read the image of the ctx's previous call:
// the views are valid until the next call_* on the ctx.)
static int call_compact_enqueue(amp_ctx *c, const amp_call_params *pr, bool pinned) {
    const int32_t G = c->ref_len;
    // device buffer: [per-position calls][block counts]( + the image when it is copied); host: the output image [totals 64 B]
    // [consensus][records][relevant positions]
    const CallImage L(G);
    HIPCHK(c, c->call_buf.ensure(L.off_img + (pinned ? 64 : L.img_size)));
    uint8_t *base = c->call_buf.as<uint8_t>();
    amp_pos_call *d_pc = (amp_pos_call *)base;
    uint8_t *hz;
    if (pinned) {
        // Pipelined callers (amp_call_compact_begin): the result image is written by the compaction kernel straight into a
        // pinned host buffer (plain stores over the host link; half a megabyte): no copy to place.  A copy on a stream of its
        // own was only served once the kernels queued behind the calls had drained (0.61 ms per step with three steps in flight
        // instead of 0.31), a copy in the work stream cost a launch gap more (0.308 -> 0.294 ms per bench step with this).
        if (c->h_pin_cap < L.img_size) {
            if (c->h_pin) (void)hipHostFree(c->h_pin);
            c->h_pin = nullptr; c->h_pin_cap = 0;
            HIPCHK(c, hipHostMalloc(&c->h_pin, L.img_size, hipHostMallocDefault));
            c->h_pin_cap = L.img_size;
        }
        hz = (uint8_t *)c->h_pin;
    } else {
        // One-shot callers (a command line: one view per run): no page-locked memory.  In a process that has just mapped and
        // released hundreds of MB of host memory (a BAM inflated piece by piece) hipHostMalloc / hipHostFree of this 1.5 MB
        // image took 25-70 ms each (rocprofv3 --hip-trace), a third of a `variants` run over 1.5 M reads; a device image and
        // one 1.5 MB copy take 0.3 ms.
        hz = base + L.off_img;
        if (c->h_img.size() < L.img_size) c->h_img.resize(L.img_size);
    }
    if (pinned) {
        // one launch (k_call_fused); its flags are zero from the allocation on: every launch leaves them so
        const size_t sync_bytes = ((size_t)CALL_SYNC_FLAG0 + L.nblk) * sizeof(unsigned long long);
        if (c->call_sync.cap < sync_bytes) {
            HIPCHK(c, c->call_sync.ensure(sync_bytes));
            HIPCHK(c, hipMemsetAsync(c->call_sync.p, 0, c->call_sync.cap, c->stream));
        }
        k_call_fused<<<L.nblk, 256, 0, c->stream>>>(c->d_counts, c->d_ins_at, c->d_ref, G, *pr, (int8_t *)(hz + L.img_cons), (amp_var_rec *)(hz + L.img_vars),
                                                    (int32_t *)(hz + L.img_rel), (unsigned long long *)hz, c->call_sync.as<unsigned long long>());
        HIPCHK(c, hipGetLastError());
    } else {
        k_call<<<L.nblk, 256, 0, c->stream>>>(c->d_counts, c->d_ins_at, c->d_ref, G, *pr, d_pc, nullptr, (uint2 *)(base + L.off_blk));
        HIPCHK(c, hipGetLastError());
        k_call_compact<<<L.nblk, 256, 0, c->stream>>>(d_pc, c->d_counts, G, (const uint2 *)(base + L.off_blk), (int8_t *)(hz + L.img_cons),
                                                      (amp_var_rec *)(hz + L.img_vars), (int32_t *)(hz + L.img_rel), (unsigned long long *)hz);
        HIPCHK(c, hipGetLastError());
    }
    if (!pinned) HIPCHK(c, hipMemcpyAsync(c->h_img.data(), hz, L.img_size, hipMemcpyDeviceToHost, c->stream));
    c->img_pinned = pinned;
    HIPCHK(c, hipEventRecord(c->ev_call, c->stream));     // "the image has arrived"
    return AMP_OK;
}

int amp_call_compact_begin(amp_ctx *c, const amp_call_params *pr) {
    if (!c || !pr) return AMP_EINVAL;
    if (pr->run_variants && !c->have_ref) return AMP_ESTATE;
    Guard g(c->device);
    const int rc = call_compact_enqueue(c, pr, true);
    if (rc != AMP_OK) return rc;
    c->call_pending = true; c->call_pending_params = *pr;     // (the view waits for the copy's event, not for what is enqueued behind it)
    return AMP_OK;
}

int amp_call_compact_view(amp_ctx *c, const amp_call_params *pr, amp_call_view *view) {
    if (!c || !pr || !view) return AMP_EINVAL;
    if (pr->run_variants && !c->have_ref) return AMP_ESTATE;
    Guard g(c->device);
    const int32_t G = c->ref_len;
    const CallImage L(G);
    // work enqueued by amp_call_compact_begin with the same parameters is picked up here; anything else starts now
    const bool begun = c->call_pending && memcmp(&c->call_pending_params, pr, sizeof(*pr)) == 0;
    c->call_pending = false;
    if (!begun) { const int rc = call_compact_enqueue(c, pr, false); if (rc != AMP_OK) return rc; }
    uint8_t *hp = c->img_pinned ? (uint8_t *)c->h_pin : c->h_img.data();
    const unsigned long long *h_nn = (const unsigned long long *)hp;
    const int8_t *h_cons = (const int8_t *)(hp + L.img_cons);
    amp_var_rec *h_vars = (amp_var_rec *)(hp + L.img_vars);
    int32_t *h_rel = (int32_t *)(hp + L.img_rel);
    HIPCHK(c, hipEventSynchronize(c->ev_call));
    if (c->img_pinned && h_nn[2] != 0ull) {
        // (a launch that lost a block may not have left its ticket and flags zero: clear them for the next one)
        if (c->call_sync.p) HIPCHK(c, hipMemsetAsync(c->call_sync.p, 0, c->call_sync.cap, c->stream));
        snprintf(c->err, sizeof(c->err), "the calling kernel gave up waiting for one of its blocks"); return AMP_EHIP;
    }
    const int64_t nv = (int64_t)h_nn[0], nr = (int64_t)h_nn[1];
    *view = amp_call_view{h_cons, h_vars, h_rel, nv, nr};
    return AMP_OK;
}

int amp_call_compact(amp_ctx *c, const amp_call_params *pr, int8_t *consensus, amp_var_rec *vars, int64_t vars_cap,
                     int64_t *n_vars, int32_t *relevant, int64_t relevant_cap, int64_t *n_relevant) {
    if (!c || !pr || !consensus || !n_vars || !n_relevant || vars_cap < 0 || relevant_cap < 0) return AMP_EINVAL;
    amp_call_view v;
    const int rc = amp_call_compact_view(c, pr, &v);
    if (rc != AMP_OK) return rc;
    *n_vars = v.n_vars; *n_relevant = v.n_relevant;
    if (v.n_vars > vars_cap || v.n_relevant > relevant_cap) return AMP_EOVERFLOW;
    memcpy(consensus, v.consensus, (size_t)c->ref_len);
    if (v.n_vars && vars) memcpy(vars, v.vars, (size_t)v.n_vars * sizeof(amp_var_rec));
    if (v.n_relevant && relevant) memcpy(relevant, v.relevant, (size_t)v.n_relevant * 4);
    return AMP_OK;
}

int amp_event_strings(amp_ctx *c, const amp_dev_reads *rd, uint64_t read_base, int64_t n_ev, const amp_ins_event *ev,
                      const uint64_t *off, uint8_t *text) {
    if (!c || n_ev < 0 || (n_ev && (!ev || !off || !text))) return AMP_EINVAL;
    if (n_ev == 0) return AMP_OK;
    amp_dev_reads staged;
    if (!rd) {
        if (c->staged_n < 0) return AMP_ESTATE;
        staged = staged_reads(c);
        rd = &staged;
    }
    for (int64_t e = 0; e < n_ev; ++e) {
        const int64_t i = amp::ins_read_row(ev[e].read, read_base);
        if (i >= rd->n_reads || ev[e].q_from < 0 || ev[e].q_to < ev[e].q_from ||
            off[e + 1] - off[e] != (uint64_t)(ev[e].q_to - ev[e].q_from)) return AMP_EINVAL;
    }
    Guard g(c->device);
    const size_t tb = (size_t)off[n_ev];
    const size_t need = (size_t)n_ev * sizeof(amp_ins_event) + ((size_t)n_ev + 1) * 8 + tb + 64;
    HIPCHK(c, c->call_buf.ensure(need));
    uint8_t *base = c->call_buf.as<uint8_t>();
    uint64_t *d_off = (uint64_t *)base;
    amp_ins_event *d_ev = (amp_ins_event *)(base + ((size_t)n_ev + 1) * 8);
    uint8_t *d_text = (uint8_t *)(d_ev + n_ev);
    HIPCHK(c, hipMemcpyAsync(d_off, off, ((size_t)n_ev + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ev, ev, (size_t)n_ev * sizeof(amp_ins_event), hipMemcpyHostToDevice, c->stream));
    k_event_strings<<<(unsigned)((n_ev + 255) / 256), 256, 0, c->stream>>>(*rd, read_base, n_ev, d_ev, d_off, d_text);
    HIPCHK(c, hipGetLastError());
    if (tb) HIPCHK(c, hipMemcpyAsync(text, d_text, tb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMP_OK;
}

}  // extern "C"
