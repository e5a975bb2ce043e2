// amp_codec.hpp -- the host shell the device codecs share: amp_sam.hip (SAM text) and amp_bgzf.hip (BAM
// input, section 11).  A codec brings its lane functions, its Buf, its carve() and its sequence of stages; everything around
// them is here: what a codec needs to know of a ctx, the stream helpers, the scan, the stage events, the packed batch a codec
// builds (Batch) and hands to amp_process_batch_device, the results of that pass (Trim) and the first failing row.
//
// Like the lane functions, the shell compiles twice: for HIP, and for the host twins (AMPSAM_HOSTSIM or AMPBGZF_HOSTSIM: any C++
// compiler, no HIP headers), where a copy is a memcpy, a launch a loop and a wait nothing.
// A struct that holds a Shell names it `sh` and its Buf `b` (CODEC_RUN).
#pragma once

#if defined(AMPSAM_HOSTSIM) || defined(AMPBGZF_HOSTSIM)
#define AMP_CODEC_HOSTSIM 1
#endif

#ifndef AMP_CODEC_HOSTSIM
#include <hip/hip_runtime.h>
#endif

#include "../../include/amplihip.h"

#ifndef AMP_CODEC_HOSTSIM
namespace amp {

hipStream_t ctx_stream(const amp_ctx *ctx);      // the stream all work of the ctx runs on
int ctx_device(const amp_ctx *ctx);

}  // namespace amp
#endif

#ifndef AMP_CODEC_CTX_ONLY          // (amplihip.hip defines the two functions above and wants nothing else)
#ifndef AMP_CODEC_HOSTSIM
#include <hipcub/hipcub.hpp>
#define AMP_HD __host__ __device__ __forceinline__
#else
#define AMP_HD static inline
#endif

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#if defined(__HIP_DEVICE_COMPILE__)
#define AMP_MIN64(p, v) atomicMin((unsigned long long *)(p), (unsigned long long)(v))
#define AMP_ADD64(p, v) atomicAdd((unsigned long long *)(p), (unsigned long long)(v))
#else
#define AMP_MIN64(p, v) do { if ((unsigned long long)(v) < *(p)) *(p) = (unsigned long long)(v); } while (0)
#define AMP_ADD64(p, v) do { *(p) += (unsigned long long)(v); } while (0)
#endif
#define CODEC_OK(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

namespace ampcodec {

// The packed batch in a codec's memory (amp_dev_reads) with the rows' records.
struct Batch {
    int32_t *pos; uint16_t *flag; int32_t *tlen; uint32_t *lseq, *cig_off32, *cig, *seq_off8; uint8_t *seq, *qual;
    int64_t *src_index;
};
// The results of the read pass (amp_trim_out) as a later stage reads them.
struct Trim { const int32_t *new_pos; const uint32_t *new_ncig, *new_cig; const int32_t *ref_len; const uint8_t *trim_flags, *status; };

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// Hands out 256-byte aligned pieces of `base` (NULL: sizes only); `o` = the bytes handed out.
struct Carver {
    uint8_t *base; size_t o = 0;
    uint8_t *operator()(size_t bytes) { uint8_t *p = base ? base + o : nullptr; o += up256(bytes); return p; }
};

AMP_HD void lane_first_bad(const uint8_t *status, unsigned long long *key, int64_t r) {
    if (status[r]) AMP_MIN64(key, ((unsigned long long)r << 8) | status[r]);
}
typedef void (*FirstBadFn)(const uint8_t *status, unsigned long long *key, int64_t n);

enum { MAX_STAGES = 16 };

struct Shell {
    int n_stages = 0;
    bool timed = false;
    int64_t waits = 0;                                   // waits for the stream on the steady path (growth does not count)
    uint8_t *res = nullptr; size_t res_cap = 0;          // results of the read pass, the key of the first failing row behind them
    unsigned long long *bad_key = nullptr;
    FirstBadFn first_bad = nullptr;                      // the codec's CODEC_FIRST_BAD_KERNEL
#ifndef AMP_CODEC_HOSTSIM
    amp_ctx *ctx = nullptr; int device = 0; hipStream_t stream = nullptr;
    void *scan_tmp = nullptr; size_t scan_tmp_cap = 0;
    hipEvent_t ev[MAX_STAGES + 1] = {};
#endif
};

// ---- the two back ends: HIP on the ctx stream, or plain loops ---------------------------------------------------------------------
#ifndef AMP_CODEC_HOSTSIM
// lane = element i of n (of min(n, b.ctl[ctl]) for ctl >= 0), 256 lanes a workgroup, grid-stride
#define CODEC_KERNEL(name, fn)                                                                                        \
    __global__ void __launch_bounds__(256) name(Buf b, int64_t n, int ctl) {                                          \
        if (ctl >= 0 && (int64_t)b.ctl[ctl] < n) n = (int64_t)b.ctl[ctl];                                             \
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) fn(b, i);     \
    }
#define CODEC_FIRST_BAD_KERNEL(name)                                                                                  \
    __global__ void __launch_bounds__(256) name(const uint8_t *status, unsigned long long *key, int64_t n) {          \
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ampcodec::lane_first_bad(status, key, i); \
    }
#define CODEC_TRY(call) do { if ((call) != hipSuccess) return AMP_EHIP; } while (0)
#define CODEC_RUN(s, k, fn, n, cx) do { if ((n) > 0) { k<<<ampcodec::codec_grid(n), 256, 0, (s)->sh.stream>>>((s)->b, (int64_t)(n), (cx)); if (hipGetLastError() != hipSuccess) return AMP_EHIP; } } while (0)

struct DevGuard {
    int prev = -1;
    explicit DevGuard(const Shell &sh) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != sh.device) (void)hipSetDevice(sh.device); }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
static int codec_alloc(uint8_t **p, size_t bytes) { return hipMalloc((void **)p, bytes) == hipSuccess ? AMP_OK : AMP_ENOMEM; }
static void codec_free(void *p) { if (p) (void)hipFree(p); }
static int codec_copy(Shell &sh, void *dst, const void *src, size_t n, hipMemcpyKind kind) { return !n || hipMemcpyAsync(dst, src, n, kind, sh.stream) == hipSuccess ? AMP_OK : AMP_EHIP; }
static int codec_up(Shell &sh, void *dst, const void *src, size_t n) { return codec_copy(sh, dst, src, n, hipMemcpyHostToDevice); }
static int codec_down(Shell &sh, void *dst, const void *src, size_t n) { return codec_copy(sh, dst, src, n, hipMemcpyDeviceToHost); }
static int codec_d2d(Shell &sh, void *dst, const void *src, size_t n) { return codec_copy(sh, dst, src, n, hipMemcpyDeviceToDevice); }
static int codec_zero(Shell &sh, void *p, int v, size_t n) { return !n || hipMemsetAsync(p, v, n, sh.stream) == hipSuccess ? AMP_OK : AMP_EHIP; }
static int codec_sync(Shell &sh) { return hipStreamSynchronize(sh.stream) == hipSuccess ? AMP_OK : AMP_EHIP; }
static unsigned codec_grid(int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g); }
static void codec_mark(Shell &sh, int k) { if (sh.timed) (void)hipEventRecord(sh.ev[k], sh.stream); }
template <class T> static int codec_scan(Shell &sh, T *p, int64_t n) {      // exclusive sum in place
    if (n <= 0) return AMP_OK;
    size_t need = 0;
    CODEC_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, p, p, (int)n, sh.stream));
    if (need > sh.scan_tmp_cap) {
        if (sh.scan_tmp) { CODEC_OK(codec_sync(sh)); (void)hipFree(sh.scan_tmp); sh.scan_tmp = nullptr; sh.scan_tmp_cap = 0; }
        if (hipMalloc(&sh.scan_tmp, 2 * need + 256) != hipSuccess) return AMP_ENOMEM;
        sh.scan_tmp_cap = 2 * need + 256;
    }
    size_t tb = sh.scan_tmp_cap;
    CODEC_TRY(hipcub::DeviceScan::ExclusiveSum(sh.scan_tmp, tb, p, p, (int)n, sh.stream));
    return AMP_OK;
}
static int codec_run_first_bad(Shell &sh, const uint8_t *status, int64_t n) {
    if (n <= 0) return AMP_OK;
    void *args[] = {&status, &sh.bad_key, &n};
    return hipLaunchKernel((const void *)sh.first_bad, dim3(codec_grid(n)), dim3(256), args, 0, sh.stream) == hipSuccess ? AMP_OK : AMP_EHIP;
}
static int codec_open(Shell &sh, amp_ctx *ctx) {
    if (!ctx) return AMP_EINVAL;
    sh.ctx = ctx; sh.device = amp::ctx_device(ctx); sh.stream = amp::ctx_stream(ctx);
    DevGuard guard(sh);
    for (int k = 0; k <= sh.n_stages; ++k) CODEC_TRY(hipEventCreate(&sh.ev[k]));
    return AMP_OK;
}
static void codec_close_back_end(Shell &sh) {
    if (sh.scan_tmp) (void)hipFree(sh.scan_tmp);
    for (hipEvent_t e : sh.ev) if (e) (void)hipEventDestroy(e);
}
#else
#define CODEC_FIRST_BAD_KERNEL(name)                                                                                  \
    static void name(const uint8_t *status, unsigned long long *key, int64_t n) { for (int64_t i = 0; i < n; ++i) ampcodec::lane_first_bad(status, key, i); }
#define CODEC_RUN(s, k, fn, n, cx) do { int64_t n__ = (int64_t)(n); if ((cx) >= 0 && (int64_t)(s)->b.ctl[(cx) < 0 ? 0 : (cx)] < n__) n__ = (int64_t)(s)->b.ctl[(cx) < 0 ? 0 : (cx)]; \
                                         for (int64_t i__ = 0; i__ < n__; ++i__) fn((s)->b, i__); } while (0)

struct DevGuard { explicit DevGuard(const Shell &) {} };
static int codec_alloc(uint8_t **p, size_t bytes) { *p = (uint8_t *)malloc(bytes ? bytes : 1); return *p ? AMP_OK : AMP_ENOMEM; }
static void codec_free(void *p) { free(p); }
static int codec_up(Shell &, void *dst, const void *src, size_t n) { if (n) memcpy(dst, src, n); return AMP_OK; }
static int codec_down(Shell &, void *dst, const void *src, size_t n) { if (n) memcpy(dst, src, n); return AMP_OK; }
static int codec_d2d(Shell &, void *dst, const void *src, size_t n) { if (n) memmove(dst, src, n); return AMP_OK; }
static int codec_zero(Shell &, void *p, int v, size_t n) { if (n) memset(p, v, n); return AMP_OK; }
static int codec_sync(Shell &) { return AMP_OK; }
static void codec_mark(Shell &, int) {}
template <class T> static int codec_scan(Shell &, T *p, int64_t n) { T a = 0; for (int64_t i = 0; i < n; ++i) { const T v = p[i]; p[i] = a; a += v; } return AMP_OK; }
static int codec_run_first_bad(Shell &sh, const uint8_t *status, int64_t n) { sh.first_bad(status, sh.bad_key, n); return AMP_OK; }
static int codec_open(Shell &, amp_ctx *) { return AMP_OK; }
static void codec_close_back_end(Shell &) {}
#endif

// ---- what is the same over both ------------------------------------------------------------------------------------------------------
static int codec_wait(Shell &sh) { ++sh.waits; return codec_sync(sh); }

// *p to `need` bytes or more (contents lost).  Pieces of a run have one size: grown once, then reused, never on the steady path.
static int codec_grow(Shell &sh, uint8_t **p, size_t *cap, size_t need) {
    if (need <= *cap) return AMP_OK;
    CODEC_OK(codec_sync(sh));
    uint8_t *np = nullptr;
    const size_t ncap = need + need / 4 + 4096;
    CODEC_OK(codec_alloc(&np, ncap));
    codec_free(*p);
    *p = np; *cap = ncap;
    return AMP_OK;
}

// S = a codec's struct with a Shell `sh`: amp_*_create and amp_*_destroy (the codec frees its own memory first)
template <class S> static int codec_new(amp_ctx *ctx, S **out, int n_stages, FirstBadFn first_bad) {
    if (!out || n_stages > MAX_STAGES) return AMP_EINVAL;
    S *s = new (std::nothrow) S();
    if (!s) return AMP_ENOMEM;
    s->sh.n_stages = n_stages; s->sh.first_bad = first_bad;
    const int rc = codec_open(s->sh, ctx);
    if (rc) { codec_close_back_end(s->sh); delete s; return rc; }
    *out = s;
    return AMP_OK;
}
template <class S> static void codec_delete(S *s) {
    codec_free(s->sh.res);
    codec_close_back_end(s->sh);
    delete s;
}

// the batch as the read pass takes it
static amp_dev_reads codec_reads(const Batch &b, int64_t n_rows, int64_t n_cig, int64_t n_bases_padded) {
    return amp_dev_reads{n_rows, b.pos, b.flag, b.tlen, b.lseq, b.cig_off32, b.cig, b.seq_off8, b.seq, b.qual, n_cig, n_bases_padded};
}

// ReadBatch.from_segments of the batch's rows, for tests and tools: dst's arrays are written (n_rows rows expected), with
// `slack` bytes behind cig, seq and qual
static int codec_batch_to_host(Shell &sh, const Batch &b, int64_t n, int64_t n_cig, int64_t n_bases_padded, const amp_reads *dst, int64_t *src_index, size_t slack) {
    if (dst->n_reads != n) return AMP_EINVAL;
    DevGuard guard(sh);
    uint32_t *co = (uint32_t *)malloc(((size_t)n + 1) * 8);
    if (!co) return AMP_ENOMEM;
    uint32_t *so = co + n + 1;
    int rc = AMP_OK;
    if (dst->pos) rc = rc ? rc : codec_down(sh, (void *)dst->pos, b.pos, (size_t)n * 4);
    if (dst->flag) rc = rc ? rc : codec_down(sh, (void *)dst->flag, b.flag, (size_t)n * 2);
    if (dst->tlen) rc = rc ? rc : codec_down(sh, (void *)dst->tlen, b.tlen, (size_t)n * 4);
    if (dst->lseq) rc = rc ? rc : codec_down(sh, (void *)dst->lseq, b.lseq, (size_t)n * 4);
    if (dst->cig) rc = rc ? rc : codec_down(sh, (void *)dst->cig, b.cig, (size_t)n_cig * 4 + slack);
    if (dst->seq) rc = rc ? rc : codec_down(sh, (void *)dst->seq, b.seq, (size_t)n_bases_padded / 2 + slack);
    if (dst->qual) rc = rc ? rc : codec_down(sh, (void *)dst->qual, b.qual, (size_t)n_bases_padded + slack);
    if (src_index) rc = rc ? rc : codec_down(sh, src_index, b.src_index, (size_t)n * 8);
    rc = rc ? rc : codec_down(sh, co, b.cig_off32, ((size_t)n + 1) * 4);
    rc = rc ? rc : codec_down(sh, so, b.seq_off8, ((size_t)n + 1) * 4);
    rc = rc ? rc : codec_wait(sh);
    for (int64_t i = 0; !rc && i <= n; ++i) {
        if (dst->cig_off) ((uint64_t *)dst->cig_off)[i] = co[i];
        if (dst->seq_off) ((uint64_t *)dst->seq_off)[i] = (uint64_t)so[i] * 8;
    }
    free(co);
    return rc;
}

// room for the results of n rows with n_cig CIGAR words between them (three spare words a row: amp_trim_out)
static int codec_results_room(Shell &sh, int64_t n_rows, int64_t n_cig, Trim &t) {
    const size_t n = (size_t)n_rows, nc = (size_t)n_cig + 3 * n;
    Carver take{nullptr};
    for (int pass = 0; pass < 2; ++pass) {
        t.new_pos = (int32_t *)take(n * 4 + 4); t.new_ncig = (uint32_t *)take(n * 4 + 4); t.ref_len = (int32_t *)take(n * 4 + 4);
        t.new_cig = (uint32_t *)take(nc * 4 + 4); t.trim_flags = take(n + 1); t.status = take(n + 1);
        sh.bad_key = (unsigned long long *)take(8);
        if (pass == 0) { CODEC_OK(codec_grow(sh, &sh.res, &sh.res_cap, take.o)); take = Carver{sh.res}; }
    }
    return AMP_OK;
}

// the first row with a non-zero status (-1: none) and that status: one kernel, eight bytes down, one wait.  The two halves are
// there for a codec whose next stage reads the key where it lies (sh.bad_key) and brings it down with its own wait.
static int codec_first_bad_launch(Shell &sh, const Trim &t, int64_t n_rows) {
    CODEC_OK(codec_zero(sh, sh.bad_key, 0xFF, 8));
    return codec_run_first_bad(sh, t.status, n_rows);
}
static void codec_first_bad_of(unsigned long long key, int64_t *first_bad_row, uint8_t *its_status) {
    const bool any = key != ~0ull;
    if (first_bad_row) *first_bad_row = any ? (int64_t)(key >> 8) : -1;
    if (its_status) *its_status = any ? (uint8_t)(key & 255u) : 0;
}
static int codec_first_bad(Shell &sh, const Trim &t, int64_t n_rows, int64_t *first_bad_row, uint8_t *its_status) {
    CODEC_OK(codec_first_bad_launch(sh, t, n_rows));
    unsigned long long key = ~0ull;
    CODEC_OK(codec_down(sh, &key, sh.bad_key, 8));
    CODEC_OK(codec_wait(sh));
    codec_first_bad_of(key, first_bad_row, its_status);
    return AMP_OK;
}

#ifndef AMP_CODEC_HOSTSIM
// A:896-915 for the rows of the batch: amp_process_batch_device on it where it lies, the results kept in the shell (t points at
// them); the events `stage` and `stage + 1` around the read pass.  defer: the key of the first failing row stays on the device
// (sh.bad_key) and nothing is waited for
static int codec_process(Shell &sh, const Batch &b, Trim &t, int64_t n_rows, int64_t n_cig, int64_t n_bases_padded, uint64_t read_base, int stage,
                         int64_t *first_bad_row, uint8_t *its_status, bool defer = false) {
    DevGuard guard(sh);
    CODEC_OK(codec_results_room(sh, n_rows, n_cig, t));
    codec_mark(sh, stage);
    if (n_rows) {
        const amp_dev_reads rd = codec_reads(b, n_rows, n_cig, n_bases_padded);
        const amp_trim_out o{(int32_t *)t.new_pos, (uint32_t *)t.new_ncig, (uint32_t *)t.new_cig, (int32_t *)t.ref_len, (uint8_t *)t.trim_flags, (uint8_t *)t.status};
        CODEC_OK(amp_process_batch_device(sh.ctx, &rd, read_base, &o));
    }
    codec_mark(sh, stage + 1);
    if (defer) return codec_first_bad_launch(sh, t, n_rows);
    return codec_first_bad(sh, t, n_rows, first_bad_row, its_status);
}

// milliseconds of the stages of the last piece on the ctx stream (HIP events); on != 0 switches the events on
static int codec_stage_ms(Shell &sh, int on, float *ms) {
    DevGuard guard(sh);
    if (ms && sh.timed) {
        CODEC_OK(codec_wait(sh));
        for (int k = 0; k < sh.n_stages; ++k) if (hipEventElapsedTime(&ms[k], sh.ev[k], sh.ev[k + 1]) != hipSuccess) ms[k] = -1.f;
        (void)hipGetLastError();                      // (a stage that did not run: its event was never recorded)
    }
    sh.timed = on != 0;
    return AMP_OK;
}
#endif

}  // namespace ampcodec
#endif  // AMP_CODEC_CTX_ONLY
