// amp_hook.hpp -- the host shell of the opt-in kernels that run behind every batch's read pass: the QC
// report (amp_qc.hip), the strand tallies (amp_strand.hip), the per-amplicon counts (amp_amplicon.hip), the codon tallies
// (amp_codon.hip), the deletion events (amp_del.hip), the insertion evidence (amp_insev.hip), the co-occurrence tallies (amp_cooc.hip), the error profile (amp_errprof.hip), the read haplotypes (amp_hap.hip), the read-position tallies (amp_readpos.hip).  What a hook needs to know of a ctx, and what the hooks have in common -- the check macro, the device
// guard, the timer round a launch, the grid rule, the merge of host tables, the check of a trimming pass's results, the common
// part of a state and its construction, the record of what a state owns on the device with free, reset, get and add written
// from it, the frame of an enqueue, last_ms -- each once.  (What the three tally kernels share
// on the device is amp_tally.hpp.)  amp_ctx (amp_ctx.hpp) keeps one slot (switch, state) per hook and amplihip.hip walks the
// table of HookOps; a unit keeps its state, its kernels and what it enables, and no unit knows of another: nothing of one
// unit's is declared here but its HookOps.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <initializer_list>
#include <new>
#include <vector>

#include "../../include/amplihip.h"

// `call` failed: the message (with `text`, the call as written) to err and the call's code out of the enclosing function
#define AMP_HIPCHK(err, cap, text, call)                                                                                     \
    do {                                                                                                                     \
        hipError_t e__ = (call);                                                                                             \
        if (e__ != hipSuccess) {                                                                                             \
            snprintf((err), (cap), "%s failed: %s (%s:%d)", text, hipGetErrorString(e__), __FILE__, __LINE__);               \
            return e__ == hipErrorOutOfMemory ? AMP_ENOMEM : AMP_EHIP;                                                       \
        }                                                                                                                    \
    } while (0)
#define HOOKCHK(q, call) AMP_HIPCHK((q).err, (q).err_cap, #call, call)       // q: a HookCtx
// a step that gives an AMP_* code: anything but AMP_OK out of the enclosing function
#define HOOKTRY(call) do { const int rc__ = (call); if (rc__ != AMP_OK) return rc__; } while (0)

namespace amp {

struct Guard {      // the device is current for the duration of a call
    int prev = -1;
    bool ok = true;
    explicit Guard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    }
    ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// What a hook needs to know of a ctx (the struct is amp_ctx.hpp's; amplihip.hip fills this in).
struct HookCtx {
    int device;
    int32_t ref_len;
    hipStream_t stream;
    const uint32_t *counts;     // the device table as it stands
    int do_trim, have_primers, min_quality, n_cu;
    char *err; size_t err_cap;
    // the insertion-event list as the read pass leaves it (amp_insev.hip): EV_SHARDS regions of ev_cap entries, and the shards'
    // slot counters on the device.  Valid until the next read pass, which may lay the regions out again.
    const amp_ins_event *events; long long ev_cap; const unsigned long long *ev_n;
};
HookCtx ctx_hook(amp_ctx *c);

// The hooks; the numeric order is the order their kernels run in behind the read pass.
enum { HOOK_QC, HOOK_STRAND, HOOK_AMPLICON, HOOK_CODON, HOOK_DEL, HOOK_INSEV, HOOK_COOC, HOOK_ERRPROF, HOOK_HAP, HOOK_READPOS, N_HOOKS };
struct HookSlot {
    bool on;                    // the switch amplihip.hip reads per batch
    void *state;                // the hook's device state, owned by its unit; it outlives the switch (tables stay readable)
};
HookSlot &hook_slot(amp_ctx *c, int which);

// The results of a trimming pass (the fields of amp_trim_out, in its order) a hook's kernel reads.
enum : uint32_t { OUT_NEW_POS = 1u, OUT_NEW_NCIG = 2u, OUT_NEW_CIG = 4u, OUT_REF_LEN = 8u, OUT_TRIM_FLAGS = 16u, OUT_STATUS = 32u };

struct HookOps {
    const char *name;           // as a refusal begins: "the QC report needs"
    uint32_t needs;             // OUT_* bits
    int (*enqueue)(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *dev_out);       // the kernel on the ctx stream; the state exists
    void (*free_state)(void *state);        // hook_free of the unit's state; a null state is nothing to do
    // Optional (null in most units): in FRONT of a batch's read pass, on the ctx stream, while the hook is on -- what the unit has
    // to note of the ctx's device state before the pass changes it.  read_base is the pass's own.
    int (*before_pass)(amp_ctx *c, uint64_t read_base);
};
// One per unit; amplihip.hip keeps them in enum order.  (Not const objects, though nothing writes them: hipcc emits a const
// object with a constant initialiser into the device image as well, host function pointers and all.)
extern HookOps qc_hook, strand_hook, amplicon_hook, codon_hook, del_hook, insev_hook, cooc_hook, errprof_hook, hap_hook, readpos_hook;

// With trimming on, every result in `needs` must be there; otherwise the refusal is in q.err.  amplihip.hip asks in front of a
// device batch's read pass, so that a refused call changes nothing; an enqueue asks again.
inline int hook_check_out(const HookCtx &q, const amp_trim_out *o, const HookOps &ops) {
    if (!q.do_trim) return AMP_OK;
    static const char *const field[] = {"new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status"};
    const void *have[] = {o ? o->new_pos : nullptr, o ? o->new_ncig : nullptr, o ? o->new_cig : nullptr,
                          o ? o->ref_len : nullptr, o ? o->trim_flags : nullptr, o ? o->status : nullptr};
    bool all = true;
    char list[80];
    int at = 0;
    for (int k = 0; k < 6; ++k) {
        if (!((ops.needs >> k) & 1u)) continue;
        all = all && have[k];
        const uint32_t later = ops.needs >> (k + 1);
        at += snprintf(list + at, sizeof(list) - (size_t)at, "%s%s", field[k], !later ? "" : (later & (later - 1u)) ? ", " : " and ");
    }
    if (all) return AMP_OK;
    snprintf(q.err, q.err_cap, "%s %s of a trimming pass", ops.name, list);
    return AMP_EINVAL;
}

struct HookTimer {              // the time of a hook's last kernel: an event on either side of the launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;         // cleared at the start of every enqueue: a batch without reads leaves nothing to ask for
    hipError_t create() {
        const hipError_t e = hipEventCreate(&ev0);
        return e != hipSuccess ? e : hipEventCreate(&ev1);
    }
    void destroy() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
    hipError_t begin(hipStream_t s) { return hipEventRecord(ev0, s); }
    hipError_t end(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev1, s);
        timed = e == hipSuccess;
        return e;
    }
    int last_ms(const HookCtx &q, float *ms) {      // waits for the kernel; AMP_ESTATE when the last batch launched none
        if (!timed) return AMP_ESTATE;
        Guard g(q.device);
        HOOKCHK(q, hipEventSynchronize(ev1));
        float t = 0;
        HOOKCHK(q, hipEventElapsedTime(&t, ev0, ev1));
        if (ms) *ms = t;
        return AMP_OK;
    }
};

// The grid of a hook's kernel over n reads: a block takes tiles_per_block tiles of `block` reads and more (what a block pays
// once -- an LDS histogram, a window's flush -- is paid for several tiles), up to blocks_per_cu blocks per CU; from there on
// the blocks take more tiles each.
inline unsigned hook_grid(int64_t n, int block, int tiles_per_block, int blocks_per_cu, int n_cu) {
    const int64_t tiles = (n + block - 1) / block;
    return (unsigned)std::min<int64_t>(std::max<int64_t>((tiles + tiles_per_block - 1) / tiles_per_block, 1), (int64_t)blocks_per_cu * n_cu);
}

// dev[k] += host[k]: the table to the host, the sums there, and back.  A call per job (the merge of partial tables), not per
// batch.  A null host table is left out.
template <class T>
int hook_add(const HookCtx &q, T *dev, const T *host, size_t count) {
    if (!host || !count) return AMP_OK;
    std::vector<T> h(count);
    HOOKCHK(q, hipMemcpyAsync(h.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    for (size_t k = 0; k < count; ++k) h[k] += host[k];
    HOOKCHK(q, hipMemcpyAsync(dev, h.data(), count * sizeof(T), hipMemcpyHostToDevice, q.stream));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}

// What every hook's state begins with; a slot's `state` points at this part.  Next to the timer it records what the state
// owns on the device: its allocations (hook_alloc), each with what a reset does to it -- the first `ones` bytes to 0xFF (the
// free keys of a keyed table, amp_keyed.hpp), the `zeros` bytes behind them to 0 -- and its result tables in the order of the
// ABI's get / add arguments (hook_table).  A table may be a sub-range of an allocation.
struct HookState {
    struct Owned { void *p; size_t ones, zeros; };
    struct Table { void *p; size_t count, elem; };       // elem: 4 or 8 bytes
    HookTimer timer;
    Owned owned[8] = {};
    Table table[4] = {};
    int n_owned = 0, n_table = 0;
};
template <class S> S *hook_state_of(void *state) { return static_cast<S *>(static_cast<HookState *>(state)); }
template <class S> S *hook_state(amp_ctx *c, int which) { return hook_state_of<S>(hook_slot(c, which).state); }

// `bytes` of device memory that the state owns from here on, into *ptr
template <class P>
int hook_alloc(const HookCtx &q, HookState &s, P **ptr, size_t bytes, size_t zeros = 0, size_t ones = 0) {
    if (s.n_owned == (int)(sizeof(s.owned) / sizeof(s.owned[0]))) return AMP_ESTATE;
    void *p = nullptr;
    HOOKCHK(q, hipMalloc(&p, bytes));
    s.owned[s.n_owned++] = HookState::Owned{p, ones, zeros};
    *ptr = (P *)p;
    return AMP_OK;
}
// The next result table: `count` elements at p
template <class T>
void hook_table(HookState &s, T *p, size_t count) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "hook_add adds u32 or u64");
    s.table[s.n_table++] = HookState::Table{p, count, sizeof(T)};
}
// What the state owns goes back; the record is empty afterwards.  (No kernel on it may be in flight.)
inline void hook_release(HookState &s) {
    for (int k = 0; k < s.n_owned; ++k) (void)hipFree(s.owned[k].p);
    s.n_owned = s.n_table = 0;
}
// HookOps::free_state of a unit whose state is S (its host-only members go with the delete)
template <class S>
void hook_free(void *state) {
    S *s = hook_state_of<S>(state);
    if (!s) return;
    hook_release(*s);
    s->timer.destroy();
    delete s;
}
// The tables start over (amp_reset, and the end of every enable): a memset per allocation that has something to clear, two
// for a keyed table
inline int hook_zero(const HookCtx &q, const HookState &s) {
    for (int k = 0; k < s.n_owned; ++k) {
        const HookState::Owned &o = s.owned[k];
        if (o.ones) HOOKCHK(q, hipMemsetAsync(o.p, 0xFF, o.ones, q.stream));
        if (o.zeros) HOOKCHK(q, hipMemsetAsync((char *)o.p + o.ones, 0, o.zeros, q.stream));
    }
    return AMP_OK;
}

// The state's tables to the host arrays given in the record's order, a null one left out; enqueued, not waited for
inline int hook_tables_get(const HookCtx &q, const HookState &s, std::initializer_list<void *> host) {
    int k = 0;
    for (void *h : host) {
        const HookState::Table &t = s.table[k++];
        if (h && t.count) HOOKCHK(q, hipMemcpyAsync(h, t.p, t.count * t.elem, hipMemcpyDeviceToHost, q.stream));
    }
    return AMP_OK;
}
// ... and the host arrays added onto them (hook_add)
inline int hook_tables_add(const HookCtx &q, const HookState &s, std::initializer_list<const void *> host) {
    int k = 0;
    for (const void *h : host) {
        const HookState::Table &t = s.table[k++];
        HOOKTRY(t.elem == 4 ? hook_add(q, (uint32_t *)t.p, (const uint32_t *)h, t.count) : hook_add(q, (uint64_t *)t.p, (const uint64_t *)h, t.count));
    }
    return AMP_OK;
}
// amp_*_get and amp_*_add of a hook whose results are its tables: AMP_ESTATE before the first enable
inline int hook_get(amp_ctx *c, int which, std::initializer_list<void *> host) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    const HookState *s = (const HookState *)hook_slot(c, which).state;
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    HOOKTRY(hook_tables_get(q, *s, host));
    HOOKCHK(q, hipStreamSynchronize(q.stream));
    return AMP_OK;
}
inline int hook_add_tables(amp_ctx *c, int which, std::initializer_list<const void *> host) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    const HookState *s = (const HookState *)hook_slot(c, which).state;
    if (!s) return AMP_ESTATE;
    Guard g(q.device);
    return hook_tables_add(q, *s, host);
}

// A new state for the slot: fill(*s) allocates what the unit keeps (AMP_OK, or the code of what failed), then the timer;
// the state is handed to the slot, or freed again when a step failed (s is null then).
template <class S, class Fill>
int hook_new_state(const HookCtx &q, HookSlot &slot, const HookOps &ops, S *&s, Fill fill) {
    S *fresh = new (std::nothrow) S();
    s = nullptr;
    if (!fresh) return AMP_ENOMEM;
    int rc = fill(*fresh);
    if (rc == AMP_OK) rc = [&]() -> int { HOOKCHK(q, fresh->timer.create()); return AMP_OK; }();
    if (rc != AMP_OK) { ops.free_state(static_cast<HookState *>(fresh)); return rc; }
    slot.state = static_cast<HookState *>(s = fresh);
    return AMP_OK;
}

// The frame of an enqueue: a batch without reads times nothing; a missing result of the trimming pass is refused; else
// launch(grid) -- the unit's <<<>>> on q.stream -- between the timer's two events.
template <class Launch>
int hook_launch(const HookCtx &q, HookState *s, const HookOps &ops, int64_t n, const amp_trim_out *o, int block, int tiles_per_block, int blocks_per_cu,
                Launch launch) {
    s->timer.timed = false;
    if (n <= 0) return AMP_OK;
    const int rc = hook_check_out(q, o, ops);
    if (rc != AMP_OK) return rc;
    HOOKCHK(q, s->timer.begin(q.stream));
    launch(hook_grid(n, block, tiles_per_block, blocks_per_cu, q.n_cu));
    HOOKCHK(q, hipGetLastError());
    HOOKCHK(q, s->timer.end(q.stream));
    return AMP_OK;
}

// amp_*_last_ms: the time of the hook's last kernel
inline int hook_last_ms(amp_ctx *c, int which, float *ms) {
    if (!c) return AMP_EINVAL;
    HookState *s = (HookState *)hook_slot(c, which).state;
    return s ? s->timer.last_ms(ctx_hook(c), ms) : AMP_ESTATE;
}

}  // namespace amp
#endif
