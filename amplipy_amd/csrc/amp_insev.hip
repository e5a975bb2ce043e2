// amp_insev.hip -- insertion alleles: strand, quality and read-position evidence, tallied on the device (DESIGN.md section 19b;
// C ABI: the amp_insev_* entry points of amplihip.h; what one event contributes: amp_insev.hpp).
//
// A hook like the others (amp_hook.hpp), in the slot directly behind the deletion events': k_insev runs behind k_del and in
// front of k_cooc, and the two units know nothing of each other (the host report drives both: deletion.py).  k_insev reads the
// entries that THIS batch's read pass appended to the event list.  Which ones: in front of every pass, while the hook is on,
// k_insev_mark copies the eight shards' slot counters into the state's cursor (insev_before_pass, the one before_pass among the hooks); behind the pass the entries between cursor and
// counter are the batch's -- whether the caller drains per batch or never, whether amp_reset came in between, and wherever
// grow_events has moved the regions (the cursor holds indices, and the list is taken from the ctx behind the pass).  The
// number of events is known on the device only, so the grid is fixed (IE_GRID blocks) and every wave strides over the slots, an
// entry per lane.  A slot a long-CIGAR read reserved and did not use (ref_pos < 0) is skipped.  Equal keys of a wave are
// combined by wave_each_distinct -- a pile of reads with one insertion lies on neighbouring slots -- and behind the loop every
// group's leader makes ONE insert into the table in HBM, the leaders of a wave side by side: the slot claimed word by word (insev_probe), then an atomic per non-zero cell.
// There is no table in LDS in front (the list is sparse, and the wave combine already folds a pile).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "amp_hook.hpp"
#include "amp_insev.hpp"
#include "amp_tally.hpp"

namespace amp {

struct InsevTable : KeyedTable<unsigned long long, 2> {     // the keys, (count, rev) and info (amp_keyed.hpp), and a slot's other cells:
    InsevSide *side;                                        // [capacity], an allocation of its own
};

struct InsevState : HookState {
    InsevTable t = {};
    unsigned long long *cursor = nullptr;       // [8]: the shards' slot counts in front of the batch's read pass
    uint64_t read_base = 0;                     // of that pass
    bool marked = false;                        // the cursor is this batch's
};

struct InsevArgs {
    TallyReads in;
    uint64_t read_base;
    const amp_ins_event *ev;
    long long cap;
    const unsigned long long *ev_n, *cursor;
    InsevTable t;
};

__global__ void k_insev_mark(unsigned long long *cursor, const unsigned long long *ev_n) {
    if (threadIdx.x < 8u) cursor[threadIdx.x] = ev_n[threadIdx.x];
}

// One key's cells into the table: the slot claimed word by word, then the adds (agent scope: HIP's default).  `count` events
// are lost when no slot takes the key.
__device__ __forceinline__ void insev_insert(const InsevTable &t, const uint64_t *key, uint32_t count, uint32_t rev, uint32_t noqual, unsigned long long qsum,
                                             const uint32_t *bin) {
    bool fresh;
    const int64_t s = insev_probe(key, keyed_slot(insev_hash(key), t.log2_capacity), (1u << t.log2_capacity) - 1u, keyed_probes(t.log2_capacity),
                                  [&](uint32_t slot, int w, uint64_t v) {
                                      return (uint64_t)atomicCAS(&t.keys[(size_t)slot * 2 + (size_t)w], (unsigned long long)IE_EMPTY, (unsigned long long)v);
                                  }, fresh);
    keyed_tally(t, s, fresh, count, rev);
    if (s < 0) return;
    InsevSide &c = t.side[s];
    if (noqual) atomicAdd(&c.noqual, noqual);
    if (qsum) atomicAdd(&c.qsum, qsum);
#pragma unroll
    for (int b = 0; b < IE_BINS; ++b)
        if (bin[b]) atomicAdd(&c.bin[b], bin[b]);
}

__global__ void __launch_bounds__(IE_BLOCK)
k_insev(InsevArgs a) {
    const TallyReads &in = a.in;
    const int lane = (int)(threadIdx.x & 63u);
    const InsevSpan M = insev_span(a.cap, a.cursor, a.ev_n);       // (the same sixteen words for every lane: scalar loads)
    const int64_t total = M.start[8], stride = (int64_t)gridDim.x * IE_BLOCK;
    for (int64_t j0 = (int64_t)blockIdx.x * IE_BLOCK + (int64_t)(threadIdx.x & ~63u); j0 < total; j0 += stride) {     // (wave-uniform: whole waves at the ballots)
        const int64_t j = j0 + lane;
        bool have = j < total;
        uint64_t key[2] = {0ull, 0ull};
        InsevCells c = {0u, 0u, 0u, 0ull};
        if (have) {
            const amp_ins_event e = a.ev[insev_span_at(M, j)];
            const int64_t i = ins_unused(e) ? -1 : ins_read_row(e.read, a.read_base);
            // the guards: a slot reserved and not used; an entry whose read is not of this batch, or has a status (its trimmed
            // CIGAR is not there to read), or whose interval does not lie inside its read -- none of them is ever tallied
            have = i >= 0 && tally_live(in, i) && e.q_from >= 0 && e.q_from <= e.q_to && e.q_to <= (int32_t)in.lseq[i];
            if (have) {
                StrandRead R;
                uint32_t qual0;
                tally_counted_read(in, i, R, qual0);
                insev_key(in.seq, in.seq_off8, a.read_base, e, key);
                c = insev_cells(e, R.cig, R.n_ops, R.lseq, in.flag[i], in.qual, R.base);
            }
        }
        const unsigned long long revs = __ballot(have && c.rev != 0u), noqs = __ballot(have && c.noqual != 0u);
        unsigned long long bins[IE_BINS];
#pragma unroll
        for (int b = 0; b < IE_BINS; ++b) bins[b] = __ballot(have && c.bin == (uint32_t)b);
        uint64_t lk[2] = {0ull, 0ull};          // the leader's key, in every lane
        const auto same_key = [&](int src) {
            lk[0] = (uint64_t)__shfl((unsigned long long)key[0], src);
            lk[1] = (uint64_t)__shfl((unsigned long long)key[1], src);
            return have && key[0] == lk[0] && key[1] == lk[1];
        };
        // the groups' sums are worked out in the loop, wave-uniformly, and land in their leaders' registers; the inserts wait until
        // it is over, so that the leaders' claims and adds are in flight together -- a lane at a time inside the loop, every
        // distinct key of the wave would wait for the compare-and-swaps of the one before it
        bool leader = false;
        uint32_t g_count = 0u, g_rev = 0u, g_noqual = 0u, g_bin[IE_BINS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        unsigned long long g_qsum = 0ull;
        wave_each_distinct(have, same_key, [&](int src, unsigned long long same) {
            unsigned long long q = ((same >> lane) & 1ull) ? (unsigned long long)c.qsum : 0ull;      // the group's quality sum, in every lane
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d);
            if (lane != src) return;
            leader = true;
            g_count = (uint32_t)__popcll(same); g_rev = (uint32_t)__popcll(same & revs); g_noqual = (uint32_t)__popcll(same & noqs); g_qsum = q;
#pragma unroll
            for (int b = 0; b < IE_BINS; ++b) g_bin[b] = (uint32_t)__popcll(same & bins[b]);
        });
        if (leader) insev_insert(a.t, key, g_count, g_rev, g_noqual, g_qsum, g_bin);       // (a leader's own key is its group's)
    }
}

// What amp_keyed.hpp is told about the table: an entry carries the side array's cells next to (count, rev)
struct InsevKeys {
    using Word = unsigned long long;
    using Entry = amp_insev_entry;
    using Table = InsevTable;
    static constexpr int WORDS = 2, LOG2_MIN = IE_LOG2_MIN, LOG2_MAX = IE_LOG2_MAX, LOG2_DEFAULT = IE_LOG2_DEFAULT;
    static constexpr const char *NOUN = "the insertion evidence table";
    static __device__ void insert(const Table &t, const Entry &e) {
        const uint64_t key[2] = {((uint64_t)(uint32_t)e.ref_pos << 32) | (uint64_t)(uint32_t)e.len, e.hash};
        insev_insert(t, key, e.count, e.rev, e.noqual, (unsigned long long)e.qsum, e.bin);
    }
    static __device__ void to_entry(const Table &t, uint64_t s, Entry &e) {       // (field by field: the zeroed entry's padding stays zero)
        const Word *key = t.keys + (size_t)s * 2;
        e.ref_pos = (int32_t)(uint32_t)(key[0] >> 32); e.len = (int32_t)(uint32_t)key[0]; e.hash = key[1];
        e.count = t.cnt[2 * s]; e.rev = t.cnt[2 * s + 1]; e.noqual = t.side[s].noqual; e.qsum = t.side[s].qsum;
        for (int b = 0; b < IE_BINS; ++b) e.bin[b] = t.side[s].bin[b];
    }
    static __host__ __device__ bool whole(const Word *key) { return key[1] != IE_EMPTY; }       // (the last word is written last)
    static bool less(const Entry &x, const Entry &y) { return x.ref_pos != y.ref_pos ? x.ref_pos < y.ref_pos : x.len != y.len ? x.len < y.len : x.hash < y.hash; }
    static bool check(const Entry &e, long long k, char *err, size_t cap) {
        if (e.ref_pos >= 0 && e.len >= 0 && !(e.hash >> 63)) return true;
        snprintf(err, cap, "insertion evidence entry %lld: position %d, length %d, hash %llx", k, e.ref_pos, e.len, (unsigned long long)e.hash);
        return false;
    }
};

static InsevState *insev_state(amp_ctx *c) { return hook_state<InsevState>(c, HOOK_INSEV); }

static int insev_layout(const HookCtx &q, InsevState &f, uint32_t log2_capacity) {
    const size_t cap = (size_t)1 << log2_capacity;
    f.t.side = nullptr; f.cursor = nullptr;
    HOOKTRY(keyed_layout(q, f, f.t, log2_capacity));
    HOOKTRY(hook_alloc(q, f, &f.t.side, cap * sizeof(InsevSide), cap * sizeof(InsevSide)));
    return hook_alloc(q, f, &f.cursor, 64, 64);
}

// In FRONT of the read pass, while the hook is on: the event list's slot counts as they stand become the cursor -- what the
// pass appends behind them is this batch's
static int insev_before_pass(amp_ctx *c, uint64_t read_base) {
    const HookCtx q = ctx_hook(c);
    InsevState *s = insev_state(c);
    if (!s) return AMP_ESTATE;
    k_insev_mark<<<1, 64, 0, q.stream>>>(s->cursor, q.ev_n);
    HOOKCHK(q, hipGetLastError());
    s->read_base = read_base;
    s->marked = true;
    return AMP_OK;
}

static int insev_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);              // (behind the pass: the list where grow_events has left it)
    InsevState *s = insev_state(c);
    const bool marked = s->marked;
    s->marked = s->timer.timed = false;
    if (rd->n_reads > 0 && !marked) { snprintf(q.err, q.err_cap, "the insertion evidence: no mark in front of this read pass"); return AMP_ESTATE; }
    // (the grid is fixed, whatever the batch: the number of events is known on the device only)
    return hook_launch(q, s, insev_hook, rd->n_reads, o, IE_BLOCK, 1, 1, [&](unsigned) {
        if (q.events && q.ev_cap > 0)
            k_insev<<<IE_GRID, IE_BLOCK, 0, q.stream>>>(InsevArgs{tally_reads(q, rd, o), s->read_base, q.events, q.ev_cap, q.ev_n, s->cursor, s->t});
    });
}

HookOps insev_hook = {"the insertion evidence needs", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, insev_enqueue, hook_free<InsevState>, insev_before_pass};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_insev_enable(amp_ctx *c, int on, int log2_capacity) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_INSEV);
    if (!on) { slot.on = false; return AMP_OK; }
    HOOKTRY(keyed_capacity<InsevKeys>(q, log2_capacity));
    Guard g(q.device);
    InsevState *s = insev_state(c);
    const auto layout = [&](InsevState &f) -> int { return insev_layout(q, f, (uint32_t)log2_capacity); };
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, insev_hook, s, layout));
    } else if (s->t.log2_capacity != (uint32_t)log2_capacity) {
        HOOKTRY(keyed_relayout(q, slot, *s, layout));
    }
    HOOKTRY(hook_zero(q, *s));
    s->marked = false;
    slot.on = true;
    return AMP_OK;
}

int amp_insev_get(amp_ctx *c, amp_insev_entry *entries, int64_t cap, int64_t *n, amp_insev_info *info) {
    if (!c || cap < 0) return AMP_EINVAL;
    InsevState *s = insev_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    return keyed_get<InsevKeys>(ctx_hook(c), s->t, entries, cap, n, info);
}

int amp_insev_add(amp_ctx *c, const amp_insev_entry *entries, int64_t n) {
    if (!c || n < 0 || (n && !entries)) return AMP_EINVAL;
    InsevState *s = insev_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    return keyed_add(ctx_hook(c), s->t, InsevKeys{}, entries, n);
}

int amp_insev_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_INSEV, ms); }

}  // extern "C"
