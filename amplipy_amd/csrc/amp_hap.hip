// amp_hap.hip -- read haplotypes per region, tallied on the device (C ABI: the amp_hap_* entry points of
// amplihip.h; semantics: amp_hap.hpp).
//
// k_hap runs behind the read pass of every batch while the hook is on, last of the hooks.  It has k_cooc's shape and k_del's
// table.  One lane per read: a binary search finds the first region at or behind the read's start, and the lanes of a wave walk
// the regions their reads cover in step.  Per region hap_judge (amp_hap.hpp) scans the CIGAR once and compares the read's bases
// inside the region with the packed reference sixteen at a time -- a 64-bit XOR under the mask of the A C G T positions; only a
// non-zero word is opened.  The lane's key is built in its own row of LDS (a row per lane: no lane reads another's).  Per step
// the outcomes of a wave are combined twice by ballot loops: by region -- the leader adds the popcounts of COVER and of the
// outcome columns, one 64-bit atomic per non-zero column, so that a pile of reads that equal the reference costs two or three
// atomics a wave, not one per read -- and by key: the leader's fourteen words are broadcast, their holders balloted, and the
// leader makes ONE insert with count = the lanes and rev = the reverse lanes.  The insert claims a slot of the global table one
// word at a time (hap_probe): no lane ever waits for a store of another lane, every loop is bounded by a constant, and a key
// that finds no slot adds its reads to `lost`.  There is no table in LDS in front of the global one.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "amp_hap.hpp"
#include "amp_hook.hpp"
#include "amp_tally.hpp"

namespace amp {

using HapTable = KeyedTable<uint32_t, HP_KEY_WORDS>;        // the global table (amp_keyed.hpp): HP_EMPTY in a key word: free

struct HapState : HookState {
    HapTable t = {nullptr, nullptr, nullptr, 0u};
    int32_t n_regions = 0;
    int32_t *d_regions = nullptr;               // start[n_regions], end[n_regions]
    uint8_t *d_ref = nullptr;                   // code4[ref_bytes], mask4[ref_bytes]
    size_t ref_bytes = 0;
    unsigned long long *d_tally = nullptr;      // [n_regions][6], then reads[2]
    HapRegions regions() const { return HapRegions{n_regions, d_regions, d_regions + n_regions}; }
    HapRef ref() const { return HapRef{d_ref, d_ref + ref_bytes}; }
    unsigned long long *reads() const { return d_tally + (size_t)n_regions * HP_TALLY_COLS; }
};

struct HapArgs {
    TallyReads in;
    HapRegions regions;
    HapRef ref;
    HapTable t;
    unsigned long long *tally, *reads;
};

// (key, count, rev) into the global table: the slot claimed word by word, then the adds (agent scope: HIP's default)
__device__ __forceinline__ void hap_global_insert(const HapTable &t, const uint32_t *key, uint64_t hash, uint32_t count, uint32_t rev) {
    bool fresh;
    const int64_t s = hap_probe(key, hap_slot_global(hash, t.log2_capacity), (1u << t.log2_capacity) - 1u, hap_probes_global(t.log2_capacity),
                                [&](uint32_t slot, int w, uint32_t v) { return atomicCAS(&t.keys[(size_t)slot * HP_KEY_WORDS + (size_t)w], HP_EMPTY, v); }, fresh);
    keyed_tally(t, s, fresh, count, rev);
}

// What amp_keyed.hpp is told about the table: a key is the first fourteen words of an entry
struct HapKeys {
    using Word = uint32_t;
    using Entry = amp_hap_entry;
    using Table = HapTable;
    static constexpr int WORDS = HP_KEY_WORDS, LOG2_MIN = HP_LOG2_MIN, LOG2_MAX = HP_LOG2_MAX, LOG2_DEFAULT = HP_LOG2_DEFAULT;
    static constexpr const char *NOUN = "the haplotype table";
    int32_t n_regions;                          // (of the state: what check holds an entry's region to)
    static __device__ void insert(const Table &t, const Entry &e) { hap_global_insert(t, &e.head, hap_hash(&e.head), e.count, e.rev); }
    static __device__ void to_entry(const Table &t, uint64_t s, Entry &e) {
        const Word *key = t.keys + (size_t)s * HP_KEY_WORDS;
        e.head = key[0];
#pragma unroll
        for (int w = 1; w < HP_KEY_WORDS; ++w) e.diff[w - 1] = key[w];
        e.count = t.cnt[2 * s]; e.rev = t.cnt[2 * s + 1];
    }
    static __host__ __device__ bool whole(const Word *key) { return key[HP_KEY_WORDS - 1] != HP_EMPTY; }     // (the last word is written last)
    static bool less(const Entry &x, const Entry &y) { return hap_key_less(&x.head, &y.head); }
    bool check(const Entry &e, long long k, char *err, size_t cap) const {
        const uint32_t region = e.head & 0xFFFFu, nd = e.head >> 16;
        if ((int32_t)region < n_regions && nd >= 1u && nd <= (uint32_t)HP_MAX_DIFFS) return true;
        snprintf(err, cap, "haplotype entry %lld: region %u of %d, %u differences", k, region, n_regions, nd);
        return false;
    }
};

__global__ void __launch_bounds__(HP_BLOCK)
k_hap(HapArgs a) {
    __shared__ uint32_t s_key[HP_BLOCK * HP_KEY_STRIDE];
    const TallyReads &in = a.in;
    const HapRegions &G = a.regions;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    uint32_t *key = s_key + tid * HP_KEY_STRIDE;               // this lane's row: no other lane touches it
    int64_t t0, t1;
    tally_tile_range(in.n, HP_BLOCK, t0, t1);
    uint32_t n_covering = 0u, n_other = 0u;                    // this lane's reads
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t i = t * HP_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = ST_NO_READ;
        const bool live = tally_live(in, i);
        if (live) {
            tally_counted_read(in, i, R, qual0);
            sh = regular_scan(R, in.P, qual0, [](int32_t, uint64_t, uint32_t, bool) {});
        }
        // ---- the lanes of a wave walk their candidate regions in step
        int32_t r = sh.regular ? hap_first_candidate(G, R.pos) : G.n;
        bool more = sh.regular && hap_is_candidate(G, r, sh.ref_end);
        bool covered = false;
        while (__ballot(more)) {                                                              // (wave-uniform: whole waves at the ballots)
            int32_t reg = -1;
            int out = HP_OUT_NONE;
            if (more) {
                if (hap_covers(G, r, sh.ref_end)) {
                    reg = r;
                    out = hap_judge<true>(R, in.P, qual0, in.seq, in.qual, a.ref, r, G.start[r], G.end[r], key);
                    covered = true;
                }
                ++r;
                more = hap_is_candidate(G, r, sh.ref_end);
            }
            // ---- the tallies: one leader per distinct region adds the popcounts of the columns
            const unsigned long long m_ref = __ballot(out == HP_OUT_REF), m_rev = __ballot(out == HP_OUT_REF && R.rev != 0u);
            const unsigned long long m_lowq = __ballot(out == HP_OUT_LOWQ), m_over = __ballot(out == HP_OUT_OVERFLOW), m_edge = __ballot(out == HP_OUT_EDGE);
            int32_t lr = -1;                    // the leader's region, in every lane
            wave_each_distinct(reg >= 0, [&](int src) { lr = __shfl(reg, src); return reg == lr; }, [&](int src, unsigned long long same) {
                if (lane != src) return;
                unsigned long long *row = a.tally + (size_t)lr * HP_TALLY_COLS;
                const unsigned long long col[HP_TALLY_COLS] = {same, same & m_ref, same & m_rev, same & m_lowq, same & m_over, same & m_edge};
#pragma unroll
                for (int c = 0; c < HP_TALLY_COLS; ++c)
                    if (col[c]) atomicAdd(&row[c], (unsigned long long)__popcll(col[c]));
            });
            // ---- the keys: equal keys of the wave combined, one insert each
            const bool keyed = out == HP_OUT_KEY;
            const unsigned long long revs = __ballot(keyed && R.rev != 0u);
            const uint64_t h = keyed ? hap_hash(key) : 0ull;
            const auto same_key = [&](int src) {               // the hash and the fourteen words
                bool eq = keyed && h == (uint64_t)__shfl((unsigned long long)h, src);
#pragma unroll
                for (int w = 0; w < HP_KEY_WORDS; ++w) {
                    const uint32_t mine = key[w];
                    eq = eq && mine == __shfl(mine, src);
                }
                return eq;
            };
            wave_each_distinct(keyed, same_key, [&](int src, unsigned long long same) {
                if (lane == src) hap_global_insert(a.t, key, h, (uint32_t)__popcll(same), (uint32_t)__popcll(same & revs));
            });
        }
        if (live) { if (covered) ++n_covering; else ++n_other; }
    }
    tally_wave_add2(a.reads, n_covering, n_other);             // the block's reads
}

static HapState *hap_state(amp_ctx *c) { return hook_state<HapState>(c, HOOK_HAP); }

static int hap_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    HapState *s = hap_state(c);
    return hook_launch(q, s, hap_hook, rd->n_reads, o, HP_BLOCK, HP_TILES_PER_BLOCK, HP_BLOCKS_PER_CU, [&](unsigned grid) {
        k_hap<<<grid, HP_BLOCK, 0, q.stream>>>(HapArgs{tally_reads(q, rd, o), s->regions(), s->ref(), s->t, s->d_tally, s->reads()});
    });
}

HookOps hap_hook = {"the read haplotypes need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, hap_enqueue, hook_free<HapState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_hap_enable(amp_ctx *c, int32_t n_regions, const int32_t *start, const int32_t *end, const uint8_t *ref_ascii, int log2_capacity) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_HAP);
    if (n_regions == 0 || !start || !end) { slot.on = false; return AMP_OK; }
    if (n_regions < 0 || n_regions > HP_MAX_REGIONS) {
        snprintf(q.err, q.err_cap, "the haplotype regions: %d, not in [1, %d]", n_regions, HP_MAX_REGIONS);
        return AMP_EINVAL;
    }
    if (!ref_ascii) {
        snprintf(q.err, q.err_cap, "the haplotype regions need the reference letters");
        return AMP_EINVAL;
    }
    HOOKTRY(keyed_capacity<HapKeys>(q, log2_capacity));
    for (int32_t r = 0; r < n_regions; ++r) {
        const int64_t a = start[r], b = end[r];
        if (a < 0 || b <= a || b - a > HP_MAX_REGION || b > (int64_t)q.ref_len || (r > 0 && start[r] < start[r - 1])) {
            snprintf(q.err, q.err_cap, "haplotype region %d: [%lld, %lld): empty, longer than %d, outside the reference of %d bases, or in front of the region before it "
                     "(the regions are sorted by start)", r, (long long)a, (long long)b, HP_MAX_REGION, q.ref_len);
            return AMP_EINVAL;
        }
    }
    Guard g(q.device);
    HapState *s = hap_state(c);
    if (s) {
        // the tables are laid out again at every enable (a kernel of the old ones may still be in flight)
        slot.on = false;
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        hook_free<HapState>(s);
        s = nullptr; slot.state = nullptr;
    }
    const size_t ref_bytes = ((size_t)q.ref_len + 1) / 2;
    std::vector<uint8_t> packed(2 * ref_bytes, 0);
    hap_pack_ref(ref_ascii, q.ref_len, packed.data(), packed.data() + ref_bytes);
    std::vector<int32_t> regions(2 * (size_t)n_regions);
    for (int32_t r = 0; r < n_regions; ++r) { regions[r] = start[r]; regions[(size_t)n_regions + r] = end[r]; }
    HOOKTRY(hook_new_state(q, slot, hap_hook, s, [&](HapState &f) -> int {
        f.n_regions = n_regions; f.ref_bytes = ref_bytes;
        const size_t tally_words = (size_t)n_regions * HP_TALLY_COLS;
        HOOKTRY(keyed_layout(q, f, f.t, (uint32_t)log2_capacity));
        HOOKTRY(hook_alloc(q, f, &f.d_regions, regions.size() * 4));
        HOOKTRY(hook_alloc(q, f, &f.d_ref, packed.size()));
        HOOKTRY(hook_alloc(q, f, &f.d_tally, (tally_words + 2) * 8, (tally_words + 2) * 8));
        hook_table(f, f.d_tally, tally_words);
        hook_table(f, f.reads(), 2);
        HOOKCHK(q, hipMemcpyAsync(f.d_regions, regions.data(), regions.size() * 4, hipMemcpyHostToDevice, q.stream));
        HOOKCHK(q, hipMemcpyAsync(f.d_ref, packed.data(), packed.size(), hipMemcpyHostToDevice, q.stream));
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        return AMP_OK;
    }));
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_hap_get(amp_ctx *c, amp_hap_entry *entries, int64_t cap, int64_t *n, amp_hap_info *info, uint64_t *tally, uint64_t *reads) {
    if (!c || cap < 0) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HapState *s = hap_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    Guard g(q.device);
    HOOKTRY(hook_tables_get(q, *s, {tally, reads}));           // (keyed_get waits for them)
    return keyed_get<HapKeys>(q, s->t, entries, cap, n, info);
}

int amp_hap_add(amp_ctx *c, const amp_hap_entry *entries, int64_t n, const uint64_t *tally, const uint64_t *reads) {
    if (!c || n < 0 || (n && !entries)) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HapState *s = hap_state(c);
    if (!s || !s->t.keys) return AMP_ESTATE;
    Guard g(q.device);
    HOOKTRY(keyed_add(q, s->t, HapKeys{s->n_regions}, entries, n));
    return hook_tables_add(q, *s, {tally, reads});
}

int amp_hap_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_HAP, ms); }

}  // extern "C"
