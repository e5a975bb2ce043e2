// amp_cooc.hip -- co-occurrence of listed mutations on single reads, tallied on the device (C ABI: the
// amp_cooc_* entry points of amplihip.h).
//
// k_cooc runs behind the read pass of every batch while the hook is on, last of the hooks.  It has the tally skeleton's outer
// shape (amp_tally.hpp: 256-lane blocks over contiguous runs of 256-read tiles, one lane per read, a window in LDS anchored by
// the tile's span) and k_del's inner one: the table is keyed, and the usual case is a pile of thousands of neighbouring reads
// that all give the SAME (set, pattern).  Per read, one lane: the candidate sets are those whose first site lies in
// [pos - max_span, ref_end) (a binary search, then a walk); for each, cooc_read_set (amp_cooc.hpp) scans the CIGAR once and
// loads a nibble and a quality byte per substitution site the read holds; the result is the key set * 65 + cell.  Per wave:
// the lanes walk their candidates in step, and the keys of a step are combined by a ballot loop -- the leader's key is
// broadcast, its holders are balloted, the leader adds the popcount -- into the block's window of CO_W sets x 65 u32 cells
// in LDS, or, for a set outside the window, into the global table.  The window is flushed when it moves and when the block
// ends, one global atomic per non-zero cell.  No step relies on the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "amp_hook.hpp"
#include "amp_cooc.hpp"
#include "amp_tally.hpp"

namespace amp {

struct CoocState : HookState {
    int32_t n_sets = 0, n_sites = 0, max_span = 0;
    std::vector<int32_t> packed;               // the host's copy of d_sets: the tables are laid out again only when it changed
    int32_t *d_sets = nullptr;                 // first[n_sets], off[n_sets + 1], pos[n_sites], len[n_sites], sym[n_sites]
    uint32_t *d_cooc = nullptr;                // [n_sets][65]
    unsigned long long *d_reads = nullptr;     // [2]: tallied, skipped
    CoocSets sets() const {
        const int32_t *p = d_sets;
        CoocSets S;
        S.n_sets = n_sets; S.max_span = max_span;
        S.first = p; S.off = p + n_sets; S.pos = S.off + n_sets + 1; S.len = S.pos + n_sites; S.sym = S.len + n_sites;
        return S;
    }
};

struct CoocArgs {
    TallyReads in;
    CoocSets sets;
    uint32_t *cooc;
    unsigned long long *reads;
};

constexpr int32_t CO_NO_KEY = -1;

// the window to the global table.  (Only cells of sets below n_sets are ever added to.)
__device__ __forceinline__ void cooc_flush(uint32_t *s_cell, int32_t a0, const CoocArgs &a) {
    tally_flush<CO_BLOCK>(s_cell, CO_W * CO_CELLS, [&](int k, uint32_t v) { atomicAdd(&a.cooc[(size_t)a0 * CO_CELLS + (size_t)k], v); });
}

__global__ void __launch_bounds__(CO_BLOCK)
k_cooc(CoocArgs a) {
    __shared__ uint32_t s_cell[CO_W * CO_CELLS];
    __shared__ int32_t s_lo[CO_BLOCK / 64], s_hi[CO_BLOCK / 64];
    const TallyReads &in = a.in;
    const CoocSets &S = a.sets;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int k = tid; k < CO_W * CO_CELLS; k += CO_BLOCK) s_cell[k] = 0u;
    int64_t t0, t1;
    tally_tile_range(in.n, CO_BLOCK, t0, t1);
    CoocWindow win = cooc_window_none();
    int since = 0;                             // tiles since the last flush
    uint32_t n_tallied = 0u, n_skipped = 0u;   // this lane's reads
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- one lane per read: its shape, and the tile's span
        const int64_t i = t * CO_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = ST_NO_READ;
        if (tally_live(in, i)) {
            tally_counted_read(in, i, R, qual0);
            sh = regular_scan(R, in.P, qual0, [](int32_t, uint64_t, uint32_t, bool) {});
            if (sh.regular) ++n_tallied; else ++n_skipped;
        }
        int32_t lo = sh.regular ? R.pos : SPAN_NO_LO, hi = sh.regular ? sh.ref_end : SPAN_NO_HI;
        block_span<CO_BLOCK>(lo, hi, s_lo, s_hi);
        if (!cooc_window_keeps(win, S, lo, hi) || since >= CO_MAX_TILES_PER_FLUSH) {         // (the same for every lane)
            cooc_flush(s_cell, win.a0, a);
            if (lo <= hi) win = cooc_window_at(S, lo);                                        // (every lane searches: the same loads)
            since = 0;
            __syncthreads();
        }
        ++since;
        // ---- the lanes of a wave walk their candidate sets in step; equal keys of a step are combined
        int32_t s = sh.regular ? cooc_first_candidate(S, R.pos) : S.n_sets;
        bool more = sh.regular && cooc_is_candidate(S, s, sh.ref_end);
        while (__ballot(more)) {                                                              // (wave-uniform: whole waves at the ballots)
            int32_t key = CO_NO_KEY;
            if (more) {
                uint32_t cell;
                if (cooc_read_set(R, in.P, qual0, sh.ref_end, in.seq, in.qual, S, s, cell)) key = s * CO_CELLS + (int32_t)cell;
                ++s;
                more = cooc_is_candidate(S, s, sh.ref_end);
            }
            int32_t lk = CO_NO_KEY;             // the leader's key, in every lane
            wave_each_distinct(key != CO_NO_KEY, [&](int src) { lk = __shfl(key, src); return key == lk; }, [&](int src, unsigned long long same) {
                if (lane != src) return;
                const uint32_t cnt = (uint32_t)__popcll(same);
                const int32_t w = cooc_window_cell(win, lk);
                if (w >= 0) atomicAdd(&s_cell[w], cnt);
                else atomicAdd(&a.cooc[lk], cnt);
            });
        }
        __syncthreads();                       // the tile's adds are in the window before a flush; s_lo / s_hi are free again
    }
    cooc_flush(s_cell, win.a0, a);
    tally_wave_add2(a.reads, n_tallied, n_skipped);            // the block's reads
}

static CoocState *cooc_state(amp_ctx *c) { return hook_state<CoocState>(c, HOOK_COOC); }

static int cooc_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    CoocState *s = cooc_state(c);
    return hook_launch(q, s, cooc_hook, rd->n_reads, o, CO_BLOCK, CO_TILES_PER_BLOCK, CO_BLOCKS_PER_CU, [&](unsigned grid) {
        k_cooc<<<grid, CO_BLOCK, 0, q.stream>>>(CoocArgs{tally_reads(q, rd, o), s->sets(), s->d_cooc, s->d_reads});
    });
}

HookOps cooc_hook = {"the co-occurrence tallies need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, cooc_enqueue, hook_free<CoocState>};

}  // namespace amp

using namespace amp;

// The sets as given, checked and packed as d_sets holds them.  -> AMP_OK, or AMP_EINVAL with the message in q.err.
static int cooc_pack(const HookCtx &q, int32_t n_sets, const int32_t *set_off, const int32_t *site_pos, const int32_t *site_len, const uint8_t *site_sym,
                     std::vector<int32_t> &packed, int32_t &n_sites, int32_t &max_span) {
    if (n_sets < 0 || n_sets > CO_MAX_SETS) {
        snprintf(q.err, q.err_cap, "the co-occurrence sets: %d, not in [1, %d]", n_sets, CO_MAX_SETS);
        return AMP_EINVAL;
    }
    if (set_off[0] != 0) {
        snprintf(q.err, q.err_cap, "the co-occurrence sets: set_off[0] is %d, not 0", set_off[0]);
        return AMP_EINVAL;
    }
    max_span = 0;
    for (int32_t s = 0; s < n_sets; ++s) {
        const int64_t o = set_off[s], n = (int64_t)set_off[s + 1] - o;
        if (n < 1 || n > CO_SITES) {
            snprintf(q.err, q.err_cap, "co-occurrence set %d: %lld sites, not in [1, %d]", s, (long long)n, CO_SITES);
            return AMP_EINVAL;
        }
        for (int64_t j = 0; j < n; ++j) {
            const int64_t p = site_pos[o + j], len = site_len[o + j];
            const int64_t end = p + (len > 0 ? len : 1);
            if (p < 0 || len < 0 || end > (int64_t)q.ref_len || (len == 0 && site_sym[o + j] > 3)) {
                snprintf(q.err, q.err_cap, "co-occurrence set %d, site %lld: position %lld, length %lld, base %d: outside the reference of %d bases, or no base of A C G T",
                         s, (long long)j, (long long)p, (long long)len, (int)site_sym[o + j], q.ref_len);
                return AMP_EINVAL;
            }
            if (j > 0) {
                const int64_t pp = site_pos[o + j - 1], pl = site_len[o + j - 1];
                if (p < pp + (pl > 0 ? pl : 1)) {
                    snprintf(q.err, q.err_cap, "co-occurrence set %d: site %lld at %lld is not behind the end of the site before it", s, (long long)j, (long long)p);
                    return AMP_EINVAL;
                }
            }
        }
        const int64_t span = (int64_t)site_pos[o + n - 1] - site_pos[o];
        if (span > CO_MAX_SPAN) {
            snprintf(q.err, q.err_cap, "co-occurrence set %d: its sites span %lld positions, more than %d", s, (long long)span, CO_MAX_SPAN);
            return AMP_EINVAL;
        }
        if (s > 0 && site_pos[o] < site_pos[set_off[s - 1]]) {
            snprintf(q.err, q.err_cap, "co-occurrence set %d: its first site at %d lies in front of the one of the set before it (the sets are sorted by first site)", s, site_pos[o]);
            return AMP_EINVAL;
        }
        if (span > max_span) max_span = (int32_t)span;
    }
    n_sites = set_off[n_sets];
    const size_t N = (size_t)n_sets, T = (size_t)n_sites;
    packed.assign(2 * N + 1 + 3 * T, 0);
    for (size_t s = 0; s < N; ++s) packed[s] = site_pos[set_off[s]];
    for (size_t s = 0; s <= N; ++s) packed[N + s] = set_off[s];
    for (size_t k = 0; k < T; ++k) {
        packed[2 * N + 1 + k] = site_pos[k];
        packed[2 * N + 1 + T + k] = site_len[k];
        packed[2 * N + 1 + 2 * T + k] = site_len[k] == 0 ? (int32_t)site_sym[k] : 0;
    }
    return AMP_OK;
}

extern "C" {

int amp_cooc_enable(amp_ctx *c, int32_t n_sets, const int32_t *set_off, const int32_t *site_pos, const int32_t *site_len, const uint8_t *site_sym) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_COOC);
    if (n_sets == 0 || !set_off) { slot.on = false; return AMP_OK; }
    if (!site_pos || !site_len || !site_sym) {
        snprintf(q.err, q.err_cap, "the co-occurrence sets: an array of the sites is missing");
        return AMP_EINVAL;
    }
    std::vector<int32_t> packed;
    int32_t n_sites = 0, max_span = 0;
    HOOKTRY(cooc_pack(q, n_sets, set_off, site_pos, site_len, site_sym, packed, n_sites, max_span));
    Guard g(q.device);
    CoocState *s = cooc_state(c);
    if (s && s->packed != packed) {
        // other sets: the tables are laid out again (a kernel of the old ones may still be in flight)
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        hook_free<CoocState>(s);
        s = nullptr; slot.state = nullptr; slot.on = false;
    }
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, cooc_hook, s, [&](CoocState &f) -> int {
            f.n_sets = n_sets; f.n_sites = n_sites; f.max_span = max_span;
            f.packed = packed;
            const size_t cells = (size_t)n_sets * CO_CELLS;
            HOOKTRY(hook_alloc(q, f, &f.d_sets, packed.size() * 4));
            HOOKTRY(hook_alloc(q, f, &f.d_cooc, cells * 4, cells * 4));
            HOOKTRY(hook_alloc(q, f, &f.d_reads, 16, 16));
            hook_table(f, f.d_cooc, cells);
            hook_table(f, f.d_reads, 2);
            HOOKCHK(q, hipMemcpyAsync(f.d_sets, f.packed.data(), packed.size() * 4, hipMemcpyHostToDevice, q.stream));
            HOOKCHK(q, hipStreamSynchronize(q.stream));
            return AMP_OK;
        }));
    }
    slot.on = false;
    HOOKTRY(hook_zero(q, *s));
    slot.on = true;
    return AMP_OK;
}

int amp_cooc_get(amp_ctx *c, uint32_t *cooc, uint64_t *reads) { return hook_get(c, HOOK_COOC, {cooc, reads}); }

int amp_cooc_add(amp_ctx *c, const uint32_t *cooc, const uint64_t *reads) { return hook_add_tables(c, HOOK_COOC, {cooc, reads}); }

int amp_cooc_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_COOC, ms); }

}  // extern "C"
