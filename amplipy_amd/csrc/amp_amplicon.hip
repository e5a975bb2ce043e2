// amp_amplicon.hip -- per-amplicon allele counts on the device (C ABI: the amp_amplicon_* entry points
// of amplihip.h).
//
// k_amplicon runs behind the read pass of every batch while the hook is on and touches every counted base once more, in the
// shape of amp_tally.hpp; what follows is its own part.  Phase A: the read's amplicon from its ORIGINAL coordinates
// (amplicon_assign, amp_amplicon.hpp), the reads per amplicon (a ballot and run heads per wave: a pile costs one add per wave
// and amplicon), and the counted alignment as a few segments.
// The block keeps AM_SLOTS windows of AM_W positions x 6 columns in LDS (row stride 7), each bound to (amplicon, anchor); the
// distinct amplicons of a tile are found wave by wave (a loop over the wave's distinct values), and one lane settles all of
// the tile's requests against the slots (amplicon_resolve).  Slots persist across the block's tiles; a slot goes to the table
// -- its non-zero cells, one atomic each -- when it is given to another amplicon, when its anchor moves, and at block end.
// Phase B, position-major: per slot in use, each wave owns every fourth 64-position chunk of the window and each lane one
// position of it; the wave visits the segments that lie in its slot and overlap its chunk.  Reads the window did not take --
// more segments than list slots, an irregular CIGAR, an amplicon without a slot in this tile, a read outside its slot's
// window -- walk serially (amplicon_walk), with LDS atomics where slot and position are resident and global atomics
// otherwise: slow and correct.  No step relies on the reads being sorted.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "amp_hook.hpp"
#include "amp_amplicon.hpp"
#include "amp_tally.hpp"

namespace amp {

struct AmpliconState : HookState {
    int32_t n_amp = 0;
    int64_t cells = 0;                         // positions of all spans together
    int32_t *d_lo = nullptr, *d_hi = nullptr;  // one allocation: lo, hi, cell_off
    uint32_t *d_off = nullptr;
    int32_t *d_start = nullptr, *d_end = nullptr;      // one allocation: amp_start, amp_end
    uint32_t *d_counts = nullptr;              // [cells][6]
    unsigned long long *d_reads = nullptr;     // [n_amp + 1]
};

struct AmpliconArgs {
    TallyReads in;
    AmpliconTables T;
    uint32_t *counts;
    unsigned long long *reads;
};

// the slots in `mask` to the table
__device__ __forceinline__ void amplicon_flush(uint32_t *s_cell, const AmSlots &S, uint32_t mask, const AmpliconArgs &a) {
    for (int k = 0; k < AM_SLOTS; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int32_t amp = S.amp[k], anchor = S.anchor[k];
        if (amp < 0 || amp >= a.T.n_amp) continue;                 // (a free slot holds nothing)
        const int32_t lo = a.T.lo[amp], hi = a.T.hi[amp];
        const size_t row0 = (size_t)a.T.cell_off[amp];
        tally_flush<AM_BLOCK>(s_cell + k * AM_SLOT_WORDS, AM_SLOT_WORDS, [&](int i, uint32_t v) {
            const int64_t r = (int64_t)anchor + i / AM_STRIDE;
            const int c = i % AM_STRIDE;
            if (c >= AM_COLS || r < lo || r >= hi) return;         // (nothing is ever added there)
            atomicAdd(&a.counts[(row0 + (size_t)(r - lo)) * AM_COLS + c], v);
        });
    }
}

__global__ void __launch_bounds__(AM_BLOCK)
k_amplicon(AmpliconArgs a) {
    __shared__ uint32_t s_cell[AM_SLOTS * AM_SLOT_WORDS];
    __shared__ AmSeg s_seg[AM_BLOCK * AM_SEG_SLOTS];
    __shared__ AmReq s_req[AM_REQS];
    __shared__ int s_nreq[AM_BLOCK / 64];
    __shared__ AmSlots s_slots;
    __shared__ uint32_t s_nseg;
    const TallyReads &in = a.in;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < AM_SLOTS * AM_SLOT_WORDS; k += AM_BLOCK) s_cell[k] = 0u;
    if (tid == 0) { s_nseg = 0u; amplicon_slots_init(s_slots); }
    int64_t t0, t1;
    tally_tile_range(in.n, AM_BLOCK, t0, t1);
    int since = 0;                             // tiles since every slot was last flushed
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        // ---- phase A: one lane per read
        const int64_t i = t * AM_BLOCK + tid;
        StrandRead R;
        uint32_t qual0;
        tally_no_read(in, R, qual0);
        StrandShape sh = ST_NO_READ;
        const bool live = tally_live(in, i);
        int32_t amp = -1, lo_a = 0, hi_a = 0;
        size_t row0 = 0;
        if (live) {
            const uint32_t c0 = in.cig_off32[i];
            const int32_t p = in.pos[i];
            amp = amplicon_assign(p, (int64_t)p + am_cigar_ref_len(in.cig + c0, in.cig_off32[i + 1] - c0), a.T);
            if (amp >= 0) {
                lo_a = a.T.lo[amp]; hi_a = a.T.hi[amp]; row0 = (size_t)a.T.cell_off[amp];
                tally_counted_read(in, i, R, qual0);
                sh = amplicon_segments(R, in.P, qual0, 0, [](const AmSeg &) {});
            }
        }
        // reads per amplicon: neighbouring lanes with the same amplicon are one run, and its first lane adds the run's length
        {
            const int32_t key = live ? (amp >= 0 ? amp : a.T.n_amp) : -1;
            const int32_t before = __shfl_up(key, 1);
            const unsigned long long heads = __ballot(lane == 0 || key != before);
            if (key >= 0 && ((heads >> lane) & 1ull)) {
                const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
                const int len = later ? __ffsll((long long)later) : 64 - lane;
                atomicAdd(&a.reads[key], (unsigned long long)len);
            }
        }
        // the wave's distinct amplicons that want a window, one request each: (amplicon, first position, last end)
        const bool want = live && amplicon_wants_slot(amp, sh, R.pos, lo_a, hi_a);
        {
            int nreq = 0;                                          // (wave-uniform; the requests past AM_REQ_PER_WAVE are counted, not kept)
            int32_t v = -1;                                        // the leader's amplicon, in every lane
            const auto same_amp = [&](int src) {
                v = __shfl(amp, src);
                return want && amp == v;
            };
            wave_each_distinct(want, same_amp, [&](int src, unsigned long long same) {
                const bool mine = ((same >> lane) & 1ull) != 0ull;
                int32_t l = mine ? R.pos : SPAN_NO_LO, h = mine ? sh.ref_end : SPAN_NO_HI;
                wave_span(l, h);                                   // (every lane)
                if (lane == src && nreq < AM_REQ_PER_WAVE) s_req[wave * AM_REQ_PER_WAVE + nreq] = AmReq{v, l, h, lo_a};
                ++nreq;
            });
            if (lane == 0) s_nreq[wave] = min(nreq, AM_REQ_PER_WAVE);
        }
        __syncthreads();
        if (tid == 0) {                                            // one lane settles the tile's requests against the slots
            int n = 0;
            for (int w = 0; w < AM_BLOCK / 64; ++w)
                for (int k = 0; k < s_nreq[w]; ++k) s_req[n++] = s_req[w * AM_REQ_PER_WAVE + k];       // (n <= the index read)
            amplicon_resolve(s_slots, s_req, n);
        }
        __syncthreads();
        {
            uint32_t flush = s_slots.flush;                        // (the same for every lane)
            if (since >= AM_MAX_TILES_PER_FLUSH) { flush = (1u << AM_SLOTS) - 1u; since = 0; }
            if (flush) amplicon_flush(s_cell, s_slots, flush, a);
        }
        ++since;
        __syncthreads();
        if (tid == 0) amplicon_commit(s_slots);
        __syncthreads();
        const uint32_t used = s_slots.used;
        const int slot = live ? amplicon_read_slot(s_slots, amp, sh, R.pos, lo_a, hi_a) : -1;
        const bool win = slot >= 0;
        const bool nothing = live && amp >= 0 && sh.regular && sh.n_seg == 0;      // a regular read whose segments are all empty adds nothing
        if (win) {
            uint32_t at = atomicAdd(&s_nseg, (uint32_t)sh.n_seg);  // (at most AM_SEG_SLOTS per read: the list cannot overflow)
            amplicon_segments(R, in.P, qual0, slot, [&](const AmSeg &s) { s_seg[at++] = s; });
        }
        __syncthreads();
        // ---- phase B: position-major over the tile's segments; in slot k, lane `lane` of the wave owns window position
        // c * 64 + lane of chunk c; the wave visits the segments that lie in slot k and overlap the chunk.
        const uint32_t ns = s_nseg;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {                // (ns and used are block-uniform: whole waves at the ballots)
            bool have;
            const AmSeg mine = seg_take(s_seg, s0, ns, lane, have);
            const int my_slot = am_seg_slot(mine);
            for (int k = 0; k < AM_SLOTS; ++k) {
                if (!((used >> k) & 1u)) continue;
                const int32_t anchor = s_slots.anchor[k];
                const int32_t m0 = mine.r0 - anchor, m1 = m0 + am_seg_len(mine);
                for (int c = wave; c < AM_W / AM_CHUNK; c += AM_BLOCK / 64) {
                    const int32_t c0 = c * AM_CHUNK;
                    unsigned long long hits = __ballot(have && my_slot == k && m1 > c0 && m0 < c0 + AM_CHUNK);
                    const int32_t p = c0 + lane;
                    while (hits) {
                        const int src = __ffsll((long long)hits) - 1;
                        hits &= hits - 1ull;
                        const AmSeg g = seg_from(mine, src);
                        const int32_t a0 = g.r0 - anchor, a1 = a0 + am_seg_len(g);
                        if (p < a0 || p >= a1) {
                            // (not this lane's position; every lane is back for the next segment's shuffles)
                        } else if (am_seg_del(g)) {
                            s_cell[am_cell(k, p, 5u)] += 1u;
                        } else {
                            uint32_t col, qv;
                            if (strand_base(in.seq, in.qual, g.q0 + (uint64_t)(p - a0), in.P.min_quality, col, qv)) s_cell[am_cell(k, p, col)] += 1u;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_nseg = 0u;
        // ---- the serial path: assigned reads the window did not take
        if (live && amp >= 0 && !win && !nothing) {
            const int k = amplicon_slot_of(s_slots, amp);
            const int32_t anchor = k >= 0 ? s_slots.anchor[k] : 0;
            amplicon_walk(R, in.P, in.seq, in.qual, lo_a, hi_a, [&](int32_t r, uint32_t col) {
                const int64_t w = (int64_t)r - (int64_t)anchor;
                if (k >= 0 && w >= 0 && w < AM_W) atomicAdd(&s_cell[am_cell(k, (int32_t)w, col)], 1u);
                else atomicAdd(&a.counts[(row0 + (size_t)(r - lo_a)) * AM_COLS + col], 1u);
            });
        }
        __syncthreads();
    }
    amplicon_flush(s_cell, s_slots, (1u << AM_SLOTS) - 1u, a);
}

static AmpliconState *amplicon_state(amp_ctx *c) { return hook_state<AmpliconState>(c, HOOK_AMPLICON); }

static int amplicon_enqueue(amp_ctx *c, const amp_dev_reads *rd, const amp_trim_out *o) {
    const HookCtx q = ctx_hook(c);
    AmpliconState *s = amplicon_state(c);
    // (a block's slots go to the table when they move, not per tile)
    return hook_launch(q, s, amplicon_hook, rd->n_reads, o, AM_BLOCK, AM_TILES_PER_BLOCK, AM_BLOCKS_PER_CU, [&](unsigned grid) {
        const AmpliconTables T = {q.ref_len, s->n_amp, s->d_lo, s->d_hi, s->d_off, s->d_start, s->d_end};
        k_amplicon<<<grid, AM_BLOCK, 0, q.stream>>>(AmpliconArgs{tally_reads(q, rd, o), T, s->d_counts, s->d_reads});
    });
}

HookOps amplicon_hook = {"the amplicon tables need", OUT_NEW_POS | OUT_NEW_NCIG | OUT_NEW_CIG | OUT_STATUS, amplicon_enqueue, hook_free<AmpliconState>};

}  // namespace amp

using namespace amp;

extern "C" {

int amp_amplicon_enable(amp_ctx *c, int32_t n_amp, const int32_t *lo, const int32_t *hi, const int32_t *amp_start, const int32_t *amp_end) {
    if (!c) return AMP_EINVAL;
    const HookCtx q = ctx_hook(c);
    HookSlot &slot = hook_slot(c, HOOK_AMPLICON);
    if (n_amp == 0 || !lo || !hi || !amp_start || !amp_end) { slot.on = false; return AMP_OK; }
    if (n_amp < 0) return AMP_EINVAL;
    const size_t A = (size_t)n_amp, G = (size_t)q.ref_len;
    std::vector<uint32_t> off(A);
    int64_t cells = 0;
    for (size_t k = 0; k < A; ++k) {
        if (lo[k] < 0 || lo[k] >= hi[k] || hi[k] > q.ref_len) {
            snprintf(q.err, q.err_cap, "amplicon %zu: span [%d, %d) is empty or outside the reference", k, lo[k], hi[k]);
            return AMP_EINVAL;
        }
        off[k] = (uint32_t)cells;
        cells += (int64_t)hi[k] - lo[k];
        if (cells > AM_MAX_CELLS) {
            snprintf(q.err, q.err_cap, "the amplicon spans add up to more than %lld positions", (long long)AM_MAX_CELLS);
            return AMP_EINVAL;
        }
    }
    for (size_t p = 0; p < G; ++p) {
        if (amp_start[p] < -1 || amp_start[p] >= n_amp || amp_end[p] < -1 || amp_end[p] >= n_amp) {
            snprintf(q.err, q.err_cap, "owner tables: position %zu names an amplicon outside [0, %d)", p, n_amp);
            return AMP_EINVAL;
        }
    }
    Guard g(q.device);
    AmpliconState *s = amplicon_state(c);
    if (s && (s->n_amp != n_amp || s->cells != cells)) {
        // another amplicon set: the tables are laid out again (a kernel of the old one may still be in flight)
        HOOKCHK(q, hipStreamSynchronize(q.stream));
        hook_free<AmpliconState>(s);
        s = nullptr; slot.state = nullptr; slot.on = false;
    }
    if (!s) {
        HOOKTRY(hook_new_state(q, slot, amplicon_hook, s, [&](AmpliconState &f) -> int {
            f.n_amp = n_amp; f.cells = cells;
            const size_t n_counts = (size_t)cells * AM_COLS;
            HOOKTRY(hook_alloc(q, f, &f.d_lo, A * 12));
            f.d_hi = f.d_lo + A; f.d_off = (uint32_t *)(f.d_hi + A);
            HOOKTRY(hook_alloc(q, f, &f.d_start, std::max<size_t>(G * 8, 8)));
            f.d_end = f.d_start + G;
            HOOKTRY(hook_alloc(q, f, &f.d_counts, n_counts * 4, n_counts * 4));
            HOOKTRY(hook_alloc(q, f, &f.d_reads, (A + 1) * 8, (A + 1) * 8));
            hook_table(f, f.d_counts, n_counts);
            hook_table(f, f.d_reads, A + 1);
            return AMP_OK;
        }));
    }
    slot.on = false;
    HOOKCHK(q, hipMemcpyAsync(s->d_lo, lo, A * 4, hipMemcpyHostToDevice, q.stream));
    HOOKCHK(q, hipMemcpyAsync(s->d_hi, hi, A * 4, hipMemcpyHostToDevice, q.stream));
    HOOKCHK(q, hipMemcpyAsync(s->d_off, off.data(), A * 4, hipMemcpyHostToDevice, q.stream));
    if (G) {
        HOOKCHK(q, hipMemcpyAsync(s->d_start, amp_start, G * 4, hipMemcpyHostToDevice, q.stream));
        HOOKCHK(q, hipMemcpyAsync(s->d_end, amp_end, G * 4, hipMemcpyHostToDevice, q.stream));
    }
    HOOKTRY(hook_zero(q, *s));
    HOOKCHK(q, hipStreamSynchronize(q.stream));        // (the caller's arrays and `off` are free again)
    slot.on = true;
    return AMP_OK;
}

int amp_amplicon_get(amp_ctx *c, uint32_t *counts, uint64_t *reads) { return hook_get(c, HOOK_AMPLICON, {counts, reads}); }

int amp_amplicon_add(amp_ctx *c, const uint32_t *counts, const uint64_t *reads) { return hook_add_tables(c, HOOK_AMPLICON, {counts, reads}); }

int amp_amplicon_last_ms(amp_ctx *c, float *ms) { return hook_last_ms(c, HOOK_AMPLICON, ms); }

}  // extern "C"
