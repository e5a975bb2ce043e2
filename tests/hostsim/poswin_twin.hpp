// poswin_twin -- TEST INFRASTRUCTURE: the CPU loop of strand_twin.cpp and readpos_twin.cpp, once.  It is tally_poswin
// (amplipy_amd/csrc/amp_tally.hpp) over the same policy T (StrandTally, ReadposTally), in the kernel's own order of steps: tiles of
// T::BLOCK reads, their shapes, the window rule, the segment list, one add per (segment, position) into the window's words,
// the serial walk of the other reads, the flush (when the window moves, every T::MAX_TILES_PER_FLUSH tiles, at the end).
// Plain g++, no HIP headers.
#pragma once

#include <stdint.h>

#include <vector>

#include "amp_strand.hpp"

namespace amp {

// The reads are given as they are walked (with do_trim: the trimmed pos and CIGAR); `out`: the tables, added to.  info[0..3]:
// reads that took the window, reads that walked serially, flushes that found a non-zero word, walked increments that fell
// inside the window.  force_serial: every read walks (the window stays empty).  X is the twin's own part: the bits of the return
// value for a step that left its bounds (BAD_CELL: a word outside the window; BAD_FLUSH and BAD_WALK: a position past the
// tables; BAD_LIST: a segment past the list; BAD_SEG: a segment outside the window), and what it checks besides -- seg_check(g,
// k) and walk_check(x) give bits to raise, added(w, c, v) follows every add to the window, flushed(w, k, v) -> bits sees
// every non-zero word a flush takes.
template <class T, class X>
int twin_poswin(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                int32_t force_serial, const typename T::Out &out, int64_t *info, X &x) {
    using Seg = typename T::Seg;
    const StrandParams P{ref_len, min_quality};
    std::vector<uint32_t> cell((size_t)T::W * T::WORDS, 0u);
    std::vector<Seg> segs((size_t)T::BLOCK * T::SLOTS);
    int bad = 0;
    int32_t anchor = 0;
    int since = 0;
    for (int k = 0; k < 4; ++k) info[k] = 0;
    const auto plus = [](auto *p, auto v) { *p += v; };
    auto window_add = [&](int32_t w, int c, uint32_t v) {
        const int k = T::word(w, c);
        if (w < 0 || w >= T::W || k < w * T::WORDS || k >= (w + 1) * T::WORDS) { bad |= X::BAD_CELL; return; }
        cell[(size_t)k] += T::inc(c, v);
        x.added(w, c, v);
    };
    auto flush = [&]() {
        bool any = false;
        for (int k = 0; k < T::W * T::WORDS; ++k) {
            const uint32_t v = cell[(size_t)k];
            if (!v) continue;
            any = true;
            cell[(size_t)k] = 0u;
            const int64_t p = (int64_t)anchor + k / T::WORDS;
            if (p < 0 || p >= ref_len) { bad |= X::BAD_FLUSH; continue; }
            bad |= x.flushed(k / T::WORDS, k % T::WORDS, v);
            T::flush_word(out, (size_t)p, k % T::WORDS, v, plus);
        }
        if (any) ++info[2];
    };
    for (int64_t base = 0; base < n; base += T::BLOCK) {
        const int m = (int)(n - base < T::BLOCK ? n - base : T::BLOCK);
        StrandRead R[T::BLOCK];
        StrandShape sh[T::BLOCK];
        bool live[T::BLOCK], win[T::BLOCK];
        uint32_t qual0[T::BLOCK];
        int32_t lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
        for (int t = 0; t < m; ++t) {
            const int64_t i = base + t;
            live[t] = !status || status[i] == 0;
            R[t] = StrandRead{pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], (int32_t)lseq[i], (flag[i] & 0x10u) ? 1u : 0u, (uint64_t)seq_off8[i] * 8ull};
            qual0[t] = R[t].lseq > 0 ? qual[R[t].base] : 0xFFu;
            sh[t] = StrandShape{false, 0, 0};
            if (!live[t]) continue;
            sh[t] = T::segments(R[t], P, qual0[t], [](const Seg &) {});
            if (force_serial) sh[t].regular = false;
            if (sh[t].regular) { lo = R[t].pos < lo ? R[t].pos : lo; hi = sh[t].ref_end > hi ? sh[t].ref_end : hi; }
        }
        if (!poswin_keeps<T::W>(anchor, lo, hi) || since >= T::MAX_TILES_PER_FLUSH) {
            flush();
            if (lo <= hi) anchor = lo;
            since = 0;
        }
        ++since;
        size_t ns = 0;
        for (int t = 0; t < m; ++t) {
            win[t] = live[t] && poswin_read_windowed<T::W, T::SLOTS>(sh[t], R[t].pos, anchor);
            if (!win[t]) continue;
            ++info[0];
            T::segments(R[t], P, qual0[t], [&](const Seg &s) {
                if (ns < segs.size()) segs[ns++] = s; else bad |= X::BAD_LIST;
            });
        }
        for (size_t s = 0; s < ns; ++s) {
            const Seg g = segs[s];
            const int32_t a0 = g.r0 - anchor, a1 = a0 + st_seg_len(g);
            if (a0 < 0 || a1 > T::W) { bad |= X::BAD_SEG; continue; }
            for (int32_t p = a0; p < a1; ++p) {
                bad |= x.seg_check(g, p - a0);
                T::seg_adds(g, p - a0, seq, qual, min_quality, [&](int c, uint32_t v) { window_add(p, c, v); });
            }
        }
        for (int t = 0; t < m; ++t) {
            if (!live[t] || win[t]) continue;
            ++info[1];
            T::walk(R[t], P, seq, qual, [&](int32_t r, uint32_t col, auto d) {
                if (r < 0 || r >= ref_len || col > 5u) { bad |= X::BAD_WALK; return; }
                if (const int b = x.walk_check(d)) { bad |= b; return; }
                const int64_t w = (int64_t)r - (int64_t)anchor;
                const bool inside = w >= 0 && w < T::W;
                if (inside) ++info[3];
                T::walk_adds(R[t], col, d, [&](int c, uint32_t v) {
                    if (inside) window_add((int32_t)w, c, v);
                    else T::to_table(out, (size_t)r, c, v, plus);
                });
            });
        }
    }
    flush();
    return bad;
}

}  // namespace amp
