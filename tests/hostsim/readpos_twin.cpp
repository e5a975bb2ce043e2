// readpos_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_readpos.hpp that k_readpos calls per read and per
// base, looped over arrays on the CPU in the kernel's own order of steps: tiles of RP_BLOCK reads, their shapes, the window
// rule, the segment list, one add per (segment, position) into the window's 16-bit halves, the serial walk of the other reads,
// the flush (when the window moves, every RP_MAX_TILES_PER_FLUSH tiles, at the end).  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libreadpos_twin.so readpos_twin.cpp   (tests/test_readpos_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DREADPOS_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o readpos_twin readpos_twin.cpp && ./readpos_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
// The loop itself is twin_poswin of poswin_twin.hpp, shared with strand_twin.cpp.
#include <stdint.h>

#include <vector>

#include "amp_readpos.hpp"
#include "poswin_twin.hpp"

using namespace amp;

// The readpos twin's part of twin_poswin: the bits of the return value, no negative distance (64), and every add once more into
// a u32 per cell, so that a carry between the halves of a word shows when the word is flushed (32)
struct ReadposTwin {
    static constexpr int BAD_CELL = 1, BAD_FLUSH = 2, BAD_LIST = 4, BAD_SEG = 8, BAD_WALK = 16;
    std::vector<uint32_t> shadow = std::vector<uint32_t>((size_t)RP_W * RP_CELLS, 0u);
    int64_t *info;
    int seg_check(const ReadposSeg &g, int32_t k) { return rp_seg_d(g, k) < 0 ? 64 : 0; }
    int walk_check(int32_t d) { return d < 0 ? 64 : 0; }
    void added(int32_t w, int c, uint32_t v) { shadow[(size_t)w * RP_CELLS + c] += v; }
    int flushed(int32_t w, int k, uint32_t v) {
        const uint32_t half[2] = {v & 0xFFFFu, v >> 16};
        int bad = 0;
        for (int h = 0; h < 2; ++h) {
            uint32_t &want = shadow[(size_t)w * RP_CELLS + 2 * k + h];
            if (half[h] != want) bad = 32;
            if ((int64_t)half[h] > info[4]) info[4] = half[h];
            want = 0u;
        }
        return bad;
    }
};

extern "C" {

int twin_window() { return RP_W; }
int twin_slots() { return RP_SLOTS; }
int twin_flush_period() { return RP_MAX_TILES_PER_FLUSH; }
int twin_rp_bin(int32_t d) { return (int)rp_bin(d); }

// The reads are given as they are walked (with do_trim: the trimmed pos and CIGAR).  hist: uint32[ref_len][6][7], added to.
// info[0..4]: reads that took the window, reads that walked serially, flushes that found a non-zero word, adds the serial reads
// made inside the window, the largest 16-bit half a flush met.  force_serial: every read walks (the window stays empty).
// Returns non-zero when a step left its bounds (a word outside the window, a segment past the list, a position past the
// table, a negative distance, a half that carried).
int twin_readpos(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                 const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                 int32_t force_serial, uint32_t *hist, int64_t *info) {
    ReadposTwin x;
    x.info = info;
    info[4] = 0;
    return twin_poswin<ReadposTally>(n, pos, flag, lseq, cig_off, cig, seq_off8, seq, qual, status, ref_len, min_quality, force_serial,
                                     ReadposTally::Out{hist}, info, x);
}

}  // extern "C"

#ifdef READPOS_TWIN_MAIN
#define TWIN_NAME "readpos_twin"
#include "twin_main.hpp"

int main() {
    int64_t windowed = 0, serial = 0;
    for (int32_t d = 0; d < 300; ++d) {
        const uint32_t want = d < 2 ? 0u : d < 4 ? 1u : d < 8 ? 2u : d < 16 ? 3u : d < 32 ? 4u : d < 64 ? 5u : 6u;
        CHECK(rp_bin(d) == want);
    }
    CHECK(rp_bin(0x7FFFFFFF) == 6u);
    for (int round = 0; round < 300; ++round) {
        TwinReads b;
        b.draw(round);
        const size_t nh = (size_t)b.G * RP_CELLS;
        uint32_t *hist[2];
        int64_t info[2][5];
        for (int mode = 0; mode < 2; ++mode) {
            hist[mode] = (uint32_t *)calloc(nh, 4);
            CHECK(twin_readpos(b.n, b.pos, b.flag, b.lseq, b.coff, b.cig, b.soff, b.seq, b.qual, b.status, b.G, b.mq, mode, hist[mode], info[mode]) == 0);
        }
        // the window and the walk agree on every read, and the all-serial run never touches the segments
        CHECK(memcmp(hist[0], hist[1], nh * 4) == 0);
        CHECK(info[1][0] == 0 && info[0][0] + info[0][1] == info[1][1]);
        windowed += info[0][0]; serial += info[0][1];
        b.release();
        for (int mode = 0; mode < 2; ++mode) free(hist[mode]);
    }
    CHECK(windowed > 1000 && serial > 1000);
    printf("readpos_twin ok\n");
    return 0;
}
#endif
