// strand_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_strand.hpp that k_strand calls per read and per
// base, looped over arrays on the CPU in the kernel's own order of steps: tiles of ST_BLOCK reads, their shapes, the window
// rule, the segment list, one add per (segment, position) into the window's cells, the serial walk of the other reads, the
// flush.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libstrand_twin.so strand_twin.cpp   (tests/test_strand_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DSTRAND_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o strand_twin strand_twin.cpp && ./strand_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
// The loop itself is twin_poswin of poswin_twin.hpp, shared with readpos_twin.cpp.
#include <stdint.h>

#include "amp_strand.hpp"
#include "poswin_twin.hpp"

using namespace amp;

// The strand twin's part of twin_poswin: the bits of the return value, and no checks of its own
struct StrandTwin {
    static constexpr int BAD_FLUSH = 1, BAD_LIST = 2, BAD_SEG = 4, BAD_WALK = 8, BAD_CELL = 16;
    int seg_check(const StrandSeg &, int32_t) { return 0; }
    int walk_check(uint32_t) { return 0; }
    void added(int32_t, int, uint32_t) {}
    int flushed(int32_t, int, uint32_t) { return 0; }
};

extern "C" {

int twin_window() { return ST_W; }
int twin_slots() { return ST_SLOTS; }

// The reads are given as they are walked (with do_trim: the trimmed pos and CIGAR).  rev: uint32[ref_len][6], qsum:
// uint64[ref_len][5], both added to.  info[0..3]: reads that took the window, reads that walked serially, flushes that found a
// non-zero cell, adds the serial reads made inside the window.  force_serial: every read walks (the window stays empty).
// Returns non-zero when a step left its bounds (a cell outside the window, a segment past the list, a position past the tables).
int twin_strand(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
                const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *qual, const uint8_t *status, int32_t ref_len, int32_t min_quality,
                int32_t force_serial, uint32_t *rev, unsigned long long *qsum, int64_t *info) {      // (qsum: 64 bits, as the kernel's atomics name them)
    StrandTwin x;
    return twin_poswin<StrandTally>(n, pos, flag, lseq, cig_off, cig, seq_off8, seq, qual, status, ref_len, min_quality, force_serial,
                                    StrandTally::Out{rev, qsum}, info, x);
}

}  // extern "C"

#ifdef STRAND_TWIN_MAIN
#define TWIN_NAME "strand_twin"
#include "twin_main.hpp"

int main() {
    int64_t windowed = 0, serial = 0;
    for (int round = 0; round < 300; ++round) {
        TwinReads b;
        b.draw(round);
        const int32_t G = b.G, mq = b.mq;
        const size_t nr = (size_t)G * ST_REV_COLS, nq = (size_t)G * ST_QSUM_COLS;
        uint32_t *rev[2]; unsigned long long *qs[2];
        int64_t info[2][4];
        for (int mode = 0; mode < 2; ++mode) {
            rev[mode] = (uint32_t *)calloc(nr, 4); qs[mode] = (unsigned long long *)calloc(nq, 8);
            CHECK(twin_strand(b.n, b.pos, b.flag, b.lseq, b.coff, b.cig, b.soff, b.seq, b.qual, b.status, G, mq, mode, rev[mode], qs[mode], info[mode]) == 0);
        }
        // the window and the walk agree on every read, and the all-serial run never touches the segments
        CHECK(memcmp(rev[0], rev[1], nr * 4) == 0 && memcmp(qs[0], qs[1], nq * 8) == 0);
        CHECK(info[1][0] == 0 && info[0][0] + info[0][1] == info[1][1]);
        windowed += info[0][0]; serial += info[0][1];
        // a quality sum is at least min_quality per reverse read that was counted there
        for (int32_t p = 0; p < G; ++p)
            for (int c = 0; c < ST_QSUM_COLS; ++c) CHECK(qs[0][(size_t)p * ST_QSUM_COLS + c] >= (uint64_t)mq * rev[0][(size_t)p * ST_REV_COLS + c]);
        b.release();
        for (int mode = 0; mode < 2; ++mode) { free(rev[mode]); free(qs[mode]); }
    }
    CHECK(windowed > 1000 && serial > 1000);
    printf("strand_twin ok\n");
    return 0;
}
#endif
