// clip_twin -- TEST INFRASTRUCTURE: the functions of amplipy_amd/csrc/amp_clip.hpp that k_qc_clips calls per read, looped over
// arrays on the CPU.  Built with plain g++ (no HIP headers):
//   g++ -O1 -g -std=c++17 -fPIC -shared -I amplipy_amd/csrc -o libclip_twin.so clip_twin.cpp        (tests/test_clips_twin.py, ctypes)
//   g++ -O1 -g -std=c++17 -DCLIP_TWIN_MAIN -fsanitize=address,undefined -I amplipy_amd/csrc -o clip_twin clip_twin.cpp && ./clip_twin
// The second form is a program of its own, so that it runs under the sanitizers without a sanitizer runtime inside Python:
// seeded batches in heap blocks of exactly the needed size, so a read outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "amp_clip.hpp"

using namespace amp;

extern "C" {

// k_qc_clips without the wave combine: every read adds its own cells.  table: [(ref_len + 1)][2][CL_CELLS], scalars: [4];
// both are added to.  -1 when a site lies outside the table.
int twin_clips(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *lseq, const uint32_t *cig_off, const uint32_t *cig,
               const uint32_t *seq_off8, const uint8_t *seq, const uint8_t *status, int32_t ref_len, int32_t clip_min, uint32_t *table,
               uint64_t *scalars) {
    for (int64_t i = 0; i < n; ++i) {
        if (status && status[i] != 0) continue;
        const int32_t L = (int32_t)lseq[i];
        const ClipRead r = clip_scan(pos[i], cig + cig_off[i], cig_off[i + 1] - cig_off[i], L, ref_len, clip_min);
        if (r.skipped) {
            if (r.p[0] >= 0 || r.p[1] >= 0) return -1;
            ++scalars[CL_SKIPPED];
            continue;
        }
        ++scalars[CL_SCANNED];
        for (int side = 0; side < 2; ++side) {
            if (r.p[side] < 0) continue;
            if (r.p[side] > ref_len || r.L[side] < clip_min) return -1;
            ++scalars[CL_N_LEFT + side];
            uint32_t *cells = table + clip_site_word(r.p[side], side);
            const uint64_t cols = clip_cols(seq, (uint64_t)seq_off8[i] * 8ull, L, side, r.L[side]);
            cells[0] += 1u;
            cells[1] += (flag[i] & 0x10u) ? 1u : 0u;
            for (int j = 0; j < CL_K; ++j) {
                const uint32_t f = clip_field(cols, j);
                if (f == CL_NO_COL) {
                    if (j < r.L[side]) return -1;
                    continue;
                }
                if (f >= (uint32_t)CL_COLS || j >= r.L[side]) return -1;
                cells[2 + j * CL_COLS + (int)f] += 1u;
            }
        }
    }
    return 0;
}

int twin_clip_sizes(int32_t *out) {
    out[0] = CL_K; out[1] = CL_COLS; out[2] = CL_CELLS; out[3] = CL_N_SCALARS; out[4] = CL_MIN_MAX; out[5] = CL_LEFT; out[6] = CL_RIGHT;
    return 7;
}

}  // extern "C"

#ifdef CLIP_TWIN_MAIN
#define TWIN_NAME "clip_twin"
#include "twin_main.hpp"

int main() {
    for (int round = 0; round < 300; ++round) {
        TwinReads B;
        B.draw(round);
        const int32_t clip_min = 1 + (int32_t)rnd(CL_MIN_MAX);
        const size_t words = clip_table_words(B.G);
        uint32_t *table = (uint32_t *)calloc(words, 4);
        uint64_t *scalars = (uint64_t *)calloc(CL_N_SCALARS, 8);
        CHECK(twin_clips(B.n, B.pos, B.flag, B.lseq, B.coff, B.cig, B.soff, B.seq, round % 2 ? B.status : nullptr, B.G, clip_min, table, scalars) == 0);
        uint64_t live = 0, reads[2] = {0, 0};
        for (int64_t i = 0; i < B.n; ++i) live += (round % 2 && B.status[i]) ? 0u : 1u;
        CHECK(scalars[CL_SCANNED] + scalars[CL_SKIPPED] == live);
        CHECK(scalars[CL_N_LEFT] <= scalars[CL_SCANNED] && scalars[CL_N_RIGHT] <= scalars[CL_SCANNED]);
        for (int32_t p = 0; p <= B.G; ++p)
            for (int side = 0; side < 2; ++side) {
                const uint32_t *cells = table + clip_site_word(p, side);
                reads[side] += cells[0];
                CHECK(cells[1] <= cells[0]);
                uint32_t before = cells[0];
                for (int j = 0; j < CL_K; ++j) {             // the depth of an offset never grows with the offset
                    uint32_t d = 0;
                    for (int c = 0; c < CL_COLS; ++c) d += cells[2 + j * CL_COLS + c];
                    CHECK(d <= before);
                    if (j < clip_min && j < CL_K) CHECK(d == cells[0]);
                    before = d;
                }
            }
        CHECK(reads[0] == scalars[CL_N_LEFT] && reads[1] == scalars[CL_N_RIGHT]);
        free(table); free(scalars);
        B.release();
    }
    printf("clip_twin ok\n");
    return 0;
}
#endif
