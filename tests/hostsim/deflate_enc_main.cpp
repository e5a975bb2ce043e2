// deflate_enc_main.cpp -- the DEFLATE encoder's phases (amplipy_amd/csrc/amp_deflate.hip, -DAMPDF_HOSTSIM) as a program of its own,
// for -fsanitize=address,undefined on the host code: tests/test_deflate_enc_craft.py writes the crafted chunks of
// tests/deflate_enc_craft.py into a file (per chunk a line `name n_bytes room` and the bytes), this program encodes each at the four
// misalignments of its source and writes the streams into a second file (per stream a line `name skew out_len` and the bytes), and
// the test compares them with what the shared library of the same phases gives.
//
// Every buffer is a heap block of exactly the bytes the encoder may touch: the source is the aligned dwords that hold at least one
// byte of the chunk (phase 0 reads whole dwords), the destination is `room` bytes.  A read or write beyond them ends the program.
//
//   usage: deflate_enc_main cases.bin streams.bin
#include "../../amplipy_amd/csrc/amp_deflate.hip"

#include <stdlib.h>

#include <string>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin streams.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    char name[128];
    long n_bytes, room;
    int n_cases = 0, n_streams = 0;
    while (fscanf(in, "%127s %ld %ld", name, &n_bytes, &room) == 3) {
        if (fgetc(in) != '\n' || n_bytes < 1 || n_bytes > 0xFF00 || room < 0 || room > 65536) { fprintf(stderr, "%s: bad case line\n", name); return 2; }
        std::vector<uint8_t> chunk((size_t)n_bytes);
        if (fread(chunk.data(), 1, chunk.size(), in) != chunk.size()) { fprintf(stderr, "%s: short case\n", name); return 2; }
        ++n_cases;
        for (int skew = 0; skew < 4; ++skew) {
            const size_t src_bytes = ((size_t)skew + (size_t)n_bytes + 3) & ~(size_t)3;
            void *src = nullptr;
            if (posix_memalign(&src, 8, src_bytes)) return 2;
            memset(src, 0x5A, src_bytes);
            memcpy((uint8_t *)src + skew, chunk.data(), chunk.size());
            uint8_t *dst = (uint8_t *)malloc(room ? (size_t)room : 1);
            uint32_t *len = (uint32_t *)malloc(sizeof(uint32_t));
            if (!dst || !len) return 2;
            *len = 0xFFFFFFFFu;
            const int rc = ampdf_hostsim_blocks((const uint8_t *)src + skew, n_bytes, (int32_t)n_bytes, dst, room, (int32_t)room, len);
            if (rc != 0 || *len > (uint32_t)room) { fprintf(stderr, "%s skew %d: rc %d, out_len %u\n", name, skew, rc, *len); return 1; }
            fprintf(out, "%s %d %u\n", name, skew, *len);
            fwrite(dst, 1, *len, out);
            ++n_streams;
            free(src); free(dst); free(len);
        }
    }
    if (fclose(out) != 0) return 2;
    fclose(in);
    printf("cases %d, streams %d\n", n_cases, n_streams);
    return 0;
}
