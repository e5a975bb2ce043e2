// bgzf_cases -- TEST INFRASTRUCTURE: runs the crafted DEFLATE streams of tests/deflate_craft.py (dumped to a file by its dump())
// through the lane functions of the device codec for BAM input (amplipy_amd/csrc/amp_bgzf.hpp: inflate_block and the CRC-32 by 64
// lanes) under AddressSanitizer / UBSan on the CPU, as bgzf_fuzz.cpp does for zlib's streams.  A valid case must give its bytes
// and its CRC, a refused one must be refused, and neither may touch a byte outside its exactly-sized heap blocks.  One Tables
// object serves all cases, as one LDS object serves all blocks of a workgroup.
//   g++ -O1 -g -fsanitize=address,undefined -o bgzf_cases bgzf_cases.cpp && ./bgzf_cases cases.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define BGZ_HD static inline
#include "../../amplipy_amd/csrc/amp_bgzf.hpp"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bgzf_cases FILE\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    static ampbgzf::Tables tabs;
    static uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = ampbgzf::crc_table_entry(i);
    long n_valid = 0, n_refused = 0, bad = 0;
    char line[512], name[256], kind[16];
    while (fgets(line, sizeof(line), f)) {
        unsigned long n_raw = 0, n_out = 0, crc = 0;
        if (sscanf(line, "%255s %15s %lu %lu %lu", name, kind, &n_raw, &n_out, &crc) != 5) { fprintf(stderr, "bad line: %s", line); return 2; }
        const bool valid = strcmp(kind, "valid") == 0;
        uint8_t *in = (uint8_t *)malloc(n_raw ? n_raw : 1), *out = (uint8_t *)malloc(n_out ? n_out : 1), *want = (uint8_t *)malloc(n_out ? n_out : 1);
        if (fread(in, 1, n_raw, f) != n_raw || (valid && fread(want, 1, n_out, f) != n_out)) { fprintf(stderr, "%s: short file\n", name); return 2; }
        const bool ok = ampbgzf::inflate_block(in, n_raw, out, n_out, tabs);
        if (valid) {
            ++n_valid;
            if (!ok || (n_out && memcmp(out, want, n_out) != 0)) { ++bad; fprintf(stderr, "%s: %s\n", name, ok ? "wrong bytes" : "refused"); }
            uint32_t reg = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) reg ^= ampbgzf::crc_lane(want, (uint32_t)n_out, lane, crc_tab);
            if ((~reg) != (uint32_t)crc) { ++bad; fprintf(stderr, "%s: crc differs\n", name); }
        } else {
            ++n_refused;
            if (ok) { ++bad; fprintf(stderr, "%s: accepted\n", name); }
        }
        free(in); free(out); free(want);
    }
    fclose(f);
    printf("valid %ld, refused %ld, failed %ld\n", n_valid, n_refused, bad);
    return bad ? 1 : 0;
}
