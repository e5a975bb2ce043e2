// The host twin of the SAM text codec (amplipy_amd/csrc/amp_sam.hip, -DAMPSAM_HOSTSIM) as a program, so that it can run under
// -fsanitize=address,undefined without a sanitizer runtime inside the Python process (tests/test_sam_text.py, the fuzz test).
//
//   sam_twin_main IN OUT NAME...        NAME: the @SQ names
// IN:  per chunk  int64 n_bytes, the bytes.
// OUT: per chunk  amp_sam_info; and when no line is odd: the batch (pos, flag, tlen, lseq, cig_off u64[n+1], cig, seq_off u64[n+1],
//      seq, qual, src_index), then the text of the format stage for results that change nothing (new POS / CIGAR = the input's, every
//      row kept): int64 n_bytes, the bytes.
#include <stdio.h>

#include <vector>

#include "amp_sam.hip"

static void put(FILE *f, const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(2); } }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    amp_sam *s = nullptr;
    if (amp_sam_create(nullptr, &s)) return 3;
    if (amp_sam_set_references(s, argc - 3, argv + 3)) return 3;
    std::vector<uint8_t> text, seq, qual, o_text, flags, status;
    std::vector<int32_t> pos, tlen, ref_len;
    std::vector<uint16_t> flag;
    std::vector<uint32_t> lseq, cig, ncig, new_cig;
    std::vector<uint64_t> cig_off, seq_off;
    std::vector<int64_t> src;
    int64_t n_bytes = 0;
    while (fread(&n_bytes, 8, 1, in) == 1) {
        text.resize((size_t)n_bytes);                           // (exactly n_bytes: a read behind the chunk is a finding)
        if (n_bytes && fread(text.data(), 1, (size_t)n_bytes, in) != (size_t)n_bytes) return 4;
        amp_sam_info info;
        const int rc = amp_sam_parse(s, text.data(), n_bytes, &info);
        if (rc) { fprintf(stderr, "amp_sam_parse: %d\n", rc); return 5; }
        put(out, &info, sizeof(info));
        if (info.first_odd_line >= 0) continue;
        const size_t n = (size_t)info.n_rows, nc = (size_t)info.n_cig, nb = (size_t)info.n_bases_padded;
        pos.resize(n); flag.resize(n); tlen.resize(n); lseq.resize(n); cig_off.resize(n + 1); cig.resize(nc); seq_off.resize(n + 1);
        seq.resize(nb / 2); qual.resize(nb); src.resize(n);
        const amp_reads dst{(int64_t)n, pos.data(), flag.data(), tlen.data(), lseq.data(), cig_off.data(), cig.data(), seq_off.data(), seq.data(), qual.data()};
        if (amp_sam_batch_to_host(s, &dst, src.data())) return 6;
        put(out, pos.data(), n * 4); put(out, flag.data(), n * 2); put(out, tlen.data(), n * 4); put(out, lseq.data(), n * 4);
        put(out, cig_off.data(), (n + 1) * 8); put(out, cig.data(), nc * 4); put(out, seq_off.data(), (n + 1) * 8);
        put(out, seq.data(), nb / 2); put(out, qual.data(), nb); put(out, src.data(), n * 8);
        ncig.resize(n); new_cig.assign(nc + 3 * n, 0); ref_len.assign(n, 1 << 20); flags.assign(n, 0); status.assign(n, 0);
        for (size_t i = 0; i < n; ++i) {
            ncig[i] = (uint32_t)(cig_off[i + 1] - cig_off[i]);
            for (uint32_t k = 0; k < ncig[i]; ++k) new_cig[(size_t)cig_off[i] + 3 * i + k] = cig[(size_t)cig_off[i] + k];
        }
        int64_t bad = 0, need = 0, rows = 0;
        uint8_t st = 0;
        if (amp_sam_twin_set_results(s, pos.data(), ncig.data(), new_cig.data(), ref_len.data(), flags.data(), status.data(), &bad, &st)) return 7;
        if (amp_sam_format(s, 1, 1, nullptr, 0, &need, &rows) != (need ? AMP_EOVERFLOW : AMP_OK)) return 8;
        o_text.resize((size_t)need);                            // (exactly the size asked for)
        if (amp_sam_format(s, 1, 1, o_text.data(), need, &need, &rows)) return 9;
        put(out, &need, 8); put(out, o_text.data(), (size_t)need);
    }
    amp_sam_destroy(s);
    fclose(in);
    if (fclose(out)) return 2;
    return 0;
}
