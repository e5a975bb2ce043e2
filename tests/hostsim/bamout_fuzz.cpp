// The host twin of the BAM device codec with its re-encoder of trimmed records (amplipy_amd/csrc/amp_bgzf.hip + amp_bamout.hip,
// -DAMPBGZF_HOSTSIM) as a program, so that it can run under -fsanitize=address,undefined without a sanitizer runtime inside the
// Python process (tests/test_bam_reencode_twin.py).
//
//   bamout_fuzz N_FILES [SEED]
// Per file: random BAM records (names of 1 to 40 bytes, 0 to 12 CIGAR ops, 0 to 400 bases, aux of 0 to 3,000 bytes and now and
// then 70,000; unmapped ones and ones without CIGAR between them) in BGZF blocks of random sizes (stored DEFLATE blocks: no zlib
// here), fed in random runs of blocks; random results per row (0 to old + 3 ops, any op, pos from -1, random keep, sometimes a
// first failing row); amp_bam_encode behind every feed with rows, the final one at random on the last feed or as a bare flush.
// Checked: the stream of every encode against a plain serial re-encode of the same results, the framed blocks (header, BSIZE,
// stored payload = the stream's chunk, CRC-32, ISIZE, 0xFF00 bytes in all but the last), the guard bytes behind every buffer.
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "amp_bgzf.hip"

typedef std::vector<uint8_t> Bytes;
static std::mt19937_64 rng;
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }
static void put32(Bytes &b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
static void put16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static uint32_t get32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; tab[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
    return ~c;
}

// a stored DEFLATE stream of n <= 65535 bytes
static void stored(Bytes &out, const uint8_t *p, size_t n) {
    out.push_back(1); put16(out, (uint32_t)n); put16(out, (uint32_t)~n & 0xFFFFu);
    out.insert(out.end(), p, p + n);
}
static int stored_deflater(const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len) {
    for (int64_t k = 0; k * block_bytes < n_bytes; ++k) {
        const int64_t n = n_bytes - k * block_bytes < block_bytes ? n_bytes - k * block_bytes : block_bytes;
        Bytes s;
        stored(s, in + k * block_bytes, (size_t)n);
        if ((int64_t)s.size() > out_room) { out_len[k] = 0; continue; }
        memcpy(out + k * out_stride, s.data(), s.size());
        out_len[k] = (uint32_t)s.size();
    }
    return 0;
}

struct Rec { size_t off; bool row; uint32_t n_cig, l_name, bs; };

static void make_record(Bytes &img, std::vector<Rec> &recs) {
    const uint32_t l_name = (uint32_t)rnd(1, 40), l_seq = (uint32_t)rnd(0, 400);
    const bool unmapped = rnd(0, 19) == 0;
    const uint32_t n_cig = rnd(0, 24) == 0 ? 0 : (uint32_t)rnd(1, 12);
    const uint32_t aux = rnd(0, 199) == 0 ? 70000 : (uint32_t)rnd(0, rnd(0, 3) ? 60 : 3000);
    const uint32_t bs = 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq + aux;
    recs.push_back(Rec{img.size(), !unmapped && n_cig > 0, n_cig, l_name, bs});
    put32(img, bs);
    put32(img, 0); put32(img, (uint32_t)rnd(0, 29000));
    img.push_back((uint8_t)l_name); img.push_back(60); put16(img, 4681); put16(img, n_cig); put16(img, unmapped ? 4 : (uint32_t)rnd(0, 3) * 16);
    put32(img, l_seq); put32(img, 0); put32(img, (uint32_t)rnd(0, 29000)); put32(img, (uint32_t)rnd(0, 500));
    for (uint32_t k = 0; k + 1 < l_name; ++k) img.push_back((uint8_t)rnd(33, 126));
    img.push_back(0);
    for (uint32_t k = 0; k < n_cig; ++k) put32(img, ((uint32_t)rnd(1, 300) << 4) | (uint32_t)rnd(0, 8));
    for (uint32_t k = 0; k < (l_seq + 1) / 2 + l_seq + aux; ++k) img.push_back((uint8_t)rng());
}

// ampbam_write_rows' record, written the plain way
static void serial_record(Bytes &out, const uint8_t *rec, int32_t new_pos, uint32_t nn, const uint32_t *cg) {
    const uint32_t bs = get32(rec), l_name = rec[12], old_n = rec[16] | (rec[17] << 8);
    Bytes r(rec + 4, rec + 4 + 32 + l_name);
    int64_t rlen = 0;
    for (uint32_t k = 0; k < nn; ++k) { const uint32_t op = cg[k] & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += cg[k] >> 4; }
    int64_t beg = new_pos > 0 ? new_pos : 0, end = (int64_t)new_pos + (rlen ? rlen : 1);
    if (end < 1) end = 1;
    --end;
    uint32_t bin = 0;
    if (beg >> 14 == end >> 14) bin = (uint32_t)(4681 + (beg >> 14));
    else if (beg >> 17 == end >> 17) bin = (uint32_t)(585 + (beg >> 17));
    else if (beg >> 20 == end >> 20) bin = (uint32_t)(73 + (beg >> 20));
    else if (beg >> 23 == end >> 23) bin = (uint32_t)(9 + (beg >> 23));
    else if (beg >> 26 == end >> 26) bin = (uint32_t)(1 + (beg >> 26));
    for (int k = 0; k < 4; ++k) r[4 + k] = (uint8_t)((uint32_t)new_pos >> (8 * k));
    r[10] = (uint8_t)bin; r[11] = (uint8_t)(bin >> 8); r[12] = (uint8_t)nn; r[13] = (uint8_t)(nn >> 8);
    put32(out, bs - 4 * old_n + 4 * nn);
    out.insert(out.end(), r.begin(), r.end());
    for (uint32_t k = 0; k < nn; ++k) put32(out, cg[k]);
    out.insert(out.end(), rec + 4 + 32 + l_name + 4 * old_n, rec + 4 + bs);
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "file %d: %s (line %d)\n", file_no, #cond, __LINE__); return 1; } } while (0)

static int one_file(int file_no, long *mismatches) {
    Bytes img;
    std::vector<Rec> recs;
    const int n_rec = (int)rnd(0, 1) ? (int)rnd(1, 1500) : (int)rnd(0, 40);
    for (int i = 0; i < n_rec; ++i) make_record(img, recs);
    // BGZF blocks of random sizes, fed in random runs
    std::vector<amp_bam_block> blocks;
    Bytes comp;
    for (size_t at = 0; at < img.size();) {
        const size_t n = std::min<size_t>(img.size() - at, (size_t)rnd(1, rnd(0, 3) ? 65000 : 700));
        const uint32_t in_off = (uint32_t)comp.size();
        stored(comp, img.data() + at, n);
        blocks.push_back(amp_bam_block{in_off, (uint32_t)comp.size() - in_off, (uint32_t)n, crc32_of(img.data() + at, n)});
        at += n;
    }
    amp_bam *s = nullptr;
    CHECK(amp_bam_create(nullptr, &s) == 0);
    CHECK(amp_bam_twin_set_deflater(s, stored_deflater) == 0);
    const int32_t min_length = (int32_t)rnd(0, 60), inp = (int32_t)rnd(0, 1);
    int64_t rec_base = 0;
    size_t next_rec = 0;                       // the first record not yet seen complete
    Bytes want, got, file;
    bool flushed = false, stopped = false;
    for (size_t k0 = 0; k0 < blocks.size() && !stopped;) {
        const size_t k1 = std::min(blocks.size(), k0 + (size_t)rnd(1, rnd(0, 2) ? 4 : 60));
        const bool last = k1 == blocks.size();
        std::vector<amp_bam_block> piece(blocks.begin() + k0, blocks.begin() + k1);
        const uint32_t base = piece[0].in_off;
        for (auto &b : piece) b.in_off -= base;
        const size_t n_comp = blocks[k1 - 1].in_off + blocks[k1 - 1].in_len - base;
        Bytes cp(comp.begin() + base, comp.begin() + base + n_comp);          // (exactly the piece: a read behind it is a finding)
        amp_bam_info info;
        CHECK(amp_bam_feed(s, cp.data(), (int64_t)n_comp, piece.data(), (int64_t)piece.size(), k0 == 0 ? 0 : -1, 1, rec_base, &info) == 0);
        CHECK(info.n_refused == 0 && !info.bad_record);
        rec_base += info.n_records;
        // the rows of this feed: the records that ended in it
        std::vector<size_t> rows;
        for (int64_t i = 0; i < info.n_records; ++i, ++next_rec) if (recs[next_rec].row) rows.push_back(next_rec);
        CHECK((int64_t)rows.size() == info.n_rows);
        k0 = k1;
        const bool final = last && rnd(0, 1);
        if (rows.empty() && !final && rnd(0, 1)) continue;
        const size_t n = rows.size();
        std::vector<int32_t> new_pos(n), ref_len(n);
        std::vector<uint32_t> ncig(n), new_cig;
        std::vector<uint8_t> flags(n);
        std::vector<size_t> slot(n);
        size_t cig_off = 0;
        for (size_t r = 0; r < n; ++r) { slot[r] = cig_off + 3 * r; cig_off += recs[rows[r]].n_cig; }
        new_cig.assign(cig_off + 3 * n + 1, 0);
        for (size_t r = 0; r < n; ++r) {
            const uint32_t old = recs[rows[r]].n_cig;
            new_pos[r] = (int32_t)rnd(0, 9) ? (int32_t)rnd(0, 1 << 29) - (int32_t)rnd(0, 1) : (int32_t)rnd(0, 1) - 1;
            ref_len[r] = (int32_t)rnd(0, 120); flags[r] = (uint8_t)rnd(0, 7);
            ncig[r] = (uint32_t)rnd(0, old + 3);
            for (uint32_t k = 0; k < ncig[r]; ++k) new_cig[slot[r] + k] = ((uint32_t)rnd(0, 1 << 20) << 4) | (uint32_t)(rnd(0, 3) ? rnd(0, 8) : rnd(4, 6));
        }
        const int64_t first_bad = n && rnd(0, 14) == 0 ? (int64_t)rnd(0, n - 1) : -1;
        if (n) CHECK(amp_bam_twin_set_trim(s, new_pos.data(), ncig.data(), new_cig.data(), ref_len.data(), flags.data(), first_bad) == 0);
        const size_t want0 = want.size();
        for (size_t r = 0; r < n; ++r) {
            if (first_bad >= 0 && (int64_t)r >= first_bad) break;
            if (!(ref_len[r] >= min_length && ((flags[r] & 3) || inp))) continue;
            serial_record(want, img.data() + recs[rows[r]].off, new_pos[r], ncig[r], new_cig.data() + slot[r]);
        }
        amp_bam_out_info oi;
        CHECK(amp_bam_encode(s, min_length, inp, final ? 1 : 0, &oi) == 0);
        CHECK(amp_bam_twin_guards(s) == 0);
        CHECK(oi.waits == 1 && oi.n_blocks_host == 0);
        CHECK(oi.stream_bytes - oi.carry_in == (int64_t)(want.size() - want0));
        Bytes part((size_t)(oi.stream_bytes - oi.carry_in));                     // (exactly the size: a write behind it is a finding)
        CHECK(amp_bam_stream_to_host(s, oi.carry_in, (int64_t)part.size(), part.data()) == 0);
        got.insert(got.end(), part.begin(), part.end());
        Bytes fb((size_t)oi.file_bytes);
        CHECK(amp_bam_encoded_to_host(s, fb.data(), (int64_t)fb.size()) == 0);
        file.insert(file.end(), fb.begin(), fb.end());
        flushed = final;
        if (first_bad >= 0) { stopped = true; flushed = false; }
    }
    if (!flushed) {
        amp_bam_out_info oi;
        CHECK(amp_bam_encode(s, min_length, inp, 1, &oi) == 0);
        CHECK(oi.n_rows_written == 0 && oi.carry_out == 0 && oi.n_blocks <= 1);
        Bytes fb((size_t)oi.file_bytes);
        CHECK(amp_bam_encoded_to_host(s, fb.data(), (int64_t)fb.size()) == 0);
        file.insert(file.end(), fb.begin(), fb.end());
        CHECK(amp_bam_twin_guards(s) == 0);
    }
    amp_bam_destroy(s);
    if (got != want) { ++*mismatches; fprintf(stderr, "file %d: stream differs (%zu bytes, %zu wanted)\n", file_no, got.size(), want.size()); return 0; }
    // the framed blocks: stored payloads that give the stream back, chunk by chunk
    size_t at = 0, done = 0;
    while (at < file.size()) {
        const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        CHECK(at + 26 <= file.size() && memcmp(file.data() + at, hdr, 16) == 0);
        const size_t bsize = (size_t)(file[at + 16] | (file[at + 17] << 8)) + 1;
        CHECK(at + bsize <= file.size() && bsize >= 26 + 5);
        const size_t n = bsize - 26 - 5;
        CHECK(file[at + 18] == 1 && (size_t)(file[at + 19] | (file[at + 20] << 8)) == n);
        CHECK(done + n <= want.size() && memcmp(file.data() + at + 23, want.data() + done, n) == 0);
        CHECK(get32(file.data() + at + bsize - 8) == crc32_of(want.data() + done, n) && get32(file.data() + at + bsize - 4) == n);
        CHECK(n == 0xFF00 || (done + n == want.size() && n > 0));
        done += n; at += bsize;
    }
    CHECK(done == want.size());
    return 0;
}

int main(int argc, char **argv) {
    const int n_files = argc > 1 ? atoi(argv[1]) : 2000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 12345);
    long mismatches = 0;
    for (int f = 0; f < n_files; ++f) if (one_file(f, &mismatches)) return 1;
    printf("files %d, mismatches %ld\n", n_files, mismatches);
    return mismatches ? 1 : 0;
}
