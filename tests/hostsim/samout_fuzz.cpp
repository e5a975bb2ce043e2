// The host twin of the SAM-text device codec with BAM output (amplipy_amd/csrc/amp_sam.hip, -DAMPSAM_HOSTSIM)
// as a program, so that it can run under -fsanitize=address,undefined without a sanitizer runtime inside the Python process
// (tests/test_sam_to_bam_twin.py).
//
//   samout_fuzz N_RUNS [SEED]
// Per run: random SAM lines (names of 1 to 40 bytes, '*' and named references, 0 to 10 CIGAR ops, 0 to 300 bases, QUAL given or '*',
// 0 to 8 aux fields of every type, Z strings of up to 4,000 bytes, B arrays of up to 300 elements; unmapped ones, ones without
// CIGAR and lines that are no records between them; now and then a damaged aux field) cut into random chunks of whole lines;
// random results per row (0 to old + 3 ops, any op, pos from -1, random keep, sometimes a first failing row); amp_sam_encode
// behind every chunk that is not odd, the final one at random with the last chunk or as a bare flush through
// amp_sam_encode_bytes.
// Checked: a chunk is odd, or the bytes of its encode equal a plain serial encode of the same lines and results written below
// (strtol, strtod and a cast where the lane functions have their own parsers); the framed blocks (header, BSIZE, stored payload
// = the stream's chunk, CRC-32, ISIZE, 0xFF00 bytes in all but the last); the guard bytes behind every buffer.
#include <stdio.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "amp_sam.hip"

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
static int stored_deflater(const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len) {
    for (int64_t k = 0; k * block_bytes < n_bytes; ++k) {
        const int64_t n = n_bytes - k * block_bytes < block_bytes ? n_bytes - k * block_bytes : block_bytes;
        if (n + 5 > out_room) { out_len[k] = 0; continue; }
        uint8_t *o = out + k * out_stride;
        o[0] = 1; o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8);
        memcpy(o + 5, in + k * block_bytes, (size_t)n);
        out_len[k] = (uint32_t)n + 5;
    }
    return 0;
}

// ---- the lines ---------------------------------------------------------------------------------------------------------------------
static const char *REFS[2] = {"SYN_REF", "OTHER"};
struct Row { std::string line; bool row; std::vector<uint32_t> cig; };

static std::string float_text() {
    std::string s = rnd(0, 3) == 0 ? "-" : "";
    const int nd = (int)rnd(1, 15), cutp = (int)rnd(1, nd);
    std::string d;
    for (int k = 0; k < nd; ++k) d += (char)('0' + rnd(0, 9));
    s += d.substr(0, cutp);
    if (cutp < nd) s += "." + d.substr(cutp);
    const int p = (int)rnd(0, 44) - 22 + (nd - cutp);              // the power of ten behind the fold: within +-22
    if (p != 0 || rnd(0, 1)) s += std::string("e") + (p >= 0 && rnd(0, 3) == 0 ? "+" : "") + std::to_string(p);
    else if (nd - cutp > 22) s = "1";
    return s;
}

static std::string int_text(int64_t lo, int64_t hi) {
    static const int64_t edges[] = {-129, -128, 127, 128, 255, 256, 32767, 32768, 65535, 65536, -2147483648ll, 4294967295ll, 0, -1, -32768, -32769, 2147483647ll, 2147483648ll};
    for (int tries = 0; tries < 4; ++tries) { const int64_t e = edges[rnd(0, 17)]; if (e >= lo && e <= hi) return std::to_string(e); }
    const int64_t span = hi - lo;
    return std::to_string(lo + (int64_t)(rng() % ((uint64_t)span + 1)));
}

static std::string aux_field() {
    std::string f;
    f += (char)rnd(33, 126); f += (char)rnd(33, 126);
    const char type = "AifZHB"[rnd(0, 5)];
    f += ':'; f += type; f += ':';
    if (type == 'A') f += (char)rnd(33, 126);
    else if (type == 'i') f += int_text(-2147483648ll, 4294967295ll);
    else if (type == 'f') f += float_text();
    else if (type == 'Z' || type == 'H') { const size_t n = rnd(0, 99) == 0 ? rnd(1000, 4000) : rnd(0, rnd(0, 3) ? 20 : 200); for (size_t k = 0; k < n; ++k) f += (char)rnd(32, 126); }
    else {
        static const int64_t lo[6] = {-128, 0, -32768, 0, -2147483648ll, 0}, hi[6] = {127, 255, 32767, 65535, 2147483647ll, 4294967295ll};
        const int sub = (int)rnd(0, 6);
        f += "cCsSiIf"[sub];
        const size_t n = rnd(0, 49) == 0 ? 300 : rnd(0, 12);
        for (size_t k = 0; k < n; ++k) { f += ','; f += sub == 6 ? float_text() : int_text(lo[sub], hi[sub]); }
    }
    return f;
}

static Row make_line() {
    Row r;
    const uint64_t kind = rnd(0, 39);
    if (kind == 0) { r.line = "three\tfields\tonly"; r.row = false; return r; }
    if (kind == 1) { r.line = ""; r.row = false; return r; }
    std::string name;
    for (size_t k = 0, n = rnd(0, 30) == 0 ? 254 : rnd(1, 40); k < n; ++k) name += (char)rnd(33, 126);
    if (name[0] == '@') name[0] = 'a';
    const bool unmapped = rnd(0, 19) == 0, nocig = rnd(0, 24) == 0;
    const uint32_t flag = (uint32_t)(rnd(0, 3) * 16 + rnd(0, 1) * 1024 + (unmapped ? 4 : 0));
    std::string cig;
    if (!nocig) for (size_t k = 0, n = rnd(1, 10); k < n; ++k) { const uint32_t len = (uint32_t)rnd(1, 300), op = (uint32_t)rnd(0, 8); r.cig.push_back((len << 4) | op); cig += std::to_string(len) + "MIDNSHP=X"[op]; }
    else cig = "*";
    const int rn = rnd(0, 9) == 0 ? -1 : (int)rnd(0, 1);
    const uint64_t nx = rnd(0, 3);                              // '=', '*', the other name, '*'
    std::string rnext = nx == 0 && rn >= 0 ? "=" : nx == 2 && rn >= 0 ? REFS[1 - rn] : "*";
    const size_t L = rnd(0, 14) == 0 ? 0 : rnd(1, 300);
    std::string seq, qual;
    for (size_t k = 0; k < L; ++k) seq += "ACGTNacgtnRYKMSWBDHV=XZ.-"[rnd(0, rnd(0, 5) ? 4 : 24)];
    if (L && rnd(0, 5)) for (size_t k = 0; k < L; ++k) qual += (char)rnd(33, 126); else qual = "*";
    if (!L) seq = "*";
    r.line = name + "\t" + std::to_string(flag) + "\t" + (rn < 0 ? "*" : REFS[rn]) + "\t" + std::to_string(rnd(0, 29000)) + "\t" + std::to_string(rnd(0, 255)) + "\t" + cig +
             "\t" + rnext + "\t" + std::to_string(rnd(0, 29000)) + "\t" + std::to_string((int64_t)rnd(0, 1000) - 500) + "\t" + seq + "\t" + qual;
    for (size_t k = 0, n = rnd(0, 19) == 0 ? 40 : rnd(0, 8); k < n; ++k) r.line += "\t" + aux_field();
    r.row = !unmapped && !nocig;
    // a damaged aux field: a byte of the aux part replaced, removed or doubled
    if (rnd(0, 29) == 0) {
        size_t tabs = 0, from = 0;
        for (size_t k = 0; k < r.line.size(); ++k) if (r.line[k] == '\t' && ++tabs == 11) { from = k + 1; break; }
        if (from && from < r.line.size()) {
            const size_t at = rnd(from, r.line.size() - 1);
            const uint64_t what = rnd(0, 2);
            if (what == 0) r.line[at] = ":,.e-+0A9\tZ x"[rnd(0, 12)];
            else if (what == 1) r.line.erase(at, 1);
            else r.line.insert(at, 1, r.line[at]);
        }
    }
    return r;
}

// ---- aux_sam_to_bam and AlignmentWriter.write, written the plain way (for lines the codec does not call odd) --------------------------
static std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) { const size_t k = s.find(sep, at); if (k == std::string::npos) { out.push_back(s.substr(at)); return out; } out.push_back(s.substr(at, k - at)); at = k + 1; }
}
static void put_sized(Bytes &b, int64_t x, int bytes) { for (int k = 0; k < bytes; ++k) b.push_back((uint8_t)((uint64_t)x >> (8 * k))); }
static void put_f32(Bytes &b, const std::string &v) { const float f = (float)strtod(v.c_str(), nullptr); uint32_t w; memcpy(&w, &f, 4); put32(b, w); }

static void serial_aux(Bytes &b, const std::string &f) {
    b.push_back((uint8_t)f[0]); b.push_back((uint8_t)f[1]);
    const char type = f[3];
    const std::string v = f.substr(5);
    if (type == 'A') { b.push_back('A'); b.push_back((uint8_t)v[0]); }
    else if (type == 'i') {
        const long long x = strtoll(v.c_str(), nullptr, 10);
        static const long long lo[6] = {-128, 0, -32768, 0, -2147483648ll, 0}, hi[6] = {127, 255, 32767, 65535, 2147483647ll, 4294967295ll};
        for (int k = 0; k < 6; ++k) if (x >= lo[k] && x <= hi[k]) { b.push_back((uint8_t)"cCsSiI"[k]); put_sized(b, x, k < 2 ? 1 : k < 4 ? 2 : 4); break; }
    }
    else if (type == 'f') { b.push_back('f'); put_f32(b, v); }
    else if (type == 'Z' || type == 'H') { b.push_back((uint8_t)type); b.insert(b.end(), v.begin(), v.end()); b.push_back(0); }
    else {
        const char sub = v[0];
        std::vector<std::string> vals;
        if (v.size() > 1) vals = split(v.substr(2), ',');
        b.push_back('B'); b.push_back((uint8_t)sub); put32(b, (uint32_t)vals.size());
        const int bytes = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : 4;
        for (const std::string &x : vals) { if (sub == 'f') put_f32(b, x); else put_sized(b, strtoll(x.c_str(), nullptr, 10), bytes); }
    }
}

static int ref_id(const std::string &n) { return n == REFS[0] ? 0 : n == REFS[1] ? 1 : -1; }

static void serial_record(Bytes &out, const std::string &line, int32_t new_pos, const std::vector<uint32_t> &cg) {
    const std::vector<std::string> f = split(line, '\t');
    Bytes r;
    const int rn = ref_id(f[2]), rx = f[6] == "=" ? rn : ref_id(f[6]);
    const uint32_t L = f[9] == "*" ? 0 : (uint32_t)f[9].size();
    int64_t rlen = 0;
    for (uint32_t w : cg) { const uint32_t op = w & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4; }
    int64_t beg = new_pos > 0 ? new_pos : 0, end = (int64_t)new_pos + (rlen ? rlen : 1);
    if (end < 1) end = 1;
    --end;
    uint32_t bin = 0;
    if (beg >> 14 == end >> 14) bin = (uint32_t)(4681 + (beg >> 14));
    else if (beg >> 17 == end >> 17) bin = (uint32_t)(585 + (beg >> 17));
    else if (beg >> 20 == end >> 20) bin = (uint32_t)(73 + (beg >> 20));
    else if (beg >> 23 == end >> 23) bin = (uint32_t)(9 + (beg >> 23));
    else if (beg >> 26 == end >> 26) bin = (uint32_t)(1 + (beg >> 26));
    put32(r, (uint32_t)rn); put32(r, (uint32_t)new_pos);
    r.push_back((uint8_t)(f[0].size() + 1)); r.push_back((uint8_t)atoi(f[4].c_str())); put16(r, bin); put16(r, (uint32_t)cg.size()); put16(r, (uint32_t)atoi(f[1].c_str()));
    put32(r, L); put32(r, (uint32_t)rx); put32(r, (uint32_t)(atoi(f[7].c_str()) - 1)); put32(r, (uint32_t)atoi(f[8].c_str()));
    r.insert(r.end(), f[0].begin(), f[0].end()); r.push_back(0);
    for (uint32_t w : cg) put32(r, w);
    static const char *NT = "=ACMGRSVTWYHKDBN";
    std::vector<uint8_t> codes;
    for (uint32_t k = 0; k < L; ++k) {
        uint8_t c = 15;
        for (int j = 0; j < 16; ++j) if (f[9][k] == NT[j] || f[9][k] == (char)tolower(NT[j])) c = (uint8_t)j;
        codes.push_back(c);
    }
    if (L & 1) codes.push_back(0);
    for (size_t k = 0; k < codes.size(); k += 2) r.push_back((uint8_t)((codes[k] << 4) | codes[k + 1]));
    for (uint32_t k = 0; k < L; ++k) r.push_back(f[10] == "*" ? 0xFF : (uint8_t)(f[10][k] - 33));
    for (size_t k = 11; k < f.size(); ++k) serial_aux(r, f[k]);
    put32(out, (uint32_t)r.size());
    out.insert(out.end(), r.begin(), r.end());
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "run %d: %s (line %d)\n", run_no, #cond, __LINE__); return 1; } } while (0)

static long n_chunks = 0, n_odd = 0, n_guard = 0;

static int one_run(int run_no, long *mismatches) {
    std::vector<Row> rows;
    for (int i = 0, n = (int)rnd(0, 9) ? (int)rnd(1, 120) : 0; i < n; ++i) rows.push_back(make_line());
    amp_sam *s = nullptr;
    CHECK(amp_sam_create(nullptr, &s) == 0);
    CHECK(amp_sam_set_references(s, 2, REFS) == 0);
    CHECK(amp_sam_set_output(s, AMP_SAM_OUT_BAM) == 0);
    CHECK(amp_sam_twin_set_deflater(s, stored_deflater) == 0);
    const int32_t min_length = (int32_t)rnd(0, 60), inp = (int32_t)rnd(0, 1);
    Bytes want, got, file;
    bool flushed = false, stopped = false;
    for (size_t l0 = 0; l0 < rows.size() && !stopped;) {
        const size_t l1 = std::min(rows.size(), l0 + (size_t)rnd(1, rnd(0, 2) ? 6 : 40));
        const bool last = l1 == rows.size();
        std::string text;
        std::vector<size_t> mine;
        for (size_t k = l0; k < l1; ++k) { text += rows[k].line + (rnd(0, 19) == 0 ? "\r\n" : "\n"); if (rows[k].row) mine.push_back(k); }
        l0 = l1;
        Bytes chunk(text.begin(), text.end());                   // (exactly the chunk: a read behind it is a finding)
        amp_sam_info info;
        CHECK(amp_sam_parse(s, chunk.data(), (int64_t)chunk.size(), &info) == 0);
        ++n_chunks;
        if (info.first_odd_line >= 0) { ++n_odd; continue; }
        CHECK(info.n_rows == (int64_t)mine.size());
        const size_t n = mine.size();
        std::vector<int32_t> new_pos(n + 1), ref_len(n + 1);
        std::vector<uint32_t> ncig(n + 1), new_cig;
        std::vector<uint8_t> flags(n + 1), status(n + 1, 0);
        std::vector<size_t> slot(n);
        size_t cig_off = 0;
        for (size_t r = 0; r < n; ++r) { slot[r] = cig_off + 3 * r; cig_off += rows[mine[r]].cig.size(); }
        CHECK((int64_t)cig_off == info.n_cig);
        new_cig.assign(cig_off + 3 * n + 1, 0);
        for (size_t r = 0; r < n; ++r) {
            const uint32_t old = (uint32_t)rows[mine[r]].cig.size();
            new_pos[r] = (int32_t)rnd(0, 9) ? (int32_t)rnd(0, 1 << 29) - (int32_t)rnd(0, 1) : (int32_t)rnd(0, 1) - 1;
            ref_len[r] = (int32_t)rnd(0, 120); flags[r] = (uint8_t)rnd(0, 7);
            ncig[r] = (uint32_t)rnd(0, old + 3);
            for (uint32_t k = 0; k < ncig[r]; ++k) new_cig[slot[r] + k] = ((uint32_t)rnd(0, 1 << 20) << 4) | (uint32_t)(rnd(0, 3) ? rnd(0, 8) : rnd(4, 6));
        }
        const int64_t first_bad = n && rnd(0, 14) == 0 ? (int64_t)rnd(0, n - 1) : -1;
        if (first_bad >= 0) status[(size_t)first_bad] = 6;
        if (n) {
            int64_t bad = -2; uint8_t st = 0;
            CHECK(amp_sam_twin_set_results(s, new_pos.data(), ncig.data(), new_cig.data(), ref_len.data(), flags.data(), status.data(), &bad, &st) == 0);
            CHECK(bad == first_bad);
        }
        const size_t want0 = want.size();
        for (size_t r = 0; r < n; ++r) {
            if (first_bad >= 0 && (int64_t)r >= first_bad) break;
            if (!(ref_len[r] >= min_length && ((flags[r] & 3) || inp))) continue;
            serial_record(want, rows[mine[r]].line, new_pos[r], std::vector<uint32_t>(new_cig.begin() + slot[r], new_cig.begin() + slot[r] + ncig[r]));
        }
        const bool final = last && rnd(0, 1) && first_bad < 0;
        amp_bam_out_info oi;
        CHECK(amp_sam_encode(s, min_length, inp, final ? 1 : 0, &oi) == 0);
        if (amp_sam_twin_guards(s)) ++n_guard;
        CHECK(oi.waits == 1 && oi.n_blocks_host == 0);
        Bytes part((size_t)(oi.stream_bytes - oi.carry_in));                     // (exactly the size: a write behind it is a finding)
        CHECK(amp_sam_stream_to_host(s, oi.carry_in, (int64_t)part.size(), part.data()) == 0);
        if (part.size() != want.size() - want0 || (part.size() && memcmp(part.data(), want.data() + want0, part.size()) != 0)) {
            ++*mismatches;
            fprintf(stderr, "run %d: a chunk's records differ (%zu bytes, %zu wanted)\n%s", run_no, part.size(), want.size() - want0, text.c_str());
            amp_sam_destroy(s);
            return 0;
        }
        got.insert(got.end(), part.begin(), part.end());
        Bytes fb((size_t)oi.file_bytes);
        CHECK(amp_sam_encoded_to_host(s, fb.data(), (int64_t)fb.size()) == 0);
        file.insert(file.end(), fb.begin(), fb.end());
        flushed = final;
        if (first_bad >= 0) stopped = true;
    }
    if (!flushed && !stopped) {
        amp_bam_out_info oi;
        CHECK(amp_sam_encode_bytes(s, nullptr, 0, 1, &oi) == 0);
        CHECK(oi.n_rows_written == 0 && oi.carry_out == 0 && oi.n_blocks <= 1);
        Bytes fb((size_t)oi.file_bytes);
        CHECK(amp_sam_encoded_to_host(s, fb.data(), (int64_t)fb.size()) == 0);
        file.insert(file.end(), fb.begin(), fb.end());
        if (amp_sam_twin_guards(s)) ++n_guard;
    }
    amp_sam_destroy(s);
    // the framed blocks: stored payloads that give the stream back, chunk by chunk (behind a failing row: its whole blocks)
    const size_t upto = stopped ? want.size() - want.size() % 0xFF00 : want.size();
    size_t at = 0, done = 0;
    while (at < file.size()) {
        const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        CHECK(at + 26 <= file.size() && memcmp(file.data() + at, hdr, 16) == 0);
        const size_t bsize = (size_t)(file[at + 16] | (file[at + 17] << 8)) + 1;
        CHECK(at + bsize <= file.size() && bsize >= 26 + 5);
        const size_t n = bsize - 26 - 5;
        CHECK(file[at + 18] == 1 && (size_t)(file[at + 19] | (file[at + 20] << 8)) == n);
        CHECK(done + n <= upto && memcmp(file.data() + at + 23, want.data() + done, n) == 0);
        CHECK(get32(file.data() + at + bsize - 8) == crc32_of(want.data() + done, n) && get32(file.data() + at + bsize - 4) == n);
        CHECK(n == 0xFF00 || (done + n == want.size() && n > 0));
        done += n; at += bsize;
    }
    CHECK(done == upto);
    return 0;
}

int main(int argc, char **argv) {
    const int n_runs = argc > 1 ? atoi(argv[1]) : 2000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 12345);
    long mismatches = 0;
    for (int f = 0; f < n_runs; ++f) if (one_run(f, &mismatches)) return 1;
    printf("runs %d, mismatches %ld, guards %ld chunks=%ld odd=%ld\n", n_runs, mismatches, n_guard, n_chunks, n_odd);
    return mismatches || n_guard ? 1 : 0;
}
