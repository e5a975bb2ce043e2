// The host twin of the BAM device codec with its text stage (amplipy_amd/csrc/amp_bgzf.hip + amp_bamtext.hip, -DAMPBGZF_HOSTSIM) as
// a program, so that it can run under -fsanitize=address,undefined without a sanitizer runtime inside the Python process
// (tests/test_bam_to_sam_twin.py).
//
//   bamtext_fuzz N_FILES [SEED]
// Per file: random BAM records on three references (names of 1 to 40 bytes, 1 to 12 CIGAR ops, 0 to 400 bases, with and without
// qualities, 0 to 70 aux fields of every type, B arrays of up to 300 elements, Z / H bodies of up to 3,000 bytes; unmapped ones and
// ones without CIGAR between them), about one in 300 damaged (a truncated or unknown aux field, a float outside the set, a byte
// outside the printable range in a name, a tag or a string, a quality above 93, an op code above 9, a reference that does not
// exist), in BGZF blocks of random sizes (stored DEFLATE blocks: no zlib here), fed in random runs of blocks; random results per
// row (0 to old + 3 ops, any op, pos from -1, random keep, sometimes a first failing row).  amp_bam_text_check behind every feed,
// amp_bam_format behind it.  Checked: a piece is odd exactly when the plain serial formatter below finds a row it cannot write;
// otherwise its text equals that formatter's (snprintf("%g") for floats); format answers AMP_ESTATE on an odd piece; the guard
// bytes behind the text buffer.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "amp_bgzf.hip"

typedef std::vector<uint8_t> Bytes;
static std::mt19937_64 rng;
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }
static void put32(Bytes &b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
static void put16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static uint32_t get32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint32_t get16(const uint8_t *p) { return p[0] | (p[1] << 8); }

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; tab[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
    return ~c;
}
static void stored(Bytes &out, const uint8_t *p, size_t n) {
    out.push_back(1); put16(out, (uint32_t)n); put16(out, (uint32_t)~n & 0xFFFFu);
    out.insert(out.end(), p, p + n);
}

static const char *NAMES[3] = {"SYN_REF", "chr|2", "a_rather_longer_reference_name.3"};

struct Rec { size_t off; bool row; uint32_t n_cig; };

static uint32_t in_set_float() {
    if (rnd(0, 9) == 0) return (uint32_t)rnd(0, 1) << 31;
    const uint32_t b = rnd(0, 3) ? (uint32_t)rnd(0x38D1B718u, 0x5EFFFFFFu) : (uint32_t)rnd(0x3A000000u, 0x4A000000u);
    return b | ((uint32_t)rnd(0, 1) << 31);
}
static void scalar(Bytes &a, char t) {
    const uint64_t v = rng();
    switch (t) {
    case 'c': case 'C': a.push_back((uint8_t)v); break;
    case 's': case 'S': put16(a, (uint32_t)v); break;
    case 'f': put32(a, in_set_float()); break;
    default: put32(a, rnd(0, 3) ? (uint32_t)v : (uint32_t)rnd(0, 3) - 1u);
    }
}
static void aux_field(Bytes &a) {
    a.push_back((uint8_t)rnd(33, 126)); a.push_back((uint8_t)rnd(33, 126));
    const char t = "AcCsSiIfZHB"[rnd(0, 10)];
    a.push_back((uint8_t)t);
    if (t == 'A') a.push_back((uint8_t)rnd(33, 126));
    else if (t == 'Z' || t == 'H') { const size_t n = rnd(0, 19) ? rnd(0, 30) : rnd(0, 3000); for (size_t k = 0; k < n; ++k) a.push_back((uint8_t)rnd(32, 126)); a.push_back(0); }
    else if (t == 'B') {
        const char st = "cCsSiIf"[rnd(0, 6)];
        const uint32_t n = rnd(0, 9) ? (uint32_t)rnd(0, 12) : (uint32_t)rnd(0, 300);
        a.push_back((uint8_t)st); put32(a, n);
        for (uint32_t k = 0; k < n; ++k) scalar(a, st);
    } else scalar(a, t);
}

static void make_record(Bytes &img, std::vector<Rec> &recs) {
    const uint32_t l_name = (uint32_t)rnd(2, 41), l_seq = rnd(0, 15) ? (uint32_t)rnd(1, 400) : 0;
    const bool unmapped = rnd(0, 19) == 0;
    uint32_t n_cig = rnd(0, 24) == 0 ? 0 : (uint32_t)rnd(1, 12);
    Bytes name, cig, sq, aux;
    for (uint32_t k = 0; k + 1 < l_name; ++k) name.push_back((uint8_t)rnd(33, 126));
    name.push_back(0);
    for (uint32_t k = 0; k < n_cig; ++k) put32(cig, ((uint32_t)rnd(1, 300) << 4) | (uint32_t)rnd(0, 9));
    for (uint32_t k = 0; k < (l_seq + 1) / 2; ++k) sq.push_back((uint8_t)rng());
    const bool no_qual = rnd(0, 7) == 0;
    for (uint32_t k = 0; k < l_seq; ++k) sq.push_back(no_qual ? 0xFF : (uint8_t)rnd(0, 93));
    const uint32_t n_aux = rnd(0, 30) ? (uint32_t)rnd(0, 6) : (uint32_t)rnd(0, 70);
    for (uint32_t k = 0; k < n_aux; ++k) aux_field(aux);
    int32_t ref_id = (int32_t)rnd(0, 3) - 1, next_ref = (int32_t)rnd(0, 3) - 1;
    if (rnd(0, 299) == 0) {                                       // damage
        switch (rnd(0, 9)) {
        case 0: if (!aux.empty()) aux.resize(aux.size() - (size_t)rnd(1, std::min<size_t>(aux.size(), 5))); else aux.push_back('x'); break;
        case 1: aux.push_back('x'); aux.push_back('y'); aux.push_back("QzbB"[rnd(0, 3)]); aux.push_back('d'); put32(aux, 0); break;
        case 2: aux.push_back('x'); aux.push_back('f'); aux.push_back('f'); put32(aux, rnd(0, 1) ? 0x7FC00000u : (uint32_t)rnd(1, 0x38D1B717u)); break;
        case 3: aux.push_back('x'); aux.push_back('f'); aux.push_back('B'); aux.push_back('f'); put32(aux, 2); put32(aux, 0x3F800000u); put32(aux, 0x7F800000u); break;
        case 4: name[(size_t)rnd(0, name.size() - 2)] = (uint8_t)(rnd(0, 1) ? 32 : 200); break;
        case 5: aux.push_back(rnd(0, 1) ? ' ' : 'x'); aux.push_back('y'); aux.push_back('Z'); aux.push_back((uint8_t)(rnd(0, 1) ? 9 : 'k')); aux.push_back(rnd(0, 1) ? 0 : 127); aux.push_back(0); break;
        case 6: if (l_seq && !no_qual) sq[(l_seq + 1) / 2 + (size_t)rnd(0, l_seq - 1)] = (uint8_t)rnd(94, 255); else ref_id = 3; break;
        case 7: if (n_cig) cig[4 * (size_t)rnd(0, n_cig - 1)] |= 0x0A; else next_ref = 7; break;
        case 8: aux.push_back('x'); aux.push_back('y'); aux.push_back('B'); aux.push_back('i'); put32(aux, 0x40000001u); break;
        default: aux.push_back('x'); aux.push_back('y'); aux.push_back('Z'); aux.push_back('n'); aux.push_back('o'); break;
        }
    }
    const uint32_t bs = 32 + l_name + 4 * n_cig + (uint32_t)sq.size() + (uint32_t)aux.size();
    recs.push_back(Rec{img.size(), !unmapped && n_cig > 0, n_cig});
    put32(img, bs);
    put32(img, (uint32_t)ref_id); put32(img, (uint32_t)rnd(0, 29000));
    img.push_back((uint8_t)l_name); img.push_back((uint8_t)rng()); put16(img, 4681); put16(img, n_cig); put16(img, unmapped ? 4 : (uint32_t)rnd(0, 4095) & ~4u);
    put32(img, l_seq); put32(img, (uint32_t)next_ref);
    put32(img, rnd(0, 9) ? (uint32_t)rnd(0, 29000) : (rnd(0, 1) ? 0x7FFFFFFFu : 0xFFFFFFFFu));
    put32(img, rnd(0, 9) ? (uint32_t)((int32_t)rnd(0, 1000) - 500) : (rnd(0, 1) ? 0x80000000u : 0x7FFFFFFFu));
    img.insert(img.end(), name.begin(), name.end()); img.insert(img.end(), cig.begin(), cig.end());
    img.insert(img.end(), sq.begin(), sq.end()); img.insert(img.end(), aux.begin(), aux.end());
}

// ---- AlignmentWriter.write(r, pos=, cigar=) and aux_bam_to_sam, written the plain way; false: a record they would not write (or the
// device is allowed to refuse) ----------------------------------------------------------------------------------------------------
static bool graph(uint8_t c) { return c >= 33 && c <= 126; }
static bool serial_value(std::string &out, const uint8_t *p, char t) {
    char buf[64];
    switch (t) {
    case 'c': snprintf(buf, sizeof buf, "%d", (int)(int8_t)p[0]); break;
    case 'C': snprintf(buf, sizeof buf, "%u", (unsigned)p[0]); break;
    case 's': snprintf(buf, sizeof buf, "%d", (int)(int16_t)get16(p)); break;
    case 'S': snprintf(buf, sizeof buf, "%u", get16(p)); break;
    case 'i': snprintf(buf, sizeof buf, "%d", (int)(int32_t)get32(p)); break;
    case 'I': snprintf(buf, sizeof buf, "%u", get32(p)); break;
    default: {
        const uint32_t b = get32(p);
        float f;
        memcpy(&f, &b, 4);
        const double a = fabs((double)f);
        if (!(f == 0.0f || (a >= 1e-4 && a < 9223372036854775808.0))) return false;
        snprintf(buf, sizeof buf, "%g", (double)f);
    }
    }
    out += buf;
    return true;
}
static size_t width(char t) { return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0; }

static bool serial_line(std::string &out, const uint8_t *rec, int32_t new_pos, uint32_t nn, const uint32_t *cg) {
    const uint32_t bs = get32(rec);
    const uint8_t *c = rec + 4, *end = c + bs;
    const int32_t ref_id = (int32_t)get32(c), next_ref = (int32_t)get32(c + 20), next_pos = (int32_t)get32(c + 24), tlen = (int32_t)get32(c + 28);
    const uint32_t l_name = c[8], mapq = c[9], n_cig = get16(c + 12), flag = get16(c + 14), l_seq = get32(c + 16);
    if (l_name == 0 || ref_id >= 3 || next_ref >= 3) return false;
    std::string s;
    for (uint32_t k = 0; k + 1 < l_name; ++k) { if (!graph(c[32 + k])) return false; s += (char)c[32 + k]; }
    const uint8_t *p = c + 32 + l_name;
    for (uint32_t k = 0; k < n_cig; ++k) if ((get32(p + 4 * k) & 15) > 9) return false;
    p += 4 * n_cig;
    s += "\t" + std::to_string(flag) + "\t" + (ref_id < 0 ? "*" : NAMES[ref_id]) + "\t" + std::to_string((int64_t)new_pos + 1) + "\t" + std::to_string(mapq) + "\t";
    for (uint32_t k = 0; k < nn; ++k) { s += std::to_string(cg[k] >> 4); s += "MIDNSHP=XB??????"[cg[k] & 15]; }
    s += "\t";
    s += next_ref < 0 ? "*" : next_ref == ref_id ? "=" : NAMES[next_ref];
    s += "\t" + std::to_string((int64_t)next_pos + 1) + "\t" + std::to_string(tlen) + "\t";
    if (!l_seq) s += "*";
    for (uint32_t k = 0; k < l_seq; ++k) s += "=ACMGRSVTWYHKDBN"[(p[k >> 1] >> ((k & 1) ? 0 : 4)) & 15];
    p += (l_seq + 1) / 2;
    s += "\t";
    if (!l_seq || p[0] == 0xFF) s += "*";
    else for (uint32_t k = 0; k < l_seq; ++k) { if (p[k] > 93) return false; s += (char)(p[k] + 33); }
    p += l_seq;
    while (p < end) {
        if (end - p < 3 || !graph(p[0]) || !graph(p[1])) return false;
        const char t = (char)p[2];
        s += "\t"; s += (char)p[0]; s += (char)p[1]; s += ":";
        p += 3;
        if (t == 'A') { if (p >= end || !graph(p[0])) return false; s += "A:"; s += (char)*p++; }
        else if (width(t)) {
            if ((size_t)(end - p) < width(t)) return false;
            s += t == 'f' ? "f:" : "i:";
            if (!serial_value(s, p, t)) return false;
            p += width(t);
        } else if (t == 'Z' || t == 'H') {
            s += t; s += ":";
            while (p < end && *p) { if (*p < 32 || *p > 126) return false; s += (char)*p++; }
            if (p >= end) return false;
            ++p;
        } else if (t == 'B') {
            if (end - p < 5 || !width((char)p[0])) return false;
            const char st = (char)p[0];
            const uint64_t n = get32(p + 1);
            p += 5;
            if (n * width(st) > (uint64_t)(end - p)) return false;
            s += "B:"; s += st;
            for (uint64_t k = 0; k < n; ++k, p += width(st)) { s += ","; if (!serial_value(s, p, st)) return false; }
        } else return false;
    }
    out += s + "\n";
    return true;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "file %d: %s (line %d)\n", file_no, #cond, __LINE__); return 1; } } while (0)

static long n_pieces = 0, n_odd = 0, guard_hits = 0;

static int one_file(int file_no, long *mismatches) {
    Bytes img;
    std::vector<Rec> recs;
    const int n_rec = (int)rnd(0, 1) ? (int)rnd(1, 1200) : (int)rnd(0, 40);
    for (int i = 0; i < n_rec; ++i) make_record(img, recs);
    std::vector<amp_bam_block> blocks;
    Bytes comp;
    for (size_t at = 0; at < img.size();) {
        const size_t n = std::min<size_t>(img.size() - at, (size_t)rnd(1, rnd(0, 3) ? 16000 : 700));
        const uint32_t in_off = (uint32_t)comp.size();
        stored(comp, img.data() + at, n);
        blocks.push_back(amp_bam_block{in_off, (uint32_t)comp.size() - in_off, (uint32_t)n, crc32_of(img.data() + at, n)});
        at += n;
    }
    amp_bam *s = nullptr;
    CHECK(amp_bam_create(nullptr, &s) == 0);
    CHECK(amp_bam_set_references(s, 3, NAMES) == 0);
    const int32_t min_length = (int32_t)rnd(0, 60), inp = (int32_t)rnd(0, 1);
    int64_t rec_base = 0;
    size_t next_rec = 0;
    for (size_t k0 = 0; k0 < blocks.size();) {
        const size_t k1 = std::min(blocks.size(), k0 + (size_t)rnd(1, rnd(0, 2) ? 3 : 25));
        std::vector<amp_bam_block> piece(blocks.begin() + k0, blocks.begin() + k1);
        const uint32_t base = piece[0].in_off;
        for (auto &b : piece) b.in_off -= base;
        const size_t n_comp = blocks[k1 - 1].in_off + blocks[k1 - 1].in_len - base;
        Bytes cp(comp.begin() + base, comp.begin() + base + n_comp);
        amp_bam_info info;
        CHECK(amp_bam_feed(s, cp.data(), (int64_t)n_comp, piece.data(), (int64_t)piece.size(), k0 == 0 ? 0 : -1, 3, rec_base, &info) == 0);
        CHECK(info.n_refused == 0 && !info.bad_record);
        rec_base += info.n_records;
        std::vector<size_t> rows;
        for (int64_t i = 0; i < info.n_records; ++i, ++next_rec) if (recs[next_rec].row) rows.push_back(next_rec);
        CHECK((int64_t)rows.size() == info.n_rows);
        k0 = k1;
        const size_t n = rows.size();
        std::vector<int32_t> new_pos(n), ref_len(n);
        std::vector<uint32_t> ncig(n), new_cig;
        std::vector<uint8_t> flags(n);
        std::vector<size_t> slot(n);
        size_t cig_off = 0;
        for (size_t r = 0; r < n; ++r) { slot[r] = cig_off + 3 * r; cig_off += recs[rows[r]].n_cig; }
        new_cig.assign(cig_off + 3 * n + 1, 0);
        for (size_t r = 0; r < n; ++r) {
            new_pos[r] = (int32_t)rnd(0, 9) ? (int32_t)rnd(0, 1 << 29) - (int32_t)rnd(0, 1) : (int32_t)rnd(0, 1) - 1;
            ref_len[r] = (int32_t)rnd(0, 120); flags[r] = (uint8_t)rnd(0, 7);
            ncig[r] = (uint32_t)rnd(0, recs[rows[r]].n_cig + 3);
            for (uint32_t k = 0; k < ncig[r]; ++k) new_cig[slot[r] + k] = ((uint32_t)rnd(0, rnd(0, 3) ? 500 : (1 << 28) - 1) << 4) | (uint32_t)rnd(0, 9);
        }
        const int64_t first_bad = n && rnd(0, 14) == 0 ? (int64_t)rnd(0, n - 1) : -1;
        amp_bam_text_info ci, fi;
        CHECK(amp_bam_text_check(s, &ci) == 0);
        CHECK(ci.waits == (n ? 1 : 0));
        if (n) CHECK(amp_bam_twin_set_trim(s, new_pos.data(), ncig.data(), new_cig.data(), ref_len.data(), flags.data(), first_bad) == 0);
        // the serial side: every row's line (a row that cannot be written makes the piece odd), the kept ones joined
        std::string want, line;
        int64_t serial_odd = -1, kept = 0;
        for (size_t r = 0; r < n; ++r) {
            line.clear();
            if (!serial_line(line, img.data() + recs[rows[r]].off, new_pos[r], ncig[r], new_cig.data() + slot[r])) { if (serial_odd < 0) serial_odd = (int64_t)r; continue; }
            if (first_bad >= 0 && (int64_t)r >= first_bad) continue;
            if (!(ref_len[r] >= min_length && ((flags[r] & 3) || inp))) continue;
            want += line; ++kept;
        }
        ++n_pieces;
        if (ci.first_odd_row != serial_odd) { ++*mismatches; fprintf(stderr, "file %d: first odd row %lld, the serial formatter's %lld\n", file_no, (long long)ci.first_odd_row, (long long)serial_odd); continue; }
        Bytes got(serial_odd < 0 ? want.size() : 16);                     // (exactly the size: a write behind it is a finding)
        if (ci.first_odd_row >= 0) {
            ++n_odd;
            CHECK(ci.odd_reason >= 1 && ci.odd_reason <= 8);
            CHECK(amp_bam_format(s, min_length, inp, got.data(), (int64_t)got.size(), &fi) == AMP_ESTATE);
            continue;
        }
        if (!want.empty() && rnd(0, 7) == 0) {                           // a buffer that is too short names the size and writes nothing
            CHECK(amp_bam_format(s, min_length, inp, got.data(), (int64_t)want.size() - 1, &fi) == AMP_EOVERFLOW);
            CHECK(fi.n_bytes == (int64_t)want.size());
        }
        CHECK(amp_bam_format(s, min_length, inp, got.data(), (int64_t)got.size(), &fi) == 0);
        CHECK(fi.waits <= 2 && fi.n_rows_written == kept && fi.n_bytes == (int64_t)want.size());
        if (amp_bam_twin_text_guard(s) != 0) ++guard_hits;
        if (!want.empty() && memcmp(got.data(), want.data(), want.size()) != 0) {
            ++*mismatches;
            size_t at = 0;
            while (got[at] == (uint8_t)want[at]) ++at;
            fprintf(stderr, "file %d: text differs at byte %zu of %zu: ...%.60s\n", file_no, at, want.size(), want.c_str() + (at > 30 ? at - 30 : 0));
        }
    }
    amp_bam_destroy(s);
    return 0;
}

int main(int argc, char **argv) {
    const int n_files = argc > 1 ? atoi(argv[1]) : 2000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 12345);
    long mismatches = 0;
    for (int f = 0; f < n_files; ++f) if (one_file(f, &mismatches)) return 1;
    printf("files %d, pieces %ld, odd %ld, mismatches %ld, guard hits %ld\n", n_files, n_pieces, n_odd, mismatches, guard_hits);
    return mismatches || guard_hits ? 1 : 0;
}
