// amp_bamtext.hpp -- what one lane does when a kept BAM record becomes a line of SAM text on the device (amp_bamtext.hip,
// DESIGN.md section 14): the verdict on a record (would the Python codec write exactly these bytes?), the length of its line,
// the decimal fields, '%g' of a float32 in integers, the aux fields binary to text, bases and qualities eight at a time.  The
// bytes are bamio.AlignmentWriter.write's (mode "w") with aux_bam_to_sam: out_aln.write at AmpliPy.py:911.
//
// Plain C++ on raw pointers: compiles for HIP (BGZ_HD = __host__ __device__) and with any host compiler, sanitizers included
// (tests/hostsim/bamtext_fuzz.cpp).  A function writes exactly the bytes it names and reads exactly the record it is given.
// Nothing here keeps an array in a lane and nothing is chosen from a table by a chain of selects: the few constants are packed
// into 64-bit words and shifted out.  No floating-point arithmetic anywhere.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "amp_bamout.hpp"

// the reasons of amplihip.h, for a unit that has not seen it
#ifndef AMP_BAM_ODD_NONE
#define AMP_BAM_ODD_NONE 0
#define AMP_BAM_ODD_QNAME 1
#define AMP_BAM_ODD_REF 2
#define AMP_BAM_ODD_CIGAR_OP 3
#define AMP_BAM_ODD_QUAL 4
#define AMP_BAM_ODD_AUX_TYPE 5
#define AMP_BAM_ODD_AUX_TRUNC 6
#define AMP_BAM_ODD_AUX_CHAR 7
#define AMP_BAM_ODD_AUX_FLOAT 8
#endif

namespace ampbamtext {

using ampbamout::o_load8;
using ampbamout::o_rd16;
using ampbamout::o_rd32;
using ampbamout::o_store8;
using ampbamout::wave_copy;

enum : uint32_t { TEXT_WAVE = 64u };

// counters of a check / a format, in device memory
enum { TCTL_ODD = 0,       // min over odd rows of (row << 8 | reason); all ones: none
       TCTL_ROWS,          // rows written
       TCTL_WORDS = 4 };

// every pointer of the text stage: device memory in the library, host memory in the twin
struct Text {
    const int32_t *new_pos; const uint32_t *new_ncig, *new_cig; const int32_t *ref_len; const uint8_t *trim_flags;
    int64_t n_rows, good_rows;
    int32_t min_length, include_no_primer, n_names, pad;
    const uint8_t *names; const uint32_t *name_off;      // the @SQ names back to back, name r = [name_off[r], name_off[r + 1])
    uint32_t *row_tsz, *row_asz;       // per row: the line without POS and CIGAR; its aux fields with their tabs
    uint64_t *row_off;                 // [n_rows + 1]: line sizes, then their exclusive sum
    uint8_t *out;
    unsigned long long *tctl;
};

// What an amp_bam keeps for the text stage between its calls.  The buffers grow to the largest piece and are not freed during a run.
struct State {
    uint8_t *names = nullptr, *name_off = nullptr, *arena = nullptr, *out = nullptr;
    size_t cap_arena = 0, cap_out = 0;
    int64_t arena_rows = 0;
    int32_t n_names = -1;              // -1: amp_bam_set_references has not run
    bool checked = false;              // the last feed went through amp_bam_text_check
    int64_t first_odd = -1;
    int32_t odd_reason = 0;
    int64_t guard_at = 0, guard_len = 0;   // (the twin's: bytes behind the text that nothing may write)
    unsigned long long h_tctl[TCTL_WORDS];
};

// ---- decimal --------------------------------------------------------------------------------------------------------------------------
BGZ_HD uint32_t t_ndigits(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
BGZ_HD uint32_t t_nint(int64_t v) { return v < 0 ? 1u + t_ndigits(0ull - (uint64_t)v) : t_ndigits((uint64_t)v); }
BGZ_HD uint32_t t_put_uint(uint8_t *p, uint64_t v) {
    const uint32_t n = t_ndigits(v);
    for (uint32_t k = n; k-- > 0;) { p[k] = (uint8_t)('0' + v % 10); v /= 10; }
    return n;
}
BGZ_HD uint32_t t_put_int(uint8_t *p, int64_t v) {
    if (v >= 0) return t_put_uint(p, (uint64_t)v);
    *p = '-';
    return 1u + t_put_uint(p + 1, 0ull - (uint64_t)v);
}
BGZ_HD bool t_graph(uint32_t c) { return c >= 33u && c <= 126u; }
BGZ_HD uint8_t t_cigar_char(uint32_t op) {                       // "MIDNSHP=XB"
    const uint64_t lo = 0x3D504853'4E44494Dull;                  // "MIDNSHP="
    return op < 8u ? (uint8_t)(lo >> (8u * op)) : op == 8u ? (uint8_t)'X' : (uint8_t)'B';
}
BGZ_HD uint8_t t_base_char(uint32_t nib) {                       // "=ACMGRSVTWYHKDBN"
    const uint64_t lo = 0x56535247'4D43413Dull, hi = 0x4E42444B'48595754ull;
    return (uint8_t)(((nib & 8u) ? hi : lo) >> (8u * (nib & 7u)));
}

// ---- '%g' % v of a float32 ---------------------------------------------------------------------------------------------------------
// The values the device formats: +-0, and every finite v with 1e-4 <= |v| < 2^63 (the float32 behind 0x38D1B717, which is
// 9.99999975e-05, up to 0x5EFFFFFF).  Everything else -- nan, inf, subnormals, smaller and larger values -- is odd.
BGZ_HD bool g_in_set(uint32_t bits) {
    const uint32_t a = bits & 0x7FFFFFFFu;
    return a == 0u || (a >= 0x38D1B718u && a < 0x5F000000u);
}
// six significant digits D in [10^5, 10^6) and the decimal exponent X of an in-set value that is not zero: v = m * 2^e with
// m < 2^24; D = round-half-even(P / Q) with P / Q = |v| * 10^(5 - X), both exact in unsigned 64-bit integers (P < 2^63, Q < 2^44
// for the true X; the trial with X one too low multiplies P by ten only where it is below 2^48)
struct GDigits { uint32_t D; int32_t X; };
BGZ_HD void g_ratio(uint64_t m, int32_t e, int32_t X, uint64_t *P, uint64_t *Q) {
    const int32_t s = 5 - X;
    uint64_t p = m, q = 1;
    if (s >= 0) {
        for (int32_t k = 0; k < s; ++k) p *= 5u;
        if (e + s >= 0) p <<= (uint32_t)(e + s); else q <<= (uint32_t)(-e - s);
    } else {
        for (int32_t k = 0; k < -s; ++k) q *= 10u;
        if (e >= 0) p <<= (uint32_t)e; else q <<= (uint32_t)(-e);
    }
    *P = p; *Q = q;
}
BGZ_HD GDigits g_digits(uint32_t bits) {
    const uint32_t a = bits & 0x7FFFFFFFu;
    const uint64_t m = (a & 0x7FFFFFu) | 0x800000u;
    const int32_t be = (int32_t)(a >> 23) - 127, e = be - 23;
    int32_t X = (be * 1233) >> 12;                               // floor(be * log10(2)) or one below it, for be in [-14, 62]
    uint64_t P, Q;
    g_ratio(m, e, X, &P, &Q);
    if (P / Q >= 1000000u) { ++X; g_ratio(m, e, X, &P, &Q); }
    uint64_t d = P / Q;
    const uint64_t r = P - d * Q;
    if (2 * r > Q || (2 * r == Q && (d & 1u))) ++d;
    if (d >= 1000000u) { d = 100000u; ++X; }
    return GDigits{(uint32_t)d, X};
}
// the text: its length; with p, written there.  Trailing zeros stripped; exponent form for X < -4 or X >= 6, two exponent digits
BGZ_HD uint32_t g_text(uint32_t bits, uint8_t *p) {
    uint32_t n = 0;
    if (bits >> 31) { if (p) p[n] = '-'; ++n; }
    if ((bits & 0x7FFFFFFFu) == 0u) { if (p) p[n] = '0'; return n + 1; }
    const GDigits g = g_digits(bits);
    uint32_t D = g.D, nd = 6;
    while (nd > 1 && D % 10u == 0u) { D /= 10u; --nd; }          // nd significant digits in D
    const int32_t X = g.X;
    if (X >= 6) {                                                // d[.ddd]e+XX
        const uint32_t len = (nd > 1 ? nd + 1 : 1) + 4;
        if (p) {
            uint8_t *q = p + n;
            uint32_t v = D;
            for (uint32_t k = nd; k-- > 1;) { q[k + 1] = (uint8_t)('0' + v % 10u); v /= 10u; }
            q[0] = (uint8_t)('0' + v);
            if (nd > 1) q[1] = '.';
            q += nd > 1 ? nd + 1 : 1;
            q[0] = 'e'; q[1] = '+'; q[2] = (uint8_t)('0' + (uint32_t)X / 10u); q[3] = (uint8_t)('0' + (uint32_t)X % 10u);
        }
        return n + len;
    }
    if (X >= 0) {                                                // X + 1 digits in front of the point, zeros filled in
        const uint32_t ni = (uint32_t)X + 1u;
        const uint32_t len = nd > ni ? nd + 1 : ni;
        if (p) {
            uint8_t *q = p + n;
            uint32_t v = D;
            for (uint32_t k = ni; k > nd; --k) q[k - 1] = '0';
            for (uint32_t k = nd; k-- > 0;) { q[k < ni ? k : k + 1] = (uint8_t)('0' + v % 10u); v /= 10u; }
            if (nd > ni) q[ni] = '.';
        }
        return n + len;
    }
    const uint32_t nz = (uint32_t)(-X) - 1u;                     // 0.000ddd
    if (p) {
        uint8_t *q = p + n;
        q[0] = '0'; q[1] = '.';
        for (uint32_t k = 0; k < nz; ++k) q[2 + k] = '0';
        uint32_t v = D;
        for (uint32_t k = nd; k-- > 0;) { q[2 + nz + k] = (uint8_t)('0' + v % 10u); v /= 10u; }
    }
    return n + 2u + nz + nd;
}

// ---- aux fields -----------------------------------------------------------------------------------------------------------------------
// bytes of a value of type t ("cCsSiIf"; 0: none of them)
BGZ_HD uint32_t aux_scalar_bytes(uint32_t t) {
    return (t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : (t == 'i' || t == 'I' || t == 'f') ? 4u : 0u;
}
BGZ_HD int64_t aux_int(const uint8_t *p, uint32_t t) {
    if (t == 'c') return (int8_t)p[0];
    if (t == 'C') return p[0];
    if (t == 's') return (int16_t)o_rd16(p);
    if (t == 'S') return o_rd16(p);
    if (t == 'i') return (int32_t)o_rd32(p);
    return o_rd32(p);
}
// text of one value (an integer type or f): its length; with dst, written there
BGZ_HD uint32_t aux_value_text(const uint8_t *p, uint32_t t, uint8_t *dst) {
    if (t == 'f') return g_text(o_rd32(p), dst);
    const int64_t v = aux_int(p, t);
    return dst ? t_put_int(dst, v) : t_nint(v);
}

// One field at p of an aux area that ends at end.  CHECK: everything that makes it odd is looked for (reason: the smallest
// reason number found, 0 none; a field that cannot be walked past ends the walk: *in_len 0).  Without CHECK the field is one
// a check has passed.  *in_len = its bytes, *out_len = its text "\tTG:t:value".
struct AuxField { uint32_t in_len, out_len, reason, type; };

BGZ_HD uint32_t odd_min(uint32_t a, uint32_t b) { return a == 0u ? b : (b == 0u ? a : (a < b ? a : b)); }

template <bool CHECK> BGZ_HD AuxField aux_field(const uint8_t *p, const uint8_t *end) {
    AuxField f{0, 0, 0, 0};
    const uint64_t left = (uint64_t)(end - p);
    if (CHECK && left < 3) { f.reason = AMP_BAM_ODD_AUX_TRUNC; return f; }
    const uint32_t t = p[2];
    f.type = t;
    if (CHECK && (!t_graph(p[0]) || !t_graph(p[1]))) f.reason = AMP_BAM_ODD_AUX_CHAR;
    const uint8_t *v = p + 3;
    const uint32_t sz = aux_scalar_bytes(t);
    if (t == 'A') {
        if (CHECK && left < 4) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TRUNC); return f; }
        if (CHECK && !t_graph(v[0])) f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_CHAR);
        f.in_len = 4; f.out_len = 7;
    } else if (sz) {
        if (CHECK && left < 3 + sz) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TRUNC); return f; }
        if (CHECK && t == 'f' && !g_in_set(o_rd32(v))) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_FLOAT); f.in_len = 3 + sz; return f; }
        f.in_len = 3 + sz; f.out_len = 6 + aux_value_text(v, t, nullptr);
    } else if (t == 'Z' || t == 'H') {
        uint64_t n = 0;
        bool bad_char = false;
        if (CHECK) {
            while (3 + n < left && v[n]) { if (v[n] < 32u || v[n] > 126u) bad_char = true; ++n; }
            if (3 + n >= left) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TRUNC); return f; }
            if (bad_char) f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_CHAR);
        } else {
            while (v[n]) ++n;
        }
        f.in_len = (uint32_t)(4 + n); f.out_len = (uint32_t)(6 + n);
    } else if (t == 'B') {
        if (CHECK && left < 8) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TRUNC); return f; }
        const uint32_t st = v[0], esz = aux_scalar_bytes(st);
        if (CHECK && !esz) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TYPE); return f; }
        const uint64_t cnt = o_rd32(v + 1);
        if (CHECK && 8 + cnt * esz > left) { f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TRUNC); return f; }
        uint64_t out = 7;
        bool bad_float = false;
        for (uint64_t k = 0; k < cnt; ++k) {
            const uint8_t *ev = v + 5 + k * esz;
            if (CHECK && st == 'f' && !g_in_set(o_rd32(ev))) { bad_float = true; continue; }
            out += 1 + aux_value_text(ev, st, nullptr);
        }
        if (CHECK && bad_float) f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_FLOAT);
        f.in_len = (uint32_t)(8 + cnt * esz); f.out_len = (uint32_t)out;
    } else if (CHECK) {
        f.reason = odd_min(f.reason, AMP_BAM_ODD_AUX_TYPE);
    }
    return f;
}

// the text of a field a check has passed, Z / H bodies left out (the wave copies those): "\tTG:t:" and the value
BGZ_HD void aux_put(uint8_t *d, const uint8_t *p, AuxField f) {
    const uint32_t t = f.type;
    const bool is_int = t != 'A' && t != 'f' && t != 'Z' && t != 'H' && t != 'B';
    d[0] = '\t'; d[1] = p[0]; d[2] = p[1]; d[3] = ':'; d[4] = is_int ? (uint8_t)'i' : (uint8_t)t; d[5] = ':';
    const uint8_t *v = p + 3;
    if (t == 'A') d[6] = v[0];
    else if (t == 'B') {
        const uint32_t st = v[0], esz = aux_scalar_bytes(st);
        const uint64_t cnt = o_rd32(v + 1);
        uint8_t *q = d + 6;
        *q++ = (uint8_t)st;
        for (uint64_t k = 0; k < cnt; ++k) { *q++ = ','; q += aux_value_text(v + 5 + k * esz, st, q); }
    } else if (t != 'Z' && t != 'H') (void)aux_value_text(v, t, d + 6);
}

// ---- a record ----------------------------------------------------------------------------------------------------------------------------
// rec = a record of the image, from its block_size word on, that the index has walked (its fixed fields, name, CIGAR words, bases
// and qualities lie inside block_size)
struct RecView {
    const uint8_t *name, *cig, *seq, *qual, *aux, *end;
    uint32_t l_name, n_cig, flag, l_seq, mapq;
    int32_t ref_id, next_ref, next_pos, tlen;
};
BGZ_HD RecView rec_view(const uint8_t *rec) {
    RecView v;
    const uint8_t *c = rec + 4;
    v.ref_id = (int32_t)o_rd32(c); v.l_name = c[8]; v.mapq = c[9]; v.n_cig = o_rd16(c + 12); v.flag = o_rd16(c + 14);
    v.l_seq = o_rd32(c + 16); v.next_ref = (int32_t)o_rd32(c + 20); v.next_pos = (int32_t)o_rd32(c + 24); v.tlen = (int32_t)o_rd32(c + 28);
    v.name = c + 32; v.cig = v.name + v.l_name; v.seq = v.cig + 4ull * v.n_cig; v.qual = v.seq + (((uint64_t)v.l_seq + 1) >> 1);
    v.aux = v.qual + v.l_seq; v.end = c + o_rd32(rec);
    return v;
}
BGZ_HD bool qual_absent(const RecView &v) { return v.l_seq == 0u || v.qual[0] == 0xFFu; }
BGZ_HD uint32_t name_len(const Text &t, int32_t r) { return t.name_off[r + 1] - t.name_off[r]; }
// RNEXT: '*' below zero, '=' for RNAME's, else the name
BGZ_HD uint32_t rnext_len(const Text &t, const RecView &v) { return (v.next_ref < 0 || v.next_ref == v.ref_id) ? 1u : name_len(t, v.next_ref); }

// The verdict on a row and its sizes: *tsz = the line without its POS and CIGAR fields (ten tabs and the newline included),
// *asz = its aux fields with their tabs.  Returns the reason (0: the device writes it).
BGZ_HD uint32_t row_check(const Text &t, const uint8_t *rec, uint32_t *tsz, uint32_t *asz) {
    const RecView v = rec_view(rec);
    uint32_t why = 0;
    if (v.l_name == 0u) why = AMP_BAM_ODD_QNAME;
    for (uint32_t k = 0; k + 1 < v.l_name; ++k) if (!t_graph(v.name[k])) why = AMP_BAM_ODD_QNAME;
    if (v.ref_id >= t.n_names || v.next_ref >= t.n_names) why = odd_min(why, AMP_BAM_ODD_REF);
    for (uint32_t k = 0; k < v.n_cig; ++k) if ((o_rd32(v.cig + 4ull * k) & 15u) > 9u) why = odd_min(why, AMP_BAM_ODD_CIGAR_OP);
    if (!qual_absent(v)) {
        const uint64_t hi = 0x8080808080808080ull, lo7 = 0x7F7F7F7F7F7F7F7Full, add = 0x2222222222222222ull;      // byte > 93
        uint64_t bad = 0;
        uint32_t k = 0;
        for (; k + 8u <= v.l_seq; k += 8u) { const uint64_t w = o_load8(v.qual + k); bad |= (((w & lo7) + add) | w) & hi; }
        for (; k < v.l_seq; ++k) if (v.qual[k] > 93u) bad = 1;
        if (bad) why = odd_min(why, AMP_BAM_ODD_QUAL);
    }
    uint64_t a = 0;
    for (const uint8_t *p = v.aux; p < v.end;) {
        const AuxField f = aux_field<true>(p, v.end);
        why = odd_min(why, f.reason);
        if (!f.in_len) break;
        p += f.in_len; a += f.out_len;
    }
    if (why) return why;
    uint64_t n = 11;                                             // ten tabs, the newline
    n += v.l_name - 1u;
    n += t_ndigits(v.flag) + t_ndigits(v.mapq);
    n += v.ref_id < 0 ? 1u : name_len(t, v.ref_id);
    n += rnext_len(t, v);
    n += t_nint((int64_t)v.next_pos + 1) + t_nint(v.tlen);
    n += v.l_seq ? v.l_seq : 1u;
    n += qual_absent(v) ? 1u : v.l_seq;
    *tsz = (uint32_t)(n + a); *asz = (uint32_t)a;
    return 0;
}

// text length of a CIGAR of n words
BGZ_HD uint32_t cigar_text_len(const uint32_t *w, uint32_t n) {
    uint32_t len = 0;
    for (uint32_t k = 0; k < n; ++k) len += t_ndigits(w[k] >> 4) + 1u;
    return len;
}

// one lane: everything between QNAME and SEQ, "\tFLAG\tRNAME\tPOS\tMAPQ\tCIGAR\tRNEXT\tPNEXT\tTLEN\t"; returns its end
BGZ_HD uint8_t *line_head(uint8_t *d, const Text &t, const RecView &v, int32_t new_pos, const uint32_t *cg, uint32_t nn) {
    *d++ = '\t'; d += t_put_uint(d, v.flag);
    *d++ = '\t';
    if (v.ref_id < 0) *d++ = '*';
    else { const uint32_t n = name_len(t, v.ref_id); for (uint32_t k = 0; k < n; ++k) d[k] = t.names[t.name_off[v.ref_id] + k]; d += n; }
    *d++ = '\t'; d += t_put_int(d, (int64_t)new_pos + 1);
    *d++ = '\t'; d += t_put_uint(d, v.mapq);
    *d++ = '\t';
    for (uint32_t k = 0; k < nn; ++k) { d += t_put_uint(d, cg[k] >> 4); *d++ = t_cigar_char(cg[k] & 15u); }
    *d++ = '\t';
    if (v.next_ref < 0) *d++ = '*';
    else if (v.next_ref == v.ref_id) *d++ = '=';
    else { const uint32_t n = name_len(t, v.next_ref); for (uint32_t k = 0; k < n; ++k) d[k] = t.names[t.name_off[v.next_ref] + k]; d += n; }
    *d++ = '\t'; d += t_put_int(d, (int64_t)v.next_pos + 1);
    *d++ = '\t'; d += t_put_int(d, v.tlen);
    *d++ = '\t';
    return d;
}

// the wave: l_seq bases from nibbles, eight per lane and step (four packed bytes in, eight characters out); the last l_seq % 8
// one per lane
BGZ_HD void wave_bases(uint8_t *d, const uint8_t *seq, uint32_t l_seq, uint32_t lane) {
    for (uint32_t o = lane * 8u; o + 8u <= l_seq; o += TEXT_WAVE * 8u) {
        const uint32_t w = o_rd32(seq + (o >> 1));
        uint64_t out = 0;
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t byte = (w >> (8u * (k >> 1))) & 255u;
            out |= (uint64_t)t_base_char((k & 1u) ? (byte & 15u) : (byte >> 4)) << (8u * k);
        }
        o_store8(d + o, out);
    }
    const uint32_t i = (l_seq & ~7u) + lane;
    if (i < l_seq) { const uint32_t byte = seq[i >> 1]; d[i] = t_base_char((i & 1u) ? (byte & 15u) : (byte >> 4)); }
}
// ... and l_seq qualities + 33 (none above 93: no carry between bytes)
BGZ_HD void wave_quals(uint8_t *d, const uint8_t *qual, uint32_t l_seq, uint32_t lane) {
    for (uint32_t o = lane * 8u; o + 8u <= l_seq; o += TEXT_WAVE * 8u) o_store8(d + o, o_load8(qual + o) + 0x2121212121212121ull);
    const uint32_t i = (l_seq & ~7u) + lane;
    if (i < l_seq) d[i] = (uint8_t)(qual[i] + 33u);
}

// the wave: the aux fields of a record a check has passed, to d.  Every lane walks the fields (they are sequential in BAM: a field's
// place follows from the sizes of those in front of it); field k is converted by lane k % 64, so 64 fields are in work at a time,
// and the body of a Z / H field is copied by all lanes together.
BGZ_HD void wave_aux(uint8_t *d, const RecView &v, uint32_t lane) {
    uint32_t k = 0;
    for (const uint8_t *p = v.aux; p < v.end; ++k) {
        const AuxField f = aux_field<false>(p, v.end);
        if (!f.in_len) break;
        if (f.type == 'Z' || f.type == 'H') wave_copy(d + 6, p + 3, f.out_len - 6u, lane);
        if ((k & (TEXT_WAVE - 1u)) == lane) aux_put(d, p, f);
        p += f.in_len; d += f.out_len;
    }
}

}  // namespace ampbamtext
