// amp_bf.hpp -- the closed-form trims of amp_read.hpp (Cig2: reads of the shape [S a][M m1]([I|D k][M m2])[S c]) once
// more, written WITHOUT branches: every rule of primer_clip / quality_clip (A:467-510, A:524-555, A:597-622, A:658-683),
// get_pos_on_query (A:389-412) and get_pos_on_ref (A:363-386) becomes arithmetic and selects on the five lengths.
//
// Why: one lane per read means a wave executes the union of all the paths its 64 reads take, and every `if' of the
// branchy forms costs a save / branch / restore of the execution mask even when it is not taken; the per-read logic was
// a third of the fast kernel's instructions.  Here a read's whole trim is ~300 straight-line vector instructions.
// tests/hostsim fuzzes these forms against the branchy ones and against the generic code on the CPU
// (tests/test_hostsim_golden.py::test_branch_free_closed_forms), and walks them over the complete domain of reads of up to 12
// bases (tests/hostsim/bf_forms_main.cpp, tests/test_bf_forms_exhaustive.py).
//
// A rule that is a clamp or a saturating difference is written as min / max arithmetic on the lengths, not as a chain of `bool's:
// on the device a `bool' is a compare into a scalar register pair, every & | ! of two is a scalar mask operation and every field it
// decides a select, and the fast kernel has no wave to spare for scalar instructions.
#pragma once

#include "amp_read.hpp"

namespace amp {

struct Bf {                       // the shape; kind 0 none (k = m2 = 0), 1 insertion, 2 deletion
    int32_t a, m1, k, m2, c, kind;
    uint32_t op;
    uint32_t punt;                // 1: a shape the closed forms leave to the generic code
    AMP_HD int32_t kI() const { return kind == 1 ? k : 0; }
    AMP_HD int32_t kD() const { return kind == 2 ? k : 0; }
    AMP_HD int32_t query_len() const { return a + m1 + kI() + m2 + c; }
    AMP_HD int32_t ref_len() const { const int32_t r = m1 + m2 + kD(); return r ? r : 1; }
};
AMP_HD int32_t bf_sel(bool c, int32_t x, int32_t y) { return c ? x : y; }
AMP_HD int32_t bf_min(int32_t x, int32_t y) { return x < y ? x : y; }
AMP_HD int32_t bf_max(int32_t x, int32_t y) { return x > y ? x : y; }
// c ? x : y, field by field (a select of whole structs goes through memory)
AMP_HD Bf bf_pick(bool c, const Bf &x, const Bf &y) {
    return Bf{c ? x.a : y.a, c ? x.m1 : y.m1, c ? x.k : y.k, c ? x.m2 : y.m2, c ? x.c : y.c, c ? x.kind : y.kind, c ? x.op : y.op, c ? x.punt : y.punt};
}
AMP_HD Bf bf_mirror(const Bf &s) { return Bf{s.c, s.kind ? s.m2 : s.m1, s.k, s.kind ? s.m1 : s.m2, s.a, s.kind, s.op, s.punt}; }

// the shape of an input CIGAR of n ops (its first five words; words past the read's own may hold anything) -- cig2_from_words5;
// ok = 0: not a shape of the family
AMP_HD Bf bf_from_words5(int n, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, int32_t lseq, int32_t max_ins, int32_t max_del, bool &ok) {
    const bool lead = (w0 & 15u) == OP_S;
    const uint32_t v0 = lead ? w1 : w0, v1 = lead ? w2 : w1, v2 = lead ? w3 : w2, v3 = lead ? w4 : w3;
    const int m = n - (lead ? 1 : 0);                      // ops behind the leading clip: M | M S | M X M | M X M S
    const uint32_t o0 = v0 & 15u, o1 = v1 & 15u;
    const bool has3 = m >= 3, isI = o1 == OP_I, isD = o1 == OP_D;
    const bool has_tail = has3 ? m == 4 : m == 2;
    const uint32_t tail = has3 ? v3 : v1;
    Bf s;
    s.op = o0; s.punt = 0u;
    s.a = lead ? (int32_t)(w0 >> 4) : 0;
    s.m1 = (int32_t)(v0 >> 4);
    s.kind = has3 ? (isI ? 1 : 2) : 0;
    s.k = has3 ? (int32_t)(v1 >> 4) : 0;
    s.m2 = has3 ? (int32_t)(v2 >> 4) : 0;
    s.c = has_tail ? (int32_t)(tail >> 4) : 0;
    bool good = (n >= 1) & (n <= 5) & (lseq > 0) & (m >= 1) & (m <= 4) & ((o0 == OP_M) | (o0 == OP_EQ) | (o0 == OP_X)) & (s.m1 > 0);
    good = good & (!lead | (s.a > 0));
    good = good & (!has3 | ((isI | isD) & ((v2 & 15u) == o0) & (s.k > 0) & (s.m2 > 0)));
    good = good & (!has_tail | (((tail & 15u) == OP_S) & (s.c > 0)));
    good = good & (s.query_len() == lseq);
    good = good & ((s.kind != 1) | (s.k <= max_ins)) & ((s.kind != 2) | (s.k <= max_del));
    ok = good;
    return bf_pick(good, s, Bf{0, 0, 0, 0, 0, 0, 0u, 0u});
}

// get_pos_on_query (A:389-412) on the shape; t = ref_pos - reference_start
AMP_HD int32_t bf_pos_on_query(const Bf &s, int32_t t) {
    const bool in1 = (s.m1 > 0) & (t <= s.m1);
    const int32_t tD = t - s.m1;
    const bool inD = (s.kind == 2) & (tD <= s.k) & !in1;
    const int32_t u = tD - s.kD();
    const bool in2 = (s.kind != 0) & (s.m2 > 0) & (u <= s.m2) & !in1 & !inD;
    int32_t r = s.query_len();
    r = in2 ? s.a + s.m1 + s.kI() + u : r;
    r = inD ? s.a + s.m1 : r;
    r = in1 ? s.a + t : r;
    return r;
}

// get_pos_on_ref (A:363-386) on the shape, minus reference_start
AMP_HD int32_t bf_ref_offset(const Bf &s, int32_t qp) {
    const bool in0 = (s.a > 0) & (qp <= s.a);
    const int32_t x = qp - s.a;
    const bool in1 = !in0 & (s.m1 > 0) & (x <= s.m1);
    const int32_t x2 = x - s.m1;
    const bool inI = !in0 & !in1 & (s.kind == 1) & (x2 <= s.k);
    const int32_t x3 = x2 - s.kI();
    const bool in2 = !in0 & !in1 & !inI & (s.kind != 0) & (s.m2 > 0) & (x3 <= s.m2);
    int32_t r = s.m1 + s.kD() + (s.kind ? s.m2 : 0);
    r = in2 ? s.m1 + s.kD() + x3 : r;
    r = inI ? s.m1 : r;
    r = in1 ? x : r;
    r = in0 ? 0 : r;
    return r;
}

// d >= 0 query bases behind the soft clip become soft clip (primer_clip with its `del' already reduced by the clip's share,
// A:467-510, or quality_clip, A:597-622: QUALITY).  What the two differ in: a clip that ends exactly in front of the indel
// keeps it when it is a quality clip (the op is copied behind the clip) and swallows it when it is a primer clip (an
// insertion turns into soft clip, a deletion is dropped and the start jumps over it).  adv = the reference advance.
// skip: the caller's `del == 0' (both clips return at once: nothing changes, nothing is punted); it passes d = 0 with it.
//
// Written as arithmetic on the lengths, with ONE lane condition for the outcome (a `bool' costs a compare into a scalar pair, the
// mask operations that combine it and a select per field it decides):
//   the indel survives (`keep') when the clip ends inside the first match op, inside the insertion or -- a quality clip -- exactly in
//   front of the indel: d < m1 + kq with kq = the bases of the indel a clip may end in front of.  The clip then moves the start
//   by d whatever it ate: a + d, and takes min(d, m1) from the first op and the rest from the insertion.
//   otherwise the clip goes through the indel and eats t = min(d - m1 - kI, m2) of the second segment, which becomes the first.
template <bool QUALITY>
AMP_HD Bf bf_clip_left(const Bf &s, int32_t d, bool skip, int32_t &adv) {
    const int32_t kI = s.kI(), kD = s.kD();
    const int32_t e = bf_min(d, s.m1), d1 = d - e;                              // eaten from the first match op; what is left of the clip behind it
    const int32_t kq = QUALITY ? (s.kind == 2 ? 1 : kI) : kI;
    const bool keep = QUALITY ? ((d < s.m1 + kq) | skip) : (((d < s.m1 + kq) & (d != s.m1)) | skip);
    // the clip goes through the indel: what is left of the second segment (m2 = 0 without an indel)
    const int32_t t = bf_min(bf_max(d1 - kI, 0), s.m2);
    const int32_t m_left = s.m2 - t;
    const bool gone = m_left == 0;                                              // no match left: one soft clip (canon)
    Bf o;
    o.op = s.op;
    o.punt = s.punt | (((d >= s.m1) & !skip & (s.kind != 0) & (s.m2 == 0)) ? 1u : 0u);      // an indel that already touches the far clip
    o.a = keep ? s.a + d : s.a + s.m1 + kI + t + (gone ? s.c : 0);
    o.m1 = keep ? s.m1 - e : m_left;
    o.k = keep ? s.k - d1 : 0;
    o.m2 = keep ? s.m2 : 0;
    o.kind = keep ? s.kind : 0;
    o.c = (keep | !gone) ? s.c : 0;
    adv = keep ? e : s.m1 + kD + t;
    return o;
}

// primer_clip (A:467-510) of `del' query bases from the front; returns the reference advance
AMP_HD Bf bf_primer_clip(const Bf &s, int32_t del, int32_t &adv) {
    const bool neg = del < 0, zero = del == 0;
    // a soft clip stays one and eats its share.  del < 0: every query-consuming op falls into the "else" arm -- all soft clip, which
    // is what a clip longer than the read leaves; only a deletion still advances, and nothing is punted
    const int32_t d = neg ? 0x3FFFFFFF : bf_max(del - s.a, 0);
    int32_t adv_c;
    Bf o = bf_clip_left<false>(s, d, zero, adv_c);
    o.punt = neg ? s.punt : o.punt;
    adv = neg ? s.kD() : adv_c;
    return o;
}
AMP_HD Bf bf_canon(const Bf &s) {         // no match left: one soft clip
    const bool all = (s.kind == 0) & (s.m1 == 0);
    Bf o = s;
    o.a = all ? s.a + s.c : s.a;
    o.c = all ? 0 : s.c;
    return o;
}
// bf_mirror where f, the shape as it is elsewhere
AMP_HD Bf bf_mirror_if(bool f, const Bf &s) {
    const bool sw = f & (s.kind != 0);
    return Bf{f ? s.c : s.a, sw ? s.m2 : s.m1, s.k, sw ? s.m1 : s.m2, f ? s.a : s.c, s.kind, s.op, s.punt};
}

// Stage 1+2 of trim_read (A:450-558) on the shape, given the two table entries (-1 = None) and the outcome of the
// template-length test of A:452: cig2_trim_primers_isize.  A clip that is not made is a clip of 0 bases, which leaves the shape as
// it is (every shape here is canonical: bf_from_words5 gives m1 > 0, and both clips end in bf_canon or its like).
AMP_HD Bf bf_trim_primers(const Bf &s0, int32_t &pos, uint32_t &flags, uint32_t flag, bool isize_flag, int32_t lseq,
                          int32_t left_max_end, int32_t right_min_start) {
    const bool is_paired = flag & 1u, is_reverse = (flag & 0x10u) != 0;
    const bool far = is_paired & isize_flag;
    const bool do1 = !(far & is_reverse) & (left_max_end >= 0);                             // A:460
    int32_t adv1;
    const Bf s = bf_primer_clip(s0, do1 ? bf_pos_on_query(s0, left_max_end + 1 - pos) : 0, adv1);   // A:463
    pos += adv1;                                                                           // A:514
    flags |= do1 ? AMP_TRIM_PRIMER_START : 0u;
    const bool do2 = !(far & !is_reverse) & (right_min_start >= 0) & !s.punt;              // A:517
    const int32_t del2 = do2 ? lseq - bf_pos_on_query(s, right_min_start - pos) : 0;       // A:520
    int32_t adv2;
    flags |= do2 ? AMP_TRIM_PRIMER_END : 0u;
    return bf_canon(bf_mirror(bf_primer_clip(bf_mirror(s), del2, adv2)));
}

// aligned-quality window of the shape: [lo, lo + qlen) -- cig2_quality_window.  (One soft clip covering the read, whose end is not
// examined, is written [S a]: c = 0.)
AMP_HD void bf_quality_window(const Bf &s, int32_t lseq, int32_t &lo, int32_t &qlen) {
    lo = bf_min(s.a, lseq);
    qlen = bf_max(lseq - s.c, lo) - lo;
}

// Stage 3 of trim_read given the scan result i (A:589-625, A:651-686) -- cig2_trim_quality.  A read is clipped at ONE end, its 5'
// end in read direction: the forward read is mirrored, clipped like the reverse one and mirrored back.
AMP_HD Bf bf_trim_quality(const Bf &s, int32_t pos, uint32_t &flags, bool is_reverse, int32_t i, int32_t qlen) {
    int32_t adv;
    // reverse strand: trimmed only if get_pos_on_ref(del + query_alignment_start - 1) > reference_start (A:591-594);
    // reference_start is NOT advanced.  Forward: if any base goes (A:656).  (quality_clip returns at once on del == 0)
    const bool fwd = !is_reverse;
    const int32_t del = fwd ? qlen - i : i;
    const bool doit = fwd ? del != 0 : bf_ref_offset(s, del + s.a - 1) > 0;
    flags |= doit ? AMP_TRIM_QUALITY : 0u;
    const int32_t d = doit ? del : 0;
    (void)pos;
    return bf_canon(bf_mirror_if(fwd, bf_clip_left<true>(bf_mirror_if(fwd, s), d, d == 0, adv)));
}

}  // namespace amp
