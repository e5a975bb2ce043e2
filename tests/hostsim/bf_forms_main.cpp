// bf_forms_main -- TEST INFRASTRUCTURE: the branch-free closed forms of amplipy_amd/csrc/amp_bf.hpp against the branchy forms of
// amp_read.hpp over a COMPLETE small domain instead of a random one (tests/hostsim/hostsim.hip fuzzes the same pair).  A program of
// its own, host code only, so that it runs under the sanitizers without a sanitizer runtime inside Python:
//   hipcc -x hip --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o bf_forms tests/hostsim/bf_forms_main.cpp && ./bf_forms            (tests/test_bf_forms_exhaustive.py; the host half of a
//   HIP compile and nothing for the device: amp_read.hpp names device builtins in functions this program never calls)
//
// The domain: every shape [S a][M m1]([I|D k][M m2])[S c] whose query is at most QMAX bases long -- a, c >= 0, insertions
// of 1..8, deletions of 1, 2 and 16 -- and, for the clips, the shapes an earlier clip leaves behind: m1 = 0 with the indel directly
// behind the leading clip, m2 = 0 with the indel in front of the trailing one, and the read that is one soft clip.
//   clips      bf_primer_clip against cig2_primer_clip for every del in [-2, 14]; bf_clip_left<true> against cig2_quality_clip for
//              every d in [0, 14]; bf_clip_left<false> against cig2_primer_clip's body for every d in [1, 14]
//   maps       bf_pos_on_query / bf_ref_offset against cig2_pos_on_query / cig2_pos_on_ref at every offset from -2 to past the end
//   trim       bf_trim_primers against cig2_trim_primers_isize with either table entry absent or at every offset from two positions
//              in front of the read to two behind it, both strands, paired or not, the template-length test on and off; on what it
//              leaves, bf_quality_window against cig2_quality_window and bf_trim_quality against cig2_trim_quality for EVERY scan
//              outcome i in [0, qlen]
// Compared field by field: a, m1, k, m2, c, kind, op, punt, the position, the flags, the reference advance, ref_len().  A punted
// shape (Bf::punt: the generic code does the read) is compared on the punt bit alone -- the branchy forms return half-way there.
// Prints "bf_forms ok <shapes> <clips> <maps> <trims> <quality trims> <punted>"; any difference: a line per case (the first 20) and exit code 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../amplipy_amd/csrc/amp_bf.hpp"

using namespace amp;

static long n_bad = 0;

static Cig2 c2(const Bf &b) { return Cig2{b.op, b.a, b.m1, b.k, b.m2, b.c, b.kind, b.punt != 0u}; }

static void report(const char *what, const Bf &in, const Cig2 &x, const Bf &y, long p0, long p1, long p2) {
    if (n_bad++ < 20)
        fprintf(stderr, "%s: in a %d m1 %d k %d m2 %d c %d kind %d | args %ld %ld %ld | branchy a %d m1 %d k %d m2 %d c %d kind %d punt %d | "
                "branch-free a %d m1 %d k %d m2 %d c %d kind %d punt %u\n", what, in.a, in.m1, in.k, in.m2, in.c, in.kind, p0, p1, p2,
                x.a, x.m1, x.k, x.m2, x.c, x.kind, (int)x.punt, y.a, y.m1, y.k, y.m2, y.c, y.kind, y.punt);
}
static bool same_shape(const Cig2 &x, const Bf &y) {
    return x.a == y.a && x.m1 == y.m1 && x.k == y.k && x.m2 == y.m2 && x.c == y.c && x.kind == y.kind && x.op == y.op;
}

// cig2_primer_clip's body behind its del <= 0 exits and the leading clip's share: d > 0 query bases behind the soft clip
static int32_t primer_clip_behind_clip(Cig2 &s, int32_t d) {
    const int32_t a = s.a;
    s.a = 0;
    const int32_t adv = cig2_primer_clip(s, d);
    if (!s.punt) s.a += a;
    return adv;
}

int main(int argc, char **argv) {
    const int QMAX = argc > 1 ? atoi(argv[1]) : 12;
    long n_shapes = 0, n_clips = 0, n_maps = 0, n_trims = 0, n_qtrims = 0, n_punt = 0;
    const int32_t dels[] = {1, 2, 16};
    for (int kind = 0; kind <= 2; ++kind)
    for (int32_t a = 0; a <= QMAX; ++a)
    for (int32_t m1 = 0; a + m1 <= QMAX; ++m1)
    for (int ki = 0; ki < (kind == 0 ? 1 : kind == 1 ? 8 : 3); ++ki)
    for (int32_t m2 = 0; m2 <= (kind ? QMAX : 0); ++m2)
    for (int32_t c = 0; c <= QMAX; ++c)
    for (uint32_t op = OP_M; op <= OP_EQ; op += OP_EQ - OP_M) {
        const int32_t k = kind == 0 ? 0 : kind == 1 ? ki + 1 : dels[ki];
        const Bf s{a, m1, k, m2, c, kind, op, 0u};
        const int32_t lseq = s.query_len();
        if (lseq < 1 || lseq > QMAX) continue;
        if (kind && m1 == 0 && m2 == 0) continue;                    // an indel between two clips: no clip leaves it (the second one punts)
        if (!kind && m1 == 0 && c != 0) continue;                    // one soft clip is written [S a] (canon)
        if (op == OP_EQ && (a + c) % 3) continue;                     // (the op is carried along: a third of the shapes show that)
        ++n_shapes;
        const bool input = m1 > 0 && (!kind || m2 > 0);              // a shape bf_from_words5 accepts
        // ---- the clips ----------------------------------------------------------------------------------------------------
        for (int32_t del = -2; del <= 14; ++del) {
            {
                const Bf &sm = s;                                    // (no mirrored runs: the mirrored shapes are shapes of the domain themselves)
                {
                    Cig2 x = c2(sm); int32_t adv3;
                    const int32_t adv2 = cig2_primer_clip(x, del);
                    Bf y = bf_primer_clip(sm, del, adv3);
                    y = bf_canon(y);                                 // (cig2_primer_clip ends in canon(); in the kernel bf_trim_primers / the emission do)
                    ++n_clips;
                    if (x.punt != (y.punt != 0u)) report("primer_clip punt", sm, x, y, del, 0, 0);
                    else if (x.punt) ++n_punt;
                    else if (!same_shape(x, y) || adv2 != adv3) report("primer_clip", sm, x, y, del, adv2, adv3);
                }
                if (del >= 0) {
                    Cig2 x = c2(sm); int32_t adv3;
                    cig2_quality_clip(x, del);
                    const Bf y = bf_canon(bf_clip_left<true>(sm, del, del == 0, adv3));
                    ++n_clips;
                    if (x.punt != (y.punt != 0u)) report("quality_clip punt", sm, x, y, del, 0, 0);
                    else if (x.punt) ++n_punt;
                    else if (!same_shape(x, y)) report("quality_clip", sm, x, y, del, 0, 0);
                }
                if (del >= 1) {
                    Cig2 x = c2(sm); int32_t adv3;
                    const int32_t adv2 = primer_clip_behind_clip(x, del);
                    const Bf y = bf_canon(bf_clip_left<false>(sm, del, false, adv3));
                    ++n_clips;
                    if (x.punt != (y.punt != 0u)) report("clip_left<false> punt", sm, x, y, del, 0, 0);
                    else if (x.punt) ++n_punt;
                    else if (!same_shape(x, y) || adv2 != adv3) report("clip_left<false>", sm, x, y, del, adv2, adv3);
                }
            }
        }
        // ---- the coordinate maps ------------------------------------------------------------------------------------------
        for (int32_t t = -2; t <= m1 + m2 + k + 3; ++t) {
            ++n_maps;
            if (cig2_pos_on_query(c2(s), 7 + t, 7) != bf_pos_on_query(s, t)) report("pos_on_query", s, c2(s), s, t, 0, 0);
        }
        for (int32_t q = -2; q <= lseq + 3; ++q) {
            ++n_maps;
            if (cig2_pos_on_ref(c2(s), q, 7) - 7 != bf_ref_offset(s, q)) report("ref_offset", s, c2(s), s, q, 0, 0);
        }
        if (!input) continue;
        // ---- the whole trim -----------------------------------------------------------------------------------------------
        const int32_t pos = 4, span = m1 + m2 + (kind == 2 ? k : 0);
        for (int32_t Lo = -3; Lo <= span + 2; ++Lo)                  // -3: the entry is absent; else max_end = pos + Lo
        for (int32_t Ro = -3; Ro <= span + 2; ++Ro)
        for (uint32_t fl = 0; fl < 8; ++fl) {
            const int32_t L = Lo == -3 ? -1 : pos + Lo, R = Ro == -3 ? -1 : pos + Ro;
            const uint32_t flag = (fl & 1u) | ((fl & 2u) << 3);
            const bool isize = (fl & 4u) != 0, rev = (flag & 0x10u) != 0;
            Cig2 s2 = c2(s);
            TrimState t2{pos, 1, 0u, 0};
            cig2_trim_primers_isize(t2, flag, isize, lseq, s2, L, R);
            int32_t p3 = pos; uint32_t f3 = 0u;
            const Bf s3 = bf_trim_primers(s, p3, f3, flag, isize, lseq, L, R);
            ++n_trims;
            if (s2.punt != (s3.punt != 0u)) { report("trim_primers punt", s, s2, s3, L, R, fl); continue; }
            if (s2.punt) { ++n_punt; continue; }
            if (!same_shape(s2, s3) || t2.pos != p3 || t2.flags != f3) { report("trim_primers", s, s2, s3, L, R, fl); continue; }
            int32_t lo2, ql2, lo3, ql3;
            cig2_quality_window(s2, lseq, lo2, ql2);
            bf_quality_window(s3, lseq, lo3, ql3);
            if (lo2 != lo3 || ql2 != ql3) { report("quality_window", s, s2, s3, L, R, fl); continue; }
            for (int32_t i = 0; i <= ql2; ++i) {
                Cig2 a2 = s2; TrimState u2 = t2;
                cig2_trim_quality(u2, rev, i, ql2, a2);
                uint32_t g3 = f3;
                const Bf a3 = bf_trim_quality(s3, p3, g3, rev, i, ql3);
                ++n_qtrims;
                if (a2.punt != (a3.punt != 0u)) { report("trim_quality punt", s3, a2, a3, i, ql2, fl); continue; }
                if (a2.punt) { ++n_punt; continue; }
                if (!same_shape(a2, a3) || u2.flags != g3 || u2.pos != p3 || a2.ref_len() != a3.ref_len()) report("trim_quality", s3, a2, a3, i, ql2, fl);
            }
        }
    }
    if (n_bad) { fprintf(stderr, "bf_forms: %ld differences\n", n_bad); return 1; }
    printf("bf_forms ok %ld %ld %ld %ld %ld %ld\n", n_shapes, n_clips, n_maps, n_trims, n_qtrims, n_punt);
    return 0;
}
