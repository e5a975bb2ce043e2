// amp_bamtext.hip -- trimmed reads of a BAM input as SAM text on the device: the last cell of the matrix of
// inputs and trimmed outputs, and the mirror of section 13's k_sam_bam_records.  Part of amp_bgzf.hip's translation unit (included
// there behind amp_bamout.hip; it reads the image, record offsets, batch and Trim arrays of struct amp_bam); the lane functions
// are in amp_bamtext.hpp.
//
// The Python codec writes a trimmed read with AlignmentWriter(mode="w").write(r, pos=, cigar=) (out_aln.write, AmpliPy.py:911): a
// Rec per record, a join per base, aux fields through aux_bam_to_sam.  Here the same line is made in HBM from the record where it
// lies in the piece's image:
//   check    lane = row, behind the feed: name, CIGAR words, qualities and aux fields walked once -- the verdict (would the Python
//            codec write exactly what the device would?) and the length of the line without its POS and CIGAR fields
//   size     lane = row, behind amp_bam_process: a kept row's length with the new POS and CIGAR; a 64-bit exclusive sum
//   lines    one wave per kept row, four per workgroup: QNAME and Z / H bodies by wide copies, the decimal fields and the CIGAR by
//            one lane, bases and qualities eight per lane and step, aux fields a lane each
// A piece with an odd row is not formatted here at all: the caller hands its records to the Python codec, so the device never
// emits what that codec would not.  A check costs one wait, a format two (the sizes, then the copy).

using namespace ampbamtext;

namespace ampbgzf {

BGZ_HD void lane_text_check(const Buf &b, int64_t r) {
    const Text &x = b.x;
    uint32_t tsz = 0, asz = 0;
    const uint32_t why = row_check(x, out_rec(b, r), &tsz, &asz);
    if (why) AMP_MIN64(&x.tctl[TCTL_ODD], ((unsigned long long)r << 8) | why);
    x.row_tsz[r] = tsz; x.row_asz[r] = asz;
}

BGZ_HD bool text_kept(const Text &x, int64_t r) {
    return r < x.good_rows && row_kept(x.ref_len[r], x.trim_flags[r], x.min_length, x.include_no_primer);
}
BGZ_HD const uint32_t *text_new_cig(const Buf &b, int64_t r) { return b.x.new_cig + b.cig_off32[r] + 3u * (uint64_t)r; }

BGZ_HD void lane_text_size(const Buf &b, int64_t r) {            // r == n_rows: the slot the scan leaves the total in
    const Text &x = b.x;
    uint64_t sz = 0;
    if (r < x.n_rows && text_kept(x, r)) {
        sz = (uint64_t)x.row_tsz[r] + t_nint((int64_t)x.new_pos[r] + 1) + cigar_text_len(text_new_cig(b, r), x.new_ncig[r]);
        AMP_ADD64(&x.tctl[TCTL_ROWS], 1);
    }
    x.row_off[r] = sz;
}

BGZ_HD void lane_text_line(const Buf &b, int64_t r, uint32_t lane) {
    const Text &x = b.x;
    const uint64_t from = x.row_off[r], to = x.row_off[r + 1];
    if (to == from) return;
    const RecView v = rec_view(out_rec(b, r));
    uint8_t *d = x.out + from, *end = x.out + to;
    // from the line's end backwards: newline, aux, QUAL, tab, SEQ; the head fills what lies between QNAME and SEQ
    uint8_t *aux = end - 1 - x.row_asz[r];
    const uint32_t nq = qual_absent(v) ? 1u : v.l_seq, ns = v.l_seq ? v.l_seq : 1u;
    uint8_t *qual = aux - nq, *seq = qual - 1 - ns;
    wave_copy(d, v.name, v.l_name - 1u, lane);
    if (lane == 0) {
        (void)line_head(d + v.l_name - 1u, x, v, x.new_pos[r], text_new_cig(b, r), x.new_ncig[r]);
        if (!v.l_seq) *seq = '*';
        qual[-1] = '\t';
        if (qual_absent(v)) *qual = '*';
        end[-1] = '\n';
    }
    wave_bases(seq, v.seq, v.l_seq, lane);
    if (!qual_absent(v)) wave_quals(qual, v.qual, v.l_seq, lane);
    wave_aux(aux, v, lane);
}

}  // namespace ampbgzf

#ifndef AMPBGZF_HOSTSIM
CODEC_KERNEL(k_bamtext_check, lane_text_check)
CODEC_KERNEL(k_bamtext_size, lane_text_size)
// One wave per row (four a workgroup), as k_bamout_records: no LDS, and nothing a lane keeps lives in an array.
__global__ void __launch_bounds__(256) k_bamtext_lines(Buf b) {
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < b.x.n_rows; r += (int64_t)gridDim.x * 4) lane_text_line(b, r, lane);
}
static int text_lines(amp_bam *s) {
    k_bamtext_lines<<<codec_grid(s->b.x.n_rows * 64), 256, 0, s->sh.stream>>>(s->b);
    return hipGetLastError() == hipSuccess ? AMP_OK : AMP_EHIP;
}
#else
static int text_lines(amp_bam *s) {
    for (int64_t r = 0; r < s->b.x.n_rows; ++r) for (uint32_t lane = 0; lane < TEXT_WAVE; ++lane) lane_text_line(s->b, r, lane);
    return AMP_OK;
}
#endif

// the per-row tables of pieces of up to n rows (grown once, then reused)
static int text_ensure(amp_bam *s, int64_t n) {
    State &t = s->text;
    Text &x = s->b.x;
    if (!t.arena || n > t.arena_rows) {
        const int64_t cr = n + n / 8 + 64;
        Carver take{nullptr};
        for (int pass = 0; pass < 2; ++pass) {
            x.row_tsz = (uint32_t *)take((size_t)cr * 4); x.row_asz = (uint32_t *)take((size_t)cr * 4);
            x.row_off = (uint64_t *)take(((size_t)cr + 2) * 8); x.tctl = (unsigned long long *)take(TCTL_WORDS * 8);
            if (pass == 0) { CODEC_OK(codec_grow(s->sh, &t.arena, &t.cap_arena, take.o)); take = Carver{t.arena}; }
        }
        t.arena_rows = cr;
    }
    x.names = t.names; x.name_off = (const uint32_t *)t.name_off; x.n_names = t.n_names;
    return AMP_OK;
}

static void text_info(amp_bam *s, int64_t rows, int64_t bytes, int64_t waits, int64_t down, amp_bam_text_info *info) {
    amp_bam_text_info I{};
    I.first_odd_row = s->text.first_odd; I.odd_reason = s->text.odd_reason;
    I.n_rows_written = rows; I.n_bytes = bytes; I.waits = waits; I.bytes_down = down;
    *info = I;
}

extern "C" {

// header.refs of bamio.AlignmentWriter: the names RNAME and RNEXT are written from (the table amp_sam_set_references takes)
int amp_bam_set_references(amp_bam *s, int32_t n_ref, const char *const *names) {
    if (!s || n_ref < 0 || n_ref > AMP_SAM_MAX_REFS || (n_ref && !names)) return AMP_EINVAL;
    DevGuard guard(s->sh);
    uint32_t off[AMP_SAM_MAX_REFS + 1];
    uint8_t blob[AMP_SAM_MAX_REF_BYTES + 16];
    size_t tot = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (!names[r]) return AMP_EINVAL;
        const size_t n = strlen(names[r]);
        if (tot + n > AMP_SAM_MAX_REF_BYTES) return AMP_EINVAL;
        off[r] = (uint32_t)tot;
        memcpy(blob + tot, names[r], n);
        tot += n;
    }
    off[n_ref] = (uint32_t)tot;
    State &t = s->text;
    if (!t.names) {
        CODEC_OK(codec_alloc(&t.names, AMP_SAM_MAX_REF_BYTES + 16));
        CODEC_OK(codec_alloc(&t.name_off, sizeof(off)));
    }
    CODEC_OK(codec_up(s->sh, t.names, blob, tot));
    CODEC_OK(codec_up(s->sh, t.name_off, off, ((size_t)n_ref + 1) * 4));
    CODEC_OK(codec_sync(s->sh));                         // (blob and off are this call's own)
    t.n_names = n_ref;
    t.checked = false;
    return AMP_OK;
}

// Would AlignmentWriter.write give, for every row of the last feed, exactly the line the device makes?  The first odd row and why
int amp_bam_text_check(amp_bam *s, amp_bam_text_info *info) {
    if (!s || !info) return AMP_EINVAL;
    if (!s->fed || s->info.n_refused || s->info.bad_record || s->text.n_names < 0) return AMP_ESTATE;
    DevGuard guard(s->sh);
    State &t = s->text;
    const int64_t n = s->info.n_rows, waits0 = s->sh.waits;
    t.checked = false; t.first_odd = -1; t.odd_reason = AMP_BAM_ODD_NONE;
    int64_t down = 0;
    if (n > 0) {
        CODEC_OK(text_ensure(s, n));
        s->b.x.n_rows = n;
        codec_mark(s->sh, 12);
        CODEC_OK(codec_zero(s->sh, s->b.x.tctl, 0xFF, 8));
        CODEC_RUN(s, k_bamtext_check, lane_text_check, n, -1);
        codec_mark(s->sh, 13);
        CODEC_OK(codec_down(s->sh, t.h_tctl, s->b.x.tctl, 8));
        CODEC_OK(codec_wait(s->sh));
        down = 8;
        if (t.h_tctl[TCTL_ODD] != ~0ull) { t.first_odd = (int64_t)(t.h_tctl[TCTL_ODD] >> 8); t.odd_reason = (int32_t)(t.h_tctl[TCTL_ODD] & 255u); }
    }
    t.checked = true;
    text_info(s, 0, 0, s->sh.waits - waits0, down, info);
    return AMP_OK;
}

// out_aln.write(s) of A:911 under the filter of A:910 for the rows in front of the first failing one, as amp_sam_format
int amp_bam_format(amp_bam *s, int32_t min_length, int32_t include_no_primer, uint8_t *out, int64_t cap, amp_bam_text_info *info) {
    if (!s || !info || cap < 0 || (cap && !out)) return AMP_EINVAL;
    State &t = s->text;
    const int64_t n = s->fed ? s->info.n_rows : 0;
    if (!s->fed || !t.checked || t.first_odd >= 0 || (n && !s->processed)) return AMP_ESTATE;
    DevGuard guard(s->sh);
    const int64_t waits0 = s->sh.waits;
    if (n == 0) { text_info(s, 0, 0, 0, 0, info); return AMP_OK; }
    Text &x = s->b.x;
    x.new_pos = s->trim.new_pos; x.new_ncig = s->trim.new_ncig; x.new_cig = s->trim.new_cig; x.ref_len = s->trim.ref_len; x.trim_flags = s->trim.trim_flags;
    x.n_rows = n; x.good_rows = s->good_rows; x.min_length = min_length; x.include_no_primer = include_no_primer ? 1 : 0;
    codec_mark(s->sh, 14);
    CODEC_OK(codec_zero(s->sh, &x.tctl[TCTL_ROWS], 0, 8));
    CODEC_RUN(s, k_bamtext_size, lane_text_size, n + 1, -1);
    CODEC_OK(codec_scan(s->sh, x.row_off, n + 1));
    unsigned long long total = 0;
    CODEC_OK(codec_down(s->sh, &t.h_tctl[TCTL_ROWS], &x.tctl[TCTL_ROWS], 8));
    CODEC_OK(codec_down(s->sh, &total, &x.row_off[n], 8));
    CODEC_OK(codec_wait(s->sh));
    const int64_t rows = (int64_t)t.h_tctl[TCTL_ROWS];
    if ((int64_t)total > cap || total >= (1ull << 32)) { text_info(s, rows, (int64_t)total, s->sh.waits - waits0, 16, info); return AMP_EOVERFLOW; }
    if (total) {
#ifdef AMPBGZF_HOSTSIM
        CODEC_OK(codec_grow(s->sh, &t.out, &t.cap_out, (size_t)total + 256));
        t.guard_at = (int64_t)total; t.guard_len = (int64_t)(t.cap_out - (size_t)total);
        memset(t.out + t.guard_at, 0xA5, (size_t)t.guard_len);
#else
        CODEC_OK(codec_grow(s->sh, &t.out, &t.cap_out, (size_t)total + 64));
#endif
        x.out = t.out;
        CODEC_OK(text_lines(s));
        codec_mark(s->sh, 15);
        CODEC_OK(codec_down(s->sh, out, t.out, (size_t)total));
        codec_mark(s->sh, 16);
        CODEC_OK(codec_wait(s->sh));
    }
    text_info(s, rows, (int64_t)total, s->sh.waits - waits0, 16 + (int64_t)total, info);
    return AMP_OK;
}

#ifdef AMPBGZF_HOSTSIM
// 0 when the last format wrote nothing behind its text (the twin's guard bytes)
int amp_bam_twin_text_guard(amp_bam *s) {
    if (!s) return AMP_EINVAL;
    for (int64_t k = 0; k < s->text.guard_len; ++k) if (s->text.out[s->text.guard_at + k] != 0xA5) return 1;
    return 0;
}
#endif

}  // extern "C"
