// amp_bamout.hip -- the device re-encoder of trimmed BAM records: what lets `trim` and `aio` stay on the
// device codec for BAM input.  Part of amp_bgzf.hip's translation unit (included there behind struct amp_bam, whose image,
// record offsets, batch and Trim arrays it reads); the lane functions are in amp_bamout.hpp.
//
// The host codec writes trimmed reads with ampbam_write_rows (out_aln.write, AmpliPy.py:911): the unchanged parts of every kept
// record copied from the piece's host image, 0xFF00-byte chunks of the record stream compressed and framed by flush_blocks.
// Here the same bytes are made in HBM, per piece, on the ctx stream, behind amp_bam_process:
//   sizes    lane = row: keep (A:910, rows in front of the first failing one), the new record's size; a 64-bit exclusive sum
//   records  one wave per kept row: name and tail by wide loads and stores, one lane the 36 fixed bytes and the CIGAR words
// and from the record stream to framed BGZF blocks by the tail the SAM codec shares (amp_bamtail.hpp): plan, deflate, crc, frame,
// gather, the carry across calls.
// One wait per encode: every launch is sized by what the host knows after the feed (rows, image bytes) and trimmed on the device
// by the plan's counters.  The stream is continuous across pieces: the bytes behind the last whole chunk open the next call's
// stream, so block boundaries are the host writer's whatever the piece size.

using namespace ampbamout;

namespace ampbgzf {

BGZ_HD const uint8_t *out_rec(const Buf &b, int64_t r) { return b.img + b.rec_off[b.src_index[r] - b.rec_base]; }
BGZ_HD const uint32_t *out_new_cig(const Buf &b, int64_t r) { return b.o.new_cig + b.cig_off32[r] + 3u * (uint64_t)r; }

BGZ_HD void lane_out_size(const Buf &b, int64_t r) {              // r == n_rows: the slot the scan leaves the total in
    const Out &o = b.o;
    uint64_t sz = 0;
    if (r < o.good_rows && row_kept(o.ref_len[r], o.trim_flags[r], o.min_length, o.include_no_primer)) {
        const uint8_t *rec = out_rec(b, r);
        if (!ncig_fits(rec, o.new_ncig[r])) AMP_ADD64(&o.octl[OCTL_BAD], 1);
        else { sz = record_size(rec, o.new_ncig[r]); AMP_ADD64(&o.octl[OCTL_ROWS], 1); }
    }
    o.row_off[r] = sz;
}

BGZ_HD void lane_out_record(const Buf &b, int64_t r, uint32_t lane) {
    const Out &o = b.o;
    if (o.octl[OCTL_BAD] || o.row_off[r + 1] == o.row_off[r]) return;
    const uint8_t *rec = out_rec(b, r);
    uint8_t *dst = o.stream + o.carry_in + o.row_off[r];
    record_copy(dst, rec, o.new_ncig[r], lane);
    if (lane == 0) record_head(dst, rec, o.new_pos[r], o.new_ncig[r], out_new_cig(b, r));
}

}  // namespace ampbgzf

#ifndef AMPBGZF_HOSTSIM
CODEC_KERNEL(k_bamout_size, lane_out_size)
// One wave per row (four a workgroup): a record's name and tail are a few hundred bytes, eight per lane and step.
__global__ void __launch_bounds__(256) k_bamout_records(Buf b) {
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < b.o.n_rows; r += (int64_t)gridDim.x * 4) lane_out_record(b, r, lane);
}
static int out_records(amp_bam *s) {
    if (s->b.o.n_rows > 0) {
        k_bamout_records<<<codec_grid(s->b.o.n_rows * 64), 256, 0, s->sh.stream>>>(s->b);
        if (hipGetLastError() != hipSuccess) return AMP_EHIP;
    }
    return AMP_OK;
}
#else
static int out_records(amp_bam *s) {
    for (int64_t r = 0; r < s->b.o.n_rows; ++r) for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) lane_out_record(s->b, r, lane);
    return AMP_OK;
}
#endif

extern "C" {

// ampbam_write_rows + flush_blocks for the rows of the last feed (none when it was encoded already: a bare flush)
int amp_bam_encode(amp_bam *s, int32_t min_length, int32_t include_no_primer, int32_t final, amp_bam_out_info *info) {
    if (!s || !info) return AMP_EINVAL;
    const bool fresh = s->fed && !s->encoded && !s->info.n_refused && !s->info.bad_record;
    const int64_t n_rows = fresh ? s->info.n_rows : 0;
    if (n_rows && !s->processed) return AMP_ESTATE;
    DevGuard guard(s->sh);
    const int64_t waits0 = s->sh.waits;
    Buf &b = s->b;
    Out &o = b.o;
    // the new records: every record of the image at most, twelve bytes more per row (three CIGAR words)
    CODEC_OK(tail_begin(s->sh, s->tail, o, n_rows, n_rows ? b.n_img + 4 * (int64_t)OUT_SPARE_OPS * n_rows : 0, final, 8));
    o.new_pos = s->trim.new_pos; o.new_ncig = s->trim.new_ncig; o.new_cig = s->trim.new_cig; o.ref_len = s->trim.ref_len; o.trim_flags = s->trim.trim_flags;
    o.good_rows = n_rows ? s->good_rows : 0;
    o.min_length = min_length; o.include_no_primer = include_no_primer ? 1 : 0;
    if (n_rows) {
        CODEC_RUN(s, k_bamout_size, lane_out_size, n_rows + 1, -1);
        CODEC_OK(codec_scan(s->sh, o.row_off, n_rows + 1));
    }
    CODEC_OK(tail_plan<amp_bam>(s->sh, o));
    CODEC_OK(out_records(s));
    CODEC_OK(tail_finish<amp_bam>(s->sh, s->tail, o, 8, waits0, info));
    if (fresh) s->encoded = true;
    return AMP_OK;
}

// the framed blocks of the last encode, back to back: file_bytes of them (the blocks handed to the host left out)
int amp_bam_encoded_to_host(amp_bam *s, uint8_t *dst, int64_t cap) { return s ? tail_encoded_to_host(s->sh, s->tail, s->b.o, dst, cap, 12) : AMP_EINVAL; }

// the size of every block of the last encode in the file; 0: handed to the host, which takes its bytes from the stream
int amp_bam_encoded_blocks(amp_bam *s, uint32_t *blk_len, int64_t cap) { return s ? tail_encoded_blocks(s->sh, s->tail, s->b.o, blk_len, cap) : AMP_EINVAL; }

// n bytes from offset `from` of the uncompressed stream [carry | records] of the last encode: tests, and the host's fallback
int amp_bam_stream_to_host(amp_bam *s, int64_t from, int64_t n, uint8_t *dst) { return s ? tail_stream_to_host(s->sh, s->tail, s->b.o, from, n, dst) : AMP_EINVAL; }

#ifdef AMPBGZF_HOSTSIM
// Entry points of the host twin alone (not part of include/amplihip.h).  The twin has neither read pass nor DEFLATE encoder: the
// results of the last feed's rows as amp_trim_out lays them out (row r's CIGAR words at cig_off[r] + 3 r; first_bad < 0: no
// failing row), kept by the caller until the encode, and the encoder (amp_deflate.hip's host phases, ampdf_hostsim_blocks)
int amp_bam_twin_set_trim(amp_bam *s, const int32_t *new_pos, const uint32_t *new_ncig, const uint32_t *new_cig, const int32_t *ref_len,
                          const uint8_t *trim_flags, int64_t first_bad) {
    if (!s || !s->fed) return AMP_ESTATE;
    s->trim = Trim{new_pos, new_ncig, new_cig, ref_len, trim_flags, nullptr};
    s->good_rows = first_bad >= 0 ? first_bad : s->info.n_rows;
    s->processed = true;
    return AMP_OK;
}
// 0 when no encode so far wrote behind one of its buffers (the guard bytes carve_out leaves there), else 1 + the buffer's number
int amp_bam_twin_guards(amp_bam *s) { return s ? tail_guards(s->tail) : AMP_EINVAL; }
int amp_bam_twin_set_deflater(amp_bam *s, amp_bam_twin_deflate_fn fn) {
    if (!s) return AMP_EINVAL;
    s->tail.twin_deflate = fn;
    return AMP_OK;
}
#endif

}  // extern "C"
