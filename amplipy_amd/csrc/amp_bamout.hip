// amp_bamout.hip -- the device re-encoder of trimmed BAM records: what lets `trim` and `aio` stay on the
// device codec for BAM input.  Part of amp_bgzf.hip's translation unit (included there behind struct amp_bam, whose image,
// record offsets, batch and Trim arrays it reads); the lane functions are in amp_bamout.hpp.
//
// The host codec writes trimmed reads with ampbam_write_rows (out_aln.write, AmpliPy.py:911): the unchanged parts of every kept
// record copied from the piece's host image, 0xFF00-byte chunks of the record stream compressed and framed by flush_blocks.
// Here the same bytes are made in HBM, per piece, on the ctx stream, behind amp_bam_process:
//   sizes    lane = row: keep (A:910, rows in front of the first failing one), the new record's size; a 64-bit exclusive sum
//   plan     one lane: stream bytes, how many of them are whole chunks (all of them on the final call), the carry
//   records  one wave per kept row: name and tail by wide loads and stores, one lane the 36 fixed bytes and the CIGAR words
//   deflate  amp_deflate_blocks_device_counted: the encoder of section 9 on the chunks, their number read from the plan
//   crc      one wave per chunk (crc_lane of amp_bgzf.hpp), the value stored
//   frame    lane = chunk: header, BSIZE, CRC-32, ISIZE; block lengths, their exclusive sum
//   gather   one wave per chunk: the framed blocks back to back, so that one copy brings exactly the file's bytes
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

BGZ_HD void lane_out_plan(const Buf &b, int64_t) {
    const Out &o = b.o;
    const uint64_t total = (uint64_t)o.carry_in + (o.octl[OCTL_BAD] ? 0ull : o.row_off[o.n_rows]);
    const uint64_t enc = o.final ? total : total - total % OUT_BS;
    o.octl[OCTL_TOTAL] = total; o.octl[OCTL_ENC] = enc; o.octl[OCTL_CHUNKS] = (enc + OUT_BS - 1) / OUT_BS; o.octl[OCTL_CARRY] = total - enc;
}

BGZ_HD void lane_out_record(const Buf &b, int64_t r, uint32_t lane) {
    const Out &o = b.o;
    if (o.octl[OCTL_BAD] || o.row_off[r + 1] == o.row_off[r]) return;
    const uint8_t *rec = out_rec(b, r);
    uint8_t *dst = o.stream + o.carry_in + o.row_off[r];
    record_copy(dst, rec, o.new_ncig[r], lane);
    if (lane == 0) record_head(dst, rec, o.new_pos[r], o.new_ncig[r], out_new_cig(b, r));
}

BGZ_HD uint32_t lane_out_crc(const Buf &b, int64_t k, uint32_t lane, const uint32_t *tab) {
    return crc_lane(b.o.stream + (uint64_t)k * OUT_BS, chunk_len(b.o.octl[OCTL_ENC], (uint64_t)k), lane, tab);
}

BGZ_HD void lane_out_frame(const Buf &b, int64_t k) {             // k == nb_max: the slot the scan leaves the total in
    const Out &o = b.o;
    uint32_t n = 0;
    if (k < (int64_t)o.octl[OCTL_CHUNKS]) {
        const uint32_t clen = o.clen[k];
        if (clen == 0 || clen > OUT_ROOM) AMP_ADD64(&o.octl[OCTL_HOST], 1);
        else n = frame_block(o.comp + (uint64_t)k * OUT_STRIDE, clen, o.crc[k], chunk_len(o.octl[OCTL_ENC], (uint64_t)k));
    }
    o.blk_len[k] = n; o.blk_off[k] = n;
}

BGZ_HD void lane_out_gather(const Buf &b, int64_t k, uint32_t lane) {
    const Out &o = b.o;
    wave_copy(o.dense + o.blk_off[k], o.comp + (uint64_t)k * OUT_STRIDE, o.blk_len[k], lane);
    if (lane == 0 && k + 1 == (int64_t)o.octl[OCTL_CHUNKS]) o.octl[OCTL_FILE] = (uint64_t)o.blk_off[k] + o.blk_len[k];
}

// Carves `base` (NULL: sizes only) for encodes of up to `rows` rows, `stream` stream bytes and `blocks` blocks; returns the bytes
// needed.  Behind every buffer lie 256 bytes and more that nothing may write: `guards` (the twin's) gets their places.
typedef std::vector<std::pair<uint8_t *, size_t>> Guards;
static size_t carve_out(Out &o, uint8_t *base, int64_t rows, int64_t stream, int64_t blocks, Guards *guards) {
    const size_t nb = (size_t)blocks;
    ampcodec::Carver take{base};
    auto buf = [&](size_t bytes) {
        uint8_t *p = take(bytes);
        (void)take(256);
        if (base && guards) guards->push_back({p + bytes, ampcodec::up256(bytes) - bytes + 256});
        return p;
    };
    o.row_off = (uint64_t *)buf(((size_t)rows + 2) * 8);
    o.stream = buf((size_t)stream + 64);
    o.comp = buf(nb * OUT_STRIDE); o.dense = buf(nb * 65536u + 64);
    uint32_t **per_block[] = {&o.clen, &o.crc, &o.blk_len, &o.blk_off};
    for (uint32_t **p : per_block) *p = (uint32_t *)buf((nb + 1) * 4);
    o.octl = (unsigned long long *)buf(OCTL_WORDS * 8);
    return take.o;
}

}  // namespace ampbgzf

#ifndef AMPBGZF_HOSTSIM
CODEC_KERNEL(k_bamout_size, lane_out_size)
CODEC_KERNEL(k_bamout_plan, lane_out_plan)
CODEC_KERNEL(k_bamout_frame, lane_out_frame)
// One wave per row (four a workgroup): a record's name and tail are a few hundred bytes, eight per lane and step.
__global__ void __launch_bounds__(256) k_bamout_records(Buf b) {
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < b.o.n_rows; r += (int64_t)gridDim.x * 4) lane_out_record(b, r, lane);
}
// One wave per chunk; the byte table of the CRC in LDS (k_bgzf_crc with the value stored instead of compared).
__global__ void __launch_bounds__(256) k_bamout_crc(Buf b) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t n = (int64_t)b.o.octl[OCTL_CHUNKS];
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * 4) {
        uint32_t reg = lane_out_crc(b, k, lane, tab);
        for (int d = 32; d >= 1; d >>= 1) reg ^= __shfl_xor(reg, d, 64);
        if (lane == 0) b.o.crc[k] = ~reg;
    }
}
__global__ void __launch_bounds__(256) k_bamout_gather(Buf b) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t n = (int64_t)b.o.octl[OCTL_CHUNKS];
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * 4) lane_out_gather(b, k, lane);
}
#define OUT_WAVES(s, kern, n) do { if ((n) > 0) { kern<<<codec_grid((int64_t)(n) * 64), 256, 0, (s)->sh.stream>>>((s)->b); if (hipGetLastError() != hipSuccess) return AMP_EHIP; } } while (0)

static int out_deflate(amp_bam *s) {
    const Out &o = s->b.o;
    return amp_deflate_blocks_device_counted(s->sh.device, o.stream, (const uint64_t *)&o.octl[OCTL_ENC], o.nb_max * (int64_t)OUT_BS, (int32_t)OUT_BS,
                                             o.comp + 18, (int64_t)OUT_STRIDE, (int32_t)OUT_ROOM, o.clen, (void *)s->sh.stream);
}
static int out_records(amp_bam *s) { OUT_WAVES(s, k_bamout_records, s->b.o.n_rows); return AMP_OK; }
static int out_crc(amp_bam *s) { OUT_WAVES(s, k_bamout_crc, s->b.o.nb_max); return AMP_OK; }
static int out_gather(amp_bam *s) { OUT_WAVES(s, k_bamout_gather, s->b.o.nb_max); return AMP_OK; }
#else
static int out_deflate(amp_bam *s) {
    const Out &o = s->b.o;
    const int64_t enc = (int64_t)o.octl[OCTL_ENC];
    if (!enc) return AMP_OK;
    if (!s->twin_deflate) return AMP_ESTATE;
    return s->twin_deflate(o.stream, enc, (int32_t)OUT_BS, o.comp + 18, (int64_t)OUT_STRIDE, (int32_t)OUT_ROOM, o.clen) ? AMP_EHIP : AMP_OK;
}
static int out_records(amp_bam *s) {
    for (int64_t r = 0; r < s->b.o.n_rows; ++r) for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) lane_out_record(s->b, r, lane);
    return AMP_OK;
}
static int out_crc(amp_bam *s) {
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i);
    for (int64_t k = 0; k < (int64_t)s->b.o.octl[OCTL_CHUNKS]; ++k) {
        uint32_t reg = 0;
        for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) reg ^= lane_out_crc(s->b, k, lane, tab);
        s->b.o.crc[k] = ~reg;
    }
    return AMP_OK;
}
static int out_gather(amp_bam *s) {
    for (int64_t k = 0; k < (int64_t)s->b.o.octl[OCTL_CHUNKS]; ++k) for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) lane_out_gather(s->b, k, lane);
    return AMP_OK;
}
#endif

// the buffers of the encoder belong to the amp_bam, grow to the largest piece and are not freed during a run
static int out_ensure(amp_bam *s, int64_t rows, int64_t stream, int64_t blocks) {
    if (!s->ocarry) CODEC_OK(codec_grow(s->sh, &s->ocarry, &s->cap_ocarry, (size_t)OUT_BS + 64));
    if (!s->oarena || rows > s->oarena_rows || stream > s->oarena_stream || blocks > s->oarena_blocks) {
        const int64_t cr = rows > s->oarena_rows ? rows + rows / 8 + 64 : s->oarena_rows;
        const int64_t cs = stream > s->oarena_stream ? stream + stream / 8 + 4096 : s->oarena_stream;
        const int64_t cb = blocks > s->oarena_blocks ? blocks + blocks / 8 + 4 : s->oarena_blocks;
        Out probe = s->b.o;
        const size_t need = carve_out(probe, nullptr, cr, cs, cb, nullptr);
        CODEC_OK(codec_grow(s->sh, &s->oarena, &s->cap_oarena, need));
#ifdef AMPBGZF_HOSTSIM
        s->guards.clear();
        (void)carve_out(s->b.o, s->oarena, cr, cs, cb, &s->guards);
        for (const auto &g : s->guards) memset(g.first, 0xA5, g.second);
#else
        (void)carve_out(s->b.o, s->oarena, cr, cs, cb, nullptr);
#endif
        s->oarena_rows = cr; s->oarena_stream = cs; s->oarena_blocks = cb;
    }
    return AMP_OK;
}

extern "C" {

// ampbam_write_rows + flush_blocks for the rows of the last feed (none when it was encoded already: a bare flush)
int amp_bam_encode(amp_bam *s, int32_t min_length, int32_t include_no_primer, int32_t final, amp_bam_out_info *info) {
    if (!s || !info) return AMP_EINVAL;
    const bool fresh = s->fed && !s->encoded && !s->info.n_refused && !s->info.bad_record;
    const int64_t n_rows = fresh ? s->info.n_rows : 0;
    if (n_rows && !s->processed) return AMP_ESTATE;
    DevGuard guard(s->sh);
    const int64_t waits0 = s->sh.waits, carry = s->ocarry_len;
    // the stream: the carry, every record of the image at most, twelve bytes more per row (three CIGAR words)
    const int64_t bound = carry + (n_rows ? s->b.n_img + 4 * (int64_t)OUT_SPARE_OPS * n_rows : 0);
    const int64_t nb_max = bound / (int64_t)OUT_BS + 1;
    CODEC_OK(out_ensure(s, n_rows, bound, nb_max));
    Buf &b = s->b;
    Out &o = b.o;
    o.new_pos = s->trim.new_pos; o.new_ncig = s->trim.new_ncig; o.new_cig = s->trim.new_cig; o.ref_len = s->trim.ref_len; o.trim_flags = s->trim.trim_flags;
    o.n_rows = n_rows; o.good_rows = n_rows ? s->good_rows : 0; o.carry_in = carry; o.nb_max = nb_max;
    o.min_length = min_length; o.include_no_primer = include_no_primer ? 1 : 0; o.final = final ? 1 : 0;
    s->out_ok = false;
    codec_mark(s->sh, 8);
    CODEC_OK(codec_zero(s->sh, o.octl, 0, OCTL_WORDS * 8));
    CODEC_OK(codec_zero(s->sh, o.row_off, 0, 8));
    CODEC_OK(codec_d2d(s->sh, o.stream, s->ocarry, (size_t)carry));
    if (n_rows) {
        CODEC_RUN(s, k_bamout_size, lane_out_size, n_rows + 1, -1);
        CODEC_OK(codec_scan(s->sh, o.row_off, n_rows + 1));
    }
    CODEC_RUN(s, k_bamout_plan, lane_out_plan, 1, -1);
    CODEC_OK(out_records(s));
    codec_mark(s->sh, 9);
    CODEC_OK(out_deflate(s));
    codec_mark(s->sh, 10);
    CODEC_OK(out_crc(s));
    CODEC_RUN(s, k_bamout_frame, lane_out_frame, nb_max + 1, -1);
    CODEC_OK(codec_scan(s->sh, o.blk_off, nb_max + 1));
    CODEC_OK(out_gather(s));
    codec_mark(s->sh, 11);
    unsigned long long *c = s->h_octl;
    CODEC_OK(codec_down(s->sh, c, o.octl, OCTL_WORDS * 8));
    CODEC_OK(codec_wait(s->sh));
    if (c[OCTL_BAD]) return AMP_EINVAL;                                   // (nothing of this call was appended: the carry stands)
    // the bytes behind the last whole chunk open the next call's stream (a device-to-device copy of less than one chunk)
    CODEC_OK(codec_d2d(s->sh, s->ocarry, o.stream + c[OCTL_ENC], (size_t)c[OCTL_CARRY]));
    s->ocarry_len = (int64_t)c[OCTL_CARRY];
    if (fresh) s->encoded = true;
    amp_bam_out_info &I = s->oinfo;
    I.n_rows_written = (int64_t)c[OCTL_ROWS]; I.stream_bytes = (int64_t)c[OCTL_TOTAL]; I.carry_in = carry; I.carry_out = (int64_t)c[OCTL_CARRY];
    I.n_blocks = (int64_t)c[OCTL_CHUNKS]; I.file_bytes = (int64_t)c[OCTL_FILE]; I.n_blocks_host = (int64_t)c[OCTL_HOST];
    I.waits = s->sh.waits - waits0; I.bytes_down = OCTL_WORDS * 8 + I.file_bytes;
    s->out_ok = true;
    *info = I;
    return AMP_OK;
}

// the framed blocks of the last encode, back to back: file_bytes of them (the blocks handed to the host left out)
int amp_bam_encoded_to_host(amp_bam *s, uint8_t *dst, int64_t cap) {
    if (!s || cap < 0 || (cap && !dst)) return AMP_EINVAL;
    if (!s->out_ok) return AMP_ESTATE;
    if (cap < s->oinfo.file_bytes) return AMP_EOVERFLOW;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, dst, s->b.o.dense, (size_t)s->oinfo.file_bytes));
    codec_mark(s->sh, 12);
    return codec_wait(s->sh);
}

// the size of every block of the last encode in the file; 0: handed to the host, which takes its bytes from the stream
int amp_bam_encoded_blocks(amp_bam *s, uint32_t *blk_len, int64_t cap) {
    if (!s || cap < 0 || (cap && !blk_len)) return AMP_EINVAL;
    if (!s->out_ok) return AMP_ESTATE;
    if (cap < s->oinfo.n_blocks) return AMP_EOVERFLOW;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, blk_len, s->b.o.blk_len, (size_t)s->oinfo.n_blocks * 4));
    return codec_wait(s->sh);
}

// n bytes from offset `from` of the uncompressed stream [carry | records] of the last encode: tests, and the host's fallback
int amp_bam_stream_to_host(amp_bam *s, int64_t from, int64_t n, uint8_t *dst) {
    if (!s || from < 0 || n < 0 || (n && !dst)) return AMP_EINVAL;
    if (!s->out_ok) return AMP_ESTATE;
    if (from + n > s->oinfo.stream_bytes) return AMP_EOVERFLOW;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, dst, s->b.o.stream + from, (size_t)n));
    return codec_wait(s->sh);
}

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
int amp_bam_twin_guards(amp_bam *s) {
    if (!s) return AMP_EINVAL;
    for (size_t k = 0; k < s->guards.size(); ++k)
        for (size_t i = 0; i < s->guards[k].second; ++i) if (s->guards[k].first[i] != 0xA5) return 1 + (int)k;
    return 0;
}
int amp_bam_twin_set_deflater(amp_bam *s, amp_bam_twin_deflate_fn fn) {
    if (!s) return AMP_EINVAL;
    s->twin_deflate = fn;
    return AMP_OK;
}
#endif

}  // extern "C"
