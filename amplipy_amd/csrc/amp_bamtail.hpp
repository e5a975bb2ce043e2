// amp_bamtail.hpp -- from a stream of BAM records in HBM to framed BGZF blocks: the tail both device encoders of trimmed BAM share
// (amp_bamout.hip behind BAM input; amp_sam.hip behind SAM text, section 13).  A codec sizes its records,
// has the sizes summed into Out::row_off and writes the records behind the carry into Out::stream; everything else is here:
//   plan     one lane: stream bytes, how many of them are whole 0xFF00-byte chunks (all of them on the final call), the carry
//   deflate  amp_deflate_blocks_device_counted: the encoder of section 9 on the chunks, their number read from the plan
//   crc      one wave per chunk (crc_lane of amp_bgzf.hpp), the value stored
//   frame    lane = chunk: header, BSIZE, CRC-32, ISIZE; block lengths, their exclusive sum
//   gather   one wave per chunk: the framed blocks back to back, so that one copy brings exactly the file's bytes
// and the buffers of an encode (carve_out), the carry across calls, the counters' way down with the one wait of an encode, and
// the copies tests and the host's fallback ask for.  The order of a codec's encode:
//   tail_begin -> its sizes and their sum -> tail_plan -> its records -> tail_finish
// Every launch is sized by what the host knows (rows, a bound of the stream) and trimmed on the device by the plan's counters.
//
// The kernels are templates on the codec's struct: each codec's translation unit gets its own instances.
// BGZ_HD is defined by the including unit (AMP_HD) in front of this header.
#pragma once

#include <utility>
#include <vector>

#include "amp_codec.hpp"
#include "amp_bgzf.hpp"
#include "amp_bamout.hpp"

namespace ampbamout {

BGZ_HD void lane_out_plan(const Out &o) {
    const uint64_t total = (uint64_t)o.carry_in + (o.octl[OCTL_BAD] ? 0ull : o.row_off[o.n_rows]);
    const uint64_t enc = o.final ? total : total - total % OUT_BS;
    o.octl[OCTL_TOTAL] = total; o.octl[OCTL_ENC] = enc; o.octl[OCTL_CHUNKS] = (enc + OUT_BS - 1) / OUT_BS; o.octl[OCTL_CARRY] = total - enc;
}

BGZ_HD uint32_t lane_out_crc(const Out &o, int64_t k, uint32_t lane, const uint32_t *tab) {
    return ampbgzf::crc_lane(o.stream + (uint64_t)k * OUT_BS, chunk_len(o.octl[OCTL_ENC], (uint64_t)k), lane, tab);
}

BGZ_HD void lane_out_frame(const Out &o, int64_t k) {             // k == nb_max: the slot the scan leaves the total in
    uint32_t n = 0;
    if (k < (int64_t)o.octl[OCTL_CHUNKS]) {
        const uint32_t clen = o.clen[k];
        if (clen == 0 || clen > OUT_ROOM) AMP_ADD64(&o.octl[OCTL_HOST], 1);
        else n = frame_block(o.comp + (uint64_t)k * OUT_STRIDE, clen, o.crc[k], chunk_len(o.octl[OCTL_ENC], (uint64_t)k));
    }
    o.blk_len[k] = n; o.blk_off[k] = n;
}

BGZ_HD void lane_out_gather(const Out &o, int64_t k, uint32_t lane) {
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

// What an encoder keeps between its calls, beside the Out in its Buf.  The buffers grow to the largest piece and are not freed
// during a run.
struct Tail {
    uint8_t *oarena = nullptr, *ocarry = nullptr;
    size_t cap_oarena = 0, cap_ocarry = 0;
    int64_t oarena_rows = 0, oarena_stream = 0, oarena_blocks = 0;
    int64_t ocarry_len = 0;                           // bytes of the record stream behind its last whole 0xFF00-byte chunk, kept in `ocarry`
    bool out_ok = false;                              // the last encode stands: its stream, blocks and info can be asked for
    amp_bam_out_info oinfo{};
    unsigned long long h_octl[OCTL_WORDS];
#ifdef AMP_CODEC_HOSTSIM
    amp_bam_twin_deflate_fn twin_deflate = nullptr;
    Guards guards;                                    // the bytes behind the encoder's buffers, which nothing may write
#endif
};

#ifndef AMP_CODEC_HOSTSIM
template <class Tag> __global__ void __launch_bounds__(64) k_out_plan(Out o) { if (threadIdx.x == 0) lane_out_plan(o); }
template <class Tag> __global__ void __launch_bounds__(256) k_out_frame(Out o, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) lane_out_frame(o, k);
}
// One wave per chunk; the byte table of the CRC in LDS (k_bgzf_crc with the value stored instead of compared).
template <class Tag> __global__ void __launch_bounds__(256) k_out_crc(Out o) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = ampbgzf::crc_table_entry(threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t n = (int64_t)o.octl[OCTL_CHUNKS];
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * 4) {
        uint32_t reg = lane_out_crc(o, k, lane, tab);
        for (int d = 32; d >= 1; d >>= 1) reg ^= __shfl_xor(reg, d, 64);
        if (lane == 0) o.crc[k] = ~reg;
    }
}
template <class Tag> __global__ void __launch_bounds__(256) k_out_gather(Out o) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t n = (int64_t)o.octl[OCTL_CHUNKS];
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * 4) lane_out_gather(o, k, lane);
}
#define OUT_LAUNCHED() do { if (hipGetLastError() != hipSuccess) return AMP_EHIP; } while (0)

template <class Tag> static int tail_plan(ampcodec::Shell &sh, const Out &o) {
    k_out_plan<Tag><<<1, 64, 0, sh.stream>>>(o);
    OUT_LAUNCHED();
    return AMP_OK;
}
template <class Tag> static int tail_blocks(ampcodec::Shell &sh, Tail &, const Out &o, int mark) {
    CODEC_OK(amp_deflate_blocks_device_counted(sh.device, o.stream, (const uint64_t *)&o.octl[OCTL_ENC], o.nb_max * (int64_t)OUT_BS, (int32_t)OUT_BS,
                                               o.comp + 18, (int64_t)OUT_STRIDE, (int32_t)OUT_ROOM, o.clen, (void *)sh.stream));
    ampcodec::codec_mark(sh, mark);
    k_out_crc<Tag><<<ampcodec::codec_grid(o.nb_max * 64), 256, 0, sh.stream>>>(o);
    OUT_LAUNCHED();
    k_out_frame<Tag><<<ampcodec::codec_grid(o.nb_max + 1), 256, 0, sh.stream>>>(o, o.nb_max + 1);
    OUT_LAUNCHED();
    CODEC_OK(ampcodec::codec_scan(sh, o.blk_off, o.nb_max + 1));
    k_out_gather<Tag><<<ampcodec::codec_grid(o.nb_max * 64), 256, 0, sh.stream>>>(o);
    OUT_LAUNCHED();
    return AMP_OK;
}
#else
template <class Tag> static int tail_plan(ampcodec::Shell &, const Out &o) { lane_out_plan(o); return AMP_OK; }
template <class Tag> static int tail_blocks(ampcodec::Shell &sh, Tail &t, const Out &o, int) {
    const int64_t enc = (int64_t)o.octl[OCTL_ENC], n = (int64_t)o.octl[OCTL_CHUNKS];
    if (enc) {
        if (!t.twin_deflate) return AMP_ESTATE;
        if (t.twin_deflate(o.stream, enc, (int32_t)OUT_BS, o.comp + 18, (int64_t)OUT_STRIDE, (int32_t)OUT_ROOM, o.clen)) return AMP_EHIP;
    }
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = ampbgzf::crc_table_entry(i);
    for (int64_t k = 0; k < n; ++k) {
        uint32_t reg = 0;
        for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) reg ^= lane_out_crc(o, k, lane, tab);
        o.crc[k] = ~reg;
    }
    for (int64_t k = 0; k <= o.nb_max; ++k) lane_out_frame(o, k);
    CODEC_OK(ampcodec::codec_scan(sh, o.blk_off, o.nb_max + 1));
    for (int64_t k = 0; k < n; ++k) for (uint32_t lane = 0; lane < OUT_WAVE; ++lane) lane_out_gather(o, k, lane);
    return AMP_OK;
}
#endif

static int tail_ensure(ampcodec::Shell &sh, Tail &t, Out &o, int64_t rows, int64_t stream, int64_t blocks) {
    using namespace ampcodec;
    if (!t.ocarry) CODEC_OK(codec_grow(sh, &t.ocarry, &t.cap_ocarry, (size_t)OUT_BS + 64));
    if (!t.oarena || rows > t.oarena_rows || stream > t.oarena_stream || blocks > t.oarena_blocks) {
        const int64_t cr = rows > t.oarena_rows ? rows + rows / 8 + 64 : t.oarena_rows;
        const int64_t cs = stream > t.oarena_stream ? stream + stream / 8 + 4096 : t.oarena_stream;
        const int64_t cb = blocks > t.oarena_blocks ? blocks + blocks / 8 + 4 : t.oarena_blocks;
        Out probe = o;
        const size_t need = carve_out(probe, nullptr, cr, cs, cb, nullptr);
        CODEC_OK(codec_grow(sh, &t.oarena, &t.cap_oarena, need));
#ifdef AMP_CODEC_HOSTSIM
        t.guards.clear();
        (void)carve_out(o, t.oarena, cr, cs, cb, &t.guards);
        for (const auto &g : t.guards) memset(g.first, 0xA5, g.second);
#else
        (void)carve_out(o, t.oarena, cr, cs, cb, nullptr);
#endif
        t.oarena_rows = cr; t.oarena_stream = cs; t.oarena_blocks = cb;
    }
    return AMP_OK;
}

// Opens an encode of n_rows rows whose records take at most `new_bytes` bytes: the buffers, the Out's sizes, the counters zeroed
// and the carry in front of the stream.  mark: the stage event of the encode's begin.
static int tail_begin(ampcodec::Shell &sh, Tail &t, Out &o, int64_t n_rows, int64_t new_bytes, int final, int mark) {
    using namespace ampcodec;
    const int64_t carry = t.ocarry_len, bound = carry + new_bytes, nb_max = bound / (int64_t)OUT_BS + 1;
    CODEC_OK(tail_ensure(sh, t, o, n_rows, bound, nb_max));
    o.n_rows = n_rows; o.carry_in = carry; o.nb_max = nb_max; o.final = final ? 1 : 0;
    t.out_ok = false;
    codec_mark(sh, mark);
    CODEC_OK(codec_zero(sh, o.octl, 0, OCTL_WORDS * 8));
    CODEC_OK(codec_zero(sh, o.row_off, 0, 8));
    CODEC_OK(codec_d2d(sh, o.stream, t.ocarry, (size_t)carry));
    return AMP_OK;
}

// Behind the records: the blocks, the counters' way down, the one wait, the carry for the next call.  mark + 1 .. mark + 3: the
// stage events in front of DEFLATE, of CRC and framing, of the copy down.  AMP_EINVAL when the codec counted a row it cannot
// write (OCTL_BAD): nothing of this call was appended, the carry stands.
template <class Tag> static int tail_finish(ampcodec::Shell &sh, Tail &t, const Out &o, int mark, int64_t waits0, amp_bam_out_info *info) {
    using namespace ampcodec;
    codec_mark(sh, mark + 1);
    CODEC_OK(tail_blocks<Tag>(sh, t, o, mark + 2));
    codec_mark(sh, mark + 3);
    unsigned long long *c = t.h_octl;
    CODEC_OK(codec_down(sh, c, o.octl, OCTL_WORDS * 8));
    CODEC_OK(codec_wait(sh));
    if (c[OCTL_BAD]) return AMP_EINVAL;
    // the bytes behind the last whole chunk open the next call's stream (a device-to-device copy of less than one chunk)
    CODEC_OK(codec_d2d(sh, t.ocarry, o.stream + c[OCTL_ENC], (size_t)c[OCTL_CARRY]));
    t.ocarry_len = (int64_t)c[OCTL_CARRY];
    amp_bam_out_info &I = t.oinfo;
    I.n_rows_written = (int64_t)c[OCTL_ROWS]; I.stream_bytes = (int64_t)c[OCTL_TOTAL]; I.carry_in = o.carry_in; I.carry_out = (int64_t)c[OCTL_CARRY];
    I.n_blocks = (int64_t)c[OCTL_CHUNKS]; I.file_bytes = (int64_t)c[OCTL_FILE]; I.n_blocks_host = (int64_t)c[OCTL_HOST];
    I.waits = sh.waits - waits0; I.bytes_down = OCTL_WORDS * 8 + I.file_bytes;
    t.out_ok = true;
    *info = I;
    return AMP_OK;
}

// the framed blocks of the last encode, back to back: file_bytes of them (the blocks handed to the host left out)
static int tail_encoded_to_host(ampcodec::Shell &sh, Tail &t, const Out &o, uint8_t *dst, int64_t cap, int mark) {
    using namespace ampcodec;
    if (cap < 0 || (cap && !dst)) return AMP_EINVAL;
    if (!t.out_ok) return AMP_ESTATE;
    if (cap < t.oinfo.file_bytes) return AMP_EOVERFLOW;
    DevGuard guard(sh);
    CODEC_OK(codec_down(sh, dst, o.dense, (size_t)t.oinfo.file_bytes));
    codec_mark(sh, mark);
    return codec_wait(sh);
}
// the size of every block of the last encode in the file; 0: handed to the host, which takes its bytes from the stream
static int tail_encoded_blocks(ampcodec::Shell &sh, Tail &t, const Out &o, uint32_t *blk_len, int64_t cap) {
    using namespace ampcodec;
    if (cap < 0 || (cap && !blk_len)) return AMP_EINVAL;
    if (!t.out_ok) return AMP_ESTATE;
    if (cap < t.oinfo.n_blocks) return AMP_EOVERFLOW;
    DevGuard guard(sh);
    CODEC_OK(codec_down(sh, blk_len, o.blk_len, (size_t)t.oinfo.n_blocks * 4));
    return codec_wait(sh);
}
// n bytes from offset `from` of the uncompressed stream [carry | records] of the last encode: tests, and the host's fallback
static int tail_stream_to_host(ampcodec::Shell &sh, Tail &t, const Out &o, int64_t from, int64_t n, uint8_t *dst) {
    using namespace ampcodec;
    if (from < 0 || n < 0 || (n && !dst)) return AMP_EINVAL;
    if (!t.out_ok) return AMP_ESTATE;
    if (from + n > t.oinfo.stream_bytes) return AMP_EOVERFLOW;
    DevGuard guard(sh);
    CODEC_OK(codec_down(sh, dst, o.stream + from, (size_t)n));
    return codec_wait(sh);
}
static void tail_free(Tail &t) { ampcodec::codec_free(t.oarena); ampcodec::codec_free(t.ocarry); }

#ifdef AMP_CODEC_HOSTSIM
// 0 when no encode so far wrote behind one of its buffers (the guard bytes carve_out leaves there), else 1 + the buffer's number
static int tail_guards(const Tail &t) {
    for (size_t k = 0; k < t.guards.size(); ++k)
        for (size_t i = 0; i < t.guards[k].second; ++i) if (t.guards[k].first[i] != 0xA5) return 1 + (int)k;
    return 0;
}
#endif

}  // namespace ampbamout
