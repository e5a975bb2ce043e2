// amp_bamout.hpp -- what one lane does when trimmed BAM records are re-encoded and framed as BGZF on the device (amp_bamout.hip,
// DESIGN.md section 12): the size of a re-encoded record, the wave's copy of its unchanged parts, the one lane's 36 fixed bytes
// and CIGAR words, and the 26 bytes a BGZF block has around its DEFLATE stream.  The bytes are ampbam_write_rows' (ampbam.cpp;
// out_aln.write at AmpliPy.py:911) and flush_blocks' for the same results.
//
// Plain C++ on raw pointers: compiles for HIP (BGZ_HD = __host__ __device__) and with any host compiler, sanitizers included
// (tests/hostsim/bamout_fuzz.cpp).  A function writes exactly the bytes it names and reads exactly the record it is given.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef BGZ_HD
#define BGZ_HD static inline
#endif

namespace ampbamout {

enum : uint32_t {
    OUT_BS = 0xFF00u,                  // uncompressed bytes of a BGZF block: the host writer's (flush_blocks)
    OUT_STRIDE = 65536u + 64u,         // a framed block's slot; its DEFLATE stream starts 18 bytes in
    OUT_ROOM = 65536u - 26u,           // what a BGZF block can hold of a stream
    OUT_WAVE = 64u,
    OUT_SPARE_OPS = 3u                 // a trimmed CIGAR has at most three ops more than the read's (amp_trim_out)
};

// counters of one encode, in device memory; all of them come down with the one wait
enum { OCTL_TOTAL = 0,     // bytes of the stream [carry | this call's records]
       OCTL_ENC,           // ... of them compressed now: whole blocks, or everything on the final call
       OCTL_CHUNKS,        // blocks
       OCTL_CARRY,         // bytes left for the next call
       OCTL_ROWS,          // rows written
       OCTL_FILE,          // bytes of the framed blocks
       OCTL_HOST,          // blocks whose stream did not fit (handed to the host)
       OCTL_BAD,           // rows with a CIGAR of more than 65,535 ops: ampbam_write_rows refuses the batch
       OCTL_WORDS = 16 };

// every pointer of one encode: device memory in the library, host memory in the twin
struct Out {
    const int32_t *new_pos; const uint32_t *new_ncig, *new_cig; const int32_t *ref_len; const uint8_t *trim_flags;
    int64_t n_rows, good_rows, carry_in, nb_max;
    int32_t min_length, include_no_primer, final, pad;
    uint64_t *row_off;                 // [n_rows + 1]: sizes, then their exclusive sum
    uint8_t *stream, *comp, *dense;    // [carry | records]; nb_max slots of OUT_STRIDE; the framed blocks back to back
    uint32_t *clen, *crc, *blk_len, *blk_off;
    unsigned long long *octl;
};

BGZ_HD uint32_t o_rd32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
BGZ_HD uint32_t o_rd16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
BGZ_HD void o_wr32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
BGZ_HD void o_wr16(uint8_t *p, uint32_t v) { const uint16_t h = (uint16_t)v; __builtin_memcpy(p, &h, 2); }
BGZ_HD uint64_t o_load8(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
BGZ_HD void o_store8(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }

// n bytes by the 64 lanes of a wave, 8 per lane and step, unaligned on both sides; the last n % 8 one per lane
BGZ_HD void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    for (uint32_t o = lane * 8u; o + 8u <= n; o += OUT_WAVE * 8u) o_store8(dst + o, o_load8(src + o));
    const uint32_t tail = n & ~7u;
    if (tail + lane < n) dst[tail + lane] = src[tail + lane];
}

// SAMv1 5.3: bin of the 0-based half-open interval [beg, end)
BGZ_HD uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// A:910
BGZ_HD bool row_kept(int32_t ref_len, uint8_t trim_flags, int32_t min_length, int32_t include_no_primer) {
    return ref_len >= min_length && ((trim_flags & 3u) || include_no_primer);
}

// rec = a record of the image, from its block_size word on
BGZ_HD uint32_t rec_old_ncig(const uint8_t *rec) { return o_rd16(rec + 4 + 12); }
BGZ_HD bool ncig_fits(const uint8_t *rec, uint32_t new_ncig) { return new_ncig <= 65535u && new_ncig <= rec_old_ncig(rec) + OUT_SPARE_OPS; }
// bytes of the record with new_ncig CIGAR ops, its block_size word included
BGZ_HD uint64_t record_size(const uint8_t *rec, uint32_t new_ncig) {
    return 4ull + o_rd32(rec) - 4ull * rec_old_ncig(rec) + 4ull * new_ncig;
}

// one lane: block_size, the 32 fixed bytes with the new pos, bin and n_cigar_op, and the CIGAR words behind the name
BGZ_HD void record_head(uint8_t *o, const uint8_t *rec, int32_t new_pos, uint32_t nn, const uint32_t *cg) {
    const uint32_t bs = o_rd32(rec), l_name = rec[4 + 8], old_n = rec_old_ncig(rec);
    o_wr32(o, bs - 4u * old_n + 4u * nn);
    for (int k = 0; k < 4; ++k) o_store8(o + 4 + 8 * k, o_load8(rec + 4 + 8 * k));
    int64_t rlen = 0;
    for (uint32_t k = 0; k < nn; ++k) {
        const uint32_t op = cg[k] & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += cg[k] >> 4;
    }
    const int64_t pos = new_pos, end = pos + (rlen ? rlen : 1);
    o_wr32(o + 4 + 4, (uint32_t)new_pos);
    o_wr16(o + 4 + 10, reg2bin(pos > 0 ? pos : 0, end > 1 ? end : 1));
    o_wr16(o + 4 + 12, nn);
    uint8_t *c = o + 36 + l_name;
    for (uint32_t k = 0; k < nn; ++k) o_wr32(c + 4 * k, cg[k]);
}

// the wave: the name, and the tail (packed bases, qualities, aux) behind the new CIGAR
BGZ_HD void record_copy(uint8_t *o, const uint8_t *rec, uint32_t nn, uint32_t lane) {
    const uint32_t bs = o_rd32(rec), l_name = rec[4 + 8], old_n = rec_old_ncig(rec);
    wave_copy(o + 36, rec + 36, l_name, lane);
    const uint32_t tail_from = 32u + l_name + 4u * old_n;
    wave_copy(o + 36 + l_name + 4u * nn, rec + 4 + tail_from, bs - tail_from, lane);
}

// bytes of chunk k of `enc` compressed bytes
BGZ_HD uint32_t chunk_len(uint64_t enc, uint64_t k) { return (uint32_t)(enc - k * OUT_BS < OUT_BS ? enc - k * OUT_BS : OUT_BS); }

// The 26 bytes around a DEFLATE stream of clen bytes that lies at blk + 18: gzip header with the BC subfield (BSIZE = block
// size - 1), CRC-32 and ISIZE.  Returns the block's size.
BGZ_HD uint32_t frame_block(uint8_t *blk, uint32_t clen, uint32_t crc, uint32_t isize) {
    const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int k = 0; k < 16; ++k) blk[k] = hdr[k];
    o_wr16(blk + 16, clen + 25u);
    o_wr32(blk + 18 + clen, crc);
    o_wr32(blk + 18 + clen + 4, isize);
    return clen + 26u;
}

}  // namespace ampbamout

// The DEFLATE encoder of the host twin's encodes (amp_bam_twin_set_deflater of amp_bamout.hip): amp_deflate_blocks without its device.
typedef int (*amp_bam_twin_deflate_fn)(const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_stride,
                                       int32_t out_room, uint32_t *out_len);
