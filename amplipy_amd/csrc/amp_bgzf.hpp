// amp_bgzf.hpp -- the lane functions of the opt-in device codec for BAM input (amp_bgzf.hip): inflate of
// one BGZF block's raw DEFLATE stream, the block's CRC-32 by 64 lanes, and the BAM record tests of the record index.
//
// Everything here compiles for the device and for the host (the includer defines BGZ_HD: __host__ __device__ for hipcc,
// static inline for the twin built with -DAMPBGZF_HOSTSIM, which needs no HIP and runs under the sanitizers).
//
// The decoder is amp_inflate.hpp's (libampbam's own: the output IS the window, the inflated size is known, a 64-bit bit
// buffer, two-level tables of 10 / 8 first-level bits) with every piece of state that is indexed at run time moved into one
// Tables object -- on the device that object lies in LDS, one per decoder, so nothing of it goes to scratch memory -- and
// without library calls.  Every write is checked against the end of the block's output range, every match distance against
// the bytes produced so far, every read against the end of the stream (missing bits read as zeros and are counted).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ampbgzf {

enum { LIT_TB = 10, DST_TB = 8, PRE_TB = 7, MAX_LEN = 15, N_LITLEN = 288, N_DIST = 32, N_PRE = 19 };
// table entry: bits 0-4 code length, bits 5-7 kind, bits 8-12 extra bits, bits 16-31 value (amp_inflate.hpp)
enum : uint32_t { K_LITERAL = 0u << 5, K_LENGTH = 1u << 5, K_EOB = 2u << 5, K_SUB = 3u << 5, K_INVALID = 4u << 5, K_MASK = 7u << 5 };

struct Tables {                                  // 13,344 bytes: twelve decoders in a CU's 160 KB of LDS
    uint32_t lit[(1 << LIT_TB) + 1024];
    uint32_t dst[(1 << DST_TB) + 512];
    uint32_t pre[1 << PRE_TB];
    uint32_t count[MAX_LEN + 1], next_code[MAX_LEN + 2], nc[MAX_LEN + 2];
    uint8_t lens[N_LITLEN + N_DIST], pl[N_PRE + 1], sub_bits[1 << LIT_TB];
    uint32_t fixed_built;                        // lit / dst hold the fixed code of RFC 1951 3.2.6
};

BGZ_HD uint32_t mk(uint32_t len, uint32_t kind, uint32_t extra, uint32_t value) { return len | kind | (extra << 8) | (value << 16); }
BGZ_HD uint32_t bit_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// base and extra bits of length symbol 257 + k and of distance symbol k (RFC 1951 3.2.5), computed: no table to index
BGZ_HD void len_code(int k, uint32_t &base, uint32_t &extra) {
    if (k < 8) { base = 3u + (uint32_t)k; extra = 0; return; }
    if (k == 28) { base = 258; extra = 0; return; }
    extra = (uint32_t)(k - 4) >> 2;
    base = 3u + ((4u + ((uint32_t)k & 3u)) << extra);
}
BGZ_HD void dst_code(int k, uint32_t &base, uint32_t &extra) {
    if (k < 4) { base = 1u + (uint32_t)k; extra = 0; return; }
    extra = (uint32_t)(k - 2) >> 1;
    base = 1u + ((2u + ((uint32_t)k & 1u)) << extra);
}

BGZ_HD uint32_t symbol_entry(int which, int sym, uint32_t len) {
    uint32_t base, extra;
    if (which == 2) return mk(len, K_LITERAL, 0, (uint32_t)sym);
    if (which == 1) { if (sym >= 30) return mk(len, K_INVALID, 0, 0); dst_code(sym, base, extra); return mk(len, K_LENGTH, extra, base); }
    if (sym < 256) return mk(len, K_LITERAL, 0, (uint32_t)sym);
    if (sym == 256) return mk(len, K_EOB, 0, 0);
    if (sym >= 286) return mk(len, K_INVALID, 0, 0);
    len_code(sym - 257, base, extra);
    return mk(len, K_LENGTH, extra, base);
}

// Canonical Huffman decoding table from code lengths (RFC 1951 3.2.2); false for an over-subscribed code or one whose
// second-level tables do not fit `cap`.  An incomplete code is accepted (unused patterns decode to K_INVALID), as zlib does.
BGZ_HD bool build_table(Tables &T, int which, const uint8_t *lens, int n_sym, uint32_t *tab, int tb, int cap) {
    for (int l = 0; l <= MAX_LEN; ++l) T.count[l] = 0;
    for (int s = 0; s < n_sym; ++s) ++T.count[lens[s] & 15];
    T.count[0] = 0;
    int left = 1;
    for (int l = 1; l <= MAX_LEN; ++l) { left = (left << 1) - (int)T.count[l]; if (left < 0) return false; }
    uint32_t code = 0;
    for (int l = 1; l <= MAX_LEN; ++l) { code = (code + T.count[l - 1]) << 1; T.next_code[l] = code; T.nc[l] = code; }
    const int first = 1 << tb;
    for (int i = 0; i < first; ++i) { tab[i] = mk(1, K_INVALID, 0, 0); T.sub_bits[i] = 0; }
    for (int s = 0; s < n_sym; ++s) {
        const int l = lens[s] & 15;
        if (l <= tb) { if (l) ++T.nc[l]; continue; }
        const uint32_t pfx = bit_reverse(T.nc[l]++, l) & (uint32_t)(first - 1);
        if (l - tb > T.sub_bits[pfx]) T.sub_bits[pfx] = (uint8_t)(l - tb);
    }
    int used = first;
    for (int pfx = 0; pfx < first; ++pfx) {
        if (!T.sub_bits[pfx]) continue;
        const int n = 1 << T.sub_bits[pfx];
        if (used + n > cap) return false;
        tab[pfx] = mk((uint32_t)tb, K_SUB, T.sub_bits[pfx], (uint32_t)used);
        for (int i = 0; i < n; ++i) tab[used + i] = mk(1, K_INVALID, 0, 0);
        used += n;
    }
    for (int s = 0; s < n_sym; ++s) {
        const int l = lens[s] & 15;
        if (!l) continue;
        const uint32_t rev = bit_reverse(T.next_code[l]++, l);
        const uint32_t e = symbol_entry(which, s, (uint32_t)l);
        if (l <= tb) {
            for (uint32_t i = rev; i < (uint32_t)first; i += 1u << l) tab[i] = e;
        } else {
            const uint32_t p = tab[rev & (uint32_t)(first - 1)];
            const uint32_t start = p >> 16, bits = (p >> 8) & 31u;
            for (uint32_t i = rev >> tb; i < (1u << bits); i += 1u << (l - tb)) tab[start + i] = e;
        }
    }
    return true;
}

struct Bits {
    const uint8_t *in, *end;
    uint64_t buf;
    int cnt;                     // valid bits in buf
    int64_t phantom;             // zero bits supplied behind the end of the input
};
BGZ_HD void refill(Bits &b) {
    if (b.end - b.in >= 8) {
        uint64_t w;
        __builtin_memcpy(&w, b.in, 8);                       // little-endian on both sides
        b.buf |= w << b.cnt;
        b.in += (63 - b.cnt) >> 3;
        b.cnt |= 56;
    } else {
        while (b.cnt <= 56) {
            if (b.in < b.end) b.buf |= (uint64_t)*b.in++ << b.cnt; else b.phantom += 8;
            b.cnt += 8;
        }
    }
}
BGZ_HD uint32_t peek(const Bits &b, int n) { return (uint32_t)(b.buf & ((1ull << n) - 1ull)); }
BGZ_HD void drop(Bits &b, int n) { b.buf >>= n; b.cnt -= n; }
BGZ_HD uint32_t take(Bits &b, int n) { const uint32_t v = peek(b, n); drop(b, n); return v; }
BGZ_HD bool overrun(const Bits &b) { return b.phantom > (int64_t)b.cnt; }

// Inflates exactly out_len bytes from the raw DEFLATE stream in[0, in_len): true when the stream ended with its final block
// after exactly out_len bytes.  Stored, fixed and dynamic blocks, any number of them.
BGZ_HD bool inflate_block(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, Tables &T) {
    Bits b{in, in + in_len, 0, 0, 0};
    uint8_t *o = out, *const o_end = out + out_len;
    T.fixed_built = 0;
    for (;;) {
        refill(b);
        const uint32_t final = take(b, 1), type = take(b, 2);
        if (type == 0) {
            drop(b, b.cnt & 7);                                  // to the byte boundary
            refill(b);
            const uint32_t len = take(b, 16), nlen = take(b, 16);
            if ((len ^ 0xFFFFu) != nlen || overrun(b)) return false;
            uint32_t left = len;
            if ((size_t)(o_end - o) < left) return false;
            while (left && b.cnt >= 8) {                         // the whole bytes still in the bit buffer first
                if ((int64_t)b.cnt - b.phantom < 8) return false;
                *o++ = (uint8_t)take(b, 8); --left;
            }
            if (left) {
                if (b.cnt != 0 || (size_t)(b.end - b.in) < left) return false;
                for (uint32_t k = 0; k < left; ++k) o[k] = b.in[k];
                b.in += left; o += left;
                b.buf = 0;
            }
            if (final) break;
            continue;
        } else if (type == 1) {
            if (!T.fixed_built) {
                for (int i = 0; i < 144; ++i) T.lens[i] = 8;
                for (int i = 144; i < 256; ++i) T.lens[i] = 9;
                for (int i = 256; i < 280; ++i) T.lens[i] = 7;
                for (int i = 280; i < 288; ++i) T.lens[i] = 8;
                for (int i = 0; i < N_DIST; ++i) T.lens[N_LITLEN + i] = 5;
                (void)build_table(T, 0, T.lens, N_LITLEN, T.lit, LIT_TB, (int)(sizeof(T.lit) / 4));
                (void)build_table(T, 1, T.lens + N_LITLEN, N_DIST, T.dst, DST_TB, (int)(sizeof(T.dst) / 4));
                T.fixed_built = 1;
            }
        } else if (type == 2) {
            T.fixed_built = 0;
            const uint32_t hlit = take(b, 5) + 257, hdist = take(b, 5) + 1, hclen = take(b, 4) + 4;
            if (hlit > 286 || hdist > 30) return false;
            for (int i = 0; i < N_PRE; ++i) T.pl[i] = 0;
            for (uint32_t i = 0; i < hclen; ++i) {
                if (b.cnt < 3) refill(b);
                const uint32_t v = take(b, 3);
                // the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const uint32_t at = i < 3 ? 16u + i : i == 3 ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1);
                T.pl[at] = (uint8_t)v;
            }
            if (!build_table(T, 2, T.pl, N_PRE, T.pre, PRE_TB, 1 << PRE_TB)) return false;
            uint32_t i = 0;
            while (i < hlit + hdist) {
                refill(b);
                const uint32_t e = T.pre[peek(b, PRE_TB)];
                if ((e & K_MASK) != K_LITERAL) return false;
                drop(b, (int)(e & 31u));
                const uint32_t sym = e >> 16;
                if (sym < 16) { T.lens[i++] = (uint8_t)sym; continue; }
                uint32_t rep, val = 0;
                if (sym == 16) { if (i == 0) return false; val = T.lens[i - 1]; rep = 3 + take(b, 2); }
                else if (sym == 17) rep = 3 + take(b, 3);
                else rep = 11 + take(b, 7);
                if (i + rep > hlit + hdist) return false;
                for (uint32_t k = 0; k < rep; ++k) T.lens[i + k] = (uint8_t)val;
                i += rep;
            }
            if (overrun(b) || T.lens[256] == 0) return false;
            if (!build_table(T, 1, T.lens + hlit, (int)hdist, T.dst, DST_TB, (int)(sizeof(T.dst) / 4))) return false;
            if (!build_table(T, 0, T.lens, (int)hlit, T.lit, LIT_TB, (int)(sizeof(T.lit) / 4))) return false;
        } else {
            return false;
        }
        // ---- the symbols of a compressed block ----
        for (;;) {
            refill(b);                                           // >= 56 bits: length code + extra + distance code + extra <= 48
            uint32_t e = T.lit[peek(b, LIT_TB)];
            if ((e & K_MASK) == K_SUB) e = T.lit[(e >> 16) + ((uint32_t)(b.buf >> LIT_TB) & ((1u << ((e >> 8) & 31u)) - 1u))];
            drop(b, (int)(e & 31u));
            const uint32_t kind = e & K_MASK;
            if (kind == K_LITERAL) {
                if (o >= o_end) return false;
                *o++ = (uint8_t)(e >> 16);
                const uint32_t e2 = T.lit[peek(b, LIT_TB)];      // a second literal from the same refill
                if ((e2 & K_MASK) == K_LITERAL && o < o_end) { drop(b, (int)(e2 & 31u)); *o++ = (uint8_t)(e2 >> 16); }
                continue;
            }
            if (kind == K_EOB) break;
            if (kind != K_LENGTH) return false;
            const uint32_t len = (e >> 16) + take(b, (int)((e >> 8) & 31u));
            uint32_t d = T.dst[peek(b, DST_TB)];
            if ((d & K_MASK) == K_SUB) d = T.dst[(d >> 16) + ((uint32_t)(b.buf >> DST_TB) & ((1u << ((d >> 8) & 31u)) - 1u))];
            if ((d & K_MASK) != K_LENGTH) return false;
            drop(b, (int)(d & 31u));
            const uint32_t dist = (d >> 16) + take(b, (int)((d >> 8) & 31u));
            if (dist > (size_t)(o - out) || len > (size_t)(o_end - o)) return false;
            const uint8_t *s = o - dist;
            if (dist >= 8 && (size_t)(o_end - o) >= (size_t)len + 8) {
                uint8_t *const stop = o + len;                    // eight bytes at a time, up to seven of over-copy inside the range
                do { uint64_t w; __builtin_memcpy(&w, s, 8); __builtin_memcpy(o, &w, 8); s += 8; o += 8; } while (o < stop);
                o = stop;
            } else {
                for (uint32_t k = 0; k < len; ++k) o[k] = s[k];
                o += len;
            }
        }
        if (overrun(b)) return false;
        if (final) break;
    }
    return o == o_end && !overrun(b);
}

// ---- CRC-32 (gzip polynomial, bit-reflected 0xEDB88320) by 64 lanes ------------------------------------------------------------
// The register after a message is linear in (start value, message) over GF(2): lane l runs the byte-wise update over slice l
// (lane 0 from 0xFFFFFFFF, the others from 0), multiplies its register by x^(8 * bytes behind its slice) mod P, and the XOR of
// the 64 products is the register of the whole block (what zlib's crc32_combine does for two).
BGZ_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    return c;
}
BGZ_HD uint32_t multmodp(uint32_t a, uint32_t b) {          // a * b mod P, x^0 = bit 31
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
BGZ_HD uint32_t x8n_modp(uint32_t n) {                      // x^(8 n) mod P
    uint32_t r = 1u << 31, b = 1u << 23;
    for (; n; n >>= 1) { if (n & 1u) r = multmodp(r, b); b = multmodp(b, b); }
    return r;
}
// lane's share of the register of data[0, n); tab = the 256 entries of crc_table_entry
BGZ_HD uint32_t crc_lane(const uint8_t *data, uint32_t n, uint32_t lane, const uint32_t *tab) {
    const uint32_t per = (n + 63u) >> 6;
    const uint32_t lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u;
    uint32_t p = lo;
    for (; p + 8 <= hi; p += 8) {
        uint64_t w;
        __builtin_memcpy(&w, data + p, 8);
        for (int k = 0; k < 8; ++k) { c = tab[(c ^ (uint32_t)w) & 255u] ^ (c >> 8); w >>= 8; }
    }
    for (; p < hi; ++p) c = tab[(c ^ data[p]) & 255u] ^ (c >> 8);
    if (lo == hi && lane != 0) return 0u;
    return multmodp(c, x8n_modp(n - hi));
}

// ---- BAM records (SAMv1 4.2) -----------------------------------------------------------------------------------------------------
BGZ_HD uint32_t rd32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
BGZ_HD uint32_t rd16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

enum { STEP_OK = 0, STEP_STOP = 1, STEP_BAD = 2 };
// The record at d[o] of an image of n bytes, as index_records' step() of ampbam.cpp takes it: STEP_STOP when its fixed fields
// or its body reach behind the image (the next piece completes it), STEP_BAD for block_size < 32 or > 2^27 or a body longer
// than block_size.  *next = the offset behind it.
BGZ_HD int record_step(const uint8_t *d, uint64_t n, uint64_t o, uint64_t *next) {
    if (o + 36 > n) return STEP_STOP;
    const uint64_t bs = rd32(d + o);
    if (bs < 32 || bs > (1u << 27)) return STEP_BAD;
    if (o + 4 + bs > n) return STEP_STOP;
    const uint8_t *c = d + o + 4;
    const uint64_t n_cig = rd16(c + 12), l_seq = rd32(c + 16), l_name = c[8];
    if (32ull + l_name + 4ull * n_cig + (l_seq + 1) / 2 + l_seq > bs) return STEP_BAD;
    *next = o + 4 + bs;
    return STEP_OK;
}

// plausible_record() of ampbam.cpp: does a plausible record start at d[o]?
BGZ_HD bool record_plausible(const uint8_t *d, uint64_t n, uint64_t o, int32_t n_ref, uint64_t *next) {
    if (o + 36 > n) return false;
    const uint64_t bs = rd32(d + o);
    if (bs < 32 || bs > (1u << 27)) return false;
    const uint8_t *c = d + o + 4;
    const int32_t ref_id = (int32_t)rd32(c), pos = (int32_t)rd32(c + 4), next_ref = (int32_t)rd32(c + 20), next_pos = (int32_t)rd32(c + 24);
    const uint32_t l_name = c[8], n_cig = rd16(c + 12), l_seq = rd32(c + 16);
    if (ref_id < -1 || ref_id >= n_ref || next_ref < -1 || next_ref >= n_ref || pos < -1 || next_pos < -1 || l_name < 1) return false;
    if (32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq > bs) return false;
    if (o + 4 + 32 + l_name + 4ull * n_cig > n) { *next = o + 4 + bs; return true; }      // the fixed part is all that can be seen
    if (c[32 + l_name - 1] != 0) return false;
    for (uint32_t k = 0; k + 1 < l_name; ++k) if (c[32 + k] < 33 || c[32 + k] > 126) return false;
    for (uint32_t k = 0; k < n_cig; ++k) if ((rd32(c + 32 + l_name + 4 * k) & 15u) > 8u) return false;
    *next = o + 4 + bs;
    return true;
}

}  // namespace ampbgzf
