// amp_sam.hip -- the opt-in device codec for SAM text.
//
// The reference reads and writes SAM through pysam (AmpliPy.py:296-360): text parsing in front of the per-read loop
// (A:896-915) and out_aln.write(s) behind it (A:911).  The host mirror does the same per line in Python
// (bamio.AlignmentReader._iter_sam, AlignmentWriter.write).  Here a chunk of text (whole lines) goes to the device once,
// a packed amp_dev_reads batch is built from it in HBM, amp_process_batch_device runs on that batch, and for a trimmed
// text output the kept lines are assembled on the device: the input line with POS and CIGAR replaced.
//
// Stages of a chunk (lane = what one thread works on):
//   scan     lane = 16 bytes of text (one 16-byte load): bit masks of '\n', '\t' and of bytes below '!', their counts, the
//            first byte no canonical SAM line holds (>= 0x80, NUL, a '\r' not in front of '\n')
//   rank     exclusive sums of the counts (hipcub): a byte's rank among the newlines / tabs / low bytes is the sum in front
//            of its slot plus a popcount of its slot's mask -- no lane walks a line to find its fields
//   lines    lane = slot: positions of the newlines, the tab rank at every line start
//   tabs     lane = slot: a tab's field number = its rank - the rank at its line's start; the first 11 are kept per line
//   records  lane = line: 11 fields?  integers, RNAME / RNEXT, CIGAR syntax, SEQ / QUAL lengths, the oddness verdict, the
//            row predicate of A:902; then exclusive sums over the lines give record, row, CIGAR-word and 8-base-slot offsets
//   rows     lane = line: the row's scalars, its CIGAR as BAM words, src_index
//   pack     lane = one 8-base slot of the whole batch: 8 SEQ letters -> 4 bytes of nibbles, 8 QUAL characters -> 8 bytes
//   format   lane = row: length of its output line; a sum; then one wave per row copies the three unchanged pieces of the
//            line with 8-byte loads and stores (unaligned on both sides) while its first lane renders POS and the CIGAR
// Only the short fields (integers, names, the CIGAR string) are walked byte by byte by one lane.
//
// The same lane functions compile for the host (-DAMPSAM_HOSTSIM, no HIP headers needed: any C++ compiler, sanitizers
// included) and a driver runs the stages lane after lane: the twin the CPU tests check against the Python codec.
// What surrounds the stages -- stream, copies, scan, events, the batch's way into the read pass and back -- is the shell of
// amp_codec.hpp.
#include "amp_codec.hpp"

namespace ampsam {

enum { CTL_NLINES = 0, CTL_NREC, CTL_NROWS, CTL_NCIG, CTL_NBASES, CTL_NSLOTS, CTL_ODD, CTL_BADBYTE, CTL_FMT_BYTES, CTL_FMT_ROWS,
       CTL_WORDS = 16 };
enum { FTABS = 11, WAVE = 64 };
static const uint32_t QUAL_STAR = 0xFFFFFFFFu;

// Every pointer of a chunk: device memory in the library, host memory in the twin.  Buf is a kernel argument and its layout
// the kernels' view of it: text and lines, the batch (amp_dev_reads: the shell's struct), the rows, the results of the read
// pass (the shell's struct), format -- in this order.
struct BufLines {
    const uint8_t *text; int64_t n_bytes, n_slots16, line_cap;
    uint32_t *mask;            // [n_slots16] newline bits | tab bits << 16
    uint32_t *lowmask;         // [n_slots16] bytes below '!' other than tab, newline and carriage return
    uint64_t *rank;            // [n_slots16] newlines | tabs << 32 in front of the slot (the counts before the sum)
    uint32_t *lowrank;         // [n_slots16] low bytes in front of the slot
    uint32_t *nl_pos;          // [line_cap]
    uint32_t *line_tab0;       // [line_cap + 1] tabs in front of the line
    uint32_t *ftab;            // [line_cap][FTABS]
    uint32_t *l_rec, *l_row, *l_ncig, *l_slots;      // per line: is a record, is a row, its CIGAR ops, its 8-base slots
    uint32_t *s_rec, *s_row, *s_ncig, *s_slots;      // their exclusive sums
};
struct BufRows {
    uint32_t *row_line, *row_seq, *row_qual;       // what pack and format need per row
    // @SQ names
    const uint8_t *names; const uint32_t *ref_off; int32_t n_ref;
    unsigned long long *ctl;   // [CTL_WORDS]
};
struct Buf : BufLines, ampcodec::Batch, BufRows, ampcodec::Trim {
    uint32_t *out_off, *cig_tlen; uint8_t *out;
    int32_t min_length, include_no_primer; int64_t good_rows;
};

AMP_HD uint64_t load8(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
AMP_HD void store8(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }
AMP_HD void odd(const Buf &b, int64_t line, int reason) { AMP_MIN64(&b.ctl[CTL_ODD], ((unsigned long long)line << 8) | (unsigned)reason); }

// ---- scan: lane = 16 bytes ---------------------------------------------------------------------------------------------
AMP_HD void lane_scan(const Buf &b, int64_t j) {
    const int64_t base = j * 16;
    uint32_t w[4];
    __builtin_memcpy(w, __builtin_assume_aligned(b.text + base, 16), 16);       // (the text buffer is 16-byte aligned and padded)
    const int64_t left = b.n_bytes - base;
    const uint32_t valid = left >= 16 ? 0xFFFFu : ((1u << left) - 1u);
    const uint32_t next = left > 16 ? b.text[base + 16] : 10u;
    uint32_t nl = 0, tab = 0, low = 0, bad = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        const uint32_t c1 = k < 15 ? (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u : next;
        nl |= (c == 10u ? 1u : 0u) << k;
        tab |= (c == 9u ? 1u : 0u) << k;
        low |= ((c < 33u && c != 9u && c != 10u && c != 13u) ? 1u : 0u) << k;
        bad |= ((c >= 128u || c == 0u || (c == 13u && c1 != 10u)) ? 1u : 0u) << k;
    }
    nl &= valid; tab &= valid; low &= valid; bad &= valid;
    b.mask[j] = nl | (tab << 16);
    b.lowmask[j] = low;
    b.rank[j] = (uint64_t)__builtin_popcount(nl) | ((uint64_t)__builtin_popcount(tab) << 32);
    b.lowrank[j] = (uint32_t)__builtin_popcount(low);
    if (bad) AMP_MIN64(&b.ctl[CTL_BADBYTE], base + __builtin_ctz(bad));
}

// ---- lines / tabs: lane = 16-byte slot, masks only ----------------------------------------------------------------------
AMP_HD void lane_lines(const Buf &b, int64_t j) {
    const uint32_t m = b.mask[j], tabm = m >> 16;
    uint32_t nl = m & 0xFFFFu;
    const uint64_t r = b.rank[j];
    uint32_t line = (uint32_t)r;
    const uint32_t tabr = (uint32_t)(r >> 32);
    if (j == 0) b.line_tab0[0] = 0;
    while (nl) {
        const int k = __builtin_ctz(nl);
        nl &= nl - 1;
        if ((int64_t)line < b.line_cap) {
            b.nl_pos[line] = (uint32_t)(j * 16 + k);
            b.line_tab0[line + 1] = tabr + (uint32_t)__builtin_popcount(tabm & ((1u << k) - 1u));
        }
        ++line;
    }
    if (j == b.n_slots16 - 1) b.ctl[CTL_NLINES] = line;
}

AMP_HD void lane_tabs(const Buf &b, int64_t j) {
    const uint32_t m = b.mask[j], nlm = m & 0xFFFFu;
    uint32_t tab = m >> 16;
    const uint64_t r = b.rank[j];
    uint32_t tabr = (uint32_t)(r >> 32);
    while (tab) {
        const int k = __builtin_ctz(tab);
        tab &= tab - 1;
        const uint32_t line = (uint32_t)r + (uint32_t)__builtin_popcount(nlm & ((1u << k) - 1u));
        if ((int64_t)line < b.line_cap) {
            const uint32_t f = tabr - b.line_tab0[line];
            if (f < FTABS) b.ftab[(size_t)line * FTABS + f] = (uint32_t)(j * 16 + k);
        }
        ++tabr;
    }
}

// ---- records: lane = line -------------------------------------------------------------------------------------------------
struct Line { uint32_t start, end, ntab; };

AMP_HD Line line_of(const Buf &b, int64_t i) {
    Line ln;
    ln.start = i ? b.nl_pos[i - 1] + 1u : 0u;
    ln.end = b.nl_pos[i];
    if (ln.end > ln.start && b.text[ln.end - 1] == 13) --ln.end;          // a '\r' before the '\n' is dropped
    ln.ntab = b.line_tab0[i + 1] - b.line_tab0[i];
    return ln;
}

// field k (0..10) of a line with at least 10 tabs
AMP_HD void field(const Buf &b, int64_t i, const Line &ln, int k, uint32_t &fs, uint32_t &fe) {
    fs = k == 0 ? ln.start : b.ftab[(size_t)i * FTABS + k - 1] + 1u;
    fe = (k < 10 || ln.ntab >= FTABS) ? b.ftab[(size_t)i * FTABS + k] : ln.end;
}

// -?(0|[1-9][0-9]*) and not "-0" (int() reads it, str() does not give it back): 0 ok, 1 otherwise
AMP_HD int parse_int(const uint8_t *t, uint32_t fs, uint32_t fe, int64_t &v) {
    if (fe == fs) return 1;
    const bool neg = t[fs] == '-';
    uint32_t p = fs + (neg ? 1u : 0u);
    if (p == fe) return 1;
    if (t[p] == '0' && (fe - p > 1 || neg)) return 1;
    int64_t a = 0;
    for (; p < fe; ++p) {
        const uint32_t c = (uint32_t)t[p] - '0';
        if (c > 9u) return 1;
        if (a < (1ll << 40)) a = a * 10 + (int64_t)c;
    }
    v = neg ? -a : a;
    return 0;
}

// -2: '*', -1: not an @SQ name, else its number
AMP_HD int name_id(const Buf &b, uint32_t fs, uint32_t fe) {
    const uint32_t n = fe - fs;
    if (n == 1 && b.text[fs] == '*') return -2;
    for (int r = 0; r < b.n_ref; ++r) {
        const uint32_t o = b.ref_off[r];
        if (b.ref_off[r + 1] - o != n) continue;
        uint32_t k = 0;
        while (k < n && b.names[o + k] == b.text[fs + k]) ++k;
        if (k == n) return r;
    }
    return -1;
}

AMP_HD int cigar_op(uint32_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; case 'B': return 9;
        default: return -1;
    }
}

// The CIGAR string: number of ops (0: '*'), -1 where parse_cigar would refuse it, -2 for an op length of 2^28 or more or one
// written with leading zeros.  out != NULL: the BAM words.
AMP_HD int cigar_scan(const uint8_t *t, uint32_t fs, uint32_t fe, uint32_t *out) {
    if (fe - fs == 1 && t[fs] == '*') return 0;
    if (fe == fs) return -1;
    int n = 0;
    uint32_t p = fs;
    while (p < fe) {
        uint64_t len = 0;
        const uint32_t p0 = p;
        while (p < fe && (uint32_t)t[p] - '0' <= 9u) {
            if (len < (1ull << 40)) len = len * 10 + ((uint32_t)t[p] - '0');
            ++p;
        }
        if (p == p0 || p == fe) return -1;
        const int op = cigar_op(t[p]);
        if (op < 0) return -1;
        if (len >= (1ull << 28) || (p - p0 > 1 && t[p0] == '0')) return -2;
        if (out) out[n] = ((uint32_t)len << 4) | (uint32_t)op;
        ++n; ++p;
    }
    return n;
}

AMP_HD uint32_t low_before(const Buf &b, uint32_t p) {
    return b.lowrank[p >> 4] + (uint32_t)__builtin_popcount(b.lowmask[p >> 4] & ((1u << (p & 15u)) - 1u));
}

AMP_HD void lane_records(const Buf &b, int64_t i) {
    uint32_t rec = 0, row = 0, ncig = 0, slots = 0;
    const int64_t n_lines = (int64_t)b.ctl[CTL_NLINES];
    if (i < n_lines) {
        const Line ln = line_of(b, i);
        int why = 0;
        const unsigned long long fb = b.ctl[CTL_BADBYTE];
        if (fb >= ln.start && fb <= b.nl_pos[i]) why = AMP_SAM_ODD_BYTE;
        if (ln.ntab >= 10) {
            rec = 1;
            const uint8_t *t = b.text;
            uint32_t fs, fe;
            int64_t flag = 0, v = 0;
            // the five integers: FLAG POS MAPQ PNEXT TLEN
            field(b, i, ln, 1, fs, fe);
            if (!why && parse_int(t, fs, fe, flag)) why = AMP_SAM_ODD_INT;
            if (!why && (flag < 0 || flag > 65535)) why = AMP_SAM_ODD_RANGE;
            field(b, i, ln, 3, fs, fe);
            if (!why && parse_int(t, fs, fe, v)) why = AMP_SAM_ODD_INT;
            if (!why && (v < 0 || v > 0x7FFFFFFFll)) why = AMP_SAM_ODD_RANGE;
            field(b, i, ln, 4, fs, fe);
            if (!why && parse_int(t, fs, fe, v)) why = AMP_SAM_ODD_INT;
            if (!why && (v < 0 || v > 255)) why = AMP_SAM_ODD_RANGE;
            field(b, i, ln, 7, fs, fe);
            if (!why && parse_int(t, fs, fe, v)) why = AMP_SAM_ODD_INT;
            if (!why && (v < 0 || v > 0x7FFFFFFFll)) why = AMP_SAM_ODD_RANGE;
            field(b, i, ln, 8, fs, fe);
            if (!why && parse_int(t, fs, fe, v)) why = AMP_SAM_ODD_INT;
            if (!why && (v < -0x80000000ll || v > 0x7FFFFFFFll)) why = AMP_SAM_ODD_RANGE;
            // RNAME, RNEXT in the spellings the writer gives back
            field(b, i, ln, 2, fs, fe);
            const int rn = name_id(b, fs, fe);
            if (!why && rn == -1) why = AMP_SAM_ODD_RNAME;
            field(b, i, ln, 6, fs, fe);
            if (!why) {
                if (fe - fs == 1 && t[fs] == '=') { if (rn < 0) why = AMP_SAM_ODD_RNEXT; }
                else {
                    const int rx = name_id(b, fs, fe);
                    if (rx == -1 || (rx >= 0 && rx == rn)) why = AMP_SAM_ODD_RNEXT;
                }
            }
            field(b, i, ln, 5, fs, fe);
            const int nc = cigar_scan(t, fs, fe, nullptr);
            if (!why && nc == -1) why = AMP_SAM_ODD_CIGAR;
            if (!why && nc == -2) why = AMP_SAM_ODD_CIGAR_LEN;
            field(b, i, ln, 9, fs, fe);
            const uint32_t slen = fe - fs;
            const bool sstar = slen == 1 && t[fs] == '*';
            field(b, i, ln, 10, fs, fe);
            const uint32_t qlen = fe - fs;
            const bool qstar = qlen == 1 && t[fs] == '*';
            if (!why && (slen == 0 || qlen == 0)) why = AMP_SAM_ODD_EMPTY;
            if (!why && !qstar && sstar) why = AMP_SAM_ODD_QUAL_NO_SEQ;
            if (!why && !qstar && qlen != slen) why = AMP_SAM_ODD_QUAL_LEN;
            if (!why && !qstar && low_before(b, fe) != low_before(b, fs)) why = AMP_SAM_ODD_QUAL_CHAR;
            if (!why && !(flag & 4) && nc > 0) {                     // A:902
                row = 1; ncig = (uint32_t)nc; slots = sstar ? 0u : (slen + 7u) >> 3;
            }
        }
        if (why) odd(b, i, why);
    }
    b.l_rec[i] = b.s_rec[i] = rec; b.l_row[i] = b.s_row[i] = row;
    b.l_ncig[i] = b.s_ncig[i] = ncig; b.l_slots[i] = b.s_slots[i] = slots;
}

// ---- rows: lane = line ----------------------------------------------------------------------------------------------------
AMP_HD void lane_rows(const Buf &b, int64_t i) {
    const int64_t n_lines = (int64_t)b.ctl[CTL_NLINES];
    const int64_t last = (n_lines < b.line_cap ? n_lines : b.line_cap) - 1;
    if (i > last) return;
    if (b.l_row[i]) {
        const uint32_t r = b.s_row[i];
        const Line ln = line_of(b, i);
        const uint8_t *t = b.text;
        uint32_t fs, fe;
        int64_t v = 0;
        field(b, i, ln, 1, fs, fe); (void)parse_int(t, fs, fe, v); b.flag[r] = (uint16_t)v;
        field(b, i, ln, 3, fs, fe); (void)parse_int(t, fs, fe, v); b.pos[r] = (int32_t)(v - 1);
        field(b, i, ln, 8, fs, fe); (void)parse_int(t, fs, fe, v); b.tlen[r] = (int32_t)v;
        field(b, i, ln, 5, fs, fe); (void)cigar_scan(t, fs, fe, b.cig + b.s_ncig[i]);
        field(b, i, ln, 9, fs, fe);
        const bool sstar = fe - fs == 1 && t[fs] == '*';
        const uint32_t L = sstar ? 0u : fe - fs;
        b.lseq[r] = L; b.row_seq[r] = fs;
        field(b, i, ln, 10, fs, fe);
        b.row_qual[r] = (fe - fs == 1 && t[fs] == '*') ? QUAL_STAR : fs;
        b.cig_off32[r] = b.s_ncig[i]; b.seq_off8[r] = b.s_slots[i];
        b.src_index[r] = (int64_t)b.s_rec[i]; b.row_line[r] = (uint32_t)i;
        AMP_ADD64(&b.ctl[CTL_NBASES], L);
    }
    if (i == last) {
        const uint32_t n = b.s_row[i] + b.l_row[i];
        b.cig_off32[n] = b.s_ncig[i] + b.l_ncig[i]; b.seq_off8[n] = b.s_slots[i] + b.l_slots[i];
        b.ctl[CTL_NREC] = b.s_rec[i] + b.l_rec[i]; b.ctl[CTL_NROWS] = n;
        b.ctl[CTL_NCIG] = b.cig_off32[n]; b.ctl[CTL_NSLOTS] = b.seq_off8[n];
    }
}

// ---- pack: lane = 8-base slot of the batch ----------------------------------------------------------------------------------
// "=ACMGRSVTWYHKDBN" in both cases, any other byte 15: the letters a..p and q..z as nibbles of two constants
AMP_HD uint32_t nt16(uint32_t c) {
    if (c == '=') return 0;
    const uint32_t k = (c | 0x20u) - 'a';
    if (k < 16u) return (uint32_t)(0xFFF3FCFFB4FFD2E1ull >> (4 * k)) & 15u;
    if (k < 26u) return (uint32_t)(0xFAF97F865Full >> (4 * (k - 16u))) & 15u;
    return 15u;
}

AMP_HD void lane_pack(const Buf &b, int64_t s) {
    const uint32_t n = (uint32_t)b.ctl[CTL_NROWS];
    uint32_t lo = 0, hi = n;                                  // the last row r with seq_off8[r] <= s (rows without bases own no slot)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (b.seq_off8[mid] <= (uint32_t)s) lo = mid; else hi = mid; }
    const uint32_t r = lo, k = (uint32_t)s - b.seq_off8[r], L = b.lseq[r];
    const uint32_t nb = L - 8u * k >= 8u ? 8u : L - 8u * k;
    const uint64_t keep = nb == 8u ? ~0ull : ((1ull << (8 * nb)) - 1ull);
    const uint64_t sq = load8(b.text + b.row_seq[r] + 8u * k) & keep;
    uint32_t packed = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t code = (uint32_t)q < nb ? nt16((uint32_t)(sq >> (8 * q)) & 255u) : 0u;
        packed |= code << (8 * (q >> 1) + ((q & 1) ? 0 : 4));      // byte q / 2, high nibble first
    }
    __builtin_memcpy(b.seq + 4 * (size_t)s, &packed, 4);
    uint64_t ql;
    if (b.row_qual[r] == QUAL_STAR) ql = keep;                  // 0xFF in all l_seq bytes
    else ql = ((load8(b.text + b.row_qual[r] + 8u * k) | ~keep) - 0x2121212121212121ull) & keep;     // every byte >= '!': no borrow
    store8(b.qual + 8 * (size_t)s, ql);
}

// ---- format -----------------------------------------------------------------------------------------------------------------
AMP_HD uint32_t ndigits(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
AMP_HD uint32_t put_uint(uint8_t *p, uint64_t v) {
    const uint32_t n = ndigits(v);
    for (uint32_t k = n; k-- > 0;) { p[k] = (uint8_t)('0' + v % 10); v /= 10; }
    return n;
}
AMP_HD bool row_kept(const Buf &b, int64_t r) {                 // A:910, and nothing from the first failing read on (A:907-911)
    return r < b.good_rows && b.ref_len[r] >= b.min_length && ((b.trim_flags[r] & 3u) || b.include_no_primer);
}
AMP_HD const uint32_t *row_new_cig(const Buf &b, int64_t r) { return b.new_cig + b.cig_off32[r] + 3 * (size_t)r; }

AMP_HD void lane_fmt_len(const Buf &b, int64_t r) {
    uint32_t len = 0, ct = 0;
    if (row_kept(b, r)) {
        const int64_t i = b.row_line[r];
        const Line ln = line_of(b, i);
        uint32_t f3s, f3e, f5s, f5e;
        field(b, i, ln, 3, f3s, f3e);
        field(b, i, ln, 5, f5s, f5e);
        const uint32_t *w = row_new_cig(b, r);
        for (uint32_t k = 0; k < b.new_ncig[r]; ++k) ct += ndigits(w[k] >> 4) + 1u;
        const int64_t p1 = (int64_t)b.new_pos[r] + 1;
        len = (ln.end - ln.start) - (f3e - f3s) - (f5e - f5s) + ct + (p1 < 0 ? 1u + ndigits((uint64_t)-p1) : ndigits((uint64_t)p1)) + 1u;
        AMP_ADD64(&b.ctl[CTL_FMT_ROWS], 1);
        AMP_ADD64(&b.ctl[CTL_FMT_BYTES], len);
    }
    b.out_off[r] = len; b.cig_tlen[r] = ct;
}

// n bytes by the 64 lanes of a wave, 8 per lane and step; the last n % 8 one per lane
AMP_HD void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    for (uint32_t o = lane * 8u; o + 8u <= n; o += WAVE * 8u) store8(dst + o, load8(src + o));
    const uint32_t tail = n & ~7u;
    if (tail + lane < n) dst[tail + lane] = src[tail + lane];
}

AMP_HD void lane_fmt_copy(const Buf &b, int64_t r, uint32_t lane) {
    if (!row_kept(b, r)) return;
    const int64_t i = b.row_line[r];
    const Line ln = line_of(b, i);
    uint32_t f3s, f3e, f5s, f5e;
    field(b, i, ln, 3, f3s, f3e);
    field(b, i, ln, 5, f5s, f5e);
    const int64_t p1 = (int64_t)b.new_pos[r] + 1;
    const uint32_t pd = p1 < 0 ? 1u + ndigits((uint64_t)-p1) : ndigits((uint64_t)p1);
    uint8_t *d = b.out + b.out_off[r];
    wave_copy(d, b.text + ln.start, f3s - ln.start, lane);
    d += f3s - ln.start;
    if (lane == 0) { uint8_t *p = d; if (p1 < 0) *p++ = '-'; (void)put_uint(p, (uint64_t)(p1 < 0 ? -p1 : p1)); }
    d += pd;
    wave_copy(d, b.text + f3e, f5s - f3e, lane);
    d += f5s - f3e;
    if (lane == 0) {
        const uint32_t *w = row_new_cig(b, r);
        uint8_t *p = d;
        for (uint32_t k = 0; k < b.new_ncig[r]; ++k) {
            p += put_uint(p, w[k] >> 4);
            const uint32_t op = w[k] & 15u;
            *p++ = op < 10u ? (uint8_t)"MIDNSHP=XB"[op] : (uint8_t)'?';
        }
    }
    d += b.cig_tlen[r];
    wave_copy(d, b.text + f5e, ln.end - f5e, lane);
    d += ln.end - f5e;
    if (lane == 0) *d = '\n';
}

// ---- layout of a chunk's memory ---------------------------------------------------------------------------------------------
static inline int64_t line_cap_for(int64_t n_bytes) { return n_bytes / 64 + 1024; }       // a record is far longer than 64 bytes; a chunk
                                                                                         // with more lines than this is odd (AMP_SAM_ODD_LINES)
// Carves `base` (NULL: sizes only) for chunks of up to cap_bytes of text; returns the bytes needed.
static size_t carve(Buf &b, uint8_t *base, int64_t cap_bytes) {
    const size_t n = (size_t)cap_bytes, S = n / 16 + 2, LC = (size_t)line_cap_for(cap_bytes);
    ampcodec::Carver take{base};
    b.text = take(n + 64);
    b.mask = (uint32_t *)take(S * 4); b.lowmask = (uint32_t *)take(S * 4); b.rank = (uint64_t *)take(S * 8); b.lowrank = (uint32_t *)take(S * 4);
    b.nl_pos = (uint32_t *)take(LC * 4); b.line_tab0 = (uint32_t *)take((LC + 1) * 4); b.ftab = (uint32_t *)take(LC * FTABS * 4);
    uint32_t **per_line[] = {&b.l_rec, &b.l_row, &b.l_ncig, &b.l_slots, &b.s_rec, &b.s_row, &b.s_ncig, &b.s_slots};
    for (uint32_t **p : per_line) *p = (uint32_t *)take(LC * 4);
    b.pos = (int32_t *)take((LC + 1) * 4); b.flag = (uint16_t *)take((LC + 1) * 2); b.tlen = (int32_t *)take((LC + 1) * 4);
    b.lseq = (uint32_t *)take((LC + 1) * 4); b.cig_off32 = (uint32_t *)take((LC + 1) * 4); b.seq_off8 = (uint32_t *)take((LC + 1) * 4);
    b.row_line = (uint32_t *)take((LC + 1) * 4); b.row_seq = (uint32_t *)take((LC + 1) * 4); b.row_qual = (uint32_t *)take((LC + 1) * 4);
    b.src_index = (int64_t *)take((LC + 1) * 8);
    // a row of L bases has L + 21 bytes of text or more and an op two: the padded bases fit n bytes, the ops n / 2 words
    b.cig = (uint32_t *)take((n / 2 + 4) * 4); b.seq = take(n / 2 + 64); b.qual = take(n + 64);
    b.out_off = (uint32_t *)take((LC + 1) * 4); b.cig_tlen = (uint32_t *)take((LC + 1) * 4);
    b.ctl = (unsigned long long *)take(CTL_WORDS * 8);
    return take.o;
}

}  // namespace ampsam

using namespace ampsam;
using namespace ampcodec;

#ifndef AMPSAM_HOSTSIM
CODEC_KERNEL(k_sam_scan, lane_scan)
CODEC_KERNEL(k_sam_lines, lane_lines)
CODEC_KERNEL(k_sam_tabs, lane_tabs)
CODEC_KERNEL(k_sam_records, lane_records)
CODEC_KERNEL(k_sam_rows, lane_rows)
CODEC_KERNEL(k_sam_pack, lane_pack)
CODEC_KERNEL(k_sam_fmt_len, lane_fmt_len)
__global__ void __launch_bounds__(256) k_sam_fmt_copy(Buf b, int64_t n_rows) {      // one wave per row
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += (int64_t)gridDim.x * 4) lane_fmt_copy(b, r, lane);
}
#endif
CODEC_FIRST_BAD_KERNEL(k_sam_first_bad)

struct amp_sam {
    Shell sh;
    Buf b{};
    int64_t cap_bytes = 0;
    uint8_t *arena = nullptr;
    uint8_t *names = nullptr; uint32_t *ref_off = nullptr; int32_t n_ref = -1;      // -1: amp_sam_set_references not called yet
    uint8_t *out = nullptr; size_t out_cap = 0;       // output text
    amp_sam_info info{};
    bool parsed = false, processed = false;
    int64_t good_rows = 0;
    unsigned long long h_ctl[CTL_WORDS];
};

static int sam_ensure(amp_sam *s, int64_t n_bytes) {
    if (n_bytes <= s->cap_bytes) return AMP_OK;
    CODEC_OK(codec_sync(s->sh));
    const int64_t cap = n_bytes + n_bytes / 8 + 4096;           // chunks of a run have one size: grown once, then reused
    Buf nb = s->b;
    const size_t bytes = carve(nb, nullptr, cap);
    uint8_t *p = nullptr;
    CODEC_OK(codec_alloc(&p, bytes));
    codec_free(s->arena);
    s->arena = p; s->cap_bytes = cap;
    (void)carve(s->b, p, cap);
    return AMP_OK;
}

extern "C" {

// bamio.AlignmentReader / AlignmentWriter of one run; A:296-360
int amp_sam_create(amp_ctx *ctx, amp_sam **out) { return codec_new(ctx, out, AMP_SAM_N_STAGES, k_sam_first_bad); }

void amp_sam_destroy(amp_sam *s) {
    if (!s) return;
    DevGuard guard(s->sh);
    (void)codec_wait(s->sh);
    codec_free(s->arena); codec_free(s->names); codec_free(s->ref_off); codec_free(s->out);
    codec_delete(s);
}

// the @SQ SN names in header order: header.refs of bamio.AlignmentReader (what RNAME / RNEXT are looked up in)
int amp_sam_set_references(amp_sam *s, int32_t n_ref, const char *const *names) {
    if (!s || n_ref < 0 || n_ref > AMP_SAM_MAX_REFS || (n_ref && !names)) return AMP_EINVAL;
    DevGuard guard(s->sh);
    uint32_t off[AMP_SAM_MAX_REFS + 1];
    size_t tot = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (!names[r]) return AMP_EINVAL;
        off[r] = (uint32_t)tot;
        tot += strlen(names[r]);
        if (tot > AMP_SAM_MAX_REF_BYTES) return AMP_EINVAL;
    }
    off[n_ref] = (uint32_t)tot;
    if (!s->names) {
        CODEC_OK(codec_alloc(&s->names, AMP_SAM_MAX_REF_BYTES + 16));
        CODEC_OK(codec_alloc((uint8_t **)&s->ref_off, sizeof(off)));
    }
    uint8_t blob[AMP_SAM_MAX_REF_BYTES + 16];
    for (int32_t r = 0; r < n_ref; ++r) memcpy(blob + off[r], names[r], off[r + 1] - off[r]);
    CODEC_OK(codec_up(s->sh, s->names, blob, tot));
    CODEC_OK(codec_up(s->sh, s->ref_off, off, sizeof(uint32_t) * (size_t)(n_ref + 1)));
    CODEC_OK(codec_wait(s->sh));
    s->n_ref = n_ref;
    return AMP_OK;
}

// pysam's text parsing in front of A:896 and the skip of A:902 for a chunk of lines: bamio._iter_sam + ReadBatch.from_segments
int amp_sam_parse(amp_sam *s, const uint8_t *text, int64_t n_bytes, amp_sam_info *info) {
    if (!s || !info || n_bytes < 0 || n_bytes >= (1ll << 30) || (n_bytes && !text)) return AMP_EINVAL;
    if (n_bytes && text[n_bytes - 1] != '\n') return AMP_EINVAL;
    if (s->n_ref < 0) return AMP_ESTATE;
    DevGuard guard(s->sh);
    s->parsed = s->processed = false;
    amp_sam_info z{};
    z.first_odd_line = -1;
    s->info = *info = z;
    CODEC_OK(sam_ensure(s, n_bytes > 0 ? n_bytes : 1));
    Buf &b = s->b;
    b.n_bytes = n_bytes; b.n_slots16 = (n_bytes + 15) / 16; b.line_cap = line_cap_for(n_bytes);
    b.names = s->names; b.ref_off = s->ref_off; b.n_ref = s->n_ref;
    codec_mark(s->sh, 0);
    CODEC_OK(codec_up(s->sh, (void *)b.text, text, (size_t)n_bytes));
    CODEC_OK(codec_zero(s->sh, (uint8_t *)b.text + n_bytes, 0, 48));
    CODEC_OK(codec_zero(s->sh, b.ctl, 0, CTL_WORDS * 8));
    CODEC_OK(codec_zero(s->sh, &b.ctl[CTL_ODD], 0xFF, 16));             // CTL_ODD, CTL_BADBYTE: minima
    CODEC_OK(codec_zero(s->sh, b.cig_off32, 0, 4));
    CODEC_OK(codec_zero(s->sh, b.seq_off8, 0, 4));
    codec_mark(s->sh, 1);
    if (n_bytes) {
        const int64_t S = b.n_slots16, LC = b.line_cap;
        CODEC_RUN(s, k_sam_scan, lane_scan, S, -1);
        CODEC_OK(codec_scan(s->sh, b.rank, S));
        CODEC_OK(codec_scan(s->sh, b.lowrank, S));
        codec_mark(s->sh, 2);
        CODEC_RUN(s, k_sam_lines, lane_lines, S, -1);
        CODEC_RUN(s, k_sam_tabs, lane_tabs, S, -1);
        codec_mark(s->sh, 3);
        CODEC_RUN(s, k_sam_records, lane_records, LC, -1);
        CODEC_OK(codec_scan(s->sh, b.s_rec, LC));
        CODEC_OK(codec_scan(s->sh, b.s_row, LC));
        CODEC_OK(codec_scan(s->sh, b.s_ncig, LC));
        CODEC_OK(codec_scan(s->sh, b.s_slots, LC));
        CODEC_RUN(s, k_sam_rows, lane_rows, LC, CTL_NLINES);
        codec_mark(s->sh, 4);
        CODEC_RUN(s, k_sam_pack, lane_pack, n_bytes / 8 + 1, CTL_NSLOTS);
        codec_mark(s->sh, 5);
    }
    CODEC_OK(codec_down(s->sh, s->h_ctl, b.ctl, CTL_WORDS * 8));
    CODEC_OK(codec_wait(s->sh));
    const unsigned long long *c = s->h_ctl;
    amp_sam_info &I = s->info;
    I.n_lines = (int64_t)c[CTL_NLINES]; I.n_records = (int64_t)c[CTL_NREC]; I.n_rows = (int64_t)c[CTL_NROWS];
    I.n_cig = (int64_t)c[CTL_NCIG]; I.n_bases = (int64_t)c[CTL_NBASES]; I.n_bases_padded = (int64_t)c[CTL_NSLOTS] * 8;
    if (c[CTL_ODD] != ~0ull) { I.first_odd_line = (int64_t)(c[CTL_ODD] >> 8); I.odd_reason = (int32_t)(c[CTL_ODD] & 255u); }
    if (I.n_lines > b.line_cap && (I.first_odd_line < 0 || I.first_odd_line >= b.line_cap)) { I.first_odd_line = b.line_cap; I.odd_reason = AMP_SAM_ODD_LINES; }
    *info = I;
    s->parsed = true;
    return AMP_OK;
}

// the batch of the last parse as the read pass takes it
int amp_sam_reads(amp_sam *s, amp_dev_reads *out) {
    if (!s || !out) return AMP_EINVAL;
    if (!s->parsed) return AMP_ESTATE;
    *out = codec_reads(s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded);
    return AMP_OK;
}

// ReadBatch.from_segments of the chunk's records, for tests and tools: dst's arrays are written (n_reads rows expected)
int amp_sam_batch_to_host(amp_sam *s, const amp_reads *dst, int64_t *src_index) {
    if (!s || !dst) return AMP_EINVAL;
    if (!s->parsed) return AMP_ESTATE;
    return codec_batch_to_host(s->sh, s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, dst, src_index, 0);
}

// format writes nothing from the first failing row on
static int sam_processed(amp_sam *s, int rc, int64_t bad, int64_t *first_bad_row) {
    if (rc) return rc;
    s->good_rows = bad >= 0 ? bad : s->info.n_rows;
    s->processed = true;
    if (first_bad_row) *first_bad_row = bad;
    return AMP_OK;
}

#ifndef AMPSAM_HOSTSIM
// A:896-915 for the rows of the chunk: amp_process_batch_device on the batch of the last parse, results kept in s
int amp_sam_process(amp_sam *s, uint64_t read_base, int64_t *first_bad_row, uint8_t *its_status) {
    if (!s) return AMP_EINVAL;
    if (!s->parsed || s->info.first_odd_line >= 0) return AMP_ESTATE;
    int64_t bad = -1;
    const int rc = codec_process(s->sh, s->b, s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, read_base, 6, &bad, its_status);
    return sam_processed(s, rc, bad, first_bad_row);
}

// milliseconds of the stages of the last parse / process / format on the ctx stream (HIP events); on != 0 switches the events on
int amp_sam_stage_ms(amp_sam *s, int on, float *ms) { return s ? codec_stage_ms(s->sh, on, ms) : AMP_EINVAL; }
#else
// the twin has no read pass: the test hands it the results the format stage is to work from
int amp_sam_twin_set_results(amp_sam *s, const int32_t *new_pos, const uint32_t *new_ncig, const uint32_t *new_cig, const int32_t *ref_len,
                             const uint8_t *trim_flags, const uint8_t *status, int64_t *first_bad_row, uint8_t *its_status) {
    if (!s || !new_pos || !new_ncig || !new_cig || !ref_len || !trim_flags || !status) return AMP_EINVAL;
    if (!s->parsed || s->info.first_odd_line >= 0) return AMP_ESTATE;
    CODEC_OK(codec_results_room(s->sh, s->info.n_rows, s->info.n_cig, s->b));
    const Buf &b = s->b;
    const size_t n = (size_t)s->info.n_rows;
    memcpy((void *)b.new_pos, new_pos, n * 4); memcpy((void *)b.new_ncig, new_ncig, n * 4); memcpy((void *)b.ref_len, ref_len, n * 4);
    memcpy((void *)b.new_cig, new_cig, ((size_t)s->info.n_cig + 3 * n) * 4);
    memcpy((void *)b.trim_flags, trim_flags, n); memcpy((void *)b.status, status, n);
    int64_t bad = -1;
    const int rc = codec_first_bad(s->sh, s->b, s->info.n_rows, &bad, its_status);
    return sam_processed(s, rc, bad, first_bad_row);
}
#endif

// out_aln.write(s) of A:911 under the filter of A:910 for the rows in front of the first failing one: AlignmentWriter.write(r, pos=, cigar=)
int amp_sam_format(amp_sam *s, int32_t min_length, int32_t include_no_primer, uint8_t *out, int64_t cap, int64_t *n_bytes, int64_t *n_rows_written) {
    if (!s || !n_bytes || cap < 0 || (cap && !out)) return AMP_EINVAL;
    if (!s->parsed || !s->processed) return AMP_EINVAL;
    DevGuard guard(s->sh);
    Buf &b = s->b;
    const int64_t n = s->info.n_rows;
    b.min_length = min_length; b.include_no_primer = include_no_primer ? 1 : 0; b.good_rows = s->good_rows;
    codec_mark(s->sh, 8);
    CODEC_OK(codec_zero(s->sh, &b.ctl[CTL_FMT_BYTES], 0, 16));
    CODEC_RUN(s, k_sam_fmt_len, lane_fmt_len, n, -1);
    CODEC_OK(codec_scan(s->sh, b.out_off, n));
    unsigned long long tot[2] = {0, 0};
    CODEC_OK(codec_down(s->sh, tot, &b.ctl[CTL_FMT_BYTES], 16));
    CODEC_OK(codec_wait(s->sh));
    *n_bytes = (int64_t)tot[0];
    if (n_rows_written) *n_rows_written = (int64_t)tot[1];
    if ((int64_t)tot[0] > cap) return AMP_EOVERFLOW;
    if (tot[0] >= (1ull << 32)) return AMP_EOVERFLOW;
    CODEC_OK(codec_grow(s->sh, &s->out, &s->out_cap, (size_t)tot[0] + 64));
    b.out = s->out;
#ifndef AMPSAM_HOSTSIM
    if (n > 0 && tot[0]) {
        k_sam_fmt_copy<<<codec_grid(n * 64), 256, 0, s->sh.stream>>>(b, n);
        if (hipGetLastError() != hipSuccess) return AMP_EHIP;
    }
#else
    for (int64_t r = 0; r < n; ++r) for (uint32_t lane = 0; lane < WAVE; ++lane) lane_fmt_copy(b, r, lane);
#endif
    codec_mark(s->sh, 9);
    CODEC_OK(codec_down(s->sh, out, s->out, (size_t)tot[0]));
    codec_mark(s->sh, 10);
    return codec_wait(s->sh);
}

}  // extern "C"
