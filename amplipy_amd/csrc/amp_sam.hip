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
#define BGZ_HD AMP_HD
#include "amp_bamtail.hpp"

namespace ampsam {

enum { CTL_NLINES = 0, CTL_NREC, CTL_NROWS, CTL_NCIG, CTL_NBASES, CTL_NSLOTS, CTL_ODD, CTL_BADBYTE, CTL_FMT_BYTES, CTL_FMT_ROWS,
       CTL_NTABS, CTL_BAM_BYTES, CTL_WORDS = 16 };
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
// BAM output (amp_sam_set_output): a table per tab of the chunk, a size per row, the encoder's Out
struct BufBam {
    int32_t bam_mode, pad; int64_t tab_cap;
    uint32_t *tab_pos;         // [tab_cap] where tab T of the chunk lies
    uint32_t *aux_sz;          // [tab_cap + 1] BAM bytes of the aux field behind tab T (0: no aux field), then their exclusive sum
    uint32_t *row_bsz;         // [line_cap + 1] per row: bytes of its BAM record, block_size word included, CIGAR left out
    const unsigned long long *bad_key;      // the key of the first failing row where the read pass left it (NULL: good_rows holds it)
    ampbamout::Out o;
};
struct Buf : BufLines, ampcodec::Batch, BufRows, ampcodec::Trim, BufBam {
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
    if (j == b.n_slots16 - 1) { b.ctl[CTL_NLINES] = line; b.ctl[CTL_NTABS] = tabr + (uint32_t)__builtin_popcount(tabm); }
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
        if (b.bam_mode && (int64_t)tabr < b.tab_cap) b.tab_pos[tabr] = (uint32_t)(j * 16 + k);
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
            if (b.bam_mode) {                                        // what a BAM record's fields cannot hold
                field(b, i, ln, 0, fs, fe);
                if (!why && fe - fs > 254u) why = AMP_SAM_ODD_QNAME;
                if (!why && nc > 65535 - (int)ampbamout::OUT_SPARE_OPS) why = AMP_SAM_ODD_CIGAR_OPS;
            }
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
        if (b.bam_mode) {
            field(b, i, ln, 0, fs, fe);
            const uint32_t aux = b.aux_sz[b.line_tab0[i + 1]] - b.aux_sz[b.line_tab0[i] + 10u];
            b.row_bsz[r] = 36u + (fe - fs) + 1u + ((L + 1u) >> 1) + L + aux;
            AMP_ADD64(&b.ctl[CTL_BAM_BYTES], b.row_bsz[r]);
        }
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

// ---- BAM output: aux fields, text to binary (aux_sam_to_bam of bamio.py) ------------------------------------------------------------
using ampbamout::o_wr16;
using ampbamout::o_wr32;

// -?(0|[1-9][0-9]*); values beyond 2^40 stay beyond it
AMP_HD bool aux_int(const uint8_t *t, uint32_t fs, uint32_t fe, int64_t &v) {
    if (fe == fs) return false;
    const bool neg = t[fs] == '-';
    uint32_t p = fs + (neg ? 1u : 0u);
    if (p == fe || (t[p] == '0' && fe - p > 1)) return false;
    int64_t a = 0;
    for (; p < fe; ++p) {
        const uint32_t c = (uint32_t)t[p] - '0';
        if (c > 9u) return false;
        if (a < (1ll << 40)) a = a * 10 + (int64_t)c;
    }
    v = neg ? -a : a;
    return true;
}
// the first of c C s S i I that holds x (the order of the Python loop): 0..5, -1: none
AMP_HD int int_code(int64_t x) {
    if (x >= -128 && x <= 127) return 0;
    if (x >= 0 && x <= 255) return 1;
    if (x >= -32768 && x <= 32767) return 2;
    if (x >= 0 && x <= 65535) return 3;
    if (x >= -2147483648ll && x <= 2147483647ll) return 4;
    if (x >= 0 && x <= 4294967295ll) return 5;
    return -1;
}
AMP_HD bool int_fits(int code, int64_t x) {
    switch (code) {
        case 0: return x >= -128 && x <= 127;
        case 1: return x >= 0 && x <= 255;
        case 2: return x >= -32768 && x <= 32767;
        case 3: return x >= 0 && x <= 65535;
        case 4: return x >= -2147483648ll && x <= 2147483647ll;
        default: return x >= 0 && x <= 4294967295ll;
    }
}
AMP_HD uint32_t int_bytes(int code) { return code < 2 ? 1u : code < 4 ? 2u : 4u; }
AMP_HD void put_int(uint8_t *d, int code, int64_t x) {
    if (code < 2) d[0] = (uint8_t)x;
    else if (code < 4) o_wr16(d, (uint32_t)x);
    else o_wr32(d, (uint32_t)x);
}

// struct.pack("<f", float(v)) for the spellings -?digits[.digits][e[+-]digits] with at most 15 significant digits and a power of
// ten, the fraction folded in, within +-22: the digits are an integer M < 10^15 < 2^53 and 10^|p| <= 10^22, both exact doubles, so
// ONE multiplication or division gives the correctly rounded double (what float() gives); the cast rounds once more, as pack does.
// Everything else -- inf, nan, more digits, a bare '.', an 'E' -- is not taken (false): the line is odd.  No fused operation can
// arise from a single product or quotient, and this unit is built without fast-math.
AMP_HD bool aux_float(const uint8_t *t, uint32_t fs, uint32_t fe, float &out) {
    uint32_t p = fs;
    bool neg = false;
    if (p < fe && t[p] == '-') { neg = true; ++p; }
    uint64_t M = 0;
    int nsig = 0;
    int64_t nfrac = 0, e = 0;
    uint32_t p0 = p;
    for (; p < fe && (uint32_t)t[p] - '0' <= 9u; ++p) {
        const uint32_t d = (uint32_t)t[p] - '0';
        if (M || d) ++nsig;
        if (nsig <= 15) M = M * 10 + d;
    }
    if (p == p0) return false;
    if (p < fe && t[p] == '.') {
        p0 = ++p;
        for (; p < fe && (uint32_t)t[p] - '0' <= 9u; ++p) {
            const uint32_t d = (uint32_t)t[p] - '0';
            if (M || d) ++nsig;
            if (nsig <= 15) M = M * 10 + d;
            ++nfrac;
        }
        if (p == p0) return false;
    }
    if (p < fe && t[p] == 'e') {
        ++p;
        bool eneg = false;
        if (p < fe && (t[p] == '+' || t[p] == '-')) { eneg = t[p] == '-'; ++p; }
        p0 = p;
        for (; p < fe && (uint32_t)t[p] - '0' <= 9u; ++p) if (e < 100000) e = e * 10 + (int64_t)((uint32_t)t[p] - '0');
        if (p == p0) return false;
        if (eneg) e = -e;
    }
    if (p != fe || nsig > 15) return false;
    const int64_t pw = e - nfrac;
    if (pw < -22 || pw > 22) return false;
    double t10 = 1.0;                                               // 10^k, k <= 22: every product is exact
    for (int64_t k = 0; k < (pw < 0 ? -pw : pw); ++k) t10 *= 10.0;
    const double d = pw >= 0 ? (double)M * t10 : (double)M / t10;
    out = (float)(neg ? -d : d);
    return true;
}
AMP_HD void put_float(uint8_t *d, float f) { uint32_t w; __builtin_memcpy(&w, &f, 4); o_wr32(d, w); }

// One aux field text[fs, fe) as BAM: its size; d != NULL: its bytes, all but the body of a Z / H string (the wave copies that to
// d + 3).  why = the reason the field makes its line odd (then the size means nothing), 0: none.
AMP_HD uint32_t aux_conv(const uint8_t *t, uint32_t fs, uint32_t fe, uint8_t *d, int &why) {
    why = 0;
    if (fe - fs < 5u || t[fs + 2] != ':' || t[fs + 4] != ':' || (uint32_t)t[fs] - 33u > 93u || (uint32_t)t[fs + 1] - 33u > 93u) { why = AMP_SAM_ODD_AUX_TAG; return 0; }
    const uint32_t type = t[fs + 3], vs = fs + 5u, vn = fe - vs;
    if (d) { d[0] = t[fs]; d[1] = t[fs + 1]; }
    if (type == 'A') {
        if (vn != 1u) { why = AMP_SAM_ODD_AUX_A; return 0; }
        if (d) { d[2] = 'A'; d[3] = t[vs]; }
        return 4u;
    }
    if (type == 'i') {
        int64_t x = 0;
        if (!aux_int(t, vs, fe, x)) { why = AMP_SAM_ODD_AUX_INT; return 0; }
        const int code = int_code(x);
        if (code < 0) { why = AMP_SAM_ODD_AUX_INT_RANGE; return 0; }
        if (d) { d[2] = (uint8_t)"cCsSiI"[code]; put_int(d + 3, code, x); }
        return 3u + int_bytes(code);
    }
    if (type == 'f') {
        float f = 0.f;
        if (!aux_float(t, vs, fe, f)) { why = AMP_SAM_ODD_AUX_FLOAT; return 0; }
        if (d) { d[2] = 'f'; put_float(d + 3, f); }
        return 7u;
    }
    if (type == 'Z' || type == 'H') {
        if (d) { d[2] = (uint8_t)type; d[3 + vn] = 0; }
        return 4u + vn;
    }
    if (type != 'B') { why = AMP_SAM_ODD_AUX_TAG; return 0; }
    if (vn == 0) { why = AMP_SAM_ODD_AUX_B; return 0; }
    const uint32_t sub = t[vs];
    int code = -1;                                                  // 0..5: c C s S i I, 6: f
    for (int k = 0; k < 7; ++k) if (sub == (uint32_t)"cCsSiIf"[k]) code = k;
    if (code < 0) { why = AMP_SAM_ODD_AUX_B; return 0; }
    const uint32_t esz = code == 6 ? 4u : int_bytes(code);
    uint32_t count = 0, p = vs + 1u;
    while (p < fe) {
        if (t[p] != ',') { why = AMP_SAM_ODD_AUX_B; return 0; }
        uint32_t q = ++p;
        while (q < fe && t[q] != ',') ++q;
        if (q == p) { why = AMP_SAM_ODD_AUX_B; return 0; }
        uint8_t *e = d ? d + 8 + (size_t)count * esz : nullptr;
        if (code == 6) {
            float f = 0.f;
            if (!aux_float(t, p, q, f)) { why = AMP_SAM_ODD_AUX_FLOAT; return 0; }
            if (e) put_float(e, f);
        } else {
            int64_t x = 0;
            if (!aux_int(t, p, q, x)) { why = AMP_SAM_ODD_AUX_B; return 0; }
            if (!int_fits(code, x)) { why = AMP_SAM_ODD_AUX_B_RANGE; return 0; }
            if (e) put_int(e, code, x);
        }
        ++count; p = q;
    }
    if (d) { d[2] = 'B'; d[3] = (uint8_t)sub; o_wr32(d + 4, count); }
    return 8u + count * esz;
}

// where the aux field behind tab T of line i ends (the line's tabs are [line_tab0[i], line_tab0[i + 1]))
AMP_HD uint32_t aux_end(const Buf &b, int64_t i, const Line &ln, uint32_t T) { return T + 1u < b.line_tab0[i + 1] ? b.tab_pos[T + 1u] : ln.end; }

// aux: lane = tab of the chunk.  A tab with number 10 or more in its line opens an aux field: its BAM size, its verdict.
AMP_HD void lane_aux(const Buf &b, int64_t T) {
    const uint32_t p = b.tab_pos[T], m = b.mask[p >> 4] & 0xFFFFu;
    const int64_t i = (int64_t)((uint32_t)b.rank[p >> 4] + (uint32_t)__builtin_popcount(m & ((1u << (p & 15u)) - 1u)));
    uint32_t sz = 0;
    if (i < b.line_cap && (uint32_t)T - b.line_tab0[i] >= 10u) {
        const Line ln = line_of(b, i);
        int why = 0;
        sz = aux_conv(b.text, p + 1u, aux_end(b, i, ln, (uint32_t)T), nullptr, why);
        if (why) { odd(b, i, why); sz = 0; }
    }
    b.aux_sz[T] = sz;
}

// ---- BAM output: the records (AlignmentWriter.write of bamio.py, mode "wb") -----------------------------------------------------
AMP_HD void lane_bam_size(const Buf &b, int64_t r) {              // r == n_rows: the slot the scan leaves the total in
    const ampbamout::Out &o = b.o;
    uint64_t sz = 0;
    // (the verdict of a deferred amp_sam_process is read where it lies: rows in front of the first failing one)
    const int64_t good = !b.bad_key ? b.good_rows : *b.bad_key == ~0ull ? o.n_rows : (int64_t)(*b.bad_key >> 8);
    if (r < o.n_rows && r < good && row_kept(b, r)) {
        // (the stream has room for three ops more than the line's, and the line has 65,532 at most: see lane_records)
        if (b.new_ncig[r] > b.cig_off32[r + 1] - b.cig_off32[r] + ampbamout::OUT_SPARE_OPS) AMP_ADD64(&o.octl[ampbamout::OCTL_BAD], 1);
        else { sz = (uint64_t)b.row_bsz[r] + 4ull * b.new_ncig[r]; AMP_ADD64(&o.octl[ampbamout::OCTL_ROWS], 1); }
    }
    o.row_off[r] = sz;
}

// One wave per kept row.  Lane 0: block_size, the 32 fixed bytes, the new CIGAR words.  The wave: QNAME from the text; packed
// bases and qualities from the row's slots of the resident batch, where k_sam_pack left them in BAM's own form (nibbles with
// a zero spare nibble, character - 33, 0xFF for '*') -- (l_seq + 1) / 2 + l_seq bytes to copy instead of 2 l_seq bytes of text
// to read and map again; aux fields one per lane (64 at a time), the bodies of Z / H strings by the whole wave.
AMP_HD void lane_bam_record(const Buf &b, int64_t r, uint32_t lane) {
    const ampbamout::Out &o = b.o;
    if (o.octl[ampbamout::OCTL_BAD] || o.row_off[r + 1] == o.row_off[r]) return;
    uint8_t *d = o.stream + o.carry_in + o.row_off[r];
    const int64_t i = b.row_line[r];
    const Line ln = line_of(b, i);
    const uint8_t *t = b.text;
    uint32_t qs, qe, fs, fe;
    field(b, i, ln, 0, qs, qe);
    const uint32_t l_name = qe - qs + 1u, nn = b.new_ncig[r], L = b.lseq[r];
    if (lane == 0) {
        const uint32_t *cg = row_new_cig(b, r);
        int64_t v = 0, rlen = 0;
        for (uint32_t k = 0; k < nn; ++k) {
            const uint32_t op = cg[k] & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += cg[k] >> 4;
        }
        const int64_t pos = b.new_pos[r], end = pos + (rlen ? rlen : 1);
        field(b, i, ln, 2, fs, fe);
        const int rn = name_id(b, fs, fe);
        field(b, i, ln, 6, fs, fe);
        const int rx = (fe - fs == 1 && t[fs] == '=') ? rn : name_id(b, fs, fe);
        o_wr32(d, b.row_bsz[r] - 4u + 4u * nn);
        o_wr32(d + 4, (uint32_t)(rn < 0 ? -1 : rn));
        o_wr32(d + 8, (uint32_t)b.new_pos[r]);
        d[12] = (uint8_t)l_name;
        field(b, i, ln, 4, fs, fe); (void)parse_int(t, fs, fe, v); d[13] = (uint8_t)v;
        o_wr16(d + 14, ampbamout::reg2bin(pos > 0 ? pos : 0, end > 1 ? end : 1));
        o_wr16(d + 16, nn);
        o_wr16(d + 18, b.flag[r]);
        o_wr32(d + 20, L);
        o_wr32(d + 24, (uint32_t)(rx < 0 ? -1 : rx));
        field(b, i, ln, 7, fs, fe); (void)parse_int(t, fs, fe, v); o_wr32(d + 28, (uint32_t)(v - 1));
        o_wr32(d + 32, (uint32_t)b.tlen[r]);
        d[36 + l_name - 1u] = 0;
        for (uint32_t k = 0; k < nn; ++k) o_wr32(d + 36 + l_name + 4 * k, cg[k]);
    }
    wave_copy(d + 36, t + qs, qe - qs, lane);
    uint8_t *sq = d + 36 + l_name + 4u * nn;
    wave_copy(sq, b.seq + 4 * (size_t)b.seq_off8[r], (L + 1u) >> 1, lane);
    wave_copy(sq + ((L + 1u) >> 1), b.qual + 8 * (size_t)b.seq_off8[r], L, lane);
    uint8_t *ax = sq + ((L + 1u) >> 1) + L;
    const uint32_t T0 = b.line_tab0[i] + 10u, T1 = b.line_tab0[i + 1], base = b.aux_sz[T0];
    for (uint32_t T = T0 + lane; T < T1; T += WAVE) {
        int why = 0;
        (void)aux_conv(t, b.tab_pos[T] + 1u, aux_end(b, i, ln, T), ax + (b.aux_sz[T] - base), why);
    }
    for (uint32_t T = T0; T < T1; ++T) {
        const uint32_t as = b.tab_pos[T] + 1u, type = t[as + 3];
        if (type == 'Z' || type == 'H') wave_copy(ax + (b.aux_sz[T] - base) + 3, t + as + 5u, aux_end(b, i, ln, T) - as - 5u, lane);
    }
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
    if (b.bam_mode) {                                               // a chunk has fewer tabs than bytes
        b.tab_cap = cap_bytes + 16;
        b.tab_pos = (uint32_t *)take(((size_t)b.tab_cap + 1) * 4); b.aux_sz = (uint32_t *)take(((size_t)b.tab_cap + 2) * 4);
        b.row_bsz = (uint32_t *)take((LC + 1) * 4);
    }
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
CODEC_KERNEL(k_sam_aux, lane_aux)
CODEC_KERNEL(k_sam_bam_size, lane_bam_size)
__global__ void __launch_bounds__(256) k_sam_fmt_copy(Buf b, int64_t n_rows) {      // one wave per row
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += (int64_t)gridDim.x * 4) lane_fmt_copy(b, r, lane);
}
// One wave per row (four a workgroup), as k_sam_fmt_copy: no LDS, and nothing a lane keeps lives in an array.
__global__ void __launch_bounds__(256) k_sam_bam_records(Buf b) {
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < b.o.n_rows; r += (int64_t)gridDim.x * 4) lane_bam_record(b, r, lane);
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
    // trimmed reads as BAM (amp_sam_set_output, amp_sam_encode)
    bool encoded = false;                             // the rows of the last parse went into the stream
    bool verdict_pending = false;                     // amp_sam_process was deferred: the first failing row is not known here yet
    int64_t bad_row = -1; uint8_t bad_status = 0;     // the verdict of the last amp_sam_process
    unsigned long long h_key = ~0ull;
    ampbamout::Tail tail;
    uint64_t h_new_bytes = 0;                         // (amp_sam_encode_bytes: what its one "row" holds, on its way up)
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
    ampbamout::tail_free(s->tail);
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
    s->parsed = s->processed = s->encoded = false;
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
        if (b.bam_mode) {
            CODEC_RUN(s, k_sam_aux, lane_aux, b.tab_cap, CTL_NTABS);
            CODEC_OK(codec_scan(s->sh, b.aux_sz, b.tab_cap + 1));
        }
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
    s->bad_row = bad;
    s->processed = true; s->verdict_pending = false;
    if (first_bad_row) *first_bad_row = bad;
    return AMP_OK;
}
// the key of a deferred amp_sam_process has come down (h_key)
static void sam_verdict(amp_sam *s) {
    codec_first_bad_of(s->h_key, &s->bad_row, &s->bad_status);
    s->good_rows = s->bad_row >= 0 ? s->bad_row : s->info.n_rows;
    s->verdict_pending = false;
}
static int sam_verdict_now(amp_sam *s) {
    if (!s->verdict_pending) return AMP_OK;
    DevGuard guard(s->sh);
    CODEC_OK(codec_down(s->sh, &s->h_key, s->sh.bad_key, 8));
    CODEC_OK(codec_wait(s->sh));
    sam_verdict(s);
    return AMP_OK;
}

#ifndef AMPSAM_HOSTSIM
// A:896-915 for the rows of the chunk: amp_process_batch_device on the batch of the last parse, results kept in s
int amp_sam_process(amp_sam *s, uint64_t read_base, int64_t *first_bad_row, uint8_t *its_status) {
    if (!s) return AMP_EINVAL;
    if (!s->parsed || s->info.first_odd_line >= 0) return AMP_ESTATE;
    int64_t bad = -1;
    uint8_t st = 0;
    if (!first_bad_row && !its_status) {              // deferred: amp_sam_encode or amp_sam_first_bad brings the verdict down
        CODEC_OK(codec_process(s->sh, s->b, s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, read_base, 6, nullptr, nullptr, true));
        s->processed = s->verdict_pending = true;
        return AMP_OK;
    }
    const int rc = codec_process(s->sh, s->b, s->b, s->info.n_rows, s->info.n_cig, s->info.n_bases_padded, read_base, 6, &bad, &st);
    s->bad_status = st;
    if (its_status) *its_status = st;
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
    uint8_t st = 0;
    const int rc = codec_first_bad(s->sh, s->b, s->info.n_rows, &bad, &st);
    s->bad_status = st;
    if (its_status) *its_status = st;
    return sam_processed(s, rc, bad, first_bad_row);
}
#endif

// out_aln.write(s) of A:911 under the filter of A:910 for the rows in front of the first failing one: AlignmentWriter.write(r, pos=, cigar=)
int amp_sam_format(amp_sam *s, int32_t min_length, int32_t include_no_primer, uint8_t *out, int64_t cap, int64_t *n_bytes, int64_t *n_rows_written) {
    if (!s || !n_bytes || cap < 0 || (cap && !out)) return AMP_EINVAL;
    if (!s->parsed || !s->processed) return AMP_EINVAL;
    CODEC_OK(sam_verdict_now(s));
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

// ---- trimmed reads as BAM -----------------------------------------------------------------------------------
// what the trimmed reads of the run are written as; before the first parse (the tables of a chunk depend on it)
int amp_sam_set_output(amp_sam *s, int32_t mode) {
    if (!s || (mode != AMP_SAM_OUT_TEXT && mode != AMP_SAM_OUT_BAM)) return AMP_EINVAL;
    if ((mode == AMP_SAM_OUT_BAM) == (s->b.bam_mode != 0)) return AMP_OK;
    DevGuard guard(s->sh);
    CODEC_OK(codec_sync(s->sh));
    s->b.bam_mode = mode == AMP_SAM_OUT_BAM ? 1 : 0;
    s->cap_bytes = 0;                                 // the next parse carves its memory anew
    s->parsed = s->processed = false;
    return AMP_OK;
}

static int sam_out_records(amp_sam *s) {
#ifndef AMPSAM_HOSTSIM
    if (s->b.o.n_rows > 0) {
        k_sam_bam_records<<<codec_grid(s->b.o.n_rows * 64), 256, 0, s->sh.stream>>>(s->b);
        if (hipGetLastError() != hipSuccess) return AMP_EHIP;
    }
#else
    for (int64_t r = 0; r < s->b.o.n_rows; ++r) for (uint32_t lane = 0; lane < WAVE; ++lane) lane_bam_record(s->b, r, lane);
#endif
    return AMP_OK;
}

// AlignmentWriter(mode="wb").write(r, pos=, cigar=) + BgzfWriter for the kept rows of the last parse (none when they were encoded
// already, or the chunk was odd: a bare flush)
int amp_sam_encode(amp_sam *s, int32_t min_length, int32_t include_no_primer, int32_t final, amp_bam_out_info *info) {
    if (!s || !info) return AMP_EINVAL;
    if (!s->b.bam_mode) return AMP_ESTATE;
    const bool fresh = s->parsed && !s->encoded && s->info.first_odd_line < 0;
    const int64_t n_rows = fresh ? s->info.n_rows : 0;
    if (n_rows && !s->processed) return AMP_ESTATE;
    DevGuard guard(s->sh);
    const int64_t waits0 = s->sh.waits;
    Buf &b = s->b;
    // the new records: the rows' sizes without their CIGARs came down with the parse, a new CIGAR has three ops more at most
    const int64_t new_bytes = n_rows ? (int64_t)s->h_ctl[CTL_BAM_BYTES] + 4 * (s->info.n_cig + (int64_t)ampbamout::OUT_SPARE_OPS * n_rows) : 0;
    CODEC_OK(ampbamout::tail_begin(s->sh, s->tail, b.o, n_rows, new_bytes, final, 11));
    const bool pending = n_rows && s->verdict_pending;
    b.min_length = min_length; b.include_no_primer = include_no_primer ? 1 : 0; b.good_rows = n_rows ? s->good_rows : 0;
    b.bad_key = pending ? s->sh.bad_key : nullptr;
    if (pending) { b.good_rows = n_rows; CODEC_OK(codec_down(s->sh, &s->h_key, s->sh.bad_key, 8)); }      // (down with the encode's wait)
    if (n_rows) {
        CODEC_RUN(s, k_sam_bam_size, lane_bam_size, n_rows + 1, -1);
        CODEC_OK(codec_scan(s->sh, b.o.row_off, n_rows + 1));
    }
    CODEC_OK(ampbamout::tail_plan<amp_sam>(s->sh, b.o));
    CODEC_OK(sam_out_records(s));
    const int rc = ampbamout::tail_finish<amp_sam>(s->sh, s->tail, b.o, 11, waits0, info);
    if (pending && rc != AMP_EHIP) sam_verdict(s);    // (the wait was reached: the key is here)
    if (rc) return rc;
    if (fresh) s->encoded = true;
    return AMP_OK;
}

// the verdict of the last amp_sam_process: *first_bad_row = the first row whose status is not AMP_RS_OK and *its_status that
// status, -1 and 0 when there is none.  Waits only when the process was deferred and no encode has brought the verdict down.
int amp_sam_first_bad(amp_sam *s, int64_t *first_bad_row, uint8_t *its_status) {
    if (!s) return AMP_EINVAL;
    if (!s->parsed || !s->processed) return AMP_ESTATE;
    CODEC_OK(sam_verdict_now(s));
    if (first_bad_row) *first_bad_row = s->bad_row;
    if (its_status) *its_status = s->bad_status;
    return AMP_OK;
}

// waits for the device since the amp_sam was made (growth of a buffer does not count): tests and tools
int64_t amp_sam_waits(amp_sam *s) { return s ? s->sh.waits : -1; }

// the same tail over [carry | n record bytes made on the host]: how a chunk that went through the Python codec joins the stream
int amp_sam_encode_bytes(amp_sam *s, const uint8_t *bytes, int64_t n, int32_t final, amp_bam_out_info *info) {
    if (!s || !info || n < 0 || n >= (1ll << 31) || (n && !bytes)) return AMP_EINVAL;
    if (!s->b.bam_mode) return AMP_ESTATE;
    DevGuard guard(s->sh);
    const int64_t waits0 = s->sh.waits;
    ampbamout::Out &o = s->b.o;
    CODEC_OK(ampbamout::tail_begin(s->sh, s->tail, o, 0, n, final, 11));
    s->h_new_bytes = (uint64_t)n;
    CODEC_OK(codec_up(s->sh, o.stream + o.carry_in, bytes, (size_t)n));
    CODEC_OK(codec_up(s->sh, o.row_off, &s->h_new_bytes, 8));
    CODEC_OK(ampbamout::tail_plan<amp_sam>(s->sh, o));
    return ampbamout::tail_finish<amp_sam>(s->sh, s->tail, o, 11, waits0, info);
}

// the framed blocks, the blocks' sizes and the uncompressed stream of the last encode, as their amp_bam_* siblings
int amp_sam_encoded_to_host(amp_sam *s, uint8_t *dst, int64_t cap) { return s ? ampbamout::tail_encoded_to_host(s->sh, s->tail, s->b.o, dst, cap, 15) : AMP_EINVAL; }
int amp_sam_encoded_blocks(amp_sam *s, uint32_t *blk_len, int64_t cap) { return s ? ampbamout::tail_encoded_blocks(s->sh, s->tail, s->b.o, blk_len, cap) : AMP_EINVAL; }
int amp_sam_stream_to_host(amp_sam *s, int64_t from, int64_t n, uint8_t *dst) { return s ? ampbamout::tail_stream_to_host(s->sh, s->tail, s->b.o, from, n, dst) : AMP_EINVAL; }

#ifdef AMPSAM_HOSTSIM
// Entry points of the host twin alone (not part of include/amplihip.h): the DEFLATE encoder of its encodes (amp_deflate.hip's host
// phases, ampdf_hostsim_blocks), and the guard bytes behind the encoder's buffers (0: untouched, else 1 + the buffer's number)
int amp_sam_twin_set_deflater(amp_sam *s, amp_bam_twin_deflate_fn fn) {
    if (!s) return AMP_EINVAL;
    s->tail.twin_deflate = fn;
    return AMP_OK;
}
int amp_sam_twin_guards(amp_sam *s) { return s ? ampbamout::tail_guards(s->tail) : AMP_EINVAL; }
#endif

}  // extern "C"
