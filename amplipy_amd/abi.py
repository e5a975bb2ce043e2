"""ctypes mirrors of the structs and enums in include/amplihip.h (kept in the same order)."""
from __future__ import annotations

import ctypes as C

import numpy as np

NSYM = 6
SYMBOLS = "ACGTN-"
SEQ_ALIGN = 8

AMP_OK = 0
RC_NAMES = {0: "AMP_OK", -1: "AMP_EINVAL", -2: "AMP_ENOMEM", -3: "AMP_EHIP", -4: "AMP_ENODEV",
            -5: "AMP_ESTATE", -6: "AMP_EOVERFLOW", -7: "AMP_ERCCL"}

# amp_read_status -> exception class AmpliPy raises for that input
READ_STATUS_EXC = {0: None, 1: IndexError, 2: IndexError, 3: IndexError, 4: KeyError,
                   5: AttributeError, 6: TypeError, 7: ValueError, 8: IndexError, 9: TypeError}
READ_STATUS_NAMES = {0: "OK", 1: "INDEX_REF", 2: "INDEX_PAIRS", 3: "INDEX_QUERY", 4: "KEY_BASE",
                     5: "NO_SEQ", 6: "NO_QUAL", 7: "CLIP", 8: "CIGAR_OP", 9: "TYPE"}

TRIM_PRIMER_START, TRIM_PRIMER_END, TRIM_QUALITY = 1, 2, 4

INS_EVENT_DTYPE = np.dtype([("ref_pos", "<i4"), ("read", "<u4"), ("q_from", "<i4"), ("q_to", "<i4")])
# amp_ins_run: one record per (ref_pos, allele) of amp_aggregate_ins_events
INS_RUN_DTYPE = np.dtype([("ref_pos", "<i4"), ("read", "<u4"), ("q_from", "<i4"), ("q_to", "<i4"), ("count", "<u4"), ("reserved", "<u4")])


class AmpInsEvent(C.Structure):
    _fields_ = [("ref_pos", C.c_int32), ("read", C.c_uint32), ("q_from", C.c_int32), ("q_to", C.c_int32)]


class AmpReads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("tlen", C.c_void_p),
                ("lseq", C.c_void_p), ("cig_off", C.c_void_p), ("cig", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p)]


class AmpTrimOut(C.Structure):
    _fields_ = [("new_pos", C.c_void_p), ("new_ncig", C.c_void_p), ("new_cig", C.c_void_p),
                ("ref_len", C.c_void_p), ("trim_flags", C.c_void_p), ("status", C.c_void_p)]


class AmpDevReads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("tlen", C.c_void_p),
                ("lseq", C.c_void_p), ("cig_off32", C.c_void_p), ("cig", C.c_void_p),
                ("seq_off8", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p),
                ("n_cig", C.c_int64), ("n_bases_padded", C.c_int64)]


class AmpCallParams(C.Structure):
    _fields_ = [("min_depth_consensus", C.c_int32), ("min_depth_variants", C.c_int32),
                ("min_freq_consensus", C.c_double), ("min_freq_variants", C.c_double),
                ("run_consensus", C.c_int32), ("run_variants", C.c_int32),
                ("full_ranking", C.c_int32), ("reserved", C.c_int32)]


class AmpCallView(C.Structure):
    _fields_ = [("consensus", C.c_void_p), ("vars", C.c_void_p), ("relevant", C.c_void_p),
                ("n_vars", C.c_int64), ("n_relevant", C.c_int64)]


POS_CALL_DTYPE = np.dtype([("total_depth", "<u4"), ("ref_count", "<u4"), ("order", "<u4"), ("consensus_sym", "i1"),
                           ("flags", "u1"), ("alt_mask", "u1"), ("pad", "u1")])
CALL_VARIANT, CALL_GT_HAS_REF, CALL_INS_RELEVANT = 1, 2, 4
VAR_REC_DTYPE = np.dtype([("pos", "<i4"), ("total_depth", "<u4"), ("ref_count", "<u4"), ("n_alt", "u1"),
                          ("gt_has_ref", "u1"), ("alt_col", "u1", (6,)), ("alt_count", "<u4", (6,))])
assert VAR_REC_DTYPE.itemsize == 44

# ---- strand and base-quality tallies (amp_strand_*): rev uint32[G][NSYM], qsum uint64[G][STRAND_QSUM_COLS] ----
STRAND_QSUM_COLS = 5
STRAND_CELLS = 11          # NSYM + STRAND_QSUM_COLS: the columns of one position when both tables travel as one

# ---- per-amplicon allele counts (amp_amplicon_*): counts uint32[sum of spans][NSYM], reads uint64[n_amp + 1] ----
AMPLICON_MAX_CELLS = 1 << 22   # span positions of all amplicons together; more is refused with AMP_EINVAL

# ---- codon tallies (amp_codon_*): codon uint32[n_slots][CODON_CELLS], reads uint64[2] ----
CODON_CELLS = 65               # the 64 triplets (16 b0 + 4 b1 + b2, A C G T as 0 1 2 3), then broken
CODON_MAX_SLOTS = 1 << 20      # more is refused with AMP_EINVAL

# ---- deletion events (amp_del_*): amp_del_event[used], amp_del_info ----
DEL_LOG2_DEFAULT, DEL_LOG2_MIN, DEL_LOG2_MAX = 20, 4, 28       # slots of the device table (16 bytes each): 0 asks for the default
DEL_EVENT_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("count", "<u4"), ("rev", "<u4")])
DEL_INFO_FIELDS = ("used", "capacity", "lost")                  # amp_del_info, uint64 each
assert DEL_EVENT_DTYPE.itemsize == 16

# ---- insertion evidence (amp_insev_*): amp_insev_entry[used], amp_insev_info = amp_del_info ----
INSEV_LOG2_DEFAULT, INSEV_LOG2_MIN, INSEV_LOG2_MAX = 20, 4, 28  # slots of the device table (64 bytes each): 0 asks for the default
INSEV_BINS = 7                                                  # rp_bin's: d < 2, 2-3, 4-7, 8-15, 16-31, 32-63, >= 64
INSEV_STRIDE = 512 * 256                                        # AMP_INSEV_STRIDE: events the kernel's grid takes in one stride
INSEV_ENTRY_DTYPE = np.dtype([("ref_pos", "<i4"), ("len", "<i4"), ("hash", "<u8"), ("count", "<u4"), ("rev", "<u4"), ("noqual", "<u4"),
                              ("qsum", "<u8"), ("bin", "<u4", (INSEV_BINS,))], align=True)
assert INSEV_ENTRY_DTYPE.itemsize == 72 and INSEV_ENTRY_DTYPE.fields["qsum"][1] == 32

# ---- co-occurrence of listed mutations (amp_cooc_*): cooc uint32[n_sets][COOC_CELLS], reads uint64[2] ----
COOC_CELLS = 65                # the 64 patterns (site 0 is bit 0), then partial
COOC_SITES = 6                 # sites of a set at most
COOC_MAX_SETS = 1 << 16        # more is refused with AMP_EINVAL
COOC_MAX_SPAN = 1 << 16        # last site's position minus the first site's, at most

# ---- error profile (amp_errprof_*): cyc uint64[2][EP_CYCLES][2], qualt uint64[2][EP_QUALS][2], sub uint64[2][2][2][4][4], reads uint64[2] ----
EP_CYCLES = 512                # cycles from the 5' end of the stored SEQ; the last bin is open-ended
EP_QUALS = 94                  # reported qualities; the last bin is open-ended
EP_CYC_SHAPE, EP_QUAL_SHAPE, EP_SUB_SHAPE = (2, EP_CYCLES, 2), (2, EP_QUALS, 2), (2, 2, 2, 4, 4)

# ---- read haplotypes per region (amp_hap_*): amp_hap_entry[used], amp_hap_info, tally uint64[n_regions][HAP_TALLY_COLS], reads uint64[2] ----
HAP_MAX_DIFFS = 13             # differences of a key at most; a read with more is tallied as OVERFLOW
HAP_MAX_REGION = 4096          # positions of a region at most
HAP_MAX_REGIONS = 1 << 16      # more is refused with AMP_EINVAL
HAP_TALLY_COLS = 6
HAP_COVER, HAP_REF, HAP_REF_REV, HAP_LOWQ, HAP_OVERFLOW, HAP_EDGE = range(6)       # the columns of tally
HAP_KIND_N, HAP_KIND_DEL = 4, 5                                  # kinds 0..3: a substitution to A C G T
HAP_LOG2_DEFAULT, HAP_LOG2_MIN, HAP_LOG2_MAX = 20, 4, 28        # slots of the device table (64 bytes each): 0 asks for the default
HAP_ENTRY_DTYPE = np.dtype([("head", "<u4"), ("diff", "<u4", (HAP_MAX_DIFFS,)), ("count", "<u4"), ("rev", "<u4")])
HAP_INFO_FIELDS = ("used", "capacity", "lost")                   # amp_hap_info, uint64 each
assert HAP_ENTRY_DTYPE.itemsize == 64

# ---- read-position tallies per allele (amp_readpos_*): hist uint32[G][NSYM][RP_BINS] ----
RP_BINS = 7                    # distance-to-end bins: d < 2, 2-3, 4-7, 8-15, 16-31, 32-63, >= 64
RP_EDGES = (0, 2, 4, 8, 16, 32, 64)       # the least distance of each bin
RP_CELLS = 42                  # NSYM * RP_BINS: the columns of one position on the wire

# ---- QC report (amp_qc_*) ----
QC_MAX_DEPTHS = 4


class AmpQcParams(C.Structure):
    _fields_ = [("n_primers", C.c_int32), ("starts", C.c_void_p), ("ends", C.c_void_p), ("primer_pos_offset", C.c_int32),
                ("min_length", C.c_int32), ("include_no_primer", C.c_int32), ("n_regions", C.c_int32),
                ("region_start", C.c_void_p), ("region_end", C.c_void_p), ("n_depths", C.c_int32),
                ("depths", C.c_uint32 * QC_MAX_DEPTHS)]


# amp_qc_reads, in the order of the struct
QC_READ_FIELDS = ("rows", "errors", "primer_start", "primer_end", "primer_both", "primer_none", "quality",
                  "kept", "dropped_short", "dropped_no_primer", "ref_bases_in", "ref_bases_out")
QC_REGION_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("depth_sum", "<u8"), ("depth_min", "<u4"), ("depth_max", "<u4"),
                            ("covered", "<u4", (QC_MAX_DEPTHS,))])
assert QC_REGION_DTYPE.itemsize == 40

# ---- QC report, soft-clip sites (amp_qc_clips_*): table uint32[ref_len + 1][2][CLIP_CELLS], scalars uint64[CLIP_SCALARS] ----
CLIP_K = 16                    # clipped bases kept per site, nearest the junction first
CLIP_COLS = 5                  # A C G T other
CLIP_CELLS = 2 + CLIP_K * CLIP_COLS      # reads, rev, comp[j][c]
CLIP_LEFT, CLIP_RIGHT = 0, 1
CLIP_SCALARS = 4
CLIP_SCALAR_FIELDS = ("scanned", "skipped", "left", "right")
CLIP_MIN_MAX = 64              # clip_min: 1..64


def ptr(a):
    """Address of a contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def reads_struct(batch):
    """AmpReads view of a ReadBatch; the batch must outlive the struct."""
    return AmpReads(batch.n, ptr(batch.pos), ptr(batch.flag), ptr(batch.tlen), ptr(batch.lseq),
                    ptr(batch.cig_off), ptr(batch.cig), ptr(batch.seq_off), ptr(batch.seq), ptr(batch.qual))


class TrimResult:
    """Host arrays receiving amp_trim_out (new CIGAR of read i at cig_off[i] + 3*i)."""

    def __init__(self, batch):
        n = batch.n
        self.batch = batch
        self.new_pos = np.zeros(n, np.int32)
        self.new_ncig = np.zeros(n, np.uint32)
        self.new_cig = np.zeros(batch.cig.size + 3 * n, np.uint32)
        self.ref_len = np.zeros(n, np.int32)
        self.trim_flags = np.zeros(n, np.uint8)
        self.status = np.zeros(n, np.uint8)

    def struct(self):
        return AmpTrimOut(ptr(self.new_pos), ptr(self.new_ncig), ptr(self.new_cig), ptr(self.ref_len),
                          ptr(self.trim_flags), ptr(self.status))

    def compact_cigars(self):
        """All reads' new CIGAR words concatenated in read order (slack between slots dropped)."""
        n = self.new_ncig.astype(np.int64)
        start = self.batch.cig_off[:-1].astype(np.int64) + 3 * np.arange(n.size, dtype=np.int64)
        tot = int(n.sum())
        if tot == 0:
            return np.zeros(0, np.uint32)
        first = np.repeat(start - (np.cumsum(n) - n), n)
        return self.new_cig[first + np.arange(tot, dtype=np.int64)]

    def cigar_ops(self, i):
        o = int(self.batch.cig_off[i]) + 3 * i
        return [(int(v) & 15, int(v) >> 4) for v in self.new_cig[o:o + int(self.new_ncig[i])]]

    def cigar_string(self, i):
        from .segment import format_cigar
        return format_cigar(self.cigar_ops(i))
