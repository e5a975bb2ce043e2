/*
 * amplihip.h -- C ABI of libamplihip.so, the MI355X (gfx950) engine behind AmpliPy's
 * trim + pileup + call path.
 *
 * AmpliPy (the reference) has no FFI of its own: its hot path is three Python function
 * seams called once per read from run_amplipy's loop (AmpliPy.py:896-915):
 *     trim_read(s, min_primer_start, max_primer_end, max_primer_len, min_quality, window)
 *                                                         AmpliPy.py:426-687, called :907
 *     update_base_counts(symbol_counts_at_ref_pos, s, min_quality)
 *                                                         AmpliPy.py:690-753, called :915
 *     alleles_from_counts(symbol_counts) + calling loop   AmpliPy.py:756-771, :917-952
 * plus find_overlapping_primers (AmpliPy.py:174-209) which builds trim_read's two tables.
 * A per-read FFI call would cost more than the work, so the replacement is batch-level:
 * one call takes a packed structure-of-arrays batch of reads and performs, for every read
 * in order, exactly what :907 and :915 do.  Each entry point below names the reference
 * lines it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds to AmpliPy.py.
 *
 * Conventions
 *   - every function returns AMP_OK (0) or a negative amp_rc; nothing throws or aborts
 *   - the caller owns every buffer it passes; a ctx owns its device memory
 *   - one ctx per device; a ctx is not thread-safe; different ctxs are independent
 *   - there is NO CPU fallback: amp_ctx_create fails with AMP_ENODEV without a GPU
 *   - all integers little-endian, arrays contiguous
 */
#ifndef AMPLIHIP_H
#define AMPLIHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMP_ABI_VERSION 1
#define AMP_NSYM 6 /* count-table columns, in this order: A C G T N '-'  (AmpliPy.py:892) */
#define AMP_SEQ_ALIGN 8 /* every read starts on a multiple of 8 bases in seq/qual */
#define AMP_DEV_COLS 7 /* device table: uint32[ref_len][6] counts, then uint32[ref_len] insertion-event tally */

typedef enum amp_rc {
    AMP_OK = 0,
    AMP_EINVAL = -1,    /* bad argument (null pointer, negative size, window < 1 ...) */
    AMP_ENOMEM = -2,    /* host or device allocation failed */
    AMP_EHIP = -3,      /* a HIP runtime call failed (see amp_last_error) */
    AMP_ENODEV = -4,    /* no usable gfx950 device */
    AMP_ESTATE = -5,    /* call order violated (e.g. trim requested before amp_set_primers) */
    AMP_EOVERFLOW = -6, /* an output buffer supplied by the caller is too small */
    AMP_ERCCL = -7      /* RCCL not available / collective failed */
} amp_rc;

/*
 * Per-read status: the inputs on which the reference raises.  The
 * engine reports the condition instead of a result; amp_read_status_exception() names the
 * Python exception class AmpliPy raises for it.  When any read of a batch has a non-zero
 * status the batch's count contribution is unspecified (the reference would have died).
 */
typedef enum amp_read_status {
    AMP_RS_OK = 0,
    AMP_RS_INDEX_REF = 1,   /* IndexError: reference coordinate outside [0, ref_len)   :450-451, :715, :745, :753 */
    AMP_RS_INDEX_PAIRS = 2, /* IndexError: insertion run reaches the end of the pairs   :734 */
    AMP_RS_INDEX_QUERY = 3, /* IndexError: query index beyond the stored SEQ/QUAL       :718 */
    AMP_RS_KEY_BASE = 4,    /* KeyError: counted base is not one of A C G T N           :753 */
    AMP_RS_NO_SEQ = 5,      /* AttributeError: SEQ is '*'                               :702 */
    AMP_RS_NO_QUAL = 6,     /* TypeError: QUAL is '*'                                   :561-562, :718 */
    AMP_RS_CLIP = 7,        /* ValueError: hard clip inside soft clip (pysam accessor)  :561, :700-701 */
    AMP_RS_CIGAR_OP = 8,    /* IndexError: CIGAR op code >= 9                           :378, :404, :474 */
    AMP_RS_TYPE = 9         /* TypeError: None arithmetic (insertion followed by a deletion at ref 0) :736 */
} amp_read_status;

/* bits of trim_flags[i]: trim_read's three return values (AmpliPy.py:687) */
#define AMP_TRIM_PRIMER_START 1u
#define AMP_TRIM_PRIMER_END 2u
#define AMP_TRIM_QUALITY 4u

typedef struct amp_ctx amp_ctx;

/* One insertion allele observation (AmpliPy.py:730-748): the string is
 * SEQ[q_from:q_to] of read `read` (bounds already resolved, 0 <= q_from <= q_to <= l_seq),
 * counted at reference position ref_pos. */
typedef struct amp_ins_event {
    int32_t ref_pos;
    uint32_t read; /* row in the batch, plus the batch's read_base (amp_process_batch*) */
    int32_t q_from;
    int32_t q_to;
} amp_ins_event;

/*
 * Packed read batch.  Rows are the reads the reference's loop does not skip (mapped, with a
 * CIGAR: AmpliPy.py:902).  seq is 4-bit BAM codes "=ACMGRSVTWYHKDBN", high nibble first;
 * qual is Phred bytes, first byte 0xFF = QUAL '*'; l_seq 0 = SEQ '*'.  Offsets in `seq_off`
 * are in BASES and index both qual (bytes) and seq (nibbles); each must be a multiple of
 * AMP_SEQ_ALIGN.  cig is BAM's `len<<4 | op`.
 */
typedef struct amp_reads {
    int64_t n_reads;
    const int32_t *pos;       /* [n]   0-based leftmost coordinate (reference_start) */
    const uint16_t *flag;     /* [n]   SAM FLAG; bits 0x1 and 0x10 are read */
    const int32_t *tlen;      /* [n]   template_length */
    const uint32_t *lseq;     /* [n]   query_length */
    const uint64_t *cig_off;  /* [n+1] */
    const uint32_t *cig;      /* [cig_off[n]] */
    const uint64_t *seq_off;  /* [n+1] */
    const uint8_t *seq;       /* [seq_off[n]/2] */
    const uint8_t *qual;      /* [seq_off[n]] */
} amp_reads;

/*
 * Per-read results of trim_read (AmpliPy.py:426-687) and of the write filter's
 * reference_length (AmpliPy.py:910).  Read i's new CIGAR is written at
 * new_cig + cig_off[i] + 3*i, new_ncig[i] ops long (a trim adds at most 3 ops), so
 * new_cig needs cig_off[n] + 3*n entries.  Any pointer may be NULL to skip that output.
 */
typedef struct amp_trim_out {
    int32_t *new_pos;     /* [n] */
    uint32_t *new_ncig;   /* [n] */
    uint32_t *new_cig;    /* [cig_off[n] + 3n] */
    int32_t *ref_len;     /* [n] reference_length after trimming */
    uint8_t *trim_flags;  /* [n] AMP_TRIM_* bits */
    uint8_t *status;      /* [n] amp_read_status */
} amp_trim_out;

/* Same batch with every pointer in DEVICE memory and 32-bit offsets:
 * cig_off32[i] = cig_off[i], seq_off8[i] = seq_off[i] / 8.  seq and qual must be 8-byte aligned
 * and have 16 bytes of readable slack after the last read (the kernels use 8- and 16-byte
 * vector loads that may start in a read's last 8 bytes). */
typedef struct amp_dev_reads {
    int64_t n_reads;
    const int32_t *pos;
    const uint16_t *flag;
    const int32_t *tlen;
    const uint32_t *lseq;
    const uint32_t *cig_off32; /* [n+1] */
    const uint32_t *cig;
    const uint32_t *seq_off8;  /* [n+1] */
    const uint8_t *seq;
    const uint8_t *qual;
    int64_t n_cig;             /* cig_off32[n], known to the host */
    int64_t n_bases_padded;    /* padded bases of the rows: (seq_off8[n] - seq_off8[0]) * 8; only its mean per row is used (it picks
                                * the tile geometry of the fast kernel: a value that is too large costs speed, not correctness) */
} amp_dev_reads;

/* ---- library ------------------------------------------------------------------------ */
int amp_version(void);                        /* AMP_ABI_VERSION */
const char *amp_strerror(int rc);
const char *amp_last_error(const amp_ctx *ctx); /* text of the last failing HIP call */
const char *amp_read_status_exception(int status); /* "IndexError", "KeyError", ... */
int amp_device_count(void);

/* ---- primer tables: find_overlapping_primers, AmpliPy.py:174-209 (host, once per run) --
 * primers must be sorted ascending by (start, end) like AmpliPy.py:257.  Writes -1 for
 * None.  max_primer_len = max(end - start) (AmpliPy.py:876). */
int amp_find_overlapping_primers(int32_t ref_len, int32_t n_primers, const int32_t *starts,
                                 const int32_t *ends, int32_t primer_pos_offset,
                                 int32_t *min_primer_start, int32_t *max_primer_end,
                                 int32_t *max_primer_len);

/* ---- context -------------------------------------------------------------------------- */
/* Allocates the zeroed count table uint32[ref_len][AMP_NSYM] on `device` (AmpliPy.py:892). */
int amp_ctx_create(amp_ctx **out, int device, int32_t ref_len);
void amp_ctx_destroy(amp_ctx *ctx);
/* Optional: run all work of this ctx on the caller's HIP stream (hipStream_t). */
int amp_ctx_set_stream(amp_ctx *ctx, void *hip_stream);
/* Optional: use caller-owned DEVICE memory (uint32[ref_len*AMP_DEV_COLS], e.g. a torch
 * tensor) as the device table so torch.distributed can reduce it in place. Contents are kept. */
int amp_ctx_bind_counts(amp_ctx *ctx, void *dev_counts);

/* Tables consumed by trim_read (AmpliPy.py:450-452); host pointers, length ref_len. */
int amp_set_primers(amp_ctx *ctx, const int32_t *min_primer_start,
                    const int32_t *max_primer_end, int32_t max_primer_len);
/* min_quality / sliding_window_width of AmpliPy.py:907,915; do_trim = run_trim,
 * do_count = run_variants or run_consensus (AmpliPy.py:906, 914).
 * Any window >= 1 and any min_quality >= 0 give the reference's results; the FAST kernels (closed-form trims, one lane per
 * read) are built for windows of 1..8 bases and min_quality <= 128: a run outside of that takes the general tile kernel for
 * every read (about 1.5 x the time per batch, same results).  The third-generation kernel (variant 6) additionally needs
 * min_quality >= 1. */
int amp_set_params(amp_ctx *ctx, int32_t min_quality, int32_t window, int32_t do_trim,
                   int32_t do_count);

/* ---- the hot path: AmpliPy.py:896-915 for a whole batch --------------------------------
 * Host-pointer form: stages the batch to the device, runs the kernels, copies `out` back.
 * read_base is added to amp_ins_event.read so events of several batches stay distinct. */
int amp_process_batch(amp_ctx *ctx, const amp_reads *reads, uint64_t read_base,
                      const amp_trim_out *out);
/* Device-pointer form: inputs and outputs already resident in HBM; asynchronous on the
 * ctx stream (outputs are valid after amp_sync). */
int amp_process_batch_device(amp_ctx *ctx, const amp_dev_reads *reads, uint64_t read_base,
                             const amp_trim_out *dev_out);
int amp_sync(amp_ctx *ctx);

/* Time spent in the kernels of the last amp_process_batch* call, measured with HIP events
 * on the ctx stream: total, and the dominant (CIGAR-scan) kernel alone. */
int amp_last_kernel_ms(amp_ctx *ctx, float *total_ms, float *scan_ms);
/* split != 0: also time the first (dominant) kernel of every pass on its own; the extra event leaves the GPU idle for a
 * few microseconds behind that kernel, so it is off by default and scan_ms then repeats total_ms. */
int amp_set_timing(amp_ctx *ctx, int split);

/* ---- accumulated state ----------------------------------------------------------------- */
int amp_get_counts(amp_ctx *ctx, uint32_t *counts /* [ref_len][AMP_NSYM] host */);
int amp_add_counts(amp_ctx *ctx, const uint32_t *counts /* host, added element-wise */);
/* buf == NULL: *n = an upper bound of the events recorded so far (list slots in use; reads with long
 * CIGARs reserve a slice and may leave part of it unused).  buf != NULL (cap >= that bound): the events
 * are copied and *n = their exact number. */
int amp_get_ins_events(amp_ctx *ctx, int64_t *n, amp_ins_event *buf, int64_t cap);
/* The same, after which the event list is empty again (the per-position tally of amp_get_counts stays): for runs of many
 * batches, where the text of the events is taken batch by batch.  Call with buf == NULL first for the size, like above. */
int amp_drain_ins_events(amp_ctx *ctx, int64_t *n, amp_ins_event *buf, int64_t cap);
void *amp_counts_device_ptr(amp_ctx *ctx);
/* On-device aggregation of the insertion events recorded since the last amp_reset / drain (the dict
 * keys of AmpliPy.py:745-748, consumed at A:767-771): the device sorts the events by (ref_pos, allele length, a 64-bit hash of
 * the allele) and run-length encodes them.  One amp_ins_run per run of events with the same position and the same allele text:
 * `count` events and one representative, an event of that run (its text through amp_event_strings); `reserved` is 0.  The runs
 * are ordered by (ref_pos, allele length).  Equal alleles are adjacent, so an allele is one run, unless two alleles of one
 * position and length collide in the hash and interleave (never seen): then an allele comes as more than one run, and the
 * consumer sums counts by (ref_pos, text).  A run never mixes alleles.
 * reads = the device batch the events' read ids refer to, read_base as given to amp_process_batch* (ids are taken relative to
 * read_base modulo 2^32; reads == NULL: the batch of the last amp_process_batch call, still staged on the device --
 * AMP_ESTATE when there is none, on a ctx that has taken no batch for one, whether or not buf is NULL and whether or not there
 * are events).  buf == NULL: *n_runs = an upper bound (list slots in use); buf != NULL (cap >= that bound): the records,
 * *n_runs = their number.  AMP_EOVERFLOW when a buffer reserved with amp_reserve_events was too small for the events.
 * drain != 0: the event list is empty afterwards (the per-position tally of amp_get_counts stays). */
typedef struct amp_ins_run {
    amp_ins_event first;
    uint32_t count;
    uint32_t reserved;
} amp_ins_run;
int amp_aggregate_ins_events(amp_ctx *ctx, const amp_dev_reads *reads, uint64_t read_base, int drain, int64_t *n_runs,
                             amp_ins_run *buf, int64_t cap);
/* Sum the device tables (counts + insertion tally) over the ranks of an RCCL communicator (ncclComm_t) onto rank `root`
 * (root < 0: all ranks).  comm == NULL is a no-op (single GPU). */
int amp_reduce(amp_ctx *ctx, void *rccl_comm, int root);
int amp_reset(amp_ctx *ctx); /* zero the count table and drop recorded events */
/* Number of reads with a non-zero amp_read_status since the last amp_reset. */
int amp_error_reads(amp_ctx *ctx, int64_t *n);
/* The reference's coordinate helpers for n CIGARs at once, computed on the device by the functions the kernels use:
 *   pos_on_query_out[i] = get_pos_on_query(cigar_i, ref_pos[i], ref_start[i])        (AmpliPy.py:389-412)
 *   pos_on_ref_out[i]   = get_pos_on_ref(cigar_i, query_pos[i], ref_start[i])        (AmpliPy.py:363-386)
 *   fixed_cig[cig_off[i] ..] / fixed_n[i] = fix_cigar(cigar_i)                       (AmpliPy.py:415-423)
 * cig_off[n + 1] / cig as in amp_reads (32-bit offsets, BAM words); status[i] = amp_read_status of get_pos_on_query in the
 * low nibble and of get_pos_on_ref in the high nibble (an op code >= 9 makes the reference's table look-up fail in the helper
 * that reaches it; fix_cigar consults no table and never fails).  Host pointers; synchronous. */
int amp_coordinate_helpers(amp_ctx *ctx, int64_t n, const uint32_t *cig_off, const uint32_t *cig, const int32_t *ref_start,
                           const int32_t *ref_pos, const int32_t *query_pos, int32_t *pos_on_query_out, int32_t *pos_on_ref_out,
                           uint32_t *fixed_cig, uint32_t *fixed_n, uint8_t *status);
/* Development aid: the 16 raw device counters ([0] events, [1] event bound, [2] error reads,
 * [3] deferred reads, [8..13] per-phase cycle sums when AMPLIHIP_PHASES has bit 0x100). */
int amp_debug_counters(amp_ctx *ctx, uint64_t *out16);
/* Development aid (AMPLIHIP_PHASES bit 0x100): per tile-kernel block {cycles, window rebases,
 * quality-scan chunks, counting chunks} of the last launch. */
int amp_debug_blocks(amp_ctx *ctx, uint32_t *out, int cap_blocks, int *n_blocks);
/* Development aid (tests/test_gpu_general_grid.py; no part of the interface a caller builds on): launch the general pass / the
 * heavy pass behind a fast kernel with so many blocks, at most their full grids; 0 = by the rule at amp_set_cu_share.  Results
 * do not depend on it. */
int amp_debug_second_grids(amp_ctx *ctx, int gen_blocks, int heavy_blocks);
/* ... and the blocks the two were launched with in the ctx's last pass behind a fast kernel (0 before the first). */
int amp_debug_last_second_grids(amp_ctx *ctx, int *gen_blocks, int *heavy_blocks);
/* Slots per shard the insertion-event list has room for as it stands (development aid: the tests look at it to see the list
 * grow between batches). */
int amp_debug_event_capacity(amp_ctx *ctx, int64_t *per_shard);
/* Pre-size the insertion-event buffer.  Without it every amp_process_batch* call first runs
 * a small bound kernel and synchronises to size the buffer; with it the call is fully
 * asynchronous and amp_get_ins_events reports AMP_EOVERFLOW if the reservation was short.
 * `cap` is per list shard (there are 8, and any of them may receive most of a batch's events); size it for twice the
 * events of a batch plus 64 slots per wave of the fast kernel (8 per CU) and of the many-op kernel (24 per CU): waves
 * reserve list slots 64 at a time and leave some unused (read-out drops them). */
int amp_reserve_events(amp_ctx *ctx, int64_t cap);
/* 0 (default) = chosen per batch between 4, 5 and 7 by its mean padded read length (up to 152: 4), the window (8: 5; any other than the
 * default of 4: 4 whatever the length, the builds for longer reads exist for that window only) and its mean number
 * of CIGAR ops (long reads with three ops a read and more: 7).  4 = the fast kernel (closed-form trim +
 * pileup of reads with one match op or one insertion / deletion of up to 152 bases, every byte loaded once) followed by the
 * general pass over the reads it hands over; 5 = its second generation (reads consumed from LDS staging buffers,
 * branch-free closed forms, reads of up to 304 bases); 6 = its third generation (reads of up to 160 bases sorted into class
 * lists per block, rows gathered by LDS-DMA, three passes from LDS: amp_fast6.hpp; opt-in); 7 = the second generation driven by
 * per-block lists of reads binned by length (tiles of one length class, two lanes per read of more than 144 bases, reads for the
 * general pass never in a tile: amp_fast7.hpp; for batches of mixed read lengths); 2 = the fused tile kernel over every read; 1 = one-lane-per-read
 * kernels and 3 = the tile kernel's work cut into three kernels -- 1 to 3 are kept for on-GPU A/B checks (all give
 * identical results).  Runs with window > 8 or min_quality > 128 use variant 2 whichever of 0 and 4 to 7 is set, runs with
 * min_quality 0 variant 4 where 6 is set. */
int amp_set_kernel_variant(amp_ctx *ctx, int variant);
/* 1 when runs with the ctx's current parameters take a fast kernel (window 1..8, min_quality <= 128, variant 0 / 4 / 5 / 6 / 7), 0 when
 * every read takes the general tile kernel (same results, about 1.5 x the time); negative on a bad ctx.  Informational: lets a
 * caller that sweeps sliding-window widths know when it has left the fast path (AmpliPy.py:563 takes any width). */
int amp_fast_path_active(amp_ctx *ctx);
/* The kernel variant the last batch of the ctx took (what 0 = "chosen per batch" resolved to: 4, 5 or 7; 2 for runs outside of the
 * fast kernels' parameters; 0 before the first batch); negative on a bad ctx.  Informational. */
int amp_last_kernel_variant(amp_ctx *ctx);
/* Size the fast kernel's grid for 1 / divisor of the GPU's CUs (1, the default: one block per CU).  For callers that keep
 * several batches in flight on different streams (one ctx each): two passes side by side on half the chip each finish
 * sooner than one after the other on all of it -- a block then works twice as long, so its start-up, its flush and the idle
 * end of its last round of tiles weigh half as much (bench.py: 0.224 -> 0.212 ms per 2 M-read step with divisor 2, eight
 * steps in flight).  A pass that runs alone should keep the default.  Results do not depend on it.
 * The two kernels behind a fast kernel (the general pass over the reads it hands over, the heavy pass over the reads that one
 * defers) are launched with as many blocks as the ctx's previous pass would have kept busy, times two, between 8 and their full
 * grids for the ctx's share of the CUs: in most batches of an amplicon run both find nothing to do, and every block of an idle
 * launch still waits for a CU that no fast-kernel block of another ctx holds.  A batch with far more such reads than the one
 * before runs correctly on the small grid (a block walks several list segments), only slower; the pass after it gets the large
 * one.  "Previous" is the last pass that had finished when the next one was launched (nothing waits for it: with passes in
 * flight the two block counts depend on the host's timing, the results never do).  The ctx's first pass, the first pass behind a
 * call of amp_set_params, amp_set_kernel_variant or amp_set_cu_share that changed a value, and the pass behind one that took no
 * fast kernel take the full grids. */
int amp_set_cu_share(amp_ctx *ctx, int divisor);

/* ---- calling: alleles_from_counts (AmpliPy.py:756-771) + the loop AmpliPy.py:917-952 --------
 * One device pass decides, for every reference position, everything that does not depend on
 * the TEXT of an insertion allele: total depth (all symbols, insertion events included,
 * :767), the six base symbols ranked like sorted(..., reverse=True) (:771), the consensus
 * symbol (:928-929) and the variant record (:933-951).  Frequencies are IEEE doubles
 * count/total compared with >=, exactly as Python computes them.
 * An insertion string can only change a decision when the position's insertion events could
 * out-rank the best base symbol or reach min_freq_variants; those positions come back with
 * AMP_CALL_INS_RELEVANT and the host finishes them from amp_get_ins_events (the strings live
 * in the reads: SEQ[q_from:q_to]).  full_ranking = 1 flags every position that has events. */
typedef struct amp_call_params {
    int32_t min_depth_consensus;
    int32_t min_depth_variants;
    double min_freq_consensus;
    double min_freq_variants;
    int32_t run_consensus;
    int32_t run_variants;
    int32_t full_ranking;
    int32_t reserved;
} amp_call_params;

#define AMP_CALL_VARIANT 1u      /* a VCF record is emitted (AmpliPy.py:940) */
#define AMP_CALL_GT_HAS_REF 2u   /* GT starts at 0 (AmpliPy.py:948-949) */
#define AMP_CALL_INS_RELEVANT 4u /* insertion alleles may change this position's outcome */

typedef struct amp_pos_call {
    uint32_t total_depth; /* :767; 32-bit: the counts of a position, insertion events included, must sum below 2^32 */
    uint32_t ref_count;   /* count of the reference symbol (:937); 0 when it is not one of A C G T N - */
    uint32_t order;       /* bits 3k..3k+2: column (A C G T N - = 0..5) of the k-th ranked base symbol;
                             bits 18..20: number of base symbols with a non-zero count */
    int8_t consensus_sym; /* -1 = unknown symbol, else column 0..5 of the consensus (:929) */
    uint8_t flags;        /* AMP_CALL_* */
    uint8_t alt_mask;     /* bit k: k-th ranked base symbol is an ALT (:938-939) */
    uint8_t pad;
} amp_pos_call;

/* One VCF record decided on the device (positions not flagged AMP_CALL_INS_RELEVANT). */
typedef struct amp_var_rec {
    int32_t pos;            /* 0-based; VCF POS = pos + 1 (AmpliPy.py:947) */
    uint32_t total_depth;   /* DP */
    uint32_t ref_count;     /* REF_DP */
    uint8_t n_alt;
    uint8_t gt_has_ref;     /* GT = 0/1/../n_alt when set, 1/../n_alt otherwise (AmpliPy.py:948-951) */
    uint8_t alt_col[6];     /* ALT symbols in ranked order: columns A C G T N - = 0..5 */
    uint32_t alt_count[6];  /* ALT_DP; ALT_FREQ = alt_count / total_depth as IEEE doubles */
} amp_var_rec;

/* ASCII reference sequence, length ref_len, exactly as read from the FASTA (REF is compared
 * un-upper-cased, AmpliPy.py:923). */
int amp_set_reference(amp_ctx *ctx, const uint8_t *ref_ascii);
int amp_call_positions(amp_ctx *ctx, const amp_call_params *params, amp_pos_call *out /* host [ref_len] */,
                       int64_t *n_relevant);
/* The same decisions packed for the host: consensus column per position (-1 unknown), the
 * variant records in ascending position, and the insertion-relevant positions (whose
 * consensus / record the host finishes).  Returns AMP_EOVERFLOW (with the needed counts) when
 * a capacity is too small; ref_len entries always suffice. */
int amp_call_compact(amp_ctx *ctx, const amp_call_params *params, int8_t *consensus /* [ref_len] */,
                     amp_var_rec *vars, int64_t vars_cap, int64_t *n_vars,
                     int32_t *relevant, int64_t relevant_cap, int64_t *n_relevant);
/* amp_call_compact without the last copy: the arrays stay in host memory owned by ctx (page-locked and written by the
 * kernel itself when the call was begun with amp_call_compact_begin, else an ordinary buffer filled by one copy) and are
 * valid until the next amp_call_* on the same ctx (or amp_ctx_destroy). */
typedef struct amp_call_view {
    const int8_t *consensus;       /* [ref_len] */
    const amp_var_rec *vars;       /* [n_vars] */
    const int32_t *relevant;       /* [n_relevant] */
    int64_t n_vars, n_relevant;
} amp_call_view;
int amp_call_compact_view(amp_ctx *ctx, const amp_call_params *params, amp_call_view *out);
/* Enqueue the work of amp_call_compact_view on the ctx stream without waiting (right behind amp_process_batch_device,
 * say): a following amp_call_compact_view with the same parameters only waits for it and hands the views out.  Lets a
 * caller with several contexts in flight keep the calling kernels of one step in front of the next step's reads.
 * begin must come BEHIND the last update of the table: amp_process_batch[_device], amp_reset, amp_add_counts, amp_reduce
 * and amp_ctx_bind_counts all cancel a begun call (the following view then computes afresh), so on several GPUs the order
 * is process, amp_reduce, begin, view.  From begin onward the memory behind the previous view is being overwritten. */
int amp_call_compact_begin(amp_ctx *ctx, const amp_call_params *params);
/* Text of insertion events from a DEVICE-resident batch: text[off[e] .. off[e+1]) receives
 * SEQ[q_from:q_to] of event e (off[e+1]-off[e] must equal q_to-q_from). ev/off/text are host.
 * reads == NULL: the batch of the last amp_process_batch call (its device copy stays in the ctx until the next one;
 * AMP_ESTATE when there was none) -- a caller that feeds host batches gets the allele text of a batch's events
 * without gathering the bases on the host (AmpliPy.py:736-738 builds each string from the read it is looking at).
 * An event's row is (read - read_base) modulo 2^32, as in amp_aggregate_ins_events: read ids are 32-bit and a batch's ids may
 * wrap.  AMP_EINVAL when that row is not one of the batch, or q_from / q_to / off do not fit together; q_to is NOT held against
 * the row's l_seq (that lives on the device): the caller passes events of this batch. */
int amp_event_strings(amp_ctx *ctx, const amp_dev_reads *reads, uint64_t read_base, int64_t n_events,
                      const amp_ins_event *events, const uint64_t *off, uint8_t *text);

/* ---- DEFLATE of BGZF blocks (the writer's opt-in device codec) ----------
 * n = ceil(n_bytes / block_bytes) consecutive chunks of block_bytes (1..0xFF00; the last may be shorter) of `in` become n
 * complete raw DEFLATE streams (RFC 1951, one final block each, dynamic Huffman codes or stored): chunk k's stream at
 * out + k * out_stride, its length in out_len[k].  Nothing is written beyond out + k * out_stride + out_room; a chunk
 * whose stream does not fit out_room -- not even as a stored block of chunk + 5 bytes -- gets out_len[k] = 0 and the caller
 * compresses it some other way.  Framing (gzip / BGZF header, CRC-32, ISIZE) is the caller's.
 * Needs no amp_ctx: the device's stream and staging buffers of this entry point belong to the library, are made on first
 * use and kept for the process.  Calls for one device are serialised inside; a call may run on any thread, also while
 * another thread is inside amp_process_batch (a stream of its own, no synchronisation of the device).
 * in / out / out_len are host memory; n_bytes == 0 is no chunk and AMP_OK. */
int amp_deflate_blocks(int device, const uint8_t *in, int64_t n_bytes, int32_t block_bytes,
                       uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len);
/* The same on device memory, enqueued on `stream` (a hipStream_t; NULL: the library's stream of that device) without waiting:
 * the kernel alone.  Any alignment of in, out and out_stride works. */
int amp_deflate_blocks_device(int device, const uint8_t *in, int64_t n_bytes, int32_t block_bytes,
                              uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len, void *stream);
/* Waits for the library's DEFLATE stream of `device` (what a NULL stream above runs on). */
/* The same when only the device knows the byte count: the kernel reads it from *d_n_bytes (device memory, written by earlier work
 * on `stream`); max_bytes = the most it can be, which sizes the launch.  out_len[k] is written for the chunks of *d_n_bytes only. */
int amp_deflate_blocks_device_counted(int device, const uint8_t *in, const uint64_t *d_n_bytes, int64_t max_bytes, int32_t block_bytes,
                                      uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len, void *stream);
int amp_deflate_sync(int device);
/* Signature of ampbam_writer_set_deflater (include/ampbam.h): `user` points to an int32_t holding the device. */
int amp_deflate_blocks_cb(void *user, const uint8_t *in, int64_t n_bytes, int32_t block_bytes,
                          uint8_t *out, int64_t out_stride, int32_t out_room, uint32_t *out_len);

/* ---- SAM text on the device (opt-in codec of the command line: AMPLIPY_GPU_SAM=1) ----------------------
 * The reference reads SAM text through pysam in front of its per-read loop and writes it with out_aln.write (AmpliPy.py:296-360,
 * :896-915); the host mirror does that per line in Python (bamio.AlignmentReader._iter_sam, AlignmentWriter.write).  An amp_sam
 * does it for chunks of whole lines on the device of its ctx: the text goes up once, a packed batch (amp_dev_reads) is built
 * from it in HBM, amp_process_batch_device runs on that batch, and the kept lines of a trimmed output come back as text: the
 * input line with POS and CIGAR replaced.  An amp_sam owns device text, line and field tables, the batch, its results and
 * the output text; the buffers grow to the largest chunk and are reused -- nothing is freed while chunks of one size go
 * through.  Not thread-safe; all work runs on the ctx stream.
 *
 * A line is ODD when the Python codec might not give it back byte for byte, or would raise on it; a chunk with an odd line
 * is not processed here at all (amp_sam_process refuses it): the caller hands that chunk's text to the Python codec, so
 * whatever that does with the line still happens.  Reasons, in the order a line is tested: */
#define AMP_SAM_ODD_NONE 0
#define AMP_SAM_ODD_BYTE 1         /* a byte >= 0x80, a NUL, a '\r' that is not the single byte in front of a '\n' (any line) */
#define AMP_SAM_ODD_INT 2          /* FLAG POS MAPQ PNEXT TLEN not -?(0|[1-9][0-9]*), or "-0" */
#define AMP_SAM_ODD_RANGE 3        /* ... outside FLAG 0..65535, POS / PNEXT 0..2^31-1, MAPQ 0..255, TLEN int32 */
#define AMP_SAM_ODD_RNAME 4        /* RNAME neither '*' nor an @SQ name */
#define AMP_SAM_ODD_RNEXT 5        /* RNEXT not '*', '=' behind a named RNAME, or an @SQ name other than RNAME */
#define AMP_SAM_ODD_CIGAR 6        /* CIGAR neither '*' nor (\d+[MIDNSHP=XB])+ : parse_cigar raises ValueError */
#define AMP_SAM_ODD_CIGAR_LEN 7    /* an op length of 2^28 or more, or one written with leading zeros */
#define AMP_SAM_ODD_EMPTY 8        /* SEQ or QUAL empty */
#define AMP_SAM_ODD_QUAL_NO_SEQ 9  /* QUAL given, SEQ '*' */
#define AMP_SAM_ODD_QUAL_LEN 10    /* QUAL given, its length is not SEQ's */
#define AMP_SAM_ODD_QUAL_CHAR 11   /* a QUAL character below '!' */
#define AMP_SAM_ODD_LINES 12       /* more lines than the line tables hold (n_bytes / 64 + 1024): not SAM records */
/* ... and, with BAM output only (amp_sam_set_output), what aux_sam_to_bam / struct.pack would not turn into the
 * bytes the device makes; of several such faults on one line the smallest number is reported: */
#define AMP_SAM_ODD_QNAME 13       /* QNAME longer than 254 bytes (l_read_name is one byte) */
#define AMP_SAM_ODD_AUX_TAG 14     /* an aux field that is not ^[!-~]{2}:[AifZHB]: */
#define AMP_SAM_ODD_AUX_A 15       /* A whose value is not exactly one byte */
#define AMP_SAM_ODD_AUX_INT 16     /* i that is not -?(0|[1-9][0-9]*) */
#define AMP_SAM_ODD_AUX_INT_RANGE 17  /* i outside [-2^31, 2^32 - 1] */
#define AMP_SAM_ODD_AUX_B 18       /* B that is not [cCsSiIf](,value)* */
#define AMP_SAM_ODD_AUX_B_RANGE 19 /* an element of B outside its subtype's range */
#define AMP_SAM_ODD_AUX_FLOAT 20   /* f, or an element of B:f, not -?digits[.digits][e[+-]digits] with at most 15 significant digits
                                    * and a power of ten (the fraction folded in) within +-22 */
#define AMP_SAM_ODD_CIGAR_OPS 21   /* more than 65,532 CIGAR ops: the trimmed CIGAR (three more at most) might not fit n_cigar_op */
#define AMP_SAM_MAX_REFS 64        /* @SQ names the device table holds; a header with more keeps the run on the Python codec */
#define AMP_SAM_MAX_REF_BYTES 4096 /* ... and their bytes */
#define AMP_SAM_N_STAGES 15
#define AMP_SAM_OUT_TEXT 0
#define AMP_SAM_OUT_BAM 1

typedef struct amp_sam amp_sam;
typedef struct amp_sam_info {
    int64_t n_lines;         /* '\n' of the chunk */
    int64_t n_records;       /* lines of 11 fields and more (what _iter_sam yields; fewer fields: skipped, not counted) */
    int64_t n_rows;          /* records the loop does not skip (A:902): mapped, CIGAR not '*' */
    int64_t n_cig, n_bases, n_bases_padded;     /* of the rows */
    int64_t first_odd_line;  /* -1: none.  With an odd line the counts from n_rows on leave out the odd lines and mean nothing */
    int32_t odd_reason, reserved;
} amp_sam_info;
int amp_sam_create(amp_ctx *ctx, amp_sam **out);
void amp_sam_destroy(amp_sam *s);
/* header.refs of bamio.AlignmentReader: the @SQ SN names in header order, once per run and before the first parse. */
int amp_sam_set_references(amp_sam *s, int32_t n_ref, const char *const *names);
/* bamio._iter_sam + ReadBatch.from_segments (pysam's parsing in front of A:896, the skip of A:902) for n_bytes < 1 GiB of host
 * text that ends with '\n' (AMP_EINVAL otherwise; n_bytes 0: no line, AMP_OK).  Waits for the device once, for the sizes. */
int amp_sam_parse(amp_sam *s, const uint8_t *text, int64_t n_bytes, amp_sam_info *info);
/* The batch of the last parse: device pointers, valid until the next parse. */
int amp_sam_reads(amp_sam *s, amp_dev_reads *out);
/* The same batch copied into the host arrays dst points to (dst->n_reads must be n_rows; 64-bit offsets as in amp_reads) and
 * the number of each row's record among the chunk's records (ReadBatch.src_index): tests and tools. */
int amp_sam_batch_to_host(amp_sam *s, const amp_reads *dst, int64_t *src_index);
/* A:896-915 for the chunk: amp_process_batch_device on the batch, the result arrays owned by s.  *first_bad_row = the first
 * row whose status is not AMP_RS_OK and *its_status that status; -1 and 0 when there is none.  AMP_ESTATE for an odd chunk.
 * With both pointers NULL the call is DEFERRED: the pass is enqueued, nothing is waited for, and the verdict stays on the device
 * until amp_sam_encode brings it down with its own wait (or amp_sam_first_bad / amp_sam_format with one of theirs). */
int amp_sam_process(amp_sam *s, uint64_t read_base, int64_t *first_bad_row, uint8_t *its_status);
/* The verdict of the last amp_sam_process, deferred or not. */
int amp_sam_first_bad(amp_sam *s, int64_t *first_bad_row, uint8_t *its_status);
/* Waits for the device since the amp_sam was made (a parse costs one, a process that is not deferred one, a format two, an encode
 * one): tests and tools. */
int64_t amp_sam_waits(amp_sam *s);
/* AlignmentWriter.write(r, pos=, cigar=) (out_aln.write, A:911) for every row in front of the first failing one that passes
 * ref_len >= min_length and (trimmed at a primer or include_no_primer) (A:910): the input line with field 4 = new_pos + 1,
 * field 6 = the new CIGAR, a '\r' before the '\n' dropped.  AMP_EOVERFLOW with *n_bytes = the size needed when cap is
 * short; AMP_EINVAL before amp_sam_process. */
int amp_sam_format(amp_sam *s, int32_t min_length, int32_t include_no_primer, uint8_t *out, int64_t cap, int64_t *n_bytes,
                   int64_t *n_rows_written);
/* Development aid: ms[AMP_SAM_N_STAGES] of the last chunk from HIP events on the ctx stream -- [0] copy up, [1] scan and
 * ranks, [2] lines and tabs, [3] records and rows (with BAM output: aux sizes too), [4] pack, [6] the read pass, [8] format kernels,
 * [9] copy down, [11] BAM records, [12] their DEFLATE, [13] CRC and framing, [14] copy down ([5], [7], [10]: host time between the
 * calls; a stage that did not run reads -1).  on != 0 records the events from the next call on. */
int amp_sam_stage_ms(amp_sam *s, int on, float *ms);

/* ---- BAM input on the device (opt-in codec of the command line: AMPLIPY_GPU_BAM=1) ---------------------
 * The reference reads BAM through pysam (AmpliPy.py:296-324, :896) and skips unmapped reads and reads without a CIGAR (A:902);
 * the host codec does it in libampbam: ampbam_open_range_at (BGZF inflate, CRC-32 of every block, record index) and
 * ampbam_decode (the packed batch), after which the decoded batch is copied to the device.  An amp_bam takes the COMPRESSED
 * bytes of a piece of the file -- whole BGZF blocks, with the block table libampbam reads from their headers and trailers
 * (ampbam_block_table) -- and does the rest on the device of its ctx: every block's raw DEFLATE stream is inflated into the
 * piece's image [carry | inflated blocks] (carry: the bytes of the last image behind its last complete record), every block's
 * CRC-32 is compared with its trailer, the records are indexed from the KNOWN start of the first one, and the rows are
 * decoded into an amp_dev_reads on which amp_process_batch_device runs where it lies.  The buffers belong to the amp_bam, grow
 * to the largest piece and are not freed during a run.  Not thread-safe; all work runs on the ctx stream.
 *
 * A block the device refuses -- its stream breaks a rule of RFC 1951, does not end after exactly ISIZE bytes, or its CRC
 * differs -- writes nothing outside its own range of the image and is handed back: the caller inflates it on the host
 * (ampbam_inflate_raw / zlib, CRC checked), patches the bytes in and asks for the index again.  On a valid file no block is. */
#define AMP_BAM_IMAGE_LIMIT (256ll << 20) /* bytes of an image: carry + the ISIZE sum of a piece.  A record is at most 2^27 + 4 bytes
                                           * (a longer block_size is a format error), so pieces of up to 120 MiB inflated always fit */
#define AMP_BAM_N_STAGES 16
typedef struct amp_bam amp_bam;
typedef struct amp_bam_block {   /* one BGZF block of a piece */
    uint32_t in_off, in_len;     /* its raw DEFLATE stream in the piece's compressed bytes */
    uint32_t out_len, crc;       /* ISIZE and CRC-32 of its trailer */
} amp_bam_block;
typedef struct amp_bam_info {
    int64_t n_blocks, n_inflated;     /* of this piece: blocks, their ISIZE sum */
    int64_t image_bytes, carry_in;    /* the image [carry | inflated]; bytes carried in from the piece before */
    int64_t carry_out;                /* bytes behind the last complete record: they open the next image */
    int64_t next_first;               /* > 0: the first record starts that many bytes behind this image (a header longer than a piece) */
    int64_t n_records;                /* records that END in this image */
    int64_t n_rows;                   /* ... that the loop does not skip (A:902) */
    int64_t n_cig, n_bases, n_bases_padded;     /* of the rows */
    int64_t n_refused;                /* blocks handed back; the counts above are 0 until they are patched and re-indexed */
    int64_t index_rounds;             /* link / jump / settle rounds the index took (1: every guessed record start was right) */
    int64_t waits;                    /* waits for the device this piece cost (1 on the ordinary path) */
    int64_t bytes_up;                 /* host-to-device bytes of the piece: compressed bytes + block table */
    int32_t bad_record, reserved;     /* a record with block_size < 32 or > 2^27, or a body longer than block_size: the `bad` of index_records */
} amp_bam_info;
int amp_bam_create(amp_ctx *ctx, amp_bam **out);
void amp_bam_destroy(amp_bam *s);
/* ampbam_open_range_at + ampbam_decode for a piece.  first_off >= 0: the first record starts at that offset of the inflated
 * blocks and nothing is carried in (the file's first piece: the header's end); < 0: the image starts with the carry, whose first
 * byte is a record's.  rec_base = records in front of this piece (src_index counts from it); n_ref = references of the header
 * (the plausibility test of guessed record starts).  AMP_EOVERFLOW when the image would pass AMP_BAM_IMAGE_LIMIT. */
int amp_bam_feed(amp_bam *s, const uint8_t *comp, int64_t n_comp, const amp_bam_block *blocks, int64_t n_blocks, int64_t first_off,
                 int32_t n_ref, int64_t rec_base, amp_bam_info *info);
/* Development aid: the next feed hands block k of its piece back although it inflates (the test of the host fallback). */
int amp_bam_dev_refuse(amp_bam *s, int64_t k);
/* The blocks the last feed handed back (piece-relative numbers), the host's bytes for one of them, and the index and decode
 * again once all of them are patched. */
int amp_bam_refused(amp_bam *s, int64_t *idx, int64_t cap, int64_t *n);
/* Why: one byte per block of the last feed as the kernels left it (cap >= n_blocks) -- 0 accepted, 1 refused by the decoder,
 * 2 by the CRC check.  Tests and tools. */
int amp_bam_verdicts(amp_bam *s, uint8_t *verdict, int64_t cap);
int amp_bam_patch_block(amp_bam *s, int64_t k, const uint8_t *bytes, int64_t n_bytes);
int amp_bam_reindex(amp_bam *s, amp_bam_info *info);
/* The batch of the last feed (ampbam_decode's rows): device pointers, valid until the next feed. */
int amp_bam_reads(amp_bam *s, amp_dev_reads *out);
/* The same batch copied to host arrays (dst->n_reads must be n_rows; cig, seq and qual with their 16 bytes of slack) and each
 * row's record number: tests and tools. */
int amp_bam_batch_to_host(amp_bam *s, const amp_reads *dst, int64_t *src_index);
/* The image of the last feed and the offsets of its records in it (either may be NULL): tests and tools.  Both stay on the
 * device until the next feed -- what amp_bam_encode copies the unchanged parts of trimmed records from. */
int amp_bam_image_to_host(amp_bam *s, uint8_t *image, int64_t image_cap, uint32_t *rec_off, int64_t rec_cap);
/* A:896-915 for the piece: amp_process_batch_device on the batch, the result arrays owned by s (as amp_sam_process). */
int amp_bam_process(amp_bam *s, uint64_t read_base, int64_t *first_bad_row, uint8_t *its_status);
/* Development aid: ms[AMP_BAM_N_STAGES] of the last piece from HIP events on the ctx stream -- [0] copy up, [1] inflate, [2] CRC,
 * [3] record index, [4] decode, [6] the read pass, [8] re-encode of trimmed records, [9] their DEFLATE, [10] CRC and framing,
 * [11] copy down ([5], [7]: the waits and host time between the calls); with trimmed reads as SAM text (section 14) [12] the
 * text check, [14] sizes and lines, [15] the text's copy down ([13]: the read pass and host time between check and format).
 * on != 0 records from the next call on. */
int amp_bam_stage_ms(amp_bam *s, int on, float *ms);

/* ---- trimmed BAM out of an amp_bam (opt-in: AMPLIPY_GPU_BAM_WRITE=1 with AMPLIPY_GPU_BAM=1) -------------
 * The host codec writes trimmed reads with ampbam_write_rows (out_aln.write, AmpliPy.py:911), which copies the unchanged parts of
 * a record from the piece's HOST image, and compresses 0xFF00-byte chunks of the record stream into BGZF blocks.  amp_bam_encode
 * does both on the device, behind amp_bam_process, from the image, record offsets, batch and results the amp_bam holds: the
 * kept rows of the last feed (A:910: ref_len >= min_length and (trimmed at a primer or include_no_primer), rows in front of the
 * first failing one) are re-encoded -- the same bytes as ampbam_write_rows -- behind the bytes the call before left over, the
 * whole 0xFF00-byte chunks of that stream are compressed (amp_deflate_blocks_device_counted), given CRC-32 and BGZF framing and
 * gathered back to back; what is left (< 0xFF00 bytes) opens the next call's stream, so the blocks do not depend on how the
 * file was cut into pieces.  final != 0 compresses the last partial chunk too.  A call without a fresh feed behind it (the rows
 * of a feed are encoded once), or after a feed without rows, appends nothing: with final it is the bare flush.
 * One wait per call.  AMP_EINVAL when a kept row's new CIGAR has more than 65,535 ops (ampbam_write_rows refuses the batch):
 * nothing was appended.  AMP_ESTATE when the last feed has rows and amp_bam_process has not run on them.  The header's blocks
 * and the end-of-file block stay the host codec's (ampbam_writer_open_refs / ampbam_writer_append_framed / ampbam_writer_close). */
typedef struct amp_bam_out_info {
    int64_t n_rows_written;    /* rows re-encoded by this call */
    int64_t stream_bytes;      /* the call's uncompressed stream [carry_in | new records] */
    int64_t carry_in, carry_out;   /* bytes taken over from the call before / left to the next one */
    int64_t n_blocks;          /* BGZF blocks of this call */
    int64_t file_bytes;        /* ... their bytes in the file: what amp_bam_encoded_to_host copies */
    int64_t n_blocks_host;     /* blocks whose DEFLATE stream did not fit a BGZF block: not among file_bytes, the caller compresses them */
    int64_t waits;             /* waits for the device this call cost (1) */
    int64_t bytes_down;        /* device-to-host bytes: the counters and file_bytes */
} amp_bam_out_info;
int amp_bam_encode(amp_bam *s, int32_t min_length, int32_t include_no_primer, int32_t final, amp_bam_out_info *info);
/* The framed blocks of the last encode back to back, file_bytes of them, to host memory. */
int amp_bam_encoded_to_host(amp_bam *s, uint8_t *dst, int64_t cap);
/* The size in the file of every block of the last encode (n_blocks values); 0 for a block handed to the host, whose chunk is
 * bytes [k * 0xFF00, ...) of the stream. */
int amp_bam_encoded_blocks(amp_bam *s, uint32_t *blk_len, int64_t cap);
/* n bytes from offset `from` of the uncompressed stream of the last encode: tests, and the chunks of blocks handed to the host. */
int amp_bam_stream_to_host(amp_bam *s, int64_t from, int64_t n, uint8_t *dst);

/* ---- SAM text in, trimmed BAM out (opt-in: AMPLIPY_GPU_SAM=1 with AMPLIPY_GPU_BAM_WRITE=1) ---------------
 * The Python codec writes a trimmed read with AlignmentWriter(mode="wb").write(r, pos=, cigar=): the record packed with struct,
 * aux fields through aux_sam_to_bam, 0xFF00-byte chunks of the record stream compressed by BgzfWriter.  With BAM output an
 * amp_sam makes the same record bytes in HBM from the line's text, the resident batch and the results of amp_sam_process, and
 * hands the stream to the tail amp_bam_encode uses (carry, DEFLATE, CRC-32, framing, gather): amp_bam_out_info and the three
 * copies below mean what they mean there.  More lines are odd with BAM output (AMP_SAM_ODD_QNAME and following): the device never
 * emits what the Python codec would not.  The caller sends the records of such a chunk, made by the Python codec, through
 * amp_sam_encode_bytes, so the stream and its block boundaries do not depend on which side encoded a chunk. */
/* AMP_SAM_OUT_TEXT (the default) or AMP_SAM_OUT_BAM; once per run, before the first parse. */
int amp_sam_set_output(amp_sam *s, int32_t mode);
/* The kept rows of the last parse (A:910, rows in front of the first failing one) behind the bytes the call before left over; a
 * call without a fresh, processed, non-odd chunk behind it appends nothing (with final: the bare flush).  One wait per call, which
 * also brings the verdict of a deferred amp_sam_process down: a chunk then costs two waits, the parse's and this one.
 * AMP_ESTATE without BAM output, or when the chunk has rows and amp_sam_process has not run. */
int amp_sam_encode(amp_sam *s, int32_t min_length, int32_t include_no_primer, int32_t final, amp_bam_out_info *info);
/* n < 2^31 bytes of BAM records made on the host appended in the same way (n_rows_written stays 0).  One wait per call. */
int amp_sam_encode_bytes(amp_sam *s, const uint8_t *bytes, int64_t n, int32_t final, amp_bam_out_info *info);
int amp_sam_encoded_to_host(amp_sam *s, uint8_t *dst, int64_t cap);
int amp_sam_encoded_blocks(amp_sam *s, uint32_t *blk_len, int64_t cap);
int amp_sam_stream_to_host(amp_sam *s, int64_t from, int64_t n, uint8_t *dst);

/* ---- BAM in, trimmed SAM text out (opt-in: AMPLIPY_GPU_BAM=1 with AMPLIPY_GPU_SAM=1) ----------------------
 * The Python codec writes a trimmed read of a BAM input with AlignmentWriter(mode="w").write(r, pos=, cigar=) (out_aln.write,
 * AmpliPy.py:911): QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and the aux fields through aux_bam_to_sam, joined by
 * tabs.  An amp_bam makes the same line in HBM from the record where it lies in the piece's image, the new POS and CIGAR from the
 * results of amp_bam_process.  A row is ODD when the Python codec would raise on its record or might not write exactly the
 * device's bytes; a piece with an odd row is not formatted here at all (amp_bam_format refuses it): the caller brings the image
 * down (amp_bam_image_to_host) and hands its records to the Python codec, so whatever that does with the row still happens.
 * Records that are no rows (A:902) are never written and never checked.  Of several faults of one row the smallest number is
 * reported; the rule is stricter than needed in places, which costs a fallback, never a difference: */
#define AMP_BAM_ODD_NONE 0
#define AMP_BAM_ODD_QNAME 1        /* a QNAME byte outside '!'..'~', or l_read_name 0 */
#define AMP_BAM_ODD_REF 2          /* ref_id or next_ref_id not below the number of names (IndexError) */
#define AMP_BAM_ODD_CIGAR_OP 3     /* an op code above 9 in the record's CIGAR */
#define AMP_BAM_ODD_QUAL 4         /* a quality above 93 in a QUAL that does not start with 0xFF */
#define AMP_BAM_ODD_AUX_TYPE 5     /* an aux type that is none of A c C s S i I f Z H B, or a B subtype that is none of c C s S i I f */
#define AMP_BAM_ODD_AUX_TRUNC 6    /* a value, a B array, or a Z / H without its NUL reaching behind the record; 1-2 bytes left over */
#define AMP_BAM_ODD_AUX_CHAR 7     /* a tag or A byte outside '!'..'~', a Z / H byte outside ' '..'~' */
#define AMP_BAM_ODD_AUX_FLOAT 8    /* f, or an element of B:f, that is neither +-0 nor finite with 1e-4 <= |v| < 2^63 */
typedef struct amp_bam_text_info {
    int64_t first_odd_row;   /* -1: none (of the last check) */
    int32_t odd_reason, reserved;
    int64_t n_rows_written;  /* lines of this format */
    int64_t n_bytes;         /* ... and their bytes (with AMP_EOVERFLOW: the size needed) */
    int64_t waits;           /* waits for the device this call cost */
    int64_t bytes_down;      /* device-to-host bytes: the counters, and the text */
} amp_bam_text_info;
/* header.refs of the writer: the names RNAME / RNEXT are written from, at most AMP_SAM_MAX_REFS of AMP_SAM_MAX_REF_BYTES bytes
 * together.  Once per run, before the first check. */
int amp_bam_set_references(amp_bam *s, int32_t n_ref, const char *const *names);
/* The verdict on the rows of the last feed, whose index stands (no refused block left, no bad record), and the sizes of their
 * lines.  One wait (none for a piece without rows).  AMP_ESTATE without such a feed or before amp_bam_set_references. */
int amp_bam_text_check(amp_bam *s, amp_bam_text_info *info);
/* AlignmentWriter.write(r, pos=, cigar=) for every row in front of the first failing one that passes A:910 (as amp_bam_encode
 * and amp_sam_format choose them), n_bytes of text to `out`.  AMP_EOVERFLOW with n_bytes = the size needed when cap is short
 * (or the text would pass 2^32 bytes); AMP_ESTATE before amp_bam_process, or on a piece whose check found an odd row or never
 * ran.  Two waits at most: the sizes, then the copy.  The text buffer belongs to the amp_bam and grows to the largest piece. */
int amp_bam_format(amp_bam *s, int32_t min_length, int32_t include_no_primer, uint8_t *out, int64_t cap, amp_bam_text_info *info);

/* ---- amplicon QC report (opt-in) ---------------------------------------------------------------------------
 * What a run of an amplicon panel is looked at for first, from the data that is in HBM when the read pass ends: how many reads
 * each primer took, how many reads were kept or dropped, how deep each region is covered.  The reference has no such report; its
 * numbers are defined from the reference's own rules.  A read's start trim is looked up at its ORIGINAL reference_start and its
 * end trim at its original reference_end - 1 (AmpliPy.py:450-451): the primer a trim is counted for is the OWNER of that position,
 * the primer that gave the table entry trim_read read there.  A read is kept, dropped as too short or dropped for lack of a primer
 * by the write filter (AmpliPy.py:910).  With the report on, one more kernel runs behind the read pass of every amp_process_batch*
 * on the ctx stream; nothing per read leaves the device.  With it off (the default) nothing changes. */
#define AMP_QC_MAX_DEPTHS 4
typedef struct amp_qc_params {
    int32_t n_primers;               /* 0 is legal: a run without trimming has no BED */
    const int32_t *starts, *ends;    /* host; sorted ascending by (start, end) like amp_find_overlapping_primers */
    int32_t primer_pos_offset;
    int32_t min_length, include_no_primer;   /* the write filter, AmpliPy.py:910 */
    int32_t n_regions;
    const int32_t *region_start, *region_end;   /* host; half-open, clamped to [0, ref_len) by the library; region 0 is the caller's to supply */
    int32_t n_depths;                /* 0..AMP_QC_MAX_DEPTHS */
    uint32_t depths[AMP_QC_MAX_DEPTHS];
} amp_qc_params;
/* 64-bit tallies over all batches since amp_reset.  A row with a non-zero status adds to rows and errors only.  Without do_trim only
 * rows, errors and ref_bases_in are filled.  With it: the three AMP_TRIM_* bits (AmpliPy.py:687), both / neither primer bit, and
 * exactly one of kept / dropped_short / dropped_no_primer (AmpliPy.py:910), so kept + dropped_short + dropped_no_primer = rows - errors.
 * ref_bases_in: reference length of the original CIGAR (ops M D N = X); ref_bases_out: reference_length after trimming. */
typedef struct amp_qc_reads {
    uint64_t rows, errors, primer_start, primer_end, primer_both, primer_none, quality,
        kept, dropped_short, dropped_no_primer, ref_bases_in, ref_bases_out;
} amp_qc_reads;
/* depth = A + C + G + T + N + '-' of the count table (the insertion tally is not part of it; the sum must stay below 2^32 like
 * amp_pos_call.total_depth).  covered[k] = positions of the region with depth >= depths[k].  An empty region has end = start and zeros. */
typedef struct amp_qc_region {
    int32_t start, end; /* clamped */
    uint64_t depth_sum;
    uint32_t depth_min, depth_max;
    uint32_t covered[AMP_QC_MAX_DEPTHS];
} amp_qc_region;
/* The owners of every reference position (host, no ctx, no GPU).  Primer i covers p when starts[i] - offset <= p < ends[i] + offset
 * (the window of find_overlapping_primers, AmpliPy.py:174-209).  left_owner[p]: the covering primer with the largest end -- the one
 * max_primer_end[p] comes from, read at AmpliPy.py:450; right_owner[p]: the one with the smallest start (min_primer_start[p],
 * AmpliPy.py:451).  Ties go to the smallest index; -1 where no primer covers p. */
int amp_qc_find_primer_owners(int32_t ref_len, int32_t n, const int32_t *starts, const int32_t *ends, int32_t offset,
                              int32_t *left_owner, int32_t *right_owner);
/* p == NULL: off (the default; the tallies read so far stay readable).  Otherwise on, with tallies of zero: copies everything it is
 * given.  AMP_ESTATE when the ctx trims (amp_set_params) and has no primer tables (amp_set_primers).  With the report on and do_trim
 * set, amp_process_batch_device refuses a dev_out without new_pos, ref_len, trim_flags or status (AMP_EINVAL) before anything runs. */
int amp_qc_enable(amp_ctx *ctx, const amp_qc_params *p);
/* The tallies since amp_reset (waits for the stream).  primer_reads_start[i] / primer_reads_end[i]: reads whose start / end trim
 * (AmpliPy.py:450-451) primer i owns; [n_primers] each, either may be NULL. */
int amp_qc_read_tallies(amp_ctx *ctx, amp_qc_reads *out, uint64_t *primer_reads_start, uint64_t *primer_reads_end);
/* Depth per position and the figures of the regions given to amp_qc_enable, from the table as it stands (several ranks: after
 * amp_reduce / the all-reduce).  Host pointers. */
int amp_qc_depth(amp_ctx *ctx, uint32_t *depth /* [ref_len] or NULL */, amp_qc_region *regions /* [n_regions] or NULL */);
/* Time of the report's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_qc_last_ms(amp_ctx *ctx, float *reads_ms);

/* ---- QC report: soft-clip sites (opt-in sub-switch of the report) --------------------------------------------
 * A large deletion leaves no gap in an alignment: the aligner aligns one side and soft-clips the rest.  With the sub-switch on, a
 * second kernel behind the report's tallies, per reference position and side, the reads that are clipped there and their first
 * AMP_CLIP_K clipped bases, from every row with status 0 as it CAME IN (original pos, CIGAR, l_seq, FLAG, SEQ; no quality test):
 *   L_left / L_right: the S ops summed from the front (leading H ops skipped) up to the first other op / from the back down to
 *   element 1.  A read is skipped -- it adds to `skipped` and to nothing else -- when l_seq <= 0, when it has no op other than H and S,
 *   when L_left + L_right > l_seq, when pos < 0 or when pos + the CIGAR's reference length > ref_len.  Every other read is scanned.
 *   L_left >= clip_min: a LEFT site at p = pos, its clipped base at offset j the query base L_left - 1 - j (nearest the junction first);
 *   L_right >= clip_min: a RIGHT site at p = pos + the reference length, in [0, ref_len], offset j the query base l_seq - L_right + j.
 *   Per site: reads += 1, rev += 1 with FLAG 0x10, comp[j][col] += 1 for j < min(L, AMP_CLIP_K); col 0..3 for the BAM codes 1 2 4 8
 *   (A C G T), 4 for anything else.
 * table: uint32 [(ref_len + 1)][2][AMP_CLIP_CELLS], position-major, side 0 = left; a site's cells are reads, rev, comp[j][c].
 * scalars: scanned, skipped, left, right -- reads that were scanned / skipped / have a site of that side. */
#define AMP_CLIP_K 16
#define AMP_CLIP_COLS 5
#define AMP_CLIP_CELLS (2 + AMP_CLIP_K * AMP_CLIP_COLS)
#define AMP_CLIP_SCALARS 4
/* clip_min 1..64: on, the table zero; 0: off (a table read so far stays readable); anything else AMP_EINVAL.  AMP_ESTATE unless a QC
 * report exists; amp_qc_enable builds a new report, so this has to be called again after every amp_qc_enable. */
int amp_qc_clips_enable(amp_ctx *ctx, int32_t clip_min);
/* Host copies as they stand (waits for the stream); either pointer may be NULL.  AMP_ESTATE unless the clip sites were enabled
 * since the last amp_qc_enable. */
int amp_qc_clips_get(amp_ctx *ctx, uint32_t *table, uint64_t scalars[AMP_CLIP_SCALARS]);
/* Host table and scalars added element-wise onto the device's (the merge of partial tables); either pointer may be NULL. */
int amp_qc_clips_add(amp_ctx *ctx, const uint32_t *table, const uint64_t *scalars);
/* Time of the clip kernel behind the last batch; AMP_ESTATE when none ran.  amp_qc_last_ms stays the report's first kernel. */
int amp_qc_clips_last_ms(amp_ctx *ctx, float *ms);

/* ---- per-allele strand and base-quality tallies (opt-in) ----------------------------------------------------
 * The evidence behind a call that the count table forgets.  For every read with status 0, each increment update_base_counts
 * (AmpliPy.py:690-753) makes to one of the six fixed keys A C G T N '-' of position r (columns 0..5 as in the count table) also adds
 *   rev[r][c] += 1                       when the read's FLAG has 0x10      (uint32[ref_len][6]; forward support is counts - rev)
 *   qsum[r][c] += query_qual[q_pos]      for the five base columns          (uint64[ref_len][5]; a deleted position has no quality)
 * Insertion alleles are not part of the tables.  With do_trim the alignment walked is the trimmed one, without it the read as it came
 * in.  A batch with a read of non-zero status leaves the tables as unspecified as it leaves the count table.  With the tallies on,
 * one more kernel runs behind the read pass of every amp_process_batch* on the ctx stream; with them off (the default) nothing
 * changes.  amp_reset zeroes the tables. */
/* on != 0: the tallies on, the tables (64 bytes per reference position, allocated at the first call) zero.  on == 0: off; the tables
 * stay readable.  With the tallies on and do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig, new_cig
 * or status (AMP_EINVAL) before anything runs. */
int amp_strand_enable(amp_ctx *ctx, int on);
/* Host copies of the tables as they stand (waits for the stream); either pointer may be NULL.  AMP_ESTATE before the first enable. */
int amp_strand_get(amp_ctx *ctx, uint32_t *rev /* [ref_len][6] */, uint64_t *qsum /* [ref_len][5] */);
/* Host tables added element-wise, like amp_add_counts (the merge of partial tables); either pointer may be NULL. */
int amp_strand_add(amp_ctx *ctx, const uint32_t *rev, const uint64_t *qsum);
/* Time of the tallies' kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_strand_last_ms(amp_ctx *ctx, float *ms);

/* ---- per-amplicon allele counts (opt-in) ---------------------------------------------------------------------
 * Which amplicon the evidence at a position comes from.  An amplicon a has a span [lo[a], hi[a]) of the reference; amp_start[p] /
 * amp_end[p] (int32[ref_len], -1: none) name the amplicon whose left / right primer owns position p.  A read with status 0 that came
 * in at [p, e) -- ORIGINAL coordinates, e = p + the reference bases of the original CIGAR -- belongs to the first of amp_start[p]
 * (0 <= p < ref_len), amp_end[e - 1] (0 < e <= ref_len) whose span contains [p, e), else to none.  For every increment
 * update_base_counts (AmpliPy.py:690-753) makes to one of the six fixed keys A C G T N '-' at position r for a read of amplicon a,
 *   counts[cell_off[a] + r - lo[a]][c] += 1      (uint32[sum of hi - lo][6], cell_off[a] = sum of hi[b] - lo[b] over b < a)
 *   reads[a] += 1 per read of a, reads[n_amp] += 1 per read with status 0 that belongs to none      (uint64[n_amp + 1])
 * Insertion alleles are not part of the tables. */
/* The hook on for the n_amp amplicons given (the arrays are copied; 0 <= lo < hi <= ref_len, owner entries in [-1, n_amp), the spans
 * at most 2^22 positions together: AMP_EINVAL otherwise), the tables (allocated at the first call, again when the set's size changes)
 * zero.  n_amp == 0 or a NULL array: off; the tables stay readable.  With the hook on and do_trim set, amp_process_batch_device
 * refuses a dev_out without new_pos, new_ncig, new_cig or status (AMP_EINVAL) before anything runs. */
int amp_amplicon_enable(amp_ctx *ctx, int32_t n_amp, const int32_t *lo, const int32_t *hi, const int32_t *amp_start, const int32_t *amp_end);
/* Host copies of the tables as they stand (waits for the stream); either pointer may be NULL.  AMP_ESTATE before the first enable. */
int amp_amplicon_get(amp_ctx *ctx, uint32_t *counts /* [sum span][6] */, uint64_t *reads /* [n_amp + 1] */);
/* Host tables added element-wise, like amp_add_counts (the merge of partial tables); either pointer may be NULL. */
int amp_amplicon_add(amp_ctx *ctx, const uint32_t *counts, const uint64_t *reads);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_amplicon_last_ms(amp_ctx *ctx, float *ms);

/* ---- codon tallies within single reads (opt-in) --------------------------------------------------------------
 * Which bases stand together on ONE read in the three positions of a codon.  The slots are codon start positions,
 * starts[n_slots], strictly increasing, 0 <= s and s + 3 <= ref_len; names, strands and translation stay with the caller.  Only
 * reads with status 0 take part, as they were counted (the trimmed alignment with do_trim).  A read with a regular CIGAR -- hard
 * clips, soft clips, a core of M = X I D N ops, soft clips, hard clips, its query bases adding up to l_seq, QUAL present, all of it
 * inside the reference -- adds for the slot at start p:
 *   codon[slot][16 b0 + 4 b1 + b2] += 1   when [p, p + 3) lies inside one match segment (a run of M = X ops with no inserted,
 *                                         deleted or skipped base inside) and the three bases are among A C G T (0 1 2 3,
 *                                         reference-forward) with quality >= min_quality;
 *   codon[slot][64] += 1                  when [p, p + 3) lies inside [pos, ref_end) but inside no match segment: a deletion or
 *                                         skip overlaps it or an insertion sits between two of its positions (no quality test).
 * A codon the read covers only in part adds nothing.  reads[0] += 1 per such read; every other read with status 0 adds nothing to
 * the table and reads[1] += 1.  (codon: uint32[n_slots][65], reads: uint64[2].) */
/* The hook on for the slots given (the array is copied; more than 2^20 slots, an array that is not strictly increasing or a codon
 * that reaches past the reference: AMP_EINVAL), the tables zero; they are laid out again only when the set changed.  n_slots == 0
 * or a NULL array: off; the tables stay readable.  With the hook on and do_trim set, amp_process_batch_device refuses a dev_out
 * without new_pos, new_ncig, new_cig or status (AMP_EINVAL) before anything runs. */
int amp_codon_enable(amp_ctx *ctx, int32_t n_slots, const int32_t *starts);
/* Host copies of the tables as they stand (waits for the stream); either pointer may be NULL.  AMP_ESTATE before the first enable. */
int amp_codon_get(amp_ctx *ctx, uint32_t *codon /* [n_slots][65] */, uint64_t *reads /* [2] */);
/* Host tables added element-wise, like amp_add_counts (the merge of partial tables); either pointer may be NULL. */
int amp_codon_add(amp_ctx *ctx, const uint32_t *codon, const uint64_t *reads);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_codon_last_ms(amp_ctx *ctx, float *ms);

/* ---- deletion events (opt-in) ---------------------------------------------------------------------------------
 * The count table records a deleted base as one more '-' at one position (update_base_counts, AmpliPy.py:713-715): that one read
 * skipped several positions TOGETHER is lost there.  For a read with status 0, as it was counted (the trimmed alignment with
 * do_trim), an event is a maximal run of consecutive reference positions each of which the read's count walk adds to the '-' column
 * (AmpliPy.py:713-715): key (start, len), start 0-based, len >= 1.  D and N ops are alike; neighbouring D / N ops, and D / N ops
 * with only an insertion between them, are one event; a deletion that runs past the reference end is cut where the walk stops.  Per
 * key the table holds count (reads) and rev (those whose FLAG has 0x10), so that for every position p the counts of the events
 * with start <= p < start + len add up to counts[p]['-'] and their rev to rev[p][5] of the strand tallies.  The table is an
 * open-addressed hash table on the device that persists across batches; an event that finds no slot (every probe loop is
 * bounded) adds its reads to `lost` and is dropped -- never merged into another key.  amp_reset zeroes the table. */
typedef struct amp_del_event {
    int32_t start, len;         /* 0-based first deleted position, deleted positions */
    uint32_t count, rev;        /* reads that carry the event, those of them on the reverse strand */
} amp_del_event;
typedef struct amp_del_info {
    uint64_t used;              /* distinct events the table holds */
    uint64_t capacity;          /* its slots */
    uint64_t lost;              /* reads of events that found no slot */
} amp_del_info;
/* on != 0: the hook on, the table zero; 2^log2_capacity slots of 16 bytes (0: the default, 20; else 4 to 28, AMP_EINVAL
 * otherwise), laid out again only when the capacity changed.  on == 0: off; the table stays readable.  With the hook on and
 * do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig, new_cig or status (AMP_EINVAL) before
 * anything runs. */
int amp_del_enable(amp_ctx *ctx, int on, int log2_capacity);
/* The used entries as they stand (waits for the stream), compacted on the device, ordered by (start, len); *n: their number.
 * AMP_EINVAL, with the needed size in *n, when cap is smaller (info is filled in either way); AMP_ESTATE before the first enable.
 * n and info may be NULL, entries when cap is 0. */
int amp_del_get(amp_ctx *ctx, amp_del_event *entries, int64_t cap, int64_t *n, amp_del_info *info);
/* Host entries inserted through the kernel's own insert path (the merge of partial tables): a call per job, not per batch. */
int amp_del_add(amp_ctx *ctx, const amp_del_event *entries, int64_t n);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran.  Behind a batch
 * that ran with the hook off it answers what every switched-off hook answers: the time of the last batch that ran with it on
 * (AMP_ESTATE when there was none), whether the insertion evidence is on or not. */
int amp_del_last_ms(amp_ctx *ctx, float *ms);

/* ---- insertion alleles: strand, quality and read-position evidence (opt-in) ---------------------------
 * The insertion half of the indel unit: a hook of its own directly behind the deletion events', and either may be on alone
 * (amp_del_enable(ctx, 0, ...) switches the deletion events off only).  While it is on, one more kernel behind every
 * batch's read pass reads the insertion events that THIS batch's pass appended to the event list (whatever the caller's drain
 * pattern: the list's slot counts are noted in front of the pass) and tallies them per allele: key (ref_pos, len, hash) --
 * the two values amp_aggregate_ins_events sorts by, so one key is one allele of one position.  Per key: count (events), rev
 * (those of reads whose FLAG has 0x10), noqual (those of reads with QUAL '*', first byte 0xFF), qsum (the sum of the allele's
 * quality bytes over the other events) and bin[7]: the events by rp_bin(d) of the read-position tallies, d = max(0,
 * min(q_from - qs, qe - q_to)) with [qs, qe) the query span of the counted alignment (the trimmed one with do_trim).  The
 * table is an open-addressed hash table on the device that persists across batches; a key that finds no slot (every probe loop
 * is bounded) adds its events to `lost` and is dropped -- never merged into another key.  amp_reset zeroes the table. */
typedef struct amp_insev_entry {
    int32_t ref_pos, len;       /* the event's position, the allele's bases */
    uint64_t hash;              /* of the allele's base codes (63 bits) */
    uint32_t count, rev, noqual;
    uint64_t qsum;              /* (8-byte aligned: four bytes of padding in front) */
    uint32_t bin[7];
} amp_insev_entry;              /* 72 bytes */
typedef amp_del_info amp_insev_info;        /* used: distinct alleles; lost: EVENTS of keys that found no slot */
#define AMP_INSEV_STRIDE (512 * 256) /* events the kernel's fixed grid takes in one stride of its loop */
/* on != 0: the half on, the table zero; 2^log2_capacity slots of 64 bytes (0: the default, 20; else 4 to 28, AMP_EINVAL
 * otherwise), laid out again only when the capacity changed.  on == 0: off; the table stays readable.  With the hook on and
 * do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig, new_cig or status (AMP_EINVAL) before
 * anything runs, in this hook's name. */
int amp_insev_enable(amp_ctx *ctx, int on, int log2_capacity);
/* The used entries as they stand (waits for the stream), ordered by (ref_pos, len, hash); the rest as amp_del_get. */
int amp_insev_get(amp_ctx *ctx, amp_insev_entry *entries, int64_t cap, int64_t *n, amp_insev_info *info);
/* Host entries inserted through the kernel's own insert path (the merge of partial tables): a call per job, not per batch. */
int amp_insev_add(amp_ctx *ctx, const amp_insev_entry *entries, int64_t n);
/* Time of the hook's kernel (k_insev) behind the last batch, as amp_del_last_ms is k_del's; AMP_ESTATE when none ran. */
int amp_insev_last_ms(amp_ctx *ctx, float *ms);

/* ---- co-occurrence of listed mutations on single reads (opt-in) ----------------------------------------------
 * Do these listed mutations stand together on the SAME reads?  A set has 1 to 6 sites in strictly increasing position that do not
 * overlap, its first and last site at most 2^16 positions apart; set s has the sites [set_off[s], set_off[s + 1]) of site_pos
 * (0-based), site_len (0: a substitution; else a deletion of that many positions) and site_sym (substitutions: the base, 0..3 for
 * A C G T); the sets are sorted by the position of their first site (equal ones in any order).  Only reads with status 0 take
 * part, as they were counted (the trimmed alignment with do_trim, [pos, ref_end)).  On a read with a regular CIGAR (as for the
 * codon tallies) a site is
 *   substitution (p, b): MUT / NOT when p is a match position whose base is among A C G T with quality >= min_quality and is / is
 *                        not b; NOT when p is inside a D or N op; NONE otherwise (outside the alignment, base N, low quality);
 *   deletion (p, len):   NONE unless p - 1 and p + len lie in [pos, ref_end); then MUT when every position of [p, p + len) is
 *                        inside a D or N op and neither p - 1 nor p + len is, NOT otherwise (no quality test; positions, not ops);
 * and the read adds cooc[set][sum of 2^j over the sites j that are MUT] += 1 when no site is NONE, cooc[set][64] += 1 when some
 * but not all are, nothing when all are.  reads[0] += 1 per such read; every other read with status 0 adds nothing to the table
 * and reads[1] += 1.  Insertions are not sites.  (cooc: uint32[n_sets][65], reads: uint64[2].) */
/* The hook on for the sets given (the arrays are copied; more than 2^16 sets, a set without or with more than 6 sites, sites that
 * overlap or are out of order, a site outside the reference, sets that are not sorted, a span above 2^16: AMP_EINVAL), the tables
 * zero; they are laid out again only when the sets changed.  n_sets == 0 or a NULL set_off: off; the tables stay readable.  With
 * the hook on and do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig, new_cig or status
 * (AMP_EINVAL) before anything runs. */
int amp_cooc_enable(amp_ctx *ctx, int32_t n_sets, const int32_t *set_off /* [n_sets + 1] */, const int32_t *site_pos, const int32_t *site_len,
                    const uint8_t *site_sym);
/* Host copies of the tables as they stand (waits for the stream); either pointer may be NULL.  AMP_ESTATE before the first enable. */
int amp_cooc_get(amp_ctx *ctx, uint32_t *cooc /* [n_sets][65] */, uint64_t *reads /* [2] */);
/* Host tables added element-wise, like amp_add_counts (the merge of partial tables); either pointer may be NULL. */
int amp_cooc_add(amp_ctx *ctx, const uint32_t *cooc, const uint64_t *reads);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_cooc_last_ms(amp_ctx *ctx, float *ms);

/* ---- The error profile by cycle, quality and substitution (opt-in) ----
 * How often a base differs from the reference.  While the hook is on, one more kernel behind the read pass of every batch (the
 * last of the hooks) visits every read with status 0 whose counted alignment (the trimmed one with do_trim) is regular in the
 * sense of the codon tallies above.  Every base of every match op (M = X) of such a read, WHATEVER its quality, with
 *   b: the read base, one of A C G T;  x: the reference letter at its position, upper-cased, one of A C G T, not masked
 *      (a base with another b or x takes no part);
 *   m: FLAG & 0x80 (unpaired reads are mate 0);  s: FLAG & 0x10;
 *   c: min(s ? l_seq - 1 - q : q, 511) for query index q -- the cycle from the 5' end of the stored SEQ, hard clips not counted;
 *   v: min(qual, 93);  e: b != x;  g: qual >= min_quality
 * adds 1 to cyc[m][c][e], qualt[m][v][e] and sub[m][s][g][x][b] (x, b: A C G T as 0 1 2 3).  reads[0] += 1 per such read; every
 * other read with status 0 adds nothing to the tables and reads[1] += 1.  For each m the sums of cyc[m], qualt[m] and sub[m] are
 * equal; with no mask, on a batch whose status-0 reads are all regular, the sum over m, s of sub[m][s][1][X][b] is the sum of
 * counts[p][b] over the positions p whose upper-cased reference letter is X.
 * (cyc: uint64[2][512][2], qualt: uint64[2][94][2], sub: uint64[2][2][2][4][4], reads: uint64[2].) */
#define AMP_EP_CYCLES 512
#define AMP_EP_QUALS 94
/* on != 0: the hook on for the reference letters given (copied; mask_bits: bit p & 31 of word p >> 5 set for a position that
 * takes no part, NULL: none), the tables zero -- at every call.  A NULL ref_ascii with on: AMP_EINVAL.  on == 0: off; the
 * tables stay readable.  With the hook on and do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig,
 * new_cig or status (AMP_EINVAL) before anything runs. */
int amp_errprof_enable(amp_ctx *ctx, int on, const uint8_t *ref_ascii /* [ref_len] */, const uint32_t *mask_bits /* [(ref_len + 31) / 32] or NULL */);
/* Host copies of the tables as they stand (waits for the stream); any pointer may be NULL.  AMP_ESTATE before the first enable. */
int amp_errprof_get(amp_ctx *ctx, uint64_t *cyc, uint64_t *qualt, uint64_t *sub, uint64_t *reads);
/* Host tables added element-wise, like amp_add_counts (the merge of partial tables); any pointer may be NULL. */
int amp_errprof_add(amp_ctx *ctx, const uint64_t *cyc, const uint64_t *qualt, const uint64_t *sub, const uint64_t *reads);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_errprof_last_ms(amp_ctx *ctx, float *ms);

/* ---- read haplotypes per region: distinct mutation sets on single reads (opt-in) ------------------------------
 * Which combinations of differences from the reference exist on single reads over a stretch, and how many reads carry each?
 * REGIONS: [start, end), 0-based, 1 to AMP_HAP_MAX_REGION positions each, at most 2^16, sorted by start; they may overlap.
 * READS: only reads with status 0, as they were counted (the trimmed alignment [pos, ref_end) with do_trim), with a regular CIGAR
 * (as for the co-occurrence tallies).  Every other status-0 read, and a regular read that covers no region: reads[1] += 1 and
 * nothing else.  A read that covers at least one region: reads[0] += 1.  A read is tried against every region with pos <= start
 * and end <= ref_end; inside it every position is a match position or a deleted one (inside a D or N op).
 * A TRIAL adds tally[region][COVER] += 1, then exactly one of, tested in this order:
 *   1 EDGE      the region's first or last position is deleted (the run may go on outside the region: it cannot be named);
 *   2 LOWQ      some match position has a reference letter among A C G T (either case), a read base that differs from it and a
 *               quality below min_quality (a read without QUAL, 0xFF, counts as below, as everywhere else);
 *   3 OVERFLOW  the differences (below) are more than AMP_HAP_MAX_DIFFS;
 *   4 REF       there are none: tally[region][REF] += 1, and tally[region][REF_REV] += 1 when the FLAG has 0x10;
 *   5           the key (region, differences) goes to the table: count += 1, and rev += 1 when reverse.
 * DIFFERENCES, in ascending offset: a maximal run of deleted positions is one difference of kind 5 with its length (after the EDGE
 * test both flanks are match positions inside the region); a match position whose reference letter is among A C G T, whose read
 * base differs from it and whose quality is at or above min_quality is one of kind 0..3 for A C G T, 4 for N.  A position whose
 * reference letter is not A C G T is never a difference; a low-quality base that equals the reference is none and does not
 * disqualify the read.  INSERTIONS ARE NOT DIFFERENCES, as they are not co-occurrence sites: two reads that differ only by an
 * insertion fall together; the insertion alleles are in the VCF.
 * THE DIFFERENCE WORD: bits 0-11 the offset in the region, 12-14 the kind, 15-27 the deletion length (0: a substitution), the rest
 * zero.  THE KEY: 14 words: head = region index | n_diffs << 16, then 13 difference words, the unused ones zero.
 * THE INVARIANT, per region: COVER == REF + LOWQ + OVERFLOW + EDGE + the counts of the region's entries + its lost reads.
 * The table is an open-addressed hash table on the device that persists across batches; a read whose key finds no slot (every
 * probe loop is bounded) adds to `lost` -- counted, never merged into another key.  amp_reset zeroes the tables. */
#define AMP_HAP_MAX_DIFFS 13
#define AMP_HAP_MAX_REGION 4096
#define AMP_HAP_TALLY_COLS 6   /* COVER REF REF_REV LOWQ OVERFLOW EDGE */
typedef struct amp_hap_entry {   /* 64 bytes */
    uint32_t head;
    uint32_t diff[13];
    uint32_t count;
    uint32_t rev;
} amp_hap_entry;
typedef struct amp_hap_info {
    uint64_t used;              /* distinct keys the table holds */
    uint64_t capacity;          /* its slots */
    uint64_t lost;              /* reads whose key found no slot */
} amp_hap_info;
/* The hook on for the regions and the reference letters given (copied; the reference is packed once into 4-bit codes and a mask
 * of its A C G T positions), the tables zero; 2^log2_capacity slots of 64 bytes (0: the default, 20; else 4 to 28).  A region that
 * is unsorted, empty, too long or outside the reference, more than 2^16 regions, a bad capacity, regions without ref_ascii:
 * AMP_EINVAL.  n_regions == 0 or a NULL start or end: off; the tables stay readable.  With the hook on and do_trim set,
 * amp_process_batch_device refuses a dev_out without new_pos, new_ncig, new_cig or status (AMP_EINVAL) before anything runs. */
int amp_hap_enable(amp_ctx *ctx, int32_t n_regions, const int32_t *start, const int32_t *end, const uint8_t *ref_ascii /* [ref_len] */, int log2_capacity);
/* The used entries as they stand (waits for the stream), compacted on the device, ordered by their 14 key words; *n: their number.
 * AMP_EINVAL, with the needed size in *n, when cap is smaller (info, tally and reads are filled in either way); AMP_ESTATE before
 * the first enable.  n, info, tally and reads may be NULL, entries when cap is 0. */
int amp_hap_get(amp_ctx *ctx, amp_hap_entry *entries, int64_t cap, int64_t *n, amp_hap_info *info, uint64_t *tally /* [n_regions][6] */,
                uint64_t *reads /* [2] */);
/* Host entries inserted through the kernel's own insert path, tally and reads added element-wise (the merge of partial tables): a
 * call per job, not per batch.  tally and reads may be NULL. */
int amp_hap_add(amp_ctx *ctx, const amp_hap_entry *entries, int64_t n, const uint64_t *tally, const uint64_t *reads);
/* Time of the hook's kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_hap_last_ms(amp_ctx *ctx, float *ms);

/* ---- read-position tallies per allele: where on its reads an allele sits (opt-in) ---------------------------
 * For every increment the read pass makes to one of the six fixed keys A C G T N '-' of a position r (reads with status 0, the
 * trimmed alignment with do_trim), hist[r][column][bin(d)] += 1.  [qs, qe) is the kept query span of the counted alignment
 * (query_alignment_start / _end: the read without its soft clips).  A match base at query index q has d = min(q - qs, qe - 1 - q),
 * the kept query bases between it and the nearer end; a deleted position (D, N) has d = max(0, min(q_next - qs, qe - q_next) - 1),
 * the smaller distance of its two flanking bases, q_next being the query index of the next base behind the deletion.
 * bin(d) = min(6, bit_length(d >> 1)): d < 2, 2-3, 4-7, 8-15, 16-31, 32-63, >= 64.  Insertion alleles are not part of the table.
 * The sum of a cell's bins is the count table's cell, so 32 bits suffice wherever the count table's do.  amp_reset zeroes the table. */
#define AMP_RP_BINS 7
/* on != 0: the tallies on, the table (uint32[ref_len][AMP_NSYM][AMP_RP_BINS], allocated at the first call) zero.  on == 0: off; the
 * table stays readable.  With the tallies on and do_trim set, amp_process_batch_device refuses a dev_out without new_pos, new_ncig,
 * new_cig or status (AMP_EINVAL) before anything runs. */
int amp_readpos_enable(amp_ctx *ctx, int on);
/* Host copy of the table as it stands (waits for the stream); hist may be NULL.  AMP_ESTATE before the first enable. */
int amp_readpos_get(amp_ctx *ctx, uint32_t *hist /* [ref_len][AMP_NSYM][AMP_RP_BINS] */);
/* A host table added element-wise, like amp_add_counts (the merge of partial tables); hist may be NULL. */
int amp_readpos_add(amp_ctx *ctx, const uint32_t *hist);
/* Time of the tallies' kernel behind the last batch (HIP events on the ctx stream); AMP_ESTATE when none ran. */
int amp_readpos_last_ms(amp_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* AMPLIHIP_H */
