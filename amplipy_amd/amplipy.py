"""Host mirror of AmpliPy's command-line / run_amplipy surface on top of the HIP engine.

Same sub-commands, flags, defaults, log lines and error behaviour as AmpliPy.py v0.0.2
(parse_args AmpliPy.py:113-171, run_amplipy :774-963, __main__ :966-1025); the per-read loop
(:896-915) is replaced by batches handed to libamplihip.so, calling (:917-952) by
``amplipy_amd.calling``, and pysam I/O by ``amplipy_amd.bamio``.  There is no CPU execution
path: without a GPU the engine raises.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
import types
from os.path import isfile

from . import AMPLIPY_VERSION, abi, calling, clips, insevidence, lib, parallel, qc, reports
from .drivers import (NATIVE_BATCH_READS, DeviceBamDriver, NativeDriver, NativeInput, native_parts, open_driver,  # noqa: F401
                      select)
from .readloop import BATCH_READS, PROGRESS_NUM_READS, ReadLoop, error, print_log  # noqa: F401

VERSION = AMPLIPY_VERSION

DEFAULTS = dict(min_depth_consensus=10, min_depth_variants=1, min_freq_consensus=0, min_freq_variants=0.03,
                min_length=30, min_quality=20, primer_pos_offset=0, sliding_window_width=4, unknown_symbol="N")


# ---- loaders (AmpliPy.py:212-258) --------------------------------------------------------------
def load_ref_genome(reference_fn):
    if not isfile(reference_fn):
        error("File not found: %s" % reference_fn)
    with open(reference_fn) as f:
        lines = f.read().strip().splitlines()
    if len(lines) < 2 or not lines[0].startswith(">"):
        error("Invalid FASTA file: %s" % reference_fn)
    ref_id = lines[0][1:].split()[0].strip()
    seq = "".join(lines[1:])
    if ">" in seq:
        error("Multiple sequences in FASTA file: %s" % reference_fn)
    return ref_id, seq


def load_primers(primer_fn):
    if not isfile(primer_fn):
        error("File not found: %s" % primer_fn)
    with open(primer_fn) as f:
        lines = f.read().strip().splitlines()
    primers = []
    for l in lines:
        parts = l.split("\t")
        try:
            if len(parts) != 4:
                raise ValueError
            primers.append((int(parts[1]), int(parts[2])))
        except ValueError:
            error("Invalid primer BED line: %s" % l)
    if not primers:
        raise NameError("name 'header' is not defined")      # what the reference does on an empty BED (:255)
    primers.sort()
    return primers


def gpu_codec_wanted(arg, env_name):
    """The opt-in switch of a device codec: the argument of run_amplipy when it is given, else the variable set to anything but 0."""
    return bool(arg) if arg is not None else os.environ.get(env_name, "0") not in ("", "0")


def open_device_bam_text(input_fn, output_fn):
    """(bam_device.DeviceBamInput, AlignmentWriter, binary output) when the device codec for BAM input can write this run's trimmed
    reads as SAM text, None otherwise: the ``drivers.select`` route of a run with both switches on, then what
    ``drivers.DeviceBamDriver.open`` finds in the header."""
    if select(input_fn, output_fn, True, gpu_sam=True, gpu_bam=True)[:2] != ("device_bam", "text"):
        return None
    driver = DeviceBamDriver.open(input_fn, output_fn, "text")
    return driver and (driver.src, driver.sink.writer, driver.sink.outb)


class VcfWriter:
    """Text VCF with the header AmpliPy builds through pysam (AmpliPy.py:271-281)."""

    def __init__(self, fn, ref_id, strand=False, amplicon=False, codon=False, deletion=False, cooc=False, errprof=False, hap=False, readpos=False,
                 insertions=False):
        """Each keyword of calling.INFO_ORDER: the header also declares the INFO keys of that report, in that order (``line``
        appends them when given the report's tables).  insertions: the two keys of the indel unit's insertion half
        (insevidence.py), behind the deletion keys' place -- the half has no report of its own."""
        if fn.lower() == "stdout":
            self.f = sys.stdout
        elif isfile(fn):
            error("File already exists: %s" % fn)
        elif fn.lower().endswith(".vcf"):
            self.f = open(fn, "w")
        elif fn.lower().endswith(".vcf.gz"):
            self.f = gzip.open(fn, "wt")
        elif fn.lower().endswith(".bcf"):
            error("BCF output is not supported by this build (use .vcf or .vcf.gz): %s" % fn)
        else:
            error("Invalid variants extension (should be .vcf, .vcf.gz, or .bcf): %s" % fn)
        self.ref_id = ref_id
        w = self.f.write
        w("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n")
        w("##AmpliPyVersion=%s\n##source=%s\n##contig=<ID=%s>\n" % (VERSION, " ".join(sys.argv), ref_id))
        w("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        w("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Total Depth\">\n")
        w("##INFO=<ID=REF_DP,Number=1,Type=Integer,Description=\"Depth of reference base\">\n")
        w("##INFO=<ID=ALT_DP,Number=1,Type=String,Description=\"Depth of alternate base\">\n")
        w("##INFO=<ID=REF_FREQ,Number=1,Type=Float,Description=\"Frequency of reference base\">\n")
        w("##INFO=<ID=ALT_FREQ,Number=1,Type=String,Description=\"Frequency of alternate base\">\n")
        on = dict(zip(calling.INFO_ORDER, (strand, amplicon, codon, deletion, cooc, errprof, hap, readpos)))
        w("".join([(R.HEADER_LINES if on[R.name] else "") + (insevidence.HEADER_LINES if insertions and R.name == "deletion" else "") for R in reports.REGISTRY]))
        w("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")

    def line(self, r, strand=None, amplicon=None, codon=None, deletion=None, cooc=None, errprof=None, hap=None, readpos=None):
        return calling.vcf_line(self.ref_id, r, strand, amplicon, codon, deletion, cooc, errprof, hap, readpos)

    def write(self, r, strand=None, amplicon=None, codon=None, deletion=None, cooc=None, errprof=None, hap=None, readpos=None):
        self.f.write(self.line(r, strand, amplicon, codon, deletion, cooc, errprof, hap, readpos))

    def write_all(self, records, strand=None, amplicon=None, codon=None, deletion=None, cooc=None, errprof=None, hap=None, readpos=None):
        self.f.write("".join([self.line(r, strand, amplicon, codon, deletion, cooc, errprof, hap, readpos) for r in records]))

    def close(self):
        if self.f is not sys.stdout:
            self.f.close()


def run_amplipy(untrimmed_reads_fn=None, primer_fn=None, reference_fn=None, trimmed_reads_fn=None, variants_fn=None,
                consensus_fn=None, primer_pos_offset=None, min_length=None, min_quality=None, sliding_window_width=None,
                min_freq_consensus=None, min_freq_variants=None, min_depth_consensus=None, min_depth_variants=None,
                unknown_symbol=None, include_no_primer=None, run_trim=False, run_variants=False, run_consensus=False,
                device=None, gpu_sam=None, gpu_bam=None, gpu_bam_write=None, qc_fn=None, qc_regions_fn=None, qc_depths=None,
                qc_depth_fn=None, strand=False, strand_fn=None, amplicons_fn=None, amplicon_out_fn=None, codons_fn=None,
                codon_out_fn=None, aa_out_fn=None, deletions=False, del_out_fn=None, indel_vcf_fn=None, del_capacity=None, cooc_fn=None,
                cooc_out_fn=None, error_profile_fn=None, error_mask_fn=None, haplotypes_fn=None, hap_out_fn=None, hap_min_reads=None,
                hap_min_freq=None, hap_capacity=None, readpos=False, readpos_end=None, readpos_fn=None, insertions=False, ins_out_fn=None,
                ins_capacity=None, ins_end=None, qc_clips=False, qc_clip_fn=None, qc_junction_fn=None, qc_clip_min=None, qc_clip_reads=None):
    """The reference's run_amplipy (AmpliPy.py:774-963) on the MI355X engine.

    gpu_sam (default: AMPLIPY_GPU_SAM, off): SAM text in (and SAM text or nothing out) goes through the device codec of
    sam_native instead of the Python codec; one process only.  With gpu_bam_write on as well, SAM text in and a new BAM file of
    trimmed reads out does too: records, compression and framing are made on the device.
    gpu_bam (default: AMPLIPY_GPU_BAM, off): a BAM file in and no trimmed reads out (variants, consensus) is inflated, indexed and
    decoded on the device (bam_device) instead of by libampbam; one process only.  Runs that write trimmed reads keep libampbam,
    unless gpu_bam_write (default: AMPLIPY_GPU_BAM_WRITE, off) is on as well: a BAM file in and a new BAM file of trimmed reads out
    (trim, aio) then stay on the device codec, which re-encodes, compresses and frames the kept records too.
    gpu_bam and gpu_sam both on: a BAM file in and trimmed reads out as SAM text (stdout or a new .sam file; trim, aio) stay on the
    device codec for BAM input, which turns the kept records into SAM lines (bam_device); a piece with a record
    the device would not write exactly like the Python codec goes through that codec.  One process only.
    qc_fn (default: off): the amplicon QC report as JSON -- reads per primer, reads kept and dropped, depth
    per region -- tallied on the device behind every batch's read pass, whichever codec feeds it.  qc_regions_fn: a BED of further
    regions (ref, start, end, name); qc_depths: up to 4 depth thresholds (1, 10, 100); qc_depth_fn: depth of every position as a
    TSV file (runs with a count table).  With all four None the engine's report is never switched on.
    qc_clips (default: off; needs qc_fn): the report gains the section "clips"  -- soft-clip sites and the
    junctions they place: deletions and duplications the aligner clipped instead of opening a gap for them.  A second kernel of
    the QC unit tallies, per reference position and side, the reads clipped there by at least qc_clip_min bases (1..64, default
    10) and their first 16 clipped bases; the host builds a consensus per site with at least qc_clip_reads reads (default 2),
    holds it against the reference and reports what lands elsewhere.  qc_clip_fn: every such site as a TSV file; qc_junction_fn:
    the junctions as a TSV file; either switches the report's hook on by itself.  With all three off the kernel never runs.
    strand (default: off; runs that write a VCF): every VCF record also carries REF_RV, ALT_RV, REF_QUAL, ALT_QUAL and SB
     -- reverse-strand depth, mean base quality and a strand-bias p-value per allele -- from two more tables
    the device tallies behind every batch's read pass.  strand_fn: the tables of every position as a TSV file (runs with a count
    table).  With both off the engine's tallies are never switched on.
    amplicons_fn (default: off; aio only): the amplicon file -- left primer, right primer and, optionally, an amplicon name per
    line.  Every read is assigned to an amplicon by its original coordinates, the device keeps a count
    table per amplicon behind every batch's read pass, and every VCF record also carries AMP, AMP_DP, AMP_REF_DP, AMP_ALT_DP,
    AMP_NA_DP, AMP_P and PRIMER.  amplicon_out_fn: the per-amplicon table as a TSV file.  With amplicons_fn None the engine's
    hook is never switched on.
    codons_fn (default: off; runs with a count table): the CDS file -- name, start, end and, optionally, strand per line, 0-based
    and half-open.  The device tallies, behind every batch's read pass, which bases stand together on one
    read in the three positions of every codon, and every VCF record also carries CDS, CODON_DP, ALT_AA, ALT_CODON and
    ALT_CODON_DP.  codon_out_fn: the codon table as a TSV file; aa_out_fn (runs that call variants): the amino-acid changes at or
    above the variant thresholds.  With codons_fn None the engine's hook is never switched on.
    deletions (default: off; runs that write a VCF): the device tallies, behind every batch's read pass, deletions as whole
    events -- the positions ONE read skipped together, with the reads and the reverse reads that carry each (DESIGN.md section
    19) -- and every VCF record also carries DEL_N and DEL.  del_out_fn: every event as a TSV file (runs with a count table);
    indel_vcf_fn (runs that call variants): a second, spec-valid VCF of anchored indels -- the events and the call's insertion
    alleles at or above the variant thresholds.  del_capacity: log2 of the device table's slots (default 20).  Reads of events
    the table had no slot for end the run with an error.  With the first three off the engine's hook is never switched on.
    insertions (default: off; runs that write a VCF): the insertion half of the same unit.  The device
    tallies, behind every batch's read pass, the batch's insertion events per allele -- reads, reverse reads, quality sum, reads
    without qualities and seven bins of the allele's distance to the nearer end of the read's kept bases -- and every VCF record
    also carries INS_N and INS.  ins_out_fn: every allele as a TSV file (runs with a count table).  ins_capacity: log2 of the
    device table's slots (default 20).  ins_end: the distance below which an allele counts as at a read end (one of 2, 4, 8, 16,
    32, 64; default 8).  With the half on, the insertion rows of indel_vcf_fn carry RV.  The device entries are joined with the
    run's allele texts as a check: a miss, a double hit or a count mismatch ends the run with an error that names the position.
    cooc_fn (default: off; runs with a count table): the mutation-set file -- a name and a comma-separated list of mutations per
    line, A23403G, del21765-21770 or del21991, POSITIONS 1-BASED as in the VCF.  The device tallies,
    behind every batch's read pass, per set the reads that show all its sites by the pattern of mutations they carry, and every
    VCF record also carries COOC.  cooc_out_fn: the pattern table as a TSV file.  With cooc_fn None the engine's hook is never
    switched on.
    error_profile_fn (default: off; runs with a count table): the error profile as JSON -- how often a base
    differs from the reference by sequencing cycle, by reported quality and by substitution class, tallied on the device behind
    every batch's read pass over every match base of every regular read -- and, on runs that write a VCF, ERR_RATE and ERR_P
    on every record: the run's rate of reading the REF base as the ALT base, and the binomial tail of the ALT depth under it.
    error_mask_fn: positions that take no part, as a VCF (of a first run, say) or a BED file; WITHOUT A MASK THE SITE'S OWN BASES
    ARE PART OF THE RATE, so a real variant at high frequency raises the rate it is held against.  With error_profile_fn None
    the engine's hook is never switched on.
    haplotypes_fn (default: off; runs with a count table): the region file, a BED (ref, start, end, name; 0-based, half-open; 1 to
    4096 positions a region).  The device tallies, behind every batch's read pass, per region the distinct
    sets of differences from the reference -- substitutions and deletions, never insertions -- that single reads carry over the
    whole region, and the reads that carry each; every VCF record also carries HAP_N and HAP.  hap_out_fn: the haplotype table as
    a TSV file, mutations 1-based in the grammar of cooc_fn; hap_min_reads (2) and hap_min_freq (0): what it lists.  hap_capacity:
    log2 of the device table's slots (default 20).  Reads whose haplotype the table had no slot for end the run with an error.
    With haplotypes_fn None the engine's hook is never switched on.
    readpos (default: off; runs that write a VCF): every VCF record also carries REF_RP, ALT_RP, REF_END, ALT_END, RPB and RPZ
     -- where on its reads an allele sits: the supporting bases by their distance to the nearer end of the
    read's kept bases in seven bins, the support within readpos_end (one of 2, 4, 8, 16, 32, 64; default 8) of a read end, a
    Fisher p-value and a rank-sum z against the reference base -- from one more table the device tallies behind every batch's
    read pass.  readpos_fn: the table of every position as a TSV file (runs with a count table); it alone switches the tallies on.
    With both off the engine's hook is never switched on.

    One process drives one GPU.  Under ``torchrun`` (WORLD_SIZE > 1, or AMPLIPY_FORCE_DIST=1 for a one-rank
    rehearsal) the job is range-partitioned: rank r takes the r-th contiguous run of BAM records (coordinate
    order), every rank's count table is summed with ONE all-reduce over RCCL (parallel.allreduce_table), the
    insertion alleles of the flagged positions are exchanged, and rank 0 writes the VCF / consensus and every report.
    Trimmed reads are written per rank (``<name>.part<rank><ext>``).  For BAM input (libampbam) rank 0 joins the parts into
    the ONE file the caller named and removes them.  For text input the reads are dealt out one by one and the parts are
    NOT joined: they stay, and their records together are the one-process file's records in another order.
    """
    run = types.SimpleNamespace(**locals())      # (first statement: the keyword arguments, under their names, and nothing else)
    dist, rank, world = parallel.init_from_env()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if dist is not None else 0
    v_min_depth = min_depth_variants if min_depth_variants is not None else 0
    v_min_freq = min_freq_variants if min_freq_variants is not None else 0
    vars(run).update(dist=dist, rank=rank, world=world, device=device, min_quality=min_quality if min_quality is not None else 20,
                     v_min_depth=v_min_depth, v_min_freq=v_min_freq)
    # argument checks and banner: AmpliPy.py:836-866
    if primer_pos_offset is not None and primer_pos_offset < 0:
        error("Primer position offset must be non-negative: %s" % primer_pos_offset)
    if min_length is not None and min_length < 1:
        error("Minimum length must be >= 1: %s" % min_length)
    if min_quality is not None and min_quality < 0:
        error("Minimum quality must be non-negative: %s" % min_quality)
    if sliding_window_width is not None and sliding_window_width < 1:
        error("Sliding window width must be >= 1: %s" % sliding_window_width)
    for v in (min_freq_consensus, min_freq_variants):
        if v is not None and (v < 0 or v > 1):
            error("Minimum frequency must be between 0 and 1: %s" % v)
    for v in (min_depth_consensus, min_depth_variants):
        if v is not None and v < 0:
            error("Minimum depth must be positive: %s" % v)
    if unknown_symbol is not None and len(unknown_symbol) != 1:
        error("Unknown symbol must be exactly 1 character: %s" % unknown_symbol)
    if not (run_trim or run_variants or run_consensus):
        error("Not running any of the AmpliPy operations")
    if qc_fn is None and (qc_regions_fn is not None or qc_depths is not None):
        error("QC regions and QC depth thresholds need a QC report (--qc)")
    if qc_depth_fn is not None and not (run_variants or run_consensus):
        error("A run that only trims has no count table: no per-position depth (--qc_depth_out)")
    clips_on = bool(qc_clips) or qc_clip_fn is not None or qc_junction_fn is not None       # (the run's arguments alone: every rank agrees)
    if qc_clips and qc_fn is None:
        error("The clip section is part of the QC report: it needs one (--qc_clips needs --qc)")
    if not clips_on and (qc_clip_min is not None or qc_clip_reads is not None):
        error("A clip length or a read threshold without clip sites (--qc_clip_min and --qc_clip_reads need --qc_clips, --qc_clip_out or --qc_junction_out)")
    if clips_on:
        qc_clip_min = clips.DEFAULT_CLIP_MIN if qc_clip_min is None else qc_clip_min
        qc_clip_reads = clips.DEFAULT_MIN_READS if qc_clip_reads is None else qc_clip_reads
        if not 1 <= qc_clip_min <= abi.CLIP_MIN_MAX:
            error("Minimum clip length must be between 1 and %d: %s" % (abi.CLIP_MIN_MAX, qc_clip_min))
        if qc_clip_reads < 1:
            error("Minimum reads of a clip site must be >= 1: %s" % qc_clip_reads)
    every = [R() for R in reports.REGISTRY]
    for r in every:
        r.check(run)
    on = [r for r in every if r.active(run)]
    qc_on = qc_fn is not None or qc_depth_fn is not None or clips_on
    if qc_on:
        qc_depths = list(qc.DEFAULT_DEPTHS) if qc_depths is None else list(qc_depths)
        if len(qc_depths) > 4 or any(d < 0 for d in qc_depths):
            error("QC depth thresholds: at most 4, each non-negative: %s" % (qc_depths,))
    mode = "Trim" if run_trim and not (run_variants or run_consensus) else \
        "Variants" if run_variants and not (run_trim or run_consensus) else \
        "Consensus" if run_consensus and not (run_trim or run_variants) else "All-In-One"
    print_log("Executing AmpliPy %s (v%s)" % (mode, VERSION))

    ref_id = ref_seq = None
    if reference_fn is not None:
        print_log("Loading reference genome: %s" % reference_fn)
        ref_id, ref_seq = load_ref_genome(reference_fn)
    G = len(ref_seq)
    vars(run).update(G=G, ref_id=ref_id, ref_seq=ref_seq)
    eng = lib.Engine(G, device=device)
    if os.environ.get("AMPLIPY_DEV") == "1" and os.environ.get("AMPLIPY_KERNEL_VARIANT"):      # (A/B checks of the tests: all variants give the same files)
        eng.set_kernel_variant(int(os.environ["AMPLIPY_KERNEL_VARIANT"]))
    table = None
    final_trimmed_fn = None
    if dist is not None:
        import torch
        torch.cuda.set_device(device)
        table = torch.zeros(G * 7, dtype=torch.int32, device="cuda:%d" % device)   # counts + insertion tally
        eng.bind_counts(table.data_ptr())
        if run_trim and trimmed_reads_fn is not None and world > 1:
            # every rank writes the trimmed reads of its share to a file of its own; rank 0 joins them into the ONE file the
            # caller asked for once every rank is done (BGZF members concatenate: bam_native.stitch_bam_parts)
            final_trimmed_fn = trimmed_reads_fn
            root, ext = os.path.splitext(trimmed_reads_fn)
            trimmed_reads_fn = "%s.part%d%s" % (root, rank, ext)
    if primer_fn is not None:
        print_log("Loading primers: %s" % primer_fn)
        primers = load_primers(primer_fn)
        print_log("Precalculating overlapping primers...")
        mn, mx, mpl = lib.find_overlapping_primers(G, primers, primer_pos_offset)
        eng.set_primers(mn, mx, mpl)
    # Opening the files can fail on ONE rank of a multi-rank run (a missing share, an output that exists): the other ranks must
    # not be left waiting in the collective, so with several ranks the failure is carried to the exchange in front of it
    driver = vcf = rank_error = None
    qc_files, qc_regions, qc_primers = [None, None, None, None], [], []
    reads_in, reads_out = (untrimmed_reads_fn, trimmed_reads_fn) if run_trim else (trimmed_reads_fn, None)
    try:
        if rank == 0 and final_trimmed_fn is not None and final_trimmed_fn.lower() != "stdout" and isfile(final_trimmed_fn):
            raise FileExistsError("File already exists: %s" % final_trimmed_fn)      # (only rank 0 looks: carried to the exchange like the rest)
        if run_trim:
            print_log("Input untrimmed SAM/BAM: %s" % untrimmed_reads_fn)
            print_log("Output trimmed SAM/BAM: %s" % trimmed_reads_fn)
        else:
            print_log("Input trimmed SAM/BAM: %s" % trimmed_reads_fn)
        route = select(reads_in, reads_out, run_trim, gpu_codec_wanted(gpu_sam, "AMPLIPY_GPU_SAM"), gpu_codec_wanted(gpu_bam, "AMPLIPY_GPU_BAM"),
                       gpu_codec_wanted(gpu_bam_write, "AMPLIPY_GPU_BAM_WRITE"), several=dist is not None)
        driver = open_driver(route, reads_in, reads_out, rank, world, device, several=dist is not None)
        if route.note:
            print_log(route.note)
        if variants_fn is not None and rank == 0:
            print_log("Output variants VCF: %s" % variants_fn)
            vcf = VcfWriter(variants_fn, ref_id, insertions=bool(insertions), **{r.name: r.annotates(run) for r in on})
        for r in on:
            r.open(run)
        if qc_on:
            qc_regions = [(0, G, qc.WHOLE)] + (qc.load_regions(qc_regions_fn) if qc_regions_fn is not None else [])
            qc_primers = qc.load_primer_rows(primer_fn) if run_trim else []
            if rank == 0:
                qc_files = [qc.open_new(fn) if fn is not None else None for fn in (qc_fn, qc_depth_fn, qc_clip_fn, qc_junction_fn)]
    except (Exception, SystemExit) as e:
        if dist is None:
            raise
        rank_error = e if isinstance(e, Exception) else RuntimeError("could not open the run's files (exit status %s)" % (e.code,))
        driver = None                     # (nothing is walked: straight to the exchange)
    do_count = run_variants or run_consensus
    eng.set_params(min_quality if min_quality is not None else 20,
                   sliding_window_width if sliding_window_width is not None else 4, run_trim, do_count)

    if qc_on and rank_error is None:
        eng.qc_enable([(s, e) for s, e, _ in qc_primers], primer_pos_offset or 0, min_length if min_length is not None else 0,
                      include_no_primer, [(s, e) for s, e, _ in qc_regions], qc_depths)
        if clips_on:
            eng.qc_clips_enable(qc_clip_min)
    if rank_error is None:
        for r in on:
            r.enable(run, eng)
    print_log("Processing reads...")
    loop = ReadLoop(eng, min_length, include_no_primer, run_trim, do_count)
    vars(run).update(ins_store=loop.ins_store)    # (the insertion evidence joins the device entries with the run's allele texts)
    if driver is not None:
        try:
            driver.run(loop)
        except Exception as e:            # with several ranks the others must not be left waiting in the collective
            if dist is None:
                raise
            rank_error = e

    if dist is not None:
        # before the one collective of the run: did every rank get through its share (a rank that raised must not leave the
        # others waiting in the all-reduce), and do the shares of neighbouring ranks meet (every share of a BAM file starts
        # where the one before it ended: what makes the split of ampbam_open_range exact)
        trouble = parallel.exchange_notes(dist, world, driver.seam if driver is not None else [None, None], rank_error)
        if trouble:
            print_log("ERROR: %s" % trouble)          # (every rank's log names the rank that failed and what it failed of)
            eng.close()
            parallel.finish(dist)
            if rank_error is not None:
                raise rank_error
            raise RuntimeError(trouble)
        shares = parallel.gather_objects(dist, rank, world, (loop.n_seen, loop.n_bases))
        if rank == 0 and isinstance(driver, NativeDriver):
            # the file is cut by compressed bytes (ampbam_open_range): what that gave every rank, in records and in bases
            tot = max(sum(b_ for _, b_ in shares), 1)
            print_log("Shares of the %d ranks: records %s; bases %s (%s %% of the job)" % (world, [r_ for r_, _ in shares], [b_ for _, b_ in shares],
                                                                                        ", ".join("%.1f" % (100.0 * b_ / tot) for _, b_ in shares)))
        if qc_on:                        # every rank's tallies to rank 0, which adds them up
            qc_parts = parallel.gather_objects(dist, rank, world, eng.qc_read_tallies())
        if clips_on:                     # ... and the clip sites, summed on every rank; rank 0 uses them
            clip_tables = clips.from_wire(parallel.allreduce_numpy(dist, device, clips.to_wire(*eng.qc_clips_tables())), G)
        if final_trimmed_fn is not None and driver.part_writer is not None:
            # the ranks' files (all closed by now: the writer threads were joined in run()) become the one trimmed BAM
            parts = parallel.gather_objects(dist, rank, world, (driver.part_writer.path, driver.part_writer.header_bytes))
            if rank == 0:
                from . import bam_native
                bam_native.stitch_bam_parts(final_trimmed_fn, parts)
                for path, _ in parts:
                    os.remove(path)
                print_log("Trimmed reads of %d ranks joined: %s" % (world, final_trimmed_fn))

    failed = True
    try:
        qc_depth = qc_region_recs = None
        if qc_on and rank == 0:
            qc_tallies = qc.merge_read_tallies(qc_parts) if dist is not None else eng.qc_read_tallies()
            if clips_on and dist is None:
                clip_tables = eng.qc_clips_tables()
        if do_count:
            cp = calling.call_params(min_depth_consensus if min_depth_consensus is not None else 0,
                                     min_freq_consensus if min_freq_consensus is not None else 0,
                                     min_depth_variants if min_depth_variants is not None else 0,
                                     min_freq_variants if min_freq_variants is not None else 0,
                                     run_consensus, run_variants)
            eng.set_reference(ref_seq)
            if dist is not None:
                eng.sync()
                parallel.allreduce_table(dist, table)      # the ONE collective of the run: every rank now holds the job's table
            if qc_on and rank == 0:                        # depth from the job's table
                qc_depth, qc_region_recs = eng.qc_depth(want_depth=qc_depth_fn is not None or clips_on)      # (a junction's flank depths)
            for r in on:                                   # one more all-reduce or gather per report, in the same order on every rank
                r.collect(run, eng)

            def ins_tallies(positions):
                triples = loop.ins_store.counted_pairs(positions)
                if dist is not None:                       # all ranks flag the same positions (same table): symmetric exchange
                    triples = parallel.allgather_relevant_events(dist, world, triples)
                return calling.tallies_from_runs(triples, positions)
            res = calling.call(eng, ref_seq, cp, ins_tallies)
            if rank != 0:
                run_variants = run_consensus = False       # rank 0 writes the outputs
            if run_variants:
                vcf.f.write(res.vcf_text(vcf.ref_id, **{r.name: r.vcf_tables(run) for r in on}))      # (= vcf.write(r) for r in res.records)
                vcf.close()
            for r in on:
                if r.with_calls:
                    r.write(run, res)
            if run_consensus:
                f = gzip.open(consensus_fn, "wt") if consensus_fn.lower().endswith(".gz") else open(consensus_fn, "w")
                f.write(">sample\n%s\n" % res.consensus_string(unknown_symbol))
                f.close()
            for r in on:                                   # (a report is on only in a run with a count table)
                if not r.with_calls:
                    r.write(run, res)
        if clips_on and rank == 0:
            clip_sites = clips.find_sites(clip_tables[0], ref_seq, qc_clip_reads)
            clip_junctions = clips.find_junctions(clip_sites, G, qc_depth)
        if qc_on and rank == 0:
            if qc_fn is not None:
                report = qc.build_report(
                    dict(primer_pos_offset=primer_pos_offset or 0, min_length=min_length, include_no_primer=bool(include_no_primer), depths=qc_depths)
                    if run_trim else dict(depths=qc_depths),
                    qc_tallies[0], run_trim, qc_primers, qc_tallies[1], qc_tallies[2],
                    [name for _, _, name in qc_regions], qc_region_recs, qc_depths)
                for r in on:
                    r.add_to_qc(report)
                if qc_clips:
                    report["clips"] = clips.section(qc_clip_min, qc_clip_reads, clip_tables[1], clip_sites, clip_junctions)
                qc.write_json(qc_files[0], report)
                print_log("Output QC report: %s" % qc_fn)
                print_log(qc.summary_line(report))
            if qc_depth_fn is not None:
                qc.write_depth(qc_files[1], ref_id, qc_depth)
            if qc_clip_fn is not None:
                clips.write_sites(qc_files[2], ref_id, clip_sites)
            if qc_junction_fn is not None:
                clips.write_junctions(qc_files[3], ref_id, clip_junctions)
            if clips_on:
                print_log("Clip sites: %d with at least %d reads, %d junctions" % (len(clip_sites), qc_clip_reads, len(clip_junctions)))
        for r in on:
            r.summary(run)
        for r in on:
            r.after(run)
        failed = False
    finally:
        for f in qc_files + [f for r in on for f in r.files()]:
            if f is not None:
                f.close()
        driver.finish(failed)             # (the writer thread of the libampbam path, which ran on under the calls)
    eng.close()
    parallel.finish(dist)
    s_i = loop.s_i
    if s_i is None:
        if dist is None or world == 1:
            raise NameError("name 's_i' is not defined")       # the reference's behaviour on an empty input (:963)
        s_i = -1                                               # (a rank whose share is empty: more ranks than pieces of the file)
    print_log("Finished Processing %d reads" % s_i)


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        argv.append("-h")
    D = DEFAULTS
    fmt = argparse.ArgumentDefaultsHelpFormatter
    parser = argparse.ArgumentParser(description="amplipy_amd: AmpliPy's toolkit surface on MI355X", formatter_class=fmt)
    sub = parser.add_subparsers(dest="command")

    def trim_args(p):
        p.add_argument("-p", "--primer", required=True, type=str, help="Primer File (BED)")
        p.add_argument("-r", "--reference", required=True, type=str, help="Reference Genome (FASTA)")

    t = sub.add_parser("trim", formatter_class=fmt)
    t.add_argument("-i", "--input", required=False, type=str, default="stdin", help="Untrimmed Reads (SAM/BAM)")
    trim_args(t)
    t.add_argument("-o", "--output", required=False, type=str, default="stdout", help="Trimmed Reads (SAM/BAM)")
    t.add_argument("-x", "--primer_pos_offset", required=False, type=int, default=D["primer_pos_offset"], help="Primer position offset")
    t.add_argument("-ml", "--min_length", required=False, type=int, default=D["min_length"], help="Minimum length of read to retain after trimming")
    t.add_argument("-mq", "--min_quality", required=False, type=int, default=D["min_quality"], help="Minimum quality threshold")
    t.add_argument("-s", "--sliding_window_width", required=False, type=int, default=D["sliding_window_width"], help="Width of sliding window")
    t.add_argument("-e", "--include_no_primer", action="store_true", help="Include reads with no primers")

    v = sub.add_parser("variants", formatter_class=fmt)
    v.add_argument("-i", "--input", required=False, type=str, default="stdin", help="Trimmed Reads (SAM/BAM)")
    v.add_argument("-r", "--reference", required=True, type=str, help="Reference Genome (FASTA)")
    v.add_argument("-o", "--output", required=False, type=str, default="stdout", help="Variant Calls (VCF)")
    v.add_argument("-mq", "--min_quality", required=False, type=int, default=D["min_quality"], help="Minimum quality threshold")
    v.add_argument("-mf", "--min_freq", required=False, type=float, default=D["min_freq_variants"], help="Minimum frequency threshold (0-1) to call variant")
    v.add_argument("-md", "--min_depth", required=False, type=int, default=D["min_depth_variants"], help="Minimum depth to call variant")

    c = sub.add_parser("consensus", formatter_class=fmt)
    c.add_argument("-i", "--input", required=False, type=str, default="stdin", help="Trimmed Reads (SAM/BAM)")
    c.add_argument("-r", "--reference", required=True, type=str, help="Reference Genome (FASTA)")
    c.add_argument("-o", "--output", required=False, type=str, default="stdout", help="Consensus Sequence (FASTA)")
    c.add_argument("-mq", "--min_quality", required=False, type=int, default=D["min_quality"], help="Minimum quality threshold")
    c.add_argument("-mf", "--min_freq", required=False, type=float, default=D["min_freq_consensus"], help="Minimum frequency threshold (0-1) to call consensus")
    c.add_argument("-md", "--min_depth", required=False, type=int, default=D["min_depth_consensus"], help="Minimum depth to call consensus")
    c.add_argument("-n", "--unknown_symbol", required=False, type=str, default=D["unknown_symbol"], help="Character to print in regions with less than minimum coverage")

    a = sub.add_parser("aio", formatter_class=fmt)
    a.add_argument("-i", "--input", required=False, type=str, default="stdin", help="Untrimmed Reads (SAM/BAM)")
    trim_args(a)
    a.add_argument("-ot", "--output_trimmed_reads", required=True, type=str, help="Trimmed Reads (SAM/BAM)")
    a.add_argument("-ov", "--output_variants", required=True, type=str, help="Variant Calls (VCF)")
    a.add_argument("-oc", "--output_consensus", required=True, type=str, help="Consensus Sequence (FASTA)")
    a.add_argument("-x", "--primer_pos_offset", required=False, type=int, default=D["primer_pos_offset"], help="Primer position offset")
    a.add_argument("-ml", "--min_length", required=False, type=int, default=D["min_length"], help="Minimum length of read to retain after trimming")
    a.add_argument("-mq", "--min_quality", required=False, type=int, default=D["min_quality"], help="Minimum quality threshold")
    a.add_argument("-s", "--sliding_window_width", required=False, type=int, default=D["sliding_window_width"], help="Width of sliding window")
    a.add_argument("-mfc", "--min_freq_consensus", required=False, type=float, default=D["min_freq_consensus"], help="Minimum frequency threshold (0-1) to call consensus")
    a.add_argument("-mfv", "--min_freq_variants", required=False, type=float, default=D["min_freq_variants"], help="Minimum frequency threshold (0-1) to call variant")
    a.add_argument("-mdc", "--min_depth_consensus", required=False, type=int, default=D["min_depth_consensus"], help="Minimum depth to call consensus")
    a.add_argument("-mdv", "--min_depth_variants", required=False, type=int, default=D["min_depth_variants"], help="Minimum depth to call variant")
    a.add_argument("-n", "--unknown_symbol", required=False, type=str, default=D["unknown_symbol"], help="Character to print in regions with less than minimum coverage")
    a.add_argument("-e", "--include_no_primer", action="store_true", help="Include reads with no primers")
    for p in (t, v, c, a):
        p.add_argument("--qc", required=False, type=str, default=None, help="Amplicon QC report (JSON): reads per primer, reads kept and dropped, depth per region")
        p.add_argument("--qc_regions", required=False, type=str, default=None, help="Further regions of the QC report (BED: ref, start, end, name); needs --qc")
        p.add_argument("--qc_depths", required=False, type=str, default=None, help="Depth thresholds of the QC report, at most 4 (1,10,100 when omitted); needs --qc")
        p.add_argument("--qc_depth_out", required=False, type=str, default=None, help="Depth of every position (TSV or TSV.gz: ref, position, depth)")
        p.add_argument("--qc_clips", action="store_true", help="The QC report gains the section \"clips\": soft-clip sites and the junctions they place, deletions and duplications the aligner clipped instead of opening a gap; needs --qc")
        p.add_argument("--qc_clip_out", required=False, type=str, default=None, help="Every soft-clip site with at least --qc_clip_reads reads: position, side, reads, reverse reads, consensus of the clipped bases, class, partner (TSV or TSV.gz)")
        p.add_argument("--qc_junction_out", required=False, type=str, default=None, help="Junctions placed from soft-clip sites: kind, start, end, length, reads and reverse reads of either side, depth of the flanks (TSV or TSV.gz)")
        p.add_argument("--qc_clip_min", required=False, type=int, default=None, help="Clipped bases a read needs at a site, 1 to 64 (10 when omitted); needs --qc_clips, --qc_clip_out or --qc_junction_out")
        p.add_argument("--qc_clip_reads", required=False, type=int, default=None, help="Reads a site needs to be written (2 when omitted); needs --qc_clips, --qc_clip_out or --qc_junction_out")
        p.add_argument("--strand", action="store_true", help="VCF records also carry REF_RV, ALT_RV, REF_QUAL, ALT_QUAL and SB: reverse-strand depth, mean base quality and strand bias per allele (variants, aio)")
        p.add_argument("--amplicons", required=False, type=str, default=None, help="Amplicon file (TSV: left primer, right primer[, amplicon name]): per-amplicon allele counts on the device, and AMP, AMP_DP, AMP_REF_DP, AMP_ALT_DP, AMP_NA_DP, AMP_P and PRIMER on every VCF record (aio)")
        p.add_argument("--amplicon_out", required=False, type=str, default=None, help="Count of every symbol per amplicon and position of its span (TSV or TSV.gz; aio, needs --amplicons)")
        p.add_argument("--codons", required=False, type=str, default=None, help="CDS file (TSV: name, start, end[, strand]; 0-based, half-open): codon tallies within single reads on the device, and CDS, CODON_DP, ALT_AA, ALT_CODON and ALT_CODON_DP on every VCF record (variants, consensus, aio)")
        p.add_argument("--codon_out", required=False, type=str, default=None, help="Count of every codon seen on single reads, per CDS row and codon (TSV or TSV.gz; needs --codons)")
        p.add_argument("--aa_out", required=False, type=str, default=None, help="Amino-acid changes at or above the variant thresholds, per CDS row and codon (TSV or TSV.gz; variants, aio; needs --codons)")
        p.add_argument("--deletions", action="store_true", help="Deletions tallied as whole events on the device; VCF records also carry DEL_N and DEL: the events that cover the position (variants, aio)")
        p.add_argument("--del_out", required=False, type=str, default=None, help="Every deletion event: start, length, reads, reverse reads, depth, frequency, deleted text (TSV or TSV.gz; variants, consensus, aio)")
        p.add_argument("--indel_vcf", required=False, type=str, default=None, help="A second VCF of anchored indels: deletion events and insertion alleles at or above the variant thresholds (VCF or VCF.gz; variants, aio)")
        p.add_argument("--del_capacity", required=False, type=int, default=None, help="log2 of the slots of the deletion events' table on the device, 4 to 28 (20 when omitted)")
        p.add_argument("--insertions", action="store_true", help="Insertion alleles tallied with their evidence on the device; VCF records also carry INS_N and INS: the alleles anchored at the position with reads, reverse reads, mean base quality and reads near a read end; the insertion rows of --indel_vcf carry RV (variants, aio)")
        p.add_argument("--ins_out", required=False, type=str, default=None, help="Every insertion allele: position, allele, reads, reverse reads, reads without qualities, mean base quality, seven distance-to-end bins, depth, frequency (TSV or TSV.gz; variants, consensus, aio)")
        p.add_argument("--ins_capacity", required=False, type=int, default=None, help="log2 of the slots of the insertion evidence table on the device, 4 to 28 (20 when omitted)")
        p.add_argument("--ins_end", required=False, type=int, default=None, help="Distance below which an insertion allele counts as at a read end in INS: one of 2, 4, 8, 16, 32, 64 (8 when omitted); needs --insertions or --ins_out")
        p.add_argument("--cooc", required=False, type=str, default=None, help="Mutation-set file (TSV: name, comma-separated mutations such as A23403G, del21765-21770, del21991; positions 1-BASED as in the VCF, unlike --codons): per set, the reads that carry its mutations together, tallied on the device, and COOC on every VCF record (variants, consensus, aio)")
        p.add_argument("--cooc_out", required=False, type=str, default=None, help="Reads per mutation set and pattern of mutations carried (TSV or TSV.gz; needs --cooc)")
        p.add_argument("--error_profile", required=False, type=str, default=None, help="Error profile (JSON): how often a base differs from the reference by sequencing cycle, by reported quality and by substitution class, tallied on the device over every match base; ERR_RATE and ERR_P on every VCF record. Without --error_mask the site's own bases are part of the rate (variants, consensus, aio)")
        p.add_argument("--error_mask", required=False, type=str, default=None, help="Positions that take no part in the error profile, the known or called variants: a .vcf / .vcf.gz (every record masks its REF span) or a BED (columns 2 and 3; .gz allowed); needs --error_profile")
        p.add_argument("--haplotypes", required=False, type=str, default=None, help="Region file (BED: ref, start, end, name; 0-based, half-open; 1 to 4096 positions a region): per region, the distinct sets of substitutions and deletions single reads carry over the whole region, tallied on the device, and HAP_N and HAP on every VCF record; insertions are not part of a haplotype (variants, consensus, aio)")
        p.add_argument("--hap_out", required=False, type=str, default=None, help="Reads per region and haplotype, mutations 1-BASED in the grammar of --cooc (TSV or TSV.gz; needs --haplotypes)")
        p.add_argument("--hap_min_reads", required=False, type=int, default=2, help="A haplotype below this many reads is not written")
        p.add_argument("--hap_min_freq", required=False, type=float, default=0.0, help="A haplotype below this share of the region's usable reads is not written")
        p.add_argument("--hap_capacity", required=False, type=int, default=None, help="log2 of the slots of the haplotype table on the device, 4 to 28 (20 when omitted)")
        p.add_argument("--readpos", action="store_true", help="VCF records also carry REF_RP, ALT_RP, REF_END, ALT_END, RPB and RPZ: where on its reads an allele sits, by distance to the nearer end of the read's kept bases (seven bins), with a Fisher p-value and a rank-sum z against the reference base (variants, aio)")
        p.add_argument("--readpos_end", required=False, type=int, default=None, help="Distance below which a base counts as at a read end for REF_END, ALT_END and RPB: one of the bin edges 2, 4, 8, 16, 32, 64 (8 when omitted); needs --readpos")
        p.add_argument("--readpos_out", required=False, type=str, default=None, help="The seven distance-to-end bins of every position and symbol (TSV or TSV.gz; variants, consensus, aio)")
        p.add_argument("--strand_out", required=False, type=str, default=None, help="Count, reverse-strand count and quality sum of every position and symbol (TSV or TSV.gz; variants, consensus, aio)")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.qc is None and (args.qc_regions is not None or args.qc_depths is not None):
        error("--qc_regions and --qc_depths need --qc")
    if args.qc_clips and args.qc is None:
        error("--qc_clips needs --qc")
    if (args.qc_clip_min is not None or args.qc_clip_reads is not None) and not (args.qc_clips or args.qc_clip_out is not None or args.qc_junction_out is not None):
        error("--qc_clip_min and --qc_clip_reads need --qc_clips, --qc_clip_out or --qc_junction_out")
    qc_args = dict(qc_clips=args.qc_clips, qc_clip_fn=args.qc_clip_out, qc_junction_fn=args.qc_junction_out, qc_clip_min=args.qc_clip_min,
                   qc_clip_reads=args.qc_clip_reads)
    qc_args.update(qc_fn=args.qc, qc_regions_fn=args.qc_regions, qc_depth_fn=args.qc_depth_out,
                   qc_depths=qc.parse_depths(args.qc_depths) if args.qc_depths is not None else None)
    qc_args.update(strand=args.strand, strand_fn=args.strand_out, amplicons_fn=args.amplicons, amplicon_out_fn=args.amplicon_out,
                   codons_fn=args.codons, codon_out_fn=args.codon_out, aa_out_fn=args.aa_out, deletions=args.deletions,
                   del_out_fn=args.del_out, indel_vcf_fn=args.indel_vcf, del_capacity=args.del_capacity, cooc_fn=args.cooc, cooc_out_fn=args.cooc_out,
                   error_profile_fn=args.error_profile, error_mask_fn=args.error_mask, haplotypes_fn=args.haplotypes, hap_out_fn=args.hap_out,
                   hap_min_reads=args.hap_min_reads, hap_min_freq=args.hap_min_freq, hap_capacity=args.hap_capacity,
                   readpos=args.readpos, readpos_end=args.readpos_end, readpos_fn=args.readpos_out, insertions=args.insertions,
                   ins_out_fn=args.ins_out, ins_capacity=args.ins_capacity, ins_end=args.ins_end)
    if args.command == "trim":
        run_amplipy(untrimmed_reads_fn=args.input, primer_fn=args.primer, reference_fn=args.reference,
                    trimmed_reads_fn=args.output, primer_pos_offset=args.primer_pos_offset, min_length=args.min_length,
                    min_quality=args.min_quality, sliding_window_width=args.sliding_window_width,
                    include_no_primer=args.include_no_primer, run_trim=True, **qc_args)
    elif args.command == "variants":
        run_amplipy(trimmed_reads_fn=args.input, reference_fn=args.reference, variants_fn=args.output,
                    min_quality=args.min_quality, min_freq_variants=args.min_freq, min_depth_variants=args.min_depth,
                    run_variants=True, **qc_args)
    elif args.command == "consensus":
        run_amplipy(trimmed_reads_fn=args.input, reference_fn=args.reference, consensus_fn=args.output,
                    min_quality=args.min_quality, min_freq_consensus=args.min_freq, min_depth_consensus=args.min_depth,
                    unknown_symbol=args.unknown_symbol, run_consensus=True, **qc_args)
    elif args.command == "aio":
        run_amplipy(untrimmed_reads_fn=args.input, primer_fn=args.primer, reference_fn=args.reference,
                    trimmed_reads_fn=args.output_trimmed_reads, variants_fn=args.output_variants,
                    consensus_fn=args.output_consensus, primer_pos_offset=args.primer_pos_offset,
                    min_length=args.min_length, min_quality=args.min_quality,
                    sliding_window_width=args.sliding_window_width, min_freq_consensus=args.min_freq_consensus,
                    min_freq_variants=args.min_freq_variants, min_depth_consensus=args.min_depth_consensus,
                    min_depth_variants=args.min_depth_variants, unknown_symbol=args.unknown_symbol,
                    include_no_primer=args.include_no_primer, run_trim=True, run_variants=True, run_consensus=True, **qc_args)


if __name__ == "__main__":
    main()
