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
from datetime import datetime
from os.path import isfile

import numpy as np

from . import AMPLIPY_VERSION, abi, bamio, calling, lib, parallel
from .batch import ReadBatch
from .insertions import EventStore

VERSION = AMPLIPY_VERSION
PROGRESS_NUM_READS = 50000          # AmpliPy.py:19
BATCH_READS = 1 << 18              # reads per device batch on the Python-codec path (one Rec object each)
NATIVE_BATCH_READS = 1 << 18       # records per device batch on the libampbam path (the writer overlaps the next batch)

DEFAULTS = dict(min_depth_consensus=10, min_depth_variants=1, min_freq_consensus=0, min_freq_variants=0.03,
                min_length=30, min_quality=20, primer_pos_offset=0, sliding_window_width=4, unknown_symbol="N")


def print_log(s="", end="\n"):
    print("[%s] %s" % (datetime.now().strftime("%Y-%m-%d %H:%M:%S"), s), end=end, file=sys.stderr)
    sys.stderr.flush()


def error(s=None):
    print_log("ERROR" if s is None else "ERROR: %s" % s)
    sys.exit(1)


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


# ---- output openers (AmpliPy.py:261-360) --------------------------------------------------------
def _reads_mode(fn, write):
    low = fn.lower()
    if low.endswith(".sam"):
        return "w" if write else "r"
    if low.endswith(".bam"):
        return "wb" if write else "rb"
    error("Invalid read mapping extension (should be .sam or .bam): %s" % fn)


def open_alignment_files(input_fn, output_fn):
    if input_fn is None:
        error("Input alignment file is None")
    if input_fn.lower() == "stdin":
        reader = bamio.AlignmentReader("-", "r")
    elif not isfile(input_fn):
        error("File not found: %s" % input_fn)
    else:
        reader = bamio.AlignmentReader(input_fn, _reads_mode(input_fn, False))
    writer = None
    if output_fn is not None:
        hdr = reader.header.with_amplipy_pg(VERSION, " ".join(sys.argv))
        if output_fn.lower() == "stdout":
            writer = bamio.AlignmentWriter("-", "w", hdr)
        elif isfile(output_fn):
            error("File already exists: %s" % output_fn)
        else:
            writer = bamio.AlignmentWriter(output_fn, _reads_mode(output_fn, True), hdr)
    return reader, writer


NATIVE_PART_BYTES = 4 << 20        # compressed bytes of a piece of the input BAM (pieces are inflated one ahead of the GPU); on the
                                   # 11.6 MB / 1.5 M-read file of the bench: 16 MB (one piece) aio 10.5 M reads/s, 4 MB 12.4, 1 MB 12.4


def native_parts(input_fn, rank=0, world=1, part_bytes=None):
    """How a BAM file is cut for this rank: (n_parts, k_lo, k_hi) -- the file has n_parts pieces of about ``part_bytes``
    compressed bytes (ampbam_open_range: cut at BGZF block starts, i.e. by base count for a sorted BAM), of which the rank
    takes the contiguous run [k_lo, k_hi).  Every rank gets the same number of pieces (n_parts is a multiple of world)."""
    part_bytes = part_bytes or int(os.environ.get("AMPLIPY_PART_BYTES", NATIVE_PART_BYTES))
    size = os.path.getsize(input_fn)
    per_rank = max(1, -(-size // (part_bytes * world)))
    return per_rank * world, per_rank * rank, per_rank * (rank + 1)


def open_native_bam(input_fn, output_fn, rank=0, world=1, device=0):
    """(NativeInput, BamWriter or None) when the native codec can serve this run: BAM file in, and BAM file
    (or nothing) out.  None otherwise (SAM text, stdin / stdout): the Python codec handles those.
    Same checks and messages as open_alignment_files."""
    if input_fn is None or input_fn.lower() == "stdin" or not isfile(input_fn) or _reads_mode(input_fn, False) != "rb":
        return None
    if output_fn is not None and (output_fn.lower() == "stdout" or isfile(output_fn) or _reads_mode(output_fn, True) != "wb"):
        return None
    if os.environ.get("AMPLIPY_PYTHON_BAM"):
        return None
    src = NativeInput(input_fn, rank, world)
    writer = None
    if output_fn is not None:
        from . import bam_native
        first = src.first_part()
        hdr = bamio.Header(first.header_text, first.references).with_amplipy_pg(VERSION, " ".join(sys.argv))
        # zlib's default level like htslib; AMPLIPY_BAM_LEVEL=1 trades file size for speed; AMPLIPY_GPU_DEFLATE=1 hands the blocks'
        # DEFLATE streams to the HIP encoder on this rank's device
        writer = bam_native.BamWriter(output_fn, hdr.text, first, level=int(os.environ.get("AMPLIPY_BAM_LEVEL", "-1")),
                                      gpu_deflate=os.environ.get("AMPLIPY_GPU_DEFLATE", "0") not in ("", "0"), device=device)
    return src, writer


class NativeInput:
    """The rank's share of a BAM file as a sequence of pieces (bam_native.BamFile of ampbam_open_range), each inflated and
    indexed on a helper thread while the piece before it is on the GPU (AmpliPy.py:896 streams its input; here at most two
    pieces are in memory).  Pieces must meet: each starts where the one before ended (checked; ranks check their seams with
    each other through ``seam``)."""

    def __init__(self, path, rank=0, world=1):
        self.path = path
        self.n_parts, self.k_lo, self.k_hi = native_parts(path, rank, world)
        self._first = None
        self._ahead = None          # (thread, box) of the piece being opened

    def _open(self, k, first_hint=None):
        from . import bam_native
        return bam_native.BamFile(self.path, part=k, n_parts=self.n_parts, first_hint=first_hint)

    def first_part(self):
        if self._first is None:
            self._first = self._open(self.k_lo)
        return self._first

    def _start(self, k, first_hint):
        import threading
        box = {}

        def run():
            try:
                box["file"] = self._open(k, first_hint)
            except Exception as e:           # surfaced by the consumer
                box["error"] = e
        t = threading.Thread(target=run, daemon=True)
        t.start()
        self._ahead = (t, box)

    def close(self):
        """Lets go of what an abandoned walk still holds: the piece that was being opened ahead, the first piece if it was never
        yielded."""
        if self._ahead is not None:
            t, box = self._ahead
            t.join()
            if box.get("file") is not None:
                box["file"].close()
            self._ahead = None
        if self._first is not None:
            self._first.close()
            self._first = None

    def __iter__(self):
        """Yields the pieces in order; the caller closes each when it is done with it.  seam = (first, end) of the whole
        share is available afterwards."""
        prev_end = None
        self.seam = [None, None]
        cur = self.first_part()
        self._first = None
        for k in range(self.k_lo, self.k_hi):
            # the piece behind this one starts where this one ends: it is told so, and only the rank's FIRST piece (whose
            # predecessor another rank reads) is found by the codec's chain-of-plausible-records search
            a, b = cur.part_range()
            if k + 1 < self.k_hi:
                exact = cur.n_records > 0 or k > self.k_lo or self.k_lo == 0      # (a guessed piece without records does not know where it ends)
                self._start(k + 1, b if exact else None)
            if cur.n_records:
                if prev_end is not None and a != prev_end:
                    raise bam_native_error("%s: piece %d of %d starts at inflated offset %d, the piece before it ended at %d"
                                           % (self.path, k, self.n_parts, a, prev_end))
                if self.seam[0] is None:
                    self.seam[0] = a
                self.seam[1] = prev_end = b
            yield cur
            if k + 1 < self.k_hi:
                t, box = self._ahead
                t.join()
                self._ahead = None
                if "error" in box:
                    raise box["error"]
                cur = box["file"]


def bam_native_error(msg):
    from . import bam_native
    return bam_native.AmpBamError(msg)


def gpu_codec_wanted(arg, env_name):
    """The opt-in switch of a device codec: the argument of run_amplipy when it is given, else the variable set to anything but 0."""
    return bool(arg) if arg is not None else os.environ.get(env_name, "0") not in ("", "0")


def gpu_sam_wanted(gpu_sam=None):
    """The device codec for SAM text: run_amplipy(gpu_sam=...) or AMPLIPY_GPU_SAM=1."""
    return gpu_codec_wanted(gpu_sam, "AMPLIPY_GPU_SAM")


def gpu_bam_wanted(gpu_bam=None):
    """The device codec for BAM input: run_amplipy(gpu_bam=...) or AMPLIPY_GPU_BAM=1."""
    return gpu_codec_wanted(gpu_bam, "AMPLIPY_GPU_BAM")


def open_device_bam(input_fn):
    """A bam_device.DeviceBamInput when the device codec for BAM input can serve this run: an existing BAM
    file in, no trimmed reads out.  None otherwise -- under the conditions open_native_bam serves: whatever else the input is,
    the other codecs handle (and refuse) it as before."""
    if input_fn is None or input_fn.lower() == "stdin" or not isfile(input_fn) or _reads_mode(input_fn, False) != "rb":
        return None
    if os.environ.get("AMPLIPY_PYTHON_BAM"):
        return None
    return input_fn


def open_device_bam_write(input_fn, output_fn):
    """(bam_device.DeviceBamInput, bam_device.DeviceBamOutput) when the device codec can serve a run that writes trimmed reads
    (DESIGN.md section 12): an existing BAM file in and a new BAM file out, the conditions under which open_native_bam opens a
    writer.  None otherwise: the host codec serves the run as before."""
    if open_device_bam(input_fn) is None:
        return None
    if output_fn is None or output_fn.lower() == "stdout" or isfile(output_fn) or _reads_mode(output_fn, True) != "wb":
        return None
    from . import bam_device
    src = bam_device.DeviceBamInput(input_fn)
    hdr = bamio.Header(src.header_text, src.references).with_amplipy_pg(VERSION, " ".join(sys.argv))
    return src, bam_device.DeviceBamOutput(output_fn, hdr.text, src.references, level=int(os.environ.get("AMPLIPY_BAM_LEVEL", "-1")))


def open_device_bam_text(input_fn, output_fn):
    """(bam_device.DeviceBamInput, AlignmentWriter, binary output) when the device codec for BAM input can write this run's trimmed
    reads as SAM text: an existing BAM file in, under the conditions of open_device_bam, and stdout or a new
    .sam file out; a header of plain ASCII text whose @SQ names fit the device's name table (the test open_native_sam applies).
    None otherwise: the other codecs serve (and refuse) the run as before, with their own messages.  The header goes out through
    the text layer as in open_native_sam; the writer is the Python codec's, for the pieces the device hands back."""
    import io
    if open_device_bam(input_fn) is None or output_fn is None:
        return None
    to_stdout = output_fn.lower() == "stdout"
    if to_stdout and not hasattr(sys.stdout, "buffer"):
        return None
    if not to_stdout and (isfile(output_fn) or not output_fn.lower().endswith(".sam")):
        return None
    from . import bam_device, bam_native
    try:
        src = bam_device.DeviceBamInput(input_fn)
    except bam_native.AmpBamError:
        return None                       # (not a BAM file the host codec's block walk takes: the Python codec says what it finds)
    names = [n for n, _ in src.references]
    if not all(ord(c) < 128 for c in src.header_text) or len(names) > bam_device.MAX_REFS or sum(len(n) for n in names) > bam_device.MAX_REF_BYTES \
            or not all(n not in ("", "*", "=") and all(33 <= ord(c) < 127 for c in n) for n in names):
        return None
    out_hdr = bamio.Header(src.header_text, src.references).with_amplipy_pg(VERSION, " ".join(sys.argv))
    if to_stdout:
        outt, outb = sys.stdout, sys.stdout.buffer
    else:
        outb = open(output_fn, "wb")
        outt = io.TextIOWrapper(outb, write_through=True)       # (what open(output_fn, "w") is made of)
    writer = bamio.AlignmentWriter(None, "w", out_hdr, fileobj=outt)
    outt.flush()
    return src, writer, outb


def open_native_sam(input_fn, output_fn, bam_write=False):
    """(SamTextInput, Header, AlignmentWriter or None, binary output or None, device_ok, DeviceBamOutput or None) when the device
    codec for SAM text can serve this run (sam_native): stdin or an existing .sam file in, and stdout, a new
    .sam file or nothing out -- or, with bam_write (both switches on, section 13), a new .bam file, whose header blocks and
    end-of-file block a bam_device.DeviceBamOutput writes.
    None otherwise: the Python codec handles those.  Same checks and messages as open_alignment_files (what it would refuse
    is left to it).  device_ok False: the header is one the device's name table cannot take (more than 64 @SQ lines, a name
    that is not plain text) -- every chunk of the run then goes through the Python codec, and a BAM output through its
    writer, as with the switches off."""
    import io
    from . import sam_native
    if input_fn is None:
        return None
    from_stdin = input_fn.lower() == "stdin"
    if from_stdin:
        if not hasattr(sys.stdin, "buffer"):
            return None
    elif not isfile(input_fn) or _reads_mode(input_fn, False) != "r":
        return None
    to_stdout = output_fn is not None and output_fn.lower() == "stdout"
    if to_stdout and not hasattr(sys.stdout, "buffer"):
        return None
    to_bam = bool(bam_write) and output_fn is not None and not to_stdout and not isfile(output_fn) and output_fn.lower().endswith(".bam")
    if output_fn is not None and not to_stdout and not to_bam and (isfile(output_fn) or not output_fn.lower().endswith(".sam")):
        return None
    src = sam_native.SamTextInput("-" if from_stdin else input_fn)
    text = src.header_text()
    hdr = bamio.Header(text, bamio._refs_from_text(text))
    names = [n for n, _ in hdr.refs]
    device_ok = src.header_is_plain() and len(names) <= sam_native.MAX_REFS and sum(len(n) for n in names) <= sam_native.MAX_REF_BYTES \
        and all(n not in ("", "*", "=") and all(33 <= ord(c) < 127 for c in n) for n in names)
    writer = outb = bam_out = None
    if output_fn is not None:
        out_hdr = hdr.with_amplipy_pg(VERSION, " ".join(sys.argv))
        if to_bam and device_ok:
            from . import bam_device
            bam_out = bam_device.DeviceBamOutput(output_fn, out_hdr.text, hdr.refs, level=int(os.environ.get("AMPLIPY_BAM_LEVEL", "-1")))
        elif to_bam:
            writer = bamio.AlignmentWriter(output_fn, "wb", out_hdr)
        elif to_stdout:
            outt, outb = sys.stdout, sys.stdout.buffer
        else:
            outb = open(output_fn, "wb")
            outt = io.TextIOWrapper(outb, write_through=True)       # (what open(output_fn, "w") is made of)
        if outb is not None:
            writer = bamio.AlignmentWriter(None, "w", out_hdr, fileobj=outt)
            outt.flush()
    return src, hdr, writer, outb, device_ok, bam_out


class VcfWriter:
    """Text VCF with the header AmpliPy builds through pysam (AmpliPy.py:271-281)."""

    def __init__(self, fn, ref_id):
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
        w("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")

    def line(self, r):
        return "%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;REF_DP=%d;ALT_DP=%s;REF_FREQ=%g;ALT_FREQ=%s\tGT\t%s\n" % (
            self.ref_id, r.pos + 1, r.ref, ",".join(r.alts), r.DP, r.REF_DP, r.ALT_DP, r.REF_FREQ, r.ALT_FREQ, "/".join(map(str, r.GT)))

    def write(self, r):
        self.f.write(self.line(r))

    def write_all(self, records):
        self.f.write("".join([self.line(r) for r in records]))

    def close(self):
        if self.f is not sys.stdout:
            self.f.close()


def _raise_for_status(status):
    exc = abi.READ_STATUS_EXC[int(status)]
    raise exc("read rejected by the engine: %s (the reference raises %s here)" % (abi.READ_STATUS_NAMES[int(status)], exc.__name__))


def _store_events(eng, ins_store, read_base, dev_reads=None):
    """A batch's insertion alleles (A:730-748) into the store: the device sorts the batch's events by (position, allele) and
    run-length encodes them (amp_aggregate_ins_events), the text of one representative per allele is gathered on
    the device from the copy of the batch that eng.process() left there (A:736-738; dev_reads: from that device batch instead),
    and the event list starts over."""
    runs = eng.aggregate_events(dev_reads=dev_reads, read_base=read_base, drain=True)
    if runs.size == 0:
        return
    rows = np.zeros(runs.size, abi.INS_EVENT_DTYPE)
    for f in ("ref_pos", "q_from", "q_to"):
        rows[f] = runs[f]
    rows["read"] = (runs["read"].astype(np.int64) - (read_base & 0xFFFFFFFF)) & 0xFFFFFFFF     # read ids are 32-bit, relative to read_base modulo 2^32
    length, blob = eng.event_text(rows, 0, dev_reads=dev_reads)
    ins_store.add_text(runs["ref_pos"], length, blob, runs["count"])


def run_amplipy(untrimmed_reads_fn=None, primer_fn=None, reference_fn=None, trimmed_reads_fn=None, variants_fn=None,
                consensus_fn=None, primer_pos_offset=None, min_length=None, min_quality=None, sliding_window_width=None,
                min_freq_consensus=None, min_freq_variants=None, min_depth_consensus=None, min_depth_variants=None,
                unknown_symbol=None, include_no_primer=None, run_trim=False, run_variants=False, run_consensus=False,
                device=None, gpu_sam=None, gpu_bam=None, gpu_bam_write=None):
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

    One process drives one GPU.  Under ``torchrun`` (WORLD_SIZE > 1, or AMPLIPY_FORCE_DIST=1 for a one-rank
    rehearsal) the job is range-partitioned: rank r takes the r-th contiguous run of BAM records (coordinate
    order), every rank's count table is summed with ONE all-reduce over RCCL (parallel.allreduce_table), the
    insertion alleles of the flagged positions are exchanged, and rank 0 writes the VCF / consensus.  A trimmed
    BAM is written per rank (``<name>.part<rank>.bam``; the parts concatenate to the single-GPU file's records).
    """
    dist, rank, world = parallel.init_from_env()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if dist is not None else 0
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
    mode = "Trim" if run_trim and not (run_variants or run_consensus) else \
        "Variants" if run_variants and not (run_trim or run_consensus) else \
        "Consensus" if run_consensus and not (run_trim or run_variants) else "All-In-One"
    print_log("Executing AmpliPy %s (v%s)" % (mode, VERSION))

    ref_id = ref_seq = None
    if reference_fn is not None:
        print_log("Loading reference genome: %s" % reference_fn)
        ref_id, ref_seq = load_ref_genome(reference_fn)
    G = len(ref_seq)
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
            if rank == 0 and trimmed_reads_fn.lower() != "stdout" and isfile(trimmed_reads_fn):
                error("File already exists: %s" % trimmed_reads_fn)
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
    native = reader = writer = vcf = sam = bamdev = bamdev_io = bamdev_text = None
    rank_error = None
    use_sam = dist is None and gpu_sam_wanted(gpu_sam)
    use_bam = dist is None and gpu_bam_wanted(gpu_bam)
    use_bam_write = use_bam and gpu_codec_wanted(gpu_bam_write, "AMPLIPY_GPU_BAM_WRITE")
    try:
        if run_trim:
            print_log("Input untrimmed SAM/BAM: %s" % untrimmed_reads_fn)
            print_log("Output trimmed SAM/BAM: %s" % trimmed_reads_fn)
            if use_bam_write:
                bamdev_io = open_device_bam_write(untrimmed_reads_fn, trimmed_reads_fn)
                bamdev = untrimmed_reads_fn if bamdev_io is not None else None
            if bamdev is None and use_bam and use_sam:
                bamdev_text = open_device_bam_text(untrimmed_reads_fn, trimmed_reads_fn)
                bamdev = untrimmed_reads_fn if bamdev_text is not None else None
            if bamdev is None:
                native = open_native_bam(untrimmed_reads_fn, trimmed_reads_fn, rank, world, device)
            if native is not None and use_bam:
                print_log("BAM device codec: this run writes trimmed reads, the host codec reads the input")
            if native is None and bamdev is None and use_sam:
                sam = open_native_sam(untrimmed_reads_fn, trimmed_reads_fn, bam_write=gpu_codec_wanted(gpu_bam_write, "AMPLIPY_GPU_BAM_WRITE"))
            if native is None and sam is None and bamdev is None:
                reader, writer = open_alignment_files(untrimmed_reads_fn, trimmed_reads_fn)
        else:
            print_log("Input trimmed SAM/BAM: %s" % trimmed_reads_fn)
            if use_bam:
                bamdev = open_device_bam(trimmed_reads_fn)
            if bamdev is None:
                native = open_native_bam(trimmed_reads_fn, None, rank, world)
            if native is None and bamdev is None and use_sam:
                sam = open_native_sam(trimmed_reads_fn, None)
            if native is None and sam is None and bamdev is None:
                reader, writer = open_alignment_files(trimmed_reads_fn, None)
        if variants_fn is not None and rank == 0:
            print_log("Output variants VCF: %s" % variants_fn)
            vcf = VcfWriter(variants_fn, ref_id)
    except (Exception, SystemExit) as e:
        if dist is None:
            raise
        rank_error = e if isinstance(e, Exception) else RuntimeError("could not open the run's files (exit status %s)" % (e.code,))
        native = None
    do_count = run_variants or run_consensus
    eng.set_params(min_quality if min_quality is not None else 20,
                   sliding_window_width if sliding_window_width is not None else 4, run_trim, do_count)

    print_log("Processing reads...")
    writer_pending = False      # the writer thread of the native BAM path is still running (joined behind the calls)
    ins_store = EventStore()             # insertion events with their allele text (each batch's bases are at hand only now)
    pending = []
    s_i = None
    read_base = 0

    def flush():
        nonlocal read_base
        if not pending:
            return
        batch = ReadBatch.from_segments([r.to_segment() for r in pending])
        res = eng.process(batch, read_base=read_base)
        bad = np.nonzero(res.status)[0]
        good_until = int(bad[0]) if len(bad) else len(pending)
        if run_trim and writer is not None:
            for k, r in enumerate(pending[:good_until]):
                fl = int(res.trim_flags[k])
                if int(res.ref_len[k]) >= min_length and ((fl & 3) or include_no_primer):      # AmpliPy.py:910
                    writer.write(r, pos=int(res.new_pos[k]), cigar=res.cigar_ops(k))
        if len(bad):                      # the reference dies on the first such read with an uncaught exception,
            _raise_for_status(res.status[bad[0]])      # having written every read in front of it (A:907-911)
        if do_count:
            # this batch's events only: the list is drained batch by batch (read ids are 32-bit and relative to
            # read_base modulo 2^32, which a batch never spans)
            _store_events(eng, ins_store, read_base)
        read_base += batch.n
        del pending[:]

    n_seen = 0                           # records this rank has gone through (all of them when there is one rank)
    n_bases = 0                          # ... and their bases (the measure the shares of a multi-rank run should be equal in: SURVEY 8e)

    def progress(count):
        """The progress lines of the next ``count`` records."""
        for k_ in range(n_seen + (-n_seen) % PROGRESS_NUM_READS, n_seen + count, PROGRESS_NUM_READS):
            if k_:
                print_log("Processed %d reads..." % k_)

    def python_records(recs):
        """Records a device codec handed back, through the Python codec: the loop of the last branch below on them (the skip of
        A:902, the progress lines, batches through flush())."""
        nonlocal n_seen, s_i
        for rec in recs:
            s_i = n_seen
            n_seen += 1
            if s_i % PROGRESS_NUM_READS == 0 and s_i != 0:
                print_log("Processed %d reads..." % s_i)
            if (rec.flag & 4) or rec.cigar is None:            # AmpliPy.py:902
                continue
            pending.append(rec)
            if len(pending) >= BATCH_READS:
                flush()
        flush()

    def device_piece(codec, info, emit=None, defer=False):
        """A piece or chunk whose batch a device codec has built (info: n_records, n_rows, n_bases): counted, through the read pass
        where it lies, ``emit`` run on its results, its events stored.  defer: the read pass is only enqueued, ``emit`` works from
        the verdict where it lies and brings it down with its own wait (sam_native.SamCodec.encode)."""
        nonlocal n_seen, s_i, n_bases, read_base
        count = int(info.n_records)
        progress(count)
        n_seen += count
        if count:
            s_i = n_seen - 1
        if info.n_rows == 0:
            return
        n_bases += int(info.n_bases)
        if defer:
            codec.process(read_base, defer=True)
            emit()
            bad_row, bad_status = codec.verdict()
        else:
            bad_row, bad_status = codec.process(read_base)
            if emit is not None:
                emit()
        if bad_row >= 0:                  # the rows in front of it are written (A:907-911)
            _raise_for_status(bad_status)
        if do_count:
            _store_events(eng, ins_store, read_base, dev_reads=codec.dev_reads())
        read_base += int(info.n_rows)

    seam = [None, None]
    if rank_error is not None:
        pass                              # (nothing was opened: straight to the exchange)
    elif native is not None:
        # BAM in (and BAM or nothing out): libampbam decodes records straight into packed batches and
        # re-encodes the kept ones; no per-read Python object exists on this path.  The file is walked piece by piece:
        # piece k + 1 is inflated and indexed on a helper thread while piece k is decoded, trimmed and counted, and a
        # writer thread re-encodes and deflates the rows of piece k - 1 (every stage is a C call that releases the GIL;
        # rows stay in order)
        src, nwriter = native
        wq = werr = wthread = None
        if run_trim and nwriter is not None:
            import queue
            import threading
            wq = queue.Queue(maxsize=3); werr = []

            def _writer():
                while True:
                    job = wq.get()
                    if job is None:
                        return
                    try:
                        if job[0] == "close":
                            job[1].close()
                        elif not werr:
                            nwriter.write_rows(*job[1:])
                    except Exception as e:       # surfaced by the main thread
                        werr.append(e)
            wthread = threading.Thread(target=_writer, daemon=True); wthread.start()
        loop_done = False
        try:
            for piece in src:
                for first in range(0, piece.n_records, NATIVE_BATCH_READS):
                    count = min(NATIVE_BATCH_READS, piece.n_records - first)
                    batch, _ = piece.decode(first, count)
                    progress(count)
                    n_seen += count
                    s_i = n_seen - 1
                    if batch.n == 0:
                        continue
                    n_bases += int(batch.lseq.sum(dtype=np.int64))
                    res = eng.process(batch, read_base=read_base)
                    bad = np.nonzero(res.status)[0]
                    if wq is not None:
                        if werr:
                            raise werr[0]
                        keep = (res.ref_len >= min_length) & (((res.trim_flags & 3) != 0) | bool(include_no_primer))   # AmpliPy.py:910
                        if len(bad):
                            keep[int(bad[0]):] = False          # the reads in front of the failing one are still written (A:907-911)
                        slot_off = batch.cig_off[:-1] + np.uint64(3) * np.arange(batch.n, dtype=np.uint64)
                        # src_index is a view of the decoder's buffers, which the next decode overwrites
                        wq.put(("rows", piece, batch.src_index.copy(), keep, res.new_pos, res.new_ncig, slot_off, res.new_cig))
                    if len(bad):
                        _raise_for_status(res.status[bad[0]])
                    if do_count:
                        _store_events(eng, ins_store, read_base)
                    read_base += batch.n
                if wq is not None:
                    wq.put(("close", piece))        # (the writer copies the unchanged parts of a record from the piece's image)
                else:
                    piece.close()
            loop_done = True
        except Exception as e:                      # with several ranks the others must not be left waiting in the collective
            if dist is None:
                raise
            rank_error = e
        finally:
            if not loop_done:
                src.close()                 # (the piece opened ahead of the one that failed)
            if wq is not None:
                wq.put(None)
                # One process: the writer thread goes on re-encoding and deflating the last rows under the calls and the VCF
                # text below (32 ms of Python for 12,000 records) and is joined behind them.  Several ranks need to know
                # whether it failed before the collective.
                if dist is not None or not loop_done:
                    wthread.join()
                else:
                    writer_pending = True
        if not writer_pending:
            if werr and rank_error is None:
                if dist is None:
                    raise werr[0]
                rank_error = werr[0]
            if nwriter is not None and rank_error is None:
                nwriter.close()
        seam = getattr(src, "seam", [None, None])
    elif bamdev is not None:
        # BAM in with the switch on: the compressed bytes of a piece of whole BGZF blocks go to the device, which inflates them,
        # checks every block's CRC, indexes the records and decodes the rows into the packed batch (bam_device; the next piece
        # is read and copied up while this one is there).  The read pass runs on that batch.  A run that writes trimmed reads
        # (both switches on) has the kept records of every piece re-encoded, compressed and framed there as well: the BGZF
        # blocks of the trimmed BAM are all that comes back.  With the SAM switch on as well and trimmed reads going out as text
        # (section 14), the kept records of a piece become SAM lines there; a piece with a record the device calls odd comes down as
        # its image and goes through the Python codec (same Rec / flush() code as the last branch), then the next piece is the
        # device's again; rows stay in input order.
        from . import bam_device
        stats = bam_device.LAST_RUN_STATS
        stats.update(pieces=0, blocks_device=0, blocks_host=0, index_rounds=0, waits=0, records=0, bytes_up=0, bytes_file=0)
        stats.update((k_, 0) for k_ in bam_device.OUT_STATS + bam_device.TEXT_STATS)
        refuse = os.environ.get("AMPLIPY_GPU_BAM_REFUSE_BLOCK") if os.environ.get("AMPLIPY_DEV") == "1" else None
        codec = None
        out = None
        running = None
        emit = None
        flushed = False
        if bamdev_io is not None:
            src, out = bamdev_io

            def emit():
                # ampbam_write_rows of the host path: the rows in front of a failing one are written (A:907-911), and whole blocks
                # only -- the rest of the stream is flushed with the last piece, unless the run ends on a failing row (the host
                # writer is not closed then either)
                nonlocal flushed
                flushed = running["pieces"] == len(src.pieces) and codec.first_bad < 0
                out.encode(codec, running, min_length, include_no_primer, final=flushed)
        outb = None
        if bamdev_text is not None:
            src, writer, outb = bamdev_text

            def emit():                   # AmpliPy.py:910-911 for the piece: the lines of the kept rows in front of a failing one
                text, ti = codec.format(min_length, include_no_primer)
                outb.write(text)
                running["text_rows"] += int(ti.n_rows_written)
                running["text_bytes"] += int(ti.n_bytes)
                running["bytes_down"] += int(ti.bytes_down)
                running["waits"] += int(ti.waits)

        def image_records():
            """The records that end in the piece's image, as the Python codec reads them."""
            img, offs = codec.image()
            running["bytes_down"] += int(img.size) + 4 * int(offs.size)
            running["waits"] += 1
            for o in (int(x) for x in offs):
                yield bamio.rec_of_bam_bytes(img[o + 4:o + 4 + int(img[o:o + 4].view("<u4")[0])].tobytes())
        try:
            if out is None and outb is None:
                src = bam_device.DeviceBamInput(bamdev)
            codec = bam_device.BamCodec(eng)
            if outb is not None:
                codec.set_references([n for n, _ in src.references])
            for info, running in bam_device.walk(codec, src, refuse_block=int(refuse) if refuse else None):
                try:
                    odd = False
                    if outb is not None:
                        ti = codec.text_check()
                        running["waits"] += int(ti.waits)
                        running["bytes_down"] += int(ti.bytes_down)
                        odd = ti.first_odd_row >= 0
                        running["text_pieces_python" if odd else "text_pieces_device"] += 1
                    if odd:               # the read pass does not run on the device's batch of this piece: nothing is counted twice
                        try:
                            python_records(image_records())
                        finally:
                            writer._f.flush()
                    else:
                        device_piece(codec, info, emit)
                finally:
                    stats.update(running)
            if out is not None:
                # header blocks and end-of-file block are the host codec's (a last piece without rows: the bare flush)
                if not flushed:
                    out.encode(codec, stats, min_length, include_no_primer, final=True)
                out.close()
            print_log("BAM device codec: %d pieces, %d blocks on the device, %d through the host codec, %d index rounds"
                      % (stats["pieces"], stats["blocks_device"], stats["blocks_host"], stats["index_rounds"])
                      + ("" if out is None else "; trimmed reads: %d blocks on the device, %d through the host codec, %d bytes down"
                         % (stats["out_blocks_device"], stats["out_blocks_host"], stats["bytes_down"]))
                      + ("" if outb is None else "; trimmed reads as SAM text: %d pieces on the device, %d through the Python codec"
                         % (stats["text_pieces_device"], stats["text_pieces_python"])))
        finally:
            if outb is not None:
                writer._f.flush()
                outb.flush()
                if outb is not getattr(sys.stdout, "buffer", None):
                    outb.close()
            if codec is not None:
                codec.close()
    elif sam is not None:
        # SAM text in (and SAM text or nothing out) with the switch on: chunks of whole lines are parsed, packed, trimmed / counted
        # and, for a trimmed output, turned back into text on the device (sam_native; no per-read Python object).  A chunk
        # with a line the device calls odd goes through the Python codec as below (same Rec / flush() code), then the next chunk
        # is the device's again; rows stay in input order.  With both switches on and a new BAM file out (section 13) the kept
        # rows of a device chunk become BAM records, DEFLATE streams and framed BGZF blocks there (one wait per chunk behind the
        # parse's), and the records the Python codec makes of an odd chunk go up into the same stream: the file's blocks do not
        # depend on which side encoded a chunk.
        import io
        from . import sam_native
        src, sam_hdr, writer, outb, device_ok, bam_out = sam
        stats = sam_native.LAST_RUN_STATS
        stats.update(device_chunks=0, python_chunks=0, records=0)
        stats.update((k_, 0) for k_ in sam_native.OUT_STATS)
        codec = None
        py_reader = bamio.AlignmentReader.for_header(sam_hdr)
        host_recs = []                    # record bytes the Python codec made of an odd chunk, on their way into the device's stream

        class RecordSink:                 # what flush() writes kept records to on that way
            @staticmethod
            def write(r, pos=None, cigar=None):
                host_recs.append(bamio.bam_record_bytes(r, r.pos if pos is None else pos, r.cigar if cigar is None else cigar))
        if bam_out is not None:
            writer = RecordSink

        def encode_kept():                # AmpliPy.py:910-911: the rows in front of a failing one, whole blocks only
            bam_out.encode(codec, stats, min_length, include_no_primer)
            stats["encodes"] += 1

        def send_host_recs(final=False):
            if host_recs or final:
                bam_out.encode_bytes(codec, stats, b"".join(host_recs), final=final)
                stats["encodes"] += 1
                del host_recs[:]

        def write_kept():
            if run_trim and writer is not None:
                text, _ = codec.format(min_length, include_no_primer)       # AmpliPy.py:910-911
                outb.write(text)
        try:
            if device_ok:
                codec = sam_native.SamCodec(eng)
                codec.set_references([n for n, _ in sam_hdr.refs])
                if bam_out is not None:
                    codec.set_output(sam_native.OUT_BAM)
            for chunk in src:
                info = codec.parse(chunk) if codec is not None else None
                if info is None or info.first_odd_line >= 0:
                    stats["python_chunks"] += 1
                    try:
                        python_records(py_reader.records_of(io.TextIOWrapper(io.BytesIO(chunk))))
                    finally:
                        if bam_out is not None:
                            send_host_recs()          # (on a failing read too: the rows in front of it were written)
                    if outb is not None:
                        writer._f.flush()
                    continue
                stats["device_chunks"] += 1
                if bam_out is not None:
                    device_piece(codec, info, emit=encode_kept, defer=True)
                else:
                    device_piece(codec, info, emit=write_kept)
            stats["records"] = n_seen
            if bam_out is not None:
                # the partial block, then the end-of-file block; not on a failing read (the Python codec does not close its
                # writer then either).  The flush is a call of its own: a chunk's encode does not know the read pass's verdict
                send_host_recs(final=True)
                bam_out.close()
            elif writer is not None and outb is None:
                writer.close()                        # (a BAM output of a run whose header keeps it on the Python codec)
            print_log("SAM text codec: %d chunks on the device, %d through the Python codec" % (stats["device_chunks"], stats["python_chunks"])
                      + ("" if bam_out is None else "; trimmed reads went out as BAM blocks from the device: %d blocks on the device, %d "
                         "through the host, %d bytes down" % (stats["out_blocks_device"], stats["out_blocks_host"], stats["bytes_down"])))
        finally:
            if outb is not None:
                writer._f.flush()
                outb.flush()
                if outb is not getattr(sys.stdout, "buffer", None):
                    outb.close()
            if codec is not None:
                codec.close()
            src.close()
    else:
        seam = [None, None]
        try:
            for s_i, rec in enumerate(reader):
                if s_i % PROGRESS_NUM_READS == 0 and s_i != 0:
                    print_log("Processed %d reads..." % s_i)
                if (rec.flag & 4) or rec.cigar is None:            # AmpliPy.py:902
                    continue
                if world > 1 and s_i % world != rank:              # text input has no record index: deal the reads out
                    continue
                pending.append(rec)
                if len(pending) >= BATCH_READS:
                    flush()
            flush()
            if writer is not None:
                writer.close()
            reader.close()
        except Exception as e:
            if dist is None:
                raise
            rank_error = e

    if dist is not None:
        # before the one collective of the run: did every rank get through its share (a rank that raised must not leave the
        # others waiting in the all-reduce), and do the shares of neighbouring ranks meet (every share of a BAM file starts
        # where the one before it ended: what makes the split of ampbam_open_range exact)
        trouble = parallel.exchange_notes(dist, world, seam, rank_error)
        if trouble:
            eng.close()
            parallel.finish(dist)
            if rank_error is not None:
                raise rank_error
            raise RuntimeError(trouble)
        shares = parallel.gather_objects(dist, rank, world, (n_seen, n_bases))
        if rank == 0 and native is not None:
            # the file is cut by compressed bytes (ampbam_open_range): what that gave every rank, in records and in bases
            tot = max(sum(b_ for _, b_ in shares), 1)
            print_log("Shares of the %d ranks: records %s; bases %s (%s %% of the job)" % (world, [r_ for r_, _ in shares], [b_ for _, b_ in shares],
                                                                                        ", ".join("%.1f" % (100.0 * b_ / tot) for _, b_ in shares)))
        if final_trimmed_fn is not None and native is not None and native[1] is not None:
            # the ranks' files (all closed by now: the writer threads were joined above) become the one trimmed BAM
            parts = parallel.gather_objects(dist, rank, world, (native[1].path, native[1].header_bytes))
            if rank == 0:
                from . import bam_native
                bam_native.stitch_bam_parts(final_trimmed_fn, parts)
                for path, _ in parts:
                    os.remove(path)
                print_log("Trimmed reads of %d ranks joined: %s" % (world, final_trimmed_fn))

    try:
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

        def ins_tallies(positions):
            triples = ins_store.counted_pairs(positions)
            if dist is not None:                       # all ranks flag the same positions (same table): symmetric exchange
                triples = parallel.allgather_relevant_events(dist, world, triples)
            return calling.tallies_from_runs(triples, positions)
        res = calling.call(eng, ref_seq, cp, ins_tallies)
        if rank != 0:
            run_variants = run_consensus = False       # rank 0 writes the outputs
        if run_variants:
            vcf.f.write(res.vcf_text(vcf.ref_id))        # (= vcf.write(r) for r in res.records)
            vcf.close()
        if run_consensus:
            f = gzip.open(consensus_fn, "wt") if consensus_fn.lower().endswith(".gz") else open(consensus_fn, "w")
            f.write(">sample\n%s\n" % res.consensus_string(unknown_symbol))
            f.close()
    finally:
        if writer_pending:
            wthread.join()
            if nwriter is not None and sys.exc_info()[0] is not None:
                try:                        # (the calls failed: the trimmed BAM is still ended properly)
                    nwriter.close()
                except Exception:
                    pass
    if writer_pending:
        if werr:
            raise werr[0]
        if nwriter is not None:
            nwriter.close()
    eng.close()
    parallel.finish(dist)
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
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.command == "trim":
        run_amplipy(untrimmed_reads_fn=args.input, primer_fn=args.primer, reference_fn=args.reference,
                    trimmed_reads_fn=args.output, primer_pos_offset=args.primer_pos_offset, min_length=args.min_length,
                    min_quality=args.min_quality, sliding_window_width=args.sliding_window_width,
                    include_no_primer=args.include_no_primer, run_trim=True)
    elif args.command == "variants":
        run_amplipy(trimmed_reads_fn=args.input, reference_fn=args.reference, variants_fn=args.output,
                    min_quality=args.min_quality, min_freq_variants=args.min_freq, min_depth_variants=args.min_depth,
                    run_variants=True)
    elif args.command == "consensus":
        run_amplipy(trimmed_reads_fn=args.input, reference_fn=args.reference, consensus_fn=args.output,
                    min_quality=args.min_quality, min_freq_consensus=args.min_freq, min_depth_consensus=args.min_depth,
                    unknown_symbol=args.unknown_symbol, run_consensus=True)
    elif args.command == "aio":
        run_amplipy(untrimmed_reads_fn=args.input, primer_fn=args.primer, reference_fn=args.reference,
                    trimmed_reads_fn=args.output_trimmed_reads, variants_fn=args.output_variants,
                    consensus_fn=args.output_consensus, primer_pos_offset=args.primer_pos_offset,
                    min_length=args.min_length, min_quality=args.min_quality,
                    sliding_window_width=args.sliding_window_width, min_freq_consensus=args.min_freq_consensus,
                    min_freq_variants=args.min_freq_variants, min_depth_consensus=args.min_depth_consensus,
                    min_depth_variants=args.min_depth_variants, unknown_symbol=args.unknown_symbol,
                    include_no_primer=args.include_no_primer, run_trim=True, run_variants=True, run_consensus=True)


if __name__ == "__main__":
    main()
