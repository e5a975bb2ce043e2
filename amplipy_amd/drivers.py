"""The I/O paths of run_amplipy, one driver each: the Python codec (``bamio``), libampbam (``bam_native``), the device codec for BAM
input (``bam_device``) and the one for SAM text (``sam_native``).  ``select`` says which driver and which sink for the trimmed reads
serve a run, from names and switches alone; ``open_driver`` opens them.  A driver has ``open(...)`` (None: the path cannot serve this
run after all), ``run(loop)`` on a ``readloop.ReadLoop``, which walks the input and raises what the run dies of, and ``finish(failed)``
behind the calling.  The device drivers write trimmed reads to a sink: none, a ``bam_device.DeviceBamOutput``, or a ``TextSink``.
"""
from __future__ import annotations

import io
import os
import sys
from collections import namedtuple
from os.path import isfile

import numpy as np

from . import AMPLIPY_VERSION as VERSION, bamio
from .readloop import error, print_log

NATIVE_BATCH_READS = 1 << 18       # records per device batch on the libampbam path (the writer overlaps the next batch)
NATIVE_PART_BYTES = 4 << 20        # compressed bytes of a piece of the input BAM (pieces are inflated one ahead of the GPU); on the
                                   # 11.6 MB / 1.5 M-read file of the bench: 16 MB (one piece) aio 10.5 M reads/s, 4 MB 12.4, 1 MB 12.4


# ---- output openers (AmpliPy.py:261-360) --------------------------------------------------------
def _reads_mode(fn, write):
    low = fn.lower()
    if low.endswith(".sam"):
        return "w" if write else "r"
    if low.endswith(".bam"):
        return "wb" if write else "rb"
    error("Invalid read mapping extension (should be .sam or .bam): %s" % fn)


def _out_header(header):
    return header.with_amplipy_pg(VERSION, " ".join(sys.argv))


def _bam_level():
    return int(os.environ.get("AMPLIPY_BAM_LEVEL", "-1"))        # zlib's default level like htslib; 1 trades file size for speed


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
        hdr = _out_header(reader.header)
        if output_fn.lower() == "stdout":
            writer = bamio.AlignmentWriter("-", "w", hdr)
        elif isfile(output_fn):
            error("File already exists: %s" % output_fn)
        else:
            writer = bamio.AlignmentWriter(output_fn, _reads_mode(output_fn, True), hdr)
    return reader, writer


# ---- which driver, which sink -------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "driver sink note")     # driver: "python" / "native" / "device_bam" / "device_sam"; sink: None / "bam" / "text"
HOST_READS_NOTE = "BAM device codec: this run writes trimmed reads, the host codec reads the input"


def _is_new(fn, ext):
    return fn.lower() != "stdout" and not isfile(fn) and fn.lower().endswith(ext)


def _text_target(fn):       # stdout (with its binary layer at hand) or a new .sam file: where a TextSink can write
    return hasattr(sys.stdout, "buffer") if fn.lower() == "stdout" else _is_new(fn, ".sam")


def select(input_fn, output_fn, run_trim, gpu_sam=False, gpu_bam=False, gpu_bam_write=False, several=False):
    """The Route of a run, from the names of its input and of its trimmed output (None: none is written), what it does and the three
    switches as run_amplipy's docstring states them; several: more than one process, which turns every switch off.  Nothing is
    opened: a header the device's name table cannot take still sends a device route's run to the Python codec afterwards
    (``open_driver``).  Whatever no other path serves is the Python codec's, which refuses it with the reference's messages."""
    if several:
        gpu_sam = gpu_bam = gpu_bam_write = False
    if not run_trim:
        output_fn = None
    from_stdin = input_fn is not None and input_fn.lower() == "stdin"
    a_file = input_fn is not None and not from_stdin and isfile(input_fn)
    if a_file and input_fn.lower().endswith(".bam") and not os.environ.get("AMPLIPY_PYTHON_BAM"):
        if not run_trim:
            return Route("device_bam" if gpu_bam else "native", None, None)
        new_bam = output_fn is not None and _is_new(output_fn, ".bam")
        if gpu_bam and gpu_bam_write and new_bam:
            return Route("device_bam", "bam", None)
        if gpu_bam and gpu_sam and output_fn is not None and _text_target(output_fn):
            return Route("device_bam", "text", None)
        if new_bam or output_fn is None:
            return Route("native", None, HOST_READS_NOTE if gpu_bam else None)
    elif gpu_sam and (a_file and input_fn.lower().endswith(".sam") or from_stdin and hasattr(sys.stdin, "buffer")):
        if output_fn is None:
            return Route("device_sam", None, None)
        if _text_target(output_fn):
            return Route("device_sam", "text", None)
        if gpu_bam_write and _is_new(output_fn, ".bam"):
            return Route("device_sam", "bam", None)
    return Route("python", None, None)


def open_driver(route, input_fn, output_fn, rank=0, world=1, device=0, several=False):
    """The driver of ``route`` on these files (output_fn None: no trimmed reads); the Python codec's where the header turns it down."""
    if route.driver == "native":
        return NativeDriver.open(input_fn, output_fn, rank, world, device, several)
    device_driver = {"device_bam": DeviceBamDriver, "device_sam": DeviceSamDriver}.get(route.driver)
    return device_driver and device_driver.open(input_fn, output_fn, route.sink) or PythonDriver(input_fn, output_fn, rank, world)


class TextSink:
    """Trimmed reads as SAM text from a device codec: the binary layer ``outb`` of stdout or of a new file, which takes the device's
    bytes (``write``), and on top of it a text layer with the Python codec's ``writer`` for the pieces the device hands back.  The
    header went out through the text layer; what goes through it is flushed (``flush_text``) before the device's bytes follow."""

    def __init__(self, output_fn, header):
        header = _out_header(header)        # (a header it cannot be made from raises before a file is made)
        if output_fn.lower() == "stdout":
            outt, self.outb = sys.stdout, sys.stdout.buffer
        else:
            self.outb = open(output_fn, "wb")
            outt = io.TextIOWrapper(self.outb, write_through=True)       # (what open(output_fn, "w") is made of)
        self.writer = bamio.AlignmentWriter(None, "w", header, fileobj=outt)
        self.write, self.flush_text = self.outb.write, self.writer.flush
        self.flush_text()

    def close(self):
        """The text layer, then the binary one; stdout stays open."""
        self.flush_text()
        self.outb.flush()
        if self.outb is not getattr(sys.stdout, "buffer", None):
            self.outb.close()


class Driver:
    seam = (None, None)         # (first, end) of the rank's share of a BAM file in the inflated stream, where the path knows it
    part_writer = None          # the writer of the rank's own trimmed BAM, which rank 0 joins to the others'

    def finish(self, failed):
        """Behind the calling (failed: it raised)."""


class PythonDriver(Driver):
    """The Python codec: Rec objects of ``bamio`` through the loop's flush(); refuses what no path can serve, as the reference does."""

    def __init__(self, input_fn, output_fn, rank=0, world=1):
        self.reader, self.writer = open_alignment_files(input_fn, output_fn)
        self.rank, self.world = rank, world

    def run(self, loop):
        loop.python_records(self.reader, self.writer, self.rank, self.world)
        if self.writer is not None:
            self.writer.close()
        self.reader.close()


# ---- libampbam ------------------------------------------------------------------------------------------------------------------
def native_parts(input_fn, rank=0, world=1, part_bytes=None):
    """How a BAM file is cut for this rank: (n_parts, k_lo, k_hi) -- the file has n_parts pieces of about ``part_bytes``
    compressed bytes (ampbam_open_range: cut at BGZF block starts, i.e. by base count for a sorted BAM), of which the rank
    takes the contiguous run [k_lo, k_hi).  Every rank gets the same number of pieces (n_parts is a multiple of world)."""
    part_bytes = part_bytes or int(os.environ.get("AMPLIPY_PART_BYTES", NATIVE_PART_BYTES))
    size = os.path.getsize(input_fn)
    per_rank = max(1, -(-size // (part_bytes * world)))
    return per_rank * world, per_rank * rank, per_rank * (rank + 1)


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
        from . import bam_native
        prev_end = None
        self.seam = [None, None]
        cur = self.first_part()
        self._first = None
        exact = self.k_lo == 0          # the walk knows where a record starts: from the file's first piece on, else from its first record on
        for k in range(self.k_lo, self.k_hi):
            # the piece behind this one starts where this one ends: it is told so, and only the rank's FIRST pieces (whose
            # predecessor another rank reads), up to the first with a record, are found by the codec's chain-of-plausible-records
            # search (a guessed piece without records does not know where it ends; a told one hands on what it was told)
            a, b = cur.part_range()
            exact = exact or cur.n_records > 0
            if k + 1 < self.k_hi:
                self._start(k + 1, b if exact else None)
            if cur.n_records:
                if prev_end is not None and a != prev_end:
                    raise bam_native.AmpBamError("%s: piece %d of %d starts at inflated offset %d, the piece before it ended at %d"
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


class NativeDriver(Driver):
    """BAM in (and BAM or nothing out) through libampbam, without a per-read Python object; the only path besides the Python codec's
    that serves several ranks.  Piece k + 1 is inflated and indexed on a helper thread while piece k is decoded, trimmed and
    counted, and a writer thread re-encodes and deflates the rows of piece k - 1 (C calls that release the GIL; rows stay in order)."""

    def __init__(self, src, writer, several):
        self.src, self.part_writer, self.several = src, writer, several
        self.thread = None          # the writer thread, while it is still running behind run() (joined in finish())
        self.werr = []

    @classmethod
    def open(cls, input_fn, output_fn, rank=0, world=1, device=0, several=False):
        """On a BAM file in and a new BAM file (or nothing) out, as ``select`` found them."""
        from . import bam_native
        src = NativeInput(input_fn, rank, world)
        writer = None
        if output_fn is not None:
            first = src.first_part()
            hdr = _out_header(bamio.Header(first.header_text, first.references))
            # AMPLIPY_GPU_DEFLATE=1 hands the blocks' DEFLATE streams to the HIP encoder on this rank's device
            writer = bam_native.BamWriter(output_fn, hdr.text, first, level=_bam_level(),
                                          gpu_deflate=os.environ.get("AMPLIPY_GPU_DEFLATE", "0") not in ("", "0"), device=device)
        return cls(src, writer, several)

    def _write_jobs(self, wq):
        while True:
            job = wq.get()
            if job is None:
                return
            try:
                if job[0] == "close":
                    job[1].close()
                elif not self.werr:
                    self.part_writer.write_rows(*job[1:])
            except Exception as e:       # surfaced by the main thread
                self.werr.append(e)

    def run(self, loop):
        import queue
        import threading
        src, wq, wthread = self.src, None, None
        if loop.run_trim and self.part_writer is not None:
            wq = queue.Queue(maxsize=3)
            wthread = threading.Thread(target=self._write_jobs, args=(wq,), daemon=True); wthread.start()
        done = False
        try:
            for piece in src:
                for first in range(0, piece.n_records, NATIVE_BATCH_READS):
                    count = min(NATIVE_BATCH_READS, piece.n_records - first)
                    batch, _ = piece.decode(first, count)
                    loop.progress(count)
                    if batch.n == 0:
                        continue
                    loop.n_bases += int(batch.lseq.sum(dtype=np.int64))
                    res, first_bad = loop.host_batch(batch)
                    if wq is not None:
                        if self.werr:
                            raise self.werr[0]
                        slot_off = batch.cig_off[:-1] + np.uint64(3) * np.arange(batch.n, dtype=np.uint64)
                        # src_index is a view of the decoder's buffers, which the next decode overwrites
                        wq.put(("rows", piece, batch.src_index.copy(), loop.keep(res, first_bad), res.new_pos, res.new_ncig, slot_off, res.new_cig))
                    loop.batch_done(batch.n, res, first_bad)
                if wq is not None:
                    wq.put(("close", piece))        # (the writer copies the unchanged parts of a record from the piece's image)
                else:
                    piece.close()
            done = True
        finally:
            self.seam = getattr(src, "seam", self.seam)
            if not done:
                src.close()                 # (the piece opened ahead of the one that failed)
            if wq is not None:
                wq.put(None)
                # One process: the writer thread goes on with the last rows under the calls and the VCF text (32 ms of Python for
                # 12,000 records) and is joined behind them.  Several ranks need to know whether it failed before the collective.
                if self.several or not done:
                    wthread.join()
                else:
                    self.thread = wthread
        if self.thread is None:
            self._end()

    def _end(self):
        if self.werr:
            raise self.werr[0]
        if self.part_writer is not None:
            self.part_writer.close()

    def finish(self, failed):
        if self.thread is None:
            return
        self.thread.join()
        if not failed:
            return self._end()
        try:                        # (the calls failed: the trimmed BAM is still ended properly)
            self.part_writer.close()
        except Exception:
            pass


# ---- the device codecs ----------------------------------------------------------------------------------------------------------
class DeviceBamDriver(Driver):
    """BAM in with the switch on: pieces of whole BGZF blocks are inflated, checked, indexed and decoded into the packed batch on the
    device (bam_device), where the read pass runs on it.  With a DeviceBamOutput as the sink the kept records are re-encoded,
    compressed and framed there too.  With a TextSink they become SAM lines there (section 14); a piece with
    a record the device calls odd comes down as its image and goes through the loop's python_records; rows stay in input order."""

    def __init__(self, src, sink=None, path=None):
        self.src, self.sink, self.path = src, sink, path       # src None: run() opens the bam_device.DeviceBamInput of ``path``

    @classmethod
    def open(cls, input_fn, output_fn, sink):
        """sink "bam": header blocks and end-of-file block are the host codec's.  sink "text": None unless
        the file is one the host codec's block walk takes (the Python codec says what it finds) with a header of plain ASCII
        text whose @SQ names fit the device's name table."""
        from . import bam_device, bam_native, devcodec
        if sink is None:
            return cls(None, path=input_fn)
        try:
            src = bam_device.DeviceBamInput(input_fn)
        except bam_native.AmpBamError:
            if sink == "text":
                return None
            raise
        header = bamio.Header(src.header_text, src.references)
        if sink == "bam":
            return cls(src, bam_device.DeviceBamOutput(output_fn, _out_header(header).text, src.references, level=_bam_level()))
        if not all(ord(c) < 128 for c in src.header_text) or not devcodec.names_fit([n for n, _ in src.references]):
            return None
        return cls(src, TextSink(output_fn, header))

    def _encode(self, loop, codec, running):
        # the rows in front of a failing one are written (A:907-911), and whole blocks only: the rest of the stream is flushed with
        # the last piece, unless the run ends on a failing row (the host writer is not closed then either)
        self.flushed = running["pieces"] == len(self.src.pieces) and codec.first_bad < 0
        self.sink.encode(codec, running, loop.min_length, loop.include_no_primer, final=self.flushed)

    def _format(self, loop, codec, running):        # AmpliPy.py:910-911 for the piece: the lines of the kept rows in front of a failing one
        text, ti = codec.format(loop.min_length, loop.include_no_primer)
        self.sink.write(text)
        running["text_rows"] += int(ti.n_rows_written)
        running["text_bytes"] += int(ti.n_bytes)
        running["bytes_down"] += int(ti.bytes_down)
        running["waits"] += int(ti.waits)

    @staticmethod
    def _image_records(codec, running):
        """The records that end in the piece's image, as the Python codec reads them."""
        img, offs = codec.image()
        running["bytes_down"] += int(img.size) + 4 * int(offs.size)
        running["waits"] += 1
        for o in (int(x) for x in offs):
            yield bamio.rec_of_bam_bytes(img[o + 4:o + 4 + int(img[o:o + 4].view("<u4")[0])].tobytes())

    def run(self, loop):
        from . import bam_device
        stats = bam_device.LAST_RUN_STATS
        stats.update(bam_device.zeroed_stats())
        refuse = os.environ.get("AMPLIPY_GPU_BAM_REFUSE_BLOCK") if os.environ.get("AMPLIPY_DEV") == "1" else None
        sink = self.sink
        text = sink if isinstance(sink, TextSink) else None
        emit = None if sink is None else self._format if text else self._encode
        self.flushed = False
        codec = None
        try:
            if self.src is None:
                self.src = bam_device.DeviceBamInput(self.path)
            codec = bam_device.BamCodec(loop.eng)
            if text:
                codec.set_references([n for n, _ in self.src.references])
            for info, running in bam_device.walk(codec, self.src, refuse_block=int(refuse) if refuse else None):
                try:
                    odd = False
                    if text:
                        ti = codec.text_check()
                        running["waits"] += int(ti.waits)
                        running["bytes_down"] += int(ti.bytes_down)
                        odd = ti.first_odd_row >= 0
                        running["text_pieces_python" if odd else "text_pieces_device"] += 1
                    if odd:               # the read pass does not run on the device's batch of this piece: nothing is counted twice
                        try:
                            loop.python_records(self._image_records(codec, running), text.writer)
                        finally:
                            text.flush_text()
                    else:
                        loop.device_piece(codec, info, emit and (lambda: emit(loop, codec, running)))
                finally:
                    stats.update(running)
            if sink is not None and not text:
                if not self.flushed:      # (a last piece without rows: the bare flush)
                    sink.encode(codec, stats, loop.min_length, loop.include_no_primer, final=True)
                sink.close()
            print_log("BAM device codec: %d pieces, %d blocks on the device, %d through the host codec, %d index rounds"
                      % (stats["pieces"], stats["blocks_device"], stats["blocks_host"], stats["index_rounds"])
                      + ("" if sink is None or text else "; trimmed reads: %d blocks on the device, %d through the host codec, %d bytes down"
                         % (stats["out_blocks_device"], stats["out_blocks_host"], stats["bytes_down"]))
                      + ("" if not text else "; trimmed reads as SAM text: %d pieces on the device, %d through the Python codec"
                         % (stats["text_pieces_device"], stats["text_pieces_python"])))
        finally:
            if text:
                text.close()
            if codec is not None:
                codec.close()


class RecordSink:
    """Takes the kept records the Python codec makes of an odd chunk as BAM record bytes, on their way into the device's stream."""

    def __init__(self):
        self.recs = []

    def write(self, r, pos=None, cigar=None):
        self.recs.append(bamio.bam_record_bytes(r, r.pos if pos is None else pos, r.cigar if cigar is None else cigar))


class DeviceSamDriver(Driver):
    """SAM text in with the switch on: chunks of whole lines are parsed, packed, trimmed / counted and, for a TextSink, turned back
    into text on the device (sam_native).  A chunk with a line the device calls odd goes through the loop's python_records; rows
    stay in input order.  With a DeviceBamOutput as the sink the kept rows of a device chunk become framed
    BGZF blocks there, and the records of an odd chunk go up into the same stream through a RecordSink."""

    def __init__(self, src, header, device_ok, sink=None, writer=None):
        self.src, self.header, self.device_ok, self.sink = src, header, device_ok, sink
        self.text = sink if isinstance(sink, TextSink) else None
        self.bam_out = None if self.text else sink
        self.host_recs = RecordSink()
        # what python_records writes kept records to: the Python codec's BAM writer, the sink's text writer or the RecordSink
        self.writer = writer if sink is None else sink.writer if self.text else self.host_recs

    @classmethod
    def open(cls, input_fn, output_fn, sink):
        """On stdin or a .sam file in, as ``select`` found them.  device_ok False: the header is one the device's name table cannot
        take (more than 64 @SQ lines, a name that is not plain text) -- every chunk of the run then goes through the Python codec,
        and a BAM output through its writer, as with the switches off."""
        from . import bam_device, devcodec, sam_native
        src = sam_native.SamTextInput("-" if input_fn.lower() == "stdin" else input_fn)
        text = src.header_text()
        hdr = bamio.Header(text, bamio._refs_from_text(text))
        device_ok = src.header_is_plain() and devcodec.names_fit([n for n, _ in hdr.refs])
        if sink == "text":
            return cls(src, hdr, device_ok, TextSink(output_fn, hdr))
        if sink == "bam" and device_ok:
            return cls(src, hdr, device_ok, bam_device.DeviceBamOutput(output_fn, _out_header(hdr).text, hdr.refs, level=_bam_level()))
        return cls(src, hdr, device_ok, writer=bamio.AlignmentWriter(output_fn, "wb", _out_header(hdr)) if sink == "bam" else None)

    def _send_host_recs(self, codec, stats, final=False):
        recs = self.host_recs.recs
        if recs or final:
            self.bam_out.encode_bytes(codec, stats, b"".join(recs), final=final)
            stats["encodes"] += 1
            del recs[:]

    def _encode(self, loop, codec, stats):          # AmpliPy.py:910-911: the rows in front of a failing one, whole blocks only
        self.bam_out.encode(codec, stats, loop.min_length, loop.include_no_primer)
        stats["encodes"] += 1

    def run(self, loop):
        from . import sam_native
        stats = sam_native.LAST_RUN_STATS
        stats.update(sam_native.zeroed_stats())
        text, bam_out = self.text, self.bam_out
        codec = None
        py_reader = bamio.AlignmentReader.for_header(self.header)
        emit = None
        if bam_out is not None:
            emit = lambda: self._encode(loop, codec, stats)
        elif text:
            emit = lambda: text.write(codec.format(loop.min_length, loop.include_no_primer)[0])      # AmpliPy.py:910-911
        try:
            if self.device_ok:
                codec = sam_native.SamCodec(loop.eng)
                codec.set_references([n for n, _ in self.header.refs])
                if bam_out is not None:
                    codec.set_output(sam_native.OUT_BAM)
            for chunk in self.src:
                info = codec.parse(chunk) if codec is not None else None
                if info is None or info.first_odd_line >= 0:
                    stats["python_chunks"] += 1
                    try:
                        loop.python_records(py_reader.records_of(io.TextIOWrapper(io.BytesIO(chunk))), self.writer)
                    finally:
                        if bam_out is not None:
                            self._send_host_recs(codec, stats)        # (on a failing read too: the rows in front of it were written)
                    if text:
                        text.flush_text()
                    continue
                stats["device_chunks"] += 1
                loop.device_piece(codec, info, emit, defer=bam_out is not None)
            stats["records"] = loop.n_seen
            if bam_out is not None:
                # the partial block and the end-of-file block, as a call of its own (a chunk's encode does not know the read pass's
                # verdict); not on a failing read (the Python codec does not close its writer then either)
                self._send_host_recs(codec, stats, final=True)
                bam_out.close()
            elif self.sink is None and self.writer is not None:
                self.writer.close()                   # (a BAM output of a run whose header keeps it on the Python codec)
            print_log("SAM text codec: %d chunks on the device, %d through the Python codec" % (stats["device_chunks"], stats["python_chunks"])
                      + ("" if bam_out is None else "; trimmed reads went out as BAM blocks from the device: %d blocks on the device, %d "
                         "through the host, %d bytes down" % (stats["out_blocks_device"], stats["out_blocks_host"], stats["bytes_down"])))
        finally:
            if text:
                text.close()
            if codec is not None:
                codec.close()
            self.src.close()
