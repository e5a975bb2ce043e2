"""The read loop of run_amplipy (AmpliPy.py:896-915) as one object: what every I/O path of ``drivers`` shares while it walks its
input -- the engine, the insertion events, the counters of the progress lines and the shares, the pending ``Rec`` objects of the
Python codec -- and the one host-side statement of which trimmed reads are kept (A:910).  Nothing here opens a file."""
from __future__ import annotations

import sys
from datetime import datetime

import numpy as np

from . import abi
from .batch import ReadBatch
from .insertions import EventStore

PROGRESS_NUM_READS = 50000          # AmpliPy.py:19
BATCH_READS = 1 << 18              # reads per device batch on the Python-codec path (one Rec object each)


def print_log(s="", end="\n"):
    print("[%s] %s" % (datetime.now().strftime("%Y-%m-%d %H:%M:%S"), s), end=end, file=sys.stderr)
    sys.stderr.flush()


def error(s=None):
    print_log("ERROR" if s is None else "ERROR: %s" % s)
    sys.exit(1)


def keep_rows(ref_len, trim_flags, min_length, include_no_primer, first_bad=None):
    """AmpliPy.py:910 on arrays of a batch's results: a trimmed read is written when it still covers ``min_length`` reference bases
    and a primer was trimmed off it (or -e).  first_bad: the first row with a non-zero status -- nothing from it on is written, the
    rows in front of it are (A:907-911: the reference dies there).  The device encoders state the same rule on the C side."""
    keep = (ref_len >= min_length) & (((trim_flags & 3) != 0) | bool(include_no_primer))
    if first_bad is not None:
        keep[first_bad:] = False
    return keep


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


class ReadLoop:
    """n_seen, n_bases: records this rank has gone through (all of them when there is one rank) and the bases of those a BAM path
    took (the measure the shares of a multi-rank run should be equal in: SURVEY 8e).  s_i: the index of the last record seen (None:
    none yet), what "Finished Processing" prints.  read_base: rows the engine has taken, the id of the next batch's first read.
    ins_store: the insertion events with their allele text (each batch's bases are at hand only while it is on the device)."""

    def __init__(self, eng, min_length=None, include_no_primer=None, run_trim=False, do_count=False):
        self.eng, self.ins_store = eng, EventStore()
        self.min_length, self.include_no_primer, self.run_trim, self.do_count = min_length, include_no_primer, run_trim, do_count
        self.n_seen = self.n_bases = self.read_base = 0
        self.pending = []

    @property
    def s_i(self):
        return self.n_seen - 1 if self.n_seen else None

    def progress(self, count):
        """The next ``count`` records are seen: their progress lines (A:897-899: one in front of every record whose index is a
        multiple of PROGRESS_NUM_READS, record 0 excepted)."""
        k = self.n_seen + (-self.n_seen) % PROGRESS_NUM_READS
        self.n_seen += count
        while k < self.n_seen:
            if k:
                print_log("Processed %d reads..." % k)
            k += PROGRESS_NUM_READS

    def keep(self, res, first_bad=None):
        return keep_rows(res.ref_len, res.trim_flags, self.min_length, self.include_no_primer, first_bad)

    def host_batch(self, batch):
        """A batch packed on the host through the read pass: its results and its first row with a status (None: none has one).  The
        caller writes the kept rows, then calls ``batch_done``."""
        res = self.eng.process(batch, read_base=self.read_base)
        bad = np.nonzero(res.status)[0]
        return res, int(bad[0]) if len(bad) else None

    def batch_done(self, n, res, first_bad):
        """Behind the writing: the reference dies on the first read with a status with an uncaught exception, having written every
        read in front of it (A:907-911).  Then this batch's events only: the list is drained batch by batch (read ids are 32-bit
        and relative to read_base modulo 2^32, which a batch never spans)."""
        if first_bad is not None:
            _raise_for_status(res.status[first_bad])
        if self.do_count:
            _store_events(self.eng, self.ins_store, self.read_base)
        self.read_base += n

    def flush(self, writer=None):
        """The pending Rec objects as one batch; the kept ones to ``writer`` with their new POS and CIGAR."""
        pending = self.pending
        if not pending:
            return
        res, first_bad = self.host_batch(ReadBatch.from_segments([r.to_segment() for r in pending]))
        if self.run_trim and writer is not None:
            for k in np.nonzero(self.keep(res, first_bad))[0].tolist():
                writer.write(pending[k], pos=int(res.new_pos[k]), cigar=res.cigar_ops(k))
        self.batch_done(len(pending), res, first_bad)
        del pending[:]

    def python_records(self, recs, writer=None, rank=0, world=1):
        """Records through the Python codec (a reader's, or those a device codec handed back): the skip of A:902, the progress
        lines (progress() for one record, without the call), batches of BATCH_READS through flush().  world > 1: text input has
        no record index, the reads are dealt out."""
        pending, n = self.pending, self.n_seen               # (the count on a local: this is the loop with a turn per read)
        try:
            for rec in recs:
                if n % PROGRESS_NUM_READS == 0 and n:
                    print_log("Processed %d reads..." % n)
                n += 1
                if (rec.flag & 4) or rec.cigar is None:            # AmpliPy.py:902
                    continue
                if world > 1 and (n - 1) % world != rank:
                    continue
                pending.append(rec)
                if len(pending) >= BATCH_READS:
                    self.flush(writer)
        finally:
            self.n_seen = n
        self.flush(writer)

    def device_piece(self, codec, info, emit=None, defer=False):
        """A piece or chunk whose batch a device codec has built (info: n_records, n_rows, n_bases): counted, through the read pass
        where it lies, ``emit`` run on its results, its events stored.  defer: the read pass is only enqueued, ``emit`` works from
        the verdict where it lies and brings it down with its own wait (sam_native.SamCodec.encode)."""
        self.progress(int(info.n_records))
        if info.n_rows == 0:
            return
        self.n_bases += int(info.n_bases)
        if defer:
            codec.process(self.read_base, defer=True)
            emit()
            bad_row, bad_status = codec.verdict()
        else:
            bad_row, bad_status = codec.process(self.read_base)
            if emit is not None:
                emit()
        if bad_row >= 0:                  # the rows in front of it are written (A:907-911)
            _raise_for_status(bad_status)
        if self.do_count:
            _store_events(self.eng, self.ins_store, self.read_base, dev_reads=codec.dev_reads())
        self.read_base += int(info.n_rows)
