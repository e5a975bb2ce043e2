"""Deletion events of the command line (--deletions, --del_out, --indel_vcf): the two INFO keys of a VCF
record, the per-event TSV file, and the second VCF of anchored indels.  The events come from the engine
(lib.Engine.del_events), the depths from the count table, the insertion alleles from the call's own records: nothing here looks
at a read.  An event is (start, len, count, rev): ``count`` reads -- ``rev`` of them on the reverse strand -- skipped the ``len``
reference positions from 0-based ``start`` on together."""
from __future__ import annotations

import bisect
import sys

import numpy as np

from . import abi, parallel
from .readloop import error
from .reports import Report

KEYS = ("DEL_N", "DEL")
HEADER_LINES = (
    "##INFO=<ID=DEL_N,Number=1,Type=Integer,Description=\"Distinct deletion events covering the position\">\n"
    "##INFO=<ID=DEL,Number=.,Type=String,Description=\"Deletion events covering the position at or above the variant frequency: first-last:reads:reverse-strand reads, 1-based and inclusive, by descending reads\">\n")
TSV_COLUMNS = ["ref", "start", "length", "count", "rev", "depth", "freq", "deleted"]
INDEL_INFO_LINES = (
    "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth at the first deleted position (deletions: A C G T N and deleted together) or at the anchor (insertions: insertion alleles included)\">\n"
    "##INFO=<ID=AD,Number=1,Type=Integer,Description=\"Reads that carry the allele\">\n"
    "##INFO=<ID=RV,Number=1,Type=Integer,Description=\"Those of them on the reverse strand (deletions only)\">\n"
    "##INFO=<ID=AF,Number=1,Type=Float,Description=\"AD / DP\">\n")
INDEL_NOTE = ("##AmpliPyIndels=Deletions are read-level events (positions one read skipped together, D and N ops alike), insertions the "
              "alleles of the variant call; each is written as the aligner placed it: no left-alignment, no normalisation across aligners\n")


def merge_events(parts):
    """The per-key sum of several tables (abi.DEL_EVENT_DTYPE arrays), ordered by (start, len): the ranks' tables on rank 0."""
    t = {}
    for ev in parts:
        for e in np.asarray(ev, abi.DEL_EVENT_DTYPE).tolist():
            c = t.setdefault((e[0], e[1]), [0, 0])
            c[0] += e[2]
            c[1] += e[3]
    out = np.zeros(len(t), abi.DEL_EVENT_DTYPE)
    for k, key in enumerate(sorted(t)):
        out[k] = (key[0], key[1], t[key][0], t[key][1])
    return out


def check_lost(lost):
    """Reads of events the device table had no slot for: never a silent loss."""
    if int(lost) > 0:
        raise RuntimeError("The deletion events' table was full: %d reads of events that found no slot were dropped; "
                           "rerun with a larger table (--del_capacity, log2 of its slots)" % int(lost))


class Tables:
    """The job's events and its count table on the host: events abi.DEL_EVENT_DTYPE ordered by (start, len), counts
    uint32[G][6]; the variant thresholds decide what DEL lists and what the indel VCF holds."""

    def __init__(self, events, counts, ref_seq, min_depth=0, min_freq=0.0):
        ev = np.asarray(events, abi.DEL_EVENT_DTYPE)
        self.events = ev[np.lexsort((ev["len"], ev["start"]))]
        self.counts = np.asarray(counts).reshape(-1, abi.NSYM)
        self.ref = ref_seq
        self.min_depth, self.min_freq = min_depth, min_freq
        self._rows = [(int(s), int(l), int(c), int(r)) for s, l, c, r in self.events.tolist()]
        self._starts = [r[0] for r in self._rows]
        self._max_len = max((r[1] for r in self._rows), default=0)
        G = len(self.counts)
        for s, l, c, r in self._rows:
            if not (0 <= s and l >= 1 and s + l <= G and 0 <= r <= c):
                raise ValueError("deletion event outside the reference or with more reverse reads than reads: %r" % ((s, l, c, r),))

    def covering(self, pos):
        """The events with start <= pos < start + len, in table order."""
        lo = bisect.bisect_left(self._starts, pos - self._max_len + 1)
        hi = bisect.bisect_right(self._starts, pos)
        return [r for r in self._rows[lo:hi] if r[0] + r[1] > pos]

    def depth(self, pos):
        return int(self.counts[pos].sum())

    def info(self, pos, dp):
        """'DEL_N=..;DEL=..' of a record at 0-based ``pos`` whose total depth is ``dp``."""
        cov = self.covering(pos)
        shown = sorted((r for r in cov if dp > 0 and r[2] / dp >= self.min_freq), key=lambda r: (-r[2], r[0], r[1]))
        return "DEL_N=%d;DEL=%s" % (len(cov), ",".join("%d-%d:%d:%d" % (s + 1, s + l, c, r) for s, l, c, r in shown) or ".")

    def deleted_text(self, start, length):
        return self.ref[start:start + length]

    def called(self):
        """The events the indel VCF holds: depth at ``start`` >= min_depth and count / depth >= min_freq."""
        out = []
        for s, l, c, r in self._rows:
            d = self.depth(s)
            if d >= self.min_depth and d > 0 and c / d >= self.min_freq:
                out.append((s, l, c, r, d))
        return out


def write_tsv(f, ref_id, tables):
    """A header line, then one line per event: ref_id, start + 1, length, count, rev, depth at start, frequency, deleted text."""
    f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
    lines = []
    for s, l, c, r in tables._rows:
        d = tables.depth(s)
        lines.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (ref_id, s + 1, l, c, r, d, "%.6g" % (c / d) if d else ".", tables.deleted_text(s, l)))
    f.write("".join(lines))


def insertion_rows(records):
    """[(0-based pos, allele, count, depth)] of the insertion alleles in the call's records (calling.VariantRecord): the ALTs
    of more than one letter, which passed the variant thresholds there."""
    out = []
    for r in records:
        for alt, n in zip(r.alts, r.ALT_DP.split(",")):
            if len(alt) > 1:
                out.append((r.pos, alt, int(n), int(r.DP)))
    return out


def indel_records(tables, insertions=()):
    """[(POS, REF, ALT, INFO)] of the indel VCF, by position (at one position deletions first, shorter first, then
    insertions by allele).  A deletion is anchored at the base in front of it; one that starts at the first base of the
    reference at the base behind it, as the VCF specification prescribes."""
    ref = tables.ref
    rows = []
    for s, l, c, r, d in tables.called():
        if s == 0 and l >= len(ref):
            continue                        # (nothing of the reference is left to anchor it at)
        if s > 0:
            pos, ref_text, alt = s, ref[s - 1:s + l], ref[s - 1]
        else:
            pos, ref_text, alt = 1, ref[0:l + 1], ref[l:l + 1]
        rows.append((pos, 0, l, "", ref_text, alt, "DP=%d;AD=%d;RV=%d;AF=%.6g" % (d, c, r, c / d)))
    for p, allele, n, dp in insertions:
        if dp >= tables.min_depth and dp > 0 and n / dp >= tables.min_freq:
            rows.append((p + 1, 1, 0, allele, ref[p], allele, "DP=%d;AD=%d;RV=.;AF=%.6g" % (dp, n, n / dp)))
    rows.sort(key=lambda x: x[:4])
    return [(x[0], x[4], x[5], x[6]) for x in rows]


def write_indel_vcf(f, ref_id, tables, insertions=(), source=""):
    """The second VCF: spec-valid VCF 4.2 records of anchored indels, by position."""
    f.write("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n")
    if source:
        f.write("##source=%s\n" % source)
    f.write("##contig=<ID=%s,length=%d>\n" % (ref_id, len(tables.ref)))
    f.write(INDEL_NOTE + INDEL_INFO_LINES)
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    f.write("".join(["%s\t%d\t.\t%s\t%s\t.\tPASS\t%s\n" % (ref_id, pos, r, a, info) for pos, r, a, info in indel_records(tables, insertions)]))


class DeletionReport(Report):
    """--deletions puts the keys on the VCF; --del_out or --indel_vcf alone switch the hook on too.  The indel VCF takes the
    call's insertion alleles, so both files are written beside the VCF."""
    name, HEADER_LINES, with_calls = "deletion", HEADER_LINES, True
    outputs = (("indel_vcf_fn", "indel VCF", write_indel_vcf), ("del_out_fn", "deletion events", write_tsv))

    def active(self, run):
        return bool(run.deletions) or run.del_out_fn is not None or run.indel_vcf_fn is not None

    def check(self, run):
        on = self.active(run)
        if on and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no deletion events (--deletions, --del_out, --indel_vcf)")
        if run.deletions and not run.run_variants:
            error("The deletion INFO keys need a VCF (--deletions on variants or aio)")
        if run.indel_vcf_fn is not None and not run.run_variants:
            error("The indel VCF (--indel_vcf) uses the variant thresholds: variants or aio")
        if run.del_capacity is not None and not on:
            error("The deletion events' table size (--del_capacity) needs --deletions, --del_out or --indel_vcf")
        if run.del_capacity is not None and not abi.DEL_LOG2_MIN <= run.del_capacity <= abi.DEL_LOG2_MAX:
            error("--del_capacity is the log2 of the table's slots, %d to %d: %s" % (abi.DEL_LOG2_MIN, abi.DEL_LOG2_MAX, run.del_capacity))
        if run.indel_vcf_fn is not None and not run.indel_vcf_fn.lower().endswith((".vcf", ".vcf.gz")):
            error("Invalid indel VCF extension (should be .vcf or .vcf.gz): %s" % run.indel_vcf_fn)

    def enable(self, run, eng):
        eng.del_enable(run.del_capacity or 0)

    def collect(self, run, eng):
        events, info = eng.del_events()
        self.lost = info["lost"]
        if run.dist is not None:              # every rank's events to rank 0, which sums them per key on the host
            parts = parallel.gather_objects(run.dist, run.rank, run.world, (events, info))
            if run.rank == 0:
                events = merge_events([part[0] for part in parts])
                self.lost = sum(part[1]["lost"] for part in parts)
        if run.rank == 0:
            self.tables = Tables(events, eng.counts(), run.ref_seq, run.v_min_depth, run.v_min_freq)

    def annotates(self, run):
        return bool(run.deletions)

    def writer_args(self, arg, run, res):
        more = (insertion_rows(res.records), " ".join(sys.argv)) if arg == "indel_vcf_fn" else ()
        return (run.ref_id, self.tables) + more

    def after(self, run):
        check_lost(self.lost)                 # (behind the run's last collective: no rank is left waiting)
