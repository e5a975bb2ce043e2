"""Deletion events of the command line (--deletions, --del_out, --indel_vcf): the two INFO keys of a VCF
record, the per-event TSV file, and the second VCF of anchored indels.  The events come from the engine
(lib.Engine.del_events), the depths from the count table, the insertion alleles from the call's own records: nothing here looks
at a read.  An event is (start, len, count, rev): ``count`` reads -- ``rev`` of them on the reverse strand -- skipped the ``len``
reference positions from 0-based ``start`` on together."""
from __future__ import annotations

import bisect
import sys

import numpy as np

from . import abi, insevidence, parallel
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


def indel_records(tables, insertions=(), evidence=None):
    """[(POS, REF, ALT, INFO)] of the indel VCF, by position (at one position deletions first, shorter first, then
    insertions by allele).  A deletion is anchored at the base in front of it; one that starts at the first base of the
    reference at the base behind it, as the VCF specification prescribes.  evidence: the insertion alleles' insevidence.Tables
    (--insertions, --ins_out) -- an insertion row then carries its reverse reads in RV."""
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
            rv = evidence.rev_of(p, allele) if evidence is not None else None
            rows.append((p + 1, 1, 0, allele, ref[p], allele, "DP=%d;AD=%d;RV=%s;AF=%.6g" % (dp, n, "." if rv is None else "%d" % rv, n / dp)))
    rows.sort(key=lambda x: x[:4])
    return [(x[0], x[4], x[5], x[6]) for x in rows]


def write_indel_vcf(f, ref_id, tables, insertions=(), source="", evidence=None):
    """The second VCF: spec-valid VCF 4.2 records of anchored indels, by position.  With ``evidence`` (the insertion half on)
    RV is declared for both kinds of record."""
    f.write("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n")
    if source:
        f.write("##source=%s\n" % source)
    f.write("##contig=<ID=%s,length=%d>\n" % (ref_id, len(tables.ref)))
    f.write(INDEL_NOTE + (INDEL_INFO_LINES if evidence is None else INDEL_INFO_LINES.replace(" (deletions only)", "")))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    f.write("".join(["%s\t%d\t.\t%s\t%s\t.\tPASS\t%s\n" % (ref_id, pos, r, a, info) for pos, r, a, info in indel_records(tables, insertions, evidence)]))


class IndelTables:
    """The tables of the indel unit on rank 0 when the insertion half is on: the deletion events' Tables (None with that half
    off) and the insertion alleles' insevidence.Tables (None when the device table lost events: no join)."""

    def __init__(self, deletion, insertion):
        self.deletion, self.insertion = deletion, insertion


class DeletionReport(Report):
    """The indel unit.  --deletions puts the deletion keys on the VCF; --del_out or --indel_vcf alone switch the deletion half
    on too.  The indel VCF takes the call's insertion alleles, so both files are written beside the VCF.  --insertions puts the
    insertion keys on the VCF and --ins_out writes the allele table: either switches the insertion half on (insevidence.py),
    and with it on the insertion rows of the indel VCF carry RV.  With the insertion flags off nothing of that half is called."""
    name, HEADER_LINES, with_calls = "deletion", HEADER_LINES, True
    outputs = (("indel_vcf_fn", "indel VCF", write_indel_vcf), ("del_out_fn", "deletion events", write_tsv),
               ("ins_out_fn", "insertion alleles", insevidence.write_tsv))
    ins_lost = 0

    @staticmethod
    def del_on(run):
        return bool(run.deletions) or run.del_out_fn is not None or run.indel_vcf_fn is not None

    @staticmethod
    def ins_on(run):
        return bool(getattr(run, "insertions", False)) or getattr(run, "ins_out_fn", None) is not None

    def active(self, run):
        return self.del_on(run) or self.ins_on(run)

    def check(self, run):
        on = self.del_on(run)
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
        ins, cap, end = self.ins_on(run), getattr(run, "ins_capacity", None), getattr(run, "ins_end", None)
        if ins and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no insertion events: no insertion evidence (--insertions, --ins_out)")
        if getattr(run, "insertions", False) and not run.run_variants:
            error("The insertion INFO keys need a VCF (--insertions on variants or aio)")
        if cap is not None and not ins:
            error("The insertion evidence table's size (--ins_capacity) needs --insertions or --ins_out")
        if cap is not None and not abi.INSEV_LOG2_MIN <= cap <= abi.INSEV_LOG2_MAX:
            error("--ins_capacity is the log2 of the table's slots, %d to %d: %s" % (abi.INSEV_LOG2_MIN, abi.INSEV_LOG2_MAX, cap))
        if end is not None and not ins:
            error("The read-end distance of the insertion keys (--ins_end) needs --insertions or --ins_out")
        if end is not None and end not in insevidence.END_EDGES:
            error("--ins_end is one of %s: %s" % (", ".join("%d" % e for e in insevidence.END_EDGES), end))

    def enable(self, run, eng):
        if self.del_on(run):
            eng.del_enable(run.del_capacity or 0)
        if self.ins_on(run):
            eng.insev_enable(run.ins_capacity or 0)

    def collect(self, run, eng):
        del_tables = None
        if self.del_on(run):
            events, info = eng.del_events()
            self.lost = info["lost"]
            if run.dist is not None:              # every rank's events to rank 0, which sums them per key on the host
                parts = parallel.gather_objects(run.dist, run.rank, run.world, (events, info))
                if run.rank == 0:
                    events = merge_events([part[0] for part in parts])
                    self.lost = sum(part[1]["lost"] for part in parts)
            if run.rank == 0:
                del_tables = Tables(events, eng.counts(), run.ref_seq, run.v_min_depth, run.v_min_freq)
        if not self.ins_on(run):
            self.tables = del_tables
            return
        # the insertion half: one more gather, issued by every rank whenever the flags are on -- the entries and every allele text
        # of the rank's share (the call exchanges the texts of the flagged positions only; the join wants them all)
        entries, info = eng.insev_entries()
        triples = run.ins_store.counted_pairs()
        self.ins_lost = info["lost"]
        if run.dist is not None:
            parts = parallel.gather_objects(run.dist, run.rank, run.world, (entries, info, triples))
            if run.rank == 0:
                entries = insevidence.merge_entries([part[0] for part in parts])
                self.ins_lost = sum(part[1]["lost"] for part in parts)
                triples = [t for part in parts for t in part[2]]
        if run.rank == 0 and not self.ins_lost:  # (a table that lost events cannot meet the store: after() says so)
            ins_tables = insevidence.Tables(entries, triples, eng.counts(), run.v_min_freq, run.ins_end or insevidence.END_DEFAULT)
            self.tables = IndelTables(del_tables, ins_tables)
        elif run.rank == 0:
            self.tables = IndelTables(del_tables, None)

    def annotates(self, run):
        return bool(run.deletions)

    def vcf_tables(self, run):
        t = self.tables
        if run.insertions:                        # (in front of the VCF's records: a table that lost events has no keys to give, and
            check_lost(self.lost)                 # a header that declares keys no record carries is not left behind)
            insevidence.check_lost(self.ins_lost)
        if not isinstance(t, IndelTables):
            return super().vcf_tables(run)
        d = t.deletion if self.annotates(run) else None
        i = t.insertion if run.insertions else None
        return d if i is None else insevidence.IndelInfo(d, i)

    def writer_args(self, arg, run, res):
        t = self.tables
        d, i = (t.deletion, t.insertion) if isinstance(t, IndelTables) else (t, None)
        if arg == "indel_vcf_fn":
            return (run.ref_id, d, insertion_rows(res.records), " ".join(sys.argv)) + ((i,) if i is not None else ())
        return run.ref_id, (i if arg == "ins_out_fn" else d)

    def write(self, run, res):
        if self.ins_lost:                         # (no join: the files of the indel unit are not written; every rank's after() raises)
            check_lost(self.lost)
            insevidence.check_lost(self.ins_lost)
        super().write(run, res)

    def after(self, run):
        check_lost(self.lost)                 # (behind the run's last collective: no rank is left waiting)
        insevidence.check_lost(self.ins_lost)
