"""Read haplotypes per region of the command line (--haplotypes, --hap_out): the loader of the region file,
the device's entries decoded to text, what the tables say per region -- the haplotype table (--hap_out) and the HAP_N and HAP
keys of a VCF record -- and the merge of the ranks' tables.  The numbers themselves come from the engine (lib.Engine.hap_tables):
nothing here looks at a read.

The region file is a BED (ref, start, end, name): 0-BASED AND HALF-OPEN, as every BED.  The MUTATIONS of a haplotype are written
1-BASED, in the grammar of the mutation-set file of --cooc (cooc.py): A23403G, del21765-21770, del21991 -- a row found here can
be pasted into a --cooc file for the next run.  A read base N is written A123N, which --cooc does not take.  Insertions are not
part of a haplotype: two reads that differ only by an insertion fall together; the insertion alleles are in the VCF.

The device takes the regions sorted by start; the file's order is kept for every output: ``Regions.order`` translates."""
from __future__ import annotations

import gzip
from os.path import isfile

import numpy as np

from . import abi, parallel
from .cooc import BAD_NAME_CHARS
from .readloop import error, print_log
from .reports import Report

KINDS = "ACGTN"
KEYS = ("HAP_N", "HAP")
HEADER_LINES = (
    "##INFO=<ID=HAP_N,Number=1,Type=Integer,Description=\"Read haplotypes of the regions that hold the position, at or above the variant frequency, "
    "that carry an alternate base of this record there (or a deletion over it when - is an alternate)\">\n"
    "##INFO=<ID=HAP,Number=1,Type=String,Description=\"The commonest of them: region:mutations (1-based, joined by +):reads:usable reads of the region\">\n")
COLUMNS = ["ref", "region", "start", "end", "haplotype", "reads", "reverse", "usable", "frequency", "cover", "lowq", "overflow", "edge"]
REF_TEXT = "ref"


class Regions:
    """rows: [(start, end, name)] in file order (0-based, half-open).  For the device: ``order[k]``: the file index of device
    region k (sorted by start, the file's order among equal starts); ``starts``, ``ends``: int32 in device order; ``row[i]``: the
    device region of file row i."""

    def __init__(self, rows, ref_len):
        self.rows = [(int(s), int(e), str(n)) for s, e, n in rows]
        self.ref_len = int(ref_len)
        self.order = sorted(range(len(self.rows)), key=lambda i: (self.rows[i][0], i))
        self.row = {i: k for k, i in enumerate(self.order)}
        self.starts = np.array([self.rows[i][0] for i in self.order], np.int32)
        self.ends = np.array([self.rows[i][1] for i in self.order], np.int32)

    @property
    def n(self):
        return len(self.rows)

    def holding(self, pos):
        """The file rows whose region holds 0-based ``pos``, in file order."""
        return [i for i, (s, e, _) in enumerate(self.rows) if s <= pos < e]


def parse_regions(text, ref_id, ref_len, what="region file"):
    rows, seen = [], set()
    for no, l in enumerate(text.splitlines(), 1):
        l = l.rstrip("\r")
        if not l.strip() or l.startswith("#") or l.startswith("track") or l.startswith("browser"):
            continue
        where = "%s, line %d" % (what, no)
        parts = l.split("\t")
        try:
            if len(parts) < 3:
                raise ValueError
            s, e = int(parts[1]), int(parts[2])
        except ValueError:
            error("%s: not 'ref <tab> start <tab> end [<tab> name]' (0-based, half-open): %s" % (where, l))
        if parts[0].strip() != ref_id:
            error("%s: the region lies on %s, the reference is %s" % (where, parts[0].strip(), ref_id))
        if s < 0 or e > ref_len or e <= s:
            error("%s: [%d, %d) is empty or lies outside the reference of %d bases (a BED is 0-based and half-open)" % (where, s, e, ref_len))
        if e - s > abi.HAP_MAX_REGION:
            error("%s: the region has %d positions; at most %d" % (where, e - s, abi.HAP_MAX_REGION))
        name = parts[3].strip() if len(parts) > 3 and parts[3].strip() else "region%d" % (len(rows) + 1)
        if any(ch.isspace() or ch in BAD_NAME_CHARS for ch in name):
            error("%s: region name with whitespace or with one of '%s': %r" % (where, BAD_NAME_CHARS, name))
        if name in seen:
            error("%s: region name used twice: %s" % (where, name))
        seen.add(name)
        rows.append((s, e, name))
    if not rows:
        error("No region in %s" % what)
    if len(rows) > abi.HAP_MAX_REGIONS:
        error("%s has %d regions; at most %d" % (what, len(rows), abi.HAP_MAX_REGIONS))
    return Regions(rows, ref_len)


def load_regions(fn, ref_id, ref_len):
    """The region BED (ref, start, end[, name]; 0-based, half-open; .gz allowed; '#', track and browser lines skipped) -> Regions."""
    if not isfile(fn):
        error("File not found: %s" % fn)
    with (gzip.open(fn, "rt") if fn.lower().endswith(".gz") else open(fn)) as f:
        return parse_regions(f.read(), ref_id, ref_len, "file %s" % fn)


def enable(eng, regions, ref_seq, log2_capacity=None):
    eng.hap_enable(regions.starts, regions.ends, ref_seq, log2_capacity or 0)


# ---- entries ----------------------------------------------------------------------------------------------------------------
def decode(entry):
    """An abi.HAP_ENTRY_DTYPE record -> (device region, [(offset, kind, deletion length)], count, rev)."""
    head = int(entry["head"])
    n = head >> 16
    words = [int(w) for w in entry["diff"][:n]]
    return head & 0xFFFF, [(w & 0xFFF, (w >> 12) & 7, (w >> 15) & 0x1FFF) for w in words], int(entry["count"]), int(entry["rev"])


def mutation_text(region_start, diff, ref_seq):
    """One difference in the grammar of cooc.parse_mutation, 1-based: A23403G, del21765-21770, del21991; A123N for a base N."""
    off, kind, length = diff
    p = region_start + off
    if kind == abi.HAP_KIND_DEL:
        return "del%d" % (p + 1) if length == 1 else "del%d-%d" % (p + 1, p + length)
    return "%s%d%s" % (ref_seq[p].upper(), p + 1, KINDS[kind])


def entry_key(entry):
    return (int(entry["head"]),) + tuple(int(w) for w in entry["diff"])


def merge_entries(parts):
    """The per-key sum of several tables (abi.HAP_ENTRY_DTYPE arrays), ordered by the 14 key words: the ranks' tables on rank 0."""
    t = {}
    for ev in parts:
        for e in np.asarray(ev, abi.HAP_ENTRY_DTYPE):
            c = t.setdefault(entry_key(e), [0, 0])
            c[0] += int(e["count"])
            c[1] += int(e["rev"])
    out = np.zeros(len(t), abi.HAP_ENTRY_DTYPE)
    for k, key in enumerate(sorted(t)):
        out[k] = (key[0], key[1:], t[key][0], t[key][1])
    return out


def check_lost(lost):
    """Reads whose haplotype the device table had no slot for: never a silent loss."""
    if int(lost) > 0:
        raise RuntimeError("The haplotype table was full: %d reads whose haplotype found no slot were dropped; "
                           "rerun with a larger table (--hap_capacity, log2 of its slots)" % int(lost))


class Haplotype:
    __slots__ = ("text", "diffs", "start", "reads", "reverse")

    def __init__(self, text, diffs, start, reads, reverse):
        self.text, self.diffs, self.start, self.reads, self.reverse = text, diffs, start, reads, reverse

    def substitutions_at(self, pos):
        return [KINDS[k] for off, k, l in self.diffs if k != abi.HAP_KIND_DEL and self.start + off == pos]

    def deletes(self, pos):
        return any(k == abi.HAP_KIND_DEL and self.start + off <= pos < self.start + off + l for off, k, l in self.diffs)


class Tables:
    """The job's tables on the host, next to the regions: entries abi.HAP_ENTRY_DTYPE, tally uint64[n_regions][6] in the device's
    order of regions, reads uint64[2] (reads that cover a region, other reads), lost (reads whose key found no slot).  min_reads,
    min_freq: what --hap_out lists; vcf_min_freq: the variant frequency threshold, which HAP_N and HAP use.  The invariant of
    DESIGN.md section 22 is asserted here: per region COVER is REF + LOWQ + OVERFLOW + EDGE + the entries' counts + its lost reads."""

    def __init__(self, regions, ref_seq, entries, tally, reads, lost=0, min_reads=2, min_freq=0.0, vcf_min_freq=0.0):
        self.regions = regions
        self.ref = ref_seq
        self.tally = np.asarray(tally, np.uint64).reshape(regions.n, abi.HAP_TALLY_COLS)
        self.reads = np.asarray(reads, np.uint64).reshape(2)
        self.lost = int(lost)
        self.min_reads, self.min_freq, self.vcf_min_freq = int(min_reads), float(min_freq), float(vcf_min_freq)
        self.haps = [[] for _ in regions.rows]          # per file row
        held = [0] * regions.n
        for e in np.asarray(entries, abi.HAP_ENTRY_DTYPE):
            k, diffs, count, rev = decode(e)
            if k >= regions.n or not diffs or rev > count:
                raise ValueError("haplotype entry of region %d with %d differences, %d reads, %d reverse" % (k, len(diffs), count, rev))
            i = regions.order[k]
            start = regions.rows[i][0]
            held[k] += count
            self.haps[i].append(Haplotype(",".join(mutation_text(start, d, ref_seq) for d in diffs), diffs, start, count, rev))
        for h in self.haps:
            h.sort(key=lambda x: (-x.reads, x.text))
        t = self.tally.astype(np.int64)
        rest = t[:, abi.HAP_COVER] - t[:, [abi.HAP_REF, abi.HAP_LOWQ, abi.HAP_OVERFLOW, abi.HAP_EDGE]].sum(axis=1) - np.array(held, np.int64)
        if (rest < 0).any() or int(rest.sum()) != self.lost or (t[:, abi.HAP_REF_REV] > t[:, abi.HAP_REF]).any():
            raise ValueError("haplotype tables break their invariant: per region, cover minus what is accounted for: %s; lost reads: %d" % (rest.tolist(), self.lost))

    def cols(self, i):
        """The six tally columns of file row i."""
        return [int(x) for x in self.tally[self.regions.row[i]]]

    def usable(self, i):
        c = self.cols(i)
        return c[abi.HAP_COVER] - c[abi.HAP_LOWQ] - c[abi.HAP_OVERFLOW] - c[abi.HAP_EDGE]

    def frequency(self, i, reads):
        u = self.usable(i)
        return reads / u if u > 0 else None

    def rows(self, i):
        """[(text, reads, reverse)] of file row i as --hap_out lists them: the ref row always, a haplotype at or above both
        thresholds; by reads descending, then by text."""
        c = self.cols(i)
        out = [(REF_TEXT, c[abi.HAP_REF], c[abi.HAP_REF_REV])]
        for h in self.haps[i]:
            f = self.frequency(i, h.reads)
            if h.reads >= self.min_reads and (f if f is not None else 0.0) >= self.min_freq:
                out.append((h.text, h.reads, h.reverse))
        return sorted(out, key=lambda x: (-x[1], x[0]))

    def counting(self, pos, alts):
        """[(file row, Haplotype)] that count for a record at 0-based ``pos`` with the alternates ``alts``: by reads descending,
        then by file row, then by text."""
        out = []
        for i in self.regions.holding(pos):
            for h in self.haps[i]:
                f = self.frequency(i, h.reads)
                if h.reads < self.min_reads or f is None or f < self.vcf_min_freq:
                    continue
                if any(b in alts for b in h.substitutions_at(pos)) or ("-" in alts and h.deletes(pos)):
                    out.append((i, h))
        return sorted(out, key=lambda x: (-x[1].reads, x[0], x[1].text))

    def info(self, pos, ref, alts):
        """'HAP_N=..;HAP=..' of a record at 0-based ``pos``."""
        c = self.counting(pos, alts)
        if not c:
            return "HAP_N=0;HAP=."
        i, h = c[0]
        return "HAP_N=%d;HAP=%s:%s:%d:%d" % (len(c), self.regions.rows[i][2], h.text.replace(",", "+"), h.reads, self.usable(i))

    def summary_line(self):
        return "Haplotypes: %d reads cover a region, %d other reads; %d regions, %d distinct haplotypes" % (
            int(self.reads[0]), int(self.reads[1]), self.regions.n, sum(len(h) for h in self.haps))


def write_tsv(f, ref_id, tables):
    """A header line, then per region (file order) one line per listed haplotype (Tables.rows): ref, region, start, end (as the BED
    has them: 0-based, half-open), haplotype (mutations 1-based, comma-separated; 'ref'), reads, reverse, usable = cover - lowq -
    overflow - edge, frequency = reads / usable ('.' when usable is 0), cover, lowq, overflow, edge."""
    f.write("#" + "\t".join(COLUMNS) + "\n")
    out = []
    for i, (s, e, name) in enumerate(tables.regions.rows):
        c = tables.cols(i)
        u = tables.usable(i)
        for text, reads, rev in tables.rows(i):
            out.append("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (
                ref_id, name, s, e, text, reads, rev, u, "%.6g" % (reads / u) if u > 0 else ".", c[abi.HAP_COVER], c[abi.HAP_LOWQ], c[abi.HAP_OVERFLOW],
                c[abi.HAP_EDGE]))
    f.write("".join(out))


class HapReport(Report):
    name, HEADER_LINES, outputs = "hap", HEADER_LINES, (("hap_out_fn", "haplotype table", write_tsv),)
    regions = None

    def active(self, run):
        return run.haplotypes_fn is not None

    def check(self, run):
        if run.haplotypes_fn is None and (run.hap_out_fn is not None or run.hap_capacity is not None):
            error("The haplotype table and its size (--hap_out, --hap_capacity) need the region file (--haplotypes)")
        if run.haplotypes_fn is not None and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no read haplotypes (--haplotypes, --hap_out)")
        if run.hap_capacity is not None and not abi.HAP_LOG2_MIN <= run.hap_capacity <= abi.HAP_LOG2_MAX:
            error("--hap_capacity is the log2 of the table's slots, %d to %d: %s" % (abi.HAP_LOG2_MIN, abi.HAP_LOG2_MAX, run.hap_capacity))
        if run.hap_min_reads is not None and run.hap_min_reads < 0:
            error("--hap_min_reads must be non-negative: %s" % run.hap_min_reads)
        if run.hap_min_freq is not None and not 0 <= run.hap_min_freq <= 1:
            error("--hap_min_freq must be between 0 and 1: %s" % run.hap_min_freq)

    def load(self, run):
        print_log("Loading haplotype regions: %s" % run.haplotypes_fn)
        self.regions = load_regions(run.haplotypes_fn, run.ref_id, run.G)

    def enable(self, run, eng):
        enable(eng, self.regions, run.ref_seq, run.hap_capacity)

    def collect(self, run, eng):
        entries, info, tally, reads = eng.hap_tables()
        self.lost = info["lost"]
        if run.dist is not None:              # every rank's entries and tallies to rank 0, which sums them on the host
            parts = parallel.gather_objects(run.dist, run.rank, run.world, (entries, info, tally, reads))
            if run.rank == 0:
                entries = merge_entries([part[0] for part in parts])
                self.lost = sum(part[1]["lost"] for part in parts)
                tally, reads = parallel.sum_reads([part[2] for part in parts]), parallel.sum_reads([part[3] for part in parts])
        if run.rank == 0:
            self.tables = Tables(self.regions, run.ref_seq, entries, tally, reads, self.lost, 2 if run.hap_min_reads is None else run.hap_min_reads,
                                 run.hap_min_freq or 0.0, run.v_min_freq)

    def after(self, run):
        check_lost(self.lost)                 # (behind the run's last collective: no rank is left waiting)
