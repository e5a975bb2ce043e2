"""Codon tallies of the command line (--codons): the loader of the CDS file, the codon slots the engine
takes (lib.Engine.codon_enable), the standard genetic code, and what the table says per CDS row: the five INFO keys of a VCF
record, the codon table (--codon_out) and the amino-acid calls (--aa_out).  The numbers themselves come from the engine
(lib.Engine.codon_tables): nothing here looks at a read.  The device knows the slots' start positions only; names, strands and
translation stay here."""
from __future__ import annotations

from os.path import isfile

import numpy as np

from . import abi, parallel
from .readloop import error, print_log
from .reports import Report

BAD_NAME_CHARS = ",;=|:"
BASES = "ACGT"
CELLS = abi.CODON_CELLS
BROKEN = 64
KEYS = ("CDS", "CODON_DP", "ALT_AA", "ALT_CODON", "ALT_CODON_DP")
HEADER_LINES = (
    "##INFO=<ID=CDS,Number=.,Type=String,Description=\"CDS rows that cover the position (|)\">\n"
    "##INFO=<ID=CODON_DP,Number=.,Type=String,Description=\"Reads that show all three bases of the position's codon, per listed CDS row (|)\">\n"
    "##INFO=<ID=ALT_AA,Number=.,Type=String,Description=\"Amino-acid change of the commonest codon read with the alternate base, per alternate base (comma) and listed CDS row (|)\">\n"
    "##INFO=<ID=ALT_CODON,Number=.,Type=String,Description=\"Reference codon > that codon, on the row's strand, per alternate base (comma) and listed CDS row (|)\">\n"
    "##INFO=<ID=ALT_CODON_DP,Number=.,Type=String,Description=\"Reads that carry that codon, per alternate base (comma) and listed CDS row (|)\">\n")
CODON_COLUMNS = ["ref", "cds", "codon_number", "pos", "ref_codon", "ref_aa", "codon", "aa", "count", "depth", "freq", "broken"]
AA_COLUMNS = ["ref", "cds", "change", "count", "depth", "freq", "codons"]

# the standard genetic code, TCAG order (NCBI translation table 1)
_AAS = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODE = {a + b + c: _AAS[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
TRIPLETS = [a + b + c for a in BASES for b in BASES for c in BASES]        # cell 16 b0 + 4 b1 + b2 -> its triplet, reference-forward


def translate(triplet):
    """The amino acid of a triplet on the coding strand; ``*`` a stop, ``X`` when a base is not one of A C G T."""
    return CODE.get(triplet.upper(), "X")


def revcomp(triplet):
    return "".join(_COMP.get(b, "N") for b in reversed(triplet.upper()))


class CdsSet:
    """rows: [(name, start, end, strand)] in file order (0-based, half-open); starts: int32, the slots -- the sorted,
    de-duplicated codon start positions of all rows."""

    def __init__(self, rows, ref_len):
        self.rows = list(rows)
        self.ref_len = int(ref_len)
        self.starts = build_slots(self.rows)
        self._slot = {int(s): k for k, s in enumerate(self.starts.tolist())}

    @property
    def n_slots(self):
        return int(self.starts.size)

    def slot_of(self, start):
        return self._slot[int(start)]

    def covering(self, pos):
        """The rows that cover 0-based pos, in file order."""
        return [r for r in self.rows if r[1] <= pos < r[2]]

    @staticmethod
    def codon_at(row, pos):
        """-> (codon start, offset of pos in the reference-forward triplet, 1-based codon number on the row's strand)."""
        _, start, end, strand = row
        p = start + 3 * ((pos - start) // 3)
        return p, pos - p, ((p - start) // 3 + 1) if strand == "+" else (end - p) // 3


def build_slots(rows):
    starts = set()
    for _, start, end, _ in rows:
        starts.update(range(start, end, 3))
    return np.array(sorted(starts), np.int32)


def parse_cds(text, ref_len, what="CDS file"):
    rows, seen = [], set()
    for l in text.splitlines():
        if not l.strip():
            continue
        parts = l.rstrip("\r").split("\t")
        if len(parts) < 3:
            error("Invalid CDS line (name <tab> start <tab> end [<tab> strand]): %s" % l)
        name = parts[0]
        if not name or any(ch.isspace() or ch in BAD_NAME_CHARS for ch in name):
            error("CDS name empty, with whitespace or with one of '%s': %r" % (BAD_NAME_CHARS, name))
        if name in seen:
            error("CDS name used twice: %s" % name)
        seen.add(name)
        try:
            start, end = int(parts[1]), int(parts[2])
        except ValueError:
            error("CDS %s: start and end must be integers: %s" % (name, l))
        strand = parts[3].strip() if len(parts) > 3 and parts[3].strip() else "+"
        if strand not in ("+", "-"):
            error("CDS %s: strand must be + or -, not %r" % (name, strand))
        if start < 0 or end > ref_len or start >= end:
            error("CDS %s: [%d, %d) is empty or outside the reference of %d bases" % (name, start, end, ref_len))
        if (end - start) % 3:
            error("CDS %s: its length %d is no multiple of 3" % (name, end - start))
        rows.append((name, start, end, strand))
    if not rows:
        error("No CDS in %s" % what)
    cds = CdsSet(rows, ref_len)
    if cds.n_slots > abi.CODON_MAX_SLOTS:
        error("The CDS rows have %d different codon positions; at most %d" % (cds.n_slots, abi.CODON_MAX_SLOTS))
    return cds


def load_cds(fn, ref_len):
    """The CDS file (name, start, end[, strand] per line; 0-based, half-open) -> CdsSet."""
    if not isfile(fn):
        error("File not found: %s" % fn)
    with open(fn) as f:
        return parse_cds(f.read(), ref_len, "file: %s" % fn)


def enable(eng, cds):
    eng.codon_enable(cds.starts)


class Tables:
    """The job's codon table on the host: codon uint32[n_slots][65], reads uint64[2] (tallied, skipped irregular reads), next to
    the CDS rows and the reference they are read against."""

    def __init__(self, cds, ref_seq, codon, reads, min_depth=0, min_freq=0.0):
        self.cds = cds
        self.ref = ref_seq.upper()
        self.codon = np.asarray(codon).reshape(cds.n_slots, CELLS)
        self.reads = np.asarray(reads, np.uint64).reshape(2)
        self.min_depth, self.min_freq = min_depth, min_freq

    def cells(self, start):
        return self.codon[self.cds.slot_of(start)].tolist()

    def on_strand(self, row, triplet):
        return triplet if row[3] == "+" else revcomp(triplet)

    def ref_codon(self, row, start):
        return self.on_strand(row, self.ref[start:start + 3])

    def info(self, pos, ref, alts):
        """'CDS=..;CODON_DP=..;ALT_AA=..;ALT_CODON=..;ALT_CODON_DP=..' of a record at 0-based ``pos``."""
        rows = self.cds.covering(pos)
        if not rows:
            dots = ",".join("." for _ in alts) if alts else "."
            return "CDS=.;CODON_DP=.;ALT_AA=%s;ALT_CODON=%s;ALT_CODON_DP=%s" % (dots, dots, dots)
        at = [self.cds.codon_at(r, pos) for r in rows]
        cells = [self.cells(p) for p, _, _ in at]
        aa, cod, dp = [], [], []
        for s in alts:
            b = BASES.find(s) if len(s) == 1 else -1
            if b < 0:
                aa.append("."); cod.append("."); dp.append(".")
                continue
            e_aa, e_cod, e_dp = [], [], []
            for row, (p, k, num), c in zip(rows, at, cells):
                best = -1
                for t in range(64):                 # the largest count; ties go to the smallest index
                    if (t >> (2 * (2 - k))) & 3 == b and c[t] > 0 and (best < 0 or c[t] > c[best]):
                        best = t
                if best < 0:
                    e_aa.append("."); e_cod.append("."); e_dp.append(".")
                    continue
                rc, ac = self.ref_codon(row, p), self.on_strand(row, TRIPLETS[best])
                e_aa.append("%s%d%s" % (translate(rc), num, translate(ac)))
                e_cod.append("%s>%s" % (rc, ac))
                e_dp.append(str(c[best]))
            aa.append("|".join(e_aa)); cod.append("|".join(e_cod)); dp.append("|".join(e_dp))
        return "CDS=%s;CODON_DP=%s;ALT_AA=%s;ALT_CODON=%s;ALT_CODON_DP=%s" % (
            "|".join(r[0] for r in rows), "|".join(str(sum(c[:64])) for c in cells),
            ",".join(aa) if aa else ".", ",".join(cod) if cod else ".", ",".join(dp) if dp else ".")

    def row_codons(self, row):
        """(codon number, codon start) of the row in the order of the codon numbers."""
        _, start, end, strand = row
        n = (end - start) // 3
        return [(j + 1, start + 3 * j) for j in range(n)] if strand == "+" else [(j + 1, end - 3 * (j + 1)) for j in range(n)]

    def summary_line(self):
        return "Codons: %d reads tallied, %d irregular reads skipped; %d codon positions of %d CDS rows" % (
            int(self.reads[0]), int(self.reads[1]), self.cds.n_slots, len(self.cds.rows))


def write_codon_tsv(f, ref_id, tables):
    """A header line, then per CDS row, codon (by number) and triplet with a count (ascending reference-forward cell): ref,
    cds, codon number, position of the codon's lowest base (1-based), reference codon and amino acid, codon and amino acid (on
    the row's strand), count, depth (the 64 triplet cells together), freq, broken (cell 64)."""
    f.write("#" + "\t".join(CODON_COLUMNS) + "\n")
    out = []
    for row in tables.cds.rows:
        for num, p in tables.row_codons(row):
            c = tables.cells(p)
            depth = sum(c[:64])
            rc = tables.ref_codon(row, p)
            for t in range(64):
                if c[t] > 0:
                    ac = tables.on_strand(row, TRIPLETS[t])
                    out.append("%s\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%d\t%d\t%g\t%d\n" % (
                        ref_id, row[0], num, p + 1, rc, translate(rc), ac, translate(ac), c[t], depth, c[t] / depth, c[BROKEN]))
    f.write("".join(out))


def aa_calls(tables):
    """[(cds, change, count, depth, freq, [(triplet on the row's strand, count)])]: per CDS row and codon every amino acid
    other than the reference's with depth >= min_depth and freq >= min_freq; largest count first, then by letter."""
    out = []
    for row in tables.cds.rows:
        for num, p in tables.row_codons(row):
            c = tables.cells(p)
            depth = sum(c[:64])
            if depth == 0 or depth < tables.min_depth:
                continue
            ref_aa = translate(tables.ref_codon(row, p))
            by_aa = {}
            for t in range(64):
                if c[t] > 0:
                    ac = tables.on_strand(row, TRIPLETS[t])
                    by_aa.setdefault(translate(ac), []).append((ac, c[t]))
            for aa, pairs in sorted(by_aa.items(), key=lambda kv: (-sum(n for _, n in kv[1]), kv[0])):
                count = sum(n for _, n in pairs)
                if aa == ref_aa or count / depth < tables.min_freq:
                    continue
                out.append((row[0], "%s%d%s" % (ref_aa, num, aa), count, depth, count / depth,
                            sorted(pairs, key=lambda x: -x[1])))          # (stable: equal counts stay in cell order)
    return out


def write_aa_tsv(f, ref_id, tables):
    """A header line, then one line per call of ``aa_calls``: ref, cds, change, count, depth, freq, codons (triplet:count,
    largest first)."""
    f.write("#" + "\t".join(AA_COLUMNS) + "\n")
    f.write("".join(["%s\t%s\t%s\t%d\t%d\t%g\t%s\n" % (ref_id, cds, change, count, depth, freq, ",".join("%s:%d" % x for x in pairs))
                     for cds, change, count, depth, freq, pairs in aa_calls(tables)]))


class CodonReport(Report):
    name, HEADER_LINES = "codon", HEADER_LINES
    outputs = (("codon_out_fn", "codon table", write_codon_tsv), ("aa_out_fn", "amino-acid calls", write_aa_tsv))
    cds = None

    def active(self, run):
        return run.codons_fn is not None

    def check(self, run):
        if (run.codon_out_fn is not None or run.aa_out_fn is not None) and run.codons_fn is None:
            error("The codon table and the amino-acid calls (--codon_out, --aa_out) need the CDS file (--codons)")
        if run.codons_fn is not None and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no codon tallies (--codons, --codon_out, --aa_out)")
        if run.aa_out_fn is not None and not run.run_variants:
            error("The amino-acid calls (--aa_out) use the variant thresholds: variants or aio")

    def load(self, run):
        print_log("Loading CDS rows: %s" % run.codons_fn)
        self.cds = load_cds(run.codons_fn, run.G)

    def enable(self, run, eng):
        enable(eng, self.cds)

    def collect(self, run, eng):
        codon, reads = eng.codon_tables()
        codon = parallel.allreduce_numpy(run.dist, run.device, codon.astype(np.int64).reshape(-1)).astype(np.uint32).reshape(-1, CELLS)
        reads = parallel.gather_sum_reads(run.dist, run.rank, run.world, reads)
        if run.rank == 0:
            self.tables = Tables(self.cds, run.ref_seq, codon, reads, run.v_min_depth, run.v_min_freq)
