"""Per-amplicon allele counts of the command line (--amplicons): the loader of the amplicon file -- iVar's
primer-pair file, widened by one optional column -- and what it makes of a primer BED: names, spans, the rows of either role,
and the two owner tables the engine takes (lib.Engine.amplicon_enable).  The numbers themselves come from the engine
(lib.Engine.amplicon_tables): nothing here looks at a read."""
from __future__ import annotations

from os.path import isfile

import numpy as np

from . import abi, lib, parallel, qc
from .readloop import error, print_log
from .reports import Report
from .strand import fisher_two_sided

BAD_NAME_CHARS = ",;=|"
SYMS = abi.SYMBOLS                      # A C G T N '-': the columns of the count table and of the per-amplicon table
KEYS = ("AMP", "AMP_DP", "AMP_REF_DP", "AMP_ALT_DP", "AMP_NA_DP", "AMP_P", "PRIMER")
HEADER_LINES = (
    "##INFO=<ID=AMP,Number=1,Type=String,Description=\"Amplicons whose span covers the position\">\n"
    "##INFO=<ID=AMP_DP,Number=1,Type=String,Description=\"Depth per listed amplicon\">\n"
    "##INFO=<ID=AMP_REF_DP,Number=1,Type=String,Description=\"Depth of reference base per listed amplicon\">\n"
    "##INFO=<ID=AMP_ALT_DP,Number=1,Type=String,Description=\"Depth of alternate base, per alternate base (comma) and listed amplicon (|)\">\n"
    "##INFO=<ID=AMP_NA_DP,Number=1,Type=Integer,Description=\"Depth from reads that belong to no amplicon\">\n"
    "##INFO=<ID=AMP_P,Number=1,Type=String,Description=\"Per alternate base: two-sided Fisher exact p-value of (alt, depth - alt) in the two listed amplicons of largest depth\">\n"
    "##INFO=<ID=PRIMER,Number=1,Type=String,Description=\"Primers whose binding site covers the position\">\n")
TSV_COLUMNS = ["amplicon", "ref", "pos", "A", "C", "G", "T", "N", "del"]


class AmpliconSet:
    """names[a], lo[a], hi[a] (half-open span), cell_off[a] (first row of a in the table, cell_off[n] = all rows);
    left_rows / right_rows: [(start, end, primer name, amplicon)] in BED order of (start, end); amp_start / amp_end:
    int32[ref_len], the amplicon whose left / right primer owns the position, -1: none; primers: every BED row."""

    def __init__(self, names, lo, hi, left_rows, right_rows, amp_start, amp_end, primers, ref_len):
        self.names = list(names)
        self.lo = np.asarray(lo, np.int32); self.hi = np.asarray(hi, np.int32)
        self.cell_off = np.zeros(len(self.names) + 1, np.int64)
        np.cumsum(self.hi.astype(np.int64) - self.lo, out=self.cell_off[1:])
        self.left_rows, self.right_rows = left_rows, right_rows
        self.amp_start, self.amp_end = amp_start, amp_end
        self.primers = list(primers)
        self.ref_len = int(ref_len)

    @property
    def n(self):
        return len(self.names)

    @property
    def cells(self):
        return int(self.cell_off[-1])

    def rows_of(self, a):
        """The rows of amplicon a in a table uint32[cells][6]."""
        return slice(int(self.cell_off[a]), int(self.cell_off[a + 1]))


def parse_pairs(pair_fn):
    """The amplicon file -> [(left name, right name, amplicon name)], one per line; the default amplicon name is the left
    primer's."""
    if not isfile(pair_fn):
        error("File not found: %s" % pair_fn)
    out = []
    with open(pair_fn) as f:
        for l in f.read().splitlines():
            if not l.strip():
                continue
            parts = l.rstrip("\r").split("\t")
            if len(parts) < 2 or not parts[0] or not parts[1]:
                error("Invalid amplicon line (left primer <tab> right primer [<tab> amplicon]): %s" % l)
            name = parts[2] if len(parts) > 2 and parts[2] else parts[0]
            if any(ch.isspace() or ch in BAD_NAME_CHARS for ch in name):
                error("Amplicon name with whitespace or one of '%s': %r" % (BAD_NAME_CHARS, name))
            out.append((parts[0], parts[1], name))
    if not out:
        error("No amplicon in file: %s" % pair_fn)
    return out


def owner_tables(ref_len, left_rows, right_rows, offset):
    """amp_start / amp_end from the rows of either role: amp_qc_find_primer_owners once per role (cover and tie rules of
    DESIGN.md section 15), then row -> amplicon.  The rows are in ascending (start, end), as the owners' indices are."""
    def one(rows, side):
        if not rows:
            return np.full(ref_len, -1, np.int32)
        owner = lib.find_primer_owners(ref_len, [(s, e) for s, e, _, _ in rows], offset)[side]
        amp = np.array([a for _, _, _, a in rows] + [-1], np.int32)      # (owner -1 takes the last entry)
        return amp[owner]
    return one(left_rows, 0), one(right_rows, 1)


def build_amplicons(pairs, primer_rows, offset, ref_len):
    """pairs: [(left, right, amplicon)]; primer_rows: qc.load_primer_rows -> AmpliconSet.  A primer name stands for every row
    of the BED that carries it."""
    by_name = {}
    for k, (s, e, name) in enumerate(primer_rows):
        by_name.setdefault(name, []).append(k)
    names, index = [], {}
    role = {}                                       # primer name -> (amplicon, 0 left / 1 right)
    for left, right, amp in pairs:
        a = index.setdefault(amp, len(names))
        if a == len(names):
            names.append(amp)
        for pname, side in ((left, 0), (right, 1)):
            if pname not in by_name:
                error("Amplicon %s: no primer named %s in the primer BED" % (amp, pname))
            if role.setdefault(pname, (a, side)) != (a, side):
                error("Primer %s is used in two amplicons or as left and right primer" % pname)
    left_rows, right_rows = [], []
    for k, (s, e, name) in enumerate(primer_rows):  # (BED order of (start, end): the order find_primer_owners indexes)
        if name in role:
            a, side = role[name]
            (left_rows, right_rows)[side].append((s, e, name, a))
    lo, hi = [], []
    for a, amp in enumerate(names):
        l = max(0, min(s for s, e, _, x in left_rows if x == a) - offset)
        h = min(ref_len, max(e for s, e, _, x in right_rows if x == a) + offset)
        if l >= h:
            error("Amplicon %s: its right primers end at or in front of where its left primers start" % amp)
        lo.append(l); hi.append(h)
    amp_start, amp_end = owner_tables(ref_len, left_rows, right_rows, offset)
    return AmpliconSet(names, lo, hi, left_rows, right_rows, amp_start, amp_end, primer_rows, ref_len)


def load_amplicons(pair_fn, primer_rows, offset, ref_len):
    """The amplicon file on the rows of the primer BED (qc.load_primer_rows) -> AmpliconSet."""
    return build_amplicons(parse_pairs(pair_fn), primer_rows, offset, ref_len)


def enable(eng, amps):
    eng.amplicon_enable(amps.lo, amps.hi, amps.amp_start, amps.amp_end)


class Tables:
    """The job's per-amplicon tables on the host, next to the count table: counts uint32[G][6], amp_counts
    uint32[cells][6], amp_reads uint64[n + 1] (the last cell: reads with status 0 that belong to no amplicon)."""

    def __init__(self, amps, counts, amp_counts, amp_reads):
        self.amps = amps
        self.counts = np.asarray(counts).reshape(amps.ref_len, abi.NSYM)
        self.amp_counts = np.asarray(amp_counts).reshape(amps.cells, abi.NSYM)
        self.amp_reads = np.asarray(amp_reads, np.uint64).reshape(amps.n + 1)
        self._lo, self._hi = amps.lo.astype(np.int64), amps.hi.astype(np.int64)
        self._ps = np.array([r[0] for r in amps.primers], np.int64); self._pe = np.array([r[1] for r in amps.primers], np.int64)

    def listed(self, pos):
        """The amplicons whose span covers pos, in amplicon order."""
        return np.nonzero((self._lo <= pos) & (pos < self._hi))[0].tolist()

    def row(self, a, pos):
        return self.amp_counts[int(self.amps.cell_off[a]) + pos - int(self.amps.lo[a])].tolist()

    def primers_at(self, pos):
        """Names of the BED rows with start <= pos < end, each once, in the rows' order (ascending (start, end))."""
        out = []
        for k in np.nonzero((self._ps <= pos) & (pos < self._pe))[0].tolist():
            if self.amps.primers[k][2] not in out:
                out.append(self.amps.primers[k][2])
        return out

    def info(self, pos, ref, alts):
        """'AMP=..;AMP_DP=..;AMP_REF_DP=..;AMP_ALT_DP=..;AMP_NA_DP=..;AMP_P=..;PRIMER=..' of a record at 0-based ``pos``."""
        amps = self.listed(pos)
        rows = [self.row(a, pos) for a in amps]
        dps = [sum(r) for r in rows]
        ref_col = "ACGTN".find(ref) if len(ref) == 1 else -1
        # the two listed amplicons of largest depth, the earlier one first among equals
        top = sorted(range(len(amps)), key=lambda k: -dps[k])[:2]
        two = top if len(top) == 2 and dps[top[1]] > 0 else None
        alt_dp, alt_p = [], []
        for s in alts:
            col = SYMS.find(s) if len(s) == 1 else -1
            if col < 0:
                alt_dp.append("."); alt_p.append(".")
                continue
            alt_dp.append("|".join(str(r[col]) for r in rows) if rows else ".")
            if two is None:
                alt_p.append(".")
            else:
                (x, dx), (y, dy) = [(rows[k][col], dps[k]) for k in two]
                alt_p.append("%.4g" % fisher_two_sided(x, dx - x, y, dy - y))
        primers = self.primers_at(pos)
        return "AMP=%s;AMP_DP=%s;AMP_REF_DP=%s;AMP_ALT_DP=%s;AMP_NA_DP=%d;AMP_P=%s;PRIMER=%s" % (
            ",".join(self.amps.names[a] for a in amps) if amps else ".", ",".join(map(str, dps)) if amps else ".",
            ",".join(str(r[ref_col]) for r in rows) if amps and ref_col >= 0 else ".", ",".join(alt_dp),
            int(self.counts[pos].sum()) - sum(dps), ",".join(alt_p), ",".join(primers) if primers else ".")

    def report_entries(self):
        """The ``amplicons`` list of the QC report: name, start, end, reads, bases (the sum of the amplicon's cells)."""
        a = self.amps
        return [{"name": a.names[k], "start": int(a.lo[k]), "end": int(a.hi[k]), "reads": int(self.amp_reads[k]),
                 "bases": int(self.amp_counts[a.rows_of(k)].sum(dtype=np.uint64))} for k in range(a.n)]

    def summary_line(self):
        assigned, seen = int(self.amp_reads[:-1].sum()), int(self.amp_reads.sum())
        return "Amplicons: %d of %d reads assigned; %d of %d amplicons without a read" % (
            assigned, seen, int((self.amp_reads[:-1] == 0).sum()), self.amps.n)


def write_tsv(f, ref_id, tables):
    """A header line, then per amplicon and per position of its span: amplicon, ref_id, pos + 1, and the six counts."""
    f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
    a = tables.amps
    ref = ref_id.replace("%", "%%")
    for k in range(a.n):
        fmt = a.names[k].replace("%", "%%") + "\t" + ref + "\t%d" * 7 + "\n"
        rows = tables.amp_counts[a.rows_of(k)].tolist()
        f.write("".join([fmt % tuple([int(a.lo[k]) + 1 + j] + r) for j, r in enumerate(rows)]))


def add_to_report(report, tables):
    """The QC report of a run with --amplicons: ``reads`` gains no_amplicon, and ``amplicons`` comes last."""
    report["reads"]["no_amplicon"] = int(tables.amp_reads[-1])
    report["amplicons"] = tables.report_entries()
    return report


class AmpliconReport(Report):
    name, HEADER_LINES, outputs = "amplicon", HEADER_LINES, (("amplicon_out_fn", "per-amplicon counts", write_tsv),)
    amps = None

    def active(self, run):
        return run.amplicons_fn is not None

    def check(self, run):
        if run.amplicon_out_fn is not None and run.amplicons_fn is None:
            error("The per-amplicon table (--amplicon_out) needs the amplicon file (--amplicons)")
        if run.amplicons_fn is not None and not (run.run_trim and run.run_variants and run.run_consensus):
            error("Per-amplicon counts (--amplicons, --amplicon_out) work on aio only: reads are assigned to amplicons by their original "
                  "coordinates against the primer BED, which only a run that trims has, and are counted for a VCF, which only a run that "
                  "calls variants writes")

    def load(self, run):
        print_log("Loading amplicons: %s" % run.amplicons_fn)
        self.amps = load_amplicons(run.amplicons_fn, qc.load_primer_rows(run.primer_fn), run.primer_pos_offset or 0, run.G)

    def enable(self, run, eng):
        enable(eng, self.amps)

    def collect(self, run, eng):
        counts, reads = eng.amplicon_tables()
        counts = parallel.allreduce_numpy(run.dist, run.device, counts.astype(np.int64).reshape(-1)).astype(np.uint32).reshape(-1, abi.NSYM)
        reads = parallel.gather_sum_reads(run.dist, run.rank, run.world, reads)
        if run.rank == 0:
            self.tables = Tables(self.amps, eng.counts(), counts, reads)

    def add_to_qc(self, report):
        add_to_report(report, self.tables)
