"""Read-position evidence per allele of the command line (--readpos, --readpos_end, --readpos_out): the
six INFO keys of a VCF record, the per-position TSV file, the rank-sum z of binned distances and the wire format of the
all-reduce.  The numbers themselves come from the engine (lib.Engine.readpos_tables): nothing here looks at a read."""
from __future__ import annotations

import math

import numpy as np

from . import abi, parallel
from .readloop import error
from .reports import Report
from .strand import fisher_two_sided

SYMS = abi.SYMBOLS                      # A C G T N '-': the columns of the count table and of hist
BINS = abi.RP_BINS
EDGES = abi.RP_EDGES                    # the least distance of each bin: 0 2 4 8 16 32 64
END_CHOICES = EDGES[1:]                 # what --readpos_end may be: an "end" is a whole number of bins
DEFAULT_END = 8
KEYS = ("REF_RP", "ALT_RP", "REF_END", "ALT_END", "RPB", "RPZ")
HEADER_LINES = (
    "##INFO=<ID=REF_RP,Number=1,Type=String,Description=\"Reference base by distance to the nearer end of the read's kept bases: counts of d<2|2-3|4-7|8-15|16-31|32-63|>=64\">\n"
    "##INFO=<ID=ALT_RP,Number=1,Type=String,Description=\"Alternate base by distance to the nearer read end, the same seven counts\">\n"
    "##INFO=<ID=REF_END,Number=1,Type=Integer,Description=\"Depth of reference base within the read-end distance of --readpos_end\">\n"
    "##INFO=<ID=ALT_END,Number=1,Type=String,Description=\"Depth of alternate base within the read-end distance of --readpos_end\">\n"
    "##INFO=<ID=RPB,Number=1,Type=String,Description=\"Read-position bias of alternate base: two-sided Fisher exact p-value of (ref end, ref interior; alt end, alt interior)\">\n"
    "##INFO=<ID=RPZ,Number=1,Type=String,Description=\"Rank-sum z of alternate against reference read-end distances on the binned data; negative: the alternate base sits nearer the read ends\">\n")
BIN_NAMES = ["0-1", "2-3", "4-7", "8-15", "16-31", "32-63", "64+"]
TSV_COLUMNS = ["ref", "pos"] + [("del" if s == "-" else s) + "_" + b for s in SYMS for b in BIN_NAMES]


def end_bins(end):
    """The number of bins below distance ``end``; ValueError (naming the bin edges) for anything that is not an edge."""
    if isinstance(end, bool) or not isinstance(end, (int, np.integer)) or int(end) not in END_CHOICES:
        raise ValueError("--readpos_end must be one of the bin edges %s: %s" % (", ".join(map(str, END_CHOICES)), end))
    return EDGES.index(int(end))


def rank_sum_z(a, r):
    """The Mann-Whitney z of sample ``a`` against sample ``r``, both given as histograms over the same ordered bins (every
    value of a bin ties with every other): U = sum_b a_b (sum_{b' < b} r_b' + r_b / 2), mu = n1 n2 / 2,
    sigma^2 = n1 n2 / 12 ((N + 1) - sum_b (t_b^3 - t_b) / (N (N - 1))).  None when a side is empty or sigma is 0."""
    a = [int(x) for x in a]; r = [int(x) for x in r]
    n1, n2 = sum(a), sum(r)
    if n1 == 0 or n2 == 0:
        return None
    N = n1 + n2
    below, u2 = 0, 0                    # u2 = 2 U, an integer
    for ab, rb in zip(a, r):
        u2 += ab * (2 * below + rb)
        below += rb
    ties = sum((x + y) ** 3 - (x + y) for x, y in zip(a, r))
    var_num = n1 * n2 * ((N + 1) * N * (N - 1) - ties)        # sigma^2 = var_num / (12 N (N - 1)), exact so far
    if var_num <= 0:
        return None
    return (u2 - n1 * n2) / 2.0 / math.sqrt(var_num / (12.0 * N * (N - 1)))


class Tables:
    """The job's tables on the host: counts uint32[G][6] (the count table) and hist uint32[G][6][7]; end: --readpos_end."""

    def __init__(self, counts, hist, end=DEFAULT_END):
        G = len(counts)
        self.counts = np.asarray(counts).reshape(G, abi.NSYM)
        self.hist = np.asarray(hist).reshape(G, abi.NSYM, BINS)
        self.end = int(end)
        self.n_end = end_bins(end)

    def _cell(self, pos, sym):
        """The seven counts of a fixed symbol at pos, None for anything else (an insertion allele, a reference letter that is
        none of A C G T N) and where the symbol's count is 0."""
        col = SYMS.find(sym) if len(sym) == 1 else -1
        if col < 0 or int(self.counts[pos, col]) == 0:
            return None
        return [int(x) for x in self.hist[pos, col]]

    def info(self, pos, ref, alts):
        """'REF_RP=..;ALT_RP=..;REF_END=..;ALT_END=..;RPB=..;RPZ=..' of a record at 0-based ``pos``.  A value is '.' for an
        insertion allele, where the symbol's count is 0 and where the reference letter is none of A C G T N (then RPB and RPZ
        too: they have no reference row).  '-' has values: a deletion has a position."""
        r = self._cell(pos, ref) if ref != "-" else None
        k = self.n_end
        alt_rp, alt_end, rpb, rpz = [], [], [], []
        for s in alts:
            c = self._cell(pos, s)
            if c is None:
                alt_rp.append("."); alt_end.append("."); rpb.append("."); rpz.append(".")
                continue
            alt_rp.append("|".join(map(str, c)))
            alt_end.append(str(sum(c[:k])))
            if r is None:
                rpb.append("."); rpz.append(".")
                continue
            rpb.append("%.4g" % fisher_two_sided(sum(r[:k]), sum(r[k:]), sum(c[:k]), sum(c[k:])))
            z = rank_sum_z(c, r)
            rpz.append("." if z is None else "%.3f" % z)
        return "REF_RP=%s;ALT_RP=%s;REF_END=%s;ALT_END=%s;RPB=%s;RPZ=%s" % (
            "." if r is None else "|".join(map(str, r)), ",".join(alt_rp), "." if r is None else sum(r[:k]), ",".join(alt_end),
            ",".join(rpb), ",".join(rpz))


def write_tsv(f, ref_id, tables):
    """A header line, then one line per position: ref_id, pos + 1, and the seven bins of A C G T N '-'."""
    f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
    G = len(tables.counts)
    rows = np.concatenate([np.arange(1, G + 1, dtype=np.uint64).reshape(G, 1), tables.hist.reshape(G, abi.RP_CELLS).astype(np.uint64)], axis=1).tolist()
    fmt = ref_id.replace("%", "%%") + "\t%d" * (1 + abi.RP_CELLS) + "\n"
    f.write("".join([fmt % tuple(r) for r in rows]))


def to_wire(hist):
    """The table of a rank as one int64[G * 42] array for the all-reduce, and back."""
    return np.asarray(hist).astype(np.int64).reshape(-1)


def from_wire(wire):
    return np.asarray(wire, np.int64).reshape(-1, abi.NSYM, BINS).astype(np.uint32)


class ReadposReport(Report):
    """--readpos puts the keys on the VCF; --readpos_out alone switches the tallies on too."""
    name, HEADER_LINES, outputs = "readpos", HEADER_LINES, (("readpos_fn", "read-position tallies", write_tsv),)

    def active(self, run):
        return bool(run.readpos) or run.readpos_fn is not None

    def check(self, run):
        if self.active(run) and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no read-position tallies (--readpos, --readpos_out)")
        if run.readpos and not run.run_variants:
            error("The read-position INFO keys need a VCF (--readpos on variants or aio)")
        if run.readpos_end is not None and not run.readpos:
            error("The read-end distance (--readpos_end) needs --readpos")
        if run.readpos_end is not None:
            try:
                end_bins(run.readpos_end)
            except ValueError as e:
                error(str(e))

    def enable(self, run, eng):
        eng.readpos_enable()

    def collect(self, run, eng):
        hist = from_wire(parallel.allreduce_numpy(run.dist, run.device, to_wire(eng.readpos_tables())))      # the table as one int64 array of G x 42
        if run.rank == 0:
            self.tables = Tables(eng.counts(), hist, DEFAULT_END if run.readpos_end is None else run.readpos_end)

    def annotates(self, run):
        return bool(run.readpos)
