"""Per-allele strand and base-quality evidence of the command line (--strand, --strand_out): the five
INFO keys of a VCF record, the per-position TSV file, and Fisher's exact test for strand bias.  The numbers themselves come
from the engine (lib.Engine.strand_tables) and from the count table: nothing here looks at a read."""
from __future__ import annotations

import math

import numpy as np

from . import abi, parallel
from .readloop import error
from .reports import Report

SYMS = abi.SYMBOLS                      # A C G T N '-': the columns of the count table and of rev; qsum has the first five
QSUM_COLS = abi.STRAND_QSUM_COLS
KEYS = ("REF_RV", "ALT_RV", "REF_QUAL", "ALT_QUAL", "SB")
HEADER_LINES = (
    "##INFO=<ID=REF_RV,Number=1,Type=Integer,Description=\"Reverse-strand depth of reference base\">\n"
    "##INFO=<ID=ALT_RV,Number=1,Type=String,Description=\"Reverse-strand depth of alternate base\">\n"
    "##INFO=<ID=REF_QUAL,Number=1,Type=Integer,Description=\"Mean base quality of reference base\">\n"
    "##INFO=<ID=ALT_QUAL,Number=1,Type=String,Description=\"Mean base quality of alternate base\">\n"
    "##INFO=<ID=SB,Number=1,Type=String,Description=\"Strand bias of alternate base: two-sided Fisher exact p-value of (ref fwd, ref rev; alt fwd, alt rev)\">\n")
TSV_COLUMNS = ["ref", "pos"] + [n + s for n in ("A", "C", "G", "T", "N") for s in ("", "_rv", "_qsum")] + ["del", "del_rv"]
TIE = 1e-7                              # tables whose probability is within this relative distance of the observed one count as ties


def _log_choose(n, k):
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def fisher_two_sided(a, b, c, d):
    """Two-sided Fisher exact p-value of the 2x2 table (a, b; c, d): the sum of the probabilities of all tables with the same
    margins whose probability is <= the observed table's times (1 + TIE).

    The hypergeometric distribution over x (the first cell) has one mode, so those tables are the two tails outside the observed
    value and its counterpart on the other side of the mode.  The observed table's probability and the tail boundaries come from
    math.lgamma (a bisection on the far side: a handful of terms); the terms of a tail then follow from the first one by the
    ratio of neighbouring probabilities, walking away from the mode until a term no longer changes the sum.  That is a few
    multiplications per term and some tens to hundreds of terms, whatever the depth, where one lgamma term per table would cost
    the allele's depth in terms."""
    a, b, c, d = int(a), int(b), int(c), int(d)
    if min(a, b, c, d) < 0:
        raise ValueError("negative cell in a 2x2 table: %r" % ((a, b, c, d),))
    n, r1, c1 = a + b + c + d, a + b, a + c
    if n == 0:
        return 1.0
    lo, hi = max(0, c1 - (n - r1)), min(r1, c1)
    base = _log_choose(n, c1)
    off = n - r1 - c1                   # the fourth cell is off + x

    def logp(x):
        return _log_choose(r1, x) + _log_choose(n - r1, c1 - x) - base

    log_obs = logp(a)
    limit = log_obs + math.log1p(TIE)
    mode = min(max((r1 + 1) * (c1 + 1) // (n + 2), lo), hi)
    mode = max((x for x in (mode - 1, mode, mode + 1) if lo <= x <= hi), key=logp)

    def tail(x, step):
        """sum of p(x), p(x + step), ... relative to the observed probability; x lies on the side of the mode it walks away from"""
        t = math.exp(logp(x) - log_obs)
        total = 0.0
        while lo <= x <= hi:
            total += t
            if t < 1e-18 * total:
                break
            if step > 0:
                t *= (r1 - x) * (c1 - x) / ((x + 1) * (off + x + 1))
            else:
                t *= x * (off + x) / ((r1 - x + 1) * (c1 - x + 1))
            x += step
        return total

    def first_within(near, far, step):
        """the table nearest the mode among near, near + step, ..., far whose probability is within the limit (the probabilities
        fall from near to far), or None"""
        if (far - near) * step < 0 or logp(far) > limit:
            return None
        while near != far:
            mid = near + (far - near) // 2 if step > 0 else near - (near - far) // 2
            if logp(mid) <= limit:
                far = mid
            else:
                near = mid + step
        return far

    if a <= mode:
        left, right = a, first_within(mode if a < mode else mode + 1, hi, 1)
    else:
        left, right = first_within(mode, lo, -1), a
    rel = (tail(left, -1) if left is not None else 0.0) + (tail(right, 1) if right is not None else 0.0)
    return min(1.0, math.exp(log_obs) * rel)


class Tables:
    """The job's three tables on the host: counts uint32[G][6] (the count table), rev uint32[G][6], qsum uint64[G][5]."""

    def __init__(self, counts, rev, qsum):
        G = len(counts)
        self.counts = np.asarray(counts).reshape(G, abi.NSYM)
        self.rev = np.asarray(rev).reshape(G, abi.NSYM)
        self.qsum = np.asarray(qsum).reshape(G, QSUM_COLS)

    def _cell(self, pos, sym):
        """(count, rev, qsum or None) of a fixed symbol at pos, None for anything else (an insertion allele, a reference letter
        that is none of A C G T N)."""
        col = SYMS.find(sym) if len(sym) == 1 else -1
        if col < 0:
            return None
        return int(self.counts[pos, col]), int(self.rev[pos, col]), int(self.qsum[pos, col]) if col < QSUM_COLS else None

    def info(self, pos, ref, alts):
        """'REF_RV=..;ALT_RV=..;REF_QUAL=..;ALT_QUAL=..;SB=..' of a record at 0-based ``pos``.  A value is '.' for an insertion
        allele, for '-' (the quality keys), where the symbol's count is 0 and where the reference letter is none of A C G T N
        (then SB too: it has no reference row)."""
        r = self._cell(pos, ref) if ref != "-" else None
        if r is not None and r[0] == 0:
            r = None
        alt_rv, alt_q, sb = [], [], []
        for s in alts:
            c = self._cell(pos, s)
            if c is None or c[0] == 0:
                alt_rv.append("."); alt_q.append("."); sb.append(".")
                continue
            alt_rv.append(str(c[1]))
            alt_q.append("." if c[2] is None else str(c[2] // c[0]))
            sb.append("." if r is None else "%.4g" % fisher_two_sided(r[0] - r[1], r[1], c[0] - c[1], c[1]))
        return "REF_RV=%s;ALT_RV=%s;REF_QUAL=%s;ALT_QUAL=%s;SB=%s" % (
            "." if r is None else r[1], ",".join(alt_rv), "." if r is None else r[2] // r[0], ",".join(alt_q), ",".join(sb))


def write_tsv(f, ref_id, tables):
    """A header line, then one line per position: ref_id, pos + 1, and count, rev, qsum of A C G T N, count and rev of '-'."""
    f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
    G = len(tables.counts)
    cols = [np.arange(1, G + 1, dtype=np.uint64)]
    for c in range(QSUM_COLS):
        cols += [tables.counts[:, c], tables.rev[:, c], tables.qsum[:, c]]
    cols += [tables.counts[:, 5], tables.rev[:, 5]]
    rows = np.stack([np.asarray(c, np.uint64) for c in cols], axis=1).tolist()
    fmt = ref_id.replace("%", "%%") + "\t%d" * len(cols) + "\n"
    f.write("".join([fmt % tuple(r) for r in rows]))


def to_wire(rev, qsum):
    """Both tables of a rank as one int64[G * 11] array for the all-reduce, and back."""
    G = len(rev)
    out = np.empty((G, abi.STRAND_CELLS), np.int64)
    out[:, :abi.NSYM] = np.asarray(rev).reshape(G, abi.NSYM)
    out[:, abi.NSYM:] = np.asarray(qsum).reshape(G, QSUM_COLS).astype(np.int64)
    return out.reshape(-1)


def from_wire(wire):
    t = np.asarray(wire, np.int64).reshape(-1, abi.STRAND_CELLS)
    return t[:, :abi.NSYM].astype(np.uint32), t[:, abi.NSYM:].astype(np.uint64)


class StrandReport(Report):
    """--strand puts the keys on the VCF; --strand_out alone switches the tallies on too."""
    name, HEADER_LINES, outputs = "strand", HEADER_LINES, (("strand_fn", "strand tallies", write_tsv),)

    def active(self, run):
        return bool(run.strand) or run.strand_fn is not None

    def check(self, run):
        if self.active(run) and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no strand tallies (--strand, --strand_out)")
        if run.strand and not run.run_variants:
            error("The strand INFO keys need a VCF (--strand on variants or aio)")

    def enable(self, run, eng):
        eng.strand_enable()

    def collect(self, run, eng):
        rev, qsum = from_wire(parallel.allreduce_numpy(run.dist, run.device, to_wire(*eng.strand_tables())))      # both tables as one int64 array of G x 11
        if run.rank == 0:
            self.tables = Tables(eng.counts(), rev, qsum)

    def annotates(self, run):
        return bool(run.strand)
