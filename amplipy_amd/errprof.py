"""The error profile of the command line (--error_profile, --error_mask): the loaders of the mask, the
JSON report, and the two keys of a VCF record (ERR_RATE, ERR_P).  The numbers themselves come from the engine
(lib.Engine.errprof_tables): nothing here looks at a read.

The tables are in ALIGNED orientation: sub[m][s][g][x][b] is reference letter x read as base b on strand s.  The report's
``substitutions`` are in SEQUENCING orientation -- what the instrument read against what the template had: a reverse-strand
read's pair is complemented, mates and strands are summed.  ERR_RATE and ERR_P of a VCF record stay in aligned orientation, like
the record's own REF and ALT.  Without a mask the bases of a site itself are part of the rate it is compared with."""
from __future__ import annotations

import gzip
import math
from os.path import isfile

import numpy as np

from . import abi, parallel, qc
from .readloop import error, print_log
from .reports import Report

BASES = "ACGT"
CYCLES, QUALS = abi.EP_CYCLES, abi.EP_QUALS
HEADER_LINES = ("##INFO=<ID=ERR_RATE,Number=A,Type=String,Description=\"Rate at which the run reads the reference base as this alternate base, over all "
                "profiled bases at or above the minimum quality (without --error_mask the site's own bases are part of it)\">\n"
                "##INFO=<ID=ERR_P,Number=A,Type=String,Description=\"P(K >= ALT_DP) for K ~ Binomial(depth over A C G T, ERR_RATE)\">\n")
CLASSES = [a + ">" + b for a in BASES for b in BASES if a != b]
FOLDED = ["C>A", "C>G", "C>T", "T>A", "T>C", "T>G"]
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ---- the mask ---------------------------------------------------------------------------------------------------------------
def _lines(fn):
    if not isfile(fn):
        error("File not found: %s" % fn)
    f = gzip.open(fn, "rt") if fn.lower().endswith(".gz") else open(fn)
    with f:
        return f.read().splitlines()


def load_mask(fn, ref_len):
    """bool[ref_len]: True for a position that takes no part.  A name ending in .vcf or .vcf.gz: every record masks
    [POS - 1, POS - 1 + len(REF)); anything else: BED columns 2 and 3 (0-based, half-open; .gz allowed; the first column is not
    looked at, as in the region BED of --qc_regions).  A row outside the reference is an error."""
    mask = np.zeros(ref_len, bool)
    is_vcf = fn.lower().endswith((".vcf", ".vcf.gz"))
    for l in _lines(fn):
        if not l.strip() or (is_vcf and l.startswith("#")):
            continue
        parts = l.split("\t")
        try:
            if is_vcf:
                if len(parts) < 4 or not parts[3]:
                    raise ValueError
                s = int(parts[1]) - 1
                e = s + len(parts[3])
            else:
                if len(parts) < 3:
                    raise ValueError
                s, e = int(parts[1]), int(parts[2])
        except ValueError:
            error("Invalid error mask %s line: %s" % ("VCF" if is_vcf else "BED", l))
        if s < 0 or e > ref_len or e < s:
            error("Error mask row outside the reference of %d bases: %s" % (ref_len, l))
        mask[s:e] = True
    return mask


def enable(eng, ref_seq, mask):
    eng.errprof_enable(ref_seq, mask if mask is not None and mask.any() else None)


# ---- the binomial tail ------------------------------------------------------------------------------------------------------
def binom_sf(k, n, p):
    """P(K >= k) for K ~ Binomial(n, p), without SciPy, in the manner of strand.fisher_two_sided: the first term by math.lgamma,
    its neighbours by the ratio of neighbouring terms, until a term no longer changes the sum.  The sum starts at the largest
    term of the tail -- k, or the mode when k lies below it -- and walks away from it on both sides; when the tail holds the mode
    the complement is the shorter sum, so that one is taken."""
    k, n = int(k), int(n)
    if k <= 0:
        return 1.0
    if k > n or p <= 0.0:
        return 0.0
    if p >= 1.0:
        return 1.0

    def logpmf(x):
        return math.lgamma(n + 1) - math.lgamma(x + 1) - math.lgamma(n - x + 1) + x * math.log(p) + (n - x) * math.log1p(-p)

    odds = p / (1.0 - p)

    def walk(x, step, stop):
        """sum of pmf(x), pmf(x + step), ... up to and including stop"""
        if (stop - x) * step < 0:
            return 0.0
        t = math.exp(logpmf(x))
        total = 0.0
        while True:
            total += t
            if x == stop or t < 1e-18 * total:
                break
            t *= (n - x) / (x + 1) * odds if step > 0 else x / (n - x + 1) / odds
            x += step
        return total

    mode = min(int((n + 1) * p), n)
    if k > mode:
        return min(1.0, walk(k, 1, n))                  # the terms fall from k on
    # the tail holds the mode: 1 - P(K <= k - 1), whose terms fall from k - 1 down
    return max(0.0, 1.0 - walk(k - 1, -1, 0))


# ---- the tables -------------------------------------------------------------------------------------------------------------
def _rate(n, of):
    return None if of == 0 else float("%.6g" % (n / of))


def to_wire(cyc, qualt, sub, reads):
    """The three tables and the read counters of a rank as one int64 array for the all-reduce, and back."""
    return np.concatenate([np.asarray(a).astype(np.int64).reshape(-1) for a in (cyc, qualt, sub, reads)])


def from_wire(wire):
    w = np.asarray(wire, np.int64).astype(np.uint64)
    n1, n2, n3 = (int(np.prod(s)) for s in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE))
    assert w.size == n1 + n2 + n3 + 2
    return w[:n1].reshape(abi.EP_CYC_SHAPE), w[n1:n1 + n2].reshape(abi.EP_QUAL_SHAPE), w[n1 + n2:n1 + n2 + n3].reshape(abi.EP_SUB_SHAPE), w[-2:]


class Tables:
    """The job's tables on the host (cyc, qualt, sub, reads as lib.Engine.errprof_tables gives them), the count table for the
    depth of a VCF record's position (None: no VCF keys are asked for), and what the report says beside them."""

    def __init__(self, cyc, qualt, sub, reads, min_quality, masked_positions, counts=None):
        self.cyc = np.asarray(cyc).reshape(abi.EP_CYC_SHAPE)
        self.qualt = np.asarray(qualt).reshape(abi.EP_QUAL_SHAPE)
        self.sub = np.asarray(sub).reshape(abi.EP_SUB_SHAPE)
        self.reads = [int(x) for x in np.asarray(reads).reshape(2)]
        self.min_quality = int(min_quality)
        self.masked_positions = int(masked_positions)
        self.counts = None if counts is None else np.asarray(counts).reshape(-1, abi.NSYM)
        self.S = self.sub[:, :, 1].astype(np.int64).sum(axis=(0, 1))        # [x][b] at or above min_quality, aligned orientation

    # -- the report
    def totals(self):
        bases, mism = int(self.cyc.sum()), int(self.cyc[:, :, 1].sum())
        return {"bases": bases, "mismatches": mism, "rate": _rate(mism, bases)}

    def oriented(self, g_from):
        """int[4][4]: template base x read as b in sequencing orientation, over g >= g_from, mates and strands summed."""
        t = self.sub[:, :, g_from:].astype(np.int64).sum(axis=(0, 2))       # [s][x][b]
        return t[0] + t[1][::-1, ::-1]                                     # (the complement of code k is 3 - k)

    def _classes(self, t):
        out = {}
        for name in CLASSES:
            x, b = BASES.index(name[0]), BASES.index(name[2])
            n, of = int(t[x, b]), int(t[x].sum())
            out[name] = {"n": n, "of": of, "rate": _rate(n, of)}
        return out

    def _folded(self, t):
        out = {}
        for name in FOLDED:
            x, b = BASES.index(name[0]), BASES.index(name[2])
            cx, cb = 3 - x, 3 - b
            n, of = int(t[x, b] + t[cx, cb]), int(t[x].sum() + t[cx].sum())
            out[name] = {"n": n, "of": of, "rate": _rate(n, of)}
        return out

    def report(self):
        """The report as a dict, keys in the order the file has them."""
        rep = {"amplipy_error_profile": 1, "min_quality": self.min_quality, "masked_positions": self.masked_positions,
               "reads": {"profiled": self.reads[0], "skipped": self.reads[1]}, "total": self.totals()}
        for m, name in enumerate(("read1", "read2")):
            if not self.cyc[m].any():
                continue
            used = np.nonzero(self.cyc[m].sum(axis=1))[0]
            last = int(used[-1]) + 1
            rows = []
            for v in np.nonzero(self.qualt[m].sum(axis=1))[0].tolist():
                bases, mism = int(self.qualt[m, v].sum()), int(self.qualt[m, v, 1])
                rows.append({"q": v, "bases": bases, "mismatches": mism, "empirical": round(-10.0 * math.log10((mism + 1) / (bases + 2)), 2)})
            rep[name] = {"cycle": {"bases": self.cyc[m, :last].sum(axis=1).astype(np.int64).tolist(), "mismatches": self.cyc[m, :last, 1].astype(np.int64).tolist(),
                                   "open_ended": last == CYCLES},
                         "quality": rows}
        all_, pass_ = self.oriented(0), self.oriented(1)
        rep["substitutions"] = {"all": self._classes(all_), "pass": self._classes(pass_), "folded": self._folded(all_)}
        return rep

    def summary_line(self):
        t = self.totals()
        return "Error profile: %d of %d reads profiled; %d mismatches in %d bases (rate %s)" % (
            self.reads[0], self.reads[0] + self.reads[1], t["mismatches"], t["bases"], "n/a" if t["rate"] is None else "%g" % t["rate"])

    # -- the VCF keys
    def info(self, pos, ref, alts):
        """'ERR_RATE=..;ERR_P=..' of a record at 0-based ``pos``: per ALT base b, S[X][b] / sum of S[X] with X the upper-cased
        REF letter, and P(K >= ALT_DP) for K ~ Binomial(depth over A C G T, that rate).  '.' for '-', N, an insertion allele, a
        REF letter outside A C G T and an empty row of S."""
        X = BASES.find(ref.upper()) if len(ref) == 1 else -1
        row_sum = int(self.S[X].sum()) if X >= 0 else 0
        rates, ps = [], []
        for a in alts:
            b = BASES.find(a) if len(a) == 1 else -1
            if X < 0 or b < 0 or row_sum == 0:
                rates.append("."); ps.append(".")
                continue
            rate = int(self.S[X, b]) / row_sum
            k, n = int(self.counts[pos, b]), int(self.counts[pos, :4].sum())
            rates.append("%.4g" % rate)
            ps.append("%.4g" % binom_sf(k, n, rate))
        return "ERR_RATE=%s;ERR_P=%s" % (",".join(rates), ",".join(ps))


class ErrprofReport(Report):
    name, HEADER_LINES = "errprof", HEADER_LINES
    outputs = (("error_profile_fn", "error profile", lambda f, ref_id, tables: qc.write_json(f, tables.report())),)
    mask = None

    def active(self, run):
        return run.error_profile_fn is not None

    def check(self, run):
        if run.error_mask_fn is not None and run.error_profile_fn is None:
            error("The error mask (--error_mask) needs the error profile (--error_profile)")
        if run.error_profile_fn is not None and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no error profile (--error_profile, --error_mask)")

    def load(self, run):
        if run.error_mask_fn is not None:
            print_log("Loading error mask: %s" % run.error_mask_fn)
            self.mask = load_mask(run.error_mask_fn, run.G)

    def enable(self, run, eng):
        enable(eng, run.ref_seq, self.mask)

    def collect(self, run, eng):
        tabs = from_wire(parallel.allreduce_numpy(run.dist, run.device, to_wire(*eng.errprof_tables())))      # the three tables and the read counters as one int64 array
        if run.rank == 0:
            self.tables = Tables(*tabs, run.min_quality, int(self.mask.sum()) if self.mask is not None else 0, eng.counts() if run.run_variants else None)
