"""Co-occurrence of listed mutations of the command line (--cooc): the loader of the mutation-set file,
the arrays the engine takes (lib.Engine.cooc_enable), and what the table says per set: the COOC key of a VCF record and the
pattern table (--cooc_out).  The numbers themselves come from the engine (lib.Engine.cooc_tables): nothing here looks at a read.

POSITIONS IN THE FILE ARE 1-BASED, as in a VCF and in the literature (A23403G is the base the VCF calls POS 23403) -- unlike
the CDS file of --codons, which is 0-based and half-open.  The device is 0-based: the loader converts.

The device takes the sets sorted by their first site; the file's order -- of the sets and of the mutations inside a set -- is
kept for every output: ``CoocSets.order`` and ``CoocSets.bit`` translate."""
from __future__ import annotations

import re
from os.path import isfile

import numpy as np

from . import abi, parallel
from .readloop import error, print_log
from .reports import Report

BAD_NAME_CHARS = ",;=|:"
BASES = "ACGT"
CELLS = abi.COOC_CELLS
PARTIAL = 64
KEY = "COOC"
HEADER_LINES = ("##INFO=<ID=COOC,Number=.,Type=String,Description=\"Mutation sets with a substitution to an alternate base of this record: "
                "name:reads with all the set's mutations:reads that show all its sites (|)\">\n")
COLUMNS = ["ref", "set", "mutations", "pattern", "reads", "complete", "frequency", "partial"]
_SUB = re.compile(r"([ACGTN])(\d+)([ACGT])")
_DEL = re.compile(r"del(\d+)(?:-(\d+))?")


class CoocSets:
    """sets: [(name, [(text, pos, len, sym)])] in file order, the mutations in file order too (pos 0-based; len 0: a
    substitution to BASES[sym]).  For the device: ``order[k]``: the file index of device set k; ``set_off``, ``site_pos``,
    ``site_len``, ``site_sym``: the sites of the device sets by position; ``bit[i][m]``: the device bit of file set i's m-th
    mutation."""

    def __init__(self, sets, ref_len):
        self.sets = [(name, list(muts)) for name, muts in sets]
        self.ref_len = int(ref_len)
        by_pos = [sorted(range(len(m)), key=lambda j, m=m: m[j][1]) for _, m in self.sets]
        self.order = sorted(range(len(self.sets)), key=lambda i: (self.sets[i][1][by_pos[i][0]][1], i))
        self.row = {i: k for k, i in enumerate(self.order)}            # file index -> device set
        self.bit = [[0] * len(m) for _, m in self.sets]
        off, pos, ln, sym = [0], [], [], []
        for i in self.order:
            muts = self.sets[i][1]
            for b, j in enumerate(by_pos[i]):
                self.bit[i][j] = b
                pos.append(muts[j][1]); ln.append(muts[j][2]); sym.append(muts[j][3])
            off.append(len(pos))
        self.set_off = np.array(off, np.int32)
        self.site_pos = np.array(pos, np.int32)
        self.site_len = np.array(ln, np.int32)
        self.site_sym = np.array(sym, np.uint8)
        self._at = {}                       # 0-based position of a substitution site -> [(file set, sym)]
        for i, (_, muts) in enumerate(self.sets):
            for _, p, l, s in muts:
                if l == 0:
                    self._at.setdefault(p, []).append((i, s))

    @property
    def n_sets(self):
        return len(self.sets)

    def substitutions_at(self, pos):
        return self._at.get(pos, ())

    def all_mutated(self, i):
        return (1 << len(self.sets[i][1])) - 1

    def pattern_text(self, i, cell):
        """Device cell ``cell`` of file set i as 0 / 1 in the file's mutation order."""
        return "".join("1" if (cell >> b) & 1 else "0" for b in self.bit[i])


def parse_mutation(text, ref_seq, where):
    """'A23403G' / 'del21765-21770' / 'del21991' (1-based, inclusive) -> (text, pos 0-based, len, sym)."""
    G = len(ref_seq)
    m = _SUB.fullmatch(text)
    if m:
        ref, p, alt = m.group(1), int(m.group(2)) - 1, m.group(3)
        if p < 0 or p >= G:
            error("%s: %s lies outside the reference of %d bases (positions are 1-based)" % (where, text, G))
        if ref_seq[p].upper() != ref:
            error("%s: %s names %s as the reference base at %d (1-based), the reference has %s" % (where, text, ref, p + 1, ref_seq[p].upper()))
        if alt == ref:
            error("%s: %s changes nothing" % (where, text))
        return text, p, 0, BASES.index(alt)
    m = _DEL.fullmatch(text)
    if m:
        a = int(m.group(1)) - 1
        b = int(m.group(2)) if m.group(2) is not None else a + 1          # 0-based, half-open [a, b)
        if b <= a:
            error("%s: %s ends in front of its start" % (where, text))
        if a < 0 or b > G:
            error("%s: %s lies outside the reference of %d bases (positions are 1-based)" % (where, text, G))
        return text, a, b - a, 0
    error("%s: not a mutation (A23403G, del21765-21770 or del21991; positions are 1-based): %r" % (where, text))


def parse_sets(text, ref_seq, what="mutation-set file"):
    sets, seen = [], set()
    for no, l in enumerate(text.splitlines(), 1):
        l = l.split("#", 1)[0].rstrip("\r")
        if not l.strip():
            continue
        where = "%s, line %d" % (what, no)
        parts = l.split("\t")
        if len(parts) < 2 or not parts[1].strip():
            error("%s: not 'name <tab> mutations': %s" % (where, l))
        name = parts[0].strip()
        if not name or any(ch.isspace() or ch in BAD_NAME_CHARS for ch in name):
            error("%s: set name empty, with whitespace or with one of '%s': %r" % (where, BAD_NAME_CHARS, name))
        if name in seen:
            error("%s: set name used twice: %s" % (where, name))
        seen.add(name)
        muts = [parse_mutation(t.strip(), ref_seq, where) for t in parts[1].split(",")]
        if len(muts) > abi.COOC_SITES:
            error("%s: set %s has %d mutations; at most %d" % (where, name, len(muts), abi.COOC_SITES))
        by_pos = sorted(muts, key=lambda m: m[1])
        for x, y in zip(by_pos, by_pos[1:]):
            if y[1] < x[1] + max(x[2], 1):
                error("%s: set %s: %s and %s overlap" % (where, name, x[0], y[0]))
        if by_pos[-1][1] - by_pos[0][1] > abi.COOC_MAX_SPAN:
            error("%s: set %s spans %d positions; at most %d" % (where, name, by_pos[-1][1] - by_pos[0][1], abi.COOC_MAX_SPAN))
        sets.append((name, muts))
    if not sets:
        error("No mutation set in %s" % what)
    if len(sets) > abi.COOC_MAX_SETS:
        error("%s has %d sets; at most %d" % (what, len(sets), abi.COOC_MAX_SETS))
    return CoocSets(sets, len(ref_seq))


def load_sets(fn, ref_seq):
    """The mutation-set file (name <tab> comma-separated mutations per line, '#' starts a comment, 1-based) -> CoocSets."""
    if not isfile(fn):
        error("File not found: %s" % fn)
    with open(fn) as f:
        return parse_sets(f.read(), ref_seq, "file %s" % fn)


def enable(eng, sets):
    eng.cooc_enable(sets.set_off, sets.site_pos, sets.site_len, sets.site_sym)


class Tables:
    """The job's table on the host: cooc uint32[n_sets][65] in the device's order of sets, reads uint64[2] (tallied, skipped
    irregular reads), next to the sets."""

    def __init__(self, sets, cooc, reads):
        self.sets = sets
        self.cooc = np.asarray(cooc).reshape(sets.n_sets, CELLS)
        self.reads = np.asarray(reads, np.uint64).reshape(2)

    def cells(self, i):
        """The 65 cells of file set i."""
        return self.cooc[self.sets.row[i]].tolist()

    def info(self, pos, ref, alts):
        """'COOC=..' of a record at 0-based ``pos``."""
        out = []
        for i, sym in self.sets.substitutions_at(pos):
            if BASES[sym] in alts:
                c = self.cells(i)
                out.append("%s:%d:%d" % (self.sets.sets[i][0], c[self.sets.all_mutated(i)], sum(c[:64])))
        return "COOC=" + ("|".join(out) if out else ".")

    def summary_line(self):
        return "Co-occurrence: %d reads tallied, %d irregular reads skipped; %d mutation sets" % (
            int(self.reads[0]), int(self.reads[1]), self.sets.n_sets)


def write_tsv(f, ref_id, tables):
    """A header line, then per set (file order) and non-zero pattern (ascending device cell): ref, set, mutations (file order),
    pattern (0 / 1 per mutation, file order), reads, complete (the 64 pattern cells together), frequency, partial (cell 64).  A
    set with nothing complete has one line, for the all-mutated pattern, with 0 reads and frequency 0."""
    f.write("#" + "\t".join(COLUMNS) + "\n")
    out = []
    S = tables.sets
    for i, (name, muts) in enumerate(S.sets):
        c = tables.cells(i)
        complete = sum(c[:64])
        text = ",".join(m[0] for m in muts)
        cells = [t for t in range(64) if c[t] > 0] or [S.all_mutated(i)]
        for t in cells:
            out.append("%s\t%s\t%s\t%s\t%d\t%d\t%g\t%d\n" % (ref_id, name, text, S.pattern_text(i, t), c[t], complete,
                                                           c[t] / complete if complete else 0.0, c[PARTIAL]))
    f.write("".join(out))


class CoocReport(Report):
    name, HEADER_LINES, outputs = "cooc", HEADER_LINES, (("cooc_out_fn", "co-occurrence table", write_tsv),)
    sets = None

    def active(self, run):
        return run.cooc_fn is not None

    def check(self, run):
        if run.cooc_out_fn is not None and run.cooc_fn is None:
            error("The co-occurrence table (--cooc_out) needs the mutation-set file (--cooc)")
        if run.cooc_fn is not None and not (run.run_variants or run.run_consensus):
            error("A run that only trims has no count table: no co-occurrence tallies (--cooc, --cooc_out)")

    def load(self, run):
        print_log("Loading mutation sets: %s" % run.cooc_fn)
        self.sets = load_sets(run.cooc_fn, run.ref_seq)

    def enable(self, run, eng):
        enable(eng, self.sets)

    def collect(self, run, eng):
        cooc, reads = eng.cooc_tables()
        cooc = parallel.allreduce_numpy(run.dist, run.device, cooc.astype(np.int64).reshape(-1)).astype(np.uint32).reshape(-1, CELLS)
        reads = parallel.gather_sum_reads(run.dist, run.rank, run.world, reads)
        if run.rank == 0:
            self.tables = Tables(self.sets, cooc, reads)
