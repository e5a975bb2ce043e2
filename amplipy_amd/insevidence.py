"""Insertion alleles of the command line with their evidence (--insertions, --ins_out, and RV on the insertion rows of
--indel_vcf): per allele the reads, the reverse reads, the mean base quality and where on its reads the
allele sits.  The cells come from the engine (lib.Engine.insev_entries), keyed by (ref_pos, len, hash); the allele TEXT comes
from the run's EventStore, which gathers every batch's alleles anyway.  The join of the two is a check, not a lookup: every
entry must meet exactly one allele text and carry the store's count of it.  Nothing here looks at a read."""
from __future__ import annotations

import numpy as np

from . import abi
from .batch import SEQ_NT16

KEYS = ("INS_N", "INS")
HEADER_LINES = (
    "##INFO=<ID=INS_N,Number=1,Type=Integer,Description=\"Distinct insertion alleles anchored at the position\">\n"
    "##INFO=<ID=INS,Number=.,Type=String,Description=\"Insertion alleles anchored at the position at or above the variant frequency: allele:reads:reverse-strand reads:mean base quality:reads with the allele less than E kept bases from a read end (E: --ins_end), by descending reads\">\n")
TSV_COLUMNS = ["ref", "pos", "allele", "length", "count", "rev", "noqual", "mean_qual"] + ["b%d" % b for b in range(abi.INSEV_BINS)] + ["depth", "freq"]
END_EDGES = (2, 4, 8, 16, 32, 64)              # the upper edges of bins 0..5 (rp_bin): what --ins_end may be
END_DEFAULT = 8
CELLS = ("count", "rev", "noqual", "qsum")
M64 = (1 << 64) - 1
_CODE = {c: k for k, c in enumerate(SEQ_NT16)}


# ---- the allele hash of amp_ins.hpp (ins_hash_seed / ins_hash_step / ins_hash_final), over the NT16 codes of the text --------
def allele_hash(text):
    h = 0x9E3779B97F4A7C15
    for c in text:
        h ^= _CODE[c] + 1
        h = (h * 0xFF51AFD7ED558CCD) & M64
        h ^= h >> 29
    return h >> 1


def key_of(pos, text):
    """The device key of allele ``text`` anchored at 0-based ``pos``."""
    return (int(pos), len(text), allele_hash(text))


# ---- entries ------------------------------------------------------------------------------------------------------------------
def merge_entries(parts):
    """The per-key sum of several tables (abi.INSEV_ENTRY_DTYPE arrays), ordered by (ref_pos, len, hash): the ranks' tables on
    rank 0."""
    t = {}
    for ev in parts:
        ev = np.asarray(ev, abi.INSEV_ENTRY_DTYPE)
        for k in range(ev.size):
            e = ev[k]
            c = t.setdefault((int(e["ref_pos"]), int(e["len"]), int(e["hash"])), [0, 0, 0, 0] + [0] * abi.INSEV_BINS)
            for j, f in enumerate(CELLS):
                c[j] += int(e[f])
            for b in range(abi.INSEV_BINS):
                c[4 + b] += int(e["bin"][b])
    out = np.zeros(len(t), abi.INSEV_ENTRY_DTYPE)
    for k, key in enumerate(sorted(t)):
        c = t[key]
        out[k] = (key[0], key[1], key[2], c[0], c[1], c[2], c[3], c[4:])
    return out


def check_lost(lost):
    """Events of alleles the device table had no slot for: never a silent loss."""
    if int(lost) > 0:
        raise RuntimeError("The insertion evidence table was full: %d events of alleles that found no slot were dropped; "
                           "rerun with a larger table (--ins_capacity, log2 of its slots)" % int(lost))


def store_counts(triples):
    """{(ref_pos, text): events} of EventStore.counted_pairs rows (one allele may come in several rows: batches, ranks)."""
    out = {}
    for p, s, c in triples:
        out[(int(p), s)] = out.get((int(p), s), 0) + int(c)
    return out


class JoinError(RuntimeError):
    """The device entries and the store's allele texts do not meet one to one."""


class Allele:
    __slots__ = ("pos", "text", "count", "rev", "noqual", "qsum", "bins")

    def __init__(self, pos, text, e):
        self.pos, self.text = pos, text
        self.count, self.rev, self.noqual, self.qsum = (int(e[f]) for f in CELLS)
        self.bins = [int(b) for b in e["bin"]]

    def mean_qual(self):
        """'%.3g' of qsum / ((count - noqual) * len), or '.' when no base with a quality stands behind it."""
        div = (self.count - self.noqual) * len(self.text)
        return "%.3g" % (self.qsum / div) if div > 0 else "."

    def near_end(self, end):
        """Events with d < end (end: one of END_EDGES)."""
        return sum(self.bins[:END_EDGES.index(end) + 1])


class Tables:
    """The job's insertion alleles on the host: the device entries joined with the store's texts, and the count table for the
    depths.  ``triples``: EventStore.counted_pairs() of the whole job; counts: uint32[G][6] or None (no depth, no freq)."""

    def __init__(self, entries, triples, counts=None, min_freq=0.0, end=END_DEFAULT):
        assert end in END_EDGES
        ev = np.asarray(entries, abi.INSEV_ENTRY_DTYPE)
        self.counts = None if counts is None else np.asarray(counts).reshape(-1, abi.NSYM)
        self.min_freq, self.end = min_freq, end
        by_key = {}
        for k in range(ev.size):
            e = ev[k]
            key = (int(e["ref_pos"]), int(e["len"]), int(e["hash"]))
            if key in by_key:
                raise JoinError("insertion evidence: position %d holds two entries of one key (length %d)" % (key[0] + 1, key[1]))
            by_key[key] = e
        met = {}
        wanted = sorted(store_counts(triples).items())
        for (pos, text), n in wanted:       # two texts of one position and length under one hash: looked for first, since it
            key = key_of(pos, text)         # shows as a count mismatch as well
            if key in met:
                raise JoinError("insertion evidence: alleles %r and %r at position %d share one entry of the device table (a hash collision)"
                                % (met[key], text, pos + 1))
            met[key] = text
        self.alleles = []
        for (pos, text), n in wanted:
            e = by_key.get(key_of(pos, text))
            if e is None:
                raise JoinError("insertion evidence: allele %r at position %d (%d events) has no entry in the device table" % (text, pos + 1, n))
            if int(e["count"]) != n:
                raise JoinError("insertion evidence: allele %r at position %d: the device table counts %d events, the run's alleles %d"
                                % (text, pos + 1, int(e["count"]), n))
            self.alleles.append(Allele(pos, text, e))
        for key in by_key:
            if key not in met:
                raise JoinError("insertion evidence: the entry at position %d (length %d, %d events) meets no allele of the run" %
                                (key[0] + 1, key[1], int(by_key[key]["count"])))
        self.alleles.sort(key=lambda a: (a.pos, len(a.text), a.text))
        self._at = {}
        for a in self.alleles:
            self._at.setdefault(a.pos, []).append(a)

    def at(self, pos):
        return self._at.get(pos, [])

    def rev_of(self, pos, text):
        """Reverse reads of allele ``text`` at 0-based ``pos``, or None when the table has no such allele."""
        for a in self.at(pos):
            if a.text == text:
                return a.rev
        return None

    def depth(self, pos):
        """Depth at the anchor, insertion alleles included (the DP of a record there)."""
        return int(self.counts[pos].sum()) + sum(a.count for a in self.at(pos))

    def info(self, pos, dp):
        """'INS_N=..;INS=..' of a record at 0-based ``pos`` whose total depth is ``dp``."""
        here = self.at(pos)
        shown = sorted((a for a in here if dp > 0 and a.count / dp >= self.min_freq), key=lambda a: (-a.count, a.text))
        return "INS_N=%d;INS=%s" % (len(here), ",".join("%s:%d:%d:%s:%d" % (a.text, a.count, a.rev, a.mean_qual(), a.near_end(self.end)) for a in shown) or ".")


def write_tsv(f, ref_id, tables):
    """A header line, then one line per allele by (position, length, allele): ref_id, pos + 1, allele, length, count, rev, noqual,
    mean quality, the seven bins, depth at the anchor (insertion alleles included), frequency."""
    f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
    lines = []
    for a in tables.alleles:
        d = tables.depth(a.pos) if tables.counts is not None else 0
        lines.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%s\n" % (ref_id, a.pos + 1, a.text, len(a.text), a.count, a.rev, a.noqual, a.mean_qual(),
                                                                  "\t".join("%d" % b for b in a.bins), d, "%.6g" % (a.count / d) if d else "."))
    f.write("".join(lines))


class IndelInfo:
    """The INFO keys of the indel unit on a VCF record: the deletion events' (when the run writes them), then the insertion
    alleles'."""

    def __init__(self, deletion, insertion):
        self.parts = [t for t in (deletion, insertion) if t is not None]

    def info(self, pos, dp):
        return ";".join(t.info(pos, dp) for t in self.parts)
