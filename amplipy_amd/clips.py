"""Soft-clip sites and deletion junctions of the QC report (--qc_clips): the host half.  The engine
tallies, per reference position and side, the reads that are soft-clipped there and their first abi.CLIP_K clipped bases
(lib.Engine.qc_clips_tables); here a site's bases become a consensus, the consensus is held against the reference next to the
site and then looked for elsewhere in it, and the sites that land somewhere else become junctions: deletions and duplications
the aligner clipped instead of opening a gap for them.  Nothing here looks at a read.

All coordinates are 0-based inside and 1-based in every output, as in the VCF.  A site's position p is the reference base
right of the junction: a LEFT site's first aligned base, the base behind a RIGHT site's last aligned one (at most ref_len)."""
from __future__ import annotations

import numpy as np

from . import abi

SIDES = ("left", "right")
CLASSES = ("contiguous", "short", "novel", "repeat", "deletion", "duplication")
MIN_PLACED = 12                   # a consensus shorter than this is not looked for in the reference
DEFAULT_CLIP_MIN, DEFAULT_MIN_READS = 10, 2
_ACGT = "ACGT"


def to_wire(table, scalars):
    """The table and its scalars as one int64 array (the all-reduce of several ranks)."""
    return np.concatenate([np.asarray(table, np.int64).reshape(-1), np.asarray(scalars, np.int64).reshape(-1)])


def from_wire(wire, ref_len):
    wire = np.asarray(wire)
    n = (ref_len + 1) * 2 * abi.CLIP_CELLS
    return wire[:n].astype(np.uint64).reshape(ref_len + 1, 2, abi.CLIP_CELLS), wire[n:n + abi.CLIP_SCALARS].astype(np.uint64)


def merge_tables(parts):
    """Element-wise sum of partial (table, scalars) pairs."""
    parts = list(parts)
    return (np.sum([np.asarray(t, np.uint64) for t, _ in parts], axis=0, dtype=np.uint64),
            np.sum([np.asarray(s, np.uint64) for _, s in parts], axis=0, dtype=np.uint64))


def consensus(cells, side):
    """One site's cells (reads, rev, comp[j][c]) -> (m, text): m leading offsets at which at least half of the site's reads
    still have a clipped base; per offset the base more than half of those reads agree on, else N; the text in reference
    orientation -- a RIGHT site's begins at the junction, a LEFT site's ends there."""
    cells = [int(x) for x in np.asarray(cells).reshape(-1)]
    n = cells[0]
    letters = []
    for j in range(abi.CLIP_K):
        comp = cells[2 + j * abi.CLIP_COLS:2 + (j + 1) * abi.CLIP_COLS]
        depth = sum(comp)
        if 2 * depth < n:
            break
        best = [c for c in range(4) if 2 * comp[c] > depth]
        letters.append(_ACGT[best[0]] if best else "N")
    text = "".join(letters)
    return len(letters), text if side == abi.CLIP_RIGHT else text[::-1]


def _mismatches(R, start, text):
    """Letters of ``text`` that differ from R[start : start + len(text)]: N in the text is neither a match nor a mismatch;
    outside the reference, or on a reference letter that is not A C G T, is a mismatch."""
    bad = 0
    for k, ch in enumerate(text):
        if ch == "N":
            continue
        q = start + k
        if q < 0 or q >= len(R) or R[q] not in _ACGT or R[q] != ch:
            bad += 1
    return bad


def _occurrences(R, text):
    """Start of every exact occurrence of ``text`` in R, forward strand, overlapping ones included; at most two are needed."""
    out = []
    at = R.find(text)
    while at >= 0 and len(out) < 2:
        out.append(at)
        at = R.find(text, at + 1)
    return out


def left_align(R, s, length):
    """The interval [s, s + length) moved left while the base in front of it equals its last base: the same event seen from
    either side, with any microhomology, lands on one start."""
    while s > 0 and R[s - 1] == R[s + length - 1]:
        s -= 1
    return s


def classify(R, p, side, m, text):
    """-> (class, partner, interval): partner is the 0-based reference position of the clipped base nearest the junction of a
    placed site (None otherwise); interval the left-aligned (start, length) of its deletion or duplication."""
    start = p if side == abi.CLIP_RIGHT else p - m
    if _mismatches(R, start, text) <= m // 8:
        return "contiguous", None, None
    if m < MIN_PLACED or "N" in text:
        return "short", None, None
    hits = _occurrences(R, text)
    if not hits:
        return "novel", None, None
    if len(hits) > 1:
        return "repeat", None, None
    t = hits[0]
    if side == abi.CLIP_RIGHT:
        kind, s, e, partner = ("deletion", p, t, t) if t > p else ("duplication", t, p, t)
    else:
        end = t + m
        kind, s, e, partner = ("deletion", end, p, end - 1) if end < p else ("duplication", p, end, end - 1)
    return kind, partner, (left_align(R, s, e - s), e - s)


class Site:
    __slots__ = ("p", "side", "reads", "rev", "m", "text", "cls", "partner", "interval")

    def __init__(self, p, side, reads, rev, m, text, cls, partner, interval):
        self.p, self.side, self.reads, self.rev, self.m, self.text = p, side, reads, rev, m, text
        self.cls, self.partner, self.interval = cls, partner, interval


def find_sites(table, ref_seq, min_reads=DEFAULT_MIN_READS):
    """Every (position, side) of the table with at least ``min_reads`` reads -> [Site], by position, left before right."""
    R = ref_seq.upper()
    table = np.asarray(table).reshape(-1, 2, abi.CLIP_CELLS)
    out = []
    for p, side in np.argwhere(table[:, :, 0] >= max(int(min_reads), 1)).tolist():
        cells = table[p, side]
        m, text = consensus(cells, side)
        cls, partner, interval = classify(R, p, side, m, text)
        out.append(Site(p, side, int(cells[0]), int(cells[1]), m, text, cls, partner, interval))
    return out


def find_junctions(sites, ref_len, depth=None):
    """The placed sites by (kind, start, length) -> rows (dicts, coordinates 1-based: start .. end inclusive), most reads
    first, then by start and length.  depth: the depth of every position (the six symbols of the count table), or None."""
    rows = {}
    for s in sites:
        if s.interval is None:
            continue
        key = (s.cls, s.interval[0], s.interval[1])
        r = rows.setdefault(key, dict(right_reads=0, right_reverse=0, left_reads=0, left_reverse=0))
        r[SIDES[s.side] + "_reads"] += s.reads
        r[SIDES[s.side] + "_reverse"] += s.rev

    def flank(q):
        return int(depth[q]) if depth is not None and 0 <= q < ref_len else None
    out = []
    for (kind, s, length), r in sorted(rows.items(), key=lambda kv: (-(kv[1]["right_reads"] + kv[1]["left_reads"]), kv[0][1], kv[0][2], kv[0][0])):
        out.append(dict(kind=kind, start=s + 1, end=s + length, length=length, **r, flank_depth_left=flank(s - 1), flank_depth_right=flank(s + length)))
    return out


SITE_COLUMNS = ("ref", "position", "side", "reads", "reverse_reads", "consensus", "class", "partner")
JUNCTION_COLUMNS = ("ref", "kind", "start", "end", "length", "right_reads", "right_reverse", "left_reads", "left_reverse",
                    "flank_depth_left", "flank_depth_right")


def write_sites(f, ref_id, sites):
    """One line per site: ref, position (1-based), side, reads, reverse reads, consensus ('.' when empty), class, partner (the
    1-based position of the clipped base nearest the junction of a placed site, '.' otherwise)."""
    f.write("#" + "\t".join(SITE_COLUMNS) + "\n")
    f.write("".join(["%s\t%d\t%s\t%d\t%d\t%s\t%s\t%s\n" % (ref_id, s.p + 1, SIDES[s.side], s.reads, s.rev, s.text or ".", s.cls,
                                                       "." if s.partner is None else s.partner + 1) for s in sites]))


def write_junctions(f, ref_id, junctions):
    """One line per junction row of find_junctions; a flank depth that is not known is '.'."""
    f.write("#" + "\t".join(JUNCTION_COLUMNS) + "\n")
    f.write("".join(["\t".join([ref_id] + ["." if j[k] is None else str(j[k]) for k in JUNCTION_COLUMNS[1:]]) + "\n" for j in junctions]))


def section(clip_min, min_reads, scalars, sites, junctions):
    """The dict of the QC report's key "clips"."""
    by_class = {c: 0 for c in CLASSES}
    for s in sites:
        by_class[s.cls] += 1
    out = {"clip_min": int(clip_min), "min_reads": int(min_reads)}
    out.update({k: int(v) for k, v in zip(abi.CLIP_SCALAR_FIELDS, np.asarray(scalars).tolist())})
    out.update(sites=len(sites), sites_by_class=by_class, junctions=[dict(j) for j in junctions])
    return out
