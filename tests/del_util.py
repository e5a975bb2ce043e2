"""TEST INFRASTRUCTURE of the deletion events: a plain restatement over Segments, written from the
definition -- for one counted read, an event is a maximal run of consecutive reference positions each of which that read's
count walk adds to the '-' column -- pair by pair over the read's CIGAR, and from nothing in amplipy_amd/csrc; ``expand``, which
turns events back into per-position '-' and reverse counts (the invariant that pins the events to the count table); and the
hash of the two tables restated, for the tests that look for colliding keys."""
import numpy as np

from amplipy_amd import abi

EMPTY = (1 << 64) - 1
M64 = (1 << 64) - 1


# ---- the restatement --------------------------------------------------------------------------------------------------------
def deleted_positions(seg, min_quality, ref_len):
    """The reference positions the count walk of this read adds to '-' (update_base_counts, A:690-753), in walk order.  The
    walk ends where the reference would raise (a position past the reference, a read without QUAL at its first base, a base
    that is none of A C G T N): what came before stays."""
    qs, qe = seg.query_alignment_start, seg.query_alignment_end
    seq, qual = (seg.query_sequence or "").upper(), seg.query_qualities
    pairs = seg.get_aligned_pairs()
    out = []
    i = 0
    while i < len(pairs):
        q, r = pairs[i]
        i += 1
        if q is None:                       # a deleted position counts whatever surrounds it (A:713-715)
            if not 0 <= r < ref_len:
                break
            out.append(r)
            continue
        if qual is None or q >= len(qual):
            break
        if qual[q] < min_quality:
            continue
        if q < qs:
            continue
        if q >= qe:
            break
        if r is None:                       # an insertion: its scan takes pairs with it, and hands the last one back when it has a position
            stop = False
            while r is None and q is not None and q < qe:
                if q >= len(qual) or (qual[q] >= min_quality and i >= len(pairs)):
                    stop = True
                    break
                if qual[q] < min_quality:
                    break
                q, r = pairs[i]
                i += 1
            if stop:
                break
            if r is not None:
                i -= 1
            continue
        if not 0 <= r < ref_len or seq[q] not in "ACGTN":
            break
    return out


def read_events(seg, min_quality, ref_len):
    """[(start, len)] of one read: its deleted positions, runs of consecutive ones joined."""
    ev = []
    for r in deleted_positions(seg, min_quality, ref_len):
        if ev and ev[-1][0] + ev[-1][1] == r:
            ev[-1][1] += 1
        else:
            ev.append([r, 1])
    return [(s, l) for s, l in ev]


def table(segments, min_quality, ref_len):
    """{(start, len): [count, rev]} of the reads."""
    t = {}
    for seg in segments:
        for key in read_events(seg, min_quality, ref_len):
            c = t.setdefault(key, [0, 0])
            c[0] += 1
            c[1] += 1 if seg.flag & 0x10 else 0
    return t


def as_array(t):
    """The table as amp_del_get gives it: abi.DEL_EVENT_DTYPE ordered by (start, len)."""
    out = np.zeros(len(t), abi.DEL_EVENT_DTYPE)
    for k, key in enumerate(sorted(t)):
        out[k] = (key[0], key[1], t[key][0], t[key][1])
    return out


def as_dict(events):
    return {(int(e["start"]), int(e["len"])): [int(e["count"]), int(e["rev"])] for e in events}


def add_tables(a, b):
    out = {k: list(v) for k, v in a.items()}
    for k, v in b.items():
        c = out.setdefault(k, [0, 0])
        c[0] += v[0]
        c[1] += v[1]
    return out


def expand(events, ref_len):
    """(dash uint64[ref_len], rev uint64[ref_len]): per position the counts and reverse counts of the events that cover it.
    ``events``: a structured array, or a {(start, len): [count, rev]} table."""
    dash = np.zeros(ref_len, np.uint64); rev = np.zeros(ref_len, np.uint64)
    items = events.items() if isinstance(events, dict) else as_dict(events).items()
    for (s, l), (c, r) in items:
        assert l >= 1 and 0 <= s and s + l <= ref_len
        dash[s:s + l] += np.uint64(c)
        rev[s:s + l] += np.uint64(r)
    return dash, rev


# ---- the hash, restated -----------------------------------------------------------------------------------------------------
def key_of(start, length):
    return (start << 32) | length


def mix(key):
    x = key & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def slot_lds(key, lds_slots):
    return mix(key) & (lds_slots - 1)


def slot_global(key, log2_capacity):
    return (mix(key) >> 32) & ((1 << log2_capacity) - 1)


def colliding_keys(slot_fn, starts, length, how_many=2):
    """The first ``how_many`` keys (start, length) with start in ``starts`` that share a slot under ``slot_fn``."""
    seen = {}
    for s in starts:
        group = seen.setdefault(slot_fn(key_of(s, length)), [])
        group.append(s)
        if len(group) == how_many:
            return [(g, length) for g in group]
    raise AssertionError("no collision found")
