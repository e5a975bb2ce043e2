"""TEST INFRASTRUCTURE of the read-position tallies: a plain restatement of the table over Segments,
written from the definitions and from nothing in amplipy_amd/csrc; the closed form for a read of good match bases; and the
construction that pins the restatement to the reference-pinned oracle with no new oracle code -- the clip sweep: soft-clip t
more kept query bases at each end of every read, and the oracle's count table is the increments with d >= t."""
import numpy as np

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from tests import strand_util as S

BINS = 7
EDGES = (0, 2, 4, 8, 16, 32, 64)            # the least distance of each bin
COL = S.COL


def rp_bin(d):
    return min(6, (int(d) >> 1).bit_length())


def match_d(q, qs, qe):
    return min(q - qs, qe - 1 - q)


def del_d(q_next, qs, qe):
    return max(0, min(q_next - qs, qe - q_next) - 1)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def read_adds(seg, min_quality):
    """[(reference position, column, d)] of every increment update_base_counts makes to one of the six fixed keys for this
    read (status 0: nothing raises): strand_util.read_adds with the distance in place of the quality.  Column 5 is '-'."""
    qs, qe = seg.query_alignment_start, seg.query_alignment_end
    seq, qual = seg.query_sequence.upper(), seg.query_qualities
    pairs = seg.get_aligned_pairs()
    q_after = []                            # per pair: the query index the next pair with a query index takes
    nq = 0
    for q, r in pairs:
        if q is not None:
            nq = q + 1
        q_after.append(nq)
    out = []
    i = 0
    while i < len(pairs):
        q, r = pairs[i]
        i += 1
        if q is None:
            out.append((r, 5, del_d(q_after[i - 1], qs, qe)))
        elif qual[q] < min_quality:
            continue
        elif q < qs:
            continue
        elif q >= qe:
            break
        elif r is None:
            while r is None and q < qe and qual[q] >= min_quality:
                q, r = pairs[i]
                i += 1
            if r is not None:
                i -= 1
        else:
            out.append((r, COL[seq[q]], match_d(q, qs, qe)))
    return out


def tables(segments, ref_len, min_quality):
    """(counts uint32[G][6], hist uint32[G][6][7]) of the reads, Python integers all the way."""
    hist = [[0] * (abi.NSYM * BINS) for _ in range(ref_len)]
    for seg in segments:
        for r, c, d in read_adds(seg, min_quality):
            hist[r][c * BINS + rp_bin(d)] += 1
    hist = np.array(hist, np.uint32).reshape(ref_len, abi.NSYM, BINS)
    return hist.sum(axis=2, dtype=np.uint64).astype(np.uint32), hist


def at_least(segments, ref_len, min_quality, t):
    """uint32[G][6]: the increments with d >= t."""
    out = np.zeros((ref_len, abi.NSYM), np.uint32)
    for seg in segments:
        for r, c, d in read_adds(seg, min_quality):
            if d >= t:
                out[r, c] += 1
    return out


def closed_form(L):
    """The histogram of a read of L good match bases, all columns together: two bases per d < L // 2, one more when L is odd."""
    h = [0] * BINS
    for d in range(L // 2):
        h[rp_bin(d)] += 2
    if L % 2:
        h[rp_bin(L // 2)] += 1
    return h


# ---- the clip sweep -----------------------------------------------------------------------------------------------------------
_M, _I, _D, _N, _S, _H = 0, 1, 2, 3, 4, 5


def clipped(seg, t):
    """``seg`` with t more kept query bases at each end turned into soft clips, or None when its kept span is <= 2 t.  Consumed
    M advances the position, consumed I does not; a D / N met on the way, or left at the very edge, is dropped and advances
    the position (at the tail it is just dropped)."""
    if t == 0:
        return seg
    if seg.query_alignment_end - seg.query_alignment_start <= 2 * t:
        return None
    ops = [(int(op), int(l)) for op, l in seg.cigartuples if l > 0]
    lead_h = []; tail_h = []
    while ops and ops[0][0] == _H:
        lead_h.append(ops.pop(0))
    while ops and ops[-1][0] == _H:
        tail_h.insert(0, ops.pop())
    lead_s = tail_s = 0
    while ops and ops[0][0] == _S:
        lead_s += ops.pop(0)[1]
    while ops and ops[-1][0] == _S:
        tail_s += ops.pop()[1]
    assert all(op in (_M, _I, _D, _N, 7, 8) for op, _ in ops), "the sweep is for regular CIGARs"
    pos = seg.reference_start

    def eat(core, from_left):
        nonlocal pos
        need, took = t, 0
        while core:
            k = 0 if from_left else len(core) - 1
            op, l = core[k]
            if op in (_D, _N):
                core.pop(k)
                if from_left:
                    pos += l
                continue
            if need == 0:
                break
            take = min(l, need)
            need -= take; took += take
            if from_left and op != _I:
                pos += take
            if take == l:
                core.pop(k)
            else:
                core[k] = (op, l - take)
        assert need == 0
        return took

    lead_s += eat(ops, True)
    tail_s += eat(ops, False)
    cig = lead_h + ([(_S, lead_s)] if lead_s else []) + ops + ([(_S, tail_s)] if tail_s else []) + tail_h
    return Segment(flag=seg.flag, reference_start=pos, cigar=cig, query_sequence=seg.query_sequence, query_qualities=list(seg.query_qualities))


def sweep(process, segments, ref_len, min_quality, window=4):
    """hist by the oracle alone: N(t) is the count table of the reads clipped by t, counted without trimming, and bin b is
    N(lo_b) - N(lo_{b+1}).  -> (hist uint32[G][6][7], [N(t) for t in EDGES])."""
    tabs = []
    for t in EDGES:
        kept = [c for c in (clipped(s, t) for s in segments) if c is not None]
        if kept:
            tabs.append(S.oracle_counts(process, ReadBatch.from_segments(kept), ref_len, None, min_quality, window, False)[0].astype(np.int64))
        else:
            tabs.append(np.zeros((ref_len, abi.NSYM), np.int64))
    hist = np.zeros((ref_len, abi.NSYM, BINS), np.int64)
    for b in range(BINS):
        hist[:, :, b] = tabs[b] - (tabs[b + 1] if b + 1 < BINS else 0)
    assert (hist >= 0).all()
    return hist.astype(np.uint32), tabs


# ---- crafted reads --------------------------------------------------------------------------------------------------------------
SPANS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 300]


def good(pos, cigar, rng, flag=0):
    """A read whose every base reaches any min_quality the tests use below 40."""
    return S.seg(pos, cigar, rng, flag, qual=40)
