"""TEST INFRASTRUCTURE of the strand and base-quality tallies: a plain restatement of the tables over
Segments, written from the definitions and from nothing in amplipy_amd/csrc; the seeded inputs the strand tests share; and the
two constructions that pin the restatement to the reference-pinned oracle -- the count table of the reverse reads alone is
``rev``, and the count tables of a sweep of quality thresholds add up to ``qsum``."""
import numpy as np

from amplipy_amd import abi, synth
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from tests import qc_util as Q

COL = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
QSUM_COLS = 5


# ---- the restatement --------------------------------------------------------------------------------------------------------
def read_adds(seg, min_quality):
    """[(reference position, column, quality)] of every increment update_base_counts makes to one of the six fixed keys for
    this read (status 0: nothing raises).  Column 5 is '-', its quality 0."""
    qs, qe = seg.query_alignment_start, seg.query_alignment_end
    seq, qual = seg.query_sequence.upper(), seg.query_qualities
    pairs = seg.get_aligned_pairs()
    out = []
    i = 0
    while i < len(pairs):
        q, r = pairs[i]
        i += 1
        if q is None:                       # a deleted position counts whatever surrounds it
            out.append((r, 5, 0))
        elif qual[q] < min_quality:         # the quality test comes first ...
            continue
        elif q < qs:                        # ... then the leading soft clip ...
            continue
        elif q >= qe:                       # ... and the first good base at or past the alignment end ends the read
            break
        elif r is None:                     # an insertion: its scan takes pairs with it, and hands the last one back when it has a position
            while r is None and q < qe and qual[q] >= min_quality:
                q, r = pairs[i]
                i += 1
            if r is not None:
                i -= 1
        else:
            out.append((r, COL[seq[q]], qual[q]))
    return out


def tables(segments, ref_len, min_quality):
    """(counts uint32[G][6], rev uint32[G][6], qsum uint64[G][5]) of the reads, Python integers all the way."""
    counts = [[0] * abi.NSYM for _ in range(ref_len)]
    rev = [[0] * abi.NSYM for _ in range(ref_len)]
    qsum = [[0] * QSUM_COLS for _ in range(ref_len)]
    for seg in segments:
        is_rev = bool(seg.flag & 0x10)
        for r, c, q in read_adds(seg, min_quality):
            counts[r][c] += 1
            if is_rev:
                rev[r][c] += 1
            if c < QSUM_COLS:
                qsum[r][c] += q
    return np.array(counts, np.uint32).reshape(ref_len, abi.NSYM), np.array(rev, np.uint32).reshape(ref_len, abi.NSYM), \
        np.array(qsum, np.uint64).reshape(ref_len, QSUM_COLS)


def walked_segments(batch, res=None):
    """The reads as they are counted: with trim results ``res`` (abi.TrimResult) the trimmed alignment of the reads with status
    0, without them the reads as they came in."""
    out = []
    for i in range(batch.n):
        s = batch.segment(i)
        if res is not None:
            if int(res.status[i]) != 0:
                continue
            s.reference_start = int(res.new_pos[i])
            s.cigartuples = res.cigar_ops(i)
        out.append(s)
    return out


def walked_batch(batch, res=None):
    return ReadBatch.from_segments(walked_segments(batch, res))


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
def strand_batch(n, ref_len, primers, seed, sort=True):
    """``n`` reads of the QC tests' mix (qc_util.mixed_batch without its bad read) with the strand flags drawn again: about
    half the reads reverse, paired and unpaired; the paired reverse reads of the mix keep their insert size."""
    b = Q.mixed_batch(n, ref_len, primers, seed, bad_read=False, sort=False)
    rng = np.random.default_rng(seed + 7919)
    draw = rng.choice(np.array([0x0, 0x10, 0x1 | 0x20, 0x1 | 0x10], np.uint16), size=b.n)
    b.flag = np.where(b.flag == 0, draw, b.flag).astype(np.uint16)
    if sort and b.n:
        b = synth.gather_rows(b, np.argsort(b.pos, kind="stable"))
    return b


def seg(pos, cigar, rng, flag=0, qual=None):
    """One read with seeded bases; qualities 25..39 unless given (a list, or one value for every base)."""
    qlen = sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    seq = Q._ACGT[rng.integers(0, 4, size=qlen)].tobytes().decode("ascii")
    if qual is None:
        qual = rng.integers(25, 40, size=qlen).tolist()
    elif isinstance(qual, int):
        qual = [qual] * qlen
    return Segment(flag=flag, reference_start=int(pos), cigar=cigar, query_sequence=seq, query_qualities=qual)


def many_segment_cigar(n_pairs):
    """2M 1D repeated: 2 * n_pairs + 1 ops, n_pairs + 1 match segments and n_pairs deletions."""
    cig = []
    for _ in range(n_pairs):
        cig += [(0, 2), (2, 1)]
    return cig + [(0, 3)]


# ---- the oracle's word on the tables ----------------------------------------------------------------------------------------
def oracle_counts(process, batch, ref_len, tables_, min_quality, window, do_trim):
    """``process``: oracle.process.  -> (counts, trim results); every read must have status 0."""
    mn, mx, mpl = tables_ if tables_ is not None else (None, None, 0)
    r = process(batch, ref_len, mn, mx, mpl, min_quality, window, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    return r.counts, r.trim


def oracle_rev(process, batch, ref_len, tables_, min_quality, window, do_trim):
    """``rev`` by the oracle: the count table of the batch's reverse reads alone.  Also checks that the forward and the reverse
    reads' tables add up to the batch's."""
    is_rev = (batch.flag & 0x10) != 0
    parts = []
    for mask in (is_rev, ~is_rev):
        sub = synth.gather_rows(batch, np.nonzero(mask)[0])
        parts.append(oracle_counts(process, sub, ref_len, tables_, min_quality, window, do_trim)[0] if sub.n
                     else np.zeros((ref_len, abi.NSYM), np.uint32))
    whole = oracle_counts(process, batch, ref_len, tables_, min_quality, window, do_trim)[0]
    assert np.array_equal(parts[0].astype(np.uint64) + parts[1], whole)
    return parts[0], whole


def oracle_qsum(process, walked, ref_len, min_quality, window=4):
    """``qsum`` by the oracle: the already trimmed batch ``walked`` counted without trimming at every threshold t from
    min_quality to one past the largest quality.  A base of quality v >= min_quality is in N(t) for t <= v, so
    min_quality * N(min_quality) + sum over t > min_quality of N(t) counts it v times.  -> (qsum, N(min_quality))."""
    qmax = int(walked.qual.max()) if walked.qual.size else 0
    first = oracle_counts(process, walked, ref_len, None, min_quality, window, False)[0]
    total = first[:, :QSUM_COLS].astype(np.uint64) * np.uint64(min_quality)
    for t in range(min_quality + 1, qmax + 2):
        total += oracle_counts(process, walked, ref_len, None, t, window, False)[0][:, :QSUM_COLS]
    return total, first
