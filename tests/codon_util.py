"""TEST INFRASTRUCTURE of the codon tallies: a plain restatement of the table over Segments, written
from the definitions and from nothing in amplipy_amd/csrc; the checks that pin it to the reference-pinned oracle's count table;
CDS sets and crafted reads the codon tests share; and the synthetic job of the command-line tests."""
import bisect
import re

import numpy as np

from amplipy_amd import codon as codon_mod, synth
from amplipy_amd.batch import ReadBatch
from tests import strand_util as S

CELLS = 65
BROKEN = 64
BASE = {"A": 0, "C": 1, "G": 2, "T": 3}
_REGULAR = re.compile(r"H*S*[MIDN=X]+S*H*")


# ---- the restatement --------------------------------------------------------------------------------------------------------
def is_regular(seg, ref_len):
    """Hard clips, soft clips, a core of M = X I D N ops, soft clips, hard clips; the query bases add up to l_seq; QUAL is
    there; the alignment lies inside the reference."""
    ops = seg.cigartuples or []
    if seg.query_length <= 0 or seg.query_qualities is None or seg.reference_start < 0:
        return False
    if any(op > 8 for op, _ in ops) or not _REGULAR.fullmatch("".join("MIDNSHP=X"[op] for op, _ in ops)):
        return False
    if sum(n for op, n in ops if op in (0, 1, 4, 7, 8)) != seg.query_length:
        return False
    return seg.reference_start + sum(n for op, n in ops if op in (0, 2, 3, 7, 8)) <= ref_len


def read_adds(seg, ref_len, starts, min_quality):
    """[(slot, cell)] of a read with status 0, or None when the read is not regular.  ``starts``: a sorted list."""
    if not is_regular(seg, ref_len):
        return None
    seq, qual = seg.query_sequence.upper(), seg.query_qualities
    where = {}                              # reference position -> (query index, match segment)
    q, r, run = 0, seg.reference_start, 0
    for op, n in seg.cigartuples:
        if op in (0, 7, 8):
            for k in range(n):
                where[r + k] = (q + k, run)
            q += n; r += n
        elif op in (1, 4):
            q += n
            run += 1 if op == 1 and n > 0 else 0        # an inserted base ends the match segment
        elif op in (2, 3):
            r += n
            run += 1 if n > 0 else 0                    # ... and so does a deleted or skipped one
    out = []
    for slot in range(bisect.bisect_left(starts, seg.reference_start), bisect.bisect_right(starts, r - 3)):
        p = starts[slot]
        at = [where.get(p + k) for k in range(3)]
        if None in at or len({run for _, run in at}) != 1:
            out.append((slot, BROKEN))      # inside [pos, ref_end), inside no single match segment
        elif all(qual[i] >= min_quality and seq[i] in BASE for i, _ in at):
            out.append((slot, 16 * BASE[seq[at[0][0]]] + 4 * BASE[seq[at[1][0]]] + BASE[seq[at[2][0]]]))
    return out


def tables(segments, ref_len, starts, min_quality):
    """(codon uint32[n_slots][65], reads uint64[2]) of reads with status 0, Python integers all the way."""
    starts = [int(s) for s in starts]
    codon = [[0] * CELLS for _ in starts]
    reads = [0, 0]
    for seg in segments:
        adds = read_adds(seg, ref_len, starts, min_quality)
        reads[adds is None] += 1
        for slot, cell in adds or ():
            codon[slot][cell] += 1
    return np.array(codon, np.uint32).reshape(len(starts), CELLS), np.array(reads, np.uint64)


# ---- the oracle's word on the table -----------------------------------------------------------------------------------------
def marginals(codon):
    """uint64[n_slots][3][4]: per slot, offset k and base b the sum of the triplets with b at offset k."""
    c = np.asarray(codon)[:, :64].astype(np.uint64).reshape(-1, 4, 4, 4)
    return np.stack([c.sum(axis=(2, 3)), c.sum(axis=(1, 3)), c.sum(axis=(1, 2))], axis=1)


def check_at_most_counts(codon, starts, counts):
    """Invariant 1: no marginal exceeds the ORACLE's count of that base at that position."""
    m = marginals(codon)
    st = np.asarray(starts, np.int64)
    for k in range(3):
        assert (m[:, k, :] <= counts[st + k, :4]).all(), k


def check_equal_counts(codon, starts, counts, covered):
    """Invariant 2 (single-M reads without N, every quality good, whole codons of one frame): the marginals ARE the count table
    on every covered position, and no codon is broken.  ``covered``: bool[G]."""
    m = marginals(codon)
    st = np.asarray(starts, np.int64)
    assert not np.asarray(codon)[:, BROKEN].any()
    seen = np.zeros(len(covered), bool)
    for k in range(3):
        assert np.array_equal(m[:, k, :], counts[st + k, :4].astype(np.uint64)), k
        seen[st + k] = True
    assert not (covered & ~seen).any() and not counts[:, 4:].any()


# ---- CDS sets ---------------------------------------------------------------------------------------------------------------
def cds_set(rows, ref_len):
    return codon_mod.CdsSet(rows, ref_len)


def three_frames(ref_len, lo=0):
    """Three rows over (nearly) the whole reference, one per frame, the middle one on the reverse strand: every position from
    lo on starts a codon."""
    rows = []
    for f, strand in ((0, "+"), (1, "-"), (2, "+")):
        n = (ref_len - lo - f) // 3
        if n > 0:
            rows.append(("frame%d" % f, lo + f, lo + f + 3 * n, strand))
    return cds_set(rows, ref_len)


def one_frame(ref_len, lo=0):
    return cds_set([("orf", lo, lo + 3 * ((ref_len - lo) // 3), "+")], ref_len)


def overlapping(ref_len):
    """ORF1a / ORF1b style: two rows that overlap out of frame, a third inside the first on the other strand, one far away."""
    a = ref_len // 10
    rows = [("orf1a", a, a + 3 * (ref_len // 9), "+"), ("orf1b", a + 3 * (ref_len // 9) - 4, a + 3 * (ref_len // 9) - 4 + 3 * (ref_len // 12), "+"),
            ("inner", a + 8, a + 8 + 3 * (ref_len // 30), "-"), ("far", ref_len - 3 * (ref_len // 20), ref_len, "+")]
    return cds_set(rows, ref_len)


def whole_codon_reads(n, ref_len, frame, rng, max_codons=40):
    """Single-M reads without N, every quality >= 30, each covering whole codons of the frame only."""
    segs = []
    last = (ref_len - frame) // 3
    for _ in range(n):
        k = int(rng.integers(1, min(max_codons, last) + 1))
        j = int(rng.integers(0, last - k + 1))
        segs.append(S.seg(frame + 3 * j, [(0, 3 * k)], rng, flag=int(rng.integers(0, 2)) * 0x10, qual=int(rng.integers(30, 41))))
    return segs


# ---- the synthetic job of the command-line tests ----------------------------------------------------------------------------
def _edit(seg, changes):
    """The read's bases at reference positions ``changes`` {position: base} replaced (where it has a match base there)."""
    seq = list(seg.query_sequence)
    for q, r in seg.get_aligned_pairs():
        if q is not None and r in changes:
            seq[q] = changes[r]
    seg.query_sequence = "".join(seq)


def synthetic_job(n=3000, seed=17):
    """About ``n`` reads of three neighbouring amplicons of the synthetic ARTIC scheme, with three constructions inside the
    second one's left end, where CDS row orfA has codons at pa, pb and pc (reference codon CGG = R at pa and pb):
      (a) at pa, AAG (K) on about 60 % of the reads -- read one substitution at a time that is AGG (R) and CAG (Q);
      (b) at pb, AGG on about 30 % of the reads and CAG on another 30 %: never both;
      (c) at pc, the three bases deleted from about half of the single-M reads that reach 6 bases past either side.
    -> dict(genome (codes), primers, rows (CDS rows), segments, pa, pb, pc)."""
    g = synth.make_genome().copy()
    primers, amps = synth.make_artic_scheme()
    a0 = int(amps[10, 0])
    start = a0 + 40
    pa, pb, pc = start + 15, start + 30, start + 45
    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    for p in (pa, pb):
        g[p:p + 3] = [code[b] for b in "CGG"]
    batch = synth.make_amplicon_batch(g, amps[9:12], n, seed, sub_rate=0.0)
    rng = np.random.default_rng(seed + 1)
    segs = []
    for i in range(batch.n):
        s = batch.segment(i)
        u = rng.random(3)
        if u[0] < 0.6:
            _edit(s, {pa: "A", pa + 1: "A"})
        if u[1] < 0.3:
            _edit(s, {pb: "A"})
        elif u[1] < 0.6:
            _edit(s, {pb + 1: "A"})
        ops = s.cigartuples
        if u[2] < 0.5 and len(ops) == 1 and s.reference_start <= pc - 6 and s.reference_start + ops[0][1] >= pc + 9:
            cut = pc - s.reference_start
            s.cigartuples = [(0, cut), (2, 3), (0, ops[0][1] - cut - 3)]
            s.query_sequence = s.query_sequence[:cut] + s.query_sequence[cut + 3:]
            quals = list(s.query_qualities)
            s.query_qualities = type(s.query_qualities)("B", quals[:cut] + quals[cut + 3:])
        segs.append(s)
    rows = [("orfA", start, start + 90, "+"), ("orfB", start + 10, start + 10 + 60, "-"), ("orfC", start + 2, start + 2 + 300, "+"),
            ("tail", int(g.size) - 300, int(g.size), "-")]
    return dict(genome=g, primers=primers, rows=rows, batch=ReadBatch.from_segments(segs), pa=pa, pb=pb, pc=pc)


# ---- crafted reads ----------------------------------------------------------------------------------------------------------
def cell_of(triplet):
    return 16 * BASE[triplet[0]] + 4 * BASE[triplet[1]] + BASE[triplet[2]]


def _read(pos, cigar, seq, qual=35, flag=0):
    from amplipy_amd.segment import Segment
    return Segment(flag=flag, reference_start=pos, cigar=cigar, query_sequence=seq, query_qualities=[qual] * len(seq) if isinstance(qual, int) else qual)


def crafted(W, slots, block=256):
    """[(name, G, CdsSet, segments, min_quality, expect)]: ``expect(codon, reads, cds)`` asserts what the case is about on a table
    (the restatement's, the twin's, the device's).  W: slots of the window, slots: list entries per read."""
    rng = np.random.default_rng(23)
    out = []
    G = 600
    one = one_frame(G)                      # codons at 0, 3, 6, ...
    row = lambda cds, p: cds.slot_of(p)

    def case(name, G, cds, segs, mq, expect):
        out.append((name, G, cds, segs, mq, expect))

    # a codon at the read's first and last three bases; a codon cut by the read's end is neither counted nor broken
    def e(c, r, cds):
        assert c[row(cds, 30)].tolist().count(1) == 1 and c[row(cds, 30), cell_of("ACG")] == 1 and c[row(cds, 36), cell_of("TTA")] == 1
        assert not c[row(cds, 27)].any() and not c[row(cds, 39)].any() and int(c.sum()) == 3 and list(r) == [1, 0]
    case("first_last_cut", G, one, [_read(30, [(0, 10)], "ACGCCCTTAG")], 20, e)

    # an insertion between offsets 0|1 and between 1|2: broken; in front of offset 0: not
    def e(c, r, cds):
        assert c[row(cds, 33), BROKEN] == 1 and c[row(cds, 45), BROKEN] == 1 and int(c[:, BROKEN].sum()) == 2
        assert c[row(cds, 54), cell_of("GGG")] == 1 and c[row(cds, 51), cell_of("AAA")] == 1
    case("insertions", G, one, [_read(30, [(0, 4), (1, 2), (0, 5)], "AAAA" "TT" "CCCCC"), _read(42, [(0, 5), (1, 1), (0, 4)], "AAAAA" "T" "CCCC"),
                                _read(51, [(0, 3), (1, 2), (0, 3)], "AAA" "TT" "GGG")], 20, e)

    # a 1-base and a 3-base in-frame deletion; two deletions touching one codon: broken once
    def e(c, r, cds):
        assert c[row(cds, 33), BROKEN] == 1 and c[row(cds, 63), BROKEN] == 1 and c[row(cds, 93), BROKEN] == 1
        assert int(c[:, BROKEN].sum()) == 3 and c[row(cds, 60), cell_of("AAA")] == 1 and c[row(cds, 66), cell_of("CCC")] == 1
    case("deletions", G, one, [_read(30, [(0, 4), (2, 1), (0, 4)], "AAAA" "CCCC"), _read(60, [(0, 3), (2, 3), (0, 3)], "AAA" "CCC"),
                               _read(90, [(0, 3), (2, 1), (0, 1), (2, 1), (0, 3)], "AAA" "G" "CCC")], 20, e)

    # a soft clip next to a codon; one low-quality base or one N among the three
    def e(c, r, cds):
        assert c[row(cds, 30), cell_of("ACG")] == 1 and int(c.sum()) == 2 and c[row(cds, 69), cell_of("GGG")] == 1
    case("clip_lowq_n", G, one, [_read(30, [(4, 2), (0, 3), (4, 2)], "TT" "ACG" "TT"), _read(60, [(0, 6)], "ACGACG", qual=[35, 35, 5, 35, 5, 35]),
                                 _read(66, [(0, 6)], "ANGGGG")], 20, e)

    # a slot at G - 3, a reference of 3 bases
    def e(c, r, cds):
        assert c[-1, cell_of("CAT")] == 1 and int(c.sum()) == 1
    case("slot_at_G_minus_3", G, one, [_read(G - 4, [(0, 4)], "GCAT")], 20, e)
    case("reference_of_3", 3, one_frame(3), [_read(0, [(0, 3)], "CAT"), _read(1, [(0, 2)], "AT")], 20, e)

    # more list entries than the read has room for: the read goes serially, its neighbours take the window
    def e(c, r, cds):
        assert list(r) == [4, 0] and int(c[:, BROKEN].sum()) > slots
    many = S.many_segment_cigar(slots)      # 2M 1D repeated: one entry of broken codons (merged), and no match segment of 3 bases but the last
    wide = []
    for _ in range(slots):
        wide += [(0, 6), (2, 1)]
    wide += [(0, 6)]                        # 6M 1D repeated: 2 * slots + 1 entries
    case("more_entries_than_slots", G, three_frames(G), [S.seg(10, [(0, 50)], rng), S.seg(12, wide, rng), S.seg(12, many, rng), S.seg(14, [(0, 9), (1, 2), (0, 9)], rng)], 20, e)

    # three overlapping frames: the window spans W / 3 codons of each; tiles that span W - 1, W, W + 1 and 3 W slots
    for span in (W - 1, W, W + 1, 3 * W):
        G3 = 4 * W + 100

        def e(c, r, cds, span=span):
            assert list(r) == [2 * block + 2, 0] and c[:, :64].sum() > 0
        # (every position starts a codon: a tile from 5 to 5 + span takes span slots of a window anchored at the slot of 5 - 2)
        segs = [S.seg(5, [(0, 40)], rng) for _ in range(block)] + [S.seg(5, [(0, 40)], rng), S.seg(5 + span - 40, [(0, 40)], rng)] + \
               [S.seg(5 + span - 40, [(0, 40)], rng) for _ in range(block)]
        case("span_%d" % span, G3, three_frames(G3), segs, 20, e)

    # min_quality 0, and a min_quality above every quality: only cell 64 is left
    segs = [S.seg(30, [(0, 21), (2, 3), (0, 21)], rng), S.seg(33, [(0, 22), (1, 3), (0, 20)], rng, qual=0)]

    def e(c, r, cds):
        assert int(c[:, :64].sum()) == 7 + 7 + 7 + 6 and int(c[:, BROKEN].sum()) == 1 + 1
    case("min_quality_0", G, one, segs, 0, e)

    def e(c, r, cds):
        assert int(c[:, :64].sum()) == 0 and int(c[:, BROKEN].sum()) == 2
    case("min_quality_200", G, one, segs, 200, e)
    return out
