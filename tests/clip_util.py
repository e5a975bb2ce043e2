"""TEST INFRASTRUCTURE: a plain restatement of the clip table of the QC report over the rows of a
ReadBatch, written from the rule and from nothing in amplipy_amd/csrc, in Python integers read after read.  Plus the crafted
reads and the wave-shaped batches the clip tests share."""
import numpy as np

from amplipy_amd.batch import ReadBatch, unpack_nibbles
from amplipy_amd.segment import Segment

K, COLS, CELLS = 16, 5, 82
LEFT, RIGHT = 0, 1
REF_OPS = (0, 2, 3, 7, 8)
COL_OF = {1: 0, 2: 1, 4: 2, 8: 3}


def scan(ops, pos, lseq, ref_len):
    """ops: [(op, length)] -> None when the read is skipped, else (L_left, L_right, reference length)."""
    left = 0
    k = 0
    while k < len(ops) and ops[k][0] in (4, 5):
        if ops[k][0] == 4:
            left += ops[k][1]
        k += 1
    if k == len(ops):
        return None                                   # no op other than H / S
    right = 0
    b = len(ops) - 1
    while b >= 1 and ops[b][0] in (4, 5):             # element 0 is never examined from the back
        if ops[b][0] == 4:
            right += ops[b][1]
        b -= 1
    ref = sum(l for op, l in ops if op in REF_OPS)
    if lseq <= 0 or left + right > lseq or pos < 0 or pos + ref > ref_len:
        return None
    return left, right, ref


def tables(batch, ref_len, clip_min, status=None):
    """(table uint32[ref_len + 1][2][CELLS], scalars uint64[4]: scanned, skipped, left, right) of one batch."""
    table = np.zeros((ref_len + 1, 2, CELLS), np.uint32)
    scalars = [0, 0, 0, 0]
    for i in range(batch.n):
        if status is not None and int(status[i]) != 0:
            continue
        ops = [(int(w) & 15, int(w) >> 4) for w in batch.cig[int(batch.cig_off[i]):int(batch.cig_off[i + 1])]]
        lseq, pos = int(batch.lseq[i]), int(batch.pos[i])
        got = scan(ops, pos, lseq, ref_len)
        if got is None:
            scalars[1] += 1
            continue
        scalars[0] += 1
        left, right, ref = got
        o = int(batch.seq_off[i])
        codes = unpack_nibbles(batch.seq[o // 2:(o + lseq + 1) // 2], lseq).tolist()
        rev = 1 if int(batch.flag[i]) & 0x10 else 0
        for side, L, p in ((LEFT, left, pos), (RIGHT, right, pos + ref)):
            if L < clip_min:
                continue
            scalars[2 + side] += 1
            cells = table[p, side]
            cells[0] += 1
            cells[1] += rev
            for j in range(min(L, K)):
                q = L - 1 - j if side == LEFT else lseq - L + j
                cells[2 + j * COLS + COL_OF.get(codes[q], 4)] += 1
    return table, np.array(scalars, np.uint64)


# ---- crafted reads --------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def seg(pos, cigar, rng, flag=0, seq=None, qual=True):
    """A Segment with a seeded SEQ of the CIGAR's query length (``seq``: the text itself; '*' gives a read without bases)."""
    qlen = sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    if seq == "*":
        return Segment(flag=flag, reference_start=int(pos), cigar=cigar, template_length=0, query_sequence=None, query_qualities=None)
    if seq is None:
        seq = _ACGT[rng.integers(0, 4, size=qlen)].tobytes().decode("ascii")
    quals = rng.integers(25, 40, size=len(seq)).tolist() if qual else None
    return Segment(flag=flag, reference_start=int(pos), cigar=cigar, template_length=0, query_sequence=seq, query_qualities=quals)


def crafted_batch(G, clip_min, seed=11):
    """The edge cases of the rule on a reference of G bases (G >= 400), each twice: once as it stands and once with FLAG 0x10."""
    rng = np.random.default_rng(seed)
    S, M, H, I, D = 4, 0, 5, 1, 2
    segs = []
    lengths = sorted({0, clip_min - 1, clip_min, 15, 16, 17})
    for L in lengths:                                    # clips of every length at either end, and both; even and odd offsets
        for pos in (100, 101):
            if L:
                segs.append(seg(pos, [(S, L), (M, 50)], rng))
                segs.append(seg(pos, [(M, 50), (S, L)], rng))
                segs.append(seg(pos, [(S, L), (M, 51), (S, L + 1)], rng))
                segs.append(seg(pos, [(S, L + 1), (M, 51), (S, L)], rng))
            else:
                segs.append(seg(pos, [(M, 50)], rng))
    segs.append(seg(120, [(S, 59), (M, 1)], rng))        # L = lseq - 1
    segs.append(seg(120, [(M, 1), (S, 59)], rng))
    segs.append(seg(130, [(H, 5), (S, 20), (M, 40), (S, 20), (H, 3)], rng))      # H in front of S and behind it
    segs.append(seg(130, [(S, 12), (H, 5), (S, 8), (M, 40), (S, 8), (H, 2), (S, 12)], rng))      # H between the S ops: both are summed
    segs.append(seg(140, [(S, 30)], rng))                # an S-only read
    segs.append(seg(140, [(H, 4), (S, 30), (H, 4)], rng))
    segs.append(seg(150, [(M, 40)], rng, seq="*"))       # SEQ '*'
    segs.append(seg(150, [(S, 20), (M, 40)], rng, seq="*"))
    segs.append(seg(160, [(S, 20), (M, 40), (S, 20)], rng, seq="ACGT" * 9))      # L_left + L_right > lseq: 40 > 36
    segs.append(seg(G - 40, [(S, 20), (M, 40)], rng))    # ends on the reference's last base; no right clip
    segs.append(seg(G - 40, [(M, 40), (S, 20)], rng))    # a RIGHT site at ref_len
    segs.append(seg(0, [(S, 20), (M, 40)], rng))         # a LEFT site at 0
    segs.append(seg(G - 39, [(M, 40), (S, 20)], rng))    # runs past the reference
    segs.append(seg(G + 5, [(S, 20), (M, 10)], rng))
    segs.append(seg(-3, [(S, 20), (M, 40)], rng))        # in front of the reference
    segs.append(seg(200, [(S, 18), (M, 30), (I, 2), (M, 10), (D, 7), (M, 20), (S, 11)], rng))      # D counts for the RIGHT site, I does not
    segs.append(seg(200, [(S, 20), (M, 40)], rng, seq="ACGTN=RYKM" * 2 + "A" * 40))      # N, = and IUPAC codes among the clipped bases
    segs.append(seg(201, [(M, 40), (S, 20)], rng, seq="C" * 40 + "NNACGT=SWBDHVACGT"[:17] + "ACG"))
    segs.append(seg(210, [(S, 25), (M, 40)], rng, qual=False))      # QUAL '*' takes part
    flipped = [Segment(flag=g.flag | 0x10, reference_start=g.reference_start, cigar=list(g.cigartuples), template_length=0,
                       query_sequence=g.query_sequence, query_qualities=g.query_qualities) for g in segs]
    return ReadBatch.from_segments(segs + flipped)


def wave_batch(kind, n, G, seed, clip=20):
    """n reads shaped for the kernel's wave combine.  'one_site': every read clipped at one LEFT and one RIGHT site;
    'distinct': every read a site of its own on either side; 'mixed': piles of random size among lone reads; 'left_only' /
    'right_only' / 'none': no read has a clip of the other side / of either."""
    rng = np.random.default_rng(seed)
    segs = []
    for k in range(n):
        if kind == "one_site":
            pos = 300
        elif kind == "distinct":
            pos = 100 + k % (G - 300)
        else:
            pos = 100 + int(rng.integers(0, 6)) * 7 if rng.random() < 0.7 else 100 + int(rng.integers(0, G - 300))
        left = kind in ("one_site", "distinct", "left_only") or (kind == "mixed" and rng.random() < 0.6)
        right = kind in ("one_site", "distinct", "right_only") or (kind == "mixed" and rng.random() < 0.6)
        cig = ([(4, clip + int(rng.integers(0, 3)))] if left else []) + [(0, 60)] + ([(4, clip - int(rng.integers(0, 8)))] if right else [])
        segs.append(seg(pos, cig, rng, flag=0x10 if rng.random() < 0.4 else 0))
    return ReadBatch.from_segments(segs)
