"""Shared by the SAM-text tests: seeded SAM text, the Python codec of bamio applied to a chunk of bytes, and the host twin of the
device codec (amplipy_amd/csrc/amp_sam.hip compiled with -DAMPSAM_HOSTSIM)."""
import io
import os

import numpy as np

from amplipy_amd import bamio, sam_native
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment

REF_NAME = "SYN_REF"


def header(ref_len, pg=True):
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n@SQ\tSN:OTHER\tLN:1000\n" % (REF_NAME, ref_len)
    if pg:
        text += "@PG\tID:sim\tPN:sim\n"
    return bamio.Header(text, [(REF_NAME, ref_len), ("OTHER", 1000)])


def ref_names(hdr):
    return [n for n, _ in hdr.refs]


AUX_POOL = ["NM:i:1", "AS:i:290", "XS:A:+", "MD:Z:12A30^CG5", "RG:Z:grp 1 lane 2", "XA:Z:chr1,+100,50M,0;", "ZB:B:c,1,-2,3", "YF:f:0.25",
            "ZH:H:1AE301", "XT:A:U", "X0:i:1", "X1:i:0", "XM:i:0", "XO:i:0", "XG:i:0", "SA:Z:OTHER,5,+,10S20M,60,0;", "MC:Z:150M", "MQ:i:60",
            "ms:i:270", "CO:Z:a comment with spaces"]


def segments_to_lines(segs, hdr, rng, max_aux=4, paired=True):
    """One SAM line (bytes, LF) per segment, rendered by bamio.AlignmentWriter in text mode."""
    out = io.StringIO()
    w = bamio.AlignmentWriter(None, "w", hdr, fileobj=out)
    start = out.tell()
    for i, s in enumerate(segs):
        q = s.query_qualities
        n_aux = int(rng.integers(0, max_aux + 1))
        aux = [AUX_POOL[int(k)] for k in rng.choice(len(AUX_POOL), n_aux, replace=False)]
        mate = bool(paired and (s.flag & 1) and rng.random() < 0.8)
        w.write(bamio.Rec("read%d/%d" % (i, int(rng.integers(0, 1000))), s.flag, 0, s.reference_start, int(rng.integers(0, 61)), s.cigartuples,
                          0 if mate else -1, int(rng.integers(0, 29000)) if mate else -1, s.template_length,
                          s.query_sequence, None if q is None else bytes(q), aux_sam=aux))
    text = out.getvalue()[start:]
    return [l.encode("ascii") + b"\n" for l in text.split("\n")[:-1]]


def many_op_segments(rng, n, ref_len, max_len=600, max_ops=16):
    """Reads whose CIGARs have many ops (M / = / X alternating with I / D / N), optional soft clips."""
    segs = []
    for _ in range(n):
        n_body = int(rng.integers(1, max_ops // 2 + 1)) * 2 - 1
        L_target = int(rng.integers(50, max_len + 1))
        ops, q = [], 0
        if rng.random() < 0.4:
            k = int(rng.integers(1, 30)); ops.append((4, k)); q += k
        per = max(1, (L_target - q) // ((n_body + 1) // 2))
        for b in range(n_body):
            if b % 2 == 0:
                k = int(rng.integers(1, per + 1)); ops.append((int(rng.choice([0, 0, 7, 8])), k)); q += k
            else:
                op = int(rng.choice([1, 2, 3])); k = int(rng.integers(1, 9)); ops.append((op, k)); q += k if op == 1 else 0
        if rng.random() < 0.4:
            k = int(rng.integers(1, 30)); ops.append((4, k)); q += k
        span = sum(k for o, k in ops if o in (0, 2, 3, 7, 8))
        pos = int(rng.integers(0, max(1, ref_len - span - 1)))
        seq = "".join(rng.choice(list("ACGTN"), q, p=[0.245, 0.245, 0.245, 0.245, 0.02]))
        qual = rng.choice([37, 25, 11, 2], q, p=[0.8, 0.12, 0.06, 0.02]).astype(np.uint8)
        segs.append(Segment(flag=int(rng.choice([0, 16, 99, 147])), reference_start=pos, cigar=ops,
                            template_length=int(rng.integers(-500, 500)), query_sequence=seq, query_qualities=qual.tolist()))
    return segs


# ---- the Python codec on a chunk of bytes ----------------------------------------------------------------------------------------
def python_records(chunk, hdr):
    """(Rec list, number of lines) of a chunk: decoded and split the way the text-mode reader does it."""
    lines = list(io.TextIOWrapper(io.BytesIO(chunk)))
    return list(bamio.AlignmentReader.for_header(hdr).records_of(lines)), len(lines)


def python_batch(recs):
    return ReadBatch.from_segments([r.to_segment() for r in recs])


def python_text(recs, batch, hdr, new_pos, cigars, keep):
    """What AlignmentWriter.write(r, pos=, cigar=) writes for the kept rows: bytes."""
    out = io.StringIO()
    w = bamio.AlignmentWriter(None, "w", hdr, fileobj=out)
    start = out.tell()
    for k in range(batch.n):
        if keep[k]:
            w.write(recs[int(batch.src_index[k])], pos=int(new_pos[k]), cigar=cigars[k])
    return out.getvalue()[start:].encode()


def keep_rule(res, min_length, include_no_primer):
    keep = (res.ref_len >= min_length) & (((res.trim_flags & 3) != 0) | bool(include_no_primer))      # AmpliPy.py:910
    bad = np.nonzero(res.status)[0]
    if len(bad):
        keep[int(bad[0]):] = False
    return keep


class IdentityResult:
    """Trim results that change nothing: new POS and CIGAR = the input's; every row kept by the rule with include_no_primer."""

    def __init__(self, batch):
        n = batch.n
        self.new_pos = batch.pos.copy()
        self.new_ncig = (batch.cig_off[1:] - batch.cig_off[:-1]).astype(np.uint32)
        self.new_cig = np.zeros(batch.cig.size + 3 * n, np.uint32)
        for i in range(n):
            a, b = int(batch.cig_off[i]), int(batch.cig_off[i + 1])
            self.new_cig[a + 3 * i:b + 3 * i] = batch.cig[a:b]
        self.ref_len = np.full(n, 1 << 20, np.int32)
        self.trim_flags = np.zeros(n, np.uint8)
        self.status = np.zeros(n, np.uint8)


def result_cigars(batch, res):
    return [[(int(v) & 15, int(v) >> 4) for v in res.new_cig[int(batch.cig_off[i]) + 3 * i:int(batch.cig_off[i]) + 3 * i + int(res.new_ncig[i])]]
            for i in range(batch.n)]


def same_batch(a, b):
    """'' when two ReadBatch objects are equal in all ten arrays and src_index, else what differs."""
    if a.n != b.n:
        return "n %d != %d" % (a.n, b.n)
    for f in ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual", "src_index"):
        x, y = getattr(a, f), getattr(b, f)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return f
    return ""


# ---- the twin ----------------------------------------------------------------------------------------------------------------------
_TWIN = {}


def twin_path(tmpdir, sanitize=False, main_source=None):
    key = (sanitize, main_source)
    if key not in _TWIN:
        name = "sam_twin_main" if main_source else "libampsam_twin.so"
        _TWIN[key] = sam_native.build_twin(os.path.join(str(tmpdir), ("asan_" if sanitize else "") + name), sanitize=sanitize, main_source=main_source)
    return _TWIN[key]
