"""The crafted corners of the four device codecs (DESIGN.md sections 10, 12, 13, 14) in the shape a real read pass needs, shared by
tests/test_codec_corners.py (the host twins) and tests/test_gpu_codec_corners.py (the card).

The twin suites hand their twins invented results (POS 0 and -1, 0 ops, old + 3 ops); a device takes results from its own read
pass only.  So: every crafted line and record is sorted into ``good`` (the oracle accepts its row with trim on, count off) or
``failing`` (its row gets a status) -- none is dropped --, the good ones are also moved onto a primer, where the oracle does
change POS and CIGAR, and each check function renders its expectation with the Python codec from the oracle's results and
compares a codec's output with it byte for byte.  The codec is an argument: a twin, or the device.  Nothing here imports GPU
code or builds a twin."""
import numpy as np

from amplipy_amd import bam_device, bam_native, bamio, sam_native, synth
from tests import sam_util as U
from tests import test_bam_reencode_twin as BB
from tests import test_bam_to_sam_twin as BT
from tests import test_sam_text as ST
from tests import test_sam_to_bam_twin as SB

G = synth.make_genome()
GSTR = synth.genome_string(G)
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = ST.HDR                                          # of the SAM lines: SYN_REF and OTHER
BAM_HDR = BT.HDR                                      # of the BAM files: SYN_REF, chr|2, third.ref
MIN_QUALITY, WINDOW = 20, 4
_TABLES = []


def primer_tables():
    if not _TABLES:
        from oracle import oracle
        _TABLES.append(oracle.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0))
    return _TABLES[0]


def oracle_trim(batch, count=False):
    """The oracle's trim results of a batch with the tests' parameters: trim on, count off (or on)."""
    from oracle import oracle
    mn, mx, mpl = primer_tables()
    return oracle.process(batch, G.size, mn, mx, mpl, MIN_QUALITY, WINDOW, do_trim=True, do_count=count).trim


def first_status(t):
    """(first row with a status or -1, that status): what amp_*_process answers."""
    bad = np.nonzero(t.status)[0]
    return (int(bad[0]), int(t.status[bad[0]])) if len(bad) else (-1, 0)


# ---- the failing-row partition ---------------------------------------------------------------------------------------------------------
# name -> status, as the oracle gives them with trim on and count off ...
FAILING = {
    "hand": {"qstar": 6, "sstar": 6, "one_qual_star_len1": 6, "negtlen": 1, "zeros": 1},
    "corner": {"no_seq": 6, "qual_star": 6, "one_base_qual_star": 6, "pos_before": 1},
    "length": {"bases0": 6},
}
# ... and the rows that fail with counting on only
FAILING_COUNTED = {
    "hand": {"opP": 3, "long": 2, "iupac": 4},
    "corner": {"long_cigar": 2, "iupac": 4},
    "length": {},
}


def line_name(line):
    return line.split(b"\t")[0].rstrip(b"\r\n").decode("latin-1")


def line_status(line, count=False):
    recs, _ = U.python_records(line, HDR)
    pb = U.python_batch(recs)
    return int(oracle_trim(pb, count).status[0]) if pb.n else 0


def partition(lines, corpus, count=False, moved=False):
    """(good, failing): every line of ``lines`` in one of the two, failing as [(line, status)].  The failing names are the fixed
    lists above (moved: those of the good lines' variants on a primer); the oracle must agree on every line."""
    want = dict(ON_PRIMER_FAILING[corpus] if moved else FAILING[corpus])
    if count:
        want.update(FAILING_COUNTED[corpus])
    good, failing, seen = [], [], set()
    for l in lines:
        st = line_status(l, count)
        assert st == want.get(line_name(l), 0), (line_name(l), st)
        if st:
            failing.append((l, st)); seen.add(line_name(l))
        else:
            good.append(l)
    assert seen == set(want) and len(good) + len(failing) == len(lines)
    return good, failing


# rows of corner_recs() with a status: l_seq 0 under a CIGAR, no qualities with trimming on (6); a read that ends behind the
# reference (1)
RECS_FAILING = dict([("c0", 6)] + [("c%d" % k, 6) for k in range(1, 26, 2)] + [("c62", 1), ("c70", 1)])
# moved onto a primer, two good rows fail: op B under a trim (8) -- 'opB' of hand_written_lines(), and the record with every op code
ON_PRIMER_FAILING = {"hand": {"opB": 8}, "corner": {}, "length": {}}
ON_PRIMER_RECS_FAILING = {"c69": 8}


def rec_status(r):
    from amplipy_amd.batch import ReadBatch
    if (r.flag & 4) or r.cigar is None:
        return 0
    return int(oracle_trim(ReadBatch.from_segments([r.to_segment()])).status[0])


def partition_recs(recs, want=None):
    """(good, failing) of Recs, failing as [(rec, status)]; ``want``: name -> status the oracle must agree with (None: whatever
    the oracle says, for variants of records already sorted)."""
    good, failing = [], []
    for r in recs:
        st = rec_status(r)
        assert want is None or st == want.get(r.qname, 0), (r.qname, st)
        if st:
            failing.append((r, st))
        else:
            good.append(r)
    assert want is None or {r.qname for r, _ in failing} == set(want)
    return good, failing


# ---- variants on a primer ---------------------------------------------------------------------------------------------------------------
def left_primers():
    """PRIMERS[0] and the next two left primers that give three residues of POS mod 8."""
    out = []
    for s, e, name in PRIMERS:
        if name.endswith("LEFT") and s % 8 not in {p[0] % 8 for p in out}:
            out.append((s, e))
        if len(out) == 3:
            break
    assert out[0] == PRIMERS[0][:2] and len(out) == 3
    return out


def _is_row(f):
    return len(f) >= 11 and f[2] == U.REF_NAME.encode() and f[5] != b"*" and f[1].isdigit() and not int(f[1]) & 4


def on_primer(lines):
    """The lines that are rows with POS rewritten to the first base of a left primer (the three of left_primers() in turn); a
    SEQ of plain ACGT is taken from the genome at that place.  Lines that are no rows are left out."""
    out, prim = [], left_primers()
    for l in lines:
        f = l[:-1].split(b"\t")
        if not _is_row(f):
            continue
        s = prim[len(out) % 3][0]
        f[3] = b"%d" % (s + 1)
        if set(f[9]) <= set(b"ACGT"):
            f[9] = GSTR[s:s + len(f[9])].encode()
        out.append(b"\t".join(f) + b"\n")
    return out


def on_primer_recs(recs):
    out, prim = [], left_primers()
    for r in recs:
        if (r.flag & 4) or r.cigar is None:
            continue
        s = prim[len(out) % 3][0]
        seq = None if r.seq is None else GSTR[s:s + len(r.seq)]
        out.append(bamio.Rec(r.qname, r.flag, r.ref_id, s, r.mapq, r.cigar, r.next_ref_id, r.next_pos, r.tlen, seq, r.qual, aux_bam=r.aux_bam,
                             aux_sam=r.aux_sam))
    return out


def crafted_on_primer():
    """Reads written for a primer.  On PRIMERS[0] (30 to 57): 60M -> 28S32M; 5M2I53M -> 30S30M; a low-quality second half ->
    28S1M31S; 27M -> 27S and sixty '#' -> 60S (no reference-consuming op: the `rlen ? rlen : 1` branch of reg2bin); a
    reverse-strand read, untouched; low-quality tails of 1, 10 and 25 bases (a third op); a deletion and an insertion inside the
    primer; a leading soft and hard clip; 1M; a read over the whole first amplicon (both primers clipped); and one on
    SYN_3_RIGHT (992 to 1019), the scheme's only primer whose clipped POS + 1 (1020) has more digits than the read's (993)."""
    s = PRIMERS[0][0]
    a0, a1 = int(AMPS[0][0]), int(AMPS[0][1])
    d = [p for p in PRIMERS if len(str(p[0] + 1)) != len(str(p[1] + 1))]
    assert a0 == s and len(d) == 1
    g = lambda name, cigar, n, at=s, **kw: ST.good_line(name, pos=at + 1, cigar=cigar, seq=GSTR[at:at + n], **kw)        # noqa: E731
    out = [g("p60M", "60M", 60), g("p_ins", "5M2I53M", 60), g("p_half_low", "60M", 60, qual="I" * 30 + "#" * 30), g("p27M", "27M", 27),
           g("p_all_low", "60M", 60, qual="#" * 60), g("p_reverse", "60M", 60, flag=147), g("p_tail1", "60M", 60, qual="I" * 59 + "#"),
           g("p_tail10", "60M", 60, qual="I" * 50 + "#" * 10), g("p_tail25", "80M", 80, qual="I" * 55 + "#" * 25),
           g("p_del", "20M5D40M", 60), g("p_ins_in", "10M3I47M", 60), g("p_soft", "10S50M", 60), g("p_hard", "5H60M", 60),
           g("p1M", "1M", 1), g("p_amplicon", "%dM" % (a1 - a0), a1 - a0), g("p_digits", "60M", 60, at=d[0][0])]
    return out


def primer_effects(lines):
    """What the oracle makes of ``lines`` as one batch: asserts that among the accepted rows one grows by at least 2 ops, one
    shrinks, one has no reference-consuming op, one keeps its POS and one changes the number of digits of its POS field -- so a
    later change to the scheme cannot empty the tests.  Returns (batch, results)."""
    recs, _ = U.python_records(b"".join(lines), HDR)
    pb = U.python_batch(recs)
    t = oracle_trim(pb)
    ok = t.status == 0
    old = np.diff(pb.cig_off.astype(np.int64))
    new = t.new_ncig.astype(np.int64)
    cigs = U.result_cigars(pb, t)
    assert (ok & (new >= old + 2)).any() and (ok & (new < old)).any()
    assert any(ok[i] and cigs[i] and not any(op in (0, 2, 3, 7, 8) for op, _ in cigs[i]) for i in range(pb.n))
    assert (ok & (t.new_pos == pb.pos)).any() and (ok & (t.new_pos != pb.pos)).any()
    assert any(ok[i] and len(str(int(t.new_pos[i]) + 1)) != len(str(int(pb.pos[i]) + 1)) for i in range(pb.n))
    return pb, t


# ---- lengths the wide copies turn on ------------------------------------------------------------------------------------------------------
QNAME_LENGTHS = tuple(range(1, 17)) + tuple(range(505, 521))
BASE_LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000)


def _bases_line(name, n, pos, **kw):
    if n == 0:
        return ST.good_line(name, pos=pos + 1, cigar="1M", seq="*", qual="*", **kw)
    return ST.good_line(name, pos=pos + 1, cigar="%dM" % n, seq=GSTR[pos:pos + n], qual=("!#5?I~+,IIIIIIIIII" * (n // 18 + 1))[:n], **kw)


def crlf_line(n, pos, tail=b"\r\n"):
    """A line of n bases that ends in CRLF, QNAME padded so that -- the line a chunk of its own -- the LF is the first byte of a
    16-byte scan slot and the CR the last of the slot before."""
    name = "crlf%d_" % n
    while len(_bases_line(name, n, pos)[:-1] + tail) % 16 != 1:
        name += "x"
    return _bases_line(name, n, pos)[:-1] + tail


def length_lines(pos=100):
    """Text-mode lines (QNAME is not limited there): QNAME of 1 to 16 and 505 to 520 bytes -- the first unchanged piece of
    lane_fmt_copy at every residue mod 8 and across one 512-byte step of wave_copy; reads of BASE_LENGTHS bases, with aux and as
    the line's last field; one CRLF line per length with the LF on a slot's first byte.  'bases0' (SEQ '*' under 1M) fails with
    status 6, its twin without a CIGAR is no row."""
    out = [ST.good_line(("q" * 520)[:n], pos=pos + 1, seq=GSTR[pos:pos + 20]) for n in QNAME_LENGTHS]
    for n in BASE_LENGTHS:
        out.append(_bases_line("bases%d" % n, n, pos))
        out.append(_bases_line("bases%d_noaux" % n, n, pos, aux=()) if n else ST.good_line("bases0_nocigar", pos=pos + 1, cigar="*", seq="*", qual="*"))
        if n:
            out.append(crlf_line(n, pos))
    return out


def length_odd_lines(pos=100):
    """The same CR on a slot's last byte with something else behind it: odd, BYTE."""
    return [(crlf_line(n, pos, tail=b"\rX\n"), "BYTE") for n in BASE_LENGTHS if n]


# ---- the corpora, sorted once --------------------------------------------------------------------------------------------------------------
_CORPORA = {}


def _once(f):
    def g():
        if f.__name__ not in _CORPORA:
            _CORPORA[f.__name__] = f()
        return _CORPORA[f.__name__]
    return g


@_once
def text_corpus():
    """Text mode: {"hand", "length", "moved": good lines; "failing": [(line, status)] of all of them}.  moved = the good lines of
    hand_written_lines() on a primer, length_lines() on PRIMERS[0] and crafted_on_primer(), with the effects asserted."""
    hand, f1 = partition(ST.hand_written_lines(), "hand")
    length, f2 = partition(length_lines(), "length")
    moved, f3 = partition(on_primer(hand), "hand", moved=True)
    moved_length, f4 = partition(length_lines(PRIMERS[0][0]), "length")
    moved = moved + moved_length + crafted_on_primer()
    primer_effects(moved)
    return {"hand": hand, "length": length, "moved": moved, "failing": f1 + f2 + f3 + f4}


@_once
def bam_corpus():
    """BAM mode: the same of corner_lines() (no length lines: QNAME is limited here)."""
    corner, f1 = partition(SB.corner_lines(), "corner")
    moved, f2 = partition(on_primer(corner), "corner", moved=True)
    moved = moved + crafted_on_primer()
    primer_effects(moved)
    return {"corner": corner, "moved": moved, "failing": f1 + f2}


@_once
def counted_failing():
    """The rows that fail with counting on only: {"hand" / "corner": (good lines with counting on, [(line, status)])}."""
    out = {}
    for corpus, lines in (("hand", ST.hand_written_lines()), ("corner", SB.corner_lines())):
        good, failing = partition(lines, corpus, count=True)
        out[corpus] = good, [(l, st) for l, st in failing if line_name(l) in FAILING_COUNTED[corpus]]
    return out


@_once
def recs_corpus():
    """The BAM side: {"corner": good records of corner_recs() (records that are no rows among them); "moved": their rows on a
    primer and crafted_on_primer() as records; "failing": [(rec, status)]}."""
    corner, f1 = partition_recs(BT.corner_recs(), RECS_FAILING)
    moved, f2 = partition_recs(on_primer_recs(corner), ON_PRIMER_RECS_FAILING)
    crafted = U.python_records(b"".join(crafted_on_primer()), HDR)[0]
    return {"corner": corner, "moved": moved + crafted, "failing": f1 + f2}


def amid(good, line, n=10):
    """``line`` (or record) in the middle of the first n of ``good`` that are rows: (lines, its row)."""
    good = [x for x in good if (_is_row(x[:-1].split(b"\t")) if isinstance(x, bytes) else not (x.flag & 4) and x.cigar is not None)]
    return good[:n // 2] + [line] + good[n // 2:n], n // 2


# ---- the check functions ------------------------------------------------------------------------------------------------------------------
# give_results(codec, results, verdict, read_base): hands the codec the results of the rows it holds -- a twin takes ``results``
# (the oracle's, laid out for those rows) and ``verdict``, the device runs its own read pass -- and returns the codec's
# (first bad row, status), or None when that comes down later (the deferred process).
def _sam_chunk(codec, chunk, count):
    """Parse on both sides, compared: (recs, python batch, the oracle's results or None without rows)."""
    recs, n_lines = U.python_records(chunk, HDR)
    pb = U.python_batch(recs)
    info = codec.parse(chunk)
    assert info.first_odd_line == -1, (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason], chunk[:200])
    got = (info.n_lines, info.n_records, info.n_rows, info.n_cig, info.n_bases, info.n_bases_padded)
    assert got == (n_lines, len(recs), pb.n, pb.cig.size, int(pb.lseq.sum()), int(pb.seq_off[-1])), chunk[:200]
    assert U.same_batch(codec.batch(), pb) == "", chunk[:200]                       # the Python packer's batch, pads included
    return recs, pb, (oracle_trim(pb, count) if pb.n else None)


def check_sam_text(codec, give_results, lines, min_length, include_no_primer, chunk_bytes=1 << 30, count=False):
    """SAM text in and out (section 10).  Every chunk of ``lines``: the batch and the counters equal the Python packer's, the
    verdict equals the oracle's, the text equals AlignmentWriter.write of the kept rows with the oracle's results; the walk ends
    behind the chunk of a failing row.  Returns (text, (first bad row of the last chunk, status))."""
    out, bad = [], (-1, 0)
    for chunk in SB.cut(lines, chunk_bytes):
        recs, pb, t = _sam_chunk(codec, chunk, count)
        if t is None:
            continue
        bad = first_status(t)
        assert give_results(codec, t, bad, 0) == bad, chunk[:200]
        keep = U.keep_rule(t, min_length, include_no_primer)
        text, n_rows = codec.format(min_length, include_no_primer)
        assert n_rows == int(keep.sum())
        assert text == U.python_text(recs, pb, HDR, t.new_pos, U.result_cigars(pb, t), keep), chunk[:200]
        out.append(text)
        if bad[0] >= 0:
            break
    return b"".join(out), bad


def check_sam_bam(codec, give_results, lines, min_length, include_no_primer, chunk_bytes=1 << 30, count=False, final_with_last=False):
    """SAM text in, BAM out (section 13), the stream carried across the chunks of ``lines`` and flushed at the end: parse as in
    check_sam_text; the record stream equals python_stream of the kept rows with the oracle's results, the framed blocks inflate
    to it; one wait and no host block per encode; the verdict (which a deferred process brings down with the encode) equals
    the oracle's.  A failing row ends the walk; the flush behind it empties the codec for the next caller.
    Returns (stream, verdict)."""
    stream, framed, want, bad = [], [], [], (-1, 0)
    chunks = SB.cut(lines, chunk_bytes)
    flushed = False

    def took(blocks, oi, n_rows):
        assert oi.waits == 1 and oi.n_blocks_host == 0 and oi.n_rows_written == n_rows
        assert not codec.is_twin or codec.guards_ok()
        if oi.stream_bytes > oi.carry_in:
            stream.append(codec.stream(int(oi.carry_in)).tobytes())
        framed.append(blocks.tobytes())
    for k, chunk in enumerate(chunks):
        recs, pb, t = _sam_chunk(codec, chunk, count)
        if t is None:
            continue
        bad = first_status(t)
        early = give_results(codec, t, bad, 0)
        assert early is None or early == bad
        keep = U.keep_rule(t, min_length, include_no_primer)
        flushed = final_with_last and k + 1 == len(chunks) and bad[0] < 0
        took(*codec.encode(min_length, include_no_primer, final=flushed), int(keep.sum()))
        assert codec.verdict() == bad, chunk[:200]
        want.append(SB.python_stream(recs, pb, t.new_pos, U.result_cigars(pb, t), keep))
        if bad[0] >= 0:
            break
    if not flushed:
        took(*codec.encode_bytes(b"", final=True), 0)
    stream, want = b"".join(stream), b"".join(want)
    assert stream == want
    SB.check_blocks(b"".join(framed), want)
    return stream, bad


def _bam_file(path):
    """The Python codec's view of a BAM file: (its rows as Recs, the host decoder's batch, records, the oracle's results)."""
    f = bam_native.BamFile(path)
    n_records = f.n_records
    want, _ = f.decode(0, n_records, copy=True)
    f.close()
    rows = BT.python_rows(path)
    assert want.n == len(rows)
    t = oracle_trim(want)
    return rows, want, n_records, BB.Results.of_trim(want, t), first_status(t)


class _Rows:
    """The layout of rows [lo, hi) of a batch as a batch of their own: what Results.rows needs."""

    def __init__(self, batch, lo, hi):
        self.n = hi - lo
        self.cig_off = batch.cig_off[lo:hi + 1] - batch.cig_off[lo]


def _bam_walk(codec, give_results, path, piece_bytes, want, n_records, res, bad, text):
    """The pieces of the file fed to the codec; per piece with rows the text check (``text``) and the results; yields (info, row of
    the piece that fails or -1)."""
    lo, tot = 0, np.zeros(4, np.int64)
    src = bam_device.DeviceBamInput(path, piece_bytes)
    for info, _ in bam_device.walk(codec, src):
        tot += (info.n_records, info.n_rows, info.n_cig, info.n_bases)
        if text:
            ti = codec.text_check()
            assert ti.first_odd_row == -1 and ti.waits == (1 if info.n_rows else 0), (ti.first_odd_row, bam_device.ODD_REASONS[ti.odd_reason])
        if not info.n_rows:
            continue
        hi = lo + int(info.n_rows)
        local = (bad[0] - lo, bad[1]) if lo <= bad[0] < hi else (-1, 0)
        assert give_results(codec, res.rows(_Rows(want, lo, hi), lo, hi), local, lo) == local
        lo = hi
        yield info, local[0]
        if local[0] >= 0:
            return
    assert tuple(tot) == (n_records, want.n, want.cig.size, int(want.lseq.sum())) and lo == want.n


def check_bam_text(codec, give_results, path, piece_bytes, min_length, include_no_primer):
    """BAM in, SAM text out (section 14): no odd row; the counters of the pieces add up to the host decoder's; the verdict equals
    the oracle's; the text of all pieces equals AlignmentWriter.write of the kept rows with the oracle's results.
    Returns (text, verdict)."""
    rows, want, n_records, res, bad = _bam_file(path)
    keep = BB._keep(res, min_length, include_no_primer, bad[0])
    parts, n_rows = [], 0
    for info, local_bad in _bam_walk(codec, give_results, path, piece_bytes, want, n_records, res, bad, True):
        t, fi = codec.format(min_length, include_no_primer)
        assert fi.n_bytes == len(t) and t.count(b"\n") == fi.n_rows_written
        parts.append(t); n_rows += int(fi.n_rows_written)
    got, expect = b"".join(parts), BT.python_text(rows, res, keep, BAM_HDR)
    assert got == expect, BT.first_difference(got, expect)
    assert n_rows == int(keep.sum())
    return got, bad


def check_bam_bam(codec, give_results, path, piece_bytes, min_length, include_no_primer, host_path):
    """BAM in, BAM out (section 12): the record stream of all encodes equals the payload of the file BamWriter.write_rows writes
    (``host_path``) from the oracle's results, the framed blocks inflate to it, one wait and no host block per encode.
    Returns (payload, verdict)."""
    rows, want, n_records, res, bad = _bam_file(path)
    payload = BB.host_file(host_path, path, res, min_length, include_no_primer, bad[0])
    stream, framed, n_rows = [], [], 0

    def took(blocks, oi):
        assert oi.waits == 1 and oi.n_blocks_host == 0
        assert not codec.is_twin or codec.guards_ok()
        if oi.stream_bytes > oi.carry_in:
            stream.append(codec.stream(int(oi.carry_in)).tobytes())
        framed.append(blocks.tobytes())
        return int(oi.n_rows_written)
    for info, local_bad in _bam_walk(codec, give_results, path, piece_bytes, want, n_records, res, bad, False):
        n_rows += took(*codec.encode(min_length, include_no_primer))
    assert took(*codec.encode(min_length, include_no_primer, final=True)) == 0       # the bare flush
    assert b"".join(stream) == payload
    assert n_rows == int(BB._keep(res, min_length, include_no_primer, bad[0]).sum())
    SB.check_blocks(b"".join(framed), payload)
    return payload, bad


def assert_floats_packed(stream, vals):
    """Record k of the stream of float_lines(vals) ends with spelling k as an f field and twice in a B:f array, each
    struct.pack("<f", float(v)): the codec's fp64 multiply, divide and narrowing cast against CPython's."""
    import struct
    at = 0
    for v in vals:
        (size,) = struct.unpack_from("<i", stream, at)
        at += 4 + size
        p = struct.pack("<f", float(v))
        assert stream[at - 23:at] == b"XFf" + p + b"BFBf" + struct.pack("<I", 2) + p + p, v
    assert at == len(stream)


# ---- odd means odd --------------------------------------------------------------------------------------------------------------------------
def check_odd_lines(codec, entries, seeded):
    """Each (line, reason) once in the middle of ``seeded``: the codec names the line and the reason."""
    where = len(seeded) // 2
    for l, reason in entries:
        info = codec.parse(b"".join(seeded[:where]) + l + b"".join(seeded[where:]))
        assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (where, reason), l[-80:]


def check_first_odd_wins(codec, entries, good):
    """All the odd lines in one chunk behind ``good``, in their order and reversed -- lanes of different kernels report at once,
    one atomic min decides: the first line and its reason."""
    for es in (entries, entries[::-1]):
        info = codec.parse(b"".join(good) + b"".join(l for l, _ in es))
        assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (len(good), es[0][1]), es[0][0][-80:]


def check_odd_records(codec, path, place, reason):
    """A file of one piece whose row ``place`` is odd: text_check names the row and the reason, format answers AMP_ESTATE."""
    import pytest
    from amplipy_amd import lib
    (info, _), = list(bam_device.walk(codec, bam_device.DeviceBamInput(path, 1 << 30)))
    ti = codec.text_check()
    assert (int(ti.first_odd_row), bam_device.ODD_REASONS[ti.odd_reason]) == (place, reason)
    with pytest.raises(lib.AmpliHipError) as e:
        codec.format(30, True)
    assert e.value.rc == BT.ESTATE


# ---- the tests' bodies: the twin module and the GPU module differ in the codec and in how it gets its results --------------------------
def shuffled(lines, seed):
    rng = np.random.default_rng(seed)
    return [lines[i] for i in rng.permutation(len(lines))]


def sam_text_good(codec, give):
    """The good lines of hand_written_lines(), the length lines and everything on a primer, shuffled once: as one chunk, cut at
    4 KB, every line as a chunk of its own and as the first and the last of three; min_length 0, 1 and 30, include_no_primer both
    ways."""
    codec.set_output(sam_native.OUT_TEXT)
    t = text_corpus()
    lines = shuffled(t["hand"] + t["length"] + t["moved"], 1)
    whole, _ = check_sam_text(codec, give, lines, 0, True)
    assert whole.count(b"\n") == U.python_batch(U.python_records(b"".join(lines), HDR)[0]).n > 200       # every row: none has a status
    assert check_sam_text(codec, give, lines, 1, True, chunk_bytes=4096)[0].count(b"\n") <= whole.count(b"\n")
    some, _ = check_sam_text(codec, give, lines, 30, False)
    assert 0 < some.count(b"\n") < whole.count(b"\n")
    for l in lines:
        check_sam_text(codec, give, [l], 0, True)
        check_sam_text(codec, give, [l, lines[0], lines[1]], 1, False)
        check_sam_text(codec, give, [lines[0], lines[1], l], 0, True)


def sam_bam_good(codec, give):
    """The good lines of corner_lines() and everything on a primer in BAM mode: whole, cut at 4 KB with the last encode the final
    one, and a line per chunk with the stream carried across the chunks and a final flush."""
    codec.set_output(sam_native.OUT_BAM)
    b = bam_corpus()
    lines = shuffled(b["corner"] + b["moved"], 2)
    whole, _ = check_sam_bam(codec, give, lines, 0, True)
    check_sam_bam(codec, give, lines, 1, True, chunk_bytes=4096, final_with_last=True)
    some, _ = check_sam_bam(codec, give, lines, 30, False)
    assert 0 < len(some) < len(whole)
    assert check_sam_bam(codec, give, lines, 0, True, chunk_bytes=1)[0] == whole


def write_small_blocks(path, recs, block_bytes=3001):
    """write_raw with BGZF blocks of ``block_bytes``: a corner file is a dozen blocks then, records span two and three of them
    (a piece of one block then ends inside a record, or holds none), and the header has no block of its own."""
    w = bamio.AlignmentWriter(path, "wb", BAM_HDR)
    bz = w._w

    def write(b):
        bz.buf += b
        while len(bz.buf) >= block_bytes:
            bz._flush_block(bytes(bz.buf[:block_bytes])); del bz.buf[:block_bytes]
    bz.write = write
    for r in recs:
        w.write(r)
    w.close()
    return path


def bam_corners(codec, give, tmp_path):
    """The good records of corner_recs() and their rows on a primer, written through the Python codec in blocks of 3,001 bytes:
    pieces of one block and of the whole file, as text and as BAM."""
    r = recs_corpus()
    host = str(tmp_path / "host.bam")
    for tag, recs in (("corner", r["corner"]), ("moved", r["moved"])):
        path = write_small_blocks(str(tmp_path / (tag + ".bam")), recs)
        assert len(bam_device.DeviceBamInput(path, 1).pieces) >= 10
        for piece in (1, 1 << 30):
            whole, bad = check_bam_text(codec, give, path, piece, 0, True)
            assert bad == (-1, 0) and whole.count(b"\n") == sum(1 for x in recs if not (x.flag & 4) and x.cigar is not None)
            check_bam_bam(codec, give, path, piece, 0, True, host)
        some, _ = check_bam_text(codec, give, path, 1 << 30, 30, False)
        assert (0 < some.count(b"\n") < whole.count(b"\n")) if tag == "moved" else some == b""          # (no corner record lies on a primer)
        check_bam_bam(codec, give, path, 1, 30, False, host)


def rows_with_a_status(sam, bam, give, give_bam_out, give_bam, tmp_path):
    """Each failing line or record in the middle of ten good ones: the codec's verdict is the oracle's (asserted by the check
    functions) and names that row; the output holds exactly the rows in front of it."""
    t, b, r = text_corpus(), bam_corpus(), recs_corpus()
    sam.set_output(sam_native.OUT_TEXT)
    for l, st in t["failing"]:
        lines, place = amid(t["hand"], l)
        text, bad = check_sam_text(sam, give, lines, 0, True)
        assert bad == (place, st) and text.count(b"\n") == place
    sam.set_output(sam_native.OUT_BAM)
    for l, st in b["failing"]:
        lines, place = amid(b["corner"], l)
        assert check_sam_bam(sam, give_bam_out, lines, 0, True)[1] == (place, st)
    host = str(tmp_path / "host.bam")
    for k, (rec, st) in enumerate(r["failing"]):
        recs, place = amid(r["corner"], rec)
        path = BT.write_raw(str(tmp_path / ("bad%d.bam" % k)), recs)
        text, bad = check_bam_text(bam, give_bam, path, 1 << 30, 0, True)
        assert bad == (place, st) and text.count(b"\n") == place
        assert check_bam_bam(bam, give_bam, path, 1 << 30, 0, True, host)[1] == (place, st)


def rows_with_a_counting_status(sam, give, give_bam_out):
    """The same for the three statuses only counting gives (the caller has switched counting on)."""
    c = counted_failing()
    sam.set_output(sam_native.OUT_TEXT)
    for l, st in c["hand"][1]:
        lines, place = amid(c["hand"][0], l)
        assert check_sam_text(sam, give, lines, 0, True, count=True)[1] == (place, st)
    sam.set_output(sam_native.OUT_BAM)
    for l, st in c["corner"][1]:
        lines, place = amid(c["corner"][0], l)
        assert check_sam_bam(sam, give_bam_out, lines, 0, True, count=True)[1] == (place, st)
    assert {st for _, st in c["hand"][1]} == {2, 3, 4}


def odd_lines_text(codec):
    """Text mode: every entry of test_sam_text.odd_lines() and the CR in front of another byte; the reasons of BAM output are not
    odd here; of two odd lines the first wins; 5,000 newlines are more lines than the tables hold."""
    codec.set_output(sam_native.OUT_TEXT)
    seeded = ST.seeded_lines(31, 6, 3, 1)
    check_odd_lines(codec, ST.odd_lines() + length_odd_lines(), seeded)
    for l, _ in SB.odd_lines():
        assert codec.parse(b"".join(seeded[:3]) + l + b"".join(seeded[3:])).first_odd_line == -1, l[-80:]
    info = codec.parse(seeded[0] + seeded[1] + ST.good_line(cigar="10M5") + seeded[2] + ST.good_line(flag="099"))
    assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (2, "CIGAR")
    check_first_odd_wins(codec, ST.odd_lines(), seeded[:4])
    info = codec.parse(b"\n" * 5000)
    assert info.n_lines == 5000 and info.first_odd_line == 5000 // 64 + 1024 and sam_native.ODD_REASONS[info.odd_reason] == "LINES"


def odd_lines_bam_out(codec):
    """BAM mode: every entry of test_sam_to_bam_twin.odd_lines(), the 65,534-op line first (the arena grows once, every later chunk
    reuses it); two odd lines: the first wins; a fault in the core fields goes before one in the aux fields of the same line."""
    codec.set_output(sam_native.OUT_BAM)
    seeded = SB.seeded_lines(31, 6, 3, 1)
    entries = SB.odd_lines()
    entries.sort(key=lambda e: e[1] != "CIGAR_OPS")
    assert entries[0][1] == "CIGAR_OPS"
    check_odd_lines(codec, entries, seeded)
    info = codec.parse(seeded[0] + SB.line(aux=("XF:f:inf",)) + seeded[1] + SB.line(aux=("XA:A:",)))
    assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (1, "AUX_FLOAT")
    info = codec.parse(SB.line(flag="099", aux=("XF:f:inf",)))
    assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (0, "INT")
    check_first_odd_wins(codec, entries[1:], seeded[:4])                            # (without the 65,534-op line)
    blocks, oi = codec.encode(0, True, final=True)                                  # an odd chunk is not encoded
    assert oi.n_rows_written == 0


def odd_records(codec, tmp_path):
    """Every variant of ODD of test_bam_to_sam_twin at place 4 of 9, and the eleven out-of-set float patterns."""
    good = [BT.raw_record(name=b"g%d\0" % k, aux=b"NMC\1XSZok\0") for k in range(9)]
    variants = [(reason, v) for reason, vs in BT.ODD.items() for v in vs]
    variants += [("AUX_FLOAT", BT.raw_record(aux=aux)) for b in BT.OUT_OF_SET_BITS for aux in BT.out_of_set_aux(b)]
    assert len(variants) == sum(len(v) for v in BT.ODD.values()) + 22
    for k, (reason, v) in enumerate(variants):
        path = BT.write_raw(str(tmp_path / ("odd%d.bam" % k)), good[:4] + [v] + good[5:])
        check_odd_records(codec, path, 4, reason)


def floats(sam, bam, give_bam_out, give_bam, tmp_path):
    """Text to binary: float_spellings(3000, 5) as f fields and in B:f arrays, the bytes struct.pack("<f", float(v)).  Binary to
    text: float_patterns(100000, 7) in about fifty records, the text '%g'."""
    sam.set_output(sam_native.OUT_BAM)
    vals = SB.float_spellings(3000, 5)
    stream, _ = check_sam_bam(sam, give_bam_out, SB.float_lines(vals), 0, True)
    assert_floats_packed(stream, vals)
    bits = BT.float_patterns(100000, 7)
    path = BT.write_raw(str(tmp_path / "floats.bam"), BT.float_carrier_recs(bits))
    text, _ = check_bam_text(bam, give_bam, path, 1 << 30, 0, True)
    assert BT.percent_g_of_arrays(text) == ",".join("%g" % float(v) for v in bits.view(np.float32)).encode()


def one_codec_many_shapes(codec, give, give_bam_out):
    """Text, BAM and text again on one codec: the first chunk's text comes out as the first time; an empty chunk and an odd one
    between two good ones leave the good ones' output what the Python codec writes."""
    t, b = text_corpus(), bam_corpus()
    codec.set_output(sam_native.OUT_TEXT)
    first, _ = check_sam_text(codec, give, t["hand"], 0, True)
    codec.set_output(sam_native.OUT_BAM)
    check_sam_bam(codec, give_bam_out, b["moved"], 0, True)
    codec.set_output(sam_native.OUT_TEXT)
    assert check_sam_text(codec, give, t["hand"], 0, True)[0] == first
    info = codec.parse(b"")
    assert (info.n_lines, info.n_rows, info.first_odd_line) == (0, 0, -1)
    assert codec.parse(t["hand"][0] + ST.good_line(flag="099")).first_odd_line == 1
    check_sam_text(codec, give, t["moved"], 0, True)
    assert check_sam_text(codec, give, t["hand"], 0, True)[0] == first
