"""The device codec for SAM text (amplipy_amd/csrc/amp_sam.hip) checked on the CPU: its lane functions compiled for the host
(-DAMPSAM_HOSTSIM, the twin) against the Python codec of bamio -- AlignmentReader.records_of into ReadBatch.from_segments for the
batch, AlignmentWriter.write for the text."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from amplipy_amd import sam_native, synth
from amplipy_amd.sam_native import AmpSamInfo, SamCodec
from tests import sam_util as U

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the twin")

G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = U.header(G.size)
ODD = {v: k for k, v in sam_native.ODD_REASONS.items()}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    c = SamCodec(twin=U.twin_path(tmp_path_factory.mktemp("twin")))
    c.set_references(U.ref_names(HDR))
    yield c
    c.close()


def L(*f):
    return ("\t".join(str(x) for x in f)).encode("ascii") + b"\n"


def good_line(name="g", flag=99, pos=100, cigar="20M", seq="ACGTACGTACGTACGTACGT", qual=None, rname=U.REF_NAME, rnext="=", mapq=60,
              pnext=300, tlen=220, aux=("NM:i:0",)):
    return L(name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, "I" * len(seq) if qual is None else qual, *aux)


def hand_written_lines():
    out = [good_line("clips", cigar="5H10S30M10S5H", seq="ACGTT" * 10),
           good_line("opB", cigar="10M2B10M"), good_line("opN", cigar="10M100N10M"), good_line("opP", cigar="5M1P5M10M"),
           good_line("opEQX", cigar="10=1X9="),
           good_line("long", cigar="1M1I" * 110, seq="AC" * 110),
           good_line("qstar", qual="*"), good_line("sstar", seq="*", qual="*"),
           good_line("unmapped", flag=4), good_line("unmapped_star", flag=77, cigar="*", rname="*", pos=0, rnext="*", pnext=0, tlen=0),
           good_line("nocigar", cigar="*"),
           good_line("iupac", cigar="17M", seq="acgtnRYKMSWBDHVN="), good_line("alien", cigar="8M", seq="ACGTXZ.-"),
           good_line("other", rname="OTHER", rnext="*", pnext=0), good_line("mate_elsewhere", rnext="OTHER"),
           good_line("negtlen", tlen=-2147483648, pos=2147483647, pnext=2147483647, flag=65535 & ~4, mapq=255),
           good_line("zeros", flag=0, pos=0, mapq=0, pnext=0, tlen=0, rnext="*"),
           good_line("one_qual_star_len1", cigar="1M", seq="A", qual="*"),
           b"three\tfields\tonly\n", L(*["ten"] * 10), b"\n", b"\n", b"@CO\tlooks like a header line\n"]
    for n in range(1, 26):
        out.append(good_line("len%d" % n, cigar="%dM" % n, seq=("GATTACAN" * 4)[:n], qual=("!#5?I~+," * 4)[:n]))
    for k in range(0, 21):
        out.append(good_line("aux%d" % k, aux=tuple(U.AUX_POOL[:k])))
    out += [l[:-1] + b"\r\n" for l in (good_line("crlf"), good_line("crlf_noaux", aux=()), b"short\tline\n", b"\n")]
    return out


def seeded_lines(seed, n_amp=300, n_mixed=200, n_many=100):
    rng = np.random.default_rng(seed)
    segs = synth.make_amplicon_batch(G, AMPS, n_amp, seed=seed).segments() + synth.make_mixed_segments(G, AMPS, n_mixed, seed + 1) \
        + U.many_op_segments(rng, n_many, G.size)
    return U.segments_to_lines(segs, HDR, rng, max_aux=5)


def check_batch(twin, chunk):
    """The twin's batch and counts against the Python codec's; returns (recs, python batch)."""
    info = twin.parse(chunk)
    recs, n_lines = U.python_records(chunk, HDR)
    pb = U.python_batch(recs)
    assert info.first_odd_line == -1, (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason])
    got = (info.n_lines, info.n_records, info.n_rows, info.n_cig, info.n_bases, info.n_bases_padded)
    assert got == (n_lines, len(recs), pb.n, pb.cig.size, int(pb.lseq.sum()), int(pb.seq_off[-1]))
    assert U.same_batch(twin.batch(), pb) == ""
    return recs, pb


# ---- 1. batch equality ---------------------------------------------------------------------------------------------------------------
def test_batch_equals_the_python_packer(twin):
    hand = hand_written_lines()
    rng = np.random.default_rng(7)
    seeded = seeded_lines(11)
    check_batch(twin, b"".join(hand))
    check_batch(twin, b"".join(seeded))
    mixed = hand + seeded
    for _ in range(5):
        order = rng.permutation(len(mixed))
        check_batch(twin, b"".join(mixed[i] for i in order))
    for line in hand:                       # every hand-written line as a chunk of its own, and as first / last line
        check_batch(twin, line)
        check_batch(twin, line + seeded[0])
        check_batch(twin, seeded[1] + line)
    recs, pb = check_batch(twin, b"".join(hand))
    assert pb.n > 60 and any(len(r.cigar or ()) > 200 for r in recs)
    # pads: a read's padding nibbles and quality bytes are zero (equality above covers them; spelled out once)
    tb = twin.batch()
    for i in range(tb.n):
        o, n = int(tb.seq_off[i]), int(tb.lseq[i])
        assert not tb.qual[o + n:int(tb.seq_off[i + 1])].any()


def test_parse_arguments(twin):
    info = twin.parse(b"")
    assert (info.n_lines, info.n_records, info.n_rows, info.first_odd_line) == (0, 0, 0, -1) and twin.batch().n == 0
    import ctypes as C
    raw = AmpSamInfo()
    text = good_line()
    assert twin.L.amp_sam_parse(twin.h, text[:-1], C.c_int64(len(text) - 1), C.byref(raw)) == -1          # last byte is not a newline
    assert twin.L.amp_sam_parse(twin.h, None, C.c_int64(5), C.byref(raw)) == -1
    assert twin.L.amp_sam_parse(None, text, C.c_int64(len(text)), C.byref(raw)) == -1
    assert twin.L.amp_sam_parse(twin.h, text, C.c_int64(-1), C.byref(raw)) == -1
    twin.parse(text)
    nb = C.c_int64(0)
    assert twin.L.amp_sam_format(twin.h, C.c_int32(30), C.c_int32(1), None, C.c_int64(0), C.byref(nb), None) == -1       # format before the results are there


# ---- 2. text equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [21, 22])
def test_text_equals_the_python_writer(twin, seed):
    from oracle import oracle
    pr = [(s, e) for s, e, _ in PRIMERS]
    mn, mx, mpl = oracle.find_overlapping_primers(G.size, pr, 0)
    rng = np.random.default_rng(seed)
    lines = seeded_lines(seed) + hand_written_lines()
    lines = [lines[i] for i in rng.permutation(len(lines))]
    chunk = b"".join(lines)
    recs, pb = check_batch(twin, chunk)
    res = oracle.process(pb, G.size, mn, mx, mpl, 20, 4).trim
    same = U.IdentityResult(pb)
    for i in np.nonzero(res.status)[0]:            # reads the oracle rejects (op B, a position off the reference): written unchanged here
        o = int(pb.cig_off[i]) + 3 * int(i)
        res.new_pos[i] = same.new_pos[i]; res.new_ncig[i] = same.new_ncig[i]
        res.new_cig[o:o + int(same.new_ncig[i])] = same.new_cig[o:o + int(same.new_ncig[i])]
    assert (res.status == 0).sum() > pb.n * 0.9 and (res.trim_flags & 3).any() and not (res.trim_flags & 3).all()
    cigs = U.result_cigars(pb, res)
    n_kept = set()
    for planted in (False, True):
        if planted:
            res.status[:] = 0
            res.status[pb.n // 2] = 6
        else:
            res.status[:] = 0
        bad, st = twin.twin_set_results(res)
        assert (bad, st) == ((pb.n // 2, 6) if planted else (-1, 0))
        for inp in (False, True):
            for min_length in (30, 140):
                keep = U.keep_rule(res, min_length, inp)
                text, n_rows = twin.format(min_length, inp)
                assert n_rows == int(keep.sum())
                assert text == U.python_text(recs, pb, HDR, res.new_pos, cigs, keep)
                n_kept.add(n_rows)
    assert len(n_kept) >= 4 and min(n_kept) > 0          # the settings keep different sets of rows


# ---- 3. odd means odd ------------------------------------------------------------------------------------------------------------------
def odd_lines():
    g = good_line
    return [
        (g("f099", flag="099"), "INT"), (g("plus", pos="+11"), "INT"), (g("sp", mapq=" 5"), "INT"), (g("minus0", tlen="-0"), "INT"),
        (g("hex", pnext="0x10"), "INT"), (g("emptyint", flag=""), "INT"), (g("under", tlen="1_0"), "INT"),
        (g("flag", flag=65536), "RANGE"), (g("negflag", flag=-1), "RANGE"), (g("pos", pos=2147483648), "RANGE"), (g("negpos", pos=-1), "RANGE"),
        (g("mapq", mapq=256), "RANGE"), (g("pnext", pnext=2147483648), "RANGE"), (g("tlen", tlen=2147483648), "RANGE"),
        (g("ntlen", tlen=-2147483649), "RANGE"), (g("huge", pos="123456789012345678901234567890"), "RANGE"),
        (g("rnext_spelled", rnext=U.REF_NAME), "RNEXT"), (g("rname_missing", rname="chrX"), "RNAME"),
        (g("eq_behind_star", rname="*", rnext="="), "RNEXT"), (g("rnext_missing", rnext="chrX"), "RNEXT"), (g("rname_empty", rname=""), "RNAME"),
        (g("cig1", cigar="10M5"), "CIGAR"), (g("cig2", cigar="M"), "CIGAR"), (g("cig3", cigar="10Q10M"), "CIGAR"), (g("cig4", cigar=""), "CIGAR"),
        (g("cig5", cigar="20M*"), "CIGAR"), (g("cig6", cigar="20m"), "CIGAR"),
        (g("ciglen", cigar="268435456M"), "CIGAR_LEN"), (g("cigzero", cigar="020M"), "CIGAR_LEN"),
        (g("qlen", qual="IIII"), "QUAL_LEN"), (g("qnoseq", seq="*", qual="IIII"), "QUAL_NO_SEQ"), (g("qchar", qual="IIII IIIIIIIIIIIIIII"), "QUAL_CHAR"),
        (g("seq_empty", seq="", qual="*"), "EMPTY"), (g("qual_empty", qual=""), "EMPTY"),
        (g("hi").replace(b"NM:i:0", b"CO:Z:\x80"), "BYTE"), (g("nul").replace(b"nul", b"n\0l"), "BYTE"), (g("cr").replace(b"NM", b"N\rM"), "BYTE"),
        (g("crcr")[:-1] + b"\r\r\n", "BYTE"), (b"short\xc3\xa9\n", "BYTE"),
    ]


def test_odd_lines_are_reported(twin):
    seeded = seeded_lines(31, 20, 10, 5)
    for line, reason in odd_lines():
        for where in (0, len(seeded) // 2, len(seeded)):
            chunk = b"".join(seeded[:where]) + line + b"".join(seeded[where:])
            info = twin.parse(chunk)
            assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (where, reason), line
    # two odd lines: the first one is reported
    info = twin.parse(seeded[0] + seeded[1] + good_line(cigar="10M5") + seeded[2] + good_line(flag="099"))
    assert (info.first_odd_line, info.odd_reason) == (2, ODD["CIGAR"])
    # more lines than the line tables hold
    info = twin.parse(b"\n" * 5000)
    assert info.n_lines == 5000 and info.first_odd_line == 5000 // 64 + 1024 and info.odd_reason == ODD["LINES"]


def test_the_python_codec_differs_or_raises_on_odd_lines():
    """Why those lines are odd: the Python codec does not give them back byte for byte (or raises)."""
    for line, reason in odd_lines():
        if reason in ("LINES",):
            continue
        try:
            recs, _ = U.python_records(line, HDR)
            pb = U.python_batch(recs)
            res = U.IdentityResult(pb)
            text = U.python_text(recs, pb, HDR, res.new_pos, U.result_cigars(pb, res), U.keep_rule(res, 1, True))
        except Exception:
            continue
        if reason in ("RANGE", "CIGAR_LEN", "QUAL_NO_SEQ", "EMPTY", "BYTE") and text == line:
            continue                          # (the device's rule is stricter than needed here: allowed)
        assert text != line, line


# ---- 4. never silently different ---------------------------------------------------------------------------------------------------------
FUZZ_CHUNKS = 20000
FUZZ_LINES = 12
FUZZ_BYTES = [9, 10, 13, ord("0"), ord("9"), ord("A"), ord("a"), ord("M"), ord("*"), ord("="), ord("+"), ord(" "), ord("!"), 0x80]
FUZZ_FIELDS = [b"099", b"+11", b"-0", b"*", b"=", b"", b"65536", b"2147483648", b"OTHER", U.REF_NAME.encode(), b"chrX", b"10M5", b"268435456M", b"0M",
               b"05M", b"4", b"0", b"-7", b"255", b"30M", b"1M1B1M"]


def fuzz_chunk(rng, pool):
    lines = [pool[int(i)] for i in rng.integers(0, len(pool), FUZZ_LINES)]
    kind = rng.random()
    if kind < 0.6:                              # one or two bytes replaced
        buf = bytearray(b"".join(lines))
        for _ in range(1 if kind < 0.4 else 2):
            buf[int(rng.integers(0, len(buf)))] = FUZZ_BYTES[int(rng.integers(0, len(FUZZ_BYTES)))]
        chunk = bytes(buf)
    elif kind < 0.85:                           # a field replaced, dropped or doubled
        k = int(rng.integers(0, FUZZ_LINES))
        f = lines[k][:-1].split(b"\t")
        j = int(rng.integers(0, len(f)))
        what = rng.random()
        if what < 0.7:
            f[j] = FUZZ_FIELDS[int(rng.integers(0, len(FUZZ_FIELDS)))]
        elif what < 0.85:
            del f[j]
        else:
            f.insert(j, f[j])
        lines[k] = b"\t".join(f) + b"\n"
        chunk = b"".join(lines)
    else:                                       # line ends
        k = int(rng.integers(0, FUZZ_LINES))
        end = [b"\r\n", b"\r", b"\r\r\n", b"\n\n", b"", b"\n\r\n"][int(rng.integers(0, 6))]
        lines[k] = lines[k][:-1] + end
        if rng.random() < 0.5:
            lines = [l[:-1] + b"\r\n" if l.endswith(b"\n") and not l.endswith(b"\r\n") else l for l in lines]
        chunk = b"".join(lines)
    return chunk if chunk.endswith(b"\n") else chunk + b"\n"          # (the reader completes a final line)


def read_twin_output(f):
    """One chunk's record of tests/hostsim/sam_twin_main.cpp: (info, batch or None, text or None)."""
    from amplipy_amd.batch import ReadBatch
    info = AmpSamInfo.from_buffer_copy(f.read(64))
    if info.first_odd_line >= 0:
        return info, None, None
    n, nc, nb = info.n_rows, info.n_cig, info.n_bases_padded

    def arr(dt, k):
        return np.frombuffer(f.read(np.dtype(dt).itemsize * k), dt)
    pos, flag, tlen, lseq = arr(np.int32, n), arr(np.uint16, n), arr(np.int32, n), arr(np.uint32, n)
    cig_off, cig, seq_off = arr(np.uint64, n + 1), arr(np.uint32, nc), arr(np.uint64, n + 1)
    seq, qual, src = arr(np.uint8, nb // 2), arr(np.uint8, nb), arr(np.int64, n)
    (tl,) = struct.unpack("<q", f.read(8))
    return info, ReadBatch(pos, flag, tlen, lseq, cig_off, cig, seq_off, seq, qual, src_index=src), f.read(tl)


def test_fuzzed_text_is_never_silently_different(tmp_path):
    """For every fuzzed chunk exactly one holds: the twin reports an odd line, or the Python codec gives the same batch and (with
    results that change nothing) the same text.  Where the Python codec raises the twin must have reported oddness.  The twin is
    a program built with -fsanitize=address,undefined and must finish clean."""
    assert ctypes_sizeof_info() == 64
    main = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "sam_twin_main.cpp")
    exe = U.twin_path(tmp_path, sanitize=True, main_source=main)
    rng = np.random.default_rng(2024)
    segs = synth.make_amplicon_batch(G, AMPS, 400, seed=5, read_len=60).segments() + U.many_op_segments(rng, 150, G.size, max_len=90, max_ops=8) \
        + synth.random_segments(rng, 150, G.size, [(s, e) for s, e, _ in PRIMERS], domain_errors=False, max_len=70)
    pool = U.segments_to_lines(segs, HDR, rng, max_aux=3) + hand_written_lines()
    chunks = [fuzz_chunk(rng, pool) for _ in range(FUZZ_CHUNKS)]
    with open(tmp_path / "in.bin", "wb") as f:
        for c in chunks:
            f.write(struct.pack("<q", len(c))); f.write(c)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + U.ref_names(HDR), capture_output=True, text=True)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    n_odd = n_raised = 0
    with open(tmp_path / "out.bin", "rb") as f:
        for k, chunk in enumerate(chunks):
            info, tb, text = read_twin_output(f)
            try:
                recs, n_lines = U.python_records(chunk, HDR)
                pb = U.python_batch(recs)
                res = U.IdentityResult(pb)
                want = U.python_text(recs, pb, HDR, res.new_pos, U.result_cigars(pb, res), np.ones(pb.n, bool))
            except Exception:
                n_raised += 1
                assert tb is None, "chunk %d: the Python codec raises, the twin saw nothing odd: %r" % (k, chunk)
                n_odd += 1
                continue
            if tb is None:
                n_odd += 1
                continue
            assert (info.n_lines, info.n_records) == (n_lines, len(recs)), (k, chunk)
            assert U.same_batch(tb, pb) == "", (k, U.same_batch(tb, pb), chunk)
            assert text == want, (k, chunk)
        assert f.read(1) == b""
    print("fuzz: %d chunks, %d odd (%.1f %%), the Python codec raised on %d" % (FUZZ_CHUNKS, n_odd, 100.0 * n_odd / FUZZ_CHUNKS, n_raised))
    assert FUZZ_CHUNKS - n_odd >= FUZZ_CHUNKS / 3


def ctypes_sizeof_info():
    import ctypes
    return ctypes.sizeof(AmpSamInfo)
