"""SAM text in, trimmed BAM out on the device codec (amp_sam_set_output / amp_sam_encode / amp_sam_encode_bytes of
amplipy_amd/csrc/amp_sam.hip) checked on the CPU: the lane functions compiled for the host (-DAMPSAM_HOSTSIM,
the twin) against the Python codec -- what bamio.AlignmentWriter(mode="wb").write(r, pos=, cigar=) appends for the Rec that
AlignmentReader.records_of makes of the line.  No GPU needed."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, bamio, sam_native, synth
from amplipy_amd.sam_native import SamCodec
from tests import sam_util as U
from tests.test_bam_reencode_twin import _zlib_deflater, deflater        # noqa: F401 (deflater: a fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the twin")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = U.header(G.size)
ODD = {v: k for k, v in sam_native.ODD_REASONS.items()}
BS = 0xFF00


def new_twin(path, deflate_fn, mode=sam_native.OUT_BAM):
    c = SamCodec(twin=path)
    c.set_references(U.ref_names(HDR))
    c.set_output(mode)
    if deflate_fn is not None:
        c.set_deflater(deflate_fn)
    return c


@pytest.fixture(scope="module")
def twin_so(tmp_path_factory):
    return U.twin_path(tmp_path_factory.mktemp("twin"))


@pytest.fixture(scope="module")
def twin(twin_so, deflater):        # noqa: F811
    c = new_twin(twin_so, deflater)
    yield c
    c.close()


# ---- the Python codec's bytes -------------------------------------------------------------------------------------------------------
class Capture:
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))


def python_stream(recs, batch, new_pos, cigars, keep):
    """What AlignmentWriter(mode="wb").write(r, pos=, cigar=) appends for the kept rows: the writer's own method, its BGZF layer
    replaced by a list."""
    w = bamio.AlignmentWriter.__new__(bamio.AlignmentWriter)
    w.mode, w.header, w._own, w._w = "wb", HDR, False, Capture()
    for k in range(batch.n):
        if keep[k]:
            w.write(recs[int(batch.src_index[k])], pos=int(new_pos[k]), cigar=cigars[k])
    return b"".join(w._w.parts)


class Res:
    """Results of the rows of a batch as amp_trim_out lays them out (row r's CIGAR words at cig_off[r] + 3 r)."""

    def __init__(self, batch, new_pos, words, ref_len, trim_flags, status):
        n = batch.n
        self.words = words
        self.new_pos = np.ascontiguousarray(new_pos, np.int32)
        self.new_ncig = np.array([len(w) for w in words], np.uint32)
        self.new_cig = np.zeros(batch.cig.size + 3 * n + 1, np.uint32)
        for r, w in enumerate(words):
            o = int(batch.cig_off[r]) + 3 * r
            self.new_cig[o:o + len(w)] = w
        self.ref_len = np.ascontiguousarray(ref_len, np.int32)
        self.trim_flags = np.ascontiguousarray(trim_flags, np.uint8)
        self.status = np.ascontiguousarray(status, np.uint8)

    @classmethod
    def of(cls, batch, t):
        words = [np.array(t.new_cig[int(batch.cig_off[r]) + 3 * r:int(batch.cig_off[r]) + 3 * r + int(t.new_ncig[r])], np.uint32) for r in range(batch.n)]
        return cls(batch, t.new_pos.copy(), words, t.ref_len.copy(), t.trim_flags.copy(), t.status.copy())

    def rows(self, batch, lo, hi):
        return Res(batch, self.new_pos[lo:hi], self.words[lo:hi], self.ref_len[lo:hi], self.trim_flags[lo:hi], self.status[lo:hi])

    def cigars(self):
        return [[(int(v) & 15, int(v) >> 4) for v in w] for w in self.words]


def cut(lines, chunk_bytes):
    """The lines in chunks of whole lines of about chunk_bytes (1: a line per chunk)."""
    chunks, cur = [], b""
    for l in lines:
        if cur and len(cur) + len(l) > chunk_bytes:
            chunks.append(cur); cur = b""
        cur += l
    if cur:
        chunks.append(cur)
    return chunks


def check_blocks(framed, stream):
    """Every block: the 16 constant bytes, BSIZE, a stream zlib inflates to the block's chunk, CRC-32 and ISIZE; all blocks but the
    last hold 0xFF00 bytes.  Returns the blocks' ISIZEs."""
    at, got, sizes = 0, [], []
    while at < len(framed):
        assert framed[at:at + 16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
        bsize = struct.unpack_from("<H", framed, at + 16)[0] + 1
        assert bsize <= 65536
        crc, isize = struct.unpack_from("<II", framed, at + bsize - 8)
        chunk = zlib.decompress(framed[at + 18:at + bsize - 8], -15)
        assert len(chunk) == isize and (zlib.crc32(chunk) & 0xFFFFFFFF) == crc
        got.append(chunk); sizes.append(isize)
        at += bsize
    assert at == len(framed) and b"".join(got) == stream
    assert all(s == BS for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= BS)
    return sizes


def twin_run(c, chunks, res_all, min_length, inp, final_with_last=False, python_chunks=()):
    """run_amplipy's walk on the twin: every chunk parsed, given its rows of ``res_all`` and encoded (the chunks whose numbers are
    in ``python_chunks`` through the Python codec and encode_bytes instead); the walk ends behind the chunk of a failing row, else
    with the final flush.  (record stream, framed blocks, infos)."""
    stream, framed, infos, lo = [], [], [], 0
    flushed = False

    def took(blocks, oi):
        assert oi.waits == 1 and c.guards_ok()
        infos.append(oi)
        stream.append(c.stream(int(oi.carry_in)).tobytes()); framed.append(blocks.tobytes())
    for k, chunk in enumerate(chunks):
        final = final_with_last and k + 1 == len(chunks)
        recs, _ = U.python_records(chunk, HDR)
        pb = U.python_batch(recs)
        res = res_all.rows(pb, lo, lo + pb.n)
        lo += pb.n
        if k in python_chunks:
            keep = U.keep_rule(res, min_length, inp)
            took(*c.encode_bytes(python_stream(recs, pb, res.new_pos, res.cigars(), keep), final=final))
            bad = int(np.nonzero(res.status)[0][0]) if res.status.any() else -1
        else:
            info = c.parse(chunk)
            assert info.first_odd_line == -1, (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason], chunk[:300])
            assert info.n_rows == pb.n
            bad = -1
            if info.n_rows:
                bad, _ = c.twin_set_results(res)
            took(*c.encode(min_length, inp, final=final))
            assert infos[-1].n_rows_written == int(U.keep_rule(res, min_length, inp).sum())
        flushed = final
        if bad >= 0:
            return b"".join(stream), b"".join(framed), infos          # (no flush behind a failing row)
    if not flushed:
        blocks, oi = c.encode(min_length, inp, final=True)             # the bare flush
        assert oi.n_rows_written == 0 and oi.carry_out == 0 and oi.stream_bytes == oi.carry_in
        took(blocks, oi)
    return b"".join(stream), b"".join(framed), infos


def expected(lines, res_all, min_length, inp):
    recs, _ = U.python_records(b"".join(lines), HDR)
    pb = U.python_batch(recs)
    return python_stream(recs, pb, res_all.new_pos, res_all.cigars(), U.keep_rule(res_all, min_length, inp))


def whole_batch(lines):
    recs, _ = U.python_records(b"".join(lines), HDR)
    return recs, U.python_batch(recs)


def oracle_results(pb):
    from oracle import oracle
    mn, mx, mpl = oracle.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0)
    t = oracle.process(pb, G.size, mn, mx, mpl, 20, 4).trim
    same = U.IdentityResult(pb)
    for i in np.nonzero(t.status)[0]:              # reads the oracle rejects: written unchanged here
        o = int(pb.cig_off[i]) + 3 * int(i)
        t.new_pos[i] = same.new_pos[i]; t.new_ncig[i] = same.new_ncig[i]
        t.new_cig[o:o + int(same.new_ncig[i])] = same.new_cig[o:o + int(same.new_ncig[i])]
    t.status[:] = 0
    return Res.of(pb, t)


def identity(pb):
    return Res.of(pb, U.IdentityResult(pb))


def seeded_lines(seed, n_amp=500, n_mixed=300, n_many=200):
    rng = np.random.default_rng(seed)
    segs = synth.make_amplicon_batch(G, AMPS, n_amp, seed=seed).segments() + synth.make_mixed_segments(G, AMPS, n_mixed, seed + 1) \
        + U.many_op_segments(rng, n_many, G.size)
    lines = U.segments_to_lines(segs, HDR, rng, max_aux=6)
    return [lines[i] for i in rng.permutation(len(lines))]


# ---- 1. stream equality ---------------------------------------------------------------------------------------------------------------
def test_stream_equals_the_python_writer_on_seeded_lines(twin):
    """Seeded amplicon, config-5 and many-op lines with AUX_POOL aux; results from the oracle (CIGARs grow and shrink) and results
    that change nothing; include_no_primer both ways; the text as one line per chunk, 64 KB chunks and whole."""
    lines = seeded_lines(41)
    recs, pb = whole_batch(lines)
    res = oracle_results(pb)
    old = np.diff(pb.cig_off.astype(np.int64))
    assert (res.new_ncig.astype(np.int64) > old).any() and (res.new_ncig.astype(np.int64) < old).any()
    sizes = set()
    for r, tag in ((res, "oracle"), (identity(pb), "identity")):
        for inp in (False, True):
            want = expected(lines, r, 30, inp)
            sizes.add(len(want))
            for chunk_bytes in (1, 65536, 1 << 30):
                stream, framed, infos = twin_run(twin, cut(lines, chunk_bytes), r, 30, inp, final_with_last=chunk_bytes == 65536)
                assert stream == want, (tag, inp, chunk_bytes)
                assert check_blocks(framed, want) == [BS] * (len(want) // BS) + ([len(want) % BS] if len(want) % BS else [])
                assert sum(int(i.n_blocks_host) for i in infos) == 0
                assert sum(int(i.bytes_down) for i in infos) == len(framed) + 128 * len(infos)
    # the settings keep different sets of rows (results that change nothing trim at no primer: nothing is kept without
    # include_no_primer), several blocks each
    assert sorted(sizes)[0] == 0 and len(sizes) == 4 and sorted(sizes)[1] > 2 * BS


def test_rows_behind_a_failing_row_and_chunks_without_kept_rows(twin):
    lines = seeded_lines(43, 200, 100, 60)
    recs, pb = whole_batch(lines)
    res = oracle_results(pb)
    whole = expected(lines, res, 30, True)
    # a chunk whose rows are all dropped by the filter, and one without rows at all
    chunks = cut(lines, 65536)
    n0 = U.python_batch(U.python_records(chunks[0], HDR)[0]).n
    n1 = U.python_batch(U.python_records(chunks[1], HDR)[0]).n
    res.ref_len[n0:n0 + n1] = 0
    chunks.insert(3, b"u1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\nnot a record\n\n")
    want = expected(lines, res, 30, True)
    stream, framed, infos = twin_run(twin, chunks, res, 30, True)
    assert stream == want and len(want) < len(whole)
    assert infos[1].n_rows_written == 0 and infos[3].n_rows_written == 0 and infos[3].stream_bytes == infos[3].carry_in
    check_blocks(framed, want)
    # nothing kept at all: no block
    stream, framed, infos = twin_run(twin, cut(lines, 65536), res, 10 ** 6, True)
    assert stream == b"" and framed == b""
    # a failing row: the rows in front of it, whole blocks only, whatever the cut
    res.status[pb.n // 2] = 6
    want = expected(lines, res, 30, True)
    assert 0 < len(want) < len(whole)
    for chunk_bytes in (1, 65536, 1 << 30):
        stream, framed, infos = twin_run(twin, cut(lines, chunk_bytes), res, 30, True)
        assert stream == want, chunk_bytes
        check_blocks(framed, want[:len(want) - len(want) % BS])
        assert infos[-1].carry_out == len(want) % BS
        twin.encode_bytes(b"", final=True)          # (a run ends there; this codec goes on: drop what was left over)


# ---- 2. the corners ---------------------------------------------------------------------------------------------------------------------
def L(*f):
    return ("\t".join(str(x) for x in f)).encode("ascii") + b"\n"


def line(name="g", flag=99, pos=100, cigar="20M", seq="ACGTACGTACGTACGTACGT", qual=None, rname=U.REF_NAME, rnext="=", mapq=60,
         pnext=300, tlen=220, aux=("NM:i:0",)):
    return L(name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, ("I" * len(seq) if seq != "*" else "*") if qual is None else qual, *aux)


INT_EDGES = [-129, -128, 127, 128, 255, 256, 32767, 32768, 65535, 65536, -2 ** 31, 2 ** 32 - 1, 0, -1, -32768, -32769, 2 ** 31 - 1, 2 ** 31]
FLOATS = ["0.25", "-0.0", "1e-05", "123456789012345", "0.000000000000001", "0", "1", "-1.5", "3.14159", "1e22", "1e-22", "999999999999999e22",
          "0.1", "16777217", "1.17549435e-14", "3.4028234e29", "100000000000000e-22", "7e+3", "0.300000000000000", "00012.500e01"]
B_RANGES = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}


def b_values(sub, n):
    if sub == "f":
        return [FLOATS[k % len(FLOATS)] for k in range(n)]
    lo, hi = B_RANGES[sub]
    return [str((lo, hi, 0, 1, hi - 1, lo + 1, 7)[k % 7]) for k in range(n)]


def corner_lines():
    out = [line("odd_lseq", cigar="19M", seq="ACGTACGTACGTACGTACG", qual="!#5?I~+,!#5?I~+,!#5"), line("even_lseq"),
           line("no_seq", seq="*", qual="*"), line("qual_star", qual="*"), line("one_base_qual_star", cigar="1M", seq="A", qual="*"),
           line("q"), line("n" * 254), line("no_aux", aux=()), line("forty_aux", aux=tuple("X%s:i:%d" % (chr(65 + k % 26) if k < 26 else chr(97 + k % 26), k * 1000 - 7) for k in range(40))),
           line("z_empty", aux=("XZ:Z:", "NM:i:3")), line("z_5000", aux=("NM:i:3", "XZ:Z:" + "z spaced ~" * 500, "YA:A:!")),
           line("h_field", aux=("ZH:H:", "YH:H:1AE301")), line("many_z", aux=tuple("Z%s:Z:%s" % (chr(65 + k), "v" * (k * 7 % 23)) for k in range(26))),
           line("hundred_aux", aux=tuple("%s%s:Z:%d" % (chr(65 + k // 26), chr(65 + k % 26), k) for k in range(100))),
           line("ints", aux=tuple("I%s:i:%d" % (chr(65 + k), v) for k, v in enumerate(INT_EDGES))),
           line("minus_zero_int", aux=("XI:i:-0",)),
           line("floats", aux=tuple("F%s:f:%s" % (chr(65 + k), v) for k, v in enumerate(FLOATS))),
           line("printable_tags", aux=("!~:A:~", "~!:A:!", "a1:Z:x", "X0:A::")),
           line("pos0", pos=1), line("pos_before", pos=0), line("rnext_star", rnext="*", pnext=0), line("rnext_other", rnext="OTHER", pnext=17),
           line("rname_other", rname="OTHER", rnext="=", pos=5), line("pnext0", rnext="*", pnext=0, tlen=-5, mapq=0, flag=0), line("mapq255", mapq=255),
           line("iupac", cigar="17M", seq="acgtnRYKMSWBDHVN="), line("alien", cigar="8M", seq="ACGTXZ.-"),
           line("cigar_ops", cigar="5H10S30M10S5H", seq="ACGTT" * 10), line("long_cigar", cigar="1M1I" * 110, seq="AC" * 110),
           line("unmapped", flag=4), line("nocigar", cigar="*"), b"three\tfields\tonly\n", b"\n"]
    for sub in "cCsSiIf":
        out.append(line("b0_" + sub, aux=("B%s:B:%s" % (sub, sub),)))
        out.append(line("b1_" + sub, aux=("NM:i:1", "B%s:B:%s,%s" % (sub, sub, b_values(sub, 1)[0]))))
        out.append(line("b300_" + sub, aux=("B%s:B:%s,%s" % (sub, sub, ",".join(b_values(sub, 300))), "XT:A:U")))
    for n in range(1, 20):
        out.append(line("len%d" % n, cigar="%dM" % n, seq=("GATTACAN" * 4)[:n], qual=("!#5?I~+," * 4)[:n]))
    out += [l[:-1] + b"\r\n" for l in (line("crlf", aux=("XZ:Z:ends here",)), line("crlf_noaux", aux=()), line("crlf_f", aux=("XF:f:0.5",)))]
    return out


def corner_results(pb, seed):
    """Results that change nothing, then a few rows by hand: pos 0 and -1, a new CIGAR of 0 ops, of old + 3 ops, without a
    reference-consuming op."""
    rng = np.random.default_rng(seed)
    res = identity(pb)
    words = [w.copy() for w in res.words]
    pos = res.new_pos.copy()
    for r in range(pb.n):
        k = r % 6
        if k == 1:
            words[r] = np.zeros(0, np.uint32)
        elif k == 2:
            words[r] = np.concatenate([np.array([(3 << 4) | 4], np.uint32), words[r], np.array([(2 << 4) | 1, (9 << 4) | 4], np.uint32)])
        elif k == 3:
            words[r] = np.array([(int(rng.integers(1, 400)) << 4) | 4, (5 << 4) | 1], np.uint32)[:len(words[r]) + 3]
        elif k == 4:
            pos[r] = 0
        elif k == 5:
            pos[r] = int(rng.integers(0, 1 << 29))
    pos[7 % pb.n] = -1
    return Res(pb, pos, words, res.ref_len, res.trim_flags, res.status)


def test_corner_lines(twin):
    lines = corner_lines()
    recs, pb = whole_batch(lines)
    assert pb.n >= len(lines) - 4
    for seed in (1, 2):
        res = corner_results(pb, seed) if seed == 1 else identity(pb)
        want = expected(lines, res, 0, True)
        for chunk_bytes in (1, 4096, 1 << 30):
            stream, framed, infos = twin_run(twin, cut(lines, chunk_bytes), res, 0, True, final_with_last=chunk_bytes == 4096)
            assert stream == want, (seed, chunk_bytes)
            check_blocks(framed, want)
    # every line as a chunk of its own behind and in front of another one (tab tables that start and end in the line)
    res = identity(pb)
    for l in lines:
        for text in ([l, lines[1]], [lines[1], l]):
            r2, b2 = whole_batch(text)
            i2 = identity(b2)
            stream, framed, infos = twin_run(twin, [b"".join(text)], i2, 0, True)
            assert stream == expected(text, i2, 0, True), l[:60]


def float_spellings(n, seed):
    """Spellings of the exact set, seeded: up to 15 digits with or without a point and an exponent, three in ten negative (of n
    draws, those outside the set are left out)."""
    rng = np.random.default_rng(seed)
    vals = []
    for _ in range(n):
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        cutp = int(rng.integers(1, nd + 1))
        s = digits[:cutp] + ("." + digits[cutp:] if cutp < nd else "")
        p = int(rng.integers(-22, 23)) + (nd - cutp)
        if rng.random() < 0.7 and -60 < p < 60:
            s += "e" + ("+" if rng.random() < 0.2 and p >= 0 else "") + str(p)
        elif not -22 <= -(nd - cutp) <= 22:
            continue
        vals.append(("-" if rng.random() < 0.3 else "") + s)
    return vals


def float_lines(vals):
    """One line per spelling: as an f field and twice in a B:f array."""
    return [line("f%d" % k, aux=("XF:f:" + v, "BF:B:f," + v + "," + v)) for k, v in enumerate(vals)]


def test_floats_are_packed_like_struct_pack(twin):
    """Spellings of the exact set, seeded: the bytes of the f field are struct.pack("<f", float(v))."""
    vals = float_spellings(3000, 5)
    lines = float_lines(vals)
    recs, pb = whole_batch(lines)
    res = identity(pb)
    stream, framed, infos = twin_run(twin, [b"".join(lines)], res, 0, True)
    assert stream == expected(lines, res, 0, True)
    assert all(struct.pack("<f", float(v)) in stream for v in vals[:50])


# ---- 3. oddness ---------------------------------------------------------------------------------------------------------------------------
def odd_lines():
    a = lambda *x: line("odd", aux=("NM:i:1",) + x + ("XT:A:U",))        # noqa: E731
    return [
        (line("n" * 255), "QNAME"), (line("n" * 400, aux=()), "QNAME"),
        (line("ops", cigar="1M1I" * 32767, seq="AC" * 32767), "CIGAR_OPS"),
        (a("X:i:1"), "AUX_TAG"), (a("XYi:1"), "AUX_TAG"), (a("XY:i1"), "AUX_TAG"), (a("XY:i"), "AUX_TAG"), (a(""), "AUX_TAG"), (a("XY:Q:1"), "AUX_TAG"),
        (a("X Y:i:1".replace(" Y", " ")), "AUX_TAG"), (a("XY:z:abc"), "AUX_TAG"), (a("XYZ:i:1"), "AUX_TAG"),
        (a("XA:A:"), "AUX_A"), (a("XA:A:ab"), "AUX_A"),
        (a("XI:i:"), "AUX_INT"), (a("XI:i:+5"), "AUX_INT"), (a("XI:i:007"), "AUX_INT"), (a("XI:i:1_0"), "AUX_INT"), (a("XI:i: 5"), "AUX_INT"),
        (a("XI:i:0x10"), "AUX_INT"), (a("XI:i:-"), "AUX_INT"), (a("XI:i:1.0"), "AUX_INT"),
        (a("XI:i:4294967296"), "AUX_INT_RANGE"), (a("XI:i:-2147483649"), "AUX_INT_RANGE"), (a("XI:i:123456789012345678901234567890"), "AUX_INT_RANGE"),
        (a("XB:B:"), "AUX_B"), (a("XB:B:x,1"), "AUX_B"), (a("XB:B:c1"), "AUX_B"), (a("XB:B:c,"), "AUX_B"), (a("XB:B:c,1,,2"), "AUX_B"),
        (a("XB:B:c,1,"), "AUX_B"), (a("XB:B:i,+1"), "AUX_B"), (a("XB:B:s,1.5"), "AUX_B"), (a("XB:B:f,,1"), "AUX_B"),
        (a("XB:B:c,128"), "AUX_B_RANGE"), (a("XB:B:c,1,-129"), "AUX_B_RANGE"), (a("XB:B:C,-1"), "AUX_B_RANGE"), (a("XB:B:C,256"), "AUX_B_RANGE"),
        (a("XB:B:s,32768"), "AUX_B_RANGE"), (a("XB:B:S,65536"), "AUX_B_RANGE"), (a("XB:B:i,2147483648"), "AUX_B_RANGE"), (a("XB:B:I,4294967296"), "AUX_B_RANGE"),
        (a("XB:B:I,-1"), "AUX_B_RANGE"),
        (a("XF:f:inf"), "AUX_FLOAT"), (a("XF:f:nan"), "AUX_FLOAT"), (a("XF:f:1234567890123456"), "AUX_FLOAT"), (a("XF:f:1e23"), "AUX_FLOAT"),
        (a("XF:f:1e-23"), "AUX_FLOAT"), (a("XF:f:0.00000000000000000000001"), "AUX_FLOAT"), (a("XF:f:1."), "AUX_FLOAT"), (a("XF:f:.5"), "AUX_FLOAT"),
        (a("XF:f:1E5"), "AUX_FLOAT"), (a("XF:f:+1"), "AUX_FLOAT"), (a("XF:f:"), "AUX_FLOAT"), (a("XF:f:1e"), "AUX_FLOAT"), (a("XF:f:0x1p3"), "AUX_FLOAT"),
        (a("XF:f:1e400"), "AUX_FLOAT"), (a("XB:B:f,0.5,inf"), "AUX_FLOAT"), (a("XB:B:f,1e23"), "AUX_FLOAT"),
    ]


def test_new_odd_lines_are_reported_with_bam_output_only(twin, twin_so):
    """Every new category first, in the middle and last in a chunk: the right line and reason.  The same text with text output is
    not odd (MAPQ above 255, which the issue lists too, is AMP_SAM_ODD_RANGE with either output: test_sam_text.py has it)."""
    seeded = seeded_lines(31, 20, 10, 5)
    text_twin = new_twin(twin_so, None, sam_native.OUT_TEXT)
    for l, reason in odd_lines():
        for where in (0, len(seeded) // 2, len(seeded)):
            chunk = b"".join(seeded[:where]) + l + b"".join(seeded[where:])
            info = twin.parse(chunk)
            assert (info.first_odd_line, sam_native.ODD_REASONS[info.odd_reason]) == (where, reason), l[-80:]
        info = text_twin.parse(b"".join(seeded[:3]) + l + b"".join(seeded[3:]))
        assert info.first_odd_line == -1, l[-80:]
    info = twin.parse(line("mapq", mapq=256))
    assert (info.first_odd_line, info.odd_reason) == (0, ODD["RANGE"])
    # two odd lines: the first one is reported; a fault in the core fields goes before one in the aux fields of the same line
    info = twin.parse(seeded[0] + line(aux=("XF:f:inf",)) + seeded[1] + line(aux=("XA:A:",)))
    assert (info.first_odd_line, info.odd_reason) == (1, ODD["AUX_FLOAT"])
    info = twin.parse(line(flag="099", aux=("XF:f:inf",)))
    assert (info.first_odd_line, info.odd_reason) == (0, ODD["INT"])
    # an odd chunk is not encoded: the call behind it appends nothing
    blocks, oi = twin.encode(0, True, final=True)
    assert oi.n_rows_written == 0
    # aux fields of records that are no rows are looked at as well (stricter than needed: a fallback, never a difference)
    info = twin.parse(line("unmapped", flag=4, aux=("XF:f:inf",)))
    assert info.odd_reason == ODD["AUX_FLOAT"]
    text_twin.close()


def test_the_python_codec_differs_or_raises_on_the_new_odd_lines():
    """Why those lines are odd: the Python codec raises on them, writes a record a reader cannot walk, or -- where the device's rule
    is stricter than needed -- takes a spelling the device does not read."""
    strict_ok = 0
    for l, reason in odd_lines():
        try:
            recs, _ = U.python_records(l, HDR)
            pb = U.python_batch(recs)
            res = identity(pb)
            data = python_stream(recs, pb, res.new_pos, res.cigars(), np.ones(pb.n, bool))
            back = bamio.aux_bam_to_sam(bamio.aux_sam_to_bam(recs[0].aux_sam))
        except Exception:
            continue
        if back != recs[0].aux_sam:
            continue
        strict_ok += 1                              # e.g. "XI:i:007" never comes back as written, but its bytes are fine
        assert reason in ("AUX_INT", "AUX_B", "AUX_FLOAT", "AUX_TAG", "AUX_A", "QNAME", "CIGAR_OPS"), l[-80:]
        assert len(data) > 36
    assert strict_ok < len(odd_lines())


def test_a_python_chunk_between_two_device_chunks(twin):
    """A chunk with an odd line goes through the Python codec and encode_bytes: the same stream and the same block boundaries as
    the Python codec on all three chunks."""
    lines = seeded_lines(47, 600, 300, 150)
    third = len(lines) // 3
    lines.insert(third + 5, line("odd_float", pos=5000, cigar="80M", seq="ACGT" * 20, aux=("XF:f:1e23",)))
    chunks = [b"".join(lines[:third]), b"".join(lines[third:2 * third]), b"".join(lines[2 * third:])]
    assert twin.parse(chunks[1]).odd_reason == ODD["AUX_FLOAT"]
    recs, pb = whole_batch(lines)
    res = oracle_results(pb)
    want = expected(lines, res, 30, True)
    assert struct.pack("<f", 1e23) in want
    for final_with_last in (False, True):
        stream, framed, infos = twin_run(twin, chunks, res, 30, True, final_with_last=final_with_last, python_chunks=(1,))
        assert stream == want
        sizes = check_blocks(framed, want)
        assert sizes == [BS] * (len(want) // BS) + [len(want) % BS] and len(sizes) >= 5     # (no chunk ends at a block's end)
        assert infos[1].n_rows_written == 0 and infos[1].stream_bytes > infos[1].carry_in
    # all three through encode_bytes: the same blocks again
    stream2, framed2, _ = twin_run(twin, chunks, res, 30, True, python_chunks=(0, 1, 2))
    assert stream2 == want and check_blocks(framed2, want) == sizes


# ---- 4. framing ------------------------------------------------------------------------------------------------------------------------------
def test_block_that_does_not_fit_goes_through_the_host_and_is_counted(twin_so):
    lines = seeded_lines(49, 300, 150, 80)
    recs, pb = whole_batch(lines)
    res = oracle_results(pb)
    want = expected(lines, res, 30, True)
    assert len(want) > 2 * BS
    for refuse, n_host in (((1,), 1), ((), 0)):
        c = new_twin(twin_so, _zlib_deflater(refuse=refuse))
        stream, framed, infos = twin_run(c, [b"".join(lines)], res, 30, True)
        assert stream == want
        assert sum(int(i.n_blocks_host) for i in infos) == n_host
        assert sum(int(i.n_blocks) for i in infos) == (len(want) + BS - 1) // BS
        check_blocks(framed, want)                  # (the refused chunk came down raw and was compressed on the host)
        assert sum(int(i.bytes_down) for i in infos) == (sum(int(i.file_bytes) for i in infos) + 128 * len(infos) + BS * n_host)
        c.close()


def test_entry_points_and_states(twin, twin_so):
    import ctypes as C
    info = bam_device.AmpBamOutInfo()
    t = new_twin(twin_so, None, sam_native.OUT_TEXT)
    assert t.L.amp_sam_encode(t.h, C.c_int32(0), C.c_int32(1), C.c_int32(0), C.byref(info)) == -5          # text output: AMP_ESTATE
    assert t.L.amp_sam_encode_bytes(t.h, b"abcd", C.c_int64(4), C.c_int32(0), C.byref(info)) == -5
    assert t.L.amp_sam_set_output(t.h, C.c_int32(2)) == -1
    t.close()
    twin.parse(line())
    assert twin.L.amp_sam_encode(twin.h, C.c_int32(0), C.c_int32(1), C.c_int32(0), C.byref(info)) == -5     # rows, and no results yet
    assert twin.L.amp_sam_encode(None, C.c_int32(0), C.c_int32(1), C.c_int32(0), C.byref(info)) == -1
    assert twin.L.amp_sam_encode_bytes(twin.h, None, C.c_int64(4), C.c_int32(0), C.byref(info)) == -1
    pb = twin.batch()
    twin.twin_set_results(identity(pb))
    assert twin.verdict() == (-1, 0)
    blocks, oi = twin.encode(0, True)
    assert oi.n_rows_written == 1 and oi.n_blocks == 0 and oi.carry_out == oi.stream_bytes > 36
    blocks, oi2 = twin.encode(0, True)               # the same chunk again: nothing new
    assert oi2.n_rows_written == 0 and oi2.carry_in == oi.carry_out == oi2.carry_out and blocks.size == 0
    blocks, oi3 = twin.encode_bytes(b"", final=True)  # a bare flush through either entry point
    assert oi3.n_blocks == 1 and oi3.carry_out == 0 and check_blocks(blocks.tobytes(), twin.stream().tobytes()) == [oi.stream_bytes]
    assert twin.waits() > 0


def test_record_bytes_function_is_the_writers(tmp_path):
    """bamio.bam_record_bytes is what AlignmentWriter.write appends in BAM mode: a file written record by record reads back."""
    lines = corner_lines()
    recs, pb = whole_batch(lines)
    path = str(tmp_path / "w.bam")
    w = bamio.AlignmentWriter(path, "wb", HDR)
    for r in recs:
        w.write(r)
    w.close()
    payload = b"".join(bamio.bgzf_blocks(open(path, "rb")))
    assert payload.endswith(b"".join(bamio.bam_record_bytes(r, r.pos, r.cigar) for r in recs))
    back = list(bamio.AlignmentReader(path, "rb"))
    assert [(r.qname, r.flag, r.pos, r.cigar, r.mapq, r.next_ref_id, r.next_pos, r.tlen) for r in back] == \
           [(r.qname, r.flag, r.pos, r.cigar, r.mapq, r.next_ref_id, r.next_pos, r.tlen) for r in recs]


# ---- 5. sanitizers -----------------------------------------------------------------------------------------------------------------------------
def test_encode_under_the_sanitizers(tmp_path):
    """tests/hostsim/samout_fuzz.cpp: the twin as a program under -fsanitize=address,undefined (host code only), guard bytes behind
    every buffer of the encoder: random lines (damaged aux among them), results and cuts; every chunk is odd or its bytes equal a
    plain serial encode written in the fuzz program; at least half of the chunks are not odd."""
    exe = sam_native.build_twin(str(tmp_path / "samout_fuzz"), sanitize=True, main_source=os.path.join(ROOT, "tests", "hostsim", "samout_fuzz.cpp"))
    r = subprocess.run([exe, "400"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runs 400" in r.stdout and "mismatches 0" in r.stdout and "guards 0" in r.stdout
    done = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(done["chunks"]) >= 1500 and 2 * int(done["odd"]) <= int(done["chunks"])
