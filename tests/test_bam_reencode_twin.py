"""The device re-encoder of trimmed BAM records (amp_bamout.hip / bam_device.BamCodec.encode) on its host
twin: the lane functions compiled with -DAMPBGZF_HOSTSIM and run lane after lane.  The uncompressed record stream against the
payload of the file bam_native.BamWriter.write_rows writes from the same results, at several piece sizes; the framed blocks
against zlib and the BGZF rules; the file through both host readers.  No GPU needed."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from amplipy_amd import abi, bam_device, bam_native, bamio, lib, synth
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = bamio.Header("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:SYN_REF\tLN:%d\n" % G.size, [("SYN_REF", int(G.size))])
BS = 0xFF00
PIECES = (1, 65536, 1 << 20, 1 << 30)                 # one block, 64 KB, 1 MB, the whole file


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return bam_device.build_twin(str(tmp_path_factory.mktemp("twin") / "libampbgzf_twin.so"))


def _zlib_deflater(refuse=()):
    """A TWIN_DEFLATE_FN on zlib; the chunks whose numbers are in ``refuse`` come back with out_len 0 (as if they did not fit)."""
    def fn(inp, n_bytes, block_bytes, out, stride, room, out_len):
        n = (n_bytes + block_bytes - 1) // block_bytes
        for k in range(n):
            data = C.string_at(inp + k * block_bytes, min(block_bytes, n_bytes - k * block_bytes))
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            comp = co.compress(data) + co.flush()
            if k in refuse or len(comp) > room:
                out_len[k] = 0
                continue
            C.memmove(out + k * stride, comp, len(comp))
            out_len[k] = len(comp)
        return 0
    return bam_device.TWIN_DEFLATE_FN(fn)


@pytest.fixture(scope="module")
def deflater(tmp_path_factory):
    """The encoder of the twin's encodes: amp_deflate.hip's host phases (ampdf_hostsim_blocks) where hipcc can build them, zlib
    behind the same signature otherwise."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.isfile("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        return _zlib_deflater()
    from amplipy_amd import build
    so = str(tmp_path_factory.mktemp("ampdf") / "libampdf_hostsim.so")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                           "-o", so, os.path.join(build.CSRC, "amp_deflate.hip")])
    sim = C.CDLL(so)
    fn = C.cast(sim.ampdf_hostsim_blocks, C.c_void_p)
    fn._keep = sim
    return fn


class Results:
    """new_pos, new_ncig, new_cig (row r's words at cig_off[r] + 3 r), ref_len, trim_flags of the rows of ``batch``."""

    def __init__(self, batch, new_pos, new_ncig, words, ref_len, trim_flags):
        self.new_pos, self.new_ncig, self.ref_len, self.trim_flags = new_pos, new_ncig, ref_len, trim_flags
        self.words = words                                      # per row: its new CIGAR words
        self.slot_off = batch.cig_off[:-1] + np.uint64(3) * np.arange(batch.n, dtype=np.uint64)
        self.new_cig = np.zeros(int(batch.cig_off[-1]) + 3 * batch.n + 1, np.uint32)
        for r, w in enumerate(words):
            self.new_cig[int(self.slot_off[r]):int(self.slot_off[r]) + len(w)] = w

    @classmethod
    def of_trim(cls, batch, t):
        slot = batch.cig_off[:-1] + np.uint64(3) * np.arange(batch.n, dtype=np.uint64)
        words = [t.new_cig[int(slot[r]):int(slot[r]) + int(t.new_ncig[r])].copy() for r in range(batch.n)]
        return cls(batch, t.new_pos.copy(), t.new_ncig.copy(), words, t.ref_len.copy(), t.trim_flags.copy())

    def rows(self, batch, lo, hi):
        """The results of rows [lo, hi) laid out for ``batch``, the piece's own batch of those rows."""
        return Results(batch, self.new_pos[lo:hi].copy(), self.new_ncig[lo:hi].copy(), self.words[lo:hi], self.ref_len[lo:hi].copy(),
                       self.trim_flags[lo:hi].copy())


def _keep(res, min_length, include_no_primer, first_bad):
    keep = (res.ref_len >= min_length) & (((res.trim_flags & 3) != 0) | bool(include_no_primer))      # AmpliPy.py:910
    if first_bad >= 0:
        keep[first_bad:] = False
    return keep


def host_file(path, src_path, res, min_length, include_no_primer, first_bad=-1):
    """The file BamWriter.write_rows writes from the results: (its inflated payload behind the header blocks, its path)."""
    f = bam_native.BamFile(src_path)
    want, _ = f.decode(0, f.n_records, copy=True)
    w = bam_native.BamWriter(path, f.header_text, f, level=6)
    hb = w.header_bytes
    w.write_rows(f, want.src_index, _keep(res, min_length, include_no_primer, first_bad), res.new_pos, res.new_ncig, res.slot_off, res.new_cig)
    w.close(); f.close()
    return payload_behind(path, hb)


def payload_behind(path, header_bytes):
    tab = bam_device.block_table(path)
    raw = open(path, "rb").read()
    return b"".join(zlib.decompress(raw[int(o):int(o + n)], -15) for o, n, isz, _ in tab if int(o) - 18 >= header_bytes and isz)


def twin_run(twin, deflater, src_path, out_path, res, piece_bytes, min_length, include_no_primer, first_bad=-1, final_with_last=False):
    """run_amplipy's walk on the twin with the results ``res`` of the whole file's rows (first_bad: the walk ends behind the piece of
    that row, as the run does): (the record stream of all encodes, per-encode infos, stats, bytes of the header blocks); the file
    is written through bam_device.DeviceBamOutput.  final_with_last: the last piece's encode is the final one; else a bare final
    flush follows."""
    src = bam_device.DeviceBamInput(src_path, piece_bytes)
    c = bam_device.BamCodec(twin=twin)
    c.set_deflater(deflater)
    out = bam_device.DeviceBamOutput(out_path, src.header_text, src.references, level=6)
    stream, infos, lo, st = [], [], 0, None
    n_pieces = len(src.pieces)
    flushed = False
    for k, (info, st) in enumerate(bam_device.walk(c, src)):
        final = final_with_last and k + 1 == n_pieces
        local_bad = -1
        if info.n_rows:
            b = c.batch()
            hi = lo + b.n
            local_bad = first_bad - lo if lo <= first_bad < hi else -1
            c.set_trim(res.rows(b, lo, hi), first_bad=local_bad)
            lo = hi
        elif not final:
            continue                                            # run_amplipy does not encode a piece without rows
        oi = out.encode(c, st, min_length, include_no_primer, final=final)
        flushed = final
        infos.append(oi)
        stream.append(c.stream(int(oi.carry_in)).tobytes())
        assert c.guards_ok()
        if local_bad >= 0:
            flushed = False
            break
    if not flushed:
        oi = out.encode(c, st, min_length, include_no_primer, final=True)       # the bare final flush
        infos.append(oi)
        assert oi.n_rows_written == 0 and oi.carry_out == 0 and oi.stream_bytes == oi.carry_in
    assert c.guards_ok()
    out.close()
    c.close()
    return b"".join(stream), infos, dict(st), out.writer.header_bytes


def check_blocks(path, header_bytes, payload):
    """Every block behind the header blocks: the 16 constant bytes, BSIZE, a stream zlib inflates to the block's chunk, CRC-32
    and ISIZE; all blocks but the last hold 0xFF00 bytes; then the end-of-file block."""
    raw = open(path, "rb").read()
    assert raw.endswith(bam_native.BGZF_EOF)
    at, got, sizes = header_bytes, [], []
    while at < len(raw) - len(bam_native.BGZF_EOF):
        assert raw[at:at + 16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        body = raw[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        chunk = zlib.decompress(body, -15)
        assert len(chunk) == isize and (zlib.crc32(chunk) & 0xFFFFFFFF) == crc
        got.append(chunk); sizes.append(isize)
        at += bsize
    assert at == len(raw) - len(bam_native.BGZF_EOF)
    assert b"".join(got) == payload
    assert all(s == BS for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= BS)
    return len(sizes)


def check_readers(path, host_path):
    """The file reads back through bam_native.BamFile and through bamio like the host writer's."""
    a, b = bam_native.BamFile(path), bam_native.BamFile(host_path)
    assert a.n_records == b.n_records and a.header_text == b.header_text and a.references == b.references
    ba, _ = a.decode(0, a.n_records, copy=True); bb, _ = b.decode(0, b.n_records, copy=True)
    for name in ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual"):
        assert np.array_equal(getattr(ba, name), getattr(bb, name)), name
    a.close(); b.close()
    ra = [(r.qname, r.flag, r.pos, r.cigar, r.seq) for r in bamio.AlignmentReader(path, "rb")]
    rb = [(r.qname, r.flag, r.pos, r.cigar, r.seq) for r in bamio.AlignmentReader(host_path, "rb")]
    assert ra == rb
    return len(ra)


def _oracle_results(path):
    f = bam_native.BamFile(path)
    want, _ = f.decode(0, f.n_records, copy=True)
    f.close()
    mn, mx, mpl = lib.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0)
    t = oracle.process(want, G.size, mn, mx, mpl, 20, 4, do_count=False).trim
    assert not t.status.any()
    return want, Results.of_trim(want, t)


def _all_checks(twin, deflater, tmp_path, src, res, tag, min_length=30, include_no_primer=False, first_bad=-1, pieces=PIECES):
    host_path = str(tmp_path / ("host_%s.bam" % tag))
    payload = host_file(host_path, src, res, min_length, include_no_primer, first_bad)
    for pb in pieces:
        out_path = str(tmp_path / ("dev_%s_%d.bam" % (tag, pb)))
        stream, infos, st, header_bytes = twin_run(twin, deflater, src, out_path, res, pb, min_length, include_no_primer, first_bad,
                                                    final_with_last=pb == 65536)
        assert stream == payload, (tag, pb)
        assert st["out_blocks_host"] == 0 and all(i.waits == 1 for i in infos)
        assert os.path.getsize(out_path) == header_bytes + st["bytes_out_file"] + len(bam_native.BGZF_EOF)
        n_blocks = check_blocks(out_path, header_bytes, payload)
        assert n_blocks == st["out_blocks_device"] == (len(payload) + BS - 1) // BS
        assert st["bytes_out_file"] == sum(int(i.file_bytes) for i in infos)
        assert st["bytes_down"] == st["bytes_out_file"] + 128 * len(infos)
        check_readers(out_path, host_path)
    return payload


def _write_recs(path, recs):
    w = bamio.AlignmentWriter(path, "wb", HDR)
    for r in recs:
        w.write(r)
    w.close()
    return path


def test_stream_equals_write_rows_on_amplicon_and_config5_reads(twin, deflater, tmp_path):
    """The amplicon batch written by ampbam_write_batch and the config-5 mix of make_mixed_segments written by the Python codec (aux
    fields; soft clips and indels, so the trimmed CIGAR both grows and shrinks), trim results from the oracle."""
    from tools.e2e_legs import write_bam
    p1 = str(tmp_path / "amp.bam")
    write_bam(p1, synth.make_amplicon_batch(G, AMPS, 12000, seed=5), int(G.size))
    want, res = _oracle_results(p1)
    payload = _all_checks(twin, deflater, tmp_path, p1, res, "amp")
    assert len(payload) > 10 * BS
    segs = synth.make_mixed_segments(G, AMPS, 6000, seed=3)
    recs = [bamio.Rec("r%d" % i, s.flag, 0, s.reference_start, 60, s.cigartuples, 0, s.reference_start, s.template_length, s.query_sequence,
                      bytes(s.query_qualities), aux_sam=["NM:i:%d" % (i % 5), "XS:Z:%s" % ("x" * (i % 40))]) for i, s in enumerate(segs)]
    p2 = _write_recs(str(tmp_path / "c5.bam"), recs)
    want, res = _oracle_results(p2)
    old = np.diff(want.cig_off.astype(np.int64))
    assert (res.new_ncig.astype(np.int64) > old).any() and (res.new_ncig.astype(np.int64) < old).any()
    for inp in (False, True):
        _all_checks(twin, deflater, tmp_path, p2, res, "c5_%d" % inp, include_no_primer=inp, pieces=(1, 65536, 1 << 30))


def _edge_file(tmp_path):
    rng = np.random.default_rng(23)
    segs = synth.make_mixed_segments(G, AMPS, 1500, seed=9)
    recs = []
    for i, s in enumerate(segs):
        recs.append(bamio.Rec("e%d" % i, s.flag, 0, s.reference_start, 60, s.cigartuples, 0, s.reference_start, s.template_length, s.query_sequence,
                              bytes(s.query_qualities), aux_sam=["NM:i:%d" % (i % 7)]))
        if i in (200, 900):                                     # 50,000 bytes of aux: the record spans several output blocks
            r = recs[-1]
            r.aux_bam = b"zzBC" + struct.pack("<I", 50000) + bytes(rng.integers(0, 256, 50000, dtype=np.uint8))
            r.aux_sam = None
        if i % 211 == 5:                                        # unmapped, and without a CIGAR: records that are no rows
            recs.append(bamio.Rec("u%d" % i, 4, -1, -1, 0, None, -1, -1, 0, "ACGT", bytes([30] * 4)))
            recs.append(bamio.Rec("n%d" % i, 0, 0, 77, 60, None, -1, -1, 0, "ACGTA", None))
    return _write_recs(str(tmp_path / "edge.bam"), recs)


def _made_up_results(want, seed, drop_runs=True):
    """Results no read pass gave, to reach what the oracle's do not: pos 0 and -1, CIGARs without a reference-consuming op, 0 to
    old + 3 ops, long runs of rows that are not kept."""
    rng = np.random.default_rng(seed)
    n = want.n
    old = np.diff(want.cig_off.astype(np.int64))
    new_ncig = np.minimum(rng.integers(0, 4, n) + np.maximum(old - rng.integers(0, 3, n), 0), old + 3).astype(np.uint32)
    words = []
    for r in range(n):
        ops = rng.integers(0, 9, int(new_ncig[r]))
        if r % 5 == 0:
            ops = rng.choice(np.array([1, 4, 5, 6]), int(new_ncig[r]))         # I S H P: rlen 0, the `rlen ? rlen : 1` bin
        words.append(((rng.integers(1, 400, int(new_ncig[r])).astype(np.uint32) << np.uint32(4)) | ops.astype(np.uint32)).astype(np.uint32))
    new_pos = rng.integers(0, G.size, n).astype(np.int32)
    new_pos[::7] = 0
    new_pos[3::31] = -1
    ref_len = rng.integers(0, 200, n).astype(np.int32)
    flags = rng.integers(0, 4, n).astype(np.uint8) | (rng.integers(0, 2, n).astype(np.uint8) << 2)
    if drop_runs:
        ref_len[n // 3:n // 3 + 500] = 0                        # pieces of one block without a kept row
    return Results(want, new_pos, new_ncig, words, ref_len, flags)


def test_edge_cases(twin, deflater, tmp_path):
    """Records with 50,000 bytes of aux, pieces without a kept row, pos 0 and -1, CIGARs without a reference-consuming op, records
    that are no rows, include_no_primer both ways, rows behind a failing row dropped, nothing kept at all."""
    src = _edge_file(tmp_path)
    f = bam_native.BamFile(src)
    want, _ = f.decode(0, f.n_records, copy=True)
    assert f.n_records > want.n
    f.close()
    res = _made_up_results(want, 1)
    for inp in (False, True):
        _all_checks(twin, deflater, tmp_path, src, res, "edge_%d" % inp, min_length=60, include_no_primer=inp, pieces=(1, 65536, 1 << 30))
    payload = _all_checks(twin, deflater, tmp_path, src, res, "bad", min_length=60, include_no_primer=True, first_bad=want.n // 2, pieces=(1, 1 << 30))
    whole = _all_checks(twin, deflater, tmp_path, src, res, "good", min_length=60, include_no_primer=True, pieces=(1 << 30,))
    assert 0 < len(payload) < len(whole) and whole.startswith(payload)
    none = _all_checks(twin, deflater, tmp_path, src, res, "none", min_length=10 ** 6, include_no_primer=True, pieces=(1, 1 << 30))
    assert none == b""


def test_empty_file_and_zero_row_pieces(twin, deflater, tmp_path):
    """A file without records, and one whose only records are no rows: a feed with zero rows, then the final flush -- header
    blocks and the end-of-file block, like the host writer's file."""
    for tag, recs in (("empty", []), ("norows", [bamio.Rec("u%d" % i, 4, -1, -1, 0, None, -1, -1, 0, "ACGT", bytes([30] * 4)) for i in range(50)])):
        src = _write_recs(str(tmp_path / (tag + ".bam")), recs)
        f = bam_native.BamFile(src)
        want, _ = f.decode(0, f.n_records, copy=True)
        f.close()
        assert want.n == 0
        res = _made_up_results(want, 2, drop_runs=False)
        host_path = str(tmp_path / ("host_%s.bam" % tag))
        assert host_file(host_path, src, res, 30, True) == b""
        out_path = str(tmp_path / ("dev_%s.bam" % tag))
        s = bam_device.DeviceBamInput(src)
        c = bam_device.BamCodec(twin=twin)
        c.set_deflater(deflater)
        out = bam_device.DeviceBamOutput(out_path, s.header_text, s.references, level=6)
        for info, st in bam_device.walk(c, s):
            assert info.n_rows == 0
            oi = out.encode(c, st, 30, True)                    # (encode works behind a feed without rows)
            assert oi.n_blocks == 0 and oi.file_bytes == 0 and oi.stream_bytes == 0
        oi = out.encode(c, st, 30, True, final=True)
        assert oi.n_blocks == 0 and oi.file_bytes == 0
        out.close(); c.close()
        assert open(out_path, "rb").read() == open(host_path, "rb").read()


def test_encode_needs_results_and_encodes_a_feed_once(twin, deflater, tmp_path):
    from tools.e2e_legs import write_bam
    src = str(tmp_path / "a.bam")
    write_bam(src, synth.make_amplicon_batch(G, AMPS, 3000, seed=6), int(G.size))
    want, res = _oracle_results(src)
    s = bam_device.DeviceBamInput(src, 1 << 30)
    c = bam_device.BamCodec(twin=twin)
    c.set_deflater(deflater)
    (info, st), = list(bam_device.walk(c, s))
    with pytest.raises(lib.AmpliHipError):
        c.encode(30, False)                                     # rows, and no results yet
    c.set_trim(res.rows(c.batch(), 0, want.n))
    blocks, oi = c.encode(30, False)
    assert oi.n_rows_written == int(_keep(res, 30, False, -1).sum()) and oi.n_blocks == oi.stream_bytes // BS and oi.carry_out == oi.stream_bytes % BS
    blocks2, oi2 = c.encode(30, False)                          # the same feed again: nothing new
    assert oi2.n_rows_written == 0 and oi2.n_blocks == 0 and oi2.carry_in == oi.carry_out == oi2.carry_out and blocks2.size == 0
    blocks3, oi3 = c.encode(30, False, final=True)
    assert oi3.n_blocks == (1 if oi.carry_out else 0) and oi3.carry_out == 0
    # a CIGAR of more than 65,535 ops is refused like ampbam_write_rows refuses it, and nothing is appended
    (info, st), = list(bam_device.walk(c, bam_device.DeviceBamInput(src, 1 << 30)))
    bad = res.rows(c.batch(), 0, want.n)
    keep = np.nonzero(_keep(bad, 30, False, -1))[0]
    bad.new_ncig[int(keep[5])] = 70000
    c.set_trim(bad)
    with pytest.raises(bam_native.AmpBamError) as e:
        c.encode(30, False)
    assert str(e.value) == "write: invalid argument"
    c.close()


def test_block_that_does_not_fit_goes_through_the_host_and_is_counted(twin, tmp_path):
    from tools.e2e_legs import write_bam
    src = str(tmp_path / "a.bam")
    write_bam(src, synth.make_amplicon_batch(G, AMPS, 6000, seed=7), int(G.size))
    want, res = _oracle_results(src)
    host_path = str(tmp_path / "host.bam")
    payload = host_file(host_path, src, res, 30, False)
    out_path = str(tmp_path / "dev.bam")
    refusing = _zlib_deflater(refuse=(1,))
    stream, infos, st, hb = twin_run(twin, refusing, src, out_path, res, 1 << 30, 30, False)
    assert stream == payload and st["out_blocks_host"] == 1 and st["out_blocks_device"] == (len(payload) + BS - 1) // BS - 1
    check_blocks(out_path, hb, payload)
    check_readers(out_path, host_path)


def test_appending_framed_blocks_and_the_writer_without_a_file(tmp_path):
    """ampbam_writer_open_refs writes the header blocks of ampbam_writer_open; ampbam_writer_append_framed refuses while rows are
    pending."""
    src = _write_recs(str(tmp_path / "s.bam"), [bamio.Rec("r%d" % i, 0, 0, 10 + i, 60, [(0, 8)], -1, -1, 0, "ACGTACGT", bytes([30] * 8)) for i in range(20)])
    f = bam_native.BamFile(src)
    a = bam_native.BamWriter(str(tmp_path / "a.bam"), f.header_text, f, level=6)
    b = bam_native.BamWriter(str(tmp_path / "b.bam"), f.header_text, None, level=6, references=f.references)
    assert a.header_bytes == b.header_bytes
    b.append_framed(bam_device.bgzf_block(b""[:0] + b"\x24\0\0\0" + bytes(36)))
    b.append_framed(b"")
    batch, _ = f.decode(0, f.n_records, copy=True)
    a.write_batch(batch)                                        # 20 short records: pending, no whole block yet
    with pytest.raises(bam_native.AmpBamError):
        a.append_framed(bam_device.bgzf_block(b"x"))
    a.close(); b.close(); f.close()
    ra, rb = open(str(tmp_path / "a.bam"), "rb").read(), open(str(tmp_path / "b.bam"), "rb").read()
    assert ra[:a.header_bytes] == rb[:b.header_bytes] and rb.endswith(bam_native.BGZF_EOF)


def test_reencode_under_the_sanitizers(tmp_path):
    """tests/hostsim/bamout_fuzz.cpp: the twin as a program under -fsanitize=address,undefined (host code only), guard bytes behind
    every buffer of the encoder: random records, results and piece cuts, the stream against a plain serial re-encode."""
    exe = bam_device.build_twin(str(tmp_path / "bamout_fuzz"), sanitize=True, main_source=os.path.join(ROOT, "tests", "hostsim", "bamout_fuzz.cpp"))
    r = subprocess.run([exe, "60"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "files 60" in r.stdout and "mismatches 0" in r.stdout
