"""SAM text in, trimmed BAM out on the GPU (amp_sam_encode, amplipy_amd/csrc/amp_sam.hip): the device against
its host twin, and AMPLIPY_GPU_SAM=1 AMPLIPY_GPU_BAM_WRITE=1 / run_amplipy(gpu_sam=True, gpu_bam_write=True) against both switches
off -- the Python codec of bamio."""
import ctypes as C
import gc
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, bam_native, bamio, lib, sam_native, synth
from tests import sam_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = U.header(G.size)
BS = 0xFF00
INFO_BYTES = 128                                      # what an encode brings down besides the blocks: its sixteen counters
N_LINES = 20000
CHUNKS = {"64k": 64 << 10, "1m": 1 << 20, "unset": None}


def inflate_all(raw):
    """The inflated bytes of the BGZF blocks of ``raw`` (a file, or one that ends without an end-of-file block), CRC checked."""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        data = zlib.decompress(raw[at + 18:at + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        assert len(data) == isize and (zlib.crc32(data) & 0xFFFFFFFF) == crc
        out.append(data)
        at += bsize
    return b"".join(out)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def make_lines(n, seed):
    """n SAM lines of 75 to 600 bases: amplicon reads of five lengths, the config-5 mix, many-op CIGARs; AUX_POOL aux fields."""
    rng = np.random.default_rng(seed)
    segs = []
    for k, read_len in enumerate((75, 150, 250, 400, 600)):
        segs += synth.make_amplicon_batch(G, AMPS, n // 8, seed=seed + k, read_len=read_len).segments()
    segs += [s for s in synth.make_mixed_segments(G, AMPS, n // 4, seed + 7) if 75 <= len(s.query_sequence) <= 600]
    many = [s for s in U.many_op_segments(rng, n, G.size, max_len=600) if len(s.query_sequence) >= 75]
    segs += many[:n - len(segs)]
    assert len(segs) == n
    lines = U.segments_to_lines(segs, HDR, rng, max_aux=4)
    return [lines[i] for i in rng.permutation(n)]


def write_sam(path, lines, hdr=HDR):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(hdr.text.encode()); f.write(b"".join(lines))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sambam")
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(G) + "\n")
    bed = d / "p.bed"; bed.write_text("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(PRIMERS)))
    lines = make_lines(N_LINES, 301)
    return str(ref), str(bed), lines, write_sam(d / "in.sam", lines)


# ---- device = twin ------------------------------------------------------------------------------------------------------------------------
def test_device_stream_blocks_and_info_equal_the_twins(tmp_path, files):
    """Stream, framed bytes and info at three chunk sizes; a chunk costs the device two waits -- the parse's and the encode's, which
    brings the verdict of the deferred read pass down as well (the copy of the framed blocks, asked for once their size is known, is
    the caller's third, as in section 12)."""
    from amplipy_amd import build
    ref, bed, lines, path = files
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libampdf_hostsim.so")                                      # the encoder's host phases: the twin's DEFLATE
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                           "-o", so, os.path.join(build.CSRC, "amp_deflate.hip")])
    sim = C.CDLL(so)
    mn, mx, mpl = lib.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0)
    eng = lib.Engine(G.size)
    eng.set_primers(mn, mx, mpl)
    eng.set_params(20, 4, True, False)
    dev = sam_native.SamCodec(eng); twin = sam_native.SamCodec(twin=U.twin_path(tmp_path))
    for c in (dev, twin):
        c.set_references(U.ref_names(HDR)); c.set_output(sam_native.OUT_BAM)
    twin.set_deflater(C.cast(sim.ampdf_hostsim_blocks, C.c_void_p))
    fields = [f for f, _ in bam_device.AmpBamOutInfo._fields_]
    streams = []
    for chunk_bytes in (64 << 10, 1 << 20, sam_native.CHUNK_BYTES):
        src = sam_native.SamTextInput(path, chunk_bytes)
        chunks = list(src)
        src.close()
        lo = rows = n_blocks = 0
        stream, framed = [], []

        def both(final, encode):
            nonlocal rows, n_blocks
            (db, di), (tb, ti) = encode(dev, final), encode(twin, final)
            assert [getattr(di, f) for f in fields] == [getattr(ti, f) for f in fields]
            assert di.waits == 1 and di.n_blocks_host == 0
            assert np.array_equal(db, tb)
            ds, ts = dev.stream(), twin.stream()
            assert np.array_equal(ds, ts)
            stream.append(ds[int(di.carry_in):].tobytes()); framed.append(db.tobytes())
            rows += int(di.n_rows_written); n_blocks += int(di.n_blocks)
            return di
        for k, chunk in enumerate(chunks):
            w0 = dev.waits()
            di = dev.parse(chunk)
            dev.process(lo, defer=True)
            final = k + 1 == len(chunks) and chunk_bytes == 1 << 20
            info = bam_device.AmpBamOutInfo()
            assert dev.L.amp_sam_encode(dev.h, C.c_int32(30), C.c_int32(1), C.c_int32(1 if final else 0), C.byref(info)) == 0
            assert dev.waits() - w0 == 2 and info.waits == 1                        # parse, encode; the read pass waits for nothing
            assert dev.verdict() == (-1, 0) and dev.waits() - w0 == 2               # (the verdict came down with the encode)
            ti = twin.parse(chunk)
            names = [f for f, _ in di._fields_]
            assert [getattr(di, f) for f in names] == [getattr(ti, f) for f in names] and di.first_odd_line == -1 and di.n_rows > 0
            res = eng.process(dev.batch())                                          # the same rows through the host-pointer entry, for the twin
            assert twin.twin_set_results(res) == (-1, 0)
            lo += int(di.n_rows)
            both(final, lambda c, f: (c._encoded(info) if c is dev else c.encode(30, True, f)))
        if chunk_bytes != 1 << 20:
            last = both(True, lambda c, f: c.encode_bytes(b"", f))                   # the bare flush
            assert last.n_rows_written == 0
        payload = b"".join(stream)
        streams.append(payload)
        assert n_blocks == (len(payload) + BS - 1) // BS > 90 and rows > N_LINES // 2
        assert inflate_all(b"".join(framed)) == payload
        assert twin.guards_ok()
        assert len(chunks) == 1 if chunk_bytes == sam_native.CHUNK_BYTES else len(chunks) > 5
    assert streams[0] == streams[1] == streams[2]
    dev.close(); twin.close(); eng.close()


# ---- the sub-commands through the command line -------------------------------------------------------------------------------------------
MODES = {"off": {}, "on": {"AMPLIPY_GPU_SAM": "1", "AMPLIPY_GPU_BAM_WRITE": "1"}, "sam_only": {"AMPLIPY_GPU_SAM": "1"},
         "write_only": {"AMPLIPY_GPU_BAM_WRITE": "1"}}


def cli(cwd, args, mode, stdin_path=None, chunk=None):
    env = dict(os.environ)
    for k in ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_SAM_CHUNK_BYTES"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    if chunk:
        env["AMPLIPY_SAM_CHUNK_BYTES"] = str(chunk)
    env.update(MODES[mode])
    os.makedirs(cwd, exist_ok=True)
    with open(stdin_path or os.devnull, "rb") as f:
        return subprocess.run([sys.executable, "-m", "amplipy_amd"] + args, cwd=cwd, env=env, stdin=f, capture_output=True, timeout=900)


def log(r):          # the log lines without their time stamps and without the codec's own line
    return [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[") and b"SAM text codec" not in l]


def codec_line(r):
    """(device chunks, python chunks, out blocks on the device, through the host, bytes down) of the codec's log line."""
    import re
    m = re.search(rb"SAM text codec: (\d+) chunks on the device, (\d+) through the Python codec; trimmed reads went out as BAM blocks from the "
                  rb"device: (\d+) blocks on the device, (\d+) through the host, (\d+) bytes down", r.stderr)
    assert m, r.stderr[-2000:]
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("command,source,chunk", [("trim", "file", "64k"), ("trim", "pipe", "1m"), ("aio", "file", "unset"), ("aio", "pipe", "64k"),
                                                  ("trim", "file", "1m")])
def test_trim_and_aio_on_against_off(tmp_path, files, command, source, chunk):
    """Both switches on against both off: the BAMs inflate to the same bytes (header and records), VCF, FASTA and log are identical;
    every chunk on the device, no output block through the host, bytes down within the file's size and 128 bytes per encode."""
    ref, bed, lines, inp = files
    args = ([] if source == "pipe" else ["-i", inp]) + ["-p", bed, "-r", ref]
    args = ["trim"] + args + ["-e", "-o", "t.bam"] if command == "trim" else ["aio"] + args + ["-e", "-ot", "t.bam", "-ov", "a.vcf", "-oc", "a.fas"]
    out = {}
    for mode in ("off", "on"):
        d = str(tmp_path / mode)
        r = cli(d, args, mode, inp if source == "pipe" else None, CHUNKS[chunk])
        assert r.returncode == 0, r.stderr[-2000:]
        out[mode] = r, read(os.path.join(d, "t.bam"))
        if command == "aio":
            out[mode] += (read(os.path.join(d, "a.vcf")), read(os.path.join(d, "a.fas")))
    assert inflate_all(out["on"][1]) == inflate_all(out["off"][1]) and len(inflate_all(out["on"][1])) > 90 * BS
    assert out["on"][2:] == out["off"][2:] and (command == "trim" or (len(out["on"][2]) > 500 and len(out["on"][3]) > G.size))
    assert log(out["on"][0]) == log(out["off"][0]) and b"SAM text codec" not in out["off"][0].stderr
    dev_chunks, py_chunks, blocks_dev, blocks_host, down = codec_line(out["on"][0])
    assert dev_chunks > 0 and py_chunks == 0 and blocks_host == 0
    size = len(out["on"][1])
    assert blocks_dev == len(bam_device.block_table(str(tmp_path / "on" / "t.bam"))) - 2 > 90          # (header block, end-of-file block)
    assert down <= size + INFO_BYTES * (dev_chunks + 1)
    total = len(b"".join(lines))
    assert dev_chunks == 1 if chunk == "unset" else total // CHUNKS[chunk] <= dev_chunks <= total // CHUNKS[chunk] + 2
    # the file reads back through both host readers like the Python codec's
    a, b = bam_native.BamFile(str(tmp_path / "on" / "t.bam")), bam_native.BamFile(str(tmp_path / "off" / "t.bam"))
    assert a.n_records == b.n_records > N_LINES // 2 and a.header_text == b.header_text and a.references == b.references
    ba, _ = a.decode(0, a.n_records, copy=True); bb, _ = b.decode(0, b.n_records, copy=True)
    for name in ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual"):
        assert np.array_equal(getattr(ba, name), getattr(bb, name)), name
    a.close(); b.close()
    ra = [(r.qname, r.flag, r.pos, r.cigar, r.seq, bamio.aux_bam_to_sam(r.aux_bam)) for r in bamio.AlignmentReader(str(tmp_path / "on" / "t.bam"), "rb")]
    rb = [(r.qname, r.flag, r.pos, r.cigar, r.seq, bamio.aux_bam_to_sam(r.aux_bam)) for r in bamio.AlignmentReader(str(tmp_path / "off" / "t.bam"), "rb")]
    assert ra == rb


def run(monkeypatch, on, chunk_bytes=None, **kw):
    """run_amplipy with sys.argv pinned (the @PG line and the VCF header record it) and both switches on or off."""
    from amplipy_amd import amplipy
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    for k in ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE"):
        monkeypatch.delenv(k, raising=False)
    if chunk_bytes:
        monkeypatch.setenv("AMPLIPY_SAM_CHUNK_BYTES", str(chunk_bytes))
    sam_native.LAST_RUN_STATS.update(device_chunks=-1, python_chunks=-1, records=-1)
    amplipy.run_amplipy(gpu_sam=on, gpu_bam_write=on, **kw)
    return dict(sam_native.LAST_RUN_STATS)


def test_stats_and_the_device_bam_reader(tmp_path, files, monkeypatch):
    """LAST_RUN_STATS of a run, and the file through the device BAM reader of section 11 with every block on the device."""
    ref, bed, lines, inp = files
    trimmed = str(tmp_path / "t.bam")
    st = run(monkeypatch, True, 256 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=trimmed, primer_pos_offset=0,
             min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=True, run_trim=True)
    size = os.path.getsize(trimmed)
    assert st["device_chunks"] > 20 and st["python_chunks"] == 0 and st["records"] == N_LINES
    assert st["out_blocks_host"] == 0 and st["out_blocks_device"] == len(bam_device.block_table(trimmed)) - 2 > 90
    assert st["encodes"] == st["device_chunks"] + 1 == st["waits"]
    assert st["bytes_out_file"] < size and st["bytes_down"] <= size + INFO_BYTES * st["encodes"]
    assert st["out_rows"] == bam_native.BamFile(trimmed).n_records > N_LINES // 2
    kw = dict(trimmed_reads_fn=trimmed, reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
    from amplipy_amd import amplipy
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    amplipy.run_amplipy(variants_fn=str(tmp_path / "off.vcf"), gpu_bam=False, **kw)
    amplipy.run_amplipy(variants_fn=str(tmp_path / "on.vcf"), gpu_bam=True, **kw)
    bst = dict(bam_device.LAST_RUN_STATS)
    assert bst["blocks_host"] == 0 and bst["blocks_device"] == len(bam_device.block_table(trimmed))
    assert read(str(tmp_path / "off.vcf")) == read(str(tmp_path / "on.vcf")) and len(read(str(tmp_path / "on.vcf"))) > 500
    gc.collect()


# ---- a chunk for the Python codec ------------------------------------------------------------------------------------------------------------
def test_one_out_of_set_float_goes_through_the_python_codec(tmp_path, files, monkeypatch):
    ref, bed, lines, _ = files
    lines = list(lines[:3000])
    size = np.cumsum([len(l) for l in lines])
    k = int(np.searchsorted(size, 2 * (64 << 10) + 10000))                 # a line well inside the third chunk of 64 KB ...
    while not (lines[k].split(b"\t")[5].endswith(b"M") and lines[k].split(b"\t")[5][:-1].isdigit() and len(lines[k].split(b"\t")[9]) >= 150):
        k += 1                                                              # ... of a read that is kept: one long match
    assert size[k] < 3 * (64 << 10) - 2000
    lines[k] = lines[k][:-1] + b"\tXF:f:1e23\n"
    inp = write_sam(tmp_path / "in.sam", lines)
    outs = {}
    for on in (False, True):
        o = {x: str(tmp_path / ("%d_%s" % (on, x))) for x in ("t.bam", "v.vcf", "c.fas")}
        st = run(monkeypatch, on, 64 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=o["t.bam"], variants_fn=o["v.vcf"],
                 consensus_fn=o["c.fas"], primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, min_freq_consensus=0.5,
                 min_freq_variants=0.03, min_depth_consensus=10, min_depth_variants=1, unknown_symbol="N", include_no_primer=True,
                 run_trim=True, run_variants=True, run_consensus=True)
        outs[on] = o
        if on:
            assert st["python_chunks"] == 1 and st["device_chunks"] > 10 and st["records"] == 3000 and st["out_blocks_host"] == 0, st
            assert st["encodes"] == st["device_chunks"] + 2                 # the chunks, the Python chunk's records, the flush
    assert inflate_all(read(outs[True]["t.bam"])) == inflate_all(read(outs[False]["t.bam"]))
    assert struct.pack("<f", 1e23) in inflate_all(read(outs[True]["t.bam"]))
    for x in ("v.vcf", "c.fas"):
        assert read(outs[False][x]) == read(outs[True][x]), x


# ---- exceptions ------------------------------------------------------------------------------------------------------------------------------
def test_failing_read_empty_input_and_header_without_pg(tmp_path, files):
    """A read the loop fails on: the same exception as with the switches off, and a file whose inflated bytes are a prefix of the
    header and the records of the rows in front of it, no end-of-file block.  An empty input and a header without @PG behave as
    with the switches off."""
    ref, bed, lines, _ = files
    lines = list(lines[:3000])
    size = np.cumsum([len(l) for l in lines])
    k = int(np.searchsorted(size, 9 * (64 << 10) + 30000))                 # inside the tenth chunk
    f = lines[k].split(b"\t"); f[10] = b"*"; bad_line = b"\t".join(f[:11]) + b"\n"         # QUAL '*' with trimming on: TypeError
    args = ["trim", "-i", "in.sam", "-p", bed, "-r", ref, "-e", "-o", "t.bam"]
    cases = {"bad": (lines[:k] + [bad_line] + lines[k + 1:], HDR), "front": (lines[:k], HDR), "empty": ([], HDR), "nopg": (lines[:50], U.header(G.size, pg=False))}
    got = {}
    for name, (ls, hdr) in cases.items():
        for mode in ("off", "on"):
            d = str(tmp_path / name / mode)
            write_sam(os.path.join(d, "in.sam"), ls, hdr)
            r = cli(d, args, mode, chunk=64 << 10)
            p = os.path.join(d, "t.bam")
            got[name, mode] = (r.returncode, r.stderr.splitlines()[-1], log(r), read(p) if os.path.exists(p) else None)
    for name in ("bad", "empty", "nopg"):
        assert got[name, "on"][:3] == got[name, "off"][:3], name
    assert got["bad", "on"][0] != 0 and b"TypeError" in got["bad", "on"][1]
    assert got["front", "on"][0] == 0 and inflate_all(got["front", "on"][3]) == inflate_all(got["front", "off"][3])
    whole, part = inflate_all(got["front", "on"][3]), inflate_all(got["bad", "on"][3])
    n_hdr = len(inflate_all(got["nopg", "on"][3] or got["empty", "on"][3][:-len(bam_native.BGZF_EOF)]))      # the header has a block of its own
    assert whole.startswith(part) and len(part) == n_hdr + (len(whole) - n_hdr) // BS * BS > 4 * BS       # the whole blocks of the rows in front
    assert not got["bad", "on"][3].endswith(bam_native.BGZF_EOF)
    assert whole.startswith(inflate_all(got["bad", "off"][3]))
    assert got["empty", "on"][0] != 0 and got["empty", "on"][3] is not None and got["empty", "off"][3] is not None
    assert inflate_all(got["empty", "on"][3]) == inflate_all(got["empty", "off"][3])
    assert b"KeyError" in got["nopg", "on"][1] and got["nopg", "on"][3] is None and got["nopg", "off"][3] is None


def test_either_switch_alone_changes_nothing(tmp_path, files):
    """AMPLIPY_GPU_SAM=1 alone and AMPLIPY_GPU_BAM_WRITE=1 alone: the Python codec's file, byte for byte, and its log lines."""
    ref, bed, lines, _ = files
    inp = write_sam(tmp_path / "in.sam", lines[:2000])
    args = ["trim", "-i", inp, "-p", bed, "-r", ref, "-e", "-o", "t.bam"]
    out = {}
    for mode in ("off", "sam_only", "write_only"):
        r = cli(str(tmp_path / mode), args, mode)
        assert r.returncode == 0, r.stderr[-2000:]
        out[mode] = read(str(tmp_path / mode / "t.bam")), [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[")]
    assert out["sam_only"] == out["off"] and out["write_only"] == out["off"] and len(out["off"][0]) > 100000
