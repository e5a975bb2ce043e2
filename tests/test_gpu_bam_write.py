"""Trimmed BAM out of the device codec on the GPU (amp_bam_encode, amplipy_amd/csrc/amp_bamout.hip): the
device against its host twin, and AMPLIPY_GPU_BAM=1 AMPLIPY_GPU_BAM_WRITE=1 / run_amplipy(gpu_bam=True, gpu_bam_write=True)
against the switches off and against the host writer with AMPLIPY_GPU_DEFLATE=1."""
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

from amplipy_amd import bam_device, bam_native, bamio, lib, synth
from tests.test_bam_reencode_twin import BS, Results, _keep, check_readers, host_file
from tests.test_gpu_bam import G, PRIMERS, AMPS, files, read, run, seg_recs, write_packed, write_recs        # noqa: F401 (files: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_BYTES = 128                                      # what an encode brings down besides the blocks: its sixteen counters


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


# ---- device = twin ------------------------------------------------------------------------------------------------------------------------
def test_device_stream_blocks_and_info_equal_the_twins(tmp_path):
    from amplipy_amd import build
    hb = synth.make_config5_batch(G, AMPS, rep=11, pool_reads=20000)                # 220,000 reads of the config-5 mix
    path = write_packed(str(tmp_path / "big.bam"), hb)
    whole = bam_native.BamFile(path)
    assert whole.n_records >= 200000
    want, _ = whole.decode(0, whole.n_records, copy=True)
    whole.close()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libampdf_hostsim.so")                                      # the encoder's host phases: the twin's DEFLATE
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                           "-o", so, os.path.join(build.CSRC, "amp_deflate.hip")])
    sim = C.CDLL(so)
    twin_so = bam_device.build_twin(str(tmp_path / "libampbgzf_twin.so"))
    mn, mx, mpl = lib.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0)
    eng = lib.Engine(G.size)
    eng.set_primers(mn, mx, mpl)
    eng.set_params(20, 4, True, False)
    t = eng.process(want)                                                           # the results of every row, for the twin
    assert not t.status.any()
    res = Results.of_trim(want, t)
    n_kept = int(_keep(res, 30, False, -1).sum())
    assert 0 < n_kept < want.n
    payload = host_file(str(tmp_path / "host.bam"), path, res, 30, False)
    dev = bam_device.BamCodec(eng); twin = bam_device.BamCodec(twin=twin_so)
    twin.set_deflater(C.cast(sim.ampdf_hostsim_blocks, C.c_void_p))
    fields = [f for f, _ in bam_device.AmpBamOutInfo._fields_]
    for piece_bytes in (256 << 10, 1 << 20, 1 << 30):
        src_d = bam_device.DeviceBamInput(path, piece_bytes); src_t = bam_device.DeviceBamInput(path, piece_bytes)
        lo = rows = n_blocks = 0
        stream, framed = [], []

        def both(final):
            nonlocal rows, n_blocks
            (db, di), (tb, ti) = dev.encode(30, False, final), twin.encode(30, False, final)
            assert [getattr(di, f) for f in fields] == [getattr(ti, f) for f in fields]
            assert di.waits == 1 and di.n_blocks_host == 0
            assert np.array_equal(db, tb)
            ds, ts = dev.stream(), twin.stream()
            assert np.array_equal(ds, ts)
            stream.append(ds[int(di.carry_in):].tobytes()); framed.append(db.tobytes())
            rows += int(di.n_rows_written); n_blocks += int(di.n_blocks)
            return di
        n_pieces = len(src_d.pieces)
        for k, ((di, sd), (ti, st)) in enumerate(zip(bam_device.walk(dev, src_d), bam_device.walk(twin, src_t))):
            assert di.n_rows == ti.n_rows and di.n_rows > 0
            assert dev.process(lo)[0] == -1
            b = twin.batch()
            twin.set_trim(res.rows(b, lo, lo + b.n))
            lo += b.n
            both(final=k + 1 == n_pieces and piece_bytes == 1 << 20)
        if piece_bytes != 1 << 20:
            last = both(final=True)                                                  # the bare flush
            assert last.n_rows_written == 0
        assert b"".join(stream) == payload and rows == n_kept
        assert n_blocks == (len(payload) + BS - 1) // BS
        assert inflate_all(b"".join(framed)) == payload
        assert twin.guards_ok()
    dev.close(); twin.close(); eng.close()


# ---- the sub-commands through the command line -------------------------------------------------------------------------------------------
MODES = {"off": {}, "deflate": {"AMPLIPY_GPU_DEFLATE": "1"}, "on": {"AMPLIPY_GPU_BAM": "1", "AMPLIPY_GPU_BAM_WRITE": "1"},
         "write_only": {"AMPLIPY_GPU_BAM_WRITE": "1"}}


def cli(cwd, args, mode):
    env = dict(os.environ)
    for k in ("AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env["AMPLIPY_GPU_BAM_PIECE_BYTES"] = str(512 << 10)
    env.update(MODES[mode])
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([sys.executable, "-m", "amplipy_amd"] + args, cwd=cwd, env=env, capture_output=True, timeout=900)


def log(r):          # the log lines without their time stamps and without the codec's own line
    return [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[") and b"BAM device codec" not in l]


def test_trim_and_aio_on_against_off_and_against_the_device_deflate(tmp_path, files):
    """Both switches on against both off: the inflated trimmed BAM (header included), VCF, FASTA and log are identical.  Against the
    host writer with AMPLIPY_GPU_DEFLATE=1 the file itself is: the same chunks through the same deterministic encoder."""
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 80000, seed=7))
    out = {}
    for mode in ("off", "deflate", "on"):
        d = str(tmp_path / mode)
        t = cli(d, ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.bam"], mode)
        a = cli(d, ["aio", "-i", inp, "-p", bed, "-r", ref, "-ot", "a.bam", "-ov", "a.vcf", "-oc", "a.fas"], mode)
        assert t.returncode == 0 and a.returncode == 0, (t.stderr[-2000:], a.stderr[-2000:])
        out[mode] = [read(os.path.join(d, k)) for k in ("t.bam", "a.bam", "a.vcf", "a.fas")] + [log(t), log(a), t.stderr, a.stderr]
    for k in (0, 1):
        assert inflate_all(out["on"][k]) == inflate_all(out["off"][k]) and len(out["on"][k]) > 100000
        assert out["on"][k] == out["deflate"][k], k                                 # the whole file, byte for byte
    for k in (2, 3, 4, 5):
        assert out["on"][k] == out["off"][k], k
    assert len(out["on"][2]) > 500 and len(out["on"][3]) > G.size
    for k in (6, 7):
        assert out["on"][k].count(b"blocks on the device, 0 through the host codec") == 2      # input blocks, and the trimmed reads'
        assert b"this run writes trimmed reads" not in out["on"][k] and b"BAM device codec" not in out["off"][k]
    check_readers(str(tmp_path / "on" / "t.bam"), str(tmp_path / "off" / "t.bam"))
    # the new switch without the BAM-input switch: the host run, byte for byte
    w = cli(str(tmp_path / "write_only"), ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.bam"], "write_only")
    assert w.returncode == 0 and read(str(tmp_path / "write_only" / "t.bam")) == out["off"][0]
    assert log(w) == out["off"][4] and b"BAM device codec" not in w.stderr


def test_config5_reads_with_aux_fields_on_against_off(tmp_path, files):
    ref, bed = files
    inp = write_recs(str(tmp_path / "in.bam"), seg_recs(synth.make_mixed_segments(G, AMPS, 9000, 61)))
    out = {}
    for mode in ("off", "on"):
        d = str(tmp_path / mode)
        a = cli(d, ["aio", "-i", inp, "-p", bed, "-r", ref, "-ot", "a.bam", "-ov", "a.vcf", "-oc", "a.fas", "-mfv", "0.01"], mode)
        assert a.returncode == 0, a.stderr[-2000:]
        out[mode] = [read(os.path.join(d, k)) for k in ("a.bam", "a.vcf", "a.fas")] + [log(a)]
    assert inflate_all(out["on"][0]) == inflate_all(out["off"][0]) and len(out["on"][0]) > 100000
    assert out["on"][1:] == out["off"][1:]


# ---- stats, round trip ---------------------------------------------------------------------------------------------------------------------
def test_stats_and_round_trip(tmp_path, files, monkeypatch):
    """Only compressed bytes cross the link: bytes_up within the input file and its block table, bytes_down within the output file
    and the counters of each encode, no block through the host on either side, at most two waits per piece.  The file is then
    read back by the device codec with every block on the device."""
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 60000, seed=10))
    trimmed = str(tmp_path / "t.bam")
    monkeypatch.delenv("AMPLIPY_GPU_BAM_WRITE", raising=False)
    st = run(monkeypatch, True, 256 << 10, gpu_bam_write=True, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=trimmed,
             primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=False, run_trim=True)
    n_in = len(bam_device.block_table(inp))
    size = os.path.getsize(trimmed)
    assert st["pieces"] > 3 and st["blocks_host"] == 0 and st["blocks_device"] == n_in
    assert st["out_blocks_host"] == 0 and st["out_blocks_device"] == len(bam_device.block_table(trimmed)) - 2      # (header block, end-of-file block)
    assert st["bytes_up"] <= os.path.getsize(inp) + 20 * n_in
    assert st["bytes_out_file"] < size and st["bytes_down"] <= size + INFO_BYTES * (st["pieces"] + 1)
    assert st["waits"] <= 2 * st["pieces"]
    assert st["out_rows"] == bam_native.BamFile(trimmed).n_records > 20000
    kw = dict(trimmed_reads_fn=trimmed, reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
    run(monkeypatch, False, variants_fn=str(tmp_path / "off.vcf"), **kw)
    st = run(monkeypatch, True, 256 << 10, variants_fn=str(tmp_path / "on.vcf"), **kw)
    assert st["blocks_host"] == 0 and st["blocks_device"] == len(bam_device.block_table(trimmed)) and st["waits"] == st["pieces"]
    assert read(str(tmp_path / "off.vcf")) == read(str(tmp_path / "on.vcf"))
    gc.collect()


# ---- exceptions ------------------------------------------------------------------------------------------------------------------------------
def test_failing_read_and_empty_file_end_like_the_host_path(tmp_path, files):
    """A read the loop fails on: the same exception, and the same file -- header blocks and the whole blocks of the rows in front
    of it, no end-of-file block (the host path does not close its writer either).  An empty input: the same NameError, and the
    file of header blocks and end-of-file block."""
    ref, bed = files
    recs = seg_recs(synth.make_mixed_segments(G, AMPS, 3000, 71))
    r = recs[1700]
    recs[1700] = bamio.Rec(r.qname, 0, 0, r.pos, 60, [(0, 10)], -1, -1, 0, None, None)      # a CIGAR and no bases: the loop fails on it (A:702)
    bad = write_recs(str(tmp_path / "bad.bam"), recs)
    empty = write_recs(str(tmp_path / "empty.bam"), [])
    got = {}
    for mode in ("off", "deflate", "on"):
        d = str(tmp_path / mode)
        b = cli(d, ["trim", "-i", bad, "-p", bed, "-r", ref, "-o", "b.bam"], mode)
        e = cli(d, ["trim", "-i", empty, "-p", bed, "-r", ref, "-o", "e.bam"], mode)
        assert b.returncode != 0 and e.returncode != 0
        got[mode] = (read(os.path.join(d, "b.bam")), read(os.path.join(d, "e.bam")), b.stderr.splitlines()[-1], e.stderr.splitlines()[-1], log(b), log(e))
    assert got["on"][2] == got["off"][2] and b"AmpBamError" not in got["on"][2] and got["on"][3] == got["off"][3] and b"NameError" in got["on"][3]
    assert got["on"][4] == got["off"][4] and got["on"][5] == got["off"][5]
    assert inflate_all(got["on"][0]) == inflate_all(got["off"][0]) and len(inflate_all(got["on"][0])) > 3 * BS
    assert got["on"][0] == got["deflate"][0] and not got["on"][0].endswith(bam_native.BGZF_EOF)
    assert got["on"][1] == got["off"][1] == got["deflate"][1] and got["on"][1].endswith(bam_native.BGZF_EOF)
