"""The opt-in device codec for BAM input on the GPU: amp_bam_* (amplipy_amd/csrc/amp_bgzf.hip) against its host twin and libampbam,
and AMPLIPY_GPU_BAM=1 / run_amplipy(gpu_bam=True) against the switch off: byte-identical outputs, the same exceptions."""
import gc
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, bam_native, bamio, synth
from tests.bam_util import _bgzf, _blocks_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % G.size, [("SYN_REF", int(G.size))])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamfiles")
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(G) + "\n")
    bed = d / "p.bed"; bed.write_text("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(PRIMERS)))
    return str(ref), str(bed)


def write_packed(path, batch, level=6):
    """A BAM file of the rows of a packed batch, written by libampbam (ampbam_write_batch)."""
    seed = path + ".seed.bam"
    w = bamio.AlignmentWriter(seed, "wb", HDR)
    w.close()
    like = bam_native.BamFile(seed)
    w = bam_native.BamWriter(path, like.header_text, like, level=level)
    w.write_batch(batch)
    w.close(); like.close()
    os.remove(seed)
    return path


def write_recs(path, recs):
    w = bamio.AlignmentWriter(path, "wb", HDR)
    for r in recs:
        w.write(r)
    w.close()
    return path


def seg_recs(segs):
    return [bamio.Rec("r%d" % i, s.flag, 0, s.reference_start, 60, s.cigartuples, 0, s.reference_start, s.template_length, s.query_sequence,
                      bytes(s.query_qualities), aux_sam=["NM:i:%d" % (i % 5)]) for i, s in enumerate(segs)]


def run(monkeypatch, on, piece_bytes=None, **kw):
    """run_amplipy with sys.argv pinned (the VCF header records it) and the switch on or off: LAST_RUN_STATS afterwards."""
    from amplipy_amd import amplipy
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    monkeypatch.delenv("AMPLIPY_GPU_BAM", raising=False)
    if piece_bytes:
        monkeypatch.setenv("AMPLIPY_GPU_BAM_PIECE_BYTES", str(piece_bytes))
    bam_device.LAST_RUN_STATS.update(pieces=-1, blocks_device=-1, blocks_host=-1, index_rounds=-1, waits=-1, records=-1)
    amplipy.run_amplipy(gpu_bam=on, **kw)
    return dict(bam_device.LAST_RUN_STATS)


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- device = twin = libampbam ------------------------------------------------------------------------------------------------------------
def test_device_image_and_batch_equal_twin_and_libampbam(tmp_path):
    from amplipy_amd import lib
    hb = synth.make_config5_batch(G, AMPS, rep=11, pool_reads=20000)                # 220,000 reads of the config-5 mix
    path = write_packed(str(tmp_path / "big.bam"), hb)
    whole = bam_native.BamFile(path)                                                 # ampbam_open
    assert whole.n_records >= 200000
    want, _ = whole.decode(0, whole.n_records)
    image = b"".join(zlib.decompress(raw, -15) for raw, _, _ in _blocks_of(path))    # what libampbam inflates
    twin_so = bam_device.build_twin(str(tmp_path / "libampbgzf_twin.so"))
    eng = lib.Engine(G.size)
    dev = bam_device.BamCodec(eng); twin = bam_device.BamCodec(twin=twin_so)
    for piece_bytes in (256 << 10, 1 << 20, 1 << 30):
        src_d = bam_device.DeviceBamInput(path, piece_bytes); src_t = bam_device.DeviceBamInput(path, piece_bytes)
        rows = at = n_pieces = 0
        sd = st = None
        for (di, sd), (ti, st) in zip(bam_device.walk(dev, src_d), bam_device.walk(twin, src_t)):
            fields = [f for f, _ in di._fields_ if f != "waits"]
            assert [getattr(di, f) for f in fields] == [getattr(ti, f) for f in fields]
            assert di.waits == 1                                                     # counts and verdicts together: one wait per piece
            dimg, doff = dev.image(); timg, toff = twin.image()
            assert np.array_equal(dimg, timg) and np.array_equal(doff, toff)
            fresh = dimg[int(di.carry_in):].tobytes()
            assert fresh == image[at:at + len(fresh)]
            at += len(fresh)
            (db, dtails), (tb, ttails) = dev.batch(slack=True), twin.batch(slack=True)
            for a, b in zip(dtails, ttails):
                assert np.array_equal(a, b) and not a.any()
            lo, hi = rows, rows + db.n
            c0, s0 = int(want.cig_off[lo]), int(want.seq_off[lo])
            for name in ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual", "src_index"):
                assert np.array_equal(getattr(db, name), getattr(tb, name)), name
            assert np.array_equal(db.pos, want.pos[lo:hi]) and np.array_equal(db.flag, want.flag[lo:hi]) and np.array_equal(db.tlen, want.tlen[lo:hi])
            assert np.array_equal(db.lseq, want.lseq[lo:hi]) and np.array_equal(db.src_index, want.src_index[lo:hi])
            assert np.array_equal(db.cig_off, want.cig_off[lo:hi + 1] - np.uint64(c0)) and np.array_equal(db.cig, want.cig[c0:int(want.cig_off[hi])])
            assert np.array_equal(db.seq_off, want.seq_off[lo:hi + 1] - np.uint64(s0))
            assert np.array_equal(db.seq, want.seq[s0 // 2:int(want.seq_off[hi]) // 2]) and np.array_equal(db.qual, want.qual[s0:int(want.seq_off[hi])])
            rows = hi; n_pieces += 1
        assert rows == want.n and at == len(image)
        assert sd["blocks_host"] == 0 and st["blocks_host"] == 0 and sd["index_rounds"] == st["index_rounds"] and sd["records"] == whole.n_records
        assert sd["waits"] == sd["pieces"] == n_pieces
        assert sd["bytes_up"] <= os.path.getsize(path) + 20 * len(src_d.table)        # the compressed file and the block table, no more
        assert n_pieces == len(src_d.pieces) and (n_pieces == 1 if piece_bytes == 1 << 30 else n_pieces > 3)
    dev.close(); twin.close(); eng.close(); whole.close()


# ---- the sub-commands through the command line, switch on against off -------------------------------------------------------------------------
def cli(cwd, args, on, extra_env=None):
    env = dict(os.environ); env.pop("AMPLIPY_GPU_BAM", None)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env["AMPLIPY_GPU_BAM_PIECE_BYTES"] = str(512 << 10)
    if on:
        env["AMPLIPY_GPU_BAM"] = "1"
    env.update(extra_env or {})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([sys.executable, "-m", "amplipy_amd"] + args, cwd=cwd, env=env, capture_output=True, timeout=900)


def log(r):          # the log lines without their time stamps and without the codec's own line
    return [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[") and b"BAM device codec" not in l]


@pytest.mark.parametrize("which", ["amplicon", "config5"])
def test_variants_and_consensus_on_against_off(tmp_path, files, which):
    ref, bed = files
    if which == "amplicon":
        inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 120000, seed=7))
    else:
        inp = write_recs(str(tmp_path / "in.bam"), seg_recs(synth.make_mixed_segments(G, AMPS, 9000, 61)))
    n = bam_native.BamFile(inp).n_records
    out = {}
    for on in (False, True):
        d = str(tmp_path / ("on" if on else "off"))
        v = cli(d, ["variants", "-i", inp, "-r", ref, "-o", "v.vcf", "-mf", "0.01"], on)
        c = cli(d, ["consensus", "-i", inp, "-r", ref, "-o", "c.fas"], on)
        assert v.returncode == 0 and c.returncode == 0, (v.stderr[-2000:], c.stderr[-2000:])
        out[on] = (read(os.path.join(d, "v.vcf")), read(os.path.join(d, "c.fas")), log(v), log(c), v.stderr + c.stderr)
    assert out[True][0] == out[False][0] and len(out[True][0]) > 500
    assert out[True][1] == out[False][1] and len(out[True][1]) > G.size
    assert out[True][2] == out[False][2] and out[True][3] == out[False][3]
    assert any(l.startswith(b"Finished Processing %d reads" % (n - 1)) for l in out[True][2])
    assert out[True][4].count(b"blocks on the device, 0 through the host codec") == 2 and b"BAM device codec" not in out[False][4]


def test_trim_and_aio_keep_the_host_codec(tmp_path, files):
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 30000, seed=8))
    out = {}
    for on in (False, True):
        d = str(tmp_path / ("on" if on else "off"))
        t = cli(d, ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.bam"], on)
        a = cli(d, ["aio", "-i", inp, "-p", bed, "-r", ref, "-ot", "a.bam", "-ov", "a.vcf", "-oc", "a.fas"], on)
        assert t.returncode == 0 and a.returncode == 0, (t.stderr[-2000:], a.stderr[-2000:])
        out[on] = [read(os.path.join(d, k)) for k in ("t.bam", "a.bam", "a.vcf", "a.fas")] + [log(t), log(a), t.stderr, a.stderr]
    for k in range(6):
        assert out[True][k] == out[False][k], k
    assert len(out[True][0]) > 100000
    for k in (6, 7):
        assert out[True][k].count(b"BAM device codec: this run writes trimmed reads, the host codec reads the input") == 1
        assert b"BAM device codec" not in out[False][k]


# ---- exceptions ---------------------------------------------------------------------------------------------------------------------------------
def test_failing_read_and_empty_file_raise_what_the_host_path_raises(tmp_path, files, monkeypatch):
    ref, bed = files
    recs = seg_recs(synth.make_mixed_segments(G, AMPS, 3000, 71))
    r = recs[1700]
    recs[1700] = bamio.Rec(r.qname, 0, 0, r.pos, 60, [(0, 10)], -1, -1, 0, None, None)      # a CIGAR and no bases: the loop fails on it (A:702)
    bad = write_recs(str(tmp_path / "bad.bam"), recs)
    empty = write_recs(str(tmp_path / "empty.bam"), [])
    got = {}
    for on in (False, True):
        kw = dict(reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
        with pytest.raises(Exception) as ei:
            run(monkeypatch, on, 64 << 10, trimmed_reads_fn=bad, variants_fn=str(tmp_path / ("b%d.vcf" % on)), **kw)
        got[on] = (ei.type, str(ei.value))
        del ei
        with pytest.raises(NameError) as ei:
            run(monkeypatch, on, trimmed_reads_fn=empty, variants_fn=str(tmp_path / ("e%d.vcf" % on)), **kw)
        got[on, "empty"] = str(ei.value)
        del ei
        gc.collect()
    assert got[True] == got[False] and not issubclass(got[True][0], bam_native.AmpBamError)
    assert got[True, "empty"] == got[False, "empty"]


def test_damaged_files_raise_what_the_host_codec_raises(tmp_path, files, monkeypatch):
    """The fixed set the twin test proved safe under the sanitizers, each run once: a flipped payload bit, a wrong CRC, a wrong
    ISIZE, a file that ends inside a record, a record whose block_size is 5."""
    ref, bed = files
    good = write_recs(str(tmp_path / "good.bam"), seg_recs(synth.make_mixed_segments(G, AMPS, 3000, 81)))
    tab = bam_device.block_table(good)
    raw = read(good)
    o, n = int(tab[4, 0]), int(tab[4, 1])
    cases = {}
    for name, (at, mask) in {"bit": (o + n // 2, 0x10), "crc": (o + n + 1, 0x01), "isize": (o + n + 4, 0x01)}.items():
        b = bytearray(raw); b[at] ^= mask
        cases[name] = str(tmp_path / ("bad_%s.bam" % name))
        open(cases[name], "wb").write(bytes(b))
    image = b"".join(zlib.decompress(r, -15) for r, _, _ in _blocks_of(good))
    _, _, first = bam_device.read_header(good, tab)
    for name, img in (("cut", image[:len(image) - 7]), ("bs", image[:first] + struct.pack("<I", 5) + image[first + 4:])):
        cases[name] = str(tmp_path / ("bad_%s.bam" % name))
        with open(cases[name], "wb") as out:
            for a in range(0, len(img), 60000):
                out.write(_bgzf(img[a:a + 60000]))
            out.write(bam_native.BGZF_EOF)
    kw = dict(reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
    for name, path in cases.items():
        got = {}
        for on in (False, True):
            with pytest.raises(bam_native.AmpBamError) as ei:
                run(monkeypatch, on, 64 << 10, trimmed_reads_fn=path, variants_fn=str(tmp_path / ("%s%d.vcf" % (name, on))), **kw)
            got[on] = str(ei.value)
            del ei
            gc.collect()
        assert got[True] == got[False], name


# ---- the fallback, and the two device codecs together ------------------------------------------------------------------------------------------------
def test_refused_block_goes_through_the_host_and_is_counted(tmp_path, files, monkeypatch):
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 40000, seed=9))
    kw = dict(trimmed_reads_fn=inp, reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
    off = str(tmp_path / "off.vcf"); on = str(tmp_path / "on.vcf"); ref_on = str(tmp_path / "refused.vcf")
    run(monkeypatch, False, variants_fn=off, **kw)
    st = run(monkeypatch, True, 256 << 10, variants_fn=on, **kw)
    assert st["blocks_host"] == 0 and st["pieces"] > 3 and st["waits"] == st["pieces"]
    monkeypatch.setenv("AMPLIPY_DEV", "1"); monkeypatch.setenv("AMPLIPY_GPU_BAM_REFUSE_BLOCK", "7")
    st = run(monkeypatch, True, 256 << 10, variants_fn=ref_on, **kw)
    assert st["blocks_host"] == 1 and st["blocks_device"] == len(bam_device.block_table(inp)) - 1
    assert read(off) == read(on) == read(ref_on)


def test_round_trip_with_the_device_deflate(tmp_path, files, monkeypatch):
    """A trimmed BAM written with AMPLIPY_GPU_DEFLATE=1 is read back through the device codec: every block on the device."""
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 40000, seed=10))
    trimmed = str(tmp_path / "t.bam")
    monkeypatch.setenv("AMPLIPY_GPU_DEFLATE", "1")
    run(monkeypatch, False, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=trimmed, primer_pos_offset=0, min_length=30,
        min_quality=20, sliding_window_width=4, include_no_primer=False, run_trim=True)
    monkeypatch.delenv("AMPLIPY_GPU_DEFLATE")
    assert bam_native.BamFile(trimmed).n_records > 20000
    kw = dict(trimmed_reads_fn=trimmed, reference_fn=ref, min_quality=20, min_freq_variants=0.03, min_depth_variants=1, run_variants=True)
    run(monkeypatch, False, variants_fn=str(tmp_path / "off.vcf"), **kw)
    st = run(monkeypatch, True, 256 << 10, variants_fn=str(tmp_path / "on.vcf"), **kw)
    assert st["blocks_host"] == 0 and st["blocks_device"] == len(bam_device.block_table(trimmed)) and st["waits"] == st["pieces"]
    assert read(str(tmp_path / "off.vcf")) == read(str(tmp_path / "on.vcf"))
