"""BAM in, trimmed SAM text out on the GPU (amp_bam_text_check / amp_bam_format, amplipy_amd/csrc/amp_bamtext.hip; DESIGN.md section
14): the device against its host twin and the Python codec, and AMPLIPY_GPU_BAM=1 AMPLIPY_GPU_SAM=1 / run_amplipy(gpu_bam=True,
gpu_sam=True) against both switches off -- the Python codec of bamio."""
import gc
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from amplipy_amd import amplipy, bam_device, bam_native, bamio, lib, synth
from tests import sam_util as U
from tests.test_bam_reencode_twin import Results, _keep
from tests.test_bam_to_sam_twin import HDR, pool_recs, python_rows, python_text, write_raw
from tests.test_gpu_bam import G, PRIMERS, AMPS, HDR as PACKED_HDR, files, read, seg_recs, write_packed, write_recs        # noqa: F401 (files: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("AMPLIPY_GPU_BAM", "AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_PYTHON_BAM")
MODES = {"off": {}, "on": {"AMPLIPY_GPU_BAM": "1", "AMPLIPY_GPU_SAM": "1"}, "bam_only": {"AMPLIPY_GPU_BAM": "1"}, "sam_only": {"AMPLIPY_GPU_SAM": "1"}}
TEXT_LINE = b"trimmed reads as SAM text"
H = PACKED_HDR.text.count("\n") + 1                   # header lines of the trimmed text of a write_packed / write_recs file: its own and the new @PG


def mix_recs(n, seed):
    """n records of 75 to 600 bases: amplicon reads of five lengths, the config-5 mix, many-op CIGARs; AUX_POOL aux fields."""
    rng = np.random.default_rng(seed)
    segs = []
    for k, read_len in enumerate((75, 150, 250, 400, 600)):
        segs += synth.make_amplicon_batch(G, AMPS, n // 8, seed=seed + k, read_len=read_len).segments()
    segs += [s for s in synth.make_mixed_segments(G, AMPS, n // 4, seed + 7) if 75 <= len(s.query_sequence) <= 600]
    many = [s for s in U.many_op_segments(rng, n, G.size, max_len=600) if len(s.query_sequence) >= 75]
    segs += many[:n - len(segs)]
    assert len(segs) == n
    recs = pool_recs(segs, seed)
    return [recs[i] for i in rng.permutation(n)]


# ---- device = twin = the Python codec -----------------------------------------------------------------------------------------------------
def test_device_check_and_text_equal_the_twins_and_the_python_codecs(tmp_path):
    path = write_raw(str(tmp_path / "mix.bam"), mix_recs(20000, 401))
    whole = bam_native.BamFile(path)
    want, _ = whole.decode(0, whole.n_records, copy=True)
    whole.close()
    assert want.n == 20000
    twin_so = bam_device.build_twin(str(tmp_path / "libampbgzf_twin.so"))
    mn, mx, mpl = lib.find_overlapping_primers(G.size, [(s, e) for s, e, _ in PRIMERS], 0)
    eng = lib.Engine(G.size)
    eng.set_primers(mn, mx, mpl)
    eng.set_params(20, 4, True, False)
    t = eng.process(want)                                                           # the results of every row, for the twin
    assert not t.status.any()
    res = Results.of_trim(want, t)
    keep = _keep(res, 30, False, -1)
    assert 0 < int(keep.sum()) < want.n
    text = python_text(python_rows(path), res, keep)                                # AlignmentWriter.write of the kept rows
    dev = bam_device.BamCodec(eng); twin = bam_device.BamCodec(twin=twin_so)
    names = [n for n, _ in HDR.refs]
    dev.set_references(names); twin.set_references(names)
    fields = [f for f, _ in bam_device.AmpBamTextInfo._fields_]
    for piece_bytes in (64 << 10, 1 << 20, 1 << 30):
        src_d = bam_device.DeviceBamInput(path, piece_bytes); src_t = bam_device.DeviceBamInput(path, piece_bytes)
        lo, parts, rows = 0, [], 0
        for (di, sd), (ti, st) in zip(bam_device.walk(dev, src_d), bam_device.walk(twin, src_t)):
            assert di.n_rows == ti.n_rows and di.n_rows > 0
            dc, tc = dev.text_check(), twin.text_check()
            assert [getattr(dc, f) for f in fields] == [getattr(tc, f) for f in fields]
            assert dc.first_odd_row == -1 and dc.waits == 1                         # zero odd pieces
            assert dev.process(lo)[0] == -1
            b = twin.batch()
            twin.set_trim(res.rows(b, lo, lo + b.n))
            lo += b.n
            (dt, df), (tt, tf) = dev.format(30, False), twin.format(30, False)
            assert [getattr(df, f) for f in fields] == [getattr(tf, f) for f in fields]
            assert dt == tt
            assert di.waits + dc.waits + 1 + df.waits <= 5                          # feed, check, process, format x 2
            parts.append(dt); rows += int(df.n_rows_written)
        assert b"".join(parts) == text and rows == int(keep.sum())
        assert len(parts) > (3 if piece_bytes < (1 << 30) else 0)
    dev.close(); twin.close(); eng.close()
    gc.collect()


# ---- the sub-commands through the command line -------------------------------------------------------------------------------------------
def start(cwd, args, mode, piece_bytes=512 << 10):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env["AMPLIPY_GPU_BAM_PIECE_BYTES"] = str(piece_bytes)
    env.update(MODES[mode])
    os.makedirs(cwd, exist_ok=True)
    return subprocess.Popen([sys.executable, "-m", "amplipy_amd"] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def finish(p):
    out, err = p.communicate(timeout=900)
    return subprocess.CompletedProcess(p.args, p.returncode, out, err)


def cli(cwd, args, mode, **kw):
    return finish(start(cwd, args, mode, **kw))


def log(r):          # the log lines without their time stamps and without the codec's own line
    return [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[") and b"BAM device codec" not in l]


def test_trim_to_a_file_trim_to_stdout_and_aio_on_against_off(tmp_path, files, monkeypatch):
    """Both switches on against both off: the trimmed text (header included), VCF, consensus and the log lines are identical; every
    piece is formatted on the device.  60,000 records, so that a progress line is among the log lines."""
    ref, bed = files
    inp = write_packed(str(tmp_path / "in.bam"), synth.make_amplicon_batch(G, AMPS, 60000, seed=7))
    procs = {}
    for mode in ("off", "on"):                                                      # six runs at once: the Python codec takes its time
        d = str(tmp_path / mode)
        procs[mode] = (start(d, ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.sam"], mode),
                       start(d, ["trim", "-i", inp, "-p", bed, "-r", ref], mode),
                       start(d, ["aio", "-i", inp, "-p", bed, "-r", ref, "-ot", "a.sam", "-ov", "a.vcf", "-oc", "a.fas"], mode))
    out = {}
    for mode in ("off", "on"):
        t, s, a = (finish(p) for p in procs[mode])
        assert t.returncode == 0 and s.returncode == 0 and a.returncode == 0, (t.stderr[-2000:], s.stderr[-2000:], a.stderr[-2000:])
        d = str(tmp_path / mode)
        out[mode] = [read(os.path.join(d, "t.sam")), s.stdout, read(os.path.join(d, "a.sam")), read(os.path.join(d, "a.vcf")), read(os.path.join(d, "a.fas")),
                     log(t), log(s), log(a), t.stderr, s.stderr, a.stderr]
    for k in range(8):
        assert out["on"][k] == out["off"][k], k
    n_lines = out["on"][0].count(b"\n") - H
    assert n_lines > 20000 and len(out["on"][3]) > 500 and len(out["on"][4]) > G.size
    assert b"Processed 50000 reads..." in out["on"][5]
    # the header lines are the same in all three; the command line of the @PG line is each run's own
    assert out["on"][1].split(b"\n@PG\tID:AmpliPy")[0] == out["on"][0].split(b"\n@PG\tID:AmpliPy")[0]
    assert out["on"][1].split(b"\n")[H:] == out["on"][0].split(b"\n")[H:]
    for k in (8, 9, 10):
        assert out["on"][k].count(TEXT_LINE) == 1 and b" pieces on the device, 0 through the Python codec" in out["on"][k]
        assert b"0 through the host codec" in out["on"][k] and b"BAM device codec" not in out["off"][k]
    # the same run in this process: its statistics
    st = run(monkeypatch, True, True, 512 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=str(tmp_path / "stats.sam"),
             primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=False, run_trim=True)
    got = read(str(tmp_path / "stats.sam"))
    assert got.split(b"\n")[H:] == out["off"][0].split(b"\n")[H:]
    assert st["pieces"] > 3 and st["text_pieces_device"] == st["pieces"] and st["text_pieces_python"] == 0
    assert st["text_rows"] == n_lines and st["text_bytes"] == sum(len(l) + 1 for l in got.split(b"\n")[H:-1])
    assert st["waits"] <= 5 * st["pieces"] and st["blocks_host"] == 0
    assert st["bytes_down"] <= st["text_bytes"] + 24 * st["pieces"]                   # down: the counters and the text
    gc.collect()


def run(monkeypatch, gpu_bam, gpu_sam, piece_bytes=None, **kw):
    """run_amplipy with sys.argv pinned (the @PG line records it) and the switches as given: LAST_RUN_STATS afterwards."""
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if piece_bytes:
        monkeypatch.setenv("AMPLIPY_GPU_BAM_PIECE_BYTES", str(piece_bytes))
    bam_device.LAST_RUN_STATS.update((k, -1) for k in bam_device.LAST_RUN_STATS)
    amplipy.run_amplipy(gpu_bam=gpu_bam, gpu_sam=gpu_sam, **kw)
    return dict(bam_device.LAST_RUN_STATS)


TRIM = dict(primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=False, run_trim=True)


def test_a_record_with_a_nan_goes_through_the_python_codec_and_the_other_pieces_stay(tmp_path, files, monkeypatch):
    ref, bed = files
    recs = pool_recs(synth.make_mixed_segments(G, AMPS, 4000, 83), 5)
    recs[2100].aux_sam = None
    recs[2100].aux_bam = b"NMC\x02" + b"xff" + struct.pack("<I", 0x7FC00000) + b"XSZbehind\0"
    inp = write_raw(str(tmp_path / "nan.bam"), recs)
    run(monkeypatch, False, False, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=str(tmp_path / "off.sam"), **TRIM)
    st = run(monkeypatch, True, True, 64 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=str(tmp_path / "on.sam"), **TRIM)
    on, off = read(str(tmp_path / "on.sam")), read(str(tmp_path / "off.sam"))
    assert on == off and b"\txf:f:nan\tXS:Z:behind\n" in on
    assert st["text_pieces_python"] == 1 and st["text_pieces_device"] == st["pieces"] - 1 and st["pieces"] > 5
    assert 0 < st["text_rows"] < on.count(b"\n")
    gc.collect()


def test_failing_read_empty_file_missing_pg_and_existing_output_end_like_the_python_codec(tmp_path, files):
    """A read the loop fails on mid-file: the same partial output, the same exception type and message.  An empty BAM: the header
    and the reference's NameError.  A header without @PG: KeyError.  An existing output file: the host path's message."""
    ref, bed = files
    recs = pool_recs(synth.make_mixed_segments(G, AMPS, 3000, 71), 9)
    r = recs[1700]
    recs[1700] = bamio.Rec(r.qname, 0, 0, r.pos, 60, [(0, 10)], -1, -1, 0, None, None)      # a CIGAR and no bases: the loop fails on it (A:702)
    bad = write_raw(str(tmp_path / "bad.bam"), recs)
    empty = write_raw(str(tmp_path / "empty.bam"), [])
    nopg = write_raw(str(tmp_path / "nopg.bam"), recs[:10], bamio.Header("@HD\tVN:1.6\n@SQ\tSN:SYN_REF\tLN:%d\n" % G.size, [("SYN_REF", int(G.size))]))
    got = {}
    for mode in ("off", "on"):
        d = str(tmp_path / mode)
        os.makedirs(d)
        open(os.path.join(d, "exists.sam"), "w").write("keep me\n")
        runs = [start(d, ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", o], mode, piece_bytes=64 << 10)
                for inp, o in ((bad, "b.sam"), (empty, "e.sam"), (nopg, "n.sam"), (bad, "exists.sam"))]
        b, e, n, x = (finish(p) for p in runs)
        assert b.returncode != 0 and e.returncode != 0 and n.returncode != 0 and x.returncode != 0
        got[mode] = (read(os.path.join(d, "b.sam")), read(os.path.join(d, "e.sam")), os.path.exists(os.path.join(d, "n.sam")), read(os.path.join(d, "exists.sam")),
                     [r_.stderr.splitlines()[-1].split(b"] ", 1)[-1] for r_ in (b, e, n, x)], [log(r_) for r_ in (b, e, n, x)])
    assert got["on"] == got["off"]
    partial, header, made, kept, last, _ = got["on"]
    assert 500 < partial.count(b"\n") < 1700 and b"AmpBamError" not in last[0] and b"Error" in last[0]
    assert header.count(b"\n") == HDR.text.count("\n") + 1 and b"NameError" in last[1]
    assert not made and b"KeyError" in last[2]
    assert kept == b"keep me\n" and last[3].startswith(b"ERROR: File already exists: ")


def test_either_switch_alone_and_both_with_a_bam_output_are_the_runs_of_today(tmp_path, files):
    ref, bed = files
    inp = write_recs(str(tmp_path / "in.bam"), seg_recs(synth.make_mixed_segments(G, AMPS, 3000, 61)))
    runs = {mode: start(str(tmp_path / mode), ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.sam"], mode) for mode in ("off", "bam_only", "sam_only")}
    runs.update({mode + "_bam": start(str(tmp_path / mode), ["trim", "-i", inp, "-p", bed, "-r", ref, "-o", "t.bam"], mode) for mode in ("off", "bam_only", "on")})
    done = {k: finish(p) for k, p in runs.items()}
    assert all(r.returncode == 0 for r in done.values()), [r.stderr[-1000:] for r in done.values()]
    for mode in ("bam_only", "sam_only"):
        assert read(str(tmp_path / mode / "t.sam")) == read(str(tmp_path / "off" / "t.sam"))
        assert log(done[mode]) == log(done["off"])
        assert b"BAM device codec" not in done[mode].stderr and b"SAM text codec" not in done[mode].stderr
    for mode in ("bam_only", "on"):
        assert read(str(tmp_path / mode / "t.bam")) == read(str(tmp_path / "off" / "t.bam"))
        assert log(done[mode + "_bam"]) == log(done["off_bam"]) and TEXT_LINE not in done[mode + "_bam"].stderr
        assert done[mode + "_bam"].stderr.count(b"BAM device codec: this run writes trimmed reads, the host codec reads the input") == 1
