"""The opt-in device codec for SAM text on the GPU: amp_sam_* (amplipy_amd/csrc/amp_sam.hip) against its host twin and the Python
codec, and AMPLIPY_GPU_SAM=1 / run_amplipy(gpu_sam=True) against the switch off: byte-identical outputs."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from amplipy_amd import sam_native, synth
from tests import helpers as H
from tests import sam_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = synth.make_genome()
PRIMERS, AMPS = synth.make_artic_scheme()
HDR = U.header(G.size)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("samfiles")
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(G) + "\n")
    bed = d / "p.bed"; bed.write_text("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(PRIMERS)))
    return str(ref), str(bed)


def write_sam(path, lines, hdr=HDR):
    with open(path, "wb") as f:
        f.write(hdr.text.encode()); f.write(b"".join(lines))
    return str(path)


def amplicon_lines(n, seed, **kw):
    rng = np.random.default_rng(seed)
    return U.segments_to_lines(synth.make_amplicon_batch(G, AMPS, n, seed=seed, **kw).segments(), HDR, rng, max_aux=3)


def run(monkeypatch, on, chunk_bytes=None, **kw):
    """run_amplipy with sys.argv pinned (the @PG line and the VCF header record it) and the switch on or off."""
    from amplipy_amd import amplipy
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    monkeypatch.delenv("AMPLIPY_GPU_SAM", raising=False)
    if chunk_bytes:
        monkeypatch.setenv("AMPLIPY_SAM_CHUNK_BYTES", str(chunk_bytes))
    sam_native.LAST_RUN_STATS.update(device_chunks=-1, python_chunks=-1, records=-1)
    amplipy.run_amplipy(gpu_sam=on, **kw)
    return dict(sam_native.LAST_RUN_STATS)


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- 5. device batch = twin batch = Python packer batch ----------------------------------------------------------------------------------
def test_device_batch_equals_twin_and_python_packer(tmp_path):
    from amplipy_amd import lib
    from tests.test_sam_text import hand_written_lines
    rng = np.random.default_rng(5)
    lines = amplicon_lines(185000, 41) + U.segments_to_lines(synth.make_mixed_segments(G, AMPS, 12000, 42) + U.many_op_segments(rng, 4000, G.size), HDR, rng)
    hand = hand_written_lines()
    for k in range(0, len(lines), 9000):
        lines[k:k] = hand
    assert len(lines) >= 200000
    text = b"".join(lines)
    path = write_sam(tmp_path / "big.sam", lines)
    recs, _ = U.python_records(text, HDR)
    pb = U.python_batch(recs)
    eng = lib.Engine(G.size)
    dev = sam_native.SamCodec(eng); dev.set_references(U.ref_names(HDR))
    twin = sam_native.SamCodec(twin=U.twin_path(tmp_path)); twin.set_references(U.ref_names(HDR))
    for chunk_bytes in (64 << 10, 1 << 20, 1 << 30):
        src = sam_native.SamTextInput(path, chunk_bytes)
        assert src.header_raw == HDR.text.encode()
        rows = recs_seen = n_chunks = 0
        for chunk in src:
            di, ti = dev.parse(chunk), twin.parse(chunk)
            fields = [f for f, _ in di._fields_]
            assert [getattr(di, f) for f in fields] == [getattr(ti, f) for f in fields] and di.first_odd_line == -1
            db, tb = dev.batch(), twin.batch()
            assert U.same_batch(db, tb) == ""
            lo, hi = rows, rows + db.n
            c0, s0 = int(pb.cig_off[lo]), int(pb.seq_off[lo])
            assert np.array_equal(db.pos, pb.pos[lo:hi]) and np.array_equal(db.flag, pb.flag[lo:hi]) and np.array_equal(db.tlen, pb.tlen[lo:hi])
            assert np.array_equal(db.lseq, pb.lseq[lo:hi])
            assert np.array_equal(db.cig_off, pb.cig_off[lo:hi + 1] - np.uint64(c0)) and np.array_equal(db.cig, pb.cig[c0:int(pb.cig_off[hi])])
            assert np.array_equal(db.seq_off, pb.seq_off[lo:hi + 1] - np.uint64(s0))
            assert np.array_equal(db.seq, pb.seq[s0 // 2:int(pb.seq_off[hi]) // 2]) and np.array_equal(db.qual, pb.qual[s0:int(pb.seq_off[hi])])
            assert np.array_equal(db.src_index + recs_seen, pb.src_index[lo:hi])
            rows = hi; recs_seen += di.n_records; n_chunks += 1
        src.close()
        assert rows == pb.n and recs_seen == len(recs)
        assert n_chunks == 1 if chunk_bytes == 1 << 30 else n_chunks > len(text) // chunk_bytes - 2
    dev.close(); twin.close(); eng.close()


def test_device_format_equals_twin(tmp_path):
    """amp_sam_process + amp_sam_format on the device against the twin fed with the device's own trim results."""
    from amplipy_amd import abi, lib
    from tests.test_sam_text import hand_written_lines
    rng = np.random.default_rng(6)
    lines = amplicon_lines(20000, 43) + U.segments_to_lines(synth.make_mixed_segments(G, AMPS, 3000, 44), HDR, rng) + hand_written_lines()
    lines = [lines[i] for i in rng.permutation(len(lines))]
    chunk = b"".join(lines)
    pr = [(s, e) for s, e, _ in PRIMERS]
    mn, mx, mpl = lib.find_overlapping_primers(G.size, pr, 0)
    eng = lib.Engine(G.size); eng.set_primers(mn, mx, mpl); eng.set_params(20, 4, True, True)
    dev = sam_native.SamCodec(eng); dev.set_references(U.ref_names(HDR))
    twin = sam_native.SamCodec(twin=U.twin_path(tmp_path)); twin.set_references(U.ref_names(HDR))
    dev.parse(chunk); twin.parse(chunk)
    pb = dev.batch()
    bad, st = dev.process(0)
    res = eng.process(pb)                      # the same rows through the host-pointer entry: the results the twin formats
    first = np.nonzero(res.status)[0]
    assert (bad, st) == ((int(first[0]), int(res.status[first[0]])) if len(first) else (-1, 0))
    assert twin.twin_set_results(res) == (bad, st)
    for inp in (False, True):
        for min_length in (30, 140):
            got, want = dev.format(min_length, inp), twin.format(min_length, inp)
            assert got == want and (got[1] > 0 or bad == 0)
    dev.close(); twin.close(); eng.close()


# ---- 6. the four sub-commands, switch on against switch off --------------------------------------------------------------------------------
def golden_pileup_lines():
    from amplipy_amd import bamio
    from amplipy_amd.segment import parse_cigar
    g = H.load_json("pileup_5000.json.gz")
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % g["ref_len"], [("SYN_REF", g["ref_len"])])
    import io
    out = io.StringIO()
    w = bamio.AlignmentWriter(None, "w", hdr, fileobj=out)
    start = out.tell()
    for i, d in enumerate(g["reads"]):
        w.write(bamio.Rec("r%d" % i, d["flag"], 0, d["pos"], 60, parse_cigar(d["cigar"]), 0, d["pos"], d["tlen"], d["seq"],
                          bytes(ord(c) - 33 for c in d["qual"]), aux_sam=["NM:i:1"]))
    return g, hdr, [l.encode() + b"\n" for l in out.getvalue()[start:].split("\n")[:-1]]


@pytest.mark.parametrize("which", ["golden_pileup", "config5"])
def test_sub_commands_on_against_off(tmp_path, files, monkeypatch, which):
    ref, bed = files
    if which == "golden_pileup":
        g, hdr, lines = golden_pileup_lines()
        ref = str(tmp_path / "ref.fas"); open(ref, "w").write(">SYN_REF test\n" + g["ref_seq"] + "\n")
        bed = str(tmp_path / "p.bed"); open(bed, "w").write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e) in enumerate(g["primers"])))
        p = g["params"]
        par = dict(min_quality=p["min_quality"], sliding_window_width=p["window"], min_length=p["min_length"])
        call = dict(min_depth_consensus=p["min_depth_consensus"], min_freq_consensus=p["min_freq_consensus"],
                    min_depth_variants=p["min_depth_variants"], min_freq_variants=p["min_freq_variants"])
    else:
        rng = np.random.default_rng(9)
        hdr, lines = HDR, U.segments_to_lines(synth.make_mixed_segments(G, AMPS, 6000, 61), HDR, rng, max_aux=4)
        par = dict(min_quality=20, sliding_window_width=4, min_length=30)
        call = dict(min_depth_consensus=10, min_freq_consensus=0.5, min_depth_variants=5, min_freq_variants=0.03)
    inp = write_sam(tmp_path / "in.sam", lines, hdr)
    outs = {}
    for on in (False, True):
        t = "on" if on else "off"
        o = {k: str(tmp_path / ("%s_%s" % (t, k))) for k in ("aio_t.sam", "aio_v.vcf", "aio_c.fas", "trim.sam", "var.vcf", "cons.fas")}
        st = [run(monkeypatch, on, 256 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=o["aio_t.sam"],
                  variants_fn=o["aio_v.vcf"], consensus_fn=o["aio_c.fas"], primer_pos_offset=0, unknown_symbol="N", include_no_primer=False,
                  run_trim=True, run_variants=True, run_consensus=True, **par, **call),
              run(monkeypatch, on, 256 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=o["trim.sam"],
                  primer_pos_offset=0, include_no_primer=True, run_trim=True, **par),
              run(monkeypatch, on, 256 << 10, trimmed_reads_fn=o["aio_t.sam"], reference_fn=ref, variants_fn=o["var.vcf"], min_quality=par["min_quality"],
                  min_freq_variants=call["min_freq_variants"], min_depth_variants=call["min_depth_variants"], run_variants=True),
              run(monkeypatch, on, 256 << 10, trimmed_reads_fn=o["aio_t.sam"], reference_fn=ref, consensus_fn=o["cons.fas"], min_quality=par["min_quality"],
                  min_freq_consensus=call["min_freq_consensus"], min_depth_consensus=call["min_depth_consensus"], unknown_symbol="N", run_consensus=True)]
        outs[on] = o
        for s in st:
            if on:
                assert s["device_chunks"] >= 1 and s["python_chunks"] == 0, s          # every chunk by the device, none by the Python codec
            else:
                assert s["device_chunks"] == -1                                     # the switch is off: the path is not entered
        if on:
            assert st[0]["device_chunks"] > 2 and st[0]["records"] == len(lines)
    for k in outs[True]:
        a, b = read(outs[False][k]), read(outs[True][k])
        assert a == b, k
        assert len(a) > 100


# ---- 7. through pipes: a fresh child process ------------------------------------------------------------------------------------------------
def test_trim_through_pipes(tmp_path, files):
    ref, bed = files
    inp = write_sam(tmp_path / "in.sam", amplicon_lines(8000, 71))
    outs = {}
    for on in (False, True):
        env = dict(os.environ); env.pop("AMPLIPY_GPU_SAM", None)
        env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        env["AMPLIPY_SAM_CHUNK_BYTES"] = str(256 << 10)
        if on:
            env["AMPLIPY_GPU_SAM"] = "1"
        with open(inp, "rb") as f:
            r = subprocess.run([sys.executable, "-m", "amplipy_amd", "trim", "-p", bed, "-r", ref], stdin=f, env=env, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[on] = r
    assert outs[True].stdout == outs[False].stdout and outs[True].stdout.count(b"\n") > 4000
    assert b"chunks on the device, 0 through the Python codec" in outs[True].stderr and b"SAM text codec" not in outs[False].stderr

    def log(r):          # the log lines without their time stamps
        return [l.split(b"] ", 1)[1] for l in r.stderr.splitlines() if l.startswith(b"[") and b"SAM text codec" not in l]
    assert log(outs[True]) == log(outs[False]) and any(l.startswith(b"Finished Processing 7999 reads") for l in log(outs[True]))


# ---- 8. one odd line in the third chunk ------------------------------------------------------------------------------------------------------
def test_one_odd_line_goes_through_the_python_codec(tmp_path, files, monkeypatch):
    ref, bed = files
    lines = amplicon_lines(3000, 81)
    size = np.cumsum([len(l) for l in lines])
    k = int(np.searchsorted(size, 2 * (64 << 10) + 20000))                 # a line well inside the third chunk of 64 KB
    f = lines[k].split(b"\t"); f[1] = b"0" + f[1]; lines[k] = b"\t".join(f)       # FLAG with a leading zero: rendered without it
    inp = write_sam(tmp_path / "in.sam", lines)
    outs = {}
    for on in (False, True):
        o = {x: str(tmp_path / ("%d_%s" % (on, x))) for x in ("t.sam", "v.vcf", "c.fas")}
        st = run(monkeypatch, on, 64 << 10, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=o["t.sam"], variants_fn=o["v.vcf"],
                 consensus_fn=o["c.fas"], primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, min_freq_consensus=0.5,
                 min_freq_variants=0.03, min_depth_consensus=10, min_depth_variants=1, unknown_symbol="N", include_no_primer=True,
                 run_trim=True, run_variants=True, run_consensus=True)
        outs[on] = o
        if on:
            assert st["python_chunks"] == 1 and st["device_chunks"] > 10 and st["records"] == 3000, st
    for x in outs[True]:
        assert read(outs[False][x]) == read(outs[True][x]), x
    assert lines[k].split(b"\t")[0] + b"\t" + f[1][1:] + b"\t" in read(outs[True]["t.sam"])


# ---- 9. a read with a status -------------------------------------------------------------------------------------------------------------------
def test_read_with_a_status_ends_the_run_like_the_python_path(tmp_path, files, monkeypatch):
    ref, bed = files
    lines = amplicon_lines(1500, 91)
    size = np.cumsum([len(l) for l in lines])
    k = int(np.searchsorted(size, (64 << 10) + 30000))                     # inside the second chunk
    f = lines[k].split(b"\t"); f[10] = b"*"; lines[k] = b"\t".join(f[:11]) + b"\n"         # QUAL '*' with trimming on: TypeError
    inp = write_sam(tmp_path / "in.sam", lines)
    front = write_sam(tmp_path / "front.sam", lines[:k])
    kw = dict(primer_fn=bed, reference_fn=ref, primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=True, run_trim=True)
    got = {}
    for on in (False, True):
        out = str(tmp_path / ("%d.sam" % on))
        with pytest.raises(Exception) as ei:
            run(monkeypatch, on, 64 << 10, untrimmed_reads_fn=inp, trimmed_reads_fn=out, **kw)
        got[on] = ei.type
        del ei
        gc.collect()
        got[on, "out"] = read(out)
    assert got[True] is got[False] is TypeError
    run(monkeypatch, False, untrimmed_reads_fn=front, trimmed_reads_fn=str(tmp_path / "front_out.sam"), **kw)
    want = read(str(tmp_path / "front_out.sam"))
    assert got[True, "out"] == want and want.count(b"\n") > k // 2             # exactly the kept lines in front of it


# ---- 10. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_the_python_paths(tmp_path, files, monkeypatch):
    ref, bed = files
    lines = amplicon_lines(400, 101)
    kw = dict(primer_fn=bed, reference_fn=ref, primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, include_no_primer=False, run_trim=True)
    bad = list(lines)
    f = bad[200].split(b"\t"); f[5] = b"10M5"; bad[200] = b"\t".join(f)
    malformed = write_sam(tmp_path / "malformed.sam", bad)
    no_pg = write_sam(tmp_path / "nopg.sam", lines, U.header(G.size, pg=False))
    good = write_sam(tmp_path / "good.sam", lines)
    exists = str(tmp_path / "exists.sam"); open(exists, "w").write("already here\n")
    for on in (False, True):
        with pytest.raises(ValueError, match="malformed CIGAR"):
            run(monkeypatch, on, untrimmed_reads_fn=malformed, trimmed_reads_fn=str(tmp_path / ("m%d.sam" % on)), **kw)
        with pytest.raises(KeyError, match="PG"):
            run(monkeypatch, on, untrimmed_reads_fn=no_pg, trimmed_reads_fn=str(tmp_path / ("n%d.sam" % on)), **kw)
        with pytest.raises(SystemExit) as ei:
            run(monkeypatch, on, untrimmed_reads_fn=good, trimmed_reads_fn=exists, **kw)
        assert ei.value.code == 1 and open(exists).read() == "already here\n"
        with pytest.raises(SystemExit):
            run(monkeypatch, on, untrimmed_reads_fn=str(tmp_path / "missing.sam"), trimmed_reads_fn=str(tmp_path / ("x%d.sam" % on)), **kw)
        with pytest.raises(NameError):             # an input without records
            run(monkeypatch, on, untrimmed_reads_fn=write_sam(tmp_path / ("empty%d.sam" % on), []), trimmed_reads_fn=str(tmp_path / ("e%d.sam" % on)), **kw)
        gc.collect()


# ---- 11. insertion alleles ------------------------------------------------------------------------------------------------------------------------
def test_insertion_alleles_on_indel_heavy_text(tmp_path, files, monkeypatch):
    ref, bed = files
    inp = write_sam(tmp_path / "in.sam", amplicon_lines(30000, 111, indel_frac=0.6))
    vcf = {}
    for on in (False, True):
        vcf[on] = str(tmp_path / ("%d.vcf" % on))
        st = run(monkeypatch, on, 512 << 10, trimmed_reads_fn=inp, reference_fn=ref, variants_fn=vcf[on], min_quality=20, min_freq_variants=0.002,
                 min_depth_variants=1, run_variants=True)
        assert not on or (st["python_chunks"] == 0 and st["device_chunks"] > 5)
    a, b = read(vcf[False]), read(vcf[True])
    assert a == b
    alts = [x for l in a.decode().splitlines() if not l.startswith("#") for x in l.split("\t")[4].split(",")]
    assert sum(1 for x in alts if len(x) > 1) > 50, "no insertion alleles were called"
