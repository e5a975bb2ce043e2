"""The clip sites of the QC report on the device (amp_qc.hip: k_qc_clips) against the plain restatement of
tests/clip_util.py, applied to the batch and the DEVICE's own statuses.  Table and scalars are integers: they must be EQUAL.  The
crafted reads of the rule's edges; waves whose reads share one site, are all distinct, are mixed, or have no clip of a side;
batch sizes around a wave, a block and past a block's first tile; unsorted input; state across batches, reset, a new report,
the merge; trimming on and off; and one command-line run on a reference with a 120-base deletion the reads' CIGARs clip."""
import json
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, bamio, clips, lib, synth
from amplipy_amd.batch import SEQ_NT16, ReadBatch, unpack_nibbles
from tests import clip_util as U
from tests import qc_util as Q

pytestmark = pytest.mark.gpu

G = 3000
PRIMERS = [(100, 125), (400, 425), (1500, 1525), (2800, 2825)]
CLIP_MIN = 10
_ENG = {}
_BATCHES = {}


def engine(do_trim=True, clip_min=CLIP_MIN):
    """The shared engine, reset, a NEW report and its clip sites on."""
    if "e" not in _ENG:
        e = lib.Engine(G)
        e.set_primers(*lib.find_overlapping_primers(G, PRIMERS, 0))
        _ENG["e"] = e
    e = _ENG["e"]
    e.set_params(20, 4, do_trim, True)
    e.reset()
    e.qc_enable(PRIMERS, 0, 30, False, [(0, G)], [1])
    if clip_min:
        e.qc_clips_enable(clip_min)
    return e


def wave(kind, n, seed=5):
    key = (kind, n, seed)
    if key not in _BATCHES:
        _BATCHES[key] = U.wave_batch(kind, n, G, seed)
    return _BATCHES[key]


def assert_tables(got, want, what=""):
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])


@pytest.mark.parametrize("clip_min", [1, 10, 17])
def test_crafted_reads(clip_min):
    batch = U.crafted_batch(G, clip_min)
    e = engine(clip_min=clip_min)
    res = e.process(batch)
    want = U.tables(batch, G, clip_min, res.status)
    assert_tables(e.qc_clips_tables(), want)
    # rows with a status add to nothing, not even to `skipped`
    assert res.status.any() and int(want[1][0] + want[1][1]) == int((res.status == 0).sum())
    assert int(want[1][0]) > 40 and int(want[1][2]) > 0 and int(want[1][3]) > 0
    assert e.qc_clips_last_ms() > 0 and e.qc_last_ms() > 0


@pytest.mark.parametrize("kind", ["one_site", "distinct", "mixed", "left_only", "right_only", "none"])
def test_wave_shapes(kind):
    batch = wave(kind, 2500)
    e = engine()
    res = e.process(batch)
    assert not res.status.any()
    want = U.tables(batch, G, CLIP_MIN, res.status)
    assert_tables(e.qc_clips_tables(), want, kind)
    sites = (int((want[0][:, 0, 0] > 0).sum()), int((want[0][:, 1, 0] > 0).sum()))
    if kind == "one_site":
        assert sites == (1, 1) and int(want[0][300, 0, 0]) == 2500
    if kind == "distinct":
        assert sites == (2500, 2500)
    if kind in ("left_only", "none"):
        assert sites[1] == 0
    if kind in ("right_only", "none"):
        assert sites[0] == 0
    assert int(want[1][0]) == 2500


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 2500])
def test_read_counts(n):
    batch = wave("mixed", n, seed=40 + n)
    e = engine()
    res = e.process(batch)
    assert_tables(e.qc_clips_tables(), U.tables(batch, G, CLIP_MIN, res.status), n)


def test_unsorted_batch_gives_the_sorted_batch_s_table():
    batch = wave("mixed", 2500)
    assert (np.diff(batch.pos) < 0).any()
    ordered = synth.gather_rows(batch, np.argsort(batch.pos, kind="stable"))
    e = engine()
    e.process(batch)
    got = e.qc_clips_tables()
    e.reset()
    res = e.process(ordered)
    assert_tables(e.qc_clips_tables(), got)
    assert_tables(got, U.tables(ordered, G, CLIP_MIN, res.status))


def test_batches_accumulate_reset_clears_and_add_doubles():
    a, b = wave("mixed", 257, seed=1), wave("one_site", 300, seed=2)
    e = engine()
    ra = e.process(a)
    rb = e.process(b)
    wa, wb = U.tables(a, G, CLIP_MIN, ra.status), U.tables(b, G, CLIP_MIN, rb.status)
    total = (wa[0] + wb[0], wa[1] + wb[1])
    assert_tables(e.qc_clips_tables(), total)
    e.qc_clips_add(*total)                                     # the merge of a partial table: here its own
    assert_tables(e.qc_clips_tables(), (2 * total[0], 2 * total[1]))
    e.reset()
    t, s = e.qc_clips_tables()
    assert not t.any() and not s.any()
    e.process(a)
    assert_tables(e.qc_clips_tables(), wa)
    e.qc_clips_enable(0)                                       # off: what was tallied stays readable, nothing is added
    e.process(b)
    assert_tables(e.qc_clips_tables(), wa)


def test_a_new_report_needs_the_sub_switch_again():
    e = engine()
    e.process(wave("mixed", 65, seed=3))
    e.qc_enable(PRIMERS, 0, 30, False, [(0, G)], [1])
    for call in (e.qc_clips_tables, e.qc_clips_last_ms, lambda: e.qc_clips_add(None, None)):
        with pytest.raises(lib.AmpliHipError) as err:
            call()
        assert err.value.rc == -5 and "amp_qc_clips_enable" in str(err.value)
    batch = wave("mixed", 65, seed=3)
    e.qc_clips_enable(CLIP_MIN)
    res = e.process(batch)
    assert_tables(e.qc_clips_tables(), U.tables(batch, G, CLIP_MIN, res.status))
    for bad in (-1, 65):
        with pytest.raises(lib.AmpliHipError) as err:
            e.qc_clips_enable(bad)
        assert err.value.rc == -1 and "clip_min" in str(err.value)
    fresh = lib.Engine(500)
    with pytest.raises(lib.AmpliHipError) as err:              # no report at all
        fresh.qc_clips_enable(10)
    assert err.value.rc == -5
    fresh.close()


def test_trimming_on_and_off_give_the_same_table():
    batch = Q.mixed_batch(2500, G, PRIMERS, 9, bad_read=False)
    got = {}
    for do_trim in (True, False):
        e = engine(do_trim=do_trim)
        res = e.process(batch)
        assert not res.status.any()
        got[do_trim] = e.qc_clips_tables()
    assert_tables(got[True], got[False])
    want = U.tables(batch, G, CLIP_MIN)
    assert_tables(got[True], want)
    assert int(want[1][2]) > 50 and int(want[1][3]) > 50


def test_the_report_s_tallies_do_not_change_with_the_sub_switch():
    batch = Q.mixed_batch(2500, G, PRIMERS, 10)
    tallies = {}
    for clip_min in (0, CLIP_MIN):
        e = engine(clip_min=clip_min)
        e.process(batch)
        tallies[clip_min] = e.qc_read_tallies()
        counts = e.counts()
        tallies[clip_min] += (counts.tobytes(),)
    assert tallies[0][0] == tallies[CLIP_MIN][0] and tallies[0][0]["rows"] == 2500
    assert np.array_equal(tallies[0][1], tallies[CLIP_MIN][1]) and np.array_equal(tallies[0][2], tallies[CLIP_MIN][2])
    assert tallies[0][3] == tallies[CLIP_MIN][3]


# ---- the command line -----------------------------------------------------------------------------------------------------------
REF_LEN, DEL_AT, DEL_LEN = 600, 240, 120
N_RIGHT, N_RIGHT_REV, N_LEFT, N_LEFT_REV, N_PLAIN = 30, 12, 25, 10, 40


def write_reads(path, mode, hb, ref_len):
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % ref_len, [("SYN_REF", ref_len)])
    w = bamio.AlignmentWriter(path, mode, hdr)
    lut = np.frombuffer(SEQ_NT16.encode(), np.uint8)
    for i in range(hb.n):
        o = int(hb.seq_off[i]); L = int(hb.lseq[i])
        seq = lut[unpack_nibbles(hb.seq[o // 2:(o + L + 1) // 2], L)].tobytes().decode()
        a, c = int(hb.cig_off[i]), int(hb.cig_off[i + 1])
        w.write(bamio.Rec("r%d" % i, int(hb.flag[i]), 0, int(hb.pos[i]), 60, [(int(v) & 15, int(v) >> 4) for v in hb.cig[a:c]], 0,
                          int(hb.pos[i]), int(hb.tlen[i]), seq, bytes(hb.qual[o:o + L])))
    w.close()
    return path


@pytest.fixture(scope="module")
def deletion_job(tmp_path_factory):
    """A seeded 600-base reference, a sample without [240, 360), and reads whose CIGARs clip at the junction (no aligner):
    60M40S from the left, 40S60M from the right, and plain reads elsewhere."""
    d = tmp_path_factory.mktemp("clips_cli")
    rng = np.random.default_rng(2024)
    R = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=REF_LEN)].tobytes().decode()
    sample = R[:DEL_AT] + R[DEL_AT + DEL_LEN:]
    segs = []
    for k in range(N_PLAIN):
        pos = (0, 40, 420, 480)[k % 4]
        segs.append(U.seg(pos, [(0, 100)], rng, seq=R[pos:pos + 100]))
    for k in range(N_RIGHT):            # aligned up to the junction, the rest of the sample clipped: a RIGHT site at 240
        segs.append(U.seg(DEL_AT - 60, [(0, 60), (4, 40)], rng, flag=0x10 if k < N_RIGHT_REV else 0, seq=sample[DEL_AT - 60:DEL_AT + 40]))
    for k in range(N_LEFT):             # aligned from the junction on: a LEFT site at 360
        segs.append(U.seg(DEL_AT + DEL_LEN, [(4, 40), (0, 60)], rng, flag=0x10 if k < N_LEFT_REV else 0, seq=sample[DEL_AT - 40:DEL_AT + 60]))
    segs.sort(key=lambda g: g.reference_start)
    batch = ReadBatch.from_segments(segs)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + R + "\n")
    files = dict(ref=str(ref), bam=write_reads(str(d / "in.bam"), "wb", batch, REF_LEN), sam=write_reads(str(d / "in.sam"), "w", batch, REF_LEN))
    # what the run must find: the interval left-aligned by hand, the flank depths from the reads' aligned bases
    s = DEL_AT
    while s > 0 and R[s - 1] == R[s + DEL_LEN - 1]:
        s -= 1
    cover = np.zeros(REF_LEN, np.int64)
    for g in segs:
        cover[g.reference_start:g.reference_start + g.reference_length] += 1
    row = dict(kind="deletion", start=s + 1, end=s + DEL_LEN, length=DEL_LEN, right_reads=N_RIGHT, right_reverse=N_RIGHT_REV, left_reads=N_LEFT,
               left_reverse=N_LEFT_REV, flank_depth_left=int(cover[s - 1]), flank_depth_right=int(cover[s + DEL_LEN]))
    assert R.count(R[DEL_AT + DEL_LEN:DEL_AT + DEL_LEN + 16]) == 1 and R.count(R[DEL_AT - 16:DEL_AT]) == 1
    return files, row, d


ROUTES = [("host", "bam", {}), ("gpu_sam", "sam", dict(gpu_sam=True)), ("gpu_bam", "bam", dict(gpu_bam=True))]
_TEXTS = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_run_finds_the_deletion_on_every_route(tmp_path, deletion_job, monkeypatch, route):
    files, row, _ = deletion_job
    name, inp, switches = route
    for k in ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    out = {k: str(tmp_path / k) for k in ("v.vcf", "q.json", "j.tsv", "c.tsv", "plain.vcf")}
    amplipy.run_amplipy(trimmed_reads_fn=files[inp], reference_fn=files["ref"], variants_fn=out["v.vcf"], min_quality=20, min_freq_variants=0.03,
                        min_depth_variants=10, run_variants=True, qc_fn=out["q.json"], qc_clips=True, qc_clip_fn=out["c.tsv"],
                        qc_junction_fn=out["j.tsv"], **switches)
    amplipy.run_amplipy(trimmed_reads_fn=files[inp], reference_fn=files["ref"], variants_fn=out["plain.vcf"], min_quality=20, min_freq_variants=0.03,
                        min_depth_variants=10, run_variants=True, **switches)
    texts = {k: open(v).read() for k, v in out.items()}
    assert texts["v.vcf"] == texts["plain.vcf"]                # no key on the VCF, no other byte of it
    rep = json.loads(texts["q.json"])
    assert list(rep)[-1] == "clips"
    c = rep["clips"]
    total = N_PLAIN + N_RIGHT + N_LEFT
    assert (c["clip_min"], c["min_reads"], c["scanned"], c["skipped"], c["left"], c["right"]) == (10, 2, total, 0, N_LEFT, N_RIGHT)
    assert c["junctions"] == [row]
    assert c["sites"] == 2 and c["sites_by_class"]["deletion"] == 2 and sum(c["sites_by_class"].values()) == 2
    lines = texts["j.tsv"].splitlines()
    assert lines[0] == "#" + "\t".join(clips.JUNCTION_COLUMNS)
    assert lines[1:] == ["\t".join(["SYN_REF"] + [str(row[k]) for k in clips.JUNCTION_COLUMNS[1:]])]
    sites = [l.split("\t") for l in texts["c.tsv"].splitlines()[1:]]
    assert [(l[1], l[2], l[3], l[4], l[6]) for l in sites] == [(str(DEL_AT + 1), "right", str(N_RIGHT), str(N_RIGHT_REV), "deletion"),
                                                                 (str(DEL_AT + DEL_LEN + 1), "left", str(N_LEFT), str(N_LEFT_REV), "deletion")]
    _TEXTS[name] = (texts["q.json"], texts["j.tsv"], texts["c.tsv"])
    assert all(t == _TEXTS[name] for t in _TEXTS.values())    # the same files on every route run so far


def test_two_ranks_give_the_one_process_files(tmp_path, deletion_job):
    from tests import test_gpu_ranks as RK
    files, row, _ = deletion_job
    argv = lambda tag: ["variants", "-i", files["sam"], "-r", files["ref"], "-o", tag + ".vcf", "-mf", "0.03", "-md", "10", "--qc", tag + ".json",
                        "--qc_clips", "--qc_junction_out", tag + ".j.tsv", "--qc_clip_out", tag + ".c.tsv", "--qc_clip_min", "12", "--qc_clip_reads", "3"]
    RK.one_process(tmp_path, argv("one"))
    status, logs = RK.run_ranks(2, tmp_path, argv("two"))
    assert status == [0, 0], "".join(logs)
    for ext in (".vcf", ".json", ".j.tsv", ".c.tsv"):
        assert open(str(tmp_path / ("two" + ext))).read() == open(str(tmp_path / ("one" + ext))).read(), ext
    c = json.load(open(str(tmp_path / "two.json")))["clips"]
    assert c["junctions"] == [row] and (c["clip_min"], c["min_reads"]) == (12, 3)
