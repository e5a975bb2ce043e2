"""The host half of the clip sites (amplipy_amd/clips.py): consensus, classes, placement and junctions on
tables built by the restatement of tests/clip_util.py from crafted reads; the writers' exact text; abi.py's constants against the
header; the merge of partial tables; each new argument error.  No GPU needed."""
import io
import os
import re

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, clips
from amplipy_amd.batch import ReadBatch
from tests import clip_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, R_ = abi.CLIP_LEFT, abi.CLIP_RIGHT


def cells(reads, rev, columns):
    """A site's cells from per-offset (A, C, G, T, other) counts."""
    c = np.zeros(abi.CLIP_CELLS, np.uint32)
    c[0], c[1] = reads, rev
    for j, col in enumerate(columns):
        c[2 + j * abi.CLIP_COLS:2 + (j + 1) * abi.CLIP_COLS] = col
    return c


def seeded_ref(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


# ---- constants ------------------------------------------------------------------------------------------------------------------
def test_abi_constants_match_the_headers():
    hdr = open(os.path.join(ROOT, "include", "amplihip.h")).read()
    get = lambda name: re.search(r"#define %s (.+)" % name, hdr).group(1).strip()
    assert int(get("AMP_CLIP_K")) == abi.CLIP_K == 16 and int(get("AMP_CLIP_COLS")) == abi.CLIP_COLS == 5
    assert get("AMP_CLIP_CELLS") == "(2 + AMP_CLIP_K * AMP_CLIP_COLS)" and abi.CLIP_CELLS == 82
    assert int(get("AMP_CLIP_SCALARS")) == abi.CLIP_SCALARS == len(abi.CLIP_SCALAR_FIELDS) == 4
    hpp = open(os.path.join(ROOT, "amplipy_amd", "csrc", "amp_clip.hpp")).read()
    assert re.search(r"constexpr int CL_MIN_MAX = (\d+);", hpp).group(1) == str(abi.CLIP_MIN_MAX)
    assert re.search(r"constexpr int CL_LEFT = (\d), CL_RIGHT = (\d);", hpp).groups() == (str(abi.CLIP_LEFT), str(abi.CLIP_RIGHT))
    assert re.search(r"enum \{ CL_SCANNED = 0, CL_SKIPPED, CL_N_LEFT, CL_N_RIGHT, CL_N_SCALARS \};", hpp)
    assert abi.CLIP_SCALAR_FIELDS == ("scanned", "skipped", "left", "right")


# ---- consensus ------------------------------------------------------------------------------------------------------------------
def test_consensus_majority_ties_and_falling_depth():
    # 10 reads; offset 0: 6 A (a majority); 1: 5 C 5 G (a tie: N); 2: 5 T of 9 (a majority of the depth); 3: 4 of 8: exactly half is not
    # more than half; 4: depth 5 = half of the reads, still counted; 5: depth 4 < half: the consensus ends
    cols = [(6, 2, 1, 1, 0), (0, 5, 5, 0, 0), (0, 0, 2, 5, 2), (4, 4, 0, 0, 0), (0, 0, 0, 3, 2), (4, 0, 0, 0, 0), (4, 0, 0, 0, 0)]
    c = cells(10, 3, cols)
    assert clips.consensus(c, R_) == (5, "ANTNT")
    assert clips.consensus(c, L) == (5, "TNTNA")                # reference orientation: a LEFT site's text ends at the junction
    # `other` counts for the depth and never wins
    assert clips.consensus(cells(4, 0, [(0, 0, 0, 0, 4), (1, 0, 0, 0, 3), (3, 0, 0, 0, 1)]), R_) == (3, "NNA")
    assert clips.consensus(cells(3, 0, [(3, 0, 0, 0, 0)] * 16), R_) == (16, "A" * 16)
    assert clips.consensus(cells(3, 0, [(1, 0, 0, 0, 0)]), R_) == (0, "")


# ---- classes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,allowed", [(7, 0), (8, 1), (15, 1), (16, 2)])
def test_mismatch_allowance_of_contiguous(m, allowed):
    R = seeded_ref(300, 3)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    for side, p in ((R_, 100), (L, 100)):
        text = R[p:p + m] if side == R_ else R[p - m:p]
        for bad in range(allowed + 2):
            t = "".join(other[ch] if k < bad else ch for k, ch in enumerate(text))
            cls = clips.classify(R, p, side, m, t)[0]
            assert (cls == "contiguous") == (bad <= allowed), (side, m, bad, cls)
    # N in the text is neither a match nor a mismatch
    text = "N" * 3 + R[103:100 + m]
    assert clips.classify(R, 100, R_, m, text)[0] == "contiguous"


def test_contiguous_outside_the_reference_and_on_odd_reference_letters():
    R = seeded_ref(200, 4)
    # a RIGHT site 10 bases in front of the end: 6 of 16 letters lie outside, each a mismatch
    assert clips.classify(R, 190, R_, 16, R[190:200] + "ACGTAC")[0] != "contiguous"
    assert clips.classify(R, 190, R_, 10, R[190:200])[0] == "contiguous"
    assert clips.classify(R, 4, L, 16, "ACGTACGTACGT" + R[0:4])[0] != "contiguous"
    Rn = R[:100] + "NN" + R[102:]
    text = R[96:112]
    assert clips.classify(Rn, 96, R_, 16, text)[0] == "contiguous"          # two mismatches on the reference's N: 16 // 8
    Rn3 = R[:100] + "NNN" + R[103:]
    assert clips.classify(Rn3, 96, R_, 16, text)[0] != "contiguous"


def test_short_novel_repeat():
    R = seeded_ref(400, 5)
    unit = R[300:316]
    Rr = R[:50] + unit + R[66:]                                   # the 16-mer twice
    foreign = "ACGT" * 4
    assert foreign not in R and R.count(unit) == 1 and Rr.count(unit) == 2
    assert clips.classify(R, 100, R_, 11, R[200:211]) == ("short", None, None)
    assert clips.classify(R, 100, R_, 16, R[200:205] + "N" + R[206:216]) == ("short", None, None)
    assert clips.classify(R, 100, R_, 16, foreign) == ("novel", None, None)
    assert clips.classify(Rr, 100, R_, 16, unit) == ("repeat", None, None)
    assert clips.classify(R, 100, R_, 12, R[200:212])[0] == "deletion"      # 12 is long enough


# ---- junctions from reads -------------------------------------------------------------------------------------------------------
def junction_batch(R, right, left, rng, clip=40, aligned=60):
    """Reads of a sample that differs from R by one event, their CIGARs written directly.  right = (end of the aligned bases on R,
    where the sample goes on), left = (start of the aligned bases on R, where the sample came from): [n reads, n reverse] each."""
    segs = []
    (r_end, r_next, r_n, r_rev), (l_start, l_prev, l_n, l_rev) = right, left
    for k in range(r_n):
        segs.append(U.seg(r_end - aligned, [(0, aligned), (4, clip)], rng, flag=0x10 if k < r_rev else 0, seq=R[r_end - aligned:r_end] + R[r_next:r_next + clip]))
    for k in range(l_n):
        segs.append(U.seg(l_start, [(4, clip), (0, aligned)], rng, flag=0x10 if k < l_rev else 0, seq=R[l_prev - clip:l_prev] + R[l_start:l_start + aligned]))
    return ReadBatch.from_segments(segs)


def no_homology_ref(seed, n=600, s=240, length=120):
    """A seeded reference whose interval [s, s + length) has no microhomology on either side."""
    while True:
        R = seeded_ref(n, seed)
        if R[s - 1] != R[s + length - 1] and R[s] != R[s + length]:
            return R
        seed += 1000


def test_deletion_without_microhomology_from_either_side():
    R = no_homology_ref(7)
    rng = np.random.default_rng(1)
    batch = junction_batch(R, (240, 360, 9, 4), (360, 240, 7, 2), rng)
    table, scalars = U.tables(batch, 600, 10)
    sites = clips.find_sites(table, R.lower(), 2)                   # (the reference is upper-cased inside)
    assert [(s.p, s.side, s.reads, s.rev, s.m, s.cls, s.partner, s.interval) for s in sites] == \
        [(240, R_, 9, 4, 16, "deletion", 360, (240, 120)), (360, L, 7, 2, 16, "deletion", 239, (240, 120))]
    assert sites[0].text == R[360:376] and sites[1].text == R[224:240]
    depth = np.arange(600)
    rows = clips.find_junctions(sites, 600, depth)
    assert rows == [dict(kind="deletion", start=241, end=360, length=120, right_reads=9, right_reverse=4, left_reads=7, left_reverse=2,
                         flank_depth_left=239, flank_depth_right=360)]
    assert clips.find_junctions(sites, 600)[0]["flank_depth_left"] is None
    # a threshold above one side's reads: the junction is seen from the other side alone
    rows = clips.find_junctions(clips.find_sites(table, R, 8), 600, depth)
    assert len(rows) == 1 and (rows[0]["right_reads"], rows[0]["left_reads"]) == (9, 0)


def test_deletion_with_microhomology_is_one_junction():
    """R[s : s + 3] == R[s + len : s + len + 3]: an aligner working from the left carries the alignment through the repeat (the RIGHT
    site lies at s + 3), one working from the right stops at s + len.  Both sides must land on ONE key."""
    s, length = 240, 120
    R = no_homology_ref(11)
    R = R[:s + length] + R[s:s + 3] + R[s + length + 3:]
    if R[s + 3] == R[s + length + 3]:
        R = R[:s + length + 3] + {"A": "C", "C": "G", "G": "T", "T": "A"}[R[s + 3]] + R[s + length + 4:]
    assert R[s:s + 3] == R[s + length:s + length + 3] and R[s - 1] != R[s + length - 1] and R[s + 3] != R[s + length + 3]
    rng = np.random.default_rng(2)
    batch = junction_batch(R, (s + 3, s + length + 3, 6, 1), (s + length, s, 5, 5), rng)
    table, _ = U.tables(batch, 600, 10)
    sites = clips.find_sites(table, R, 2)
    assert [(x.p, x.side, x.cls) for x in sites] == [(s + 3, R_, "deletion"), (s + length, L, "deletion")]
    assert [x.interval for x in sites] == [(s, length), (s, length)]
    rows = clips.find_junctions(sites, 600)
    assert len(rows) == 1
    assert (rows[0]["start"], rows[0]["end"], rows[0]["right_reads"], rows[0]["left_reads"], rows[0]["left_reverse"]) == (s + 1, s + length, 6, 5, 5)


def test_tandem_duplication():
    R = no_homology_ref(13, s=200, length=80)
    a, b = 200, 280                                               # the sample has R[a:b] twice
    rng = np.random.default_rng(3)
    batch = junction_batch(R, (b, a, 5, 2), (a, b, 4, 1), rng)
    table, _ = U.tables(batch, 600, 10)
    sites = clips.find_sites(table, R, 2)
    assert [(x.p, x.side, x.cls, x.interval) for x in sites] == [(a, L, "duplication", (a, b - a)), (b, R_, "duplication", (a, b - a))]
    rows = clips.find_junctions(sites, 600, np.full(600, 7))
    assert rows == [dict(kind="duplication", start=a + 1, end=b, length=b - a, right_reads=5, right_reverse=2, left_reads=4, left_reverse=1,
                         flank_depth_left=7, flank_depth_right=7)]


def test_placement_ending_on_the_last_base_and_flank_outside():
    R = no_homology_ref(17, n=400, s=300, length=84)              # [300, 384): what follows is the reference's last 16 bases
    rng = np.random.default_rng(4)
    batch = junction_batch(R, (300, 384, 4, 0), (384, 300, 0, 0), rng, clip=16)
    table, _ = U.tables(batch, 400, 10)
    sites = clips.find_sites(table, R, 2)
    assert [(x.p, x.side, x.cls, x.partner, x.text) for x in sites] == [(300, R_, "deletion", 384, R[384:400])]
    # a deletion that reaches the reference's end: no base behind it, no depth there
    sites[0].interval = (316, 84)
    row = clips.find_junctions(sites, 400, np.ones(400, np.int64))[0]
    assert (row["end"], row["flank_depth_left"], row["flank_depth_right"]) == (400, 1, None)


def test_junction_order():
    mk = lambda p, side, reads, interval, cls="deletion": clips.Site(p, side, reads, 0, 16, "A" * 16, cls, 0, interval)
    sites = [mk(10, R_, 3, (10, 50)), mk(90, R_, 9, (90, 20)), mk(110, L, 2, (90, 20)), mk(5, R_, 3, (5, 70)), mk(5, L, 3, (5, 60)),
             mk(7, R_, 100, None, "novel")]
    rows = clips.find_junctions(sites, 1000)
    assert [(r["start"] - 1, r["length"], r["right_reads"] + r["left_reads"]) for r in rows] == [(90, 20, 11), (5, 60, 3), (5, 70, 3), (10, 50, 3)]


# ---- writers --------------------------------------------------------------------------------------------------------------------
def test_writers_exact_text():
    sites = [clips.Site(239, R_, 9, 4, 16, "ACGTACGTACGTACGT", "deletion", 360, (240, 120)),
             clips.Site(300, L, 2, 0, 0, "", "contiguous", None, None)]
    f = io.StringIO()
    clips.write_sites(f, "REF", sites)
    assert f.getvalue() == ("#ref\tposition\tside\treads\treverse_reads\tconsensus\tclass\tpartner\n"
                            "REF\t240\tright\t9\t4\tACGTACGTACGTACGT\tdeletion\t361\n"
                            "REF\t301\tleft\t2\t0\t.\tcontiguous\t.\n")
    rows = clips.find_junctions(sites, 600, None)
    f = io.StringIO()
    clips.write_junctions(f, "REF", rows)
    assert f.getvalue() == ("#ref\tkind\tstart\tend\tlength\tright_reads\tright_reverse\tleft_reads\tleft_reverse\tflank_depth_left\tflank_depth_right\n"
                            "REF\tdeletion\t241\t360\t120\t9\t4\t0\t0\t.\t.\n")
    sec = clips.section(10, 2, np.array([50, 3, 7, 9], np.uint64), sites, rows)
    assert list(sec) == ["clip_min", "min_reads", "scanned", "skipped", "left", "right", "sites", "sites_by_class", "junctions"]
    assert sec["sites"] == 2 and sec["sites_by_class"] == dict(contiguous=1, short=0, novel=0, repeat=0, deletion=1, duplication=0)
    assert (sec["scanned"], sec["skipped"], sec["left"], sec["right"]) == (50, 3, 7, 9) and sec["junctions"] == rows
    assert sec["junctions"][0]["flank_depth_left"] is None


# ---- the merge of the ranks' tables -----------------------------------------------------------------------------------------------
def test_wire_round_trip_and_merge():
    G = 700
    a = U.tables(U.wave_batch("mixed", 200, G, 1), G, 10)
    b = U.tables(U.wave_batch("one_site", 100, G, 2), G, 10)
    wire = clips.to_wire(*a) + clips.to_wire(*b)                  # what the all-reduce of two ranks leaves on each
    assert wire.dtype == np.int64 and wire.size == (G + 1) * 2 * abi.CLIP_CELLS + 4
    table, scalars = clips.from_wire(wire, G)
    assert np.array_equal(table, a[0].astype(np.uint64) + b[0]) and np.array_equal(scalars, a[1] + b[1])
    m = clips.merge_tables([a, b])
    assert np.array_equal(m[0], table) and np.array_equal(m[1], scalars)
    both = ReadBatch.from_segments(U.wave_batch("mixed", 200, G, 1).segments() + U.wave_batch("one_site", 100, G, 2).segments())
    whole = U.tables(both, G, 10)
    assert np.array_equal(whole[0], table) and np.array_equal(whole[1], scalars)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
BASE = ["variants", "-i", "in.bam", "-r", "ref.fas", "-o", "out.vcf"]


@pytest.mark.parametrize("extra,message", [
    (["--qc_clips"], "--qc_clips needs --qc"),
    (["--qc_clip_min", "12"], "--qc_clip_min and --qc_clip_reads need"),
    (["--qc_clip_reads", "3"], "--qc_clip_min and --qc_clip_reads need"),
    (["--qc", "q.json", "--qc_clip_min", "12"], "--qc_clip_min and --qc_clip_reads need"),
])
def test_command_line_argument_errors(capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        amplipy.main(BASE + extra)
    assert e.value.code != 0 and message in capsys.readouterr().err


@pytest.mark.parametrize("kw,message", [
    (dict(qc_clips=True), "needs --qc"),
    (dict(qc_clip_min=12), "without clip sites"),
    (dict(qc_clip_reads=3), "without clip sites"),
    (dict(qc_junction_fn="j.tsv", qc_clip_min=0), "between 1 and 64"),
    (dict(qc_junction_fn="j.tsv", qc_clip_min=65), "between 1 and 64"),
    (dict(qc_clip_fn="c.tsv", qc_clip_reads=0), "must be >= 1"),
])
def test_run_amplipy_argument_errors(capsys, kw, message):
    with pytest.raises(SystemExit) as e:
        amplipy.run_amplipy(trimmed_reads_fn="in.bam", reference_fn="ref.fas", variants_fn="out.vcf", run_variants=True, **kw)
    assert e.value.code != 0 and message in capsys.readouterr().err


def test_new_keywords_default_to_off():
    import inspect
    p = inspect.signature(amplipy.run_amplipy).parameters
    assert [p[k].default for k in ("qc_clips", "qc_clip_fn", "qc_junction_fn", "qc_clip_min", "qc_clip_reads")] == [False, None, None, None, None]
    a = amplipy.parse_args(BASE)
    assert (a.qc_clips, a.qc_clip_out, a.qc_junction_out, a.qc_clip_min, a.qc_clip_reads) == (False, None, None, None, None)
