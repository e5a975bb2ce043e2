"""Host side of the per-amplicon allele counts (amplipy_amd/amplicon.py): the loader of the amplicon
file with its merges and errors, spans and owner tables against a position-by-position rule, the seven INFO keys with their '.'
rules and AMP_P against exact Fraction arithmetic, the TSV writer, the addition to the QC report, and the command line's
argument errors.  No GPU needed."""
import io
import json
import math
from fractions import Fraction

import numpy as np
import pytest

from amplipy_amd import amplicon, amplipy, calling, qc, strand
from tests import amplicon_util as A
from tests import qc_util as Q


def write(path, text):
    path.write_text(text)
    return str(path)


BED = "\n".join("ref\t%d\t%d\t%s" % r for r in [
    (100, 120, "a_LEFT"), (95, 118, "a_LEFT_alt"), (400, 420, "a_RIGHT"), (330, 350, "b_LEFT"), (640, 660, "b_RIGHT"), (650, 672, "b_RIGHT_alt"),
    (100, 120, "a_LEFT"), (700, 720, "lonely")]) + "\n"


# ---- the loader ---------------------------------------------------------------------------------------------------------------
def test_loader_merges_by_third_column_and_resolves_duplicate_rows(tmp_path):
    bed = write(tmp_path / "p.bed", BED)
    pairs = write(tmp_path / "a.tsv", "a_LEFT\ta_RIGHT\tA\na_LEFT_alt\ta_RIGHT\tA\n\nb_LEFT\tb_RIGHT\nb_LEFT\tb_RIGHT_alt\n")
    rows = qc.load_primer_rows(bed)
    s = amplicon.load_amplicons(pairs, rows, 0, 1000)
    assert s.names == ["A", "b_LEFT"] and s.n == 2                       # order of first appearance; the default name is the left primer's
    assert list(s.lo) == [95, 330] and list(s.hi) == [420, 672] and s.cells == 325 + 342 and list(s.cell_off) == [0, 325, 667]
    assert [(r[2], r[3]) for r in s.left_rows] == [("a_LEFT_alt", 0), ("a_LEFT", 0), ("a_LEFT", 0), ("b_LEFT", 1)]      # both rows named a_LEFT
    assert [(r[2], r[3]) for r in s.right_rows] == [("a_RIGHT", 0), ("b_RIGHT", 1), ("b_RIGHT_alt", 1)]
    assert len(s.primers) == 8                                           # lonely is allowed and belongs to no amplicon
    assert s.amp_start[700] == -1 and s.amp_end[700] == -1
    with5 = amplicon.load_amplicons(pairs, rows, 5, 1000)
    assert list(with5.lo) == [90, 325] and list(with5.hi) == [425, 677]
    at_ends = amplicon.load_amplicons(pairs, rows, 200, 600)
    assert list(at_ends.lo) == [0, 130] and list(at_ends.hi) == [600, 600]
    # the restatement reads the same file the same way
    r = A.Amps([("a_LEFT", "a_RIGHT", "A"), ("a_LEFT_alt", "a_RIGHT", "A"), ("b_LEFT", "b_RIGHT", None), ("b_LEFT", "b_RIGHT_alt", None)], rows, 5, 1000,
               owners=Q.primer_owners_slow)
    assert r.names == with5.names and r.lo == list(with5.lo) and r.hi == list(with5.hi)
    assert np.array_equal(r.amp_start, with5.amp_start) and np.array_equal(r.amp_end, with5.amp_end)


@pytest.mark.parametrize("text, message", [
    ("a_LEFT\tnobody\n", "no primer named nobody"),
    ("a_LEFT\ta_RIGHT\tA\na_LEFT\tb_RIGHT\tB\n", "used in two amplicons"),
    ("a_LEFT\ta_RIGHT\nb_LEFT\ta_LEFT\n", "used in two amplicons or as left and right"),
    ("a_LEFT\ta_RIGHT\tmy amplicon\n", "Amplicon name"),
    ("a_LEFT\ta_RIGHT\tx,y\n", "Amplicon name"), ("a_LEFT\ta_RIGHT\tx;y\n", "Amplicon name"), ("a_LEFT\ta_RIGHT\tx=y\n", "Amplicon name"),
    ("a_LEFT\ta_RIGHT\tx|y\n", "Amplicon name"),
    ("", "No amplicon"), ("\n\n", "No amplicon"),
    ("a_LEFT\n", "Invalid amplicon line"),
    ("a_RIGHT\ta_LEFT\n", "end at or in front of"),                     # lo >= hi
])
def test_loader_errors(tmp_path, capsys, text, message):
    bed = write(tmp_path / "p.bed", BED)
    with pytest.raises(SystemExit) as e:
        amplicon.load_amplicons(write(tmp_path / "a.tsv", text), qc.load_primer_rows(bed), 0, 1000)
    assert e.value.code == 1 and message in capsys.readouterr().err


def test_example_bed_pairs_into_343_amplicons():
    """343 amplicons with spans of 116..255 bases.  The spans add up to 49,939 positions: no primer name of the BED has two
    different intervals, so first row, last row, smallest start and largest end all give this sum."""
    rows = A.example_rows()
    pairs = A.example_pairs(rows)
    amps = A.example_amps()
    assert len(pairs) == amps.n == 343 and amps.cells == 49939
    assert len({n: None for _, _, n in rows}) == len({(s, e, n) for s, e, n in rows}) == 688 and len(rows) == 690
    spans = [h - l for l, h in zip(amps.lo, amps.hi)]
    assert min(spans) == 116 and max(spans) == 255
    named = {n for p in pairs for n in p[:2]}
    assert sorted(n for _, _, n in rows if n not in named) == sorted(n for _, _, n in rows if n.endswith(("M1F", "M2F")))
    s = amplicon.build_amplicons([(l, r, l) for l, r, _ in pairs], rows, 0, 29903)
    assert s.names == amps.names and list(s.lo) == amps.lo and list(s.hi) == amps.hi
    assert np.array_equal(s.amp_start, amps.amp_start) and np.array_equal(s.amp_end, amps.amp_end)


# ---- owner tables -------------------------------------------------------------------------------------------------------------
def slow_tables(ref_len, left, right, offset):
    """Position by position: amp_start[p] is the amplicon of the left-role primer covering p (start - offset <= p < end +
    offset) with the largest end, amp_end[p] that of the right-role primer covering p with the smallest start; ties go to the
    first row in ascending (start, end)."""
    st, en = [], []
    for p in range(ref_len):
        cl = [r for r in left if r[0] - offset <= p < r[1] + offset]
        cr = [r for r in right if r[0] - offset <= p < r[1] + offset]
        st.append(min(cl, key=lambda r: -r[1])[3] if cl else -1)
        en.append(min(cr, key=lambda r: r[0])[3] if cr else -1)
    return np.array(st, np.int32), np.array(en, np.int32)


SETS = {
    # a right primer of X and a left primer of Y cover the same positions
    "shared": [((10, 30), (200, 225)), ((205, 230), (400, 420))],
    "nested": [((10, 30), (400, 420)), ((100, 120), (300, 320)), ((15, 25), (405, 415))],
    "identical": [((10, 30), (200, 220)), ((10, 30), (200, 220))],
    "both_ends": [((0, 20), (100, 120)), ((380, 400), (480, 500))],
}


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("name", sorted(SETS))
def test_owner_tables_position_by_position(name, offset):
    G = 500
    rows = []
    for k, (l, r) in enumerate(SETS[name]):
        rows += [(l[0], l[1], "L%d" % k), (r[0], r[1], "R%d" % k)]
    rows.sort(key=lambda x: (x[0], x[1]))
    s = amplicon.build_amplicons([("L%d" % k, "R%d" % k, "amp%d" % k) for k in range(len(SETS[name]))], rows, offset, G)
    st, en = slow_tables(G, s.left_rows, s.right_rows, offset)
    assert np.array_equal(s.amp_start, st) and np.array_equal(s.amp_end, en)
    assert list(s.lo) == [max(0, l[0] - offset) for l, _ in SETS[name]] and list(s.hi) == [min(G, r[1] + offset) for _, r in SETS[name]]
    r = A.simple_amps(G, SETS[name], offset)[0]
    assert np.array_equal(r.amp_start, st) and np.array_equal(r.amp_end, en) and r.lo == list(s.lo) and r.hi == list(s.hi)
    if name == "shared":        # the role split: position 210 is the end of amplicon 0 and the start of amplicon 1
        assert s.amp_end[210] == 0 and s.amp_start[210] == 1
    if name == "identical":
        assert set(s.amp_start[10:30]) == {0} and set(s.amp_end[200:220]) == {0}
    if name == "both_ends":
        assert s.amp_start[0] == 0 and s.amp_end[G - 1] == 1 and s.lo[0] == 0 and s.hi[1] == G


# ---- the keys -----------------------------------------------------------------------------------------------------------------
def fisher_exact(a, b, c, d):
    n, r1, c1 = a + b + c + d, a + b, a + c
    if n == 0:
        return Fraction(1)
    w = {x: math.comb(r1, x) * math.comb(n - r1, c1 - x) for x in range(max(0, c1 - (n - r1)), min(r1, c1) + 1)}
    return Fraction(sum(v for v in w.values() if v <= w[a]), math.comb(n, c1))


def key_tables():
    """Three amplicons on a reference of 600: X [10, 300), Y [200, 500), Z [250, 420); position 5 and 550 lie in none, 260 in
    all three.  Y has no depth at 260; 270 has depth in all three."""
    pairs = [((10, 30), (280, 300)), ((200, 220), (480, 500)), ((250, 270), (400, 420))]
    r, rows = A.simple_amps(600, pairs)
    s = amplicon.build_amplicons([("L%d" % k, "R%d" % k, "XYZ"[k]) for k in range(3)], rows, 0, 600)
    amp_counts = np.zeros((s.cells, 6), np.uint32)
    counts = np.zeros((600, 6), np.uint32)
    cell = lambda a, p: amp_counts[int(s.cell_off[a]) + p - int(s.lo[a])]
    cell(0, 260)[:] = [120, 3, 0, 0, 0, 1]; cell(2, 260)[:] = [0, 1, 0, 0, 0, 0]
    counts[260] = [125, 4, 0, 0, 0, 1]                                   # 5 A from reads of no amplicon
    cell(0, 270)[:] = [50, 0, 10, 0, 0, 0]; cell(1, 270)[:] = [50, 0, 0, 0, 0, 0]; cell(2, 270)[:] = [70, 0, 1, 0, 0, 2]
    counts[270] = [170, 0, 11, 0, 0, 2]
    cell(0, 100)[:] = [7, 0, 0, 2, 0, 0]
    counts[100] = [7, 0, 0, 2, 0, 0]
    counts[5] = [3, 1, 0, 0, 0, 0]
    reads = np.array([10, 20, 0, 4], np.uint64)
    r.names = s.names
    return s, r, rows, amplicon.Tables(s, counts, amp_counts, reads)


def parse(info):
    return dict(kv.split("=", 1) for kv in info.split(";"))


def test_keys_and_their_dot_rules():
    s, r, rows, t = key_tables()
    restated = lambda pos, ref, alts: A.info_text(A.keys(pos, ref, alts, r, rows, t.counts, t.amp_counts, strand.fisher_two_sided))
    # three amplicons, zero depth in one of them
    k = parse(t.info(260, "A", ["C", "-"]))
    assert list(k) == list(amplicon.KEYS)
    assert k == {"AMP": "X,Y,Z", "AMP_DP": "124,0,1", "AMP_REF_DP": "120,0,0", "AMP_ALT_DP": "3|0|1,1|0|0", "AMP_NA_DP": "5",
                 "AMP_P": k["AMP_P"], "PRIMER": "L2"}
    want = [fisher_exact(3, 121, 1, 0), fisher_exact(1, 123, 0, 1)]      # X and Z: the two of largest depth
    for got, w in zip(k["AMP_P"].split(","), want):
        assert abs(Fraction(float(got)) - w) <= w * Fraction(6, 10 ** 4)    # %.4g keeps four digits: 5e-4 relative, and 1e-9 of the lgamma sums
    assert t.info(260, "A", ["C", "-"]) == restated(260, "A", ["C", "-"])
    # depth in three: the two of largest AMP_DP are Z (73) and X (60); an insertion allele has no per-amplicon depth
    k = parse(t.info(270, "A", ["G", "AGT", "-"]))
    assert k["AMP_DP"] == "60,50,73" and k["AMP_ALT_DP"] == "10|0|1,.,0|0|2" and k["AMP_NA_DP"] == "0" and k["PRIMER"] == "."
    p = k["AMP_P"].split(",")
    assert p[1] == "." and abs(Fraction(float(p[0])) - fisher_exact(1, 72, 10, 50)) <= fisher_exact(1, 72, 10, 50) * Fraction(6, 10 ** 4)
    assert t.info(270, "A", ["G", "AGT", "-"]) == restated(270, "A", ["G", "AGT", "-"])
    # ties in AMP_DP go to the earlier amplicon
    t.amp_counts[int(s.cell_off[1]) + 270 - 200] = [60, 0, 0, 0, 0, 0]
    t.amp_counts[int(s.cell_off[2]) + 270 - 250] = [59, 0, 1, 0, 0, 0]
    t.counts[270] = [169, 0, 11, 0, 0, 0]
    k = parse(t.info(270, "A", ["G"]))
    assert k["AMP_DP"] == "60,60,60" and k["AMP_P"] == "%.4g" % strand.fisher_two_sided(10, 50, 0, 60)
    assert t.info(270, "A", ["G"]) == restated(270, "A", ["G"])
    # one amplicon: no pair for AMP_P; a position inside a primer
    k = parse(t.info(100, "A", ["T"]))
    assert k == {"AMP": "X", "AMP_DP": "9", "AMP_REF_DP": "7", "AMP_ALT_DP": "2", "AMP_NA_DP": "0", "AMP_P": ".", "PRIMER": "."}
    assert parse(t.info(15, "A", ["T"]))["PRIMER"] == "L0" and parse(t.info(215, "A", ["T"]))["AMP"] == "X,Y"
    # no amplicon at all
    k = parse(t.info(5, "A", ["C", "CA"]))
    assert k == {"AMP": ".", "AMP_DP": ".", "AMP_REF_DP": ".", "AMP_ALT_DP": ".,.", "AMP_NA_DP": "4", "AMP_P": ".,.", "PRIMER": "."}
    # a reference letter that is none of A C G T N
    assert parse(t.info(260, "R", ["C"]))["AMP_REF_DP"] == "." and parse(t.info(260, "N", ["C"]))["AMP_REF_DP"] == "0,0,0"
    for pos, ref, alts in ((5, "A", ["C", "CA"]), (100, "A", ["T"]), (260, "R", ["C"]), (260, "N", ["C"]), (15, "G", ["-"])):
        assert t.info(pos, ref, alts) == restated(pos, ref, alts)


def test_primer_key_lists_duplicates_once_in_bed_order(tmp_path):
    rows = qc.load_primer_rows(write(tmp_path / "p.bed", BED))
    s = amplicon.load_amplicons(write(tmp_path / "a.tsv", "a_LEFT\ta_RIGHT\n"), rows, 0, 1000)
    t = amplicon.Tables(s, np.zeros((1000, 6), np.uint32), np.zeros((s.cells, 6), np.uint32), np.zeros(2, np.uint64))
    assert parse(t.info(110, "A", ["C"]))["PRIMER"] == "a_LEFT_alt,a_LEFT"         # (95, 118) sorts first; the two a_LEFT rows once
    assert parse(t.info(119, "A", ["C"]))["PRIMER"] == "a_LEFT" and parse(t.info(120, "A", ["C"]))["PRIMER"] == "."
    assert parse(t.info(655, "A", ["C"]))["PRIMER"] == "b_RIGHT,b_RIGHT_alt" and parse(t.info(655, "A", ["C"]))["AMP"] == "."


def test_vcf_line_carries_the_keys_behind_the_strand_keys():
    s, r, rows, t = key_tables()
    rec = calling.VariantRecord(260, "A", ["C", "-"], 130, 125, [4, 1], 125 / 130, [4 / 130, 1 / 130], (0, 1, 2))
    plain = calling.vcf_line("ref", rec)
    line = calling.vcf_line("ref", rec, None, t)
    f = line.rstrip("\n").split("\t")
    kvs = f[7].split(";")
    assert [kv.split("=")[0] for kv in kvs[-7:]] == list(amplicon.KEYS) and kvs[-8].startswith("ALT_FREQ=")
    assert ";".join(kvs[-7:]) == t.info(260, "A", ["C", "-"])
    f[7] = ";".join(kvs[:-7])
    assert "\t".join(f) + "\n" == plain
    st = strand.Tables(t.counts, np.zeros((600, 6), np.uint32), np.zeros((600, 5), np.uint64))
    both = calling.vcf_line("ref", rec, st, t).split("\t")[7].split(";")
    assert [kv.split("=")[0] for kv in both[-12:]] == list(strand.KEYS) + list(amplicon.KEYS)


def test_vcf_writer_header(tmp_path, monkeypatch):
    import sys
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    texts = {}
    for tag, kw in (("off", {}), ("amp", dict(amplicon=True)), ("both", dict(strand=True, amplicon=True))):
        fn = str(tmp_path / (tag + ".vcf"))
        amplipy.VcfWriter(fn, "ref", **kw).close()
        texts[tag] = open(fn).read()
    assert texts["amp"].replace(amplicon.HEADER_LINES, "") == texts["off"] and amplicon.HEADER_LINES in texts["amp"]
    assert texts["both"].index(strand.HEADER_LINES) < texts["both"].index(amplicon.HEADER_LINES) < texts["both"].index("#CHROM")
    assert [l.split("ID=")[1].split(",")[0] for l in amplicon.HEADER_LINES.splitlines()] == list(amplicon.KEYS)


# ---- the TSV and the report ---------------------------------------------------------------------------------------------------
def test_tsv_and_report():
    s, r, rows, t = key_tables()
    f = io.StringIO()
    amplicon.write_tsv(f, "ref", t)
    lines = f.getvalue().splitlines()
    assert lines[0] == "#amplicon\tref\tpos\tA\tC\tG\tT\tN\tdel" and len(lines) == 1 + s.cells
    assert lines[1] == "X\tref\t11\t0\t0\t0\t0\t0\t0" and lines[1 + 250] == "X\tref\t261\t120\t3\t0\t0\t0\t1"
    assert lines[1 + 290] == "Y\tref\t201\t0\t0\t0\t0\t0\t0" and lines[-1].startswith("Z\tref\t420\t")
    report = {"amplipy_qc": 1, "params": {}, "reads": {"rows": 40, "errors": 6}, "primers": [], "regions": []}
    before = json.dumps(report)
    amplicon.add_to_report(report, t)
    assert list(report)[-1] == "amplicons" and list(report["reads"])[-1] == "no_amplicon" and report["reads"]["no_amplicon"] == 4
    assert report["amplicons"][0] == {"name": "X", "start": 10, "end": 300, "reads": 10, "bases": 124 + 60 + 9}
    assert [a["reads"] for a in report["amplicons"]] == [10, 20, 0]
    del report["amplicons"], report["reads"]["no_amplicon"]
    assert json.dumps(report) == before
    assert t.summary_line() == "Amplicons: 30 of 34 reads assigned; 1 of 3 amplicons without a read"


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, message", [
    (["trim", "-p", "p.bed", "-r", "r.fas", "--amplicons", "a.tsv"], "aio only"),
    (["variants", "-r", "r.fas", "--amplicons", "a.tsv"], "aio only"),
    (["consensus", "-r", "r.fas", "--amplicons", "a.tsv", "--amplicon_out", "o.tsv"], "aio only"),
    (["variants", "-r", "r.fas", "--amplicon_out", "o.tsv"], "needs the amplicon file"),
    (["aio", "-p", "p.bed", "-r", "r.fas", "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas", "--amplicon_out", "o.tsv"], "needs the amplicon file"),
])
def test_argument_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        amplipy.main(argv)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert message in err
    if message == "aio only":
        assert "original coordinates" in err                        # the message says why


def test_flags_are_long_only_and_off_by_default():
    for argv in (["trim", "-p", "p", "-r", "r"], ["variants", "-r", "r"], ["consensus", "-r", "r"],
                 ["aio", "-p", "p", "-r", "r", "-ot", "t", "-ov", "v", "-oc", "c"]):
        a = amplipy.parse_args(argv)
        assert a.amplicons is None and a.amplicon_out is None
    a = amplipy.parse_args(["aio", "-p", "p", "-r", "r", "-ot", "t", "-ov", "v", "-oc", "c", "--amplicons", "a.tsv", "--amplicon_out", "o.tsv.gz"])
    assert a.amplicons == "a.tsv" and a.amplicon_out == "o.tsv.gz"
