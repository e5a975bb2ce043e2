"""Host side of the strand tallies (amplipy_amd/strand.py): Fisher's exact test against exact rational
arithmetic, the INFO keys of a VCF line with their '.' rules, the TSV writer, the wire format of the all-reduce, and the
command line's argument errors.  No GPU needed."""
import gzip
import math
from fractions import Fraction

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, qc, strand


# ---- Fisher's exact test ------------------------------------------------------------------------------------------------------
def fisher_exact(a, b, c, d):
    """The same definition in Fractions: tables with the same margins whose probability is <= the observed one (exactly)."""
    n, r1, c1 = a + b + c + d, a + b, a + c
    if n == 0:
        return Fraction(1)
    den = math.comb(n, c1)
    w = {x: math.comb(r1, x) * math.comb(n - r1, c1 - x) for x in range(max(0, c1 - (n - r1)), min(r1, c1) + 1)}
    return Fraction(sum(v for v in w.values() if v <= w[a]), den)


TABLES = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 7), (1, 1, 1, 1), (3, 0, 0, 3), (2, 5, 7, 1), (10, 10, 10, 10), (12, 0, 9, 0), (0, 12, 0, 9),
          (5, 5, 0, 0), (8, 2, 1, 5), (1, 9, 11, 3), (100, 100, 3, 0), (100, 100, 0, 30), (500, 480, 20, 2), (1000, 1000, 25, 25),
          (2000, 2000, 30, 30), (400, 400, 400, 400), (2000, 1900, 60, 0), (1999, 2000, 19, 25), (2000, 3, 5, 0), (1500, 1500, 40, 41), (7, 2000, 0, 7),
          (1200, 800, 800, 1200), (2000, 1700, 17, 20), (1300, 2000, 200, 140), (6, 6, 6, 6), (4, 4, 4, 5)]


@pytest.mark.parametrize("t", TABLES, ids=lambda t: "_".join(map(str, t)))
def test_fisher_against_exact_fractions(t):
    """Relative tolerance 1e-9: lgamma is good to a few ulp, and at arguments <= 1e4 the error of a log-probability stays near
    1e-11.  Ties are exact in the Fractions; symmetric tables (equal probabilities on both sides) check the tie rule."""
    want = fisher_exact(*t)
    assert want > Fraction(1, 10 ** 290)              # (the tables are chosen inside the range of a double)
    got = strand.fisher_two_sided(*t)
    assert 0.0 <= got <= 1.0
    assert abs(Fraction(got) - want) <= want * Fraction(1, 10 ** 9), (got, float(want))
    # the p-value does not depend on which margin is called rows, nor on the order of rows or columns
    a, b, c, d = t
    for u in ((a, c, b, d), (c, d, a, b), (b, a, d, c)):
        assert math.isclose(strand.fisher_two_sided(*u), got, rel_tol=1e-9, abs_tol=0.0)


def test_fisher_on_seeded_small_tables():
    """400 seeded tables with entries up to 60 (many ties, empty rows and columns, observed values at, next to and far from
    the mode) against the exact fractions, and one table of depth 20,000 against the plain sum of all its lgamma terms."""
    rng = np.random.default_rng(12)
    for _ in range(400):
        t = tuple(int(v) for v in rng.integers(0, int(rng.choice([3, 8, 61])), size=4))
        want = fisher_exact(*t)
        assert abs(Fraction(strand.fisher_two_sided(*t)) - want) <= want * Fraction(1, 10 ** 9), t
    a, b, c, d = 9000, 9400, 900, 700
    n, r1, c1 = a + b + c + d, a + b, a + c
    lc = lambda n_, k: math.lgamma(n_ + 1) - math.lgamma(k + 1) - math.lgamma(n_ - k + 1)
    logp = [lc(r1, x) + lc(n - r1, c1 - x) - lc(n, c1) for x in range(max(0, c1 - (n - r1)), min(r1, c1) + 1)]
    plain = math.fsum(math.exp(v) for v in logp if v <= logp[a - max(0, c1 - (n - r1))] + math.log1p(strand.TIE))
    assert strand.fisher_two_sided(a, b, c, d) == pytest.approx(plain, rel=1e-9) and 1e-12 < plain < 1e-3


def test_fisher_known_values_and_errors():
    assert strand.fisher_two_sided(3, 0, 0, 3) == pytest.approx(0.1, rel=1e-12)
    assert strand.fisher_two_sided(1, 1, 1, 1) == pytest.approx(1.0, rel=1e-12) and strand.fisher_two_sided(0, 0, 0, 0) == 1.0
    assert strand.fisher_two_sided(2000, 0, 0, 2000) < 1e-300
    assert strand.fisher_two_sided(np.uint32(8), np.uint32(2), np.int64(1), 5) == pytest.approx(float(fisher_exact(8, 2, 1, 5)), rel=1e-9)
    with pytest.raises(ValueError):
        strand.fisher_two_sided(1, -1, 2, 2)


# ---- the INFO keys --------------------------------------------------------------------------------------------------------------
def small_tables():
    counts = np.zeros((6, abi.NSYM), np.uint32); rev = np.zeros((6, abi.NSYM), np.uint32); qsum = np.zeros((6, 5), np.uint64)
    counts[0] = [90, 0, 10, 0, 0, 4]; rev[0] = [40, 0, 10, 0, 0, 1]; qsum[0] = [90 * 35 + 7, 0, 10 * 22, 0, 0]
    counts[1] = [0, 0, 0, 12, 0, 0]; rev[1] = [0, 0, 0, 5, 0, 0]; qsum[1] = [0, 0, 0, 12 * 30, 0]       # reference base never seen
    counts[2] = [7, 3, 0, 0, 2, 0]; rev[2] = [7, 0, 0, 0, 1, 0]; qsum[2] = [7 * 38, 3 * 21 + 2, 0, 0, 2 * 25]
    counts[3] = [5, 5, 0, 0, 0, 0]; rev[3] = [2, 3, 0, 0, 0, 0]; qsum[3] = [5 * 2 ** 33, 5 * 40, 0, 0, 0]
    return strand.Tables(counts, rev, qsum)


def info_dict(text):
    return dict(kv.split("=") for kv in text.split(";"))


def test_info_fields_and_dot_rules():
    t = small_tables()
    d = info_dict(t.info(0, "A", ["G", "-"]))
    assert list(d) == list(strand.KEYS)
    assert d["REF_RV"] == "40" and d["REF_QUAL"] == "35" and d["ALT_RV"] == "10,1" and d["ALT_QUAL"] == "22,."
    assert d["SB"] == "%.4g,%.4g" % (strand.fisher_two_sided(50, 40, 0, 10), strand.fisher_two_sided(50, 40, 3, 1))
    # the reference base has count 0: its values and SB are '.'
    assert info_dict(t.info(1, "A", ["T"])) == dict(REF_RV=".", ALT_RV="5", REF_QUAL=".", ALT_QUAL="30", SB=".")
    # an insertion allele, an N, and a reference letter that is none of A C G T N
    d = info_dict(t.info(2, "A", ["CAT", "C", "N"]))
    assert d["ALT_RV"] == ".,0,1" and d["ALT_QUAL"] == ".,21,25" and d["SB"].split(",")[0] == "." and d["REF_RV"] == "7"
    assert d["SB"].split(",")[1] == "%.4g" % strand.fisher_two_sided(0, 7, 3, 0)
    for ref in ("R", "-", "a", "AC"):
        assert info_dict(t.info(2, ref, ["C"])) == dict(REF_RV=".", ALT_RV="0", REF_QUAL=".", ALT_QUAL="21", SB=".")
    # an ALT whose count is 0 (only a record built by hand has one), and a mean beyond 32 bits
    assert info_dict(t.info(1, "T", ["G"])) == dict(REF_RV="5", ALT_RV=".", REF_QUAL="30", ALT_QUAL=".", SB=".")
    assert info_dict(t.info(3, "A", ["C"]))["REF_QUAL"] == str(2 ** 33)


def test_vcf_line_and_vcf_text_carry_the_keys_behind_alt_freq():
    t = small_tables()
    rec = calling.VariantRecord(0, "A", ["G", "-"], 104, 90, [10, 4], 90 / 104, [10 / 104, 4 / 104], (0, 1, 2))
    plain = calling.vcf_line("ref", rec)
    with_keys = calling.vcf_line("ref", rec, t)
    f_plain, f_keys = plain.split("\t"), with_keys.split("\t")
    assert f_keys[:7] == f_plain[:7] and f_keys[8:] == f_plain[8:]
    assert f_keys[7] == f_plain[7] + ";" + t.info(0, "A", ["G", "-"]) and f_plain[7].endswith("ALT_FREQ=%s" % rec.ALT_FREQ)
    # CallResult: the columns and an `extra` record of an insertion position; without tables the column-wise text is untouched
    ins = calling.VariantRecord(2, "A", ["CAT", "C"], 14, 7, [4, 3], 0.5, [4 / 14, 3 / 14], (0, 1, 2))
    res = calling.CallResult("ATAAAA", np.full(6, -1, np.int8), {}, np.array([0, 3], np.int32), np.array([104, 10], np.uint32), np.array([90, 5], np.uint32),
                             np.array([True, True]), np.array([2, 1], np.int8), np.array([[2, 5, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1]], np.int8),
                             np.array([[10, 4, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0]], np.uint32), {2: ins, 4: None}, None, 1)
    off = res.vcf_text("ref")
    assert off == "".join(calling.vcf_line("ref", r) for r in res.records) and off.count("\n") == 3 and "REF_RV" not in off
    on = res.vcf_text("ref", t)
    assert on == "".join(calling.vcf_line("ref", r, t) for r in res.records)
    lines = on.splitlines()
    assert "ALT_RV=.,0;" in lines[1] and lines[1].split("\t")[4] == "CAT,C"
    strip = lambda line: "\t".join(f if k != 7 else ";".join(kv for kv in f.split(";") if kv.split("=")[0] not in strand.KEYS)
                                   for k, f in enumerate(line.split("\t")))
    assert "".join(strip(l) + "\n" for l in lines) == off


def test_vcf_writer_header(tmp_path, monkeypatch):
    import sys
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    texts = {}
    for on in (False, True):
        fn = str(tmp_path / ("h%d.vcf" % on))
        w = amplipy.VcfWriter(fn, "ref", strand=on) if on else amplipy.VcfWriter(fn, "ref")
        w.close()
        texts[on] = open(fn).read()
    assert texts[True].replace(strand.HEADER_LINES, "") == texts[False] and strand.HEADER_LINES not in texts[False]
    lines = texts[True].splitlines()
    i = lines.index('##INFO=<ID=ALT_FREQ,Number=1,Type=String,Description="Frequency of alternate base">')
    assert [l.split(",")[0] for l in lines[i + 1:i + 6]] == ["##INFO=<ID=%s" % k for k in strand.KEYS] and lines[i + 6].startswith("#CHROM")
    assert [l.split(",")[2] for l in lines[i + 1:i + 6]] == ["Type=Integer", "Type=String", "Type=Integer", "Type=String", "Type=String"]


# ---- the TSV file and the wire ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s.tsv", "s.tsv.gz"])
def test_tsv_writer(tmp_path, name):
    t = small_tables()
    f = qc.open_new(str(tmp_path / name))
    strand.write_tsv(f, "re%f", t)
    f.close()
    lines = (gzip.open(str(tmp_path / name), "rt") if name.endswith(".gz") else open(str(tmp_path / name))).read().splitlines()
    assert lines[0] == "#ref\tpos\tA\tA_rv\tA_qsum\tC\tC_rv\tC_qsum\tG\tG_rv\tG_qsum\tT\tT_rv\tT_qsum\tN\tN_rv\tN_qsum\tdel\tdel_rv"
    assert len(lines) == 7 and all(len(l.split("\t")) == 19 for l in lines)
    assert lines[1] == "re%%f\t1\t90\t40\t%d\t0\t0\t0\t10\t10\t220\t0\t0\t0\t0\t0\t0\t4\t1" % (90 * 35 + 7)
    assert lines[4].split("\t")[:5] == ["re%f", "4", "5", "2", str(5 * 2 ** 33)]
    assert lines[6] == "re%f\t6" + "\t0" * 17


def test_wire_round_trip():
    rng = np.random.default_rng(4)
    rev = rng.integers(0, 2 ** 32, size=(50, 6), dtype=np.uint64).astype(np.uint32)
    qsum = rng.integers(0, 2 ** 45, size=(50, 5), dtype=np.uint64)
    w = strand.to_wire(rev, qsum)
    assert w.dtype == np.int64 and w.shape == (50 * 11,)
    r2, q2 = strand.from_wire(w + w)          # (what the all-reduce of two equal ranks gives)
    assert np.array_equal(q2, 2 * qsum) and np.array_equal(r2.astype(np.uint64), (2 * rev.astype(np.uint64)) & 0xFFFFFFFF)
    r1, q1 = strand.from_wire(w)
    assert np.array_equal(r1, rev) and np.array_equal(q1, qsum) and r1.dtype == np.uint32 and q1.dtype == np.uint64


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, message", [
    (["trim", "-p", "p.bed", "-r", "r.fas", "--strand"], "no count table"),
    (["trim", "-p", "p.bed", "-r", "r.fas", "--strand_out", "s.tsv"], "no count table"),
    (["consensus", "-r", "r.fas", "--strand"], "need a VCF"),
])
def test_argument_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        amplipy.main(argv)
    assert e.value.code == 1
    assert message in capsys.readouterr().err


@pytest.mark.parametrize("kw, message", [
    (dict(run_trim=True, strand=True), "no count table"),
    (dict(run_trim=True, strand_fn="s.tsv"), "no count table"),
    (dict(run_consensus=True, strand=True), "need a VCF"),
])
def test_run_amplipy_argument_errors(kw, message, capsys):
    with pytest.raises(SystemExit):
        amplipy.run_amplipy(**kw)
    assert message in capsys.readouterr().err


def test_flags_are_long_only_and_off_by_default():
    for argv in (["trim", "-p", "p", "-r", "r"], ["variants", "-r", "r"], ["consensus", "-r", "r"],
                 ["aio", "-p", "p", "-r", "r", "-ot", "t", "-ov", "v", "-oc", "c"]):
        a = amplipy.parse_args(argv)
        assert a.strand is False and a.strand_out is None
    a = amplipy.parse_args(["variants", "-r", "r", "--strand", "--strand_out", "s.tsv.gz"])
    assert a.strand is True and a.strand_out == "s.tsv.gz"


def test_existing_output_is_refused(tmp_path, capsys):
    fn = tmp_path / "s.tsv"
    fn.write_text("x")
    with pytest.raises(SystemExit):
        qc.open_new(str(fn))
    assert "File already exists: %s" % fn in capsys.readouterr().err
    assert fn.read_text() == "x"
