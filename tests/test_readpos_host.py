"""The host half of the read-position tallies (amplipy_amd/readpos.py): the bins, the rank-sum z against a
brute-force midrank computation in exact arithmetic, REF_END / ALT_END for every legal --readpos_end, the six INFO keys and their
'.' rules, their place behind every other hook's keys, the TSV, the wire format and every argument error.  No GPU needed."""
import gzip
import io
import math
from fractions import Fraction

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, readpos
from amplipy_amd.strand import fisher_two_sided
from tests import readpos_util as RP


def test_rp_bin_at_every_edge_and_the_constants():
    assert abi.RP_BINS == RP.BINS == 7 and abi.RP_EDGES == RP.EDGES and abi.RP_CELLS == abi.NSYM * abi.RP_BINS == 42
    for b, lo in enumerate(RP.EDGES):
        assert RP.rp_bin(lo) == b and (lo == 0 or RP.rp_bin(lo - 1) == b - 1)
    assert RP.rp_bin(1) == 0 and RP.rp_bin(63) == 5 and RP.rp_bin(64) == 6 and RP.rp_bin(10 ** 6) == 6
    assert readpos.END_CHOICES == (2, 4, 8, 16, 32, 64) and readpos.DEFAULT_END == 8
    for k, e in enumerate(readpos.END_CHOICES):
        assert readpos.end_bins(e) == k + 1
    assert len(readpos.BIN_NAMES) == 7 and len(readpos.TSV_COLUMNS) == 2 + 42


# ---- RPZ ------------------------------------------------------------------------------------------------------------------------
def brute_z2(a, r):
    """(sign, z^2) of the Mann-Whitney U of the expanded samples with midranks and the tie-corrected variance, in Fractions;
    None when a side is empty or the variance is 0."""
    xs = [b for b, n in enumerate(a) for _ in range(n)]
    ys = [b for b, n in enumerate(r) for _ in range(n)]
    n1, n2 = len(xs), len(ys)
    if n1 == 0 or n2 == 0:
        return None
    N = n1 + n2
    allv = sorted(xs + ys)
    rank = {}
    i = 0
    while i < N:
        j = i
        while j < N and allv[j] == allv[i]:
            j += 1
        rank[allv[i]] = Fraction(i + 1 + j, 2)          # the mean of ranks i + 1 .. j
        i = j
    u = sum(rank[x] for x in xs) - Fraction(n1 * (n1 + 1), 2)
    mu = Fraction(n1 * n2, 2)
    ties = sum(c ** 3 - c for c in (allv.count(v) for v in set(allv)))
    var = Fraction(n1 * n2, 12) * ((N + 1) - Fraction(ties, N * (N - 1)))
    if var == 0:
        return None
    d = u - mu
    return (d > 0) - (d < 0), d * d / var


def test_rpz_against_brute_force_midranks_on_400_seeded_pairs():
    rng = np.random.default_rng(23)
    n_neg = n_pos = 0
    for k in range(400):
        hi = [3, 12, 60][k % 3]
        a = rng.integers(0, hi, size=7) * (rng.random(7) < 0.7)
        r = rng.integers(0, hi, size=7) * (rng.random(7) < 0.7)
        want = brute_z2(a.tolist(), r.tolist())
        z = readpos.rank_sum_z(a, r)
        if want is None:
            assert z is None
            continue
        sign, z2 = want
        assert z is not None and ((z > 0) - (z < 0)) == sign
        assert math.isclose(z * z, float(z2), rel_tol=1e-12, abs_tol=1e-300)
        n_neg += z < 0; n_pos += z > 0
    assert n_neg > 50 and n_pos > 50


def test_rpz_is_none_for_one_bin_of_ties_and_an_empty_side_and_negative_nearer_the_ends():
    assert readpos.rank_sum_z([0, 0, 5, 0, 0, 0, 0], [0, 0, 9, 0, 0, 0, 0]) is None          # sigma is 0
    assert readpos.rank_sum_z([0] * 7, [1, 2, 3, 4, 5, 6, 7]) is None
    assert readpos.rank_sum_z([1, 2, 3, 4, 5, 6, 7], [0] * 7) is None
    assert readpos.rank_sum_z([9, 1, 0, 0, 0, 0, 0], [0, 0, 1, 3, 9, 9, 2]) < -3
    assert readpos.rank_sum_z([0, 0, 1, 3, 9, 9, 2], [9, 1, 0, 0, 0, 0, 0]) > 3
    assert readpos.rank_sum_z([1, 2, 3, 4, 3, 2, 1], [1, 2, 3, 4, 3, 2, 1]) == 0


# ---- the keys ---------------------------------------------------------------------------------------------------------------------
def hand_made(end=8):
    """Four positions: 0 a clean site, 1 an end-only ALT, 2 a deletion ALT and a missing reference row, 3 nothing."""
    hist = np.zeros((4, 6, 7), np.uint32)
    hist[0, 0] = [2, 2, 4, 8, 16, 20, 0]        # A, the reference base
    hist[0, 2] = [1, 1, 2, 4, 8, 10, 0]         # G
    hist[1, 1] = [3, 3, 6, 12, 24, 30, 5]       # C, the reference base
    hist[1, 3] = [14, 5, 1, 0, 0, 0, 0]         # T: only near the ends
    hist[2, 5] = [0, 1, 2, 3, 4, 0, 0]          # '-'
    hist[2, 0] = [0, 0, 0, 0, 7, 0, 0]
    return readpos.Tables(hist.sum(axis=2), hist, end)


def test_the_six_keys_of_a_record():
    t = hand_made()
    a, g = [2, 2, 4, 8, 16, 20, 0], [1, 1, 2, 4, 8, 10, 0]
    assert t.info(0, "A", ["G"]) == "REF_RP=2|2|4|8|16|20|0;ALT_RP=1|1|2|4|8|10|0;REF_END=8;ALT_END=4;RPB=%.4g;RPZ=%.3f" % (
        fisher_two_sided(8, 44, 4, 22), readpos.rank_sum_z(g, a))
    info = dict(kv.split("=") for kv in t.info(1, "C", ["T"]).split(";"))
    assert info["ALT_RP"] == "14|5|1|0|0|0|0" and info["REF_END"] == "12" and info["ALT_END"] == "20"
    assert float(info["RPB"]) < 1e-6 and float(info["RPZ"]) < -5
    assert list(dict(kv.split("=") for kv in t.info(0, "A", ["G"]).split(";"))) == list(readpos.KEYS)


def test_the_dot_rules():
    t = hand_made()
    # an insertion allele, a symbol whose count is 0
    assert t.info(0, "A", ["AGT", "G", "T"]) .split(";")[1] == "ALT_RP=.,1|1|2|4|8|10|0,."
    info = dict(kv.split("=") for kv in t.info(0, "A", ["AGT", "G", "T"]).split(";"))
    assert info["ALT_END"] == ".,4,." and info["RPB"].split(",")[0] == "." and info["RPB"].split(",")[2] == "." and info["RPZ"].split(",")[::2] == [".", "."]
    # a reference letter that is none of A C G T N, and one whose count is 0: no reference row, so RPB and RPZ are '.' too
    for ref in ("R", "G"):
        assert t.info(2, ref, ["-", "A"]) == "REF_RP=.;ALT_RP=0|1|2|3|4|0|0,0|0|0|0|7|0|0;REF_END=.;ALT_END=3,0;RPB=.,.;RPZ=.,."
    # '-' has values: a deletion has a position
    info = dict(kv.split("=") for kv in t.info(2, "A", ["-"]).split(";"))
    assert info["ALT_RP"] == "0|1|2|3|4|0|0" and info["RPB"] != "." and info["RPZ"] != "."
    # all ties in one bin: RPZ alone is '.'
    hist = np.zeros((1, 6, 7), np.uint32); hist[0, 0, 3] = 5; hist[0, 1, 3] = 4
    info = dict(kv.split("=") for kv in readpos.Tables(hist.sum(axis=2), hist).info(0, "A", ["C"]).split(";"))
    assert info["RPZ"] == "." and info["RPB"] == "1"
    # nothing at all
    assert t.info(3, "A", ["C"]) == "REF_RP=.;ALT_RP=.;REF_END=.;ALT_END=.;RPB=.;RPZ=."


@pytest.mark.parametrize("end", [2, 4, 8, 16, 32, 64])
def test_ref_end_and_alt_end_for_every_legal_end(end):
    t = hand_made(end)
    k = RP.EDGES.index(end)
    info = dict(kv.split("=") for kv in t.info(1, "C", ["T"]).split(";"))
    ref, alt = [3, 3, 6, 12, 24, 30, 5], [14, 5, 1, 0, 0, 0, 0]
    assert info["REF_END"] == str(sum(ref[:k])) and info["ALT_END"] == str(sum(alt[:k]))
    assert info["RPB"] == "%.4g" % fisher_two_sided(sum(ref[:k]), sum(ref[k:]), sum(alt[:k]), sum(alt[k:]))
    assert info["REF_RP"] == "|".join(map(str, ref))          # the bins do not depend on the end


@pytest.mark.parametrize("end", [0, 1, 3, 7, 9, 63, 65, 128, -8, 8.0, "8", None, True])
def test_any_other_end_is_an_error_that_names_the_bin_edges(end):
    with pytest.raises(ValueError) as e:
        readpos.end_bins(end)
    assert "2, 4, 8, 16, 32, 64" in str(e.value)


class Stub:
    def __init__(self, text):
        self.text = text

    def info(self, *args):          # (the hooks' info methods take different arguments)
        return self.text


def test_the_keys_go_behind_all_others_on_a_vcf_line():
    t = hand_made()
    r = calling.VariantRecord(0, "A", ["G"], 78, 52, [26], 52 / 78, [26 / 78], (0, 1))
    plain = calling.vcf_line("chr", r)
    line = calling.vcf_line("chr", r, readpos=t)
    assert line == calling.vcf_line("chr", r, None, None, None, None, None, None, None, t)
    f, g = plain.split("\t"), line.split("\t")
    assert g[7] == f[7] + ";" + t.info(0, "A", ["G"]) and f[:7] + f[8:] == g[:7] + g[8:]
    others = [Stub(k + "=1") for k in ("SB", "PRIMER", "ALT_CODON_DP", "DEL", "COOC", "ERR_P", "HAP")]
    full = calling.vcf_line("chr", r, *others, t).split("\t")[7].split(";")
    assert [kv.split("=")[0] for kv in full[5:]] == ["SB", "PRIMER", "ALT_CODON_DP", "DEL", "COOC", "ERR_P", "HAP"] + list(readpos.KEYS)
    assert readpos.HEADER_LINES.count("##INFO=<ID=") == 6 and all("ID=%s," % k in readpos.HEADER_LINES for k in readpos.KEYS)
    res_text = calling.vcf_line("chr", r, hap=others[-1], readpos=t)
    assert res_text.split("\t")[7].endswith(";HAP=1;" + t.info(0, "A", ["G"]))


def test_the_header_declares_the_keys_last(tmp_path):
    fn = str(tmp_path / "h.vcf")
    w = amplipy.VcfWriter(fn, "chr", strand=True, hap=True, readpos=True)
    w.close()
    text = open(fn).read()
    assert text.index("ID=SB,") < text.index("ID=HAP,") < text.index("ID=REF_RP,") < text.index("ID=RPZ,") < text.index("#CHROM")
    fn = str(tmp_path / "p.vcf")
    amplipy.VcfWriter(fn, "chr").close()
    assert "REF_RP" not in open(fn).read()


# ---- the TSV and the wire ---------------------------------------------------------------------------------------------------------
def test_the_tsv_and_its_gz_form(tmp_path):
    t = hand_made()
    f = io.StringIO()
    readpos.write_tsv(f, "chr%1", t)
    lines = f.getvalue().splitlines()
    head = lines[0].split("\t")
    assert head[:2] == ["#ref", "pos"] and head[2] == "A_0-1" and head[8] == "A_64+" and head[9] == "C_0-1" and head[-7:] == ["del_" + b for b in readpos.BIN_NAMES]
    assert len(lines) == 5 and all(len(l.split("\t")) == 44 for l in lines)
    row = lines[3].split("\t")
    assert row[:2] == ["chr%1", "3"] and row[2:9] == ["0", "0", "0", "0", "7", "0", "0"] and row[-7:] == ["0", "1", "2", "3", "4", "0", "0"]
    from amplipy_amd import qc
    fn = str(tmp_path / "t.tsv.gz")
    g = qc.open_new(fn)
    readpos.write_tsv(g, "chr%1", t)
    g.close()
    assert gzip.open(fn, "rt").read() == f.getvalue()


def test_the_wire_format_goes_there_and_back_and_adds_up():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 2 ** 32, size=(9, 6, 7), dtype=np.uint64).astype(np.uint32)
    wire = readpos.to_wire(a)
    assert wire.dtype == np.int64 and wire.shape == (9 * 42,) and np.array_equal(readpos.from_wire(wire), a)
    b = rng.integers(0, 1000, size=(9, 6, 7)).astype(np.uint32)
    small = (a >> 1).astype(np.uint32)
    assert np.array_equal(readpos.from_wire(readpos.to_wire(small) + readpos.to_wire(b)), small + b)
    assert wire[42 + 7 * 2 + 3] == a[1, 2, 3]            # position-major, then column, then bin


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_parse_args_on_every_command():
    for cmd in (["variants", "-r", "r.fas"], ["consensus", "-r", "r.fas"], ["aio", "-p", "p.bed", "-r", "r.fas", "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas"],
                ["trim", "-p", "p.bed", "-r", "r.fas"]):
        a = amplipy.parse_args(cmd)
        assert (a.readpos, a.readpos_end, a.readpos_out) == (False, None, None)
        a = amplipy.parse_args(cmd + ["--readpos", "--readpos_end", "16", "--readpos_out", "r.tsv.gz"])
        assert (a.readpos, a.readpos_end, a.readpos_out) == (True, 16, "r.tsv.gz")


@pytest.mark.parametrize("kwargs, word", [
    (dict(run_trim=True, readpos=True), "A run that only trims has no count table: no read-position tallies (--readpos, --readpos_out)"),
    (dict(run_trim=True, readpos_fn="r.tsv"), "A run that only trims has no count table: no read-position tallies (--readpos, --readpos_out)"),
    (dict(run_consensus=True, readpos=True), "The read-position INFO keys need a VCF (--readpos on variants or aio)"),
    (dict(run_variants=True, readpos_end=8), "(--readpos_end) needs --readpos"),
    (dict(run_variants=True, readpos_fn="r.tsv", readpos_end=8), "(--readpos_end) needs --readpos"),
    (dict(run_variants=True, readpos=True, readpos_end=10), "--readpos_end must be one of the bin edges 2, 4, 8, 16, 32, 64: 10"),
    (dict(run_variants=True, readpos=True, readpos_end=0), "--readpos_end must be one of the bin edges 2, 4, 8, 16, 32, 64: 0"),
    (dict(run_variants=True, run_consensus=True, run_trim=True, readpos=True, readpos_end=128), "--readpos_end must be one of the bin edges")])
def test_run_amplipy_refuses_before_anything_is_opened(kwargs, word, capfd):
    with pytest.raises(SystemExit):
        amplipy.run_amplipy(**kwargs)
    assert word in capfd.readouterr().err
