"""The host side of the error profile (amplipy_amd/errprof.py): both mask parsers with each error, the
JSON report (key order, cut arrays, the folding into sequencing orientation on a hand-made table, null rates), the binomial tail
behind ERR_P against exact arithmetic, the '.' rules of the two VCF keys, the argument errors per sub-command and the wire format
of the multi-rank merge over gloo.  No GPU needed."""
import gzip
import json
import math
import os
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from amplipy_amd import abi, amplipy, calling, errprof, parallel


# ---- the mask ---------------------------------------------------------------------------------------------------------------
def test_bed_mask(tmp_path):
    fn = tmp_path / "m.bed"
    fn.write_text("anything\t0\t2\nother\t31\t33\tname\n\nx\t99\t100\nx\t5\t5\n")
    m = errprof.load_mask(str(fn), 100)
    assert np.nonzero(m)[0].tolist() == [0, 1, 31, 32, 99]
    gz = tmp_path / "m.bed.gz"
    with gzip.open(gz, "wt") as f:
        f.write("x\t7\t9\n")
    assert np.nonzero(errprof.load_mask(str(gz), 100))[0].tolist() == [7, 8]
    assert not errprof.load_mask(str(tmp_path / "m.bed"), 1000)[100:].any()


def test_vcf_mask(tmp_path):
    body = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\nR\t1\t.\tA\tG\nR\t10\t.\tACG\tA\nR\t100\t.\tT\tC\n"
    fn = tmp_path / "calls.vcf"
    fn.write_text(body)
    assert np.nonzero(errprof.load_mask(str(fn), 100))[0].tolist() == [0, 9, 10, 11, 99]
    gz = tmp_path / "calls.VCF.GZ"
    with gzip.open(gz, "wt") as f:
        f.write(body)
    assert np.nonzero(errprof.load_mask(str(gz), 100))[0].tolist() == [0, 9, 10, 11, 99]


@pytest.mark.parametrize("name,text", [("m.bed", "x\t5\n"), ("m.bed", "x\tfive\t9\n"), ("m.bed", "x\t-1\t4\n"), ("m.bed", "x\t90\t101\n"), ("m.bed", "x\t9\t5\n"),
                                       ("m.vcf", "R\t0\t.\tA\tG\n"), ("m.vcf", "R\t99\t.\tACG\tA\n"), ("m.vcf", "R\t5\t.\n"), ("m.vcf", "R\tx\t.\tA\tG\n"),
                                       ("m.vcf", "R\t5\t.\t\tG\n")])
def test_mask_errors(tmp_path, name, text):
    fn = tmp_path / name
    fn.write_text(text)
    with pytest.raises(SystemExit):
        errprof.load_mask(str(fn), 100)


def test_a_missing_mask_file(tmp_path):
    with pytest.raises(SystemExit):
        errprof.load_mask(str(tmp_path / "nothing.bed"), 100)


# ---- the report -------------------------------------------------------------------------------------------------------------
def hand_made(counts=None):
    cyc = np.zeros(abi.EP_CYC_SHAPE, np.uint64); qualt = np.zeros(abi.EP_QUAL_SHAPE, np.uint64); sub = np.zeros(abi.EP_SUB_SHAPE, np.uint64)
    cyc[0, 0] = [90, 10]; cyc[0, 2] = [50, 0]                   # mate 0: cycles 0 and 2 used, so the arrays are cut behind cycle 2
    qualt[0, 2] = [9, 9]; qualt[0, 37] = [131, 1]
    A, C, G, T = range(4)
    sub[0, 0, 1, C, C] = 60; sub[0, 0, 1, C, T] = 6             # forward reads: C read as T six times ...
    sub[0, 1, 1, G, G] = 40; sub[0, 1, 1, G, A] = 4             # ... reverse reads: G read as A is the same C>T of the instrument
    sub[0, 0, 0, C, T] = 1                                      # below min_quality: in `all`, not in `pass`
    sub[0, 0, 1, A, A] = 39
    return errprof.Tables(cyc, qualt, sub, [7, 2], 20, 3, counts)


def test_report_key_order_cut_arrays_and_null_rates():
    rep = hand_made().report()
    assert list(rep) == ["amplipy_error_profile", "min_quality", "masked_positions", "reads", "total", "read1", "substitutions"]      # no read2: it has no base
    assert rep["min_quality"] == 20 and rep["masked_positions"] == 3 and rep["reads"] == {"profiled": 7, "skipped": 2}
    assert rep["total"] == {"bases": 150, "mismatches": 10, "rate": float("%.6g" % (10 / 150))}
    assert list(rep["read1"]) == ["cycle", "quality"] and list(rep["read1"]["cycle"]) == ["bases", "mismatches", "open_ended"]
    assert rep["read1"]["cycle"] == {"bases": [100, 0, 50], "mismatches": [10, 0, 0], "open_ended": False}
    assert rep["read1"]["quality"] == [{"q": 2, "bases": 18, "mismatches": 9, "empirical": round(-10 * math.log10(10 / 20), 2)},
                                       {"q": 37, "bases": 132, "mismatches": 1, "empirical": round(-10 * math.log10(2 / 134), 2)}]
    s = rep["substitutions"]
    assert list(s) == ["all", "pass", "folded"]
    assert list(s["all"]) == ["A>C", "A>G", "A>T", "C>A", "C>G", "C>T", "G>A", "G>C", "G>T", "T>A", "T>C", "T>G"] == list(s["pass"])
    assert list(s["folded"]) == ["C>A", "C>G", "C>T", "T>A", "T>C", "T>G"]
    assert s["pass"]["C>T"] == {"n": 10, "of": 110, "rate": float("%.6g" % (10 / 110))}          # forward C>T and reverse G>A together
    assert s["all"]["C>T"] == {"n": 11, "of": 111, "rate": float("%.6g" % (11 / 111))}
    assert s["pass"]["G>A"] == {"n": 0, "of": 0, "rate": None} and s["pass"]["T>C"]["rate"] is None
    assert s["pass"]["A>G"] == {"n": 0, "of": 39, "rate": 0.0}
    assert s["folded"]["C>T"] == {"n": 11, "of": 111, "rate": float("%.6g" % (11 / 111))}        # C>T and G>A of the oriented table
    assert s["folded"]["T>C"] == {"n": 0, "of": 39, "rate": 0.0}                                 # T>C and A>G: the A row counts
    json.dumps(rep)
    t = hand_made()
    t.cyc[1, 511] = [4, 1]
    rep = t.report()
    assert list(rep)[5:7] == ["read1", "read2"] and rep["read2"]["cycle"]["open_ended"] is True and len(rep["read2"]["cycle"]["bases"]) == 512
    assert t.summary_line().startswith("Error profile: 7 of 9 reads profiled; 11 mismatches in 155 bases")


# ---- ERR_P ------------------------------------------------------------------------------------------------------------------
def exact_sf(k, n, p):
    """P(K >= k) as a Fraction.  (The rates of the test are dyadic with small numerators: exact as floats, and the integers of
    the sum stay short.)"""
    a, b = Fraction(p).as_integer_ratio()
    return Fraction(sum(math.comb(n, x) * a ** x * (b - a) ** (n - x) for x in range(max(k, 0), n + 1)), b ** n)


def test_binomial_tail_against_exact_arithmetic():
    rng = np.random.default_rng(3)
    cases = [(k, n, p) for n in (1, 2, 17, 400) for k in (0, 1, n // 2, n) for p in (0.0, 1.0, 1 / 8192, 3 / 256, 0.5, 127 / 128)]
    cases += [(int(rng.integers(0, n + 1)), n, float(p)) for n in (50, 333, 1000, 2000) for p in rng.choice([1 / 65536, 1 / 1024, 5 / 256, 5 / 16, 11 / 16], size=6)]
    cases += [(k, 2000, 1 / 1024) for k in (0, 1, 2, 3, 10, 40, 2000)] + [(k, 2000, 0.25) for k in (400, 499, 500, 501, 600, 1500)]
    for k, n, p in cases:
        want, got = exact_sf(k, n, p), errprof.binom_sf(k, n, p)
        if want == 0:
            assert got == 0.0, (k, n, p)
        elif float(want) < 1e-300:              # below what a float holds: the answer is a float that small, or 0
            assert got < 1e-290, (k, n, p)
        else:
            assert abs(Fraction(got) - want) <= Fraction(1, 10 ** 9) * want, (k, n, p, got, float(want))
    assert errprof.binom_sf(0, 10, 0.0) == 1.0 and errprof.binom_sf(3, 10, 0.0) == 0.0 and errprof.binom_sf(10, 10, 1.0) == 1.0 and errprof.binom_sf(0, 0, 0.3) == 1.0


def test_binomial_tail_at_a_million_against_the_plain_sum():
    n = 10 ** 6
    for p, ks in ((1e-3, (0, 900, 1000, 1001, 1100, 1500)), (0.02, (19000, 20000, 20500, 21000)), (2e-6, (1, 2, 10))):
        x = np.arange(0, n + 1, dtype=np.float64)
        lg = np.vectorize(math.lgamma)
        logpmf = math.lgamma(n + 1) - lg(x + 1) - lg(n - x + 1) + x * math.log(p) + (n - x) * math.log1p(-p)
        pmf = np.exp(logpmf)
        for k in ks:
            want = math.fsum(pmf[k:].tolist())
            got = errprof.binom_sf(k, n, p)
            # a term of the plain sum carries lgamma's rounding at 1.3e7, about 2e-9 relative: the two agree to 1e-7
            assert abs(got - want) <= 1e-7 * want, (k, p, got, want)


# ---- the VCF keys -----------------------------------------------------------------------------------------------------------
def test_the_two_keys_and_their_dots():
    counts = np.zeros((50, abi.NSYM), np.uint32)
    counts[4] = [2, 900, 0, 98, 5, 3]           # position 4: C 900, T 98, A 2 (N 5 and '-' 3 are outside the depth over A C G T)
    t = hand_made(counts)
    rate = 6 / 66                               # S[C][T] / sum of S[C]: g == 1 only, mates and strands summed, aligned orientation
    assert t.info(4, "C", ["T"]) == "ERR_RATE=%.4g;ERR_P=%.4g" % (rate, errprof.binom_sf(98, 1000, rate))
    assert t.info(4, "c", ["T", "A"]) == "ERR_RATE=%.4g,0;ERR_P=%.4g,0" % (rate, errprof.binom_sf(98, 1000, rate))       # rate 0, ALT_DP 2: P is 0
    assert t.info(4, "C", ["-", "N", "CAT", "T"]).startswith("ERR_RATE=.,.,.,0.09091;ERR_P=.,.,.,")
    assert t.info(4, "N", ["T"]) == "ERR_RATE=.;ERR_P=." and t.info(4, "-", ["T"]) == "ERR_RATE=.;ERR_P=."
    assert t.info(4, "T", ["C"]) == "ERR_RATE=.;ERR_P=."          # an empty row of S
    assert t.info(9, "G", ["A"]) == "ERR_RATE=%.4g;ERR_P=1" % (4 / 44)          # ALT_DP 0
    assert errprof.HEADER_LINES.count("\n") == 2 and "ID=ERR_RATE," in errprof.HEADER_LINES and "ID=ERR_P," in errprof.HEADER_LINES


def test_vcf_line_with_and_without_the_new_argument():
    counts = np.zeros((50, abi.NSYM), np.uint32)
    counts[2] = [0, 25, 0, 15, 0, 0]
    t = hand_made(counts)
    r = calling.VariantRecord(2, "C", ["T"], 40, 25, [15], 0.625, [0.375], (0, 1))
    plain = calling.vcf_line("REF1", r)
    assert plain == calling.vcf_line("REF1", r, errprof=None)
    assert plain == "REF1\t3\t.\tC\tT\t.\tPASS\tDP=40;REF_DP=25;ALT_DP=15;REF_FREQ=0.625;ALT_FREQ=0.375\tGT\t0/1\n"
    assert calling.vcf_line("REF1", r, errprof=t) == plain.replace("ALT_FREQ=0.375", "ALT_FREQ=0.375;" + t.info(2, "C", ["T"]))

    class Other:                # the keys of the hooks before it stand in front
        def info(self, *a):
            return "COOC=."
    assert calling.vcf_line("REF1", r, cooc=Other(), errprof=t).split("\t")[7].endswith("ALT_FREQ=0.375;COOC=.;" + t.info(2, "C", ["T"]))


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_run_amplipy_refusals_and_arguments():
    with pytest.raises(SystemExit):             # --error_mask needs --error_profile
        amplipy.run_amplipy(trimmed_reads_fn="x.bam", reference_fn="x.fas", variants_fn="x.vcf", run_variants=True, error_mask_fn="m.bed")
    with pytest.raises(SystemExit):             # a run that only trims has no count table
        amplipy.run_amplipy(untrimmed_reads_fn="x.bam", primer_fn="x.bed", reference_fn="x.fas", trimmed_reads_fn="y.bam", run_trim=True, error_profile_fn="e.json")
    for cmd in (["variants", "-r", "x.fas"], ["consensus", "-r", "x.fas"], ["aio", "-r", "x.fas", "-p", "p.bed", "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas"]):
        a = amplipy.parse_args(cmd + ["--error_profile", "e.json", "--error_mask", "first.vcf"])
        assert a.error_profile == "e.json" and a.error_mask == "first.vcf"
        assert amplipy.parse_args(cmd).error_profile is None
    with pytest.raises(SystemExit):             # on trim it is an error
        amplipy.main(["trim", "-r", "x.fas", "-p", "p.bed", "--error_profile", "e.json"])


# ---- the wire format of the multi-rank merge --------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def rank_tables(rank):
    rng = np.random.default_rng(40 + rank)
    tabs = [rng.integers(0, 2 ** 40, size=s, dtype=np.uint64) for s in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE)]
    return tabs + [np.array([2 ** 35 + rank, 7 * rank], np.uint64)]


def _worker(rank, world, port, out_dir):
    import torch
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        wire = torch.from_numpy(errprof.to_wire(*rank_tables(rank)))
        parallel.allreduce_table(dist, wire)
        np.save(os.path.join(out_dir, "wire%d.npy" % rank), wire.numpy())
    finally:
        dist.destroy_process_group()


def test_wire_format_of_the_multi_rank_merge(tmp_path):
    one = rank_tables(0)
    back = errprof.from_wire(errprof.to_wire(*one))
    assert all(np.array_equal(a, b) and a.shape == b.shape and b.dtype == np.uint64 for a, b in zip(one, back))
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = [sum(rank_tables(r)[k] for r in range(world)) for k in range(4)]
    for r in range(world):
        got = errprof.from_wire(np.load(tmp_path / ("wire%d.npy" % r)))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
