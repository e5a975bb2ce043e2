"""The host side of the read haplotypes (amplipy_amd/haplotype.py) on hand-made tables: the region
loader's errors, the entries decoded to text and back through cooc.parse_mutation, the order and the thresholds of --hap_out,
HAP_N and HAP of a VCF record, merge_entries, check_lost, the invariant Tables asserts, parse_args and the refusals of
run_amplipy.  No GPU needed."""
import gzip
import io

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, cooc, haplotype
from tests import hap_util as U

REF = "ACGTACGTACGTACGTACGTnnACGTacgtACGTACGTACGT"       # 42 letters
G = len(REF)


def regions(text=None):
    text = text or "chr\t10\t20\tsecond\nchr\t2\t12\tfirst\nchr\t10\t11\tone\n"
    return haplotype.parse_regions(text, "chr", G)


def entries(table):
    """{(device region, ((offset, kind, length), ..)): [count, rev]} -> abi.HAP_ENTRY_DTYPE"""
    return U.as_array(table)


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def test_regions_keep_the_file_s_order_and_are_sorted_for_the_device():
    r = regions()
    assert [n for _, _, n in r.rows] == ["second", "first", "one"]
    assert r.starts.tolist() == [2, 10, 10] and r.ends.tolist() == [12, 20, 11] and r.order == [1, 0, 2] and r.row == {1: 0, 0: 1, 2: 2}
    assert r.holding(10) == [0, 1, 2] and r.holding(11) == [0, 1] and r.holding(19) == [0] and r.holding(20) == []
    r = haplotype.parse_regions("# a comment\ntrack name=x\nchr\t0\t%d\n\nchr\t5\t6\t\n" % G, "chr", G)
    assert [n for _, _, n in r.rows] == ["region1", "region2"] and r.rows[0][:2] == (0, G)


@pytest.mark.parametrize("text, word", [
    ("chr\t5\n", "not 'ref"), ("chr\tx\t9\n", "not 'ref"), ("other\t1\t5\n", "the reference is chr"), ("chr\t5\t5\n", "empty"), ("chr\t9\t5\n", "empty"),
    ("chr\t-1\t5\n", "outside"), ("chr\t40\t43\n", "outside"), ("chr\t1\t5\ta b\n", "region name"), ("chr\t1\t5\ta:b\n", "region name"),
    ("chr\t1\t5\ta,b\n", "region name"), ("chr\t1\t5\tn\nchr\t2\t6\tn\n", "used twice"), ("# nothing\n", "No region")])
def test_the_loader_s_errors(text, word, capfd):
    with pytest.raises(SystemExit):
        haplotype.parse_regions(text, "chr", G)
    assert word in capfd.readouterr().err


def test_a_region_longer_than_4096_and_more_than_65536_regions_are_errors(capfd):
    with pytest.raises(SystemExit):
        haplotype.parse_regions("chr\t0\t4097\n", "chr", 5000)
    assert "at most 4096" in capfd.readouterr().err
    haplotype.parse_regions("chr\t0\t4096\n", "chr", 5000)
    with pytest.raises(SystemExit):
        haplotype.parse_regions("".join("chr\t%d\t%d\n" % (k, k + 1) for k in range(abi.HAP_MAX_REGIONS + 1)), "chr", 70000)
    assert "at most 65536" in capfd.readouterr().err


def test_load_regions_reads_gz_and_misses_files(tmp_path, capfd):
    fn = tmp_path / "r.bed.gz"
    with gzip.open(str(fn), "wt") as f:
        f.write("chr\t2\t12\tfirst\n")
    assert haplotype.load_regions(str(fn), "chr", G).rows == [(2, 12, "first")]
    with pytest.raises(SystemExit):
        haplotype.load_regions(str(tmp_path / "none.bed"), "chr", G)
    assert "File not found" in capfd.readouterr().err


# ---- decoding ---------------------------------------------------------------------------------------------------------------------
def test_entries_decode_to_the_grammar_of_the_mutation_sets_and_back():
    r = regions("chr\t2\t32\tw\n")
    diffs = ((0, 0, 0), (3, 3, 0), (5, U.KIND_DEL, 1), (8, U.KIND_DEL, 4), (24, 2, 0), (29, U.KIND_N, 0))
    # offsets from 2: G3A (ref[2] = G), C6T? ref[5] = C; del8; del11-14; a lower-case reference letter at 26; N at 31
    e = entries({(0, diffs): [7, 3]})[0]
    assert haplotype.decode(e) == (0, list(diffs), 7, 3)
    texts = [haplotype.mutation_text(2, d, REF) for d in diffs]
    assert texts == ["G3A", "C6T", "del8", "del11-14", "G27G".replace("G27G", "%s27G" % REF[26].upper()), "%s32N" % REF[31].upper()]
    for d, text in zip(diffs, texts):
        if d[1] == U.KIND_N:
            continue
        if REF[2 + d[0]].upper() == "ACGT"[d[1]] if d[1] < 4 else False:
            continue                                    # (a substitution to the reference letter cannot come from the device)
        t, pos, ln, sym = cooc.parse_mutation(text, REF, "here")
        assert (pos, ln) == (2 + d[0], d[2] if d[1] == U.KIND_DEL else 0) and (ln > 0 or sym == d[1])


def test_every_mutation_of_a_seeded_table_goes_back_through_parse_mutation():
    rng = np.random.default_rng(4)
    ref = U.reference(3000)
    n = 0
    for _ in range(300):
        start = int(rng.integers(0, 2900))
        off = int(rng.integers(0, 90))
        p = start + off
        if ref[p].upper() not in "ACGT":
            continue
        kind = int(rng.integers(0, 6))
        if kind < 4 and "ACGT"[kind] == ref[p].upper() or kind == U.KIND_N:
            continue
        ln = int(rng.integers(1, 9)) if kind == U.KIND_DEL else 0
        text = haplotype.mutation_text(start, (off, kind, ln), ref)
        t, pos, l2, sym = cooc.parse_mutation(text, ref, "here")
        assert (pos, l2) == (p, ln) and (ln > 0 or sym == kind)
        n += 1
    assert n > 100


# ---- the tables -------------------------------------------------------------------------------------------------------------------
def hand_made(min_reads=2, min_freq=0.0, vcf_min_freq=0.0, lost=0):
    """Three regions (file order: second [10, 20), first [2, 12), one [10, 11)); device order: first, second, one."""
    r = regions()
    table = {(0, ((8, 0, 0),)): [30, 10],                       # first: G11A  (ref[10] = G)
             (0, ((8, 0, 0), (9, U.KIND_DEL, 1))): [5, 5],      # first: G11A,del12
             (0, ((1, 1, 0),)): [1, 0],                         # first: T4C, one read
             (1, ((0, 0, 0),)): [40, 20],                       # second: G11A
             (1, ((0, 3, 0), (4, U.KIND_DEL, 3))): [40, 1],     # second: G11T,del15-17
             (2, ((0, 0, 0),)): [9, 0]}                         # one: G11A
    tally = np.array([[100, 60, 30, 2, 1, 1], [100, 15, 5, 3, 0, 2], [20, 10, 0, 0, 0, 1]], np.uint64)
    tally[0, U.COVER] += lost                                   # (the lost reads are in COVER and nowhere else)
    return haplotype.Tables(r, REF, entries(table), tally, [150, 7], lost, min_reads, min_freq, vcf_min_freq)


def tsv(tables):
    f = io.StringIO()
    haplotype.write_tsv(f, "chr", tables)
    return [l.split("\t") for l in f.getvalue().splitlines()]


def test_the_tsv_s_columns_order_and_thresholds():
    rows = tsv(hand_made())
    assert rows[0] == ["#ref", "region", "start", "end", "haplotype", "reads", "reverse", "usable", "frequency", "cover", "lowq", "overflow", "edge"]
    body = rows[1:]
    assert [(r[1], r[4], r[5], r[6]) for r in body] == [
        ("second", "G11A", "40", "20"), ("second", "G11T,del15-17", "40", "1"), ("second", "ref", "15", "5"),      # by reads, then by text
        ("first", "ref", "60", "30"), ("first", "G11A", "30", "10"), ("first", "G11A,del12", "5", "5"),             # T4C has one read
        ("one", "ref", "10", "0"), ("one", "G11A", "9", "0")]
    assert body[0][2:4] == ["10", "20"] and body[0][7:] == ["95", "%.6g" % (40 / 95), "100", "3", "0", "2"]
    assert body[3][7:] == ["96", "0.625", "100", "2", "1", "1"]
    # the thresholds: min_reads 1 lists the single read; min_freq drops what is rarer; the ref row is always written
    assert ("first", "T4C") in [(r[1], r[4]) for r in tsv(hand_made(min_reads=1))[1:]]
    few = [(r[1], r[4]) for r in tsv(hand_made(min_freq=0.4))[1:]]
    assert few == [("second", "G11A"), ("second", "G11T,del15-17"), ("second", "ref"), ("first", "ref"), ("one", "ref"), ("one", "G11A")]
    high = [(r[1], r[4]) for r in tsv(hand_made(min_reads=1000))[1:]]
    assert high == [("second", "ref"), ("first", "ref"), ("one", "ref")]
    # no usable read: the frequency is '.'
    r = regions("chr\t2\t12\tempty\n")
    t = haplotype.Tables(r, REF, entries({}), [[4, 0, 0, 3, 0, 1]], [4, 0])
    assert tsv(t)[1][4:9] == ["ref", "0", "0", "0", "."]


def test_hap_n_and_hap_of_a_record():
    t = hand_made()
    # position 10 (POS 11), ALT A: G11A of all three regions and G11A,del12 of first; the commonest is second's (40 reads; file order breaks no tie here)
    assert t.info(10, "G", ["A"]) == "HAP_N=4;HAP=second:G11A:40:95"
    assert t.info(10, "G", ["T"]) == "HAP_N=1;HAP=second:G11T+del15-17:40:95"
    assert t.info(10, "G", ["A", "T"]).startswith("HAP_N=5;HAP=second:G11A:40:95")
    assert t.info(10, "G", ["C"]) == "HAP_N=0;HAP=."
    # a deletion counts where '-' is an alternate and the position lies under it
    assert t.info(11, "T", ["-"]) == "HAP_N=1;HAP=first:G11A+del12:5:96"
    assert t.info(15, "T", ["-"]) == "HAP_N=1;HAP=second:G11T+del15-17:40:95" and t.info(17, "C", ["A"]) == "HAP_N=0;HAP=."
    assert t.info(16, "A", ["-", "AGG"]).startswith("HAP_N=1;") and t.info(13, "C", ["-"]) == "HAP_N=0;HAP=."
    # below hap_min_reads: T4C's single read does not count; with min_reads 1 it does
    assert t.info(3, "T", ["C"]) == "HAP_N=0;HAP=." and hand_made(min_reads=1).info(3, "T", ["C"]) == "HAP_N=1;HAP=first:T4C:1:96"
    # the variant frequency threshold: 5 / 96 is below 0.1
    assert hand_made(vcf_min_freq=0.1).info(11, "T", ["-"]) == "HAP_N=0;HAP=." and hand_made(vcf_min_freq=0.1).info(10, "G", ["A"]).startswith("HAP_N=3;")
    # outside every region
    assert t.info(30, "A", ["C"]) == "HAP_N=0;HAP=."


def test_the_keys_go_behind_all_others_on_a_vcf_line():
    t = hand_made()
    r = calling.VariantRecord(10, "G", ["A"], 100, 40, [60], 0.4, [0.6], (0, 1))
    plain = calling.vcf_line("chr", r)
    line = calling.vcf_line("chr", r, hap=t)
    assert line == calling.vcf_line("chr", r, None, None, None, None, None, None, t)
    f, g = plain.split("\t"), line.split("\t")
    assert g[7] == f[7] + ";HAP_N=4;HAP=second:G11A:40:95" and f[:7] + f[8:] == g[:7] + g[8:]
    assert haplotype.HEADER_LINES.count("##INFO=<ID=") == 2 and all("ID=%s," % k in haplotype.HEADER_LINES for k in haplotype.KEYS)


def test_the_invariant_is_asserted_where_a_table_is_read():
    hand_made()
    hand_made(lost=1)
    r = regions()
    with pytest.raises(ValueError):             # a read that is nowhere
        haplotype.Tables(r, REF, entries({}), [[5, 1, 0, 1, 1, 1], [0] * 6, [0] * 6], [5, 0])
    with pytest.raises(ValueError):             # more entries than COVER
        haplotype.Tables(r, REF, entries({(0, ((1, 0, 0),)): [9, 0]}), [[5, 1, 0, 1, 1, 1], [0] * 6, [0] * 6], [5, 0])
    with pytest.raises(ValueError):             # lost reads that nobody reported
        haplotype.Tables(r, REF, entries({}), [[5, 1, 0, 1, 1, 1], [0] * 6, [0] * 6], [5, 0], lost=0)
    with pytest.raises(ValueError):             # more reverse reference reads than reference reads
        haplotype.Tables(r, REF, entries({}), [[5, 2, 3, 1, 1, 1], [0] * 6, [0] * 6], [5, 0])
    with pytest.raises(ValueError):             # an entry of a region that is not there
        haplotype.Tables(r, REF, entries({(3, ((1, 0, 0),)): [1, 0]}), [[0] * 6] * 3, [0, 0])


def test_merge_entries_sums_per_key_in_key_order():
    a = {(0, ((8, 0, 0),)): [30, 10], (1, ((0, 0, 0),)): [4, 2]}
    b = {(0, ((8, 0, 0),)): [1, 1], (0, ((8, 0, 0), (9, U.KIND_DEL, 1))): [5, 5]}
    m = haplotype.merge_entries([entries(a), entries(b), entries({})])
    assert m.tobytes() == entries(U.add_tables(a, b)).tobytes() and U.as_dict(m)[(0, ((8, 0, 0),))] == [31, 11]
    assert haplotype.merge_entries([]).size == 0


def test_check_lost_names_the_flag():
    haplotype.check_lost(0)
    with pytest.raises(RuntimeError) as e:
        haplotype.check_lost(3)
    assert "--hap_capacity" in str(e.value) and "3 reads" in str(e.value)


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_parse_args_on_every_command():
    for cmd in (["variants", "-r", "r.fas"], ["consensus", "-r", "r.fas"], ["aio", "-p", "p.bed", "-r", "r.fas", "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas"],
                ["trim", "-p", "p.bed", "-r", "r.fas"]):
        a = amplipy.parse_args(cmd)
        assert (a.haplotypes, a.hap_out, a.hap_min_reads, a.hap_min_freq, a.hap_capacity) == (None, None, 2, 0.0, None)
        a = amplipy.parse_args(cmd + ["--haplotypes", "r.bed", "--hap_out", "h.tsv.gz", "--hap_min_reads", "5", "--hap_min_freq", "0.01", "--hap_capacity", "12"])
        assert (a.haplotypes, a.hap_out, a.hap_min_reads, a.hap_min_freq, a.hap_capacity) == ("r.bed", "h.tsv.gz", 5, 0.01, 12)


@pytest.mark.parametrize("kwargs, word", [
    (dict(run_trim=True, haplotypes_fn="r.bed"), "A run that only trims has no count table: no read haplotypes (--haplotypes, --hap_out)"),
    (dict(run_variants=True, hap_out_fn="h.tsv"), "need the region file (--haplotypes)"),
    (dict(run_variants=True, hap_capacity=12), "need the region file (--haplotypes)"),
    (dict(run_variants=True, haplotypes_fn="r.bed", hap_capacity=3), "--hap_capacity is the log2"),
    (dict(run_variants=True, haplotypes_fn="r.bed", hap_capacity=29), "--hap_capacity is the log2"),
    (dict(run_variants=True, haplotypes_fn="r.bed", hap_min_reads=-1), "--hap_min_reads"),
    (dict(run_consensus=True, haplotypes_fn="r.bed", hap_min_freq=1.5), "--hap_min_freq")])
def test_run_amplipy_refuses_before_anything_is_opened(kwargs, word, capfd):
    with pytest.raises(SystemExit):
        amplipy.run_amplipy(**kwargs)
    assert word in capfd.readouterr().err
