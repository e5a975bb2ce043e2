"""The host side of the deletion events (amplipy_amd/deletion.py) on hand-made tables: the two INFO keys,
the TSV rows, the indel VCF -- its anchors (start == 0 included), thresholds, ordering, header and .gz output, every record's
REF held to the reference at its POS -- the merge of the ranks' tables, the error for lost reads, and the refusals of the
command line.  No GPU needed."""
import gzip
import io
import re

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, deletion, qc

REF = "ACGTTGCAAGGCTTACGATCGGATCCTAGA"      # 30 bases


def events(rows):
    ev = np.zeros(len(rows), abi.DEL_EVENT_DTYPE)
    for k, r in enumerate(rows):
        ev[k] = r
    return ev


def small_tables(min_depth=10, min_freq=0.03):
    counts = np.zeros((len(REF), 6), np.uint32)
    counts[:, 0] = 100                                          # depth 100 everywhere ...
    counts[20] = (1, 1, 1, 1, 0, 1)                             # ... but 5 at position 20
    counts[4:13, 5] = 40; counts[4:13, 0] = 60                  # the 9-base deletion's '-' column
    rows = [(4, 9, 40, 15), (0, 2, 5, 0), (6, 1, 2, 2), (6, 3, 2, 0), (5, 4, 50, 1), (20, 2, 1, 1), (27, 3, 100, 50)]
    return deletion.Tables(events(rows), counts, REF, min_depth, min_freq)


def test_tables_are_ordered_and_checked():
    t = small_tables()
    assert [tuple(e) for e in t.events.tolist()] == sorted(tuple(e) for e in t.events.tolist())
    assert t.covering(6) == [(4, 9, 40, 15), (5, 4, 50, 1), (6, 1, 2, 2), (6, 3, 2, 0)] and t.covering(13) == [] and t.covering(29) == [(27, 3, 100, 50)]
    assert t.covering(0) == [(0, 2, 5, 0)] and t.covering(2) == []
    for bad in ((28, 3, 1, 0), (-1, 2, 1, 0), (3, 0, 1, 0), (3, 1, 1, 2)):
        with pytest.raises(ValueError):
            deletion.Tables(events([bad]), np.zeros((len(REF), 6), np.uint32), REF)


def test_info_keys():
    t = small_tables()
    assert t.info(6, 100) == "DEL_N=4;DEL=6-9:50:1,5-13:40:15"             # 2 / 100 is below min_freq; descending count
    assert t.info(6, 50) == "DEL_N=4;DEL=6-9:50:1,5-13:40:15,7-7:2:2,7-9:2:0"       # equal counts: by start, then by length
    assert t.info(13, 100) == "DEL_N=0;DEL=." and t.info(0, 1000) == "DEL_N=1;DEL=." and t.info(1, 100) == "DEL_N=1;DEL=1-2:5:0"
    assert t.info(6, 0) == "DEL_N=4;DEL=."
    assert deletion.KEYS == ("DEL_N", "DEL")
    for k in deletion.KEYS:
        assert re.search(r"^##INFO=<ID=%s,Number=[1.],Type=(Integer|String),Description=\"[^\"]+\">$" % k, deletion.HEADER_LINES, re.M)
    assert deletion.HEADER_LINES.count("\n") == 2


def test_vcf_line_and_vcf_text_carry_the_keys_last():
    t = small_tables()
    rec = calling.VariantRecord(6, "C", ["-"], 100, 58, [42], 0.58, [0.42], (0, 1))
    plain, with_keys = calling.vcf_line("ref", rec), calling.vcf_line("ref", rec, None, None, None, t)
    f_plain, f_keys = plain.split("\t"), with_keys.split("\t")
    assert f_keys[:7] == f_plain[:7] and f_keys[8:] == f_plain[8:]
    assert f_keys[7] == f_plain[7] + ";" + t.info(6, 100)
    assert calling.vcf_line("ref", rec, None, None, None, None) == plain


def test_vcf_writer_header(tmp_path, monkeypatch):
    import sys
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    texts = {}
    for on in (False, True):
        fn = str(tmp_path / ("h%d.vcf" % on))
        w = amplipy.VcfWriter(fn, "ref", deletion=True) if on else amplipy.VcfWriter(fn, "ref")
        w.close()
        texts[on] = open(fn).read()
    assert texts[True].replace(deletion.HEADER_LINES, "") == texts[False] and deletion.HEADER_LINES in texts[True]
    assert texts[True].index(deletion.HEADER_LINES) + len(deletion.HEADER_LINES) == texts[True].index("#CHROM")


@pytest.mark.parametrize("name", ["d.tsv", "d.tsv.gz"])
def test_tsv_writer(tmp_path, name):
    t = small_tables()
    f = qc.open_new(str(tmp_path / name))
    deletion.write_tsv(f, "re%f", t)
    f.close()
    lines = (gzip.open(str(tmp_path / name), "rt") if name.endswith(".gz") else open(str(tmp_path / name))).read().splitlines()
    assert lines[0] == "#ref\tstart\tlength\tcount\trev\tdepth\tfreq\tdeleted"
    assert lines[1] == "re%f\t1\t2\t5\t0\t100\t0.05\tAC" and lines[2] == "re%f\t5\t9\t40\t15\t100\t0.4\t" + REF[4:13]
    assert lines[6] == "re%f\t21\t2\t1\t1\t5\t0.2\t" + REF[20:22] and len(lines) == 8
    with pytest.raises(SystemExit):
        qc.open_new(str(tmp_path / name))


def indel_text(t, insertions=()):
    f = io.StringIO()
    deletion.write_indel_vcf(f, "ref", t, insertions, "cmd line")
    return f.getvalue()


def check_indel_vcf(text, ref):
    """The file line by line: the header a VCF 4.2 reader needs, every INFO key declared, every record's REF the reference
    at its POS, REF and ALT sharing the anchor base, positions ascending.  -> the records."""
    lines = text.splitlines()
    assert lines[0] == "##fileformat=VCFv4.2"
    header = [l for l in lines if l.startswith("##")]
    assert all(re.match(r"^##[A-Za-z]+=.+$", l) for l in header)
    declared = set(re.findall(r"^##INFO=<ID=([A-Z]+),Number=(?:1|\.),Type=(?:Integer|Float|String),Description=\"[^\"]+\">$", text, re.M))
    assert declared == {"DP", "AD", "RV", "AF"}
    assert any(l.startswith("##contig=<ID=ref,length=%d>" % len(ref)) for l in header) and any("no left-alignment" in l for l in header)
    k = len(header)
    assert lines[k] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    recs = []
    for l in lines[k + 1:]:
        f = l.split("\t")
        assert len(f) == 8 and f[0] == "ref" and f[2] == "." and f[5] == "." and f[6] == "PASS"
        pos, r, a = int(f[1]), f[3], f[4]
        assert pos >= 1 and ref[pos - 1:pos - 1 + len(r)] == r                   # REF is the reference at POS
        assert re.fullmatch("[ACGTN]+", r) and re.fullmatch("[ACGTN]+", a) and len(r) != len(a)
        info = dict(kv.split("=") for kv in f[7].split(";"))
        assert list(info) == ["DP", "AD", "RV", "AF"] and set(info) <= declared
        assert float(info["AF"]) == pytest.approx(int(info["AD"]) / int(info["DP"]), rel=1e-5)
        if len(r) > len(a):                                                       # a deletion: one base is left, at either end
            assert len(a) == 1 and (r[0] == a or (pos == 1 and r[-1] == a)) and int(info["RV"]) <= int(info["AD"])
        else:
            assert len(r) == 1 and info["RV"] == "."
        recs.append((pos, r, a, info))
    assert [x[0] for x in recs] == sorted(x[0] for x in recs)
    return recs


def test_indel_vcf_anchors_thresholds_and_order():
    t = small_tables()
    ins = [(6, "CTT", 30, 130), (6, "CA", 3, 130), (2, "GAA", 9, 109), (20, "TG", 4, 9)]
    recs = check_indel_vcf(indel_text(t, ins), REF)
    got = [(p, r, a, i["AD"], i["RV"]) for p, r, a, i in recs]
    assert got == [
        (1, "ACG", "G", "5", "0"),                       # start == 0: anchored at the base behind the deletion
        (3, "G", "GAA", "9", "."),
        (4, "TTGCAAGGCT", "T", "40", "15"),              # the 9-base deletion once: POS = start, REF = anchor + deleted text
        (5, "TGCAA", "T", "50", "1"),
        (7, "C", "CTT", "30", "."),                      # behind the deletions of its position; CA (3 / 130) is below min_freq
        (27, "TAGA", "T", "100", "50"),                  # up to the last base of the reference
    ]                                                    # (6, 1) and (6, 3): 2 / 100 below min_freq; (20, 2) and TG: depth below min_depth
    assert recs[2][3]["DP"] == "100" and recs[4][3]["DP"] == "130"
    # thresholds of zero: everything
    t0 = small_tables(0, 0.0)
    assert len(check_indel_vcf(indel_text(t0, ins), REF)) == 7 + 4
    # same position: deletions first, shorter first, then insertions by allele
    same = [x for x in check_indel_vcf(indel_text(t0, ins), REF) if x[0] in (6, 7)]
    assert [(x[0], x[1], x[2]) for x in same] == [(6, "GC", "G"), (6, "GCAA", "G"), (7, "C", "CA"), (7, "C", "CTT")]
    # an empty table is a valid file
    empty = deletion.Tables(events([]), np.zeros((len(REF), 6), np.uint32), REF)
    assert check_indel_vcf(indel_text(empty), REF) == [] and empty.info(3, 10) == "DEL_N=0;DEL=."


def test_indel_vcf_gz_and_existing_file(tmp_path):
    t = small_tables()
    fn = str(tmp_path / "i.vcf.gz")
    f = qc.open_new(fn)
    deletion.write_indel_vcf(f, "ref", t, [(2, "GAA", 9, 109)], "cmd line")
    f.close()
    assert gzip.open(fn, "rt").read() == indel_text(t, [(2, "GAA", 9, 109)])
    with pytest.raises(SystemExit):
        qc.open_new(fn)


def test_insertion_rows_come_from_the_call_s_records():
    recs = [calling.VariantRecord(6, "C", ["CTT", "-", "CA"], 130, 50, [30, 47, 3], 50 / 130, [30 / 130, 47 / 130, 3 / 130], (0, 1, 2, 3)),
            calling.VariantRecord(9, "G", ["T"], 100, 90, [10], 0.9, [0.1], (0, 1))]
    assert deletion.insertion_rows(recs) == [(6, "CTT", 30, 130), (6, "CA", 3, 130)]


def test_merge_of_the_ranks_tables_and_the_lost_error():
    a = events([(4, 9, 40, 15), (0, 2, 5, 0)])
    b = events([(0, 2, 1, 1), (7, 1, 3, 0), (4, 9, 2 ** 31, 5)])
    m = deletion.merge_events([a, b, events([])])
    assert m.dtype == abi.DEL_EVENT_DTYPE and [tuple(e) for e in m.tolist()] == [(0, 2, 6, 1), (4, 9, 40 + 2 ** 31, 20), (7, 1, 3, 0)]
    deletion.check_lost(0)
    with pytest.raises(RuntimeError) as e:
        deletion.check_lost(np.uint64(7))
    assert "--del_capacity" in str(e.value) and "7 reads" in str(e.value)


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, message", [
    (["trim", "-p", "p.bed", "-r", "r.fas", "--deletions"], "no count table"),
    (["trim", "-p", "p.bed", "-r", "r.fas", "--del_out", "d.tsv"], "no count table"),
    (["trim", "-p", "p.bed", "-r", "r.fas", "--indel_vcf", "i.vcf"], "no count table"),
    (["consensus", "-r", "r.fas", "--deletions"], "need a VCF"),
    (["consensus", "-r", "r.fas", "--indel_vcf", "i.vcf"], "variant thresholds"),
    (["variants", "-r", "r.fas", "--del_capacity", "12"], "--del_capacity) needs --deletions, --del_out or --indel_vcf"),
    (["variants", "-r", "r.fas", "--deletions", "--del_capacity", "3"], "4 to 28"),
    (["variants", "-r", "r.fas", "--deletions", "--del_capacity", "29"], "4 to 28"),
    (["variants", "-r", "r.fas", "--indel_vcf", "i.bcf"], "Invalid indel VCF extension"),
])
def test_argument_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        amplipy.main(argv)
    assert e.value.code == 1
    assert message in capsys.readouterr().err


@pytest.mark.parametrize("kw, message", [
    (dict(run_trim=True, deletions=True), "no count table"),
    (dict(run_trim=True, del_out_fn="d.tsv"), "no count table"),
    (dict(run_consensus=True, deletions=True), "need a VCF"),
    (dict(run_consensus=True, indel_vcf_fn="i.vcf"), "variant thresholds"),
])
def test_run_amplipy_argument_errors(kw, message, capsys):
    with pytest.raises(SystemExit):
        amplipy.run_amplipy(**kw)
    assert message in capsys.readouterr().err


def test_flags_are_long_only_and_off_by_default():
    for argv in (["trim", "-p", "p", "-r", "r"], ["variants", "-r", "r"], ["consensus", "-r", "r"],
                 ["aio", "-p", "p", "-r", "r", "-ot", "t", "-ov", "v", "-oc", "c"]):
        a = amplipy.parse_args(argv)
        assert a.deletions is False and a.del_out is None and a.indel_vcf is None and a.del_capacity is None
    a = amplipy.parse_args(["variants", "-r", "r", "--deletions", "--del_out", "d.tsv.gz", "--indel_vcf", "i.vcf", "--del_capacity", "22"])
    assert a.deletions is True and a.del_out == "d.tsv.gz" and a.indel_vcf == "i.vcf" and a.del_capacity == 22
