"""The host side of the co-occurrence tallies (amplipy_amd/cooc.py): the loader of the mutation-set file
and each of its errors once, the 1-based to 0-based conversion and the REF check, the order of the sets for the device and for
the output, the TSV writer and the COOC key on hand-made tables, vcf_line with and without the new argument, and the argument
refusals of run_amplipy, which happen before any engine exists.  No GPU needed."""
import io
import re

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, cooc

#      1-based:  1         11        21        31
REF = "ACGTACGTAC" "GGGTTTCCCA" "AACCGGTTAC" "GTACGTACGT"


def sets_file(tmp_path, text):
    p = tmp_path / "sets.tsv"
    p.write_text(text)
    return str(p)


def test_positions_are_one_based_and_the_ref_letter_is_checked(tmp_path):
    s = cooc.load_sets(sets_file(tmp_path, "# lineage sets\nfirst\tA1C,T40A\n\nsecond\tdel11-13, G3T\t# a comment\r\nthird\tdel20\n"), REF)
    assert [name for name, _ in s.sets] == ["first", "second", "third"]
    assert s.sets[0][1] == [("A1C", 0, 0, 1), ("T40A", 39, 0, 0)]             # 1-based in the file, 0-based here
    assert s.sets[1][1] == [("del11-13", 10, 3, 0), ("G3T", 2, 0, 3)]         # inclusive ends; the file's order is kept
    assert s.sets[2][1] == [("del20", 19, 1, 0)]
    assert REF[0] == "A" and REF[39] == "T" and REF[2] == "G"


def test_sets_are_sorted_for_the_device_and_keep_the_files_order_for_output():
    s = cooc.parse_sets("late\tG35A,A21C\nearly\tdel11-13,G3T\nalso_early\tG3A\n", REF)
    assert s.order == [1, 2, 0]                                 # by first site; equal first sites in file order
    assert s.set_off.tolist() == [0, 2, 3, 5]
    assert s.site_pos.tolist() == [2, 10, 2, 20, 34] and s.site_len.tolist() == [0, 3, 0, 0, 0] and s.site_sym.tolist() == [3, 0, 0, 1, 0]
    assert s.set_off.dtype == np.int32 and s.site_pos.dtype == np.int32 and s.site_len.dtype == np.int32 and s.site_sym.dtype == np.uint8
    assert s.row == {1: 0, 2: 1, 0: 2}
    assert s.bit == [[1, 0], [1, 0], [0]]                       # the device bit of each mutation as the file lists them
    assert s.pattern_text(0, 1) == "01" and s.pattern_text(0, 2) == "10" and s.pattern_text(0, 3) == "11" and s.pattern_text(2, 1) == "1"
    assert s.all_mutated(0) == 3 and s.all_mutated(2) == 1
    assert list(s.substitutions_at(2)) == [(1, 3), (2, 0)] and list(s.substitutions_at(10)) == []


@pytest.mark.parametrize("text, word", [
    ("a\tA1C\na\tG3T\n", "twice"),                              # a duplicate name
    ("a\tA1C,G3T,A5C,G7T,A9C,G11T,T14A\n", "at most 6"),        # more than 6 mutations
    ("a\tdel11-13,G12T\n", "overlap"),                          # overlapping mutations
    ("a\tG3T,G3A\n", "overlap"),
    ("a\tA41C\n", "outside"), ("a\tdel39-41\n", "outside"), ("a\tA0C\n", "outside"),      # outside the reference
    ("a\tC1G\n", "reference has A"),                            # a REF mismatch
    ("a\tA1A\n", "changes nothing"),
    ("a\tdel13-11\n", "in front of"),
    ("a\tins5A\n", "not a mutation"), ("a\tA1\n", "not a mutation"), ("a\t\n", "name <tab> mutations"), ("a\n", "name <tab> mutations"),
    ("a b\tA1C\n", "set name"), ("a|b\tA1C\n", "set name"), ("\tA1C\n", "set name"),
])
def test_loader_errors_go_through_error_with_the_line_number(tmp_path, text, word, capsys):
    with pytest.raises(SystemExit):
        cooc.load_sets(sets_file(tmp_path, "# header\nok\tG3T\n" + text), REF)
    log = capsys.readouterr().err
    assert word in log, log
    assert re.search(r"line %d\b" % (2 + len(text.splitlines())), log), log


def test_an_empty_file_a_missing_file_and_too_wide_a_set(tmp_path):
    for text in ("", "# nothing\n\n"):
        with pytest.raises(SystemExit):
            cooc.load_sets(sets_file(tmp_path, text), REF)
    with pytest.raises(SystemExit):
        cooc.load_sets(str(tmp_path / "nothing.tsv"), REF)
    long_ref = "A" * (abi.COOC_MAX_SPAN + 10)
    cooc.parse_sets("wide\tA1C,A%dC\n" % (abi.COOC_MAX_SPAN + 1), long_ref)
    with pytest.raises(SystemExit):
        cooc.parse_sets("wide\tA1C,A%dC\n" % (abi.COOC_MAX_SPAN + 2), long_ref)


def hand_made():
    s = cooc.parse_sets("late\tG35A,A21C\nearly\tdel11-13,G3T\nquiet\tG3A\n", REF)
    c = np.zeros((3, cooc.CELLS), np.uint32)
    c[0, [0, 1, 3, 64]] = [5, 2, 13, 4]         # device row 0 is 'early': bit 0 G3T, bit 1 del11-13
    c[2, [0, 2, 64]] = [30, 10, 1]              # device row 2 is 'late': bit 0 A21C, bit 1 G35A
    c[1, 64] = 7                                # 'quiet': nothing complete
    return s, cooc.Tables(s, c, [50, 3])


def test_tsv_writer_lists_the_sets_in_file_order_and_patterns_in_the_files_mutation_order():
    s, t = hand_made()
    f = io.StringIO()
    cooc.write_tsv(f, "REF1", t)
    assert f.getvalue().splitlines() == [
        "#ref\tset\tmutations\tpattern\treads\tcomplete\tfrequency\tpartial",
        "REF1\tlate\tG35A,A21C\t00\t30\t40\t0.75\t1",
        "REF1\tlate\tG35A,A21C\t10\t10\t40\t0.25\t1",                       # device cell 2: G35A alone, the file's first mutation
        "REF1\tearly\tdel11-13,G3T\t00\t5\t20\t0.25\t4",
        "REF1\tearly\tdel11-13,G3T\t01\t2\t20\t0.1\t4",                     # device cell 1: G3T alone
        "REF1\tearly\tdel11-13,G3T\t11\t13\t20\t0.65\t4",
        "REF1\tquiet\tG3A\t1\t0\t0\t0\t7"]                                  # nothing complete: the all-mutated pattern, 0 reads
    assert t.summary_line() == "Co-occurrence: 50 reads tallied, 3 irregular reads skipped; 3 mutation sets"


def test_cooc_key():
    s, t = hand_made()
    assert t.info(2, "G", ["T"]) == "COOC=early:13:20"                      # name : reads with all mutations : complete
    assert t.info(2, "G", ["A"]) == "COOC=quiet:0:0"
    assert t.info(2, "G", ["A", "T"]) == "COOC=early:13:20|quiet:0:0"       # the file's order of sets
    assert t.info(2, "G", ["C"]) == "COOC=." and t.info(2, "G", []) == "COOC=."
    assert t.info(34, "G", ["A", "-"]) == "COOC=late:0:40" and t.info(20, "A", ["C"]) == "COOC=late:0:40"
    assert t.info(10, "G", ["-"]) == "COOC=." and t.info(11, "G", ["A"]) == "COOC=."      # a deletion site names no record
    assert cooc.HEADER_LINES.count("\n") == 1 and cooc.HEADER_LINES.startswith("##INFO=<ID=COOC,")


def test_vcf_line_with_and_without_the_new_argument():
    s, t = hand_made()
    r = calling.VariantRecord(2, "G", ["T"], 40, 25, [15], 0.625, [0.375], (0, 1))
    plain = calling.vcf_line("REF1", r)
    assert plain == calling.vcf_line("REF1", r, None, None, None, None) == calling.vcf_line("REF1", r, cooc=None)
    assert plain == "REF1\t3\t.\tG\tT\t.\tPASS\tDP=40;REF_DP=25;ALT_DP=15;REF_FREQ=0.625;ALT_FREQ=0.375\tGT\t0/1\n"
    with_key = calling.vcf_line("REF1", r, cooc=t)
    assert with_key == plain.replace("ALT_FREQ=0.375", "ALT_FREQ=0.375;COOC=early:13:20")

    class Other:                # the keys of the other hooks stand in front
        def info(self, *a):
            return "DEL_N=0;DEL=."
    assert calling.vcf_line("REF1", r, deletion=Other(), cooc=t).split("\t")[7].endswith("ALT_FREQ=0.375;DEL_N=0;DEL=.;COOC=early:13:20")


def test_run_amplipy_refusals():
    with pytest.raises(SystemExit):             # --cooc_out needs --cooc
        amplipy.run_amplipy(trimmed_reads_fn="x.bam", reference_fn="x.fas", variants_fn="x.vcf", run_variants=True, cooc_out_fn="x.tsv")
    with pytest.raises(SystemExit):             # a run that only trims has no count table
        amplipy.run_amplipy(untrimmed_reads_fn="x.bam", primer_fn="x.bed", reference_fn="x.fas", trimmed_reads_fn="y.bam", run_trim=True, cooc_fn="x.tsv")
    a = amplipy.parse_args(["variants", "-r", "x.fas", "--cooc", "s.tsv", "--cooc_out", "o.tsv"])
    assert a.cooc == "s.tsv" and a.cooc_out == "o.tsv"
    assert amplipy.parse_args(["consensus", "-r", "x.fas"]).cooc is None
