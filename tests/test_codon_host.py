"""The host side of the codon tallies (amplipy_amd/codon.py): the CDS loader and its errors, the slots,
translation on both strands, the three writers on hand-made tables, and the argument refusals of run_amplipy, which happen
before any engine exists.  The last test holds the synthetic job of the command-line tests (tests/codon_util.synthetic_job) to
what it claims to carry, on the restatement.  No GPU needed."""
import io

import numpy as np
import pytest

from amplipy_amd import amplipy, codon, synth
from oracle import oracle
from tests import codon_util as U
from tests import strand_util as S


def cds_file(tmp_path, text):
    p = tmp_path / "cds.tsv"
    p.write_text(text)
    return str(p)


def test_load_cds_reads_rows_strands_and_blank_lines(tmp_path):
    cds = codon.load_cds(cds_file(tmp_path, "orf1a\t10\t40\n\norf1b\t36\t60\t+\r\nN\t50\t80\t-\n"), 100)
    assert cds.rows == [("orf1a", 10, 40, "+"), ("orf1b", 36, 60, "+"), ("N", 50, 80, "-")]
    assert cds.starts.dtype == np.int32 and (np.diff(cds.starts) > 0).all()


@pytest.mark.parametrize("text", [
    "", "\n\n",                                         # an empty file
    "orf\t10\n",                                        # fewer than three fields
    "orf\tten\t40\n", "orf\t10\t4e1\n",                 # non-integers
    "orf\t-3\t30\n", "orf\t10\t103\n", "orf\t40\t40\n", "orf\t40\t10\n",      # start < 0, end > G, start >= end
    "orf\t10\t41\n",                                    # no multiple of 3
    "orf\t10\t40\t*\n", "orf\t10\t40\tplus\n",          # a strand other than + or -
    "orf\t10\t40\norf\t50\t80\n",                       # a duplicate name
    "or f\t10\t40\n", "a,b\t10\t40\n", "a;b\t10\t40\n", "a=b\t10\t40\n", "a|b\t10\t40\n", "a:b\t10\t40\n", "\t10\t40\n",
])
def test_load_cds_errors_go_through_error(tmp_path, text, capsys):
    with pytest.raises(SystemExit):
        codon.load_cds(cds_file(tmp_path, text), 100)


def test_missing_file_and_a_reference_too_short_for_a_codon(tmp_path):
    with pytest.raises(SystemExit):
        codon.load_cds(str(tmp_path / "nothing.tsv"), 100)
    with pytest.raises(SystemExit):
        codon.load_cds(cds_file(tmp_path, "orf\t0\t3\n"), 2)
    assert codon.load_cds(cds_file(tmp_path, "orf\t0\t3\n"), 3).starts.tolist() == [0]


def test_slots_of_overlapping_rows_in_three_frames_are_sorted_and_unique():
    cds = codon.CdsSet([("a", 0, 12, "+"), ("b", 4, 13, "+"), ("c", 2, 11, "-"), ("a2", 6, 12, "+")], 20)
    assert cds.starts.tolist() == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10]        # 6 and 9 once, though rows a and a2 both have them
    assert cds.n_slots == 10 and cds.slot_of(7) == 6
    assert [r[0] for r in cds.covering(6)] == ["a", "b", "c", "a2"] and cds.covering(13) == []
    # codon start, offset and codon number: counted from the end on '-' rows
    assert cds.codon_at(("a", 0, 12, "+"), 7) == (6, 1, 3)
    assert cds.codon_at(("c", 2, 11, "-"), 2) == (2, 0, 3) and cds.codon_at(("c", 2, 11, "-"), 10) == (8, 2, 1)


def test_genetic_code_and_reverse_strand():
    assert len(codon.CODE) == 64 and "".join(sorted(set(codon.CODE.values()))) == "*ACDEFGHIKLMNPQRSTVWY"
    assert [codon.translate(t) for t in ("ATG", "TGG", "TAA", "TAG", "TGA", "CGG", "AAG", "AGG", "CAG", "ANG", "atg")] == \
        ["M", "W", "*", "*", "*", "R", "K", "R", "Q", "X", "M"]
    assert sum(v == "L" for v in codon.CODE.values()) == 6 and sum(v == "*" for v in codon.CODE.values()) == 3
    assert codon.revcomp("CAT") == "ATG" and codon.revcomp("AAC") == "GTT"
    assert codon.TRIPLETS[U.cell_of("CGT")] == "CGT" and len(codon.TRIPLETS) == 64


REF = "AACGGTTTCATGG" + "A" * 7                # CGG at 2; CAT at 8 is ATG on the reverse strand
ROWS = [("fwd", 2, 11, "+"), ("rev", 5, 11, "-"), ("late", 14, 20, "+")]


def hand_tables(min_depth=0, min_freq=0.0):
    cds = codon.CdsSet(ROWS, len(REF))
    c = np.zeros((cds.n_slots, 65), np.uint32)
    c[cds.slot_of(2), U.cell_of("CGG")] = 40
    c[cds.slot_of(2), U.cell_of("AAG")] = 60            # R1K
    c[cds.slot_of(2), U.cell_of("AGG")] = 5             # A at offset 0 as well: the smaller count
    c[cds.slot_of(2), 64] = 7
    c[cds.slot_of(5), U.cell_of("TTT")] = 10
    c[cds.slot_of(5), U.cell_of("TTA")] = 10            # a tie with TCA at offset 2
    c[cds.slot_of(5), U.cell_of("TCA")] = 10
    c[cds.slot_of(8), U.cell_of("CAT")] = 90
    c[cds.slot_of(8), U.cell_of("CAC")] = 10            # on the reverse row: GTG, M1V
    return codon.Tables(cds, REF, c, [100, 3], min_depth, min_freq)


def keys(text):
    return dict(kv.split("=", 1) for kv in text.split(";"))


def test_info_keys_on_hand_made_tables():
    t = hand_tables()
    # the largest count with A at offset 0 of the codon at 2 is AAG; the record at offset 1 says the same
    k = keys(t.info(2, "C", ["A"]))
    assert k == {"CDS": "fwd", "CODON_DP": "105", "ALT_AA": "R1K", "ALT_CODON": "CGG>AAG", "ALT_CODON_DP": "60"}
    assert keys(t.info(3, "G", ["A"]))["ALT_AA"] == "R1K"
    assert list(keys(t.info(2, "C", ["A"]))) == list(codon.KEYS)
    # the tie rule: TTA (index 60) and TCA (index 52) both have A at offset 2 and count 10: the smaller index wins
    k = keys(t.info(7, "T", ["A"]))
    assert k == {"CDS": "fwd|rev", "CODON_DP": "30|30", "ALT_AA": "F2S|K2*", "ALT_CODON": "TTT>TCA|AAA>TGA", "ALT_CODON_DP": "10|10"}
    # '.' entries: '-', N, an insertion allele, a base no read shows there; several ALTs are comma-joined
    k = keys(t.info(2, "C", ["A", "-", "N", "CAT", "T"]))
    assert k["ALT_AA"] == "R1K,.,.,.,." and k["ALT_CODON"] == "CGG>AAG,.,.,.,." and k["ALT_CODON_DP"] == "60,.,.,.,."
    # a position covered by two rows: the reverse row writes its codon on its own strand and counts from its end
    k = keys(t.info(10, "T", ["C"]))
    assert k == {"CDS": "fwd|rev", "CODON_DP": "100|100", "ALT_AA": "H3H|M1V", "ALT_CODON": "CAT>CAC|ATG>GTG", "ALT_CODON_DP": "10|10"}
    # a position covered by none
    assert keys(t.info(0, "A", ["C", "G"])) == {"CDS": ".", "CODON_DP": ".", "ALT_AA": ".,.", "ALT_CODON": ".,.", "ALT_CODON_DP": ".,."}
    # covered, nothing tallied
    assert keys(t.info(15, "A", ["C"])) == {"CDS": "late", "CODON_DP": "0", "ALT_AA": ".", "ALT_CODON": ".", "ALT_CODON_DP": "."}
    assert codon.HEADER_LINES.count("##INFO=<ID=") == 5 and codon.HEADER_LINES.count("Number=.,Type=String") == 5


def test_codon_out_on_hand_made_tables():
    f = io.StringIO()
    codon.write_codon_tsv(f, "REF1", hand_tables())
    lines = f.getvalue().splitlines()
    assert lines[0] == "#ref\tcds\tcodon_number\tpos\tref_codon\tref_aa\tcodon\taa\tcount\tdepth\tfreq\tbroken"
    assert lines[1:4] == ["REF1\tfwd\t1\t3\tCGG\tR\tAAG\tK\t60\t105\t0.571429\t7", "REF1\tfwd\t1\t3\tCGG\tR\tAGG\tR\t5\t105\t0.047619\t7",
                          "REF1\tfwd\t1\t3\tCGG\tR\tCGG\tR\t40\t105\t0.380952\t7"]
    # the reverse row: codon 1 is the one at its end, written on its strand
    rev = [l.split("\t") for l in lines if l.split("\t")[1] == "rev"]
    assert [(l[2], l[3], l[4], l[5], l[6], l[7], l[8]) for l in rev[:2]] == [("1", "9", "ATG", "M", "GTG", "V", "10"), ("1", "9", "ATG", "M", "ATG", "M", "90")]
    assert rev[2][2] == "2" and rev[2][3] == "6" and not [l for l in lines if "\tlate\t" in l]
    assert len(lines) == 1 + 3 + 3 + 2 + 2 + 3


def test_aa_out_thresholds_on_hand_made_tables():
    calls = codon.aa_calls(hand_tables())
    assert ("fwd", "R1K", 60, 105, 60 / 105, [("AAG", 60)]) in calls
    assert [c[1] for c in calls if c[0] == "fwd"] == ["R1K", "F2L", "F2S"]          # (H3H is silent: no call)
    assert [c for c in calls if c[0] == "rev"][0][:4] == ("rev", "M1V", 10, 100)
    f = io.StringIO()
    codon.write_aa_tsv(f, "REF1", hand_tables())
    lines = f.getvalue().splitlines()
    assert lines[0] == "#ref\tcds\tchange\tcount\tdepth\tfreq\tcodons" and lines[1] == "REF1\tfwd\tR1K\t60\t105\t0.571429\tAAG:60"
    # min_depth: the codon at 5 has depth 30; min_freq: M1V stands at 0.1
    assert [c[1] for c in codon.aa_calls(hand_tables(min_depth=31)) if c[0] == "fwd"] == ["R1K"]
    assert [c[1] for c in codon.aa_calls(hand_tables(min_depth=30)) if c[0] == "fwd"] == ["R1K", "F2L", "F2S"]
    assert [c[1] for c in codon.aa_calls(hand_tables(min_freq=0.1)) if c[0] == "rev"][:1] == ["M1V"]
    assert "M1V" not in [c[1] for c in codon.aa_calls(hand_tables(min_freq=0.11))]
    # the triplets that were summed, largest first: two codons of one amino acid
    t = hand_tables()
    t.codon[t.cds.slot_of(2), U.cell_of("AAA")] = 70
    call = [c for c in codon.aa_calls(t) if c[1] == "R1K"][0]
    assert call[2] == 130 and call[5] == [("AAA", 70), ("AAG", 60)]


def test_stop_codons_are_written_as_a_star():
    cds = codon.CdsSet([("orf", 0, 3, "+")], 3)
    c = np.zeros((1, 65), np.uint32); c[0, U.cell_of("TAA")] = 9; c[0, U.cell_of("CAA")] = 1
    t = codon.Tables(cds, "CAA", c, [10, 0])
    assert keys(t.info(0, "C", ["T"]))["ALT_AA"] == "Q1*" and codon.aa_calls(t)[0][1] == "Q1*"


def args(tmp_path, **kw):
    ref = tmp_path / "ref.fas"
    if not ref.exists():
        ref.write_text(">r\nACGTACGTAC\n")
    base = dict(reference_fn=str(ref), trimmed_reads_fn=str(tmp_path / "none.bam"))
    base.update(kw)
    return base


def test_run_amplipy_refuses_the_flags_before_any_engine_exists(tmp_path, monkeypatch):
    from amplipy_amd import lib
    monkeypatch.setattr(lib, "Engine", lambda *a, **k: pytest.fail("an engine was made"))
    cds = str(tmp_path / "cds.tsv")
    for kw in (dict(run_variants=True, codon_out_fn="c.tsv"),                   # --codon_out needs --codons
               dict(run_variants=True, aa_out_fn="a.tsv"),                      # --aa_out needs --codons
               dict(run_trim=True, codons_fn=cds),                              # a run that only trims has no count table
               dict(run_trim=True, codons_fn=cds, codon_out_fn="c.tsv"),
               dict(run_consensus=True, codons_fn=cds, aa_out_fn="a.tsv")):     # --aa_out needs a run that calls variants
        with pytest.raises(SystemExit):
            amplipy.run_amplipy(**args(tmp_path, **kw))


def test_the_command_line_knows_the_flags():
    for cmd in (["variants", "-r", "r.fas"], ["consensus", "-r", "r.fas"], ["aio", "-p", "p.bed", "-r", "r.fas", "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas"]):
        a = amplipy.parse_args(cmd + ["--codons", "cds.tsv", "--codon_out", "c.tsv", "--aa_out", "a.tsv"])
        assert (a.codons, a.codon_out, a.aa_out) == ("cds.tsv", "c.tsv", "a.tsv")
        a = amplipy.parse_args(cmd)
        assert (a.codons, a.codon_out, a.aa_out) == (None, None, None)


def test_the_synthetic_job_carries_its_three_constructions():
    """tests/codon_util.synthetic_job on the oracle's trim results and the restatement: (a) the linked pair reads R>K on both
    records, (b) the two unlinked substitutions read differently and never meet, (c) the deletion breaks its codon."""
    j = U.synthetic_job()
    g, batch = j["genome"], j["batch"]
    G = int(g.size)
    pr = sorted((s, e) for s, e, _ in j["primers"])
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    r = oracle.process(batch, G, *tabs, 20, 4, do_trim=True, do_count=True)
    assert not r.trim.status.any() and 2500 <= batch.n <= 3500
    cds = U.cds_set(j["rows"], G)
    c, rd = U.tables(S.walked_segments(batch, r.trim), G, cds.starts, 20)
    U.check_at_most_counts(c, cds.starts, r.counts)
    t = codon.Tables(cds, synth.genome_string(g), c, rd, 1, 0.03)
    pa, pb, pc = j["pa"], j["pb"], j["pc"]
    num = (pa - j["rows"][0][1]) // 3 + 1
    for pos, ref in ((pa, "C"), (pa + 1, "G")):
        k = keys(t.info(pos, ref, ["A"]))
        assert k["CDS"].split("|")[0] == "orfA" and k["ALT_AA"].split("|")[0] == "R%dK" % num and k["ALT_CODON"].split("|")[0] == "CGG>AAG"
        assert 0.5 < int(k["ALT_CODON_DP"].split("|")[0]) / int(k["CODON_DP"].split("|")[0]) < 0.7 and int(k["CODON_DP"].split("|")[0]) > 200
        # the count table alone reads about 60 % A at either position
        assert 0.5 < r.counts[pos, 0] / r.counts[pos, :4].sum() < 0.7
    numb = (pb - j["rows"][0][1]) // 3 + 1
    assert keys(t.info(pb, "C", ["A"]))["ALT_AA"].split("|")[0] == "R%dR" % numb
    assert keys(t.info(pb + 1, "G", ["A"]))["ALT_AA"].split("|")[0] == "R%dQ" % numb
    cells = t.cells(pb)
    assert cells[U.cell_of("AAG")] == 0 and cells[U.cell_of("AGG")] > 50 and cells[U.cell_of("CAG")] > 50
    assert t.cells(pc)[64] > 50 and t.cells(pc - 3)[64] < 10 and t.cells(pc + 3)[64] < 10       # (the batch's own indels break a few)
    calls = [x for x in codon.aa_calls(t) if x[0] == "orfA"]
    assert ("R%dK" % num) in [x[1] for x in calls] and ("R%dQ" % numb) in [x[1] for x in calls] and ("R%dR" % numb) not in [x[1] for x in calls]
    assert int(rd[1]) == 0 or int(rd[0]) > 2000
