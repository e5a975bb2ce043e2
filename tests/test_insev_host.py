"""The host side of the insertion evidence (amplipy_amd/insevidence.py and the insertion half of deletion.DeletionReport) without
a GPU: the Python port of the allele hash against the CPU twin's; the join of device entries and allele texts with its three
error cases; the INS_N / INS text, the TSV file and RV on the insertion rows of the indel VCF; the header of every existing flag
combination unchanged with the new flags off; the argument errors; the merge of two ranks on a stub engine."""
import inspect
import io
import types

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, calling, deletion, insevidence, parallel, reports
from tests import insev_util as U

G = 9
REF = "ACGTACGTA"
COUNTS = (np.arange(G * abi.NSYM, dtype=np.uint32).reshape(G, abi.NSYM) % 7 + 40)


def make_run(**kw):
    args = {k: p.default for k, p in inspect.signature(amplipy.run_amplipy).parameters.items()}
    run = types.SimpleNamespace(**args)
    vars(run).update(dist=None, rank=0, world=1, device=0, min_quality=20, v_min_depth=0, v_min_freq=0.0, G=G, ref_id="R", ref_seq=REF)
    vars(run).update(kw)
    return run


def entry(pos, text, count, rev=0, noqual=0, qsum=0, bins=None):
    e = np.zeros(1, abi.INSEV_ENTRY_DTYPE)
    e[0] = (pos, len(text), insevidence.allele_hash(text), count, rev, noqual, qsum, bins if bins is not None else [count, 0, 0, 0, 0, 0, 0])
    return e


def entries(*rows):
    return np.concatenate(rows) if rows else np.zeros(0, abi.INSEV_ENTRY_DTYPE)


# ---- the hash ---------------------------------------------------------------------------------------------------------------------
def test_python_hash_against_the_twin_on_every_nt16_letter(tmp_path):
    L = U.load_twin(tmp_path)
    rng = np.random.default_rng(11)
    texts = [""] + list(U.NT16) + ["".join(U.NT16[k] for k in rng.integers(0, 16, int(rng.integers(2, 200)))) for _ in range(200)]
    assert all(U.twin_hash(L, t) == insevidence.allele_hash(t) for t in texts)
    assert insevidence.allele_hash("") == 0x9E3779B97F4A7C15 >> 1 and insevidence.key_of(7, "ACG")[:2] == (7, 3)


# ---- the join ---------------------------------------------------------------------------------------------------------------------
ROWS = [(4, "CGT", 5), (4, "CGA", 2), (4, "CG", 1), (1, "", 3), (7, "GTTTT", 40)]


def good_entries():
    return entries(entry(4, "CGT", 5, 2, 0, 5 * 3 * 30, [1, 1, 3, 0, 0, 0, 0]), entry(4, "CGA", 2, 1, 1, 90, [0, 0, 0, 0, 0, 0, 2]), entry(4, "CG", 1, 0, 1, 0),
                   entry(1, "", 3, 3, 0, 0), entry(7, "GTTTT", 40, 19, 0, 40 * 5 * 37, [0, 0, 0, 10, 10, 10, 10]))


def test_join_makes_one_allele_per_entry_in_order():
    # the store's rows may split an allele over batches and ranks
    triples = [(4, "CGT", 3), (7, "GTTTT", 40), (4, "CGT", 2), (4, "CGA", 2), (4, "CG", 1), (1, "", 3)]
    t = insevidence.Tables(good_entries(), triples, COUNTS, 0.0)
    assert [(a.pos, a.text, a.count, a.rev) for a in t.alleles] == [(1, "", 3, 3), (4, "CG", 1, 0), (4, "CGA", 2, 1), (4, "CGT", 5, 2), (7, "GTTTT", 40, 19)]
    assert t.rev_of(4, "CGT") == 2 and t.rev_of(4, "CCC") is None and t.rev_of(5, "CGT") is None
    assert insevidence.Tables(entries(), [], COUNTS).alleles == []


def test_join_miss_double_hit_and_count_mismatch_name_the_position():
    triples = [(p, s, c) for p, s, c in ROWS]
    with pytest.raises(insevidence.JoinError) as e:         # an allele of the run without an entry
        insevidence.Tables(good_entries()[:-1], triples, COUNTS)
    assert "position 8" in str(e.value) and "no entry" in str(e.value)
    with pytest.raises(insevidence.JoinError) as e:         # an entry without an allele of the run
        insevidence.Tables(good_entries(), triples[:-1], COUNTS)
    assert "position 8" in str(e.value) and "meets no allele" in str(e.value)
    with pytest.raises(insevidence.JoinError) as e:         # the counts differ
        insevidence.Tables(good_entries(), triples[:1] + [(4, "CGA", 3)] + triples[2:], COUNTS)
    assert "position 5" in str(e.value) and "counts 2 events" in str(e.value)
    # two texts of one position and length under one hash: a collision cannot be made to order, so the hash is stubbed
    real = insevidence.allele_hash
    try:
        insevidence.allele_hash = lambda text: real("CGT") if text == "CGA" else real(text)
        with pytest.raises(insevidence.JoinError) as e:
            insevidence.Tables(entries(entry(4, "CGT", 7)), [(4, "CGT", 5), (4, "CGA", 2)], COUNTS)
    finally:
        insevidence.allele_hash = real
    assert "position 5" in str(e.value) and "collision" in str(e.value)
    with pytest.raises(insevidence.JoinError) as e:         # one key twice among the entries
        insevidence.Tables(entries(entry(4, "CGT", 5), entry(4, "CGT", 5)), [(4, "CGT", 5)], COUNTS)
    assert "position 5" in str(e.value)


# ---- the text ---------------------------------------------------------------------------------------------------------------------
def test_ins_keys_tsv_and_rv():
    t = insevidence.Tables(good_entries(), ROWS, COUNTS, min_freq=0.03, end=8)
    assert t.info(4, 100) == "INS_N=3;INS=CGT:5:2:30:5"                       # 2 / 100 and 1 / 100 are below the frequency
    assert insevidence.Tables(good_entries(), ROWS, COUNTS, 0.0, 2).info(4, 100) == "INS_N=3;INS=CGT:5:2:30:1,CGA:2:1:30:0,CG:1:0:.:1"
    assert insevidence.Tables(good_entries(), ROWS, COUNTS, 0.0, 64).info(7, 50) == "INS_N=1;INS=GTTTT:40:19:37:30"
    assert t.info(0, 100) == "INS_N=0;INS=." and t.info(4, 0) == "INS_N=3;INS=."
    assert t.info(1, 3) == "INS_N=1;INS=:3:3:.:3"                              # the empty allele
    both = insevidence.IndelInfo(types.SimpleNamespace(info=lambda pos, dp: "DEL_N=0;DEL=."), t)
    assert both.info(4, 100) == "DEL_N=0;DEL=.;" + t.info(4, 100) and insevidence.IndelInfo(None, t).info(4, 100) == t.info(4, 100)
    f = io.StringIO()
    insevidence.write_tsv(f, "R", t)
    lines = f.getvalue().splitlines()
    assert lines[0] == "#ref\tpos\tallele\tlength\tcount\trev\tnoqual\tmean_qual\tb0\tb1\tb2\tb3\tb4\tb5\tb6\tdepth\tfreq"
    d4 = int(COUNTS[4].sum()) + 8
    assert lines[1:] == ["R\t2\t\t0\t3\t3\t0\t.\t3\t0\t0\t0\t0\t0\t0\t%d\t%.6g" % (int(COUNTS[1].sum()) + 3, 3 / (int(COUNTS[1].sum()) + 3)),
                         "R\t5\tCG\t2\t1\t0\t1\t.\t1\t0\t0\t0\t0\t0\t0\t%d\t%.6g" % (d4, 1 / d4),
                         "R\t5\tCGA\t3\t2\t1\t1\t30\t0\t0\t0\t0\t0\t0\t2\t%d\t%.6g" % (d4, 2 / d4),
                         "R\t5\tCGT\t3\t5\t2\t0\t30\t1\t1\t3\t0\t0\t0\t0\t%d\t%.6g" % (d4, 5 / d4),
                         "R\t8\tGTTTT\t5\t40\t19\t0\t37\t0\t0\t0\t10\t10\t10\t10\t%d\t%.6g" % (int(COUNTS[7].sum()) + 40, 40 / (int(COUNTS[7].sum()) + 40))]
    # the indel VCF: numeric RV on the insertion rows with the half on, '.' and the old header line with it off
    dt = deletion.Tables(np.array([(2, 2, 30, 7)], abi.DEL_EVENT_DTYPE), COUNTS, REF, 0, 0.0)
    ins = [(4, "CGT", 5, 100), (7, "GTTTT", 40, 90), (6, "GA", 9, 90)]
    off, on = io.StringIO(), io.StringIO()
    deletion.write_indel_vcf(off, "R", dt, ins, "src")
    deletion.write_indel_vcf(on, "R", dt, ins, "src", t)
    assert "(deletions only)" in off.getvalue() and "(deletions only)" not in on.getvalue()
    assert off.getvalue().replace(" (deletions only)", "").replace("AD=5;RV=.", "AD=5;RV=2").replace("AD=40;RV=.", "AD=40;RV=19") == on.getvalue()
    assert "AD=9;RV=.;" in on.getvalue() and "AD=30;RV=7;" in on.getvalue()           # (an allele the table does not hold stays '.')


# ---- the header -------------------------------------------------------------------------------------------------------------------
def test_header_unchanged_with_the_flag_off_and_two_lines_with_it_on(tmp_path):
    combos = [dict(), dict(deletion=True), dict(strand=True, deletion=True, readpos=True), dict(codon=True, hap=True),
              dict(zip(calling.INFO_ORDER, [True] * 8))]
    for k, on in enumerate(combos):
        texts = []
        for name, kw in (("off", {}), ("default", None), ("on", dict(insertions=True))):
            fn = str(tmp_path / ("%d%s.vcf" % (k, name)))
            w = amplipy.VcfWriter(fn, "REF", **on, **(kw or {})) if kw is not None else amplipy.VcfWriter(fn, "REF", *[on.get(n, False) for n in calling.INFO_ORDER])
            w.close()
            texts.append(open(fn).read())
        want = "".join(R.HEADER_LINES for R in reports.REGISTRY if on.get(R.name))
        assert texts[0] == texts[1] and texts[0].endswith("\">\n" + want + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")
        assert "INS_N" not in texts[0] and texts[2].count("##INFO=<ID=") == texts[0].count("##INFO=<ID=") + 2
        # behind the deletion keys' place
        front = "".join(R.HEADER_LINES for R in reports.REGISTRY[:4] if on.get(R.name))
        assert texts[2].replace(insevidence.HEADER_LINES, "") == texts[0] and (front + insevidence.HEADER_LINES) in texts[2]
    assert insevidence.HEADER_LINES.count("\n") == 2 and all(("ID=%s," % k) in insevidence.HEADER_LINES for k in insevidence.KEYS)


def test_vcf_line_appends_the_keys_behind_the_deletion_keys():
    r = calling.VariantRecord(4, "A", ["C", "ACGT"], 100, 60, [30, 5], 0.6, [0.3, 0.05], (0, 1, 2))
    t = insevidence.Tables(good_entries(), ROWS, COUNTS)
    rep = deletion.DeletionReport()
    stand_in = types.SimpleNamespace(info=lambda pos, dp: "DEL_N=0;DEL=.")
    rep.tables = deletion.IndelTables(stand_in, t)
    info = lambda run: calling.vcf_line("R", r, deletion=rep.vcf_tables(run)).split("\t")[7]
    assert info(make_run(run_variants=True, deletions=True, insertions=True)).endswith("ALT_FREQ=0.3,0.05;DEL_N=0;DEL=.;" + t.info(4, 100))
    assert info(make_run(run_variants=True, insertions=True)).endswith("ALT_FREQ=0.3,0.05;" + t.info(4, 100))
    assert info(make_run(run_variants=True, deletions=True, ins_out_fn="i.tsv")).endswith("ALT_FREQ=0.3,0.05;DEL_N=0;DEL=.")
    assert rep.vcf_tables(make_run(run_variants=True, ins_out_fn="i.tsv")) is None


# ---- the arguments ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(run_trim=True, insertions=True), "only trims"), (dict(run_trim=True, ins_out_fn="i.tsv"), "only trims"),
    (dict(run_consensus=True, insertions=True), "need a VCF"), (dict(run_variants=True, ins_capacity=12), "--ins_capacity"),
    (dict(run_variants=True, insertions=True, ins_capacity=3), "4 to 28"), (dict(run_variants=True, insertions=True, ins_capacity=29), "4 to 28"),
    (dict(run_variants=True, ins_end=8), "--ins_end"), (dict(run_variants=True, insertions=True, ins_end=5), "one of 2, 4, 8, 16, 32, 64")])
def test_flag_errors(kw, word, capsys):
    with pytest.raises(SystemExit):
        deletion.DeletionReport().check(make_run(**kw))
    assert word in capsys.readouterr().err


def test_flags_switch_the_halves():
    rep = deletion.DeletionReport()
    for kw, halves in [(dict(), (False, False)), (dict(deletions=True), (True, False)), (dict(insertions=True), (False, True)),
                       (dict(ins_out_fn="i.tsv"), (False, True)), (dict(indel_vcf_fn="x.vcf", insertions=True), (True, True)),
                       (dict(run_consensus=True, ins_out_fn="i.tsv.gz", ins_capacity=20, ins_end=64), (False, True))]:
        run = make_run(**{"run_variants": True, **kw})
        rep.check(run)
        assert (rep.del_on(run), rep.ins_on(run)) == halves and rep.active(run) == any(halves)
        calls = []
        eng = types.SimpleNamespace(del_enable=lambda c: calls.append(("del", c)), insev_enable=lambda c: calls.append(("ins", c)))
        rep.enable(run, eng)
        assert [c[0] for c in calls] == [n for n, h in zip(("del", "ins"), halves) if h]
    args = amplipy.parse_args(["variants", "-i", "a.bam", "-r", "r.fas", "-o", "o.vcf", "--insertions", "--ins_out", "i.tsv", "--ins_capacity", "12", "--ins_end", "16"])
    assert (args.insertions, args.ins_out, args.ins_capacity, args.ins_end) == (True, "i.tsv", 12, 16)
    assert amplipy.parse_args(["consensus", "-i", "a.bam", "-r", "r.fas", "-o", "o.fas", "--ins_out", "i.tsv"]).ins_out == "i.tsv"


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------
class StubEngine:
    """Per rank: a deletion table and an insertion table with one allele on both ranks, one on one rank only."""

    def __init__(self, rank, lost=0, with_insev=True):
        self.rank, self.lost = rank, lost
        if with_insev:
            self.insev_entries = self._insev_entries

    def counts(self):
        return COUNTS.copy()

    def del_events(self):
        return np.array([(1, 2, 3 + self.rank, 1)], abi.DEL_EVENT_DTYPE), {"used": 1, "capacity": 16, "lost": 0}

    def _insev_entries(self):
        rows = [entry(4, "CGT", 5 + self.rank, 2, 0, (5 + self.rank) * 90, [1, 1, 3 + self.rank, 0, 0, 0, 0])]
        rows.append(entry(7, "GTTTT", 4, 1, 1, 3 * 5 * 20, [0, 0, 0, 0, 0, 0, 4]) if self.rank else entry(1, "", 3, 3))
        return entries(*rows), {"used": 2, "capacity": 16, "lost": self.lost}


def store(rank):
    rows = [(4, "CGT", 5 + rank), (7, "GTTTT", 4) if rank else (1, "", 3)]
    return types.SimpleNamespace(counted_pairs=lambda: list(rows))


def collect(monkeypatch, rank, answer, lost=0, **kw):
    calls = []

    def gather_objects(d, r, w, obj, dst=0):
        calls.append(obj)
        return answer(len(calls) - 1, obj)
    monkeypatch.setattr(parallel, "gather_objects", gather_objects)
    run = make_run(run_variants=True, dist=object(), rank=rank, world=2, ins_store=store(rank), **kw)
    rep = deletion.DeletionReport()
    rep.collect(run, StubEngine(rank, lost))
    return rep, run, calls


def test_two_rank_merge_on_a_stub(monkeypatch):
    kw = dict(deletions=True, insertions=True, ins_end=4)
    sent = [collect(monkeypatch, rank, lambda k, x: [x, x], **kw)[2] for rank in (0, 1)]
    assert len(sent[0]) == len(sent[1]) == 2                 # the deletion events' gather as it was, then one more
    assert [len(s) for s in sent[0]] == [2, 3] and sent[0][0][0].dtype == abi.DEL_EVENT_DTYPE and sent[0][1][0].dtype == abi.INSEV_ENTRY_DTYPE
    rep, run, _ = collect(monkeypatch, 0, lambda k, x: [sent[0][k], sent[1][k]], **kw)
    t = rep.tables
    assert isinstance(t, deletion.IndelTables) and t.deletion.events["count"].tolist() == [7]
    assert [(a.pos, a.text, a.count, a.rev, a.noqual, a.qsum, a.bins) for a in t.insertion.alleles] == [
        (1, "", 3, 3, 0, 0, [3, 0, 0, 0, 0, 0, 0]), (4, "CGT", 11, 4, 0, 11 * 90, [2, 2, 7, 0, 0, 0, 0]), (7, "GTTTT", 4, 1, 1, 300, [0, 0, 0, 0, 0, 0, 4])]
    assert rep.vcf_tables(run).info(4, 100) == "DEL_N=0;DEL=.;INS_N=1;INS=CGT:11:4:30:4"
    rep.after(run)
    # rank 1 makes no tables; with the insertion flags off no rank calls anything new, and the one gather is the old one
    rep1, _, _ = collect(monkeypatch, 1, lambda k, x: None, **kw)
    assert rep1.tables is None
    old, _, calls = collect(monkeypatch, 0, lambda k, x: [x, x], deletions=True)
    assert len(calls) == 1 and isinstance(old.tables, deletion.Tables)
    monkeypatch.setattr(parallel, "gather_objects", lambda *a, **k: [a[3], a[3]])
    plain = deletion.DeletionReport()
    plain.collect(make_run(run_variants=True, dist=object(), rank=0, world=2, deletions=True), StubEngine(0, with_insev=False))
    assert isinstance(plain.tables, deletion.Tables)
    # lost events are summed over the ranks and end the run in after(), never silently
    rep, run, _ = collect(monkeypatch, 0, lambda k, x: [x, x] if k == 0 else [(x[0], dict(x[1], lost=2), x[2]), (x[0], dict(x[1], lost=3), x[2])], **kw)
    assert rep.ins_lost == 5
    with pytest.raises(RuntimeError):          # in front of the VCF's records: no header without its keys is left behind
        rep.vcf_tables(run)
    with pytest.raises(RuntimeError) as e:
        rep.after(run)
    assert "--ins_capacity" in str(e.value) and "5 events" in str(e.value)


def test_merge_entries_sums_per_key_in_order():
    a = entries(entry(4, "CGT", 5, 2, 0, 450, [1, 1, 3, 0, 0, 0, 0]), entry(1, "", 3, 3))
    b = entries(entry(4, "CGT", 1, 1, 1, 0, [0, 0, 0, 0, 0, 0, 1]), entry(4, "CG", 2, 0, 0, 100))
    m = insevidence.merge_entries([a, b])
    assert [(int(e["ref_pos"]), int(e["len"]), int(e["count"])) for e in m] == [(1, 0, 3), (4, 2, 2), (4, 3, 6)]
    assert m[2]["bin"].tolist() == [1, 1, 3, 0, 0, 0, 1] and (int(m[2]["rev"]), int(m[2]["noqual"]), int(m[2]["qsum"])) == (3, 1, 450)
    assert insevidence.merge_entries([]).size == 0
