"""The report protocol of the command line on the host (amplipy_amd/reports.py): the one order that the
registry, the VCF keywords and the device's hook enum share; which arguments switch a report on and which put keys on the VCF;
and that the ranks of a run issue the same collectives and rank 0 ends with the job's tables.  No GPU: ``collect`` runs on a stub
engine with the collectives of ``parallel`` replaced by recorders."""
import inspect
import os
import re
import types

import numpy as np
import pytest

from amplipy_amd import abi, amplicon, amplipy, calling, codon, cooc, deletion, errprof, haplotype, parallel, readpos, reports, strand

MODULES = (strand, amplicon, codon, deletion, cooc, errprof, haplotype, readpos)      # in the order under test
HOOK_HPP = os.path.join(os.path.dirname(os.path.abspath(amplipy.__file__)), "csrc", "amp_hook.hpp")


def make_run(**kw):
    """The ``run`` of a run_amplipy call with the keyword arguments ``kw``, every other one at its default."""
    args = {k: p.default for k, p in inspect.signature(amplipy.run_amplipy).parameters.items()}
    assert not set(kw) - set(args) - {"dist", "rank", "world", "G", "ref_id", "ref_seq"}
    run = types.SimpleNamespace(**args)
    vars(run).update(dist=None, rank=0, world=1, device=0, min_quality=20, v_min_depth=0, v_min_freq=0.0)
    vars(run).update(kw)
    return run


# ---- one order ------------------------------------------------------------------------------------------------------------------
def test_registry_info_order_and_hook_enum_agree():
    assert [R.name for R in reports.REGISTRY] == list(calling.INFO_ORDER)
    with open(HOOK_HPP) as f:
        enum = re.search(r"enum \{ (HOOK_QC, .*?, N_HOOKS) \};", f.read()).group(1).split(", ")
    assert enum[0] == "HOOK_QC" and enum[-1] == "N_HOOKS"
    # (the one hook without a registry entry of its own: the deletion report drives it, and it runs directly behind k_del)
    assert enum.index("HOOK_INSEV") == enum.index("HOOK_DEL") + 1
    names = [n[len("HOOK_"):].lower() for n in enum[1:-1] if n != "HOOK_INSEV"]
    assert [{"del": "deletion"}.get(n, n) for n in names] == list(calling.INFO_ORDER)
    assert [R.HEADER_LINES for R in reports.REGISTRY] == [m.HEADER_LINES for m in MODULES]


def test_header_lines_in_order_in_front_of_chrom(tmp_path):
    fn = str(tmp_path / "all.vcf")
    w = amplipy.VcfWriter(fn, "REF", True, True, True, True, True, True, True, True)
    w.close()
    with open(fn) as f:
        text = f.read()
    tail = "".join(m.HEADER_LINES for m in MODULES) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n"
    assert text.endswith(tail) and text.count("##INFO=<ID=") == 5 + (5 + 7 + 5 + 2 + 1 + 2 + 2 + 6)      # (the keys of each report)
    fn = str(tmp_path / "two.vcf")
    w = amplipy.VcfWriter(fn, "REF", codon=True, hap=True)
    w.close()
    with open(fn) as f:
        assert f.read().endswith("\">\n" + codon.HEADER_LINES + haplotype.HEADER_LINES + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")


class StandIn:
    def __init__(self, name):
        self.name, self.got = name, []

    def info(self, *a):
        self.got.append(a)
        return self.name


def test_vcf_line_loops_over_the_order():
    r = calling.VariantRecord(6, "C", ["A", "GT"], 50, 30, [15, 5], 0.6, [0.3, 0.1], (0, 1, 2))
    ins = [StandIn(n) for n in calling.INFO_ORDER]
    line = calling.vcf_line("REF", r, *ins)
    assert line.split("\t")[7] == "DP=50;REF_DP=30;ALT_DP=15,5;REF_FREQ=0.6;ALT_FREQ=0.3,0.1;" + ";".join(calling.INFO_ORDER)
    for s in ins:
        assert s.got == [(6, 50) if s.name == "deletion" else (6, "C", ["A", "GT"])], s.name
    some = {n: StandIn(n) for n in ("readpos", "deletion", "strand")}
    assert calling.vcf_line("REF", r, **some).split("\t")[7].endswith("ALT_FREQ=0.3,0.1;strand;deletion;readpos")
    assert calling.vcf_line("REF", r) == calling.vcf_line("REF", r, *[None] * 8) and ";" + "strand" not in calling.vcf_line("REF", r)


# ---- which arguments switch what on ---------------------------------------------------------------------------------------------
def test_off_is_off():
    run = make_run(run_variants=True)
    for R in reports.REGISTRY:
        r = R()
        assert not r.active(run) and r.vcf_tables(run) is None and r.files() in ([], [None], [None, None]), R.name
        r.check(run)                                                    # (nothing to complain of)


@pytest.mark.parametrize("name,arg,value,keys", [
    ("strand", "strand_fn", "s.tsv", False), ("readpos", "readpos_fn", "rp.tsv", False), ("deletion", "del_out_fn", "del.tsv", False),
    ("deletion", "indel_vcf_fn", "indel.vcf", False), ("strand", "strand", True, True), ("readpos", "readpos", True, True), ("deletion", "deletions", True, True),
    ("amplicon", "amplicons_fn", "a.tsv", True), ("codon", "codons_fn", "cds.tsv", True), ("cooc", "cooc_fn", "sets.tsv", True),
    ("errprof", "error_profile_fn", "ep.json", True), ("hap", "haplotypes_fn", "r.bed", True)])
def test_switch_with_and_without_keys(name, arg, value, keys):
    run = make_run(run_trim=True, run_variants=True, run_consensus=True, **{arg: value})
    tables = object()
    for R in reports.REGISTRY:
        r = R()
        assert r.active(run) == (R.name == name), R.name
        r.check(run)
        r.tables = tables
        if R.name == name:
            assert r.annotates(run) == keys and r.vcf_tables(run) is (tables if keys else None)


# ---- collectives ----------------------------------------------------------------------------------------------------------------
G = 9
REF = "ACGTACGTA"
COUNTS = (np.arange(G * abi.NSYM, dtype=np.uint32).reshape(G, abi.NSYM) % 7 + 40)      # the job's count table: both ranks hold it


def hap_entry(region, diffs, count, rev):
    e = np.zeros(1, abi.HAP_ENTRY_DTYPE)
    e["head"] = region | (len(diffs) << 16)
    e["diff"][0, :len(diffs)] = [off | (kind << 12) | (length << 15) for off, kind, length in diffs]
    e["count"], e["rev"] = count, rev
    return e


class StubEngine:
    """Small fixed tables in the shapes lib.Engine documents, other numbers on either rank."""

    def __init__(self, rank):
        self.rank = rank

    def u(self, shape, dtype, hi=9):
        """The same numbers at every call of one method of one rank."""
        return np.random.default_rng([17, self.rank, int(np.prod(shape)), hi]).integers(0, hi, shape).astype(dtype)

    def counts(self):
        return COUNTS.copy()

    def strand_tables(self):
        return self.u((G, abi.NSYM), np.uint32), self.u((G, abi.STRAND_QSUM_COLS), np.uint64, 300)

    def readpos_tables(self):
        return self.u((G, abi.NSYM, abi.RP_BINS), np.uint32)

    def amplicon_tables(self):                  # 2 amplicons with spans [0, 5) and [3, 9): 11 cells
        return self.u((11, abi.NSYM), np.uint32), self.u(3, np.uint64, 50)

    def codon_tables(self):                     # 2 codon slots
        return self.u((2, abi.CODON_CELLS), np.uint32), self.u(2, np.uint64, 50)

    def cooc_tables(self):                      # 2 sets
        return self.u((2, abi.COOC_CELLS), np.uint32), self.u(2, np.uint64, 50)

    def errprof_tables(self):
        return self.u(abi.EP_CYC_SHAPE, np.uint64), self.u(abi.EP_QUAL_SHAPE, np.uint64), self.u(abi.EP_SUB_SHAPE, np.uint64, 90), self.u(2, np.uint64, 50)

    def del_events(self):                       # 3 events a rank, two of the keys on both ranks
        ev = np.array([(1, 2, 3 + self.rank, 1), (4, 1, 2, self.rank), (6 - 6 * self.rank, 2, 5, 2)], abi.DEL_EVENT_DTYPE)
        return ev, {"used": 3, "capacity": 16, "lost": 0}

    def hap_tables(self):                       # 2 regions, 3 entries a rank, two of the keys on both ranks
        entries = np.concatenate([hap_entry(0, [(1, 0, 0)], 4 + self.rank, 1), hap_entry(1, [(0, abi.HAP_KIND_DEL, 2), (3, 2, 0)], 3, self.rank),
                                  hap_entry(self.rank, [(2, 3, 0)], 2, 2)])
        tally = np.zeros((2, abi.HAP_TALLY_COLS), np.uint64)
        tally[:, abi.HAP_REF] = [5, 6 + self.rank]
        tally[:, abi.HAP_REF_REV] = [2, 3]
        tally[:, abi.HAP_LOWQ] = [1, self.rank]
        for e in entries:
            tally[int(e["head"]) & 0xFFFF, abi.HAP_COVER] += e["count"]
        tally[:, abi.HAP_COVER] += tally[:, [abi.HAP_REF, abi.HAP_LOWQ]].sum(axis=1)
        return entries, {"used": 3, "capacity": 16, "lost": 0}, tally, np.array([20 + self.rank, 7], np.uint64)


def loaded_reports():
    """One instance per report with what ``open`` would have loaded."""
    made = {R.name: R() for R in reports.REGISTRY}
    made["amplicon"].amps = amplicon.AmpliconSet(["a1", "a2"], [0, 3], [5, 9], [(0, 1, "a1_L", 0), (3, 4, "a2_L", 1)], [(4, 5, "a1_R", 0), (8, 9, "a2_R", 1)],
                                                 np.full(G, -1, np.int32), np.full(G, -1, np.int32),
                                                 [(0, 1, "a1_L"), (3, 4, "a2_L"), (4, 5, "a1_R"), (8, 9, "a2_R")], G)
    made["codon"].cds = codon.parse_cds("orf\t0\t6\n", G)
    made["cooc"].sets = cooc.parse_sets("s1\tA1C\ns2\tC2A,G3T\n", REF)
    made["errprof"].mask = np.arange(G) == 4
    made["hap"].regions = haplotype.parse_regions("R\t0\t4\tr1\nR\t4\t9\tr2\n", "R", G)
    assert made["codon"].cds.n_slots == 2 and made["cooc"].sets.n_sets == 2 and made["amplicon"].amps.cells == 11
    return list(made.values())


def rank_run(dist, rank, world):
    return make_run(run_trim=True, run_variants=True, run_consensus=True, dist=dist, rank=rank, world=world, G=G, ref_id="R", ref_seq=REF,
                    strand=True, readpos=True, deletions=True, amplicons_fn="a", codons_fn="c", cooc_fn="o", error_profile_fn="e", haplotypes_fn="h")


def collect_all(monkeypatch, dist, rank, world, answer):
    """``collect`` of every report on a stub engine -> (the reports, [(kind, report, array length or None, what was sent)]).
    ``answer(kind, k, sent)``: what the k-th collective gives back."""
    calls, now = [], [None]

    def allreduce_numpy(d, device, wire):
        assert d is dist and wire.dtype == np.int64 and wire.ndim == 1
        calls.append(("allreduce", now[0], len(wire), wire))
        return answer("allreduce", len(calls) - 1, wire)

    def gather_objects(d, r, w, obj, dst=0):
        assert d is dist and (r, w, dst) == (rank, world, 0)
        calls.append(("gather", now[0], None, obj))
        return answer("gather", len(calls) - 1, obj)

    monkeypatch.setattr(parallel, "allreduce_numpy", allreduce_numpy)
    monkeypatch.setattr(parallel, "gather_objects", gather_objects)
    reps, eng, run = loaded_reports(), StubEngine(rank), rank_run(dist, rank, world)
    for r in reps:
        assert r.active(run)
        now[0] = r.name
        r.collect(run, eng)
    return reps, calls


RECORDS = [(1, "C", ["A", "-"], 44), (4, "A", ["C", "GT"], 51)]


def infos(tables):
    return [t.info(p, dp) if name == "deletion" else t.info(p, ref, alts) for name, t in zip(calling.INFO_ORDER, tables) for p, ref, alts, dp in RECORDS]


def test_both_ranks_issue_the_same_collectives_and_rank_0_gets_the_jobs_tables(monkeypatch):
    dist = object()
    # what either rank sends, in order (the answers of this pass are the rank's own: nothing of it is used)
    sent = [[c[3] for c in collect_all(monkeypatch, dist, rank, 2, lambda kind, k, x: x if kind == "allreduce" else [x, x])[1]] for rank in (0, 1)]
    assert len(sent[0]) == len(sent[1])
    got = {}
    for rank in (0, 1):
        answer = lambda kind, k, x: sent[0][k] + sent[1][k] if kind == "allreduce" else [sent[0][k], sent[1][k]] if rank == 0 else None
        got[rank] = collect_all(monkeypatch, dist, rank, 2, answer)
    seq = [[c[:3] for c in got[rank][1]] for rank in (0, 1)]
    assert seq[0] == seq[1]
    assert [c[1] for c in seq[0]] == ["strand", "amplicon", "amplicon", "codon", "codon", "deletion", "cooc", "cooc", "errprof", "hap", "readpos"]
    assert {c[1]: c[2] for c in seq[0] if c[0] == "allreduce"} == {
        "strand": G * abi.STRAND_CELLS, "amplicon": 11 * abi.NSYM, "codon": 2 * abi.CODON_CELLS, "cooc": 2 * abi.COOC_CELLS,
        "errprof": sum(int(np.prod(s)) for s in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE)) + 2, "readpos": G * abi.RP_CELLS}
    assert all(r.tables is None for r in got[1][0])
    assert all(r.lost == 0 for rank in (0, 1) for r in got[rank][0])

    # the same tables from the two ranks' engines directly: element-wise sums, merge_events, merge_entries
    e0, e1 = StubEngine(0), StubEngine(1)
    both = lambda name: [getattr(e, name)() for e in (e0, e1)]
    by = {r.name: r for r in loaded_reports()}
    run = rank_run(None, 0, 1)
    add = lambda parts, k: parts[0][k] + parts[1][k]
    s, a, c, o, ep, rp, d, h = (both(n) for n in ("strand_tables", "amplicon_tables", "codon_tables", "cooc_tables", "errprof_tables", "readpos_tables",
                                                  "del_events", "hap_tables"))
    want = [strand.Tables(COUNTS, add(s, 0), add(s, 1)),
            amplicon.Tables(by["amplicon"].amps, COUNTS, add(a, 0), add(a, 1)),
            codon.Tables(by["codon"].cds, REF, add(c, 0), add(c, 1), run.v_min_depth, run.v_min_freq),
            deletion.Tables(deletion.merge_events([d[0][0], d[1][0]]), COUNTS, REF, run.v_min_depth, run.v_min_freq),
            cooc.Tables(by["cooc"].sets, add(o, 0), add(o, 1)),
            errprof.Tables(*[add(ep, k) for k in range(4)], 20, 1, COUNTS),
            haplotype.Tables(by["hap"].regions, REF, haplotype.merge_entries([h[0][0], h[1][0]]), add(h, 2), add(h, 3), 0, 2, 0.0, run.v_min_freq),
            readpos.Tables(COUNTS, rp[0] + rp[1], readpos.DEFAULT_END)]
    tables = [r.tables for r in got[0][0]]
    assert [type(t) for t in tables] == [type(t) for t in want]
    assert infos(tables) == infos(want)
    text = " ".join(infos(want))
    assert "DEL_N=2;DEL=2-3:7:2,1-2:5:2" in text and "DEL_N=1;DEL=5-5:4:1" in text and "HAP_N=1;HAP=r1:C2A:9:" in text        # (keys of both ranks were summed: 3 + 4 reads, 4 + 5 reads)
    assert [int(x) for x in tables[1].amp_reads] == [int(x) for x in add(a, 1)] and tables[6].reads.tolist() == [41, 14]
    assert len(tables[3].events) == 4 and sum(len(x) for x in tables[6].haps) == 4


def test_one_process_issues_no_collective(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a collective without ranks")
    monkeypatch.setattr(parallel, "allreduce_table", refuse)
    monkeypatch.setattr(parallel, "gather_objects", refuse)
    reps, eng, run = loaded_reports(), StubEngine(0), rank_run(None, 0, 1)
    for r in reps:
        r.collect(run, eng)
    assert all(r.tables is not None for r in reps)
    e = StubEngine(0)
    assert np.array_equal(reps[0].tables.rev, e.strand_tables()[0]) and reps[3].tables.events.tolist() == np.sort(e.del_events()[0], order=["start", "len"]).tolist()
