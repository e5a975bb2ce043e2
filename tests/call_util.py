"""Seeded tables for the calling tests (k_call / k_call_compact, amp_call.hpp, amplipy_amd/calling.py).

Nothing is committed but seeds.  A case is a reference string, a table of base counts (they go in through
Engine.add_counts) and a batch of tiny reads whose only purpose is to put insertion alleles where the case wants them:
insertion events reach the device only through the read pass.  What a position is EXPECTED to hold never comes from the
device: injected counts + the oracle's counts of those reads + the strings of the oracle's insertion events.

Rows are random (empty; k symbols sharing one small value; all six symbols in 0..3; a dominant base plus noise; a third of
them with 1-3 insertion alleles counted around the top base) or DESIGNED: one block (BLOCK below) laid at position 0,
across 255/256 and ending at G - 1, where it fits, and at further places in a large table.

Two read shapes carry an allele S to position p without touching any base count (first and last base below the quality
threshold): ``1M kI 1M`` at p with SEQ = S + one base, and, for the empty allele, ``2I 1M`` at p + 1 (a CIGAR that starts
with I: the slice A:736-738 takes is empty).  Random rows also use ``aM kI bM`` with every base counted.  Reads are
counted untrimmed (do_trim off), with min_quality 20 and no primers.
"""
from collections import Counter
from types import SimpleNamespace

import numpy as np

from amplipy_amd import abi, calling
from amplipy_amd.amplipy import VcfWriter
from amplipy_amd.batch import ReadBatch
from amplipy_amd.insertions import event_strings
from amplipy_amd.segment import Segment
from oracle import oracle
from oracle.py_restatement import call_positions

SYMS = abi.SYMBOLS
MIN_QUALITY = 20
LARGE = 1000                      # tables longer than this repeat the block and ask for 20 of every class


def _row(ref, base=None, ins=(), classes=()):
    return {"ref": ref, "base": dict(base or {}), "ins": list(ins), "classes": tuple(classes)}


# The designed rows.  ``classes``: the structural classes (see classes()) the row is there for.  Rows 0..6 need no
# insertion, so a 7-position table holds them; an insertion row at p needs p + 1 inside the reference, so the last row has none.
BLOCK = [
    _row("G", dict(A=2, C=2, G=2, T=2, N=2, **{"-": 2}), classes=("tie6", "tie_dash", "tie_N", "six_nonzero")),
    _row("C", classes=("depth0",)),
    _row("A", dict(T=3, N=3, A=1), classes=("tie2", "tie_N")),
    _row("A", dict(A=4, **{"-": 4}), classes=("tie2", "tie_dash", "ref_on_top")),
    _row("T", dict(C=3, G=3, T=1, **{"-": 3}), classes=("tie3", "tie_dash")),
    _row("A", dict(A=2, **{"-": 5}), classes=("top_dash",)),
    _row("N", dict(N=4, C=1), classes=("top_N", "ref_N_with", "ref_on_top")),
    _row("A", dict(A=2), [("AGG", 3)], classes=("ins_on_top",)),
    _row("T", dict(T=3), [("TA", 3)], classes=("ins_tied_wins",)),                    # "TA" > "T"
    _row("C", dict(C=3), [("AC", 3)], classes=("ins_tied_loses",)),                   # "AC" < "C"
    _row("G", {"-": 2}, [("", 2)], classes=("empty_allele", "ins_tied_loses", "top_dash")),   # "" < "-"
    _row("G", dict(G=40, A=1), [("GT", 1)], classes=("ins_present",)),                # 1/42: under the top and under 0.03
    _row("G", dict(G=10), [("GC", 4)], classes=("ins_present",)),                     # under the top, 4/14 of the depth
    _row("C", {}, [("CA", 2)], classes=("ins_only",)),
    _row("A", dict(A=3), [("AC", 2), ("AG", 2)], classes=("two_alleles_same_len",)),
    _row("T", dict(T=6), [("TGGA", 9)], classes=("allele_many_reads", "ins_on_top")),
    _row("a", dict(A=5, C=1), classes=("ref_lower",)),
    _row("R", dict(G=4, A=3), classes=("ref_R", "ref_absent")),
    _row("N", dict(A=3, T=2), classes=("ref_N_without", "ref_absent")),
    _row("N", dict(N=2, A=5, C=1), classes=("ref_N_with",)),
    _row("-", dict(A=4, **{"-": 3}), classes=("ref_dash_del",)),
    _row("C", dict(C=1, A=30, T=10), classes=()),                                     # 1/41: GT lacks 0 at 0.03
    _row("G", dict(G=9, T=2), classes=("ref_on_top",)),
    _row("T", dict(A=5, C=4), classes=("ref_absent",)),
    _row("A", dict(A=7, C=6, G=5, T=4, N=3, **{"-": 2}), classes=("six_nonzero",)),   # five ALTs in ranked order
    _row("N", dict(A=3, C=3, G=2, T=2, N=1, **{"-": 1}), classes=("six_nonzero", "tie2")),
    _row("T", dict(N=4, T=4, **{"-": 4}), classes=("tie3", "tie_N", "tie_dash", "ref_on_top")),
    _row("G", dict(G=2, C=2), classes=("tie2", "ref_on_top")),
]
NB = len(BLOCK)

STRUCTURAL = ("depth0", "tie2", "tie3", "tie6", "tie_dash", "tie_N", "top_dash", "top_N", "six_nonzero", "ins_present",
              "ins_on_top", "ins_tied_wins", "ins_tied_loses", "ins_only", "empty_allele", "two_alleles_same_len",
              "allele_many_reads", "ref_lower", "ref_R", "ref_N_with", "ref_N_without", "ref_dash_del",
              "ref_on_top", "ref_absent")
# classes that depend on the thresholds: counted over all the draws of one table
THRESHOLD = ("ins_irrelevant", "ins_freq_relevant", "gt_lacks_ref", "alts_3_or_more", "ins_alt",
             "depth_consensus_eq", "depth_consensus_below", "depth_variants_eq", "depth_variants_below",
             "depth_ref_eq", "depth_ref_below", "freq_consensus_eq", "freq_consensus_below",
             "freq_variants_eq", "freq_variants_below")
RUN_FLAGS = ("consensus_off", "variants_off")         # per draw, not per position: asked of the small tables (six draws and more)


def block_starts(G):
    """Where the block is laid: position 0 (cut to the table), across 255/256, ending at G - 1 -- each where it does not run
    into another -- and, in a large table, every 2,800 positions, so that every designed class occurs more than 20 times."""
    starts = [0]
    if G >= 2 * NB:
        starts.append(G - NB)
    if 256 - NB // 2 + NB <= G - NB:
        starts.append(256 - NB // 2)
    if G > LARGE:
        starts += [s for s in range(1400, G - 2 * NB, 2800)]
    return sorted(starts)


def _is_base(s):
    return len(s) == 1 and s in SYMS


def _allele_reads(rng, p, s, n, G, free):
    """``n`` reads that add the insertion allele ``s`` at position ``p``.  ``free``: None = only the two shapes that touch no base
    count; else bool[G], positions a read may add base counts to."""
    out = []
    for _ in range(n):
        if s == "":
            seq = "".join(rng.choice(list("ACGT"), 3))
            out.append(Segment(0, p + 1, "2I1M", 0, seq, [40, 40, 2]))
            continue
        k = len(s) - 1
        a, b = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        if free is not None and rng.random() < 0.5 and p - a + 1 >= 0 and p + b < G and free[p - a + 1:p + b + 1].all():
            seq = "".join(rng.choice(list("ACGT"), a - 1)) + s + "".join(rng.choice(list("ACGT"), b))
            out.append(Segment(0, p - a + 1, "%dM%dI%dM" % (a, k, b), 0, seq, [40] * len(seq)))
        else:
            seq = s + "ACGT"[int(rng.integers(4))]
            out.append(Segment(0, p, "1M%dI1M" % k, 0, seq, [2] + [40] * k + [2]))
    return out


def make_case(seed, G):
    """(ref_seq, base_counts uint32[G, 6], insertion_reads ReadBatch) of table ``seed`` over ``G`` positions."""
    rng = np.random.default_rng(seed)
    # random rows
    kind = rng.choice(4, G, p=[0.2, 0.25, 0.3, 0.25])
    share = (rng.random((G, 6)).argsort(1).argsort(1) < rng.integers(1, 7, G)[:, None]) * rng.integers(1, 5, G)[:, None]
    six = rng.integers(0, 4, (G, 6))
    dom = rng.integers(0, 3, (G, 6))
    dom[np.arange(G), rng.integers(0, 6, G)] = rng.integers(8, 21, G)
    base = np.where((kind == 1)[:, None], share, np.where((kind == 2)[:, None], six, np.where((kind == 3)[:, None], dom, 0)))
    base = base.astype(np.uint32)
    ref = rng.choice(list("ACGT"), G)
    odd = rng.random(G) < 0.08
    ref[odd] = rng.choice(list("aRN-"), int(odd.sum()))
    # designed rows
    free = np.ones(G, bool)
    segs = []
    for s0 in block_starts(G):
        for j, row in enumerate(BLOCK):
            p = s0 + j
            if p >= G:
                break
            free[p] = False
            ref[p] = row["ref"]
            base[p] = [row["base"].get(s, 0) for s in SYMS]
            if p + 1 < G:
                for s, n in row["ins"]:
                    segs += _allele_reads(rng, p, s, n, G, None)
    # insertion alleles on random rows: a third of them (fewer in a large table: one read per event)
    cand = np.nonzero(free[:G - 1] & (rng.random(G)[:G - 1] < min(1 / 3, 1500 / G)))[0] if G > 1 else []
    for p in cand:
        p = int(p)
        top = int(base[p].max())
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(1, 4)) if rng.random() < 0.9 else int(rng.integers(4, 15))
            s = "" if rng.random() < 0.05 else "".join(rng.choice(list("ACGTN"), k + 1, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
            segs += _allele_reads(rng, p, s, max(1, top + int(rng.integers(-2, 3))), G, free)
    segs.sort(key=lambda s: s.reference_start)
    return "".join(ref), base, ReadBatch.from_segments(segs)


EXTREMES = ("no_record", "all_records", "only_first", "only_last", "all_relevant")
EXTREME_PARAMS = {"min_depth_consensus": 1, "min_freq_consensus": 0.0, "min_depth_variants": 1, "min_freq_variants": 0.03,
                  "run_consensus": 1, "run_variants": 1}


def extreme_case(kind, G):
    """The ends of the compaction, as (ref_seq, base_counts, reads): no record at all; every position a record; the only record
    at position 0 / at G - 1; every position insertion-relevant (one insertion read per position and no base at all; the last
    position's read ends ``1M 1I 1S``, there is no position behind it for a match)."""
    ref_seq = ("ACGT" * (G // 4 + 1))[:G]
    col = np.arange(G) % 4
    base = np.zeros((G, 6), np.uint32)
    segs = []
    if kind == "all_relevant":
        segs = [Segment(0, p, "1M1I1M", 0, "CAG", [2, 40, 2]) for p in range(G - 1)] + [Segment(0, G - 1, "1M1I1S", 0, "CAG", [2, 40, 40])]
    else:
        base[np.arange(G), col] = 5
        if kind == "all_records":
            base[np.arange(G), (col + 1) % 4] = 3
        elif kind == "only_first":
            base[0, 5] = 4
        elif kind == "only_last":
            base[G - 1, 4] = 6
        else:
            assert kind == "no_record"
    return ref_seq, base, ReadBatch.from_segments(segs)


class Case:
    """A case with everything the CPU can say about it: the oracle's read pass over the insertion reads, the table the
    device must hold afterwards (``counts``, ``ins_at``), the allele strings and the per-position dicts calling starts from."""

    def __init__(self, seed, G, parts=None):
        self.seed, self.G = seed, G
        self.ref_seq, self.base_counts, self.reads = parts if parts is not None else make_case(seed, G)
        if self.reads.n:
            r = oracle.process(self.reads, G, min_quality=MIN_QUALITY, window=4, do_trim=False)
            assert not r.trim.status.any()
            self.counts = self.base_counts + r.counts
            self.pairs = event_strings(self.reads, r.events)
        else:
            self.counts = self.base_counts.copy()
            self.pairs = []
        self.ins_at = np.bincount(np.array([p for p, _ in self.pairs], np.int64), minlength=G).astype(np.uint32)
        self.tables = tables_from(self.counts, self.pairs)

    def provider(self, positions):
        return calling.tallies_from_events(self.pairs, positions)


def tables_from(counts, pairs):
    """One {symbol or insertion string: count} per position, the shape of the reference's table (A:892, A:745-748)."""
    tables = [dict(zip(SYMS, row)) for row in counts.tolist()]
    for p, s in pairs:
        tables[p][s] = tables[p].get(s, 0) + 1
    return tables


def make_params(seed, tables, ref_seq=None):
    """Thresholds drawn from the table itself: frequencies from {0, 1, 0.03, 1/3, the exact count / depth of a chosen base symbol
    and of a chosen insertion allele, and the same with the count lowered by one}; depths from {0, 1, a chosen row's top
    count, top + 1, depth, depth + 1, count of its reference symbol}; one of three settings of the run flags."""
    rng = np.random.default_rng(seed)
    rows = [p for p, t in enumerate(tables) if any(t.values())]
    ins_rows = [p for p in rows if any(n and not _is_base(s) for s, n in tables[p].items())]

    def freq():
        pool = [0.0, 1.0, 0.03, 1 / 3]
        if rows:
            t = tables[rows[int(rng.integers(len(rows)))]]
            n = int(rng.choice([t[s] for s in SYMS if t[s]] or [1]))
            pool += [n / sum(t.values()), (n - 1) / sum(t.values())]
        if ins_rows:
            t = tables[ins_rows[int(rng.integers(len(ins_rows)))]]
            n = int(rng.choice([c for s, c in t.items() if c and not _is_base(s)]))
            pool += [n / sum(t.values()), (n - 1) / sum(t.values())]
        return float(pool[int(rng.integers(len(pool)))])

    def depth():
        pool = [0, 1]
        if rows:
            p = rows[int(rng.integers(len(rows)))]
            t = tables[p]
            pool += [max(t.values()), max(t.values()) + 1, sum(t.values()), sum(t.values()) + 1]
            if ref_seq is not None:
                pool.append(t.get(ref_seq[p], 0))
        return int(pool[int(rng.integers(len(pool)))])

    run_c, run_v = [(1, 1), (1, 1), (1, 0), (0, 1)][int(rng.integers(4))]
    return {"min_depth_consensus": depth(), "min_freq_consensus": freq(), "min_depth_variants": depth(),
            "min_freq_variants": freq(), "run_consensus": run_c, "run_variants": run_v}


def call_params(params, full_ranking=False):
    return calling.call_params(params["min_depth_consensus"], params["min_freq_consensus"], params["min_depth_variants"],
                               params["min_freq_variants"], params["run_consensus"], params["run_variants"], full_ranking)


def classes(ref_seq, tables, params, expect=None):
    """Counter: how many positions fall into each class of STRUCTURAL and THRESHOLD, judged from the tables and the plain
    restatement's result alone.  "below" = one count short of the threshold."""
    expect = expect if expect is not None else call_positions(ref_seq, tables, params)
    dc, fc = params["min_depth_consensus"], params["min_freq_consensus"]
    dv, fv = params["min_depth_variants"], params["min_freq_variants"]
    run_c, run_v = params["run_consensus"], params["run_variants"]
    k = Counter()
    if not run_c:
        k["consensus_off"] += 1
    if not run_v:
        k["variants_off"] += 1
    for p, (cons, rec, total, ranked) in enumerate(expect):
        if total == 0:
            k["depth0"] += 1
            continue
        t, rs = tables[p], ref_seq[p]
        bases = [(n, s) for n, f, s in ranked if _is_base(s)]
        ins = [(n, s) for n, f, s in ranked if not _is_base(s)]
        top_base = bases[0][0] if bases else 0
        tied = [s for n, s in bases if n == top_base]
        if len(tied) in (2, 3, 6):
            k["tie%d" % len(tied)] += 1
        if len(tied) > 1 and "-" in tied:
            k["tie_dash"] += 1
        if len(tied) > 1 and "N" in tied:
            k["tie_N"] += 1
        if bases and bases[0][1] == "-":
            k["top_dash"] += 1
        if bases and bases[0][1] == "N":
            k["top_N"] += 1
        if len(bases) == 6:
            k["six_nonzero"] += 1
        if ins:
            n_ins = sum(n for n, s in ins)
            k["ins_present"] += 1
            if not bases:
                k["ins_only"] += 1
            elif ins[0][0] > top_base:
                k["ins_on_top"] += 1
            elif ins[0][0] == top_base:
                k["ins_tied_wins" if not _is_base(ranked[0][2]) else "ins_tied_loses"] += 1
            if any(s == "" for n, s in ins):
                k["empty_allele"] += 1
            if len(set(len(s) for n, s in ins)) < len(ins):
                k["two_alleles_same_len"] += 1
            if ins[0][0] >= 5:
                k["allele_many_reads"] += 1
            if n_ins < top_base:
                k["ins_freq_relevant" if run_v and n_ins / total >= fv else "ins_irrelevant"] += 1
        if rs == "a" and t["A"]:
            k["ref_lower"] += 1
        if rs == "R":
            k["ref_R"] += 1
        if rs == "N":
            k["ref_N_with" if t["N"] else "ref_N_without"] += 1
        if rs == "-" and t["-"]:
            k["ref_dash_del"] += 1
        if ranked[0][2] == rs:
            k["ref_on_top"] += 1
        if not t.get(rs, 0):
            k["ref_absent"] += 1
        if run_c:
            n, f = ranked[0][0], ranked[0][1]
            k["depth_consensus_eq"] += n == dc
            k["depth_consensus_below"] += n == dc - 1
            k["freq_consensus_eq"] += f == fc
            k["freq_consensus_below"] += f < fc <= (n + 1) / total
        if run_v:
            k["depth_variants_eq"] += total == dv
            k["depth_variants_below"] += total == dv - 1
            others = [(n, f) for n, f, s in ranked if s != rs]
            k["freq_variants_eq"] += any(f == fv for n, f in others)
            k["freq_variants_below"] += any(f < fv <= (n + 1) / total for n, f in others)
            if total >= dv and any(f >= fv for n, f in others):
                k["depth_ref_eq"] += t.get(rs, 0) == dv
                k["depth_ref_below"] += t.get(rs, 0) == dv - 1
        if rec is not None:
            k["gt_lacks_ref"] += rec["GT"][0] == 1 and rec["REF_DP"] > 0
            k["alts_3_or_more"] += len(rec["alts"]) >= 3
            k["ins_alt"] += any(not _is_base(s) for s in rec["alts"])
    return k


def required(G):
    """(structural classes every draw must show, threshold classes the draws of one table must show together, minimum).  A table
    that holds only part of the block answers for the rows that fit; thresholds are asked of tables that hold it whole."""
    if G >= NB:
        return STRUCTURAL, THRESHOLD, (20 if G > LARGE else 1)
    fit = set()
    for j, row in enumerate(BLOCK[:G]):
        if not row["ins"] or j + 1 < G:
            fit.update(row["classes"])
    return tuple(c for c in STRUCTURAL if c in fit), (), 1


def assert_minimums(G, per_draw):
    """The condition every test checks before it compares anything: ``per_draw`` = one classes() Counter per parameter draw."""
    structural, threshold, least = required(G)
    for k in per_draw:
        short = {c: k[c] for c in structural if k[c] < least}
        assert not short, "table of %d positions lacks designed rows: %r" % (G, short)
    total = sum(per_draw, Counter())
    short = {c: total[c] for c in threshold if total[c] < least}
    if threshold and len(per_draw) >= 6:
        short.update({c: 0 for c in RUN_FLAGS if not total[c]})
    assert not short, "the parameter draws of table %d miss threshold classes: %r" % (G, short)


# ---- comparing a CallResult with the restatement ----------------------------------------------------------------------
def assert_matches(res, ref_seq, expect, full, tag=""):
    """``res`` (calling.CallResult) against ``expect`` (py_restatement.call_positions) at every position: consensus list and
    string, records as dicts, with ``full`` the ranked alleles too, and the VCF text against the records' own."""
    cons = res.consensus
    want_cons = [e[0] for e in expect]
    assert cons == want_cons, (tag, [(p, a, b) for p, (a, b) in enumerate(zip(cons, want_cons)) if a != b][:5])
    assert res.consensus_string("N") == "".join("N" if c is None else c for c in want_cons), tag
    got = {r.pos: r.as_dict() for r in res.records}
    want = {p: e[1] for p, e in enumerate(expect) if e[1] is not None}
    assert got == want, (tag, [(p, got.get(p), want.get(p)) for p in sorted(set(got) | set(want)) if got.get(p) != want.get(p)][:3])
    assert res.n_records == len(want), tag
    if full:
        want_all = {p: (e[2], [(n, float(f).hex(), s) for n, f, s in e[3]]) for p, e in enumerate(expect) if e[2]}
        got_all = {p: (t, [(n, float(f).hex(), s) for n, f, s in ranked]) for p, (t, ranked) in res.alleles.items()}
        assert got_all == want_all, (tag, [p for p in sorted(set(got_all) | set(want_all)) if got_all.get(p) != want_all.get(p)][:5])
    writer = SimpleNamespace(ref_id="x")
    assert res.vcf_text("x") == "".join(VcfWriter.line(writer, r) for r in res.records), tag


# ---- committed seeds: chosen on the CPU so that the restatement alone meets assert_minimums ----------------------------------
# {G: (table seed, [parameter seeds])}; the CPU twin uses all eight draws of the small tables, the GPU tests the first six
# (two for the large table).
SEEDS = {
    1: (1001, [0, 1, 2, 3, 4, 5, 6, 7]),
    7: (1007, [0, 1, 2, 3, 4, 5, 6, 7]),
    255: (1255, [24, 0, 4, 1, 2, 3, 5, 6]),
    256: (1256, [24, 0, 4, 1, 2, 3, 5, 6]),
    257: (1257, [36, 0, 4, 1, 2, 3, 5, 6]),
    700: (1700, [36, 0, 4, 1, 2, 3, 5, 6]),
    70003: (71003, [1, 0]),
}
