"""Calling on the CPU suite: the device's per-position decision (amp_call.hpp, run here through tests/hostsim) plus the host
finish (amplipy_amd/calling.py) against a plain restatement of the reference's calling loop (oracle/py_restatement.py),
on seeded tables with ties, insertion alleles at the edges of the relevance rule, thresholds at equality and one below,
and reference symbols that are not upper-case ACGT (tests/call_util.py).  k_call_compact is GPU-only: tests/test_gpu_calling.py."""
import numpy as np
import pytest

from amplipy_amd import abi, calling, synth
from oracle import py_restatement
from tests import call_util as U
from tests import helpers as H
from tests import hostsim

SIZES = [1, 7, 255, 256, 257, 700]


class EngineStub:
    """What calling.call asks of an engine when the per-position records are handed to it."""

    def __init__(self, counts):
        self._counts = counts
        self.ref_len = counts.shape[0]

    def counts(self):
        return self._counts


def twin_call(ref_seq, counts, ins_at, provider, params, full):
    cp = U.call_params(params, full_ranking=full)
    pc, n_rel = hostsim.call_positions(counts, ins_at, ref_seq, cp)
    assert n_rel == int(((pc["flags"] & abi.CALL_INS_RELEVANT) != 0).sum())
    return calling.call(EngineStub(counts), ref_seq, cp, provider, positions=(pc, n_rel), want_alleles=full)


# ---- the restatement itself, anchored to the reference-derived fixtures --------------------------------------------------
def golden_tables(g):
    tables = [dict.fromkeys(U.SYMS, 0) for _ in range(g["ref_len"])]
    for p, k, n in g["counts"]:
        tables[p][k] = n
    return tables


def golden_ref(g):
    return g.get("ref_seq") or synth.genome_string(synth.make_genome())


@pytest.fixture(scope="module", params=["pileup_5000.json.gz", "pileup_notrim_1500.json.gz"])
def golden(request):
    g = H.load_json(request.param)
    return g, golden_ref(g), golden_tables(g)


def test_restatement_reproduces_golden_calls(golden):
    """call_positions over the committed counts gives the committed calls: consensus, variant dicts, totals, ranked lists with
    hex frequencies (the fixture's calls come from the reference's own alleles_from_counts)."""
    g, ref_seq, tables = golden
    got = py_restatement.call_positions(ref_seq, tables, g["params"])
    want = {c["pos"]: c for c in g["calls"]}
    assert len(want) > 1000
    for p, (cons, rec, total, ranked) in enumerate(got):
        w = want.get(p)
        if w is None:
            assert (cons, rec, total, ranked) == (None, None, 0, []), p
            continue
        assert total == w["total"], p
        assert [[n, float(f).hex(), s] for n, f, s in ranked] == w["alleles"], p
        assert cons == w.get("consensus"), p
        assert rec == w.get("variant"), p
        assert py_restatement.alleles_from_counts(tables[p]) == (total, ranked)


@pytest.mark.parametrize("full", [False, True])
def test_golden_pileups_through_the_twin(golden, full):
    g, ref_seq, tables = golden
    G = g["ref_len"]
    counts = np.array([[t[s] for s in U.SYMS] for t in tables], np.uint32)
    pairs = [(p, k) for p, k, n in g["counts"] if not U._is_base(k) for _ in range(n)]
    ins_at = np.bincount(np.array([p for p, _ in pairs], np.int64), minlength=G).astype(np.uint32)
    params = dict(g["params"], run_consensus=1, run_variants=1)
    res = twin_call(ref_seq, counts, ins_at, lambda pos: calling.tallies_from_events(pairs, pos), params, full)
    U.assert_matches(res, ref_seq, py_restatement.call_positions(ref_seq, tables, params), full, "golden")


# ---- seeded tables ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SIZES)
def case(request):
    G = request.param
    seed, pseeds = U.SEEDS[G]
    c = U.Case(seed, G)
    draws = [U.make_params(s, c.tables, c.ref_seq) for s in pseeds[:8]]
    expects = [py_restatement.call_positions(c.ref_seq, c.tables, pr) for pr in draws]
    return c, draws, expects


def test_case_meets_minimums(case):
    c, draws, expects = case
    assert len(draws) == 8
    U.assert_minimums(c.G, [U.classes(c.ref_seq, c.tables, pr, e) for pr, e in zip(draws, expects)])


def test_read_pass_twin_builds_the_same_table(case):
    """The insertion reads through the device's per-read functions on the CPU: the table the calling twin starts from."""
    c, _, _ = case
    if not c.reads.n:
        return
    r = hostsim.process(c.reads, c.G, None, None, 0, U.MIN_QUALITY, 4, do_trim=False)
    assert not r.trim.status.any()
    assert np.array_equal(c.base_counts + r.counts, c.counts)
    assert sorted(U.event_strings(c.reads, r.events)) == sorted(c.pairs)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("draw", range(8))
def test_twin_matches_restatement(case, draw, full):
    c, draws, expects = case
    U.assert_minimums(c.G, [U.classes(c.ref_seq, c.tables, pr, e) for pr, e in zip(draws, expects)])
    res = twin_call(c.ref_seq, c.counts, c.ins_at, c.provider, draws[draw], full)
    U.assert_matches(res, c.ref_seq, expects[draw], full, (c.G, draw, draws[draw]))


def test_relevant_flag_is_the_rule(case):
    """AMP_CALL_INS_RELEVANT is set exactly where the rule says (insertions >= the top base, or at / above min_freq_variants
    of the depth when variants run, or full_ranking) and nowhere else; the 32-bit depth and the ranked order are the table's."""
    c, draws, expects = case
    for pr, expect in zip(draws, expects):
        for full in (False, True):
            pc, n_rel = hostsim.call_positions(c.counts, c.ins_at, c.ref_seq, U.call_params(pr, full))
            for p, (cons, rec, total, ranked) in enumerate(expect):
                n_ins = int(c.ins_at[p])
                top = int(c.counts[p].max())
                want = n_ins > 0 and (full or n_ins >= top or bool(pr["run_variants"] and n_ins / total >= pr["min_freq_variants"]))
                assert bool(pc["flags"][p] & abi.CALL_INS_RELEVANT) == want, (p, pr, full)
                assert int(pc["total_depth"][p]) == total
                order = int(pc["order"][p])
                nnz = (order >> 18) & 7
                got = [(int(c.counts[p, (order >> (3 * k)) & 7]), U.SYMS[(order >> (3 * k)) & 7]) for k in range(nnz)]
                assert got == [(n, s) for n, f, s in ranked if U._is_base(s)], (p, pr)
                assert sorted((order >> (3 * k)) & 7 for k in range(6)) == list(range(6)), p


@pytest.mark.parametrize("kind", U.EXTREMES)
def test_compaction_extremes_on_the_twin(kind):
    """The tables of the GPU compaction extremes (tests/test_gpu_calling.py): the expectation they are held to is reachable from
    the twin too, and the read shape that puts an insertion at the last position counts the same in the device's walk."""
    G = 257
    c = U.Case(0, G, U.extreme_case(kind, G))
    if c.reads.n:
        r = hostsim.process(c.reads, G, None, None, 0, U.MIN_QUALITY, 4, do_trim=False)
        assert not r.trim.status.any() and not r.counts.any()
        assert sorted(U.event_strings(c.reads, r.events)) == sorted(c.pairs) == [(p, "CA") for p in range(G)]
    expect = py_restatement.call_positions(c.ref_seq, c.tables, U.EXTREME_PARAMS)
    n_rec = sum(e[1] is not None for e in expect)
    assert n_rec == {"no_record": 0, "all_records": G, "only_first": 1, "only_last": 1, "all_relevant": G}[kind]
    for full in (False, True):
        res = twin_call(c.ref_seq, c.counts, c.ins_at, c.provider, U.EXTREME_PARAMS, full)
        assert res.n_relevant == (G if kind == "all_relevant" else 0)
        U.assert_matches(res, c.ref_seq, expect, full, kind)
