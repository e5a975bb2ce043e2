"""Calling on the device -- k_call, k_call_compact, the pinned image of amp_call_compact_begin, the copying
amp_call_compact -- against the plain restatement of the reference's calling loop (oracle/py_restatement.py) and against
the CPU twin of the per-position decision (tests/hostsim), on the seeded tables of tests/call_util.py: ties among all six
symbols, insertion alleles at the edges of the relevance rule, thresholds at equality and one below, reference symbols
that are not upper-case ACGT, and reference lengths of 1, around one block, and past the first trip of the compaction's
prefix loop (70,003 positions: 274 blocks, a partial last one)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from amplipy_amd import abi, calling, lib
from amplipy_amd.insertions import event_strings
from oracle import py_restatement
from tests import call_util as U
from tests import hostsim

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 700, 70003]
DRAWS = [(G, d) for G in SIZES for d in range(2 if G > U.LARGE else 6)]
EXTREME_SIZES = [256, 257, 70003]          # 256: the last thread of the last block is live (it writes the totals)
EXTREME_CASES = [(G, k) for G in EXTREME_SIZES for k in U.EXTREMES if k != "all_relevant" or G == 257]
AMP_EOVERFLOW = -6
FIELDS = ("total_depth", "ref_count", "order", "consensus_sym", "flags", "alt_mask")


def load(e, c):
    """The table of case ``c`` on a reset engine: injected counts, then the insertion reads through the read pass."""
    e.reset()
    e.set_primers(np.full(c.G, -1, np.int32), np.full(c.G, -1, np.int32), 0)
    e.set_params(U.MIN_QUALITY, 4, False, True)
    e.add_counts(c.base_counts)
    if c.reads.n:
        assert not e.process(c.reads).status.any()
    e.set_reference(c.ref_seq)
    assert np.array_equal(e.counts(), c.counts)
    pairs = event_strings(c.reads, e.events()) if c.reads.n else []
    assert sorted(pairs) == sorted(c.pairs)
    return lambda positions: calling.tallies_from_events(pairs, positions)      # allele text from the DEVICE's events


class Bench:
    """One default engine per reference length and the seeded case of that length; ``use`` puts a table on the engine."""

    def __init__(self):
        self.engines, self.cases, self.loaded = {}, {}, {}

    def case(self, G):
        if G not in self.cases:
            seed, pseeds = U.SEEDS[G]
            c = U.Case(seed, G)
            draws = [U.make_params(s, c.tables, c.ref_seq) for s in pseeds[:2 if G > U.LARGE else 6]]
            expects = [py_restatement.call_positions(c.ref_seq, c.tables, pr) for pr in draws]
            per_draw = [U.classes(c.ref_seq, c.tables, pr, x) for pr, x in zip(draws, expects)]
            self.cases[G] = SimpleNamespace(c=c, draws=draws, expects=expects, per_draw=per_draw)
        return self.cases[G]

    def use(self, G, key, c):
        if G not in self.engines:
            self.engines[G] = lib.Engine(G)
        e = self.engines[G]
        if self.loaded.get(G, (None,))[0] != key:
            self.loaded[G] = (key, load(e, c))
        return e, self.loaded[G][1]

    def seeded(self, G):
        k = self.case(G)
        U.assert_minimums(G, k.per_draw)            # a condition of every comparison below, not a measurement
        e, provider = self.use(G, "seeded", k.c)
        return k, e, provider

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def sim(c, cp):
    return hostsim.call_positions(c.counts, c.ins_at, c.ref_seq, cp)


def check_compact(cons, vr, rel, pc, c, cp, expect):
    """(c) of the module: the arrays of one compaction against the twin's flags and the restatement's records."""
    flags = pc["flags"]
    is_rel = (flags & abi.CALL_INS_RELEVANT) != 0
    want_rel = np.nonzero(is_rel)[0]
    want_var = np.nonzero(((flags & abi.CALL_VARIANT) != 0) & ~is_rel)[0]
    pos = vr["pos"].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and np.all(np.diff(rel.astype(np.int64)) > 0)
    assert not set(pos.tolist()) & set(rel.tolist())
    assert np.array_equal(pos, want_var) and np.array_equal(rel, want_rel)
    assert np.array_equal(cons, pc["consensus_sym"])
    assert set(pos.tolist()) == {p for p, x in enumerate(expect) if x[1] is not None and not is_rel[p]}
    n = pos.size
    want = np.zeros(n, abi.VAR_REC_DTYPE)           # the records as the restatement has them; padding 0xFF / 0
    want["pos"] = pos
    cols = np.full((n, 6), 0xFF, np.uint8)
    cnts = np.zeros((n, 6), np.uint32)
    for i, p in enumerate(pos.tolist()):
        rec = expect[p][1]
        na = len(rec["alts"])
        cols[i, :na] = [U.SYMS.index(a) for a in rec["alts"]]
        cnts[i, :na] = [int(x) for x in rec["ALT_DP"].split(",")]
        want[i] = (p, rec["DP"], rec["REF_DP"], na, rec["GT"][0] == 0, cols[i], cnts[i])
    for f in abi.VAR_REC_DTYPE.names:
        assert np.array_equal(vr[f], want[f]), (f, pos[np.nonzero((vr[f] != want[f]).reshape(n, -1).any(1))[0][:5]])


def amp_call_compact(e, cp, vars_cap, rel_cap):
    """The copying entry point through ctypes -> (rc, consensus, records, relevant, n_vars, n_relevant)."""
    cons = np.full(e.ref_len, 99, np.int8)
    vr = np.zeros(max(vars_cap, 1), abi.VAR_REC_DTYPE)
    rel = np.zeros(max(rel_cap, 1), np.int32)
    nv, nr = C.c_int64(-1), C.c_int64(-1)
    rc = e.L.amp_call_compact(e.h, C.byref(cp), C.c_void_p(abi.ptr(cons)), C.c_void_p(abi.ptr(vr)), C.c_int64(vars_cap), C.byref(nv),
                              C.c_void_p(abi.ptr(rel)), C.c_int64(rel_cap), C.byref(nr))
    return rc, cons, vr[:vars_cap], rel[:rel_cap], int(nv.value), int(nr.value)


def same_outcome(a, b):
    return np.array_equal(a.consensus_sym, b.consensus_sym) and a.consensus_ins == b.consensus_ins and a.vcf_text("x") == b.vcf_text("x")


@pytest.mark.parametrize("G,draw", DRAWS)
def test_positions_match_the_twin(bench, G, draw):
    """(a) amp_call_positions against the same decision run on the CPU: every field of amp_pos_call, and n_relevant."""
    k, e, _ = bench.seeded(G)
    for full in (False, True):
        cp = U.call_params(k.draws[draw], full)
        got, n_rel = e.call_positions(cp)
        want, want_rel = sim(k.c, cp)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), (f, full, np.nonzero(got[f] != want[f])[0][:5])
        assert n_rel == want_rel


@pytest.mark.parametrize("G,draw", DRAWS)
def test_three_ways_to_call_match_the_restatement(bench, G, draw):
    """(b) calling.call by default, with the full ranking, and behind amp_call_compact_begin (the pinned image)."""
    k, e, provider = bench.seeded(G)
    pr, expect, c = k.draws[draw], k.expects[draw], k.c
    cp = U.call_params(pr)
    plain = calling.call(e, c.ref_seq, cp, provider)
    image = e._cv[0].consensus
    U.assert_matches(plain, c.ref_seq, expect, False, (G, draw, pr, "default"))
    full = calling.call(e, c.ref_seq, U.call_params(pr, True), provider, want_alleles=True)
    U.assert_matches(full, c.ref_seq, expect, True, (G, draw, pr, "full ranking"))
    e.call_compact_begin(cp)
    begun = calling.call(e, c.ref_seq, cp, provider)
    assert e._cv[0].consensus != image, "the call behind call_compact_begin did not pick up the pinned image"
    U.assert_matches(begun, c.ref_seq, expect, False, (G, draw, pr, "begun"))
    assert same_outcome(plain, full) and same_outcome(plain, begun)
    assert plain.n_relevant == begun.n_relevant <= full.n_relevant == int((c.ins_at > 0).sum())


@pytest.mark.parametrize("G,draw", DRAWS)
def test_compact_arrays(bench, G, draw):
    """(c) the raw arrays of amp_call_compact_view, plain and pinned, and (d) the copying amp_call_compact with exact capacities
    and with either one short."""
    k, e, _ = bench.seeded(G)
    pr, expect, c = k.draws[draw], k.expects[draw], k.c
    cp = U.call_params(pr)
    pc, n_rel = sim(c, cp)
    cons, vr, rel = [x.copy() for x in e.call_compact(cp)]
    check_compact(cons, vr, rel, pc, c, cp, expect)
    assert rel.size == n_rel
    e.call_compact_begin(cp)
    cons2, vr2, rel2 = [x.copy() for x in e.call_compact(cp)]
    assert np.array_equal(cons, cons2) and np.array_equal(vr, vr2) and np.array_equal(rel, rel2)
    nv, nr = vr.size, rel.size
    rc, cons3, vr3, rel3, nv3, nr3 = amp_call_compact(e, cp, nv, nr)
    assert (rc, nv3, nr3) == (0, nv, nr)
    assert np.array_equal(cons, cons3) and np.array_equal(vr, vr3) and np.array_equal(rel, rel3)
    if nv:
        rc, _, _, _, nv4, nr4 = amp_call_compact(e, cp, nv - 1, nr)
        assert (rc, nv4, nr4) == (AMP_EOVERFLOW, nv, nr)
    if nr:
        rc, _, _, _, nv4, nr4 = amp_call_compact(e, cp, nv, nr - 1)
        assert (rc, nv4, nr4) == (AMP_EOVERFLOW, nv, nr)


@pytest.mark.parametrize("G,kind", EXTREME_CASES)
def test_compaction_extremes(bench, G, kind):
    """No record at all, every position a record, every position relevant, the only record at position 0 and at G - 1 (with
    G = 256 that one sits in the thread that writes the totals)."""
    c = U.Case(0, G, U.extreme_case(kind, G))
    e, provider = bench.use(G, kind, c)
    pr = U.EXTREME_PARAMS
    cp = U.call_params(pr)
    expect = py_restatement.call_positions(c.ref_seq, c.tables, pr)
    pc, n_rel = sim(c, cp)
    want_nv, want_nr = {"no_record": (0, 0), "all_records": (G, 0), "only_first": (1, 0), "only_last": (1, 0), "all_relevant": (0, G)}[kind]
    for begin in (False, True):
        if begin:
            e.call_compact_begin(cp)
        cons, vr, rel = [x.copy() for x in e.call_compact(cp)]
        assert (vr.size, rel.size) == (want_nv, want_nr) and n_rel == want_nr
        check_compact(cons, vr, rel, pc, c, cp, expect)
    if kind == "only_first":
        assert vr["pos"].tolist() == [0]
    if kind == "only_last":
        assert vr["pos"].tolist() == [G - 1]
    got, got_rel = e.call_positions(cp)
    for f in FIELDS:
        assert np.array_equal(got[f], pc[f]), f
    assert got_rel == n_rel
    U.assert_matches(calling.call(e, c.ref_seq, cp, provider), c.ref_seq, expect, False, (G, kind))
    rc, cons3, vr3, rel3, nv3, nr3 = amp_call_compact(e, cp, want_nv, want_nr)
    assert (rc, nv3, nr3) == (0, want_nv, want_nr)
    assert np.array_equal(cons, cons3) and np.array_equal(vr, vr3) and np.array_equal(rel, rel3)


def test_no_reference_set(bench):
    """A context that never got a reference calls the consensus; asking it for variants is a state error, on every entry point."""
    k = bench.case(257)
    c = k.c
    e = lib.Engine(257)
    try:
        e.add_counts(c.counts)
        pr = dict(k.draws[0], run_consensus=1, run_variants=0)
        cp = U.call_params(pr)
        got, n_rel = e.call_positions(cp)
        want, want_rel = hostsim.call_positions(c.counts, np.zeros(257, np.uint32), None, cp)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), f
        assert n_rel == want_rel == 0
        assert np.array_equal(e.call_compact(cp)[0], want["consensus_sym"])
        cpv = U.call_params(dict(pr, run_variants=1))
        for fn in (e.call_positions, e.call_compact, e.call_compact_begin):
            with pytest.raises(lib.AmpliHipError):
                fn(cpv)
    finally:
        e.close()


def test_reset_then_the_same_case(bench):
    """amp_reset empties the table and the insertion counts; the same case loaded again calls the same."""
    G = 257
    k, e, provider = bench.seeded(G)
    c, pr = k.c, k.draws[0]
    cp = U.call_params(pr)
    first, first_rel = e.call_positions(cp)
    e.reset()
    bench.loaded.pop(G)
    empty, empty_rel = e.call_positions(cp)
    assert not empty["total_depth"].any() and empty_rel == 0 and not (empty["flags"] & abi.CALL_INS_RELEVANT).any()
    e, provider = bench.use(G, "seeded", c)
    again, again_rel = e.call_positions(cp)
    for f in FIELDS:
        assert np.array_equal(first[f], again[f]), f
    assert first_rel == again_rel
    U.assert_matches(calling.call(e, c.ref_seq, cp, provider), c.ref_seq, k.expects[0], False, "after reset")
