"""The kernels behind a fast kernel on grids of any size, and the calling kernels as one launch.

k_tile<LIST> (the general pass) and k_deferred_heavy (the heavy pass) walk their list segments in a block-stride loop and are
launched with as many blocks as the engine's previous pass would have kept busy (amp_plan.hpp: gen_blocks / heavy_blocks), so a
batch whose lists are far longer than predicted runs on a handful of blocks.  Every output -- count table, the six per-read
arrays, events -- is compared with the oracle, whatever the grid.  amp_call_compact_begin runs k_call_fused; its image is
compared with the two-kernel path (amp_call_compact_view without a begin), with the CPU twin and with the restatement."""
import numpy as np
import pytest

from amplipy_amd import lib, synth
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from oracle import oracle, py_restatement
from tests import call_util as U
from tests import hostsim
from tests.gpu_util import EV_ORDER, Result, assert_same
from tests.test_gpu_calling import check_compact
from tests.test_gpu_parity import _long_read_segments

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scheme():
    g = synth.make_genome()
    primers, amps = synth.make_artic_scheme()
    mn, mx, mpl = oracle.find_overlapping_primers(g.size, [(s, e) for s, e, _ in primers], 0)
    return g, amps, mn, mx, mpl


def engine(G, mn, mx, mpl, share=1):
    e = lib.Engine(int(G))
    e.set_primers(mn, mx, mpl)
    e.set_params(20, 4, True, True)
    e.set_cu_share(share)
    return e


def run(e, b):
    """One pass on a reset engine; the engine's parameters are left alone, so the next pass is planned from this one."""
    e.reset()
    trim = e.process(b)
    return Result(trim, e.counts(), e.events())


def same_with_statuses(a, d):
    """assert_same for a batch in which reads fail (QUAL '*': status 6): the statuses are compared, and the table and the events too."""
    st = a.trim.status
    assert st.any() and np.array_equal(st, d.trim.status), "status differs"
    ok = st == 0
    for f in ("new_pos", "ref_len", "trim_flags", "new_ncig"):
        assert np.array_equal(getattr(a.trim, f)[ok], getattr(d.trim, f)[ok]), f + " differs"
    words = [t.compact_cigars()[np.repeat(ok, t.new_ncig.astype(np.int64))] for t in (a.trim, d.trim)]
    assert np.array_equal(words[0], words[1]), "new CIGARs differ"
    assert np.array_equal(a.counts, d.counts), "count table differs"
    assert np.array_equal(np.sort(a.events, order=EV_ORDER), np.sort(d.events, order=EV_ORDER)), "events differ"


def general_only(simple):
    """The reads of ``simple`` (one match op each), every one changed: soft clips on both sides (three ops), a deletion and an
    insertion (five ops), or QUAL '*' (the oracle's status 6)."""
    segs = simple.segments()
    for i, s in enumerate(segs):
        L = len(s.query_sequence)
        if i % 3 == 0:
            s.cigartuples = [(4, 5), (0, L - 10), (4, 5)]
        elif i % 3 == 1:
            s.cigartuples = [(0, 60), (2, 2), (0, 40), (1, 1), (0, L - 101)]
        else:
            s.query_qualities = None
    return ReadBatch.from_segments(segs)


def _segments(n_list, gen_grid):
    """Segments the general pass cuts a list into (amp_plan.hpp: gen_segments)."""
    tiles = -(-n_list // 64)
    tpb = max(8, -(-(-(-tiles // gen_grid)) // 8) * 8)
    return -(-tiles // tpb)


# 4,096 reads are eight segments at the most (512 reads each): the predicted eight blocks are the whole grid there.  20,000 reads
# are forty, walked by eight blocks.
@pytest.fixture(scope="module", params=[4096, 20000])
def simple_and_general(scheme, request):
    g, amps, mn, mx, mpl = scheme
    simple = synth.make_amplicon_batch(g, amps, request.param, seed=61, indel_frac=0.0)
    assert int(np.diff(simple.cig_off).max()) == 1
    general = general_only(simple)
    return (simple, oracle.process(simple, g.size, mn, mx, mpl, 20, 4)), (general, oracle.process(general, g.size, mn, mx, mpl, 20, 4))


@pytest.mark.parametrize("share", [1, 2])
def test_sequence_of_passes(scheme, simple_and_general, share):
    """Empty list, then a list that fills far more segments than the eight blocks the empty pass predicted, then empty again."""
    g, amps, mn, mx, mpl = scheme
    (simple, want_s), (general, want_g) = simple_and_general
    e = engine(g.size, mn, mx, mpl, share)
    try:
        assert_same(want_s, run(e, simple), simple)
        first = e.debug_last_second_grids()
        assert int(e.debug_counters()[7]) == 0, "the simple batch left reads to the general pass"
        same_with_statuses(want_g, run(e, general))
        assert e.debug_last_second_grids() == (min(8, first[0]), min(8, first[1])), "the pass behind an empty one was not predicted small"
        n_list = int(e.debug_counters()[7])
        # (the fast kernel keeps one of the three shapes to itself)
        segs = _segments(n_list, first[0])
        # (with 4,096 reads the whole grid is eight segments: "more segments than blocks" and "twice its segments" can only be
        #  asked of the 20,000-read batch, and the two asserts below say nothing about the list's size for the small one)
        assert n_list > general.n // 2 and (segs > 2 * 8 or general.n == 4096), "most reads take the general pass, in more segments than blocks"
        assert_same(want_s, run(e, simple), simple)
        assert e.debug_last_second_grids()[0] == min(2 * segs, first[0]) > 8 or general.n == 4096, "the pass behind a long list gets twice its segments"
        assert_same(want_s, run(e, simple), simple)
        assert e.debug_last_second_grids() == (min(8, first[0]), min(8, first[1]))
    finally:
        e.close()


@pytest.fixture(scope="module")
def config5(scheme):
    g, amps, mn, mx, mpl = scheme
    b = synth.make_config5_batch(g, amps, rep=1, pool_reads=20000)
    return b, oracle.process(b, g.size, mn, mx, mpl, 20, 4)


def test_general_pass_is_the_same_on_every_grid(scheme, config5):
    """A config-5-shaped batch (20,000 mixed reads, most of them for the general pass) with the grid forced to 1, 8, 9 and the
    maximum: four runs equal to the oracle, and so to one another."""
    g, amps, mn, mx, mpl = scheme
    b, want = config5
    e = engine(g.size, mn, mx, mpl)
    try:
        for blocks in (1, 8, 9, 1 << 20):
            e.debug_second_grids(blocks, 0)
            d = run(e, b)
            got = e.debug_last_second_grids()[0]
            assert got == blocks if blocks < 100 else got > 9
            assert int(e.debug_counters()[7]) > 5120          # more than ten segments of 512 reads
            assert_same(want, d, b)
    finally:
        e.close()


@pytest.mark.parametrize("where", ["last", "first"])
def test_listed_reads_in_one_fast_block_only(scheme, where):
    """Several blocks of the fast kernel, and only the last (the first) of them hands reads to the general pass: every list
    segment but one is empty."""
    g, amps, mn, mx, mpl = scheme
    simple = synth.make_amplicon_batch(g, amps, 5000, seed=67, indel_frac=0.0)
    segs = simple.segments()
    e = engine(g.size, mn, mx, mpl)
    try:
        rpb = 1024                           # reads per block of a fast kernel at the least (two tiles a wave, eight waves)
        sel = range(len(segs) - 200, len(segs)) if where == "last" else range(0, 200)
        for i in sel:
            L = len(segs[i].query_sequence)
            segs[i].cigartuples = [(0, 60), (2, 2), (0, 40), (1, 1), (0, L - 101)]      # (five ops: no fast kernel keeps it)
        b = ReadBatch.from_segments(segs)
        assert b.n > 4 * rpb
        want = oracle.process(b, g.size, mn, mx, mpl, 20, 4)
        for blocks in (0, 1, 3):
            e.debug_second_grids(blocks, blocks)
            assert_same(want, run(e, b), b)
            assert int(e.debug_counters()[7]) == 200
    finally:
        e.close()


@pytest.mark.parametrize("heavy_blocks", [1, 1 << 20])
def test_deferred_heavy_reads_on_one_block_and_on_all(heavy_blocks):
    """Reads with more CIGAR ops than the tile kernel's column and than the heavy pass's LDS columns (the class of
    test_gpu_parity.test_long_reads_with_many_ops), with the heavy grid forced to one block and to its maximum."""
    G = 60_000
    rng = np.random.default_rng(24)
    primers = sorted((int(s), int(s) + int(rng.integers(18, 31))) for s in rng.integers(0, G - 40, 120))
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    segs = _long_read_segments(rng, 1500, G, 3000, 24)
    # ... among four times as many reads of one op, so that the batch is not one for k_long (eight ops a read on average), which
    # would take the many-op reads before the tile kernel could defer them
    for p in rng.integers(0, G - 200, 6000):
        seq = "".join(rng.choice(list("ACGT"), 100))
        segs.append(Segment(flag=0, reference_start=int(p), cigar=[(0, 100)], template_length=0, query_sequence=seq, query_qualities=[30] * 100))
    segs.sort(key=lambda s: s.reference_start)
    b = ReadBatch.from_segments(segs)
    ok = np.nonzero(oracle.process(b, G, mn, mx, mpl, 20, 4).trim.status == 0)[0]
    good = ReadBatch.from_segments([segs[i] for i in ok])
    want = oracle.process(good, G, mn, mx, mpl, 20, 4)
    assert int(np.diff(good.cig_off).max()) > 17 and int(good.cig_off[-1]) < 8 * good.n
    for variant in (0, 4):
        e = engine(G, mn, mx, mpl)
        try:
            e.set_kernel_variant(variant)
            e.debug_second_grids(0, heavy_blocks)
            assert_same(want, run(e, good), good)
            assert int(e.debug_counters()[0]) > 0, "no read reached the heavy pass"
        finally:
            e.close()


# ---- the calling kernels as one launch ----------------------------------------------------------------------------------
def _table(kind, G):
    if kind != "last_block":
        return U.extreme_case(kind, G)
    ref_seq, base, reads = U.extreme_case("no_record", G)
    first = (G - 1) // 256 * 256                     # the last block of 256 positions: partial unless 256 divides G
    p = np.arange(first, G)
    base[p, (p % 4 + 1) % 4] = 3
    return ref_seq, base, reads


@pytest.mark.parametrize("G", [255, 256, 257, 29903])
@pytest.mark.parametrize("kind", ["no_record", "all_records", "last_block"])
def test_fused_calling_kernel(G, kind):
    c = U.Case(0, G, _table(kind, G))
    pr = U.EXTREME_PARAMS
    cp = U.call_params(pr)
    expect = py_restatement.call_positions(c.ref_seq, c.tables, pr)
    pc, n_rel = hostsim.call_positions(c.counts, c.ins_at, c.ref_seq, cp)
    e = lib.Engine(G)
    try:
        e.add_counts(c.base_counts)
        e.set_reference(c.ref_seq)
        two = [x.copy() for x in e.call_compact(cp)]                 # k_call + k_call_compact
        for _ in range(2):                                           # (the second launch finds the flags as the first left them)
            e.call_compact_begin(cp)
            one = [x.copy() for x in e.call_compact(cp)]             # k_call_fused
            for a, b in zip(two, one):
                assert np.array_equal(a, b)
            check_compact(one[0], one[1], one[2], pc, c, cp, expect)
        want_nv = {"no_record": 0, "all_records": G, "last_block": G - (G - 1) // 256 * 256}[kind]
        assert (one[1].size, one[2].size) == (want_nv, 0) and n_rel == 0
        if want_nv:
            assert int(one[1]["pos"][0]) == G - want_nv and int(one[1]["pos"][-1]) == G - 1
    finally:
        e.close()


def test_fused_calling_kernel_with_insertion_relevant_positions():
    """The relevant-position list (every position relevant, and the seeded table with its mix of records and relevant positions)."""
    for G, parts in ((257, U.extreme_case("all_relevant", 257)), (700, None)):
        c = U.Case(U.SEEDS[700][0] if parts is None else 0, G, parts)
        pr = U.EXTREME_PARAMS
        cp = U.call_params(pr)
        expect = py_restatement.call_positions(c.ref_seq, c.tables, pr)
        pc, n_rel = hostsim.call_positions(c.counts, c.ins_at, c.ref_seq, cp)
        e = lib.Engine(G)
        try:
            e.set_primers(np.full(G, -1, np.int32), np.full(G, -1, np.int32), 0)
            e.set_params(U.MIN_QUALITY, 4, False, True)
            e.add_counts(c.base_counts)
            assert not e.process(c.reads).status.any()
            e.set_reference(c.ref_seq)
            assert np.array_equal(e.counts(), c.counts)
            two = [x.copy() for x in e.call_compact(cp)]
            e.call_compact_begin(cp)
            one = [x.copy() for x in e.call_compact(cp)]
            for a, b in zip(two, one):
                assert np.array_equal(a, b)
            check_compact(one[0], one[1], one[2], pc, c, cp, expect)
            assert one[2].size == n_rel > 0
        finally:
            e.close()
