"""The read-position tallies on the device (amp_readpos.hip: k_readpos) against the plain restatement of
tests/readpos_util.py, applied to the batch and the ORACLE's trim results; in every test the bin sums are held to the same
ctx's count table.  Batch sizes around a tile and past a block's first tile, on one primer and on the example BED, sorted and
shuffled; the crafted reads of the twin (closed-form spans, clips, indels at the ends and the bin edges, the window's and the
slots' edges, irregular CIGARs); a pile across the window's flush period; state across batches, reset, disable, readpos_add and
the device-pointer form; the refusal of a pass without its results; all nine hooks at once.  Last, the command line: aio with
--readpos and --readpos_out through the host codecs and a device-codec route, variants and consensus alone, two ranks."""
import gzip
import io
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, lib, readpos, synth
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from oracle import oracle
from tests import helpers as H
from tests import readpos_util as RP
from tests import strand_util as S
from tests.test_gpu_del import SWITCHES, dev_out, device_batch, write_reads

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 1000, 20011]
MQ, WINDOW = 20, 4
MESSAGE = "the read-position tallies need new_pos, new_ncig, new_cig and status of a trimming pass"


def header_constant(name):
    text = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "amplipy_amd", "csrc", "amp_readpos.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


W, SLOTS, PERIOD = header_constant("RP_W"), header_constant("RP_SLOTS"), header_constant("RP_MAX_TILES_PER_FLUSH")


def example_primers():
    bed = [l.rstrip("\r\n").split("\t") for l in open(H.GOLDEN + "/data/example_primers.bed") if l.strip()]
    return sorted((int(f[1]), int(f[2])) for f in bed)


class PrimerSet:
    """One primer set: its engine (primer tables set, trimming and counting on) and, per batch, what the tables must be: the
    restatement on the oracle's trim results, computed once."""

    def __init__(self, name):
        self.name = name
        self.G, self.primers = {"one": lambda: (2000, [(100, 130)]), "example": lambda: (29903, example_primers())}[name]()
        self.tabs = oracle.find_overlapping_primers(self.G, self.primers, 0)
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(*self.tabs)
        self.batches, self.wants = {}, {}

    def batch(self, n, seed=None):
        key = (n, seed)
        if key not in self.batches:
            self.batches[key] = S.strand_batch(n, self.G, self.primers, 1000 + n if seed is None else seed)
        return self.batches[key]

    def want(self, n, seed=None, mq=MQ, do_trim=True):
        """(counts, hist) of batch (n, seed); the restatement's bin sums are held to the oracle's count table on the way."""
        key = (n, seed, mq, do_trim)
        if key not in self.wants:
            b = self.batch(n, seed)
            r = oracle.process(b, self.G, *self.tabs, mq, WINDOW, do_trim=do_trim, do_count=True)
            assert not r.trim.status.any()
            t = RP.tables(S.walked_segments(b, r.trim if do_trim else None), self.G, mq)
            assert np.array_equal(t[0], r.counts)
            for a in t:
                a.setflags(write=False)
            self.wants[key] = t
        return self.wants[key]

    def fresh(self, mq=MQ, do_trim=True):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(0)
        self.eng.reset()
        self.eng.readpos_enable()
        return self.eng


_SETS = {}


def get_set(name):
    if name not in _SETS:
        _SETS[name] = PrimerSet(name)
    return _SETS[name]


@pytest.fixture(params=["one", "example"])
def pset(request):
    return get_set(request.param)


def assert_tables(eng, want, what=""):
    counts, hist = want
    got = eng.readpos_tables()
    table = eng.counts()
    assert np.array_equal(got.sum(axis=2, dtype=np.uint64), table), what       # the bin sums are this ctx's count table
    assert np.array_equal(table, counts), what
    assert np.array_equal(got, hist), what


# ---- 1. tables against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(pset, n, order):
    batch = pset.batch(n)
    if order == "shuffled" and n > 1:
        batch = synth.gather_rows(batch, np.random.default_rng(5).permutation(batch.n))
        assert n < 63 or (np.diff(batch.pos) < 0).any()
    eng = pset.fresh()
    eng.process(batch)
    want = pset.want(n)
    assert_tables(eng, want, (pset.name, n, order))
    if n >= 1000:           # ends and interiors, deletions off the ends
        hist = want[1]
        assert hist[:, :5, 0].any() and hist[:, :5, 3:].any() and hist[:, 5, 1:].any()
    if n:
        assert eng.readpos_last_ms() > 0


# ---- 2. crafted reads -----------------------------------------------------------------------------------------------------------
_EDGE = {}


def edge_engine(G):
    if G not in _EDGE:
        _EDGE[G] = lib.Engine(G)
    return _EDGE[G]


def run_crafted(segs, G, mq=MQ, variant=0):
    """The reads counted as they are (no trimming) -> the engine; the table must be the restatement's, whose bin sums must be
    the oracle's count table."""
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, G, None, None, 0, mq, WINDOW, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    want = RP.tables(segs, G, mq)
    assert np.array_equal(want[0], r.counts)
    eng = edge_engine(G)
    eng.set_params(mq, WINDOW, False, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    eng.readpos_enable()
    eng.process(batch)
    assert_tables(eng, want)
    eng.set_kernel_variant(0)
    return want


def pile(rng, start, n, length=60):
    return [S.seg(start + int(rng.integers(0, 8)), [(0, length)], rng, 0x10 if k % 2 else 0) for k in range(n)]


@pytest.mark.parametrize("clip", ["none", "left", "right", "both"])
def test_kept_spans_have_the_closed_form(clip):
    """One read per span on positions of its own, all in one batch: the histogram of each is two bases per d < L // 2 and one
    more when L is odd, whatever is clipped around it."""
    rng = np.random.default_rng(17)
    segs, at = [], 10
    for L in RP.SPANS:
        cig = ([(4, 5)] if clip in ("left", "both") else []) + [(0, L)] + ([(4, 7)] if clip in ("right", "both") else [])
        segs.append((at, L, RP.good(at, cig, rng)))
        at += L + 3
    counts, hist = run_crafted([s for _, _, s in segs], at + 10)
    for at, L, _ in segs:
        assert list(hist[at:at + L].sum(axis=(0, 1))) == RP.closed_form(L), L
        assert not hist[at + L:at + L + 3].any()


def test_insertions_and_deletions_at_the_ends_and_the_bin_edges():
    rng = np.random.default_rng(5)
    segs, where, at = [RP.good(5, [(0, 1), (1, 3), (0, 40)], rng)], [], 60
    for left in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65):
        for k, cig in enumerate(([(0, left), (2, 2), (0, 100)], [(0, 100), (3, 2), (0, left)])):
            segs.append(RP.good(at, cig, rng))
            where.append((at + (left if k == 0 else 100), left))
            at += 210
    segs.append(RP.good(at, [(4, 30), (0, 1), (2, 1), (0, 50), (4, 30)], rng))
    counts, hist = run_crafted(segs, at + 100)
    assert hist[6].sum(axis=0)[RP.rp_bin(4)] == 1 and hist[5].sum(axis=0)[0] == 1          # the I's bases count towards the distance
    for p, left in where:
        assert list(hist[p:p + 2, 5, :].sum(axis=0)) == [2 if b == RP.rp_bin(left - 1) else 0 for b in range(RP.BINS)], (p, left)
    assert hist[at + 1, 5, 0] == 1 and int(hist[at:, 5].sum()) == 1                          # soft clips do not count


@pytest.mark.parametrize("span", [W - 1, W, W + 1, 3 * W])
def test_tile_spans_around_the_window(span):
    rng = np.random.default_rng(span)
    segs = pile(rng, 5, 100, 40) + [S.seg(5 + span - 40, [(0, 40)], rng, 0x10), S.seg(5 + span - 41, [(0, 30), (2, 4), (0, 7)], rng, 0)]
    segs.sort(key=lambda g: g.reference_start)
    counts, hist = run_crafted(segs, 4 * W)
    assert counts[5 + span - 1].sum() == 2 and counts[5 + span:].sum() == 0


def test_more_segments_than_slots_soft_clips_and_a_deletion_across_the_edge():
    rng = np.random.default_rng(9)
    edge = 20 + W
    segs = pile(rng, 20, 300, 70)          # two tiles on one pile: the window stays
    segs += [S.seg(22, S.many_segment_cigar(SLOTS // 2), rng, 0x10), S.seg(22, S.many_segment_cigar((SLOTS - 1) // 2), rng, 0), S.seg(23, S.many_segment_cigar(20), rng, 0),
             S.seg(24, [(5, 3), (4, 6), (0, 40), (1, 2), (0, 5), (4, 9), (5, 2)], rng, 0x10), S.seg(25, [(4, 7), (0, 33)], rng, 0, qual=[2] * 7 + [35] * 33),
             S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0x10), S.seg(edge - 21, [(0, 18), (3, 5), (0, 12)], rng, 0)]
    segs.sort(key=lambda g: g.reference_start)
    counts, hist = run_crafted(segs, 4 * W)
    assert counts[edge - 3:edge + 3, 5].sum() == 10 and hist[edge - 3:edge + 3, 5, RP.rp_bin(11)].sum() == 10


def test_the_last_reference_position_and_a_reference_of_one_base():
    rng = np.random.default_rng(4)
    G = 4 * W
    run_crafted([S.seg(G - 40, [(4, 5), (0, 40)], rng, 0), S.seg(G - 3, [(0, 2), (2, 1)], rng, 0x10), S.seg(G - 1, [(0, 1)], rng, 0x10)], G)
    counts, hist = run_crafted([S.seg(0, [(0, 1)], rng, 0x10, qual=37), S.seg(0, [(4, 2), (0, 1)], rng, 0, qual=30)], 1)
    assert int(hist[0, :, 0].sum()) == 2 and int(hist.sum()) == 2


@pytest.mark.parametrize("mq", [0, 100])
def test_min_quality_zero_and_above_every_quality(mq):
    rng = np.random.default_rng(mq + 1)
    segs = pile(rng, 40, 70) + [S.seg(41, [(0, 20), (2, 3), (0, 20)], rng, 0x10), S.seg(42, [(0, 20), (1, 3), (0, 20)], rng, 0x10, qual=0),
                                S.seg(43, [(0, 9), (2, 2), (0, 9)], rng, 0)]
    counts, hist = run_crafted(segs, 3000, mq=mq)
    if mq == 0:
        assert int(counts[:, :5].sum()) == 70 * 60 + 40 + 40 + 18
    else:       # only '-' cells are left
        assert not hist[:, :5].any() and int(hist[:, 5].sum()) == 5 and int(hist[:, 5, RP.rp_bin(19)].sum()) == 3 and int(hist[:, 5, RP.rp_bin(8)].sum()) == 2


def test_irregular_reads_walk_or_add_nothing():
    """QUAL '*', a P op and a soft clip inside the core, each beside a plain neighbour.  A read the oracle counts (status 0) adds
    what the restatement says, and the bin sums are the count table.  A read the oracle gives a status adds nothing to the
    tallies; the count table of such a batch is unspecified (the reference raises part-way through the read), so there only the
    tallies are compared."""
    rng = np.random.default_rng(8)
    G = 600
    plain = RP.good(52, [(0, 30)], rng)
    odd = [Segment(flag=0, reference_start=40, cigar=[(0, 30)], query_sequence="ACGT" * 7 + "AC", query_qualities=None),
           RP.good(50, [(0, 20), (6, 2), (0, 20)], rng), RP.good(50, [(0, 20), (4, 3), (0, 20)], rng)]
    n_counted = n_status = 0
    for seg in odd:
        batch = ReadBatch.from_segments([seg, plain])
        r = oracle.process(batch, G, None, None, 0, MQ, WINDOW, do_trim=False, do_count=True)
        assert int(r.trim.status[1]) == 0
        counted = int(r.trim.status[0]) == 0
        want = RP.tables([seg, plain] if counted else [plain], G, MQ)
        eng = edge_engine(G)
        eng.set_params(MQ, WINDOW, False, True)
        eng.reset()
        eng.readpos_enable()
        res = eng.process(batch)
        assert res.status.tolist() == r.trim.status.tolist()
        if counted:
            assert np.array_equal(want[0], r.counts)
            assert_tables(eng, want)
            n_counted += 1
        else:
            assert np.array_equal(eng.readpos_tables(), want[1])
            n_status += 1
    assert n_counted >= 1 and n_status >= 1


def test_a_pile_across_the_flush_period():
    """4-base reads on one position for two tiles more than the flush period (255 tiles: below 1,024, so the pile is cheap)."""
    assert PERIOD < 1024
    n = (PERIOD + 2) * 256
    one = RP.good(77, [(0, 4)], np.random.default_rng(1))
    batch = synth.gather_rows(ReadBatch.from_segments([one]), np.zeros(n, np.int64))
    hist1 = RP.tables([one], 300, MQ)[1]
    want = (hist1.astype(np.uint64) * np.uint64(n)).astype(np.uint32)
    assert int(want.sum()) == 4 * n and int(want.max()) == n > 2 ** 16
    eng = edge_engine(300)
    eng.set_params(MQ, WINDOW, False, True)
    eng.reset()
    eng.readpos_enable()
    eng.process(batch)
    assert_tables(eng, (want.sum(axis=2, dtype=np.uint64).astype(np.uint32), want))


def test_without_trimming_the_read_is_walked_as_it_came_in():
    s = get_set("example")
    eng = s.fresh(do_trim=False)
    eng.process(s.batch(1000))
    want = s.want(1000, do_trim=False)
    assert_tables(eng, want)
    assert not np.array_equal(want[1], s.want(1000)[1])         # (trimming changes what is counted, and where the ends are)


@pytest.mark.parametrize("variant", [0, 2, 5, 7])
def test_every_read_kernel_feeds_the_same_tables(variant):
    s = get_set("example")
    eng = s.fresh()
    eng.set_kernel_variant(variant)
    eng.process(s.batch(1000))
    assert_tables(eng, s.want(1000), variant)
    eng.set_kernel_variant(0)


# ---- 3. state -----------------------------------------------------------------------------------------------------------------
def test_tables_accumulate_reset_stop_when_disabled_and_take_readpos_add():
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    eng.process(s.batch(1000))
    both = tuple(x.astype(np.uint64) + y for x, y in zip(s.want(257), s.want(1000)))
    assert_tables(eng, both)
    eng.reset()
    assert not eng.readpos_tables().any()
    eng.process(s.batch(257))
    assert_tables(eng, s.want(257))
    eng.readpos_disable()
    eng.process(s.batch(1000))
    assert np.array_equal(eng.readpos_tables(), s.want(257)[1])          # what was tallied stays readable, nothing was added
    assert np.array_equal(eng.counts(), both[0])
    eng.readpos_add(s.want(1000)[1])                                     # another rank's table
    assert_tables(eng, both)
    eng.readpos_enable()                                                 # on again: the table starts at zero
    assert not eng.readpos_tables().any()


def test_process_device_gives_the_same_tables():
    s = get_set("example")
    eng = s.fresh()
    b, out = device_batch(s.batch(1000))
    eng.process_device(b.struct(), 0, dev_out(out))
    eng.sync()
    assert_tables(eng, s.want(1000))
    eng.reset()                                # the tallies need neither ref_len nor trim_flags
    eng.process_device(b.struct(), 0, dev_out(out, drop=("ref_len", "trim_flags")))
    eng.sync()
    assert_tables(eng, s.want(1000))


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.readpos_disable()
    off = eng.process(batch)
    table_off = eng.counts()
    events_off = np.sort(eng.events(), order=["ref_pos", "read", "q_from", "q_to"])
    eng = s.fresh()
    on = eng.process(batch)
    for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status"):
        assert getattr(on, k).tobytes() == getattr(off, k).tobytes(), k
    assert eng.counts().tobytes() == table_off.tobytes()
    assert np.array_equal(np.sort(eng.events(), order=["ref_pos", "read", "q_from", "q_to"]), events_off)
    assert events_off.size > 0
    assert_tables(eng, s.want(20011))


def test_tables_before_the_first_enable_and_last_ms_after_an_empty_batch_are_errors():
    e = lib.Engine(500)
    with pytest.raises(lib.AmpliHipError) as err:
        e.readpos_tables()
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError) as err:
        e.readpos_last_ms()
    assert err.value.rc == -5
    e.readpos_disable()          # off while off: nothing to do
    e.set_params(MQ, WINDOW, False, True)
    e.readpos_enable()
    with pytest.raises(lib.AmpliHipError) as err:          # on, and no batch yet
        e.readpos_last_ms()
    assert err.value.rc == -5
    b, out = device_batch(ReadBatch.from_segments([RP.good(10, [(0, 20)], np.random.default_rng(2))]))
    e.process_device(b.struct(), 0, dev_out(out))
    e.sync()
    assert e.readpos_last_ms() > 0 and int(e.readpos_tables().sum()) == 20
    empty = b.struct()
    empty.n_reads = 0                                       # a device batch without reads launches nothing: nothing to ask for
    e.process_device(empty, 0, dev_out(out))
    e.sync()
    with pytest.raises(lib.AmpliHipError) as err:
        e.readpos_last_ms()
    assert err.value.rc == -5 and int(e.readpos_tables().sum()) == 20
    e.close()


def test_all_nine_hooks_at_once_leave_the_others_alone():
    """On the example primer set, which has amplicons: every other hook's tables are the same bytes with the read-position
    tallies on and off, and the read-position table is the restatement's."""
    from amplipy_amd import codon, errprof
    from tests import amplicon_util as A
    from tests import codon_util as CU
    from tests import cooc_util as CO
    from tests import hap_util as U
    amps, rows = A.example_amps(), A.example_rows()
    primers = sorted((s, e) for s, e, _ in rows)
    ref = U.reference(amps.G, seed=3)
    regions = U.regions_near(primers[:40], amps.G)
    tabs = oracle.find_overlapping_primers(amps.G, primers, 0)
    b = U.onto_reference(S.strand_batch(1025, amps.G, primers, 2025), ref, 5, rate=0.01, low_rate=0.02)
    cds = CU.overlapping(amps.G)
    sets = CO.mixed_sets(amps.G)
    eng = lib.Engine(amps.G)
    eng.set_primers(*tabs)
    eng.set_params(MQ, WINDOW, True, True)
    snaps = []
    for with_readpos in (False, True):
        eng.reset()
        eng.qc_enable(primers, 0, 60); eng.strand_enable(); amps.enable(eng); codon.enable(eng, cds); eng.del_enable(); eng.cooc_enable(*sets.arrays())
        errprof.enable(eng, ref, None)
        eng.hap_enable([s for s, _ in regions], [e for _, e in regions], ref, 0)
        if with_readpos:
            eng.readpos_enable()
        res = eng.process(b)
        t, ps, pe = eng.qc_read_tallies()
        h_ev, _, h_tally, h_reads = eng.hap_tables()
        snaps.append([np.array([t[k] for k in abi.QC_READ_FIELDS], np.uint64), ps, pe, *eng.strand_tables(), *eng.amplicon_tables(), *eng.codon_tables(),
                      eng.del_events()[0], *eng.cooc_tables(), *eng.errprof_tables(), h_ev, h_tally, h_reads, eng.counts(), res.status, res.new_pos,
                      res.new_ncig, res.new_cig])
    assert len(snaps[0]) == len(snaps[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(snaps[0], snaps[1]))
    assert all(np.frombuffer(snaps[0][k].tobytes(), np.uint8).any() for k in (0, 3, 5, 7, 9, 10, 12))
    r = oracle.process(b, amps.G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    want = RP.tables(S.walked_segments(b, r.trim), amps.G, MQ)
    assert np.array_equal(want[0], r.counts)
    assert_tables(eng, want)
    for h in ("qc", "strand", "amplicon", "codon", "del", "cooc", "errprof", "hap", "readpos"):
        assert getattr(eng, h + "_last_ms")() > 0
    eng.close()


# ---- 4. the refusal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [None, "new_pos", "new_ncig", "new_cig", "status"])
def test_a_trimming_pass_without_its_results_is_refused_before_it_runs(drop):
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before = eng.counts()
    b, out = device_batch(s.batch(1000))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, None if drop is None else dev_out(out, drop=(drop,)))
    assert e.value.rc == -1 and MESSAGE in str(e.value)
    eng.sync()
    assert np.array_equal(eng.counts(), before)
    assert_tables(eng, s.want(257))
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.readpos_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the tallies existed
    eng.sync()
    eng.set_params(MQ, WINDOW, False, True)                        # without trimming nothing of dev_out is needed
    eng.reset()
    eng.readpos_enable()
    eng.process_device(b.struct(), 0, None)
    eng.sync()
    assert_tables(eng, s.want(1000, do_trim=False))


# ---- 5. command line -----------------------------------------------------------------------------------------------------------
CLI_MIN_LENGTH = 30
N_CLI = 3000
ROUTES = [("host", "bam", "bam", {}), ("sam", "sam", "sam", {"AMPLIPY_GPU_SAM": 1})]          # (name, input, trimmed output, switches)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """The files of the job and the tables the outputs must show: the restatement on the oracle's trim results (aio) and on
    the reads as they are (variants)."""
    d = tmp_path_factory.mktemp("readpos_cli")
    g = synth.make_genome()
    G = int(g.size)
    primers, amps = synth.make_artic_scheme()
    pr = sorted((s, e) for s, e, _ in primers)
    batch = S.strand_batch(N_CLI, G, pr, 31)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(g) + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), primers)
    files = dict(ref=str(ref), bed=str(bed), bam=write_reads(str(d / "in.bam"), "wb", batch, G), sam=write_reads(str(d / "in.sam"), "w", batch, G))
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    want = {}
    for do_trim in (True, False):
        r = oracle.process(batch, G, *tabs, MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        t = RP.tables(S.walked_segments(batch, r.trim if do_trim else None), G, MQ)
        assert np.array_equal(t[0], r.counts)
        want[do_trim] = t
    return files, want, G


def run(monkeypatch, argv, **env):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    amplipy.main(argv)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check_vcf(with_keys, plain, tables):
    """Every record's last six keys are the tables' word; with the keys and their header lines stripped the file is ``plain``."""
    text = with_keys.decode()
    assert readpos.HEADER_LINES in text
    out = []
    n_records = n_z = 0
    for line in text.replace(readpos.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-6:]] == list(readpos.KEYS) and kvs[-7].startswith("ALT_FREQ=")
            assert ";".join(kvs[-6:]) == tables.info(int(f[1]) - 1, f[3], f[4].split(",")), line
            n_z += kvs[-1] != "RPZ=."
            f[7] = ";".join(kvs[:-6])
            line = "\t".join(f)
            n_records += 1
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    assert n_records > 12 and n_z > 0
    return n_records


def tsv_text(ref_id, tables):
    f = io.StringIO()
    readpos.write_tsv(f, ref_id, tables)
    return f.getvalue()


_TSV = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_aio_with_readpos_flags(tmp_path, job, monkeypatch, route):
    files, want, G = job
    name, inp, out, env = route
    got = {}
    for tag in ("plain", "rp"):
        base = ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + "." + out)),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        run(monkeypatch, base + (["--readpos", "--readpos_end", "16", "--readpos_out", str(tmp_path / "r.tsv")] if tag == "rp" else []), **env)
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in ("." + out, ".vcf", ".fas")]
    assert got["rp"][0] == got["plain"][0] and got["rp"][2] == got["plain"][2] and len(got["plain"][0]) > 100000
    assert b"REF_RP" not in got["plain"][1]
    tables = readpos.Tables(*want[True], end=16)
    check_vcf(got["rp"][1], got["plain"][1], tables)
    text = read(str(tmp_path / "r.tsv")).decode()
    assert text == tsv_text("SYN_REF", tables)
    _TSV[name] = text
    assert all(t == text for t in _TSV.values())          # the same file on every route run so far
    # an existing --readpos_out is refused like every other output, before a read is looked at
    with pytest.raises(SystemExit):
        run(monkeypatch, ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / ("x." + out)),
                          "-ov", str(tmp_path / "x.vcf"), "-oc", str(tmp_path / "x.fas"), "--readpos_out", str(tmp_path / "r.tsv")], **env)
    assert read(str(tmp_path / "r.tsv")).decode() == text


def test_variants_and_consensus_alone(tmp_path, job, monkeypatch):
    files, want, G = job
    tables = readpos.Tables(*want[False])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "v.vcf"), "--readpos", "--readpos_out", str(tmp_path / "v.tsv.gz")])
    check_vcf(read(str(tmp_path / "v.vcf")), read(str(tmp_path / "plain.vcf")), tables)
    assert gzip.open(str(tmp_path / "v.tsv.gz"), "rt").read() == tsv_text("SYN_REF", tables)
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "c.fas"), "--readpos_out", str(tmp_path / "c.tsv")])
    assert read(str(tmp_path / "c.fas")) == read(str(tmp_path / "plain.fas"))
    assert read(str(tmp_path / "c.tsv")).decode() == tsv_text("SYN_REF", tables)
    for argv in (["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "e.fas"), "--readpos"],
                 ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "e.bam"), "--readpos_out", str(tmp_path / "e.tsv")]):
        with pytest.raises(SystemExit):
            run(monkeypatch, argv)


def test_two_ranks_give_the_one_process_files(tmp_path, job, monkeypatch):
    """Two ranks on one card (tests/rank_worker.py: a child process per rank, a time limit per child): --readpos_out and the VCF
    equal the one-process run byte for byte."""
    from tests.test_gpu_ranks import run_ranks
    files, want, G = job
    argv = lambda tag: ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", tag + ".bam", "-ov", tag + ".vcf", "-oc", tag + ".fas",
                        "-ml", str(CLI_MIN_LENGTH), "--readpos", "--readpos_out", tag + ".tsv"]
    monkeypatch.chdir(tmp_path)
    run(monkeypatch, argv("one"))
    status, logs = run_ranks(2, tmp_path, argv("two"), part_bytes=os.path.getsize(files["bam"]) // 4 + 1)
    assert status == [0, 0], logs
    shares = [int(x) for x in re.search(r"records \[(\d+), (\d+)\]", logs[0]).groups()]
    assert sum(shares) == N_CLI and min(shares) > 0
    for ext in (".vcf", ".tsv", ".fas"):
        assert read(str(tmp_path / ("two" + ext))) == read(str(tmp_path / ("one" + ext))), ext
    assert read(str(tmp_path / "one.tsv")).decode() == tsv_text("SYN_REF", readpos.Tables(*want[True]))
