"""The per-amplicon allele counts on the device (amp_amplicon.hip: k_amplicon) against the plain
restatement of tests/amplicon_util.py applied to the batch and the DEVICE's own trim results; the count table must equal the
oracle's.  Batch sizes around a wave, a tile and past a block's first tile, on one amplicon, two overlapping ones and the
example BED, sorted and shuffled; piles of 20,000 reads on one, two and AM_SLOTS + 1 amplicons; crafted edges of the spans, the
windows and the segment list; every read kernel; state across batches, reset, disable, amplicon_add and the device-pointer form;
the refusal of a pass without its results; the exact invariants, the oracle's per-amplicon sub-batches among them.  Last, the
command line: aio with --amplicons and --amplicon_out, with --strand and --qc, through the host codecs and a device-codec route,
and one rank through RCCL -- the keys equal the restatement, and with them stripped every output is byte for byte what the same
command writes without the flags."""
import gzip
import json
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplicon, amplipy, lib, strand, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import amplicon_util as A
from tests import strand_util as S

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
MQ, WINDOW = 20, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "amplipy_amd", "csrc", "amp_amplicon.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


W, SLOTS, SEG_SLOTS = header_constant("AM_W"), header_constant("AM_SLOTS"), header_constant("AM_SEG_SLOTS")


class AmpSet:
    """One amplicon set: its engine (primer tables set) and, per batch, the oracle's results, computed once."""

    def __init__(self, name):
        self.name = name
        if name == "example":
            self.amps, self.rows = A.example_amps(), A.example_rows()
        else:
            pairs = [((100, 130), (400, 430))] + ([((330, 360), (640, 670))] if name == "two" else [])
            self.amps, self.rows = A.simple_amps(2000, pairs)
        self.G = self.amps.G
        self.primers = sorted((s, e) for s, e, _ in self.rows)
        self.tabs = oracle.find_overlapping_primers(self.G, self.primers, 0)
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(*self.tabs)
        self.batches, self.oracles = {}, {}

    def batch(self, n, seed=None):
        key = (n, seed)
        if key not in self.batches:
            self.batches[key] = S.strand_batch(n, self.G, self.primers, 1000 + n if seed is None else seed)
        return self.batches[key]

    def oracle(self, n, seed=None, mq=MQ, do_trim=True):
        key = (n, seed, mq, do_trim)
        if key not in self.oracles:
            r = oracle.process(self.batch(n, seed), self.G, *self.tabs, mq, WINDOW, do_trim=do_trim, do_count=True)
            assert not r.trim.status.any()
            r.counts.setflags(write=False)
            self.oracles[key] = r
        return self.oracles[key]

    def fresh(self, mq=MQ, do_trim=True, variant=0):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(variant)
        self.eng.reset()
        self.amps.enable(self.eng)
        return self.eng


_SETS = {}


def get_set(name):
    if name not in _SETS:
        _SETS[name] = AmpSet(name)
    return _SETS[name]


@pytest.fixture(params=["one", "two", "example"])
def aset(request):
    return get_set(request.param)


def run_and_check(eng, batch, amps, oracle_counts, mq=MQ, do_trim=True, what=""):
    """One batch through the engine: the count table is the oracle's, the tables are the restatement's on the device's own trim
    results, and the invariants hold.  -> (amp_counts, amp_reads, assignment)."""
    res = eng.process(batch)
    assert np.array_equal(eng.counts(), oracle_counts), what
    want_c, want_r, asg = A.tables(batch, res, amps, mq, do_trim)
    got_c, got_r = eng.amplicon_tables()
    assert np.array_equal(got_r, want_r), what
    assert np.array_equal(got_c, want_c), what
    A.check_invariants(got_c, got_r, asg, oracle_counts, amps)
    return got_c, got_r, asg


# ---- 1. tables against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(aset, n, order):
    batch = aset.batch(n)
    if order == "shuffled" and n > 1:
        batch = synth.gather_rows(batch, np.random.default_rng(5).permutation(batch.n))
        assert n < 63 or (np.diff(batch.pos) < 0).any()
    eng = aset.fresh()
    counts, reads, asg = run_and_check(eng, batch, aset.amps, aset.oracle(n).counts, what=(aset.name, n, order))
    if n >= 257:            # neither branch of the assignment is vacuous
        assert int((asg >= 0).sum()) >= n // 3 and int((asg == -1).sum()) >= n // 10
    if n:
        assert eng.amplicon_last_ms() > 0


def test_sub_batches_of_the_oracle():
    """For the amplicons with the most reads (and the first and the last one): the oracle's count table of their reads alone."""
    s = get_set("example")
    batch = s.batch(3001, seed=41)
    eng = s.fresh()
    counts, reads, asg = run_and_check(eng, batch, s.amps, s.oracle(3001, seed=41).counts)
    top = [int(a) for a in np.argsort(-np.bincount(asg[asg >= 0], minlength=s.amps.n), kind="stable")[:12]]
    seen = A.oracle_sub_batches(oracle.process, batch, asg, s.amps, s.tabs, counts, MQ, WINDOW, True, only=top + [0, s.amps.n - 1])
    assert len(seen) >= 12


# ---- 2. piles -----------------------------------------------------------------------------------------------------------------
def pile_set():
    """Six amplicons of 250..400 bases on a reference of 4,000, tiled so that neighbours overlap."""
    pairs = [((100 + 300 * k, 125 + 300 * k), (100 + 300 * k + 225 + 30 * k, 100 + 300 * k + 250 + 30 * k)) for k in range(6)]
    return A.simple_amps(4000, pairs)


_PILE = {}


def pile_engine():
    if not _PILE:
        amps, rows = pile_set()
        tabs = oracle.find_overlapping_primers(amps.G, sorted((s, e) for s, e, _ in rows), 0)
        eng = lib.Engine(amps.G)
        eng.set_primers(*tabs)
        _PILE.update(amps=amps, tabs=tabs, eng=eng)
    return _PILE["amps"], _PILE["tabs"], _PILE["eng"]


@pytest.mark.parametrize("order", ["interleaved", "sorted"])
@pytest.mark.parametrize("which", [[0], [1, 2], "slots+1"], ids=["one", "two", "one_more_than_slots"])
def test_piles_of_20000_reads(which, order):
    amps, tabs, eng = pile_engine()
    if which == "slots+1":
        which = list(range(SLOTS + 1))
    segs = A.pile(amps, which, 20000, 7)
    if order == "sorted":
        segs.sort(key=lambda g: g.reference_start)
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, amps.G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    eng.set_params(MQ, WINDOW, True, True)
    eng.set_kernel_variant(0)
    eng.reset()
    amps.enable(eng)
    counts, reads, asg = run_and_check(eng, batch, amps, r.counts, what=(which, order))
    assert int((asg == -1).sum()) > 1000 and all(int((asg == a).sum()) > 2000 for a in which)
    if order == "sorted":
        A.oracle_sub_batches(oracle.process, batch, asg, amps, tabs, counts, MQ, WINDOW, True, only=which[:2])


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------
_EDGE = {}


def run_crafted(segs, amps, mq=MQ, variant=0):
    """The reads counted as they are (no trimming) -> the engine."""
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, amps.G, None, None, 0, mq, WINDOW, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    if amps.G not in _EDGE:
        _EDGE[amps.G] = lib.Engine(amps.G)
    eng = _EDGE[amps.G]
    eng.set_params(mq, WINDOW, False, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    amps.enable(eng)
    out = run_and_check(eng, batch, amps, r.counts, mq=mq, do_trim=False)
    eng.set_kernel_variant(0)
    return out


def test_a_read_filling_its_span_and_one_base_over():
    rng = np.random.default_rng(3)
    amps, rows = A.simple_amps(2000, [((100, 130), (400, 430)), ((330, 360), (640, 670))])
    segs = [S.seg(100, [(0, 330)], rng), S.seg(99, [(0, 331)], rng), S.seg(100, [(0, 331)], rng), S.seg(330, [(0, 340)], rng, 0x10), S.seg(330, [(0, 341)], rng)]
    counts, reads, asg = run_crafted(segs, amps)
    assert list(asg) == [0, -1, -1, 1, -1] and list(reads) == [1, 1, 3]


@pytest.mark.parametrize("span", [W - 1, W, W + 1, 3 * W])
def test_spans_around_the_window(span):
    """A pile at either end of the span; with 3 W the forward reads come first, then the reverse ones, over several tiles: the
    anchor moves inside one amplicon."""
    rng = np.random.default_rng(span)
    amps, rows = A.simple_amps(4 * W, [((10, 30), (10 + span - 20, 10 + span))])
    segs = [S.seg(10 + k % 20, [(0, 40)], rng) for k in range(600)] + [S.seg(10, [(0, 20), (2, 5), (0, 30)], rng)]
    segs += [S.seg(10 + span - 40 - k % 20, [(0, 40)], rng, 0x10) for k in range(600)]
    counts, reads, asg = run_crafted(segs, amps)
    assert (asg == 0).all() and counts[0].sum() == 31 and counts[span - 1].sum() == 30


def test_deletion_across_a_window_edge_more_segments_than_slots_and_41_ops():
    rng = np.random.default_rng(9)
    amps, rows = A.simple_amps(4 * W, [((10, 30), (10 + 2 * W - 20, 10 + 2 * W))])
    edge = 10 + W
    segs = [S.seg(10 + k % 8, [(0, 70)], rng, 0x10 if k % 2 else 0) for k in range(300)]
    segs += [S.seg(12, [(0, W - 4), (2, 5), (0, 12)], rng), S.seg(12, S.many_segment_cigar(SEG_SLOTS), rng),
             S.seg(12, S.many_segment_cigar((SEG_SLOTS - 1) // 2), rng), S.seg(13, S.many_segment_cigar(20), rng),
             S.seg(24, [(5, 3), (4, 6), (0, 40), (1, 2), (0, 5), (4, 9), (5, 2)], rng, 0x10), S.seg(25, [(4, 7), (0, 33)], rng, 0, qual=[2] * 7 + [35] * 33)]
    segs.sort(key=lambda g: g.reference_start)
    counts, reads, asg = run_crafted(segs, amps)
    assert (asg == 0).all() and list(counts[edge - 2 - 10:edge + 3 - 10, 5]) == [1] * 5


def test_nested_and_identical_spans_an_amplicon_ending_at_G_and_a_reference_of_one_base():
    rng = np.random.default_rng(11)
    amps, rows = A.simple_amps(900, [((100, 120), (500, 520)), ((200, 220), (400, 420)), ((100, 120), (500, 520)), ((700, 720), (880, 900))])
    segs = [S.seg(100, [(0, 100)], rng), S.seg(200, [(0, 100)], rng), S.seg(320, [(0, 100)], rng, 0x10), S.seg(420, [(0, 100)], rng, 0x10),
            S.seg(800, [(0, 100)], rng, 0x10), S.seg(699, [(0, 50)], rng), S.seg(700, [(0, 50)], rng), S.seg(300, [(0, 50)], rng)]
    counts, reads, asg = run_crafted(segs, amps)
    assert list(asg) == [0, 1, 1, 0, 3, -1, 3, -1] and list(reads) == [2, 2, 0, 2, 2]
    amps = A.Amps([("l", "r", "only")], [(0, 1, "l"), (0, 1, "r")], 0, 1)
    counts, reads, asg = run_crafted([S.seg(0, [(0, 1)], rng, qual=37), S.seg(0, [(4, 2), (0, 1)], rng, qual=30)], amps)
    assert int(counts.sum()) == 2 and list(reads) == [2, 0]


@pytest.mark.parametrize("mq", [0, 100])
def test_min_quality_zero_and_above_every_quality(mq):
    rng = np.random.default_rng(mq + 1)
    amps, rows = A.simple_amps(2000, [((100, 130), (400, 430))])
    segs = [S.seg(100 + k % 8, [(0, 60)], rng) for k in range(70)] + [S.seg(110, [(0, 20), (2, 3), (0, 20)], rng, 0x10), S.seg(115, [(0, 20), (1, 3), (0, 20)], rng, qual=0)]
    counts, reads, asg = run_crafted(segs, amps, mq=mq)
    if mq == 0:
        assert int(counts[:, :5].sum()) == 70 * 60 + 40 + 40
    else:       # only '-' cells are left
        assert not counts[:, :5].any() and int(counts[:, 5].sum()) == 3


def test_without_trimming_the_read_is_walked_as_it_came_in():
    s = get_set("example")
    eng = s.fresh(do_trim=False)
    off = run_and_check(eng, s.batch(1025), s.amps, s.oracle(1025, do_trim=False).counts, do_trim=False)[0]
    eng = s.fresh()
    on = run_and_check(eng, s.batch(1025), s.amps, s.oracle(1025).counts)[0]
    assert not np.array_equal(on, off)                          # (trimming changes what is counted, not who it is counted for)


@pytest.mark.parametrize("variant", [0, 2, 5, 7])
def test_every_read_kernel_feeds_the_same_tables(variant):
    s = get_set("example")
    eng = s.fresh(variant=variant)
    run_and_check(eng, s.batch(1025), s.amps, s.oracle(1025).counts, what=variant)
    eng.set_kernel_variant(0)


# ---- 4. state -----------------------------------------------------------------------------------------------------------------
def test_tables_accumulate_reset_stop_when_disabled_and_take_amplicon_add():
    s = get_set("example")
    eng = s.fresh()
    res_a = eng.process(s.batch(257))
    res_b = eng.process(s.batch(1025))
    ta = A.tables(s.batch(257), res_a, s.amps, MQ, True)
    tb = A.tables(s.batch(1025), res_b, s.amps, MQ, True)
    counts, reads = eng.amplicon_tables()
    assert np.array_equal(counts, ta[0] + tb[0]) and np.array_equal(reads, ta[1] + tb[1])
    eng.reset()
    counts, reads = eng.amplicon_tables()
    assert not counts.any() and not reads.any()
    eng.process(s.batch(257))
    eng.amplicon_disable()
    eng.process(s.batch(1025))
    counts, reads = eng.amplicon_tables()                       # what was tallied stays readable, nothing was added
    assert np.array_equal(counts, ta[0]) and np.array_equal(reads, ta[1])
    big = np.zeros(s.amps.n + 1, np.uint64); big[3] = 2 ** 40 + 5
    eng.amplicon_add(tb[0], tb[1] + big)                        # another rank's tables, a read count beyond 32 bits
    counts, reads = eng.amplicon_tables()
    assert np.array_equal(counts, ta[0] + tb[0]) and np.array_equal(reads, ta[1] + tb[1] + big)
    s.amps.enable(eng)                                          # on again: the tables start at zero
    counts, reads = eng.amplicon_tables()
    assert not counts.any() and not reads.any()
    # a set of another size on an engine that had one: the tables are laid out again
    two, one = get_set("two"), get_set("one")
    eng2 = two.fresh()
    one.amps.enable(eng2)
    res = eng2.process(two.batch(257))
    want = A.tables(two.batch(257), res, one.amps, MQ, True)
    counts, reads = eng2.amplicon_tables()
    assert counts.shape[0] == one.amps.cells and np.array_equal(counts, want[0]) and np.array_equal(reads, want[1])


def _device_batch(batch):
    import torch
    from amplipy_amd import synth_torch
    n = batch.n
    b = synth_torch.DeviceBatch.from_host(batch, "cuda:0")
    out = {k: torch.zeros(max(sz, 1), dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", b.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    return b, out


def _dev_out(out, drop=()):
    return abi.AmpTrimOut(*[None if k in drop else out[k].data_ptr() for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")])


def test_process_device_gives_the_same_tables():
    s = get_set("example")
    eng = s.fresh()
    res = eng.process(s.batch(1025))
    want = eng.amplicon_tables()
    assert np.array_equal(want[0], A.tables(s.batch(1025), res, s.amps, MQ, True)[0])
    b, out = _device_batch(s.batch(1025))
    for drop in ((), ("ref_len", "trim_flags")):                # the hook needs neither ref_len nor trim_flags
        eng.reset()
        eng.process_device(b.struct(), 0, _dev_out(out, drop=drop))
        eng.sync()
        got = eng.amplicon_tables()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.amplicon_disable()
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


def test_tables_before_the_first_enable_and_bad_sets_are_errors():
    e = lib.Engine(500)
    with pytest.raises(lib.AmpliHipError) as err:
        e.amplicon_tables()
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError):
        e.amplicon_last_ms()
    e.amplicon_disable()        # off while off: nothing to do
    none = np.full(500, -1, np.int32)
    for lo, hi, st in (([10], [10], none), ([-1], [10], none), ([10], [501], none), ([10], [20], np.where(np.arange(500) == 7, 1, -1))):
        with pytest.raises(lib.AmpliHipError) as err:
            e.amplicon_enable(lo, hi, st, none)
        assert err.value.rc == -1
    e.close()
    big = lib.Engine(3 * 2 ** 21)           # two spans of 1.5 * 2^21 positions: more than 2^22 together
    none = np.full(big.ref_len, -1, np.int32)
    with pytest.raises(lib.AmpliHipError) as err:
        big.amplicon_enable([0, 0], [big.ref_len // 2, big.ref_len // 2 + 1], none, none)
    assert err.value.rc == -1
    big.close()


# ---- 5. the refusal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [None, "new_pos", "new_ncig", "new_cig", "status"])
def test_a_trimming_pass_without_its_results_is_refused_before_it_runs(drop):
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before, tables_before = eng.counts(), eng.amplicon_tables()
    b, out = _device_batch(s.batch(1025))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, None if drop is None else _dev_out(out, drop=(drop,)))
    assert e.value.rc == -1
    eng.sync()
    after = eng.amplicon_tables()
    assert np.array_equal(eng.counts(), before) and np.array_equal(after[0], tables_before[0]) and np.array_equal(after[1], tables_before[1])
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.amplicon_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the hook existed
    eng.sync()
    eng.set_params(MQ, WINDOW, False, True)                        # without trimming nothing of dev_out is needed
    eng.reset()
    s.amps.enable(eng)
    eng.process_device(b.struct(), 0, None)
    eng.sync()
    want = A.tables(s.batch(1025), None, s.amps, MQ, False)
    got = eng.amplicon_tables()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 6. command line ----------------------------------------------------------------------------------------------------------
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST")
CLI_MIN_LENGTH = 30
ROUTES = [("host", "bam", "bam", False), ("sam", "sam", "sam", True)]          # (name, input, trimmed output, gpu_sam)


def write_reads(path, mode, hb, G):
    from amplipy_amd import bamio
    from amplipy_amd.batch import SEQ_NT16, unpack_nibbles
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % G, [("SYN_REF", G)])
    w = bamio.AlignmentWriter(path, mode, hdr)
    lut = np.frombuffer(SEQ_NT16.encode(), np.uint8)
    for i in range(hb.n):
        o = int(hb.seq_off[i]); L = int(hb.lseq[i])
        seq = lut[unpack_nibbles(hb.seq[o // 2:(o + L + 1) // 2], L)].tobytes().decode()
        a, c = int(hb.cig_off[i]), int(hb.cig_off[i + 1])
        w.write(bamio.Rec("r%d" % i, int(hb.flag[i]), 0, int(hb.pos[i]), 60, [(int(v) & 15, int(v) >> 4) for v in hb.cig[a:c]], 0,
                          int(hb.pos[i]), int(hb.tlen[i]), seq, bytes(hb.qual[o:o + L])))
    w.close()
    return path


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """The files of the job and what the outputs must show: the restatement on the oracle's trim results."""
    d = tmp_path_factory.mktemp("amplicon_cli")
    g = synth.make_genome()
    G = int(g.size)
    primers, _ = synth.make_artic_scheme()
    rows = sorted(primers, key=lambda r: (r[0], r[1]))
    pr = sorted((s, e) for s, e, _ in primers)
    batch = S.strand_batch(3000, G, pr, 31)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(g) + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), primers)
    n_amp = len(primers) // 2
    pairs = [("SYN_%d_LEFT" % k, "SYN_%d_RIGHT" % k, "SYN_%d" % k) for k in range(1, n_amp + 1)]
    tsv = d / "amplicons.tsv"; tsv.write_text("".join("%s\t%s\t%s\n" % p for p in pairs))
    files = dict(ref=str(ref), bed=str(bed), amplicons=str(tsv), bam=write_reads(str(d / "in.bam"), "wb", batch, G),
                 sam=write_reads(str(d / "in.sam"), "w", batch, G))
    amps = A.Amps(pairs, rows, 0, G)
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    r = oracle.process(batch, G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    amp_counts, amp_reads, asg = A.tables(batch, r.trim, amps, MQ, True)
    A.check_invariants(amp_counts, amp_reads, asg, r.counts, amps)
    assert int((asg >= 0).sum()) > 1000 and int((asg == -1).sum()) > 300
    return files, dict(amps=amps, rows=rows, counts=r.counts, amp_counts=amp_counts, amp_reads=amp_reads), G


def run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    amplipy.main(argv)


def switches(monkeypatch, gpu_sam=False, dist=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, on in (("AMPLIPY_GPU_SAM", gpu_sam), ("AMPLIPY_FORCE_DIST", dist)):
        if on:
            monkeypatch.setenv(k, "1")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check_vcf(with_keys, plain, want):
    """Every record's seven keys are the restatement's word; with the keys and their header lines stripped the file is ``plain``."""
    text = with_keys.decode()
    assert amplicon.HEADER_LINES in text
    out = []
    n_records = n_two = n_primer = 0
    for line in text.replace(amplicon.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-7:]] == list(amplicon.KEYS)
            k = A.keys(int(f[1]) - 1, f[3], f[4].split(","), want["amps"], want["rows"], want["counts"], want["amp_counts"], strand.fisher_two_sided)
            assert ";".join(kvs[-7:]) == A.info_text(k), line
            n_two += "," in k["AMP"]; n_primer += k["PRIMER"] != "."
            f[7] = ";".join(kvs[:-7])
            line = "\t".join(f)
            n_records += 1
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    assert n_records > 12 and n_two > 0 and n_primer > 0
    return n_records


def tsv_text(want):
    lines = ["#amplicon\tref\tpos\tA\tC\tG\tT\tN\tdel\n"]
    amps = want["amps"]
    for a in range(amps.n):
        for j, row in enumerate(want["amp_counts"][amps.off[a]:amps.off[a + 1]].tolist()):
            lines.append("%s\tSYN_REF\t%d\t%s\n" % (amps.names[a], amps.lo[a] + 1 + j, "\t".join(map(str, row))))
    return "".join(lines)


def check_report(with_amps, plain, want):
    rep = json.loads(with_amps)
    assert list(rep)[-1] == "amplicons" and list(rep["reads"])[-1] == "no_amplicon"
    amps = want["amps"]
    assert rep["reads"].pop("no_amplicon") == int(want["amp_reads"][-1])
    assert rep.pop("amplicons") == [{"name": amps.names[a], "start": amps.lo[a], "end": amps.hi[a], "reads": int(want["amp_reads"][a]),
                                     "bases": int(want["amp_counts"][amps.off[a]:amps.off[a + 1]].sum())} for a in range(amps.n)]
    assert (json.dumps(rep, indent=1) + "\n").encode() == plain


_TSV = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_aio_with_amplicon_flags(tmp_path, job, monkeypatch, route, capfd):
    files, want, G = job
    name, inp, out, gpu_sam = route
    switches(monkeypatch, gpu_sam)
    got = {}
    extras = {"plain": [], "amp": ["--amplicons", files["amplicons"], "--amplicon_out", str(tmp_path / "a.tsv")],
              "more": ["--strand", "--qc", str(tmp_path / "more.json")],
              "amp_more": ["--strand", "--qc", str(tmp_path / "amp_more.json"), "--amplicons", files["amplicons"], "--amplicon_out", str(tmp_path / "b.tsv.gz")]}
    for tag, extra in extras.items():
        base = ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + "." + out)),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        capfd.readouterr()
        run(monkeypatch, base + extra)
        log = capfd.readouterr().err
        assert ("Amplicons: %d of %d reads assigned" % (int(want["amp_reads"][:-1].sum()), int(want["amp_reads"].sum())) in log) == ("amp" in tag)
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in ("." + out, ".vcf", ".fas")]
    for tag, base in (("amp", "plain"), ("amp_more", "more")):
        assert got[tag][0] == got[base][0] and got[tag][2] == got[base][2] and len(got[base][0]) > 100000
        assert b"AMP_DP" not in got[base][1]
        check_vcf(got[tag][1], got[base][1], want)
    assert strand.HEADER_LINES in got["amp_more"][1].decode()
    check_report(read(str(tmp_path / "amp_more.json")), read(str(tmp_path / "more.json")), want)
    text = read(str(tmp_path / "a.tsv")).decode()
    assert text == tsv_text(want) and gzip.open(str(tmp_path / "b.tsv.gz"), "rt").read() == text
    _TSV[name] = text
    assert all(t == text for t in _TSV.values())          # the same file on every route run so far
    # an existing --amplicon_out is refused like every other output, before a read is looked at
    with pytest.raises(SystemExit):
        run(monkeypatch, ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / ("x." + out)),
                          "-ov", str(tmp_path / "x.vcf"), "-oc", str(tmp_path / "x.fas"), "--amplicons", files["amplicons"], "--amplicon_out", str(tmp_path / "a.tsv")])
    assert read(str(tmp_path / "a.tsv")).decode() == text


def test_one_rank_through_rccl_gives_the_same_files(tmp_path, job, monkeypatch):
    files, want, G = job
    got = {}
    for tag, dist in (("plain", False), ("dist", True)):
        switches(monkeypatch, dist=dist)
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29549")
        run(monkeypatch, ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                          "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH),
                          "--amplicons", files["amplicons"], "--amplicon_out", str(tmp_path / (tag + ".tsv")), "--qc", str(tmp_path / (tag + ".json"))])
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".vcf", ".tsv", ".fas", ".json")]
    assert got["dist"] == got["plain"]
    assert got["plain"][1].decode() == tsv_text(want)
