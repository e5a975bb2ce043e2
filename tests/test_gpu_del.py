"""The deletion events on the device (amp_del.hip: k_del) through amp_process_batch and
amp_process_batch_device against the plain restatement of tests/del_util.py on the ORACLE's counted alignments, and against the
invariant that pins them to what is already reference-pinned: per position, the events that cover it add up to the '-' column of
the count table and of the strand tallies.  Batch sizes around a wave and a tile; one event on a pile; more keys than a wave, the
block's table and the tile's list hold; keys that collide under either hash; a global table of 16 slots that wraps and one that
is full; state across batches, reset, disable, another capacity, amp_del_add, a small array at amp_del_get; the refusal of a pass
without its results; all five hooks at once.  Last, the command line: aio with --deletions, --del_out and --indel_vcf."""
import gzip
import os
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, lib, synth
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from oracle import oracle
from tests import del_util as D
from tests import strand_util as S

pytestmark = pytest.mark.gpu

MQ, WINDOW = 20, 4
G = 4000
PRIMERS = [(10, 30), (25, 60), (400, 420), (800, 830), (3000, 3030)]
SIZES = [1, 64, 65, 256, 257, 1500]
LDS_SLOTS, LIST, ST_SLOTS = 1024, 1024, 4        # DL_LDS_SLOTS, DL_LIST (amp_del.hpp), ST_SLOTS (amp_strand.hpp); held to the headers below
MESSAGE = "the deletion events need new_pos, new_ncig, new_cig and status of a trimming pass"


def test_the_constants_used_here_are_the_headers():
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amplipy_amd", "csrc")
    text = open(os.path.join(csrc, "amp_del.hpp")).read() + open(os.path.join(csrc, "amp_strand.hpp")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert (1 << val("DL_LDS_LOG2"), val("DL_LIST"), val("ST_SLOTS")) == (LDS_SLOTS, LIST, ST_SLOTS)


_STATE = {}


def state():
    """One engine on the 4,000-base reference, primers set; batches and what their tables must be, made once."""
    if not _STATE:
        tabs = oracle.find_overlapping_primers(G, PRIMERS, 0)
        eng = lib.Engine(G)
        eng.set_primers(*tabs)
        _STATE.update(eng=eng, tabs=tabs, batches={}, wants={})
    return _STATE


def batch(n):
    st = state()
    if n not in st["batches"]:
        st["batches"][n] = S.strand_batch(n, G, PRIMERS, 2000 + n)
    return st["batches"][n]


def want(n, do_trim=True):
    """(table, counts) of batch n: the restatement on the oracle's counted alignments, held to the oracle's '-' column."""
    st = state()
    if (n, do_trim) not in st["wants"]:
        b = batch(n)
        r = oracle.process(b, G, *st["tabs"], MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        t = D.table(S.walked_segments(b, r.trim if do_trim else None), MQ, G)
        assert np.array_equal(D.expand(t, G)[0], r.counts[:, 5])
        st["wants"][(n, do_trim)] = (t, r.counts)
    return st["wants"][(n, do_trim)]


def fresh(do_trim=True, log2_capacity=0):
    eng = state()["eng"]
    eng.set_params(MQ, WINDOW, do_trim, True)
    eng.set_kernel_variant(0)
    eng.reset()
    eng.del_enable(log2_capacity)
    return eng


def got(eng, capacity=1 << 20, lost=0):
    ev, info = eng.del_events()
    assert info["used"] == len(ev) and info["capacity"] == capacity and info["lost"] == lost
    keys = [(int(e["start"]), int(e["len"])) for e in ev]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    return D.as_dict(ev)


def device_batch(b):
    import torch
    from amplipy_amd import synth_torch
    n = b.n
    d = synth_torch.DeviceBatch.from_host(b, "cuda:0")
    out = {k: torch.zeros(max(sz, 1), dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", d.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    return d, out


def dev_out(out, drop=()):
    return abi.AmpTrimOut(*[None if k in drop else out[k].data_ptr() for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")])


# ---- 1. the seeded mix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_events_match_restatement(n, do_trim, route):
    table, counts = want(n, do_trim)
    eng = fresh(do_trim)
    if route == "host":
        eng.process(batch(n))
    else:
        d, out = device_batch(batch(n))
        eng.process_device(d.struct(), 0, dev_out(out, drop=("ref_len", "trim_flags")))        # (the hook needs neither)
        eng.sync()
    assert got(eng) == table
    assert np.array_equal(eng.counts(), counts)
    assert eng.del_last_ms() > 0
    if n >= 1500:
        assert len(table) > 20 and any(v[1] for v in table.values()) and any(v[1] < v[0] for v in table.values())


def test_invariant_against_the_engine_s_own_tables():
    eng = fresh()
    eng.strand_enable()
    try:
        eng.process(batch(1500))
        dash, rev = D.expand(got(eng), G)
        assert np.array_equal(dash, eng.counts()[:, 5]) and np.array_equal(rev, eng.strand_tables()[0][:, 5]) and dash.any() and rev.any()
    finally:
        eng.strand_disable()


# ---- 2. crafted reads -----------------------------------------------------------------------------------------------------------
_EDGE = {}


def run_crafted(segs, ref_len, log2_capacity=0, lost=None):
    """The reads counted as they are (no trimming).  The oracle says which of them are counted (status 0); the table must be the
    restatement's on those, and -- when all are -- ``expand`` of it the '-' column of the oracle's and the engine's count table."""
    b = ReadBatch.from_segments(segs)
    r = oracle.process(b, ref_len, None, None, 0, MQ, WINDOW, do_trim=False, do_count=True)
    counted = [s for s, st in zip(segs, r.trim.status) if st == 0]
    table = D.table(counted, MQ, ref_len)
    if ref_len not in _EDGE:
        _EDGE[ref_len] = lib.Engine(ref_len)
    eng = _EDGE[ref_len]
    eng.set_params(MQ, WINDOW, False, True)
    eng.reset()
    eng.del_enable(log2_capacity)
    res = eng.process(b)
    assert np.array_equal(res.status, r.trim.status)
    if lost is None:
        assert got(eng, 1 << (log2_capacity or 20)) == table
        if len(counted) == len(segs):
            dash = D.expand(table, ref_len)[0]
            assert np.array_equal(dash, r.counts[:, 5]) and np.array_equal(dash, eng.counts()[:, 5])
    return eng, table, len(counted)


def reads_with(keys, rng, flags=None):
    """One read per key (start, len): 6M, the deletion, 6M."""
    return [S.seg(s - 6, [(0, 6), (2, l), (0, 6)], rng, 0 if flags is None else flags[k]) for k, (s, l) in enumerate(keys)]


def test_one_event_on_300_reads_among_300_without():
    rng = np.random.default_rng(9)
    segs = []
    for k in range(600):
        segs.append(S.seg(100, [(0, 30), (2, 9), (0, 30)], rng, 0x10 if k % 3 == 0 else 0) if k % 2 else S.seg(100 + k % 7, [(0, 60)], rng, 0x10 if k % 5 == 0 else 0))
    _, table, _ = run_crafted(segs, 1000)
    assert table == {(130, 9): [300, 100]}


def test_70_distinct_keys_in_one_wave_s_reads():
    rng = np.random.default_rng(10)
    keys = [(200 + 3 * k, 1 + k % 2) for k in range(64)]
    segs = reads_with(keys, rng, [0x10 if k % 2 else 0 for k in range(64)])
    segs[:6] = [S.seg(s.reference_start, [(0, 6), (2, 1), (0, 6), (2, 1), (0, 6)], rng, s.flag) for s in segs[:6]]       # six reads with two
    _, table, _ = run_crafted(segs, 1000)
    assert len(table) == 70


def test_more_keys_than_the_block_s_table_and_the_list_hold():
    rng = np.random.default_rng(11)
    cig = [(0, 3), (2, 1), (0, 3), (2, 2), (0, 3), (2, 1), (0, 3), (2, 3), (0, 3)]
    segs = [S.seg(10 + 40 * k, cig, rng, 0x10 if k % 2 else 0) for k in range(512)]      # two tiles of one block: 2048 keys, the flush, the straight path
    _, table, _ = run_crafted(segs, 40000)
    assert len(table) == 2048 > LDS_SLOTS
    segs = [S.seg(10 + 40 * k, cig + [(2, 2), (0, 3)], rng, 0x10 if k % 2 else 0) for k in range(256)]      # a tile with 1280 events
    _, table, _ = run_crafted(segs, 40000)
    assert len(table) == 1280 > LIST


def test_crafted_edges():
    rng = np.random.default_rng(12)
    # neighbouring deletions, an insertion or a skip between them: one event of length 5
    for k, mid in enumerate(([(2, 2), (2, 3)], [(2, 2), (1, 1), (2, 3)], [(2, 2), (3, 3)])):
        _, table, _ = run_crafted([S.seg(40, [(0, 20)] + mid + [(0, 20)], rng, 0x10 if k % 2 else 0), S.seg(41, [(0, 50)], rng, 0)], 600)
        assert table == {(60, 5): [1, k % 2]}
    # a deletion up to the last base; one on a reference of len + 1 bases; one cut by the reference end (the reference raises
    # there: the read has a status, is not counted, and adds no event)
    _, table, n = run_crafted([S.seg(80, [(0, 10), (2, 10)], rng, 0x10), S.seg(70, [(0, 10), (2, 15), (0, 5)], rng, 0)], 100)
    assert table == {(90, 10): [1, 1], (80, 15): [1, 0]} and n == 2
    _, table, n = run_crafted([S.seg(0, [(0, 1), (2, 7)], rng, 0)], 8)
    assert table == {(1, 7): [1, 0]} and n == 1
    _, table, n = run_crafted([S.seg(80, [(0, 10), (2, 15), (0, 5)], rng, 0x10), S.seg(80, [(0, 10), (2, 4), (0, 5)], rng, 0)], 100)
    assert table == {(90, 4): [1, 0]} and n == 1
    # more deletion segments than a tally kernel has segment slots
    segs = [S.seg(12, S.many_segment_cigar(ST_SLOTS + 3), rng, 0x10), S.seg(12, S.many_segment_cigar(20), rng, 0)]
    _, table, _ = run_crafted(segs, 800)
    assert len(table) == 20 and table[(14, 1)] == [2, 1]
    # irregular CIGARs walk: a soft clip inside, a padding op (the reference raises: not counted), QUAL '*'
    star = Segment(flag=0x10, reference_start=40, cigar=[(2, 3), (0, 10), (2, 2), (0, 5)], query_sequence="ACGTACGTACGTACG", query_qualities=None)
    segs = [S.seg(40, [(0, 10), (4, 5), (2, 3)], rng, 0x10), S.seg(40, [(0, 10), (2, 2), (6, 1), (2, 3), (0, 10)], rng, 0), star]
    b = ReadBatch.from_segments(segs)
    r = oracle.process(b, 600, None, None, 0, MQ, WINDOW, do_trim=False, do_count=True)
    assert list(r.trim.status != 0) == [False, True, True]
    _, table, n = run_crafted(segs, 600)
    assert table == {(50, 3): [1, 1]} and n == 1


def test_trimming_cuts_through_a_deletion():
    rng = np.random.default_rng(5)
    segs_in = [S.seg(100, [(0, 25), (2, 12), (0, 60)], rng, 0x10), S.seg(102, [(0, 20), (2, 20), (0, 60)], rng, 0), S.seg(100, [(0, 45), (2, 4), (0, 40)], rng, 0)]
    b = ReadBatch.from_segments(segs_in)
    tabs = oracle.find_overlapping_primers(600, [(100, 130)], 0)
    r = oracle.process(b, 600, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    table = D.table(S.walked_segments(b, r.trim), MQ, 600)
    eng = lib.Engine(600)
    eng.set_primers(*tabs)
    eng.set_params(MQ, WINDOW, True, True)
    eng.del_enable()
    eng.process(b)
    assert got(eng) == table != D.table(segs_in, MQ, 600)
    assert np.array_equal(D.expand(table, 600)[0], eng.counts()[:, 5]) and np.array_equal(eng.counts(), r.counts)
    eng.close()


def test_keys_that_collide_under_either_hash():
    rng = np.random.default_rng(8)
    ref_len = 200000
    lds = D.colliding_keys(lambda k: D.slot_lds(k, LDS_SLOTS), range(10, ref_len - 20), 3)
    glob = D.colliding_keys(lambda k: D.slot_global(k, 20), range(10, ref_len - 20), 4)
    keys = [lds[0], lds[1], lds[0], glob[0], glob[1], glob[1], lds[1], lds[1]]
    _, table, _ = run_crafted(reads_with(keys, rng, [0, 0x10, 0x10, 0, 0x10, 0, 0, 0x10]), ref_len)
    assert table == {lds[0]: [2, 1], lds[1]: [3, 2], glob[0]: [1, 0], glob[1]: [2, 1]}


def test_a_table_of_16_slots_wraps_and_a_full_one_loses_whole_events():
    rng = np.random.default_rng(11)
    ref_len = 100000
    last = [k for k in ((s, 2) for s in range(10, 5000)) if D.slot_global(D.key_of(*k), 4) == 15][:3]
    others = [k for k in ((s, 3) for s in range(10, 5000)) if D.slot_global(D.key_of(*k), 4) not in (15, 0, 1)][:9]
    keys12 = last + others
    reads = [k for j, k in enumerate(keys12) for _ in range(j + 1)]
    _, table, _ = run_crafted(reads_with(reads, rng, [0x10 if j % 2 else 0 for j in range(len(reads))]), ref_len, log2_capacity=4)
    assert len(table) == 12 and [table[k][0] for k in keys12] == list(range(1, 13))          # (three keys of slot 15: probing wrapped)
    # 24 keys into 16 slots
    keys24 = [(100 + 10 * j, 1 + j % 4) for j in range(24)]
    reads = [k for j, k in enumerate(keys24) for _ in range(j % 5 + 1)]
    segs = reads_with(reads, rng, [0x10 if j % 3 == 0 else 0 for j in range(len(reads))])
    eng, table, n = run_crafted(segs, ref_len, log2_capacity=4, lost=True)          # the call returns
    ev, info = eng.del_events()
    stored = D.as_dict(ev)
    assert info["used"] == 16 == len(stored) and info["capacity"] == 16 and n == len(segs)
    assert all(stored[k] == table[k] for k in stored)                                # every stored entry is exact: nothing merged
    assert info["lost"] == sum(v[0] for k, v in table.items() if k not in stored) > 0
    assert sum(v[0] for v in stored.values()) + info["lost"] == sum(v[0] for v in table.values())
    eng.del_enable(0)                                                                # (the shared engine back on the default table)


# ---- 3. state -------------------------------------------------------------------------------------------------------------------
def test_batches_accumulate_reset_zeroes_disable_keeps_and_del_add_sums():
    eng = fresh()
    eng.process(batch(257))
    eng.process(batch(1500))
    both = D.add_tables(want(257)[0], want(1500)[0])
    assert got(eng) == both
    eng.reset()
    assert got(eng) == {}
    eng.process(batch(257))
    eng.del_disable()
    eng.process(batch(1500))
    assert got(eng) == want(257)[0]                     # readable, and nothing was added
    eng.del_add(D.as_array(want(1500)[0]))              # another job's table: the per-key sum
    assert got(eng) == both
    eng.del_add(np.zeros(0, abi.DEL_EVENT_DTYPE))
    assert got(eng) == both
    eng.del_enable()                                    # on again: the table starts at zero
    assert got(eng) == {}


def test_another_capacity_lays_the_table_out_again():
    eng = fresh()
    eng.process(batch(257))
    eng.del_enable(12)
    assert got(eng, 1 << 12) == {}
    eng.process(batch(257))
    assert got(eng, 1 << 12) == want(257)[0]
    for bad in (3, 29, -1):
        with pytest.raises(lib.AmpliHipError) as e:
            eng.del_enable(bad)
        assert e.value.rc == -1
    assert got(eng, 1 << 12) == want(257)[0]
    eng.del_enable(0)
    assert got(eng) == {}


def test_get_with_a_small_array_says_how_many_and_before_the_first_enable_is_an_error():
    import ctypes as C
    eng = fresh()
    eng.process(batch(1500))
    table = want(1500)[0]
    ev = np.zeros(len(table), abi.DEL_EVENT_DTYPE)
    n = C.c_int64(-1)
    info = np.zeros(3, np.uint64)
    rc = eng.L.amp_del_get(eng.h, C.c_void_p(abi.ptr(ev)), C.c_int64(len(table) - 1), C.byref(n), C.c_void_p(abi.ptr(info)))
    assert rc == -1 and n.value == len(table) and not ev["count"].any() and list(info) == [len(table), 1 << 20, 0]
    rc = eng.L.amp_del_get(eng.h, C.c_void_p(abi.ptr(ev)), C.c_int64(len(table)), C.byref(n), None)
    assert rc == 0 and n.value == len(table) and D.as_dict(ev) == table
    e = lib.Engine(500)
    for call in (e.del_events, e.del_last_ms, lambda: e.del_add(D.as_array({(5, 1): [1, 0]}))):
        with pytest.raises(lib.AmpliHipError) as err:
            call()
        assert err.value.rc == -5
    e.del_disable()             # off while off: nothing to do
    e.close()


def test_a_pass_without_status_is_refused_with_the_hook_s_message():
    eng = fresh()
    eng.process(batch(257))
    before = eng.counts()
    d, out = device_batch(batch(1500))
    for drop in (("status",), ("new_cig",), None):
        with pytest.raises(lib.AmpliHipError) as e:
            eng.process_device(d.struct(), 0, None if drop is None else dev_out(out, drop=drop))
        assert e.value.rc == -1 and MESSAGE in str(e.value)
        eng.sync()
        assert np.array_equal(eng.counts(), before) and got(eng) == want(257)[0]
        assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.set_params(MQ, WINDOW, False, True)                            # without trimming nothing of dev_out is needed
    eng.reset()
    eng.process_device(d.struct(), 0, None)
    eng.sync()
    assert got(eng) == want(1500, do_trim=False)[0]


def test_all_five_hooks_at_once_leave_the_other_four_alone():
    from amplipy_amd import codon
    from tests import amplicon_util as A
    from tests import codon_util as U
    amps, rows = A.example_amps(), A.example_rows()
    primers = sorted((s, e) for s, e, _ in rows)
    tabs = oracle.find_overlapping_primers(amps.G, primers, 0)
    b = S.strand_batch(1025, amps.G, primers, 2025)
    cds = U.overlapping(amps.G)
    eng = lib.Engine(amps.G)
    eng.set_primers(*tabs)
    eng.set_params(MQ, WINDOW, True, True)
    snaps = []
    for with_del in (False, True):
        eng.reset()
        eng.qc_enable(primers, 0, 60); eng.strand_enable(); amps.enable(eng); codon.enable(eng, cds)
        if with_del:
            eng.del_enable()
        res = eng.process(b)
        t, ps, pe = eng.qc_read_tallies()
        snaps.append([np.array([t[k] for k in abi.QC_READ_FIELDS], np.uint64), ps, pe, *eng.strand_tables(), *eng.amplicon_tables(), *eng.codon_tables(),
                      eng.counts(), res.status, res.new_pos, res.new_ncig, res.new_cig])
    assert len(snaps[0]) == len(snaps[1]) and all(snaps[0][k].any() for k in (0, 3, 5, 7, 9))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(snaps[0], snaps[1]))
    r = oracle.process(b, amps.G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert got(eng) == D.table(S.walked_segments(b, r.trim), MQ, amps.G) != {}
    for h in ("qc", "strand", "amplicon", "codon", "del"):
        assert getattr(eng, h + "_last_ms")() > 0
    eng.close()


# ---- 4. the command line --------------------------------------------------------------------------------------------------------
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST")
N_PLANTED = 400


def write_reads(path, mode, hb, ref_len):
    from amplipy_amd import bamio
    from amplipy_amd.batch import SEQ_NT16, unpack_nibbles
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % ref_len, [("SYN_REF", ref_len)])
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


def run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    amplipy.main(argv)


def test_aio_with_the_deletion_flags(tmp_path, monkeypatch):
    """aio on a small synthetic BAM -- the seeded mix and 400 reads, on both strands, that carry one 9-base deletion -- with
    --deletions, --del_out and --indel_vcf: the default VCF's lines, the two keys stripped, are byte for byte those of a run
    without the flags, the keys and the TSV are the restatement's word, and the indel VCF holds the planted deletion once, with
    the planted read count."""
    import io
    from amplipy_amd import deletion
    g = synth.make_genome()
    ref_len = int(g.size)
    ref = synth.genome_string(g)
    primers, amps = synth.make_artic_scheme()
    pr = sorted((s, e) for s, e, _ in primers)
    rng = np.random.default_rng(77)
    a0 = int(amps[40][0])
    planted = [S.seg(a0 + k % 3, [(0, 150 - k % 3), (2, 9), (0, 50)], rng, 0x10 if k % 4 == 0 else 0) for k in range(N_PLANTED)]
    mix = S.strand_batch(1500, ref_len, pr, 41, sort=False)
    segs = sorted([mix.segment(i) for i in range(mix.n)] + planted, key=lambda s: s.reference_start)
    batch = ReadBatch.from_segments(segs)
    key = (a0 + 150, 9)
    tabs = oracle.find_overlapping_primers(ref_len, pr, 0)
    r = oracle.process(batch, ref_len, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    table = D.table(S.walked_segments(batch, r.trim), MQ, ref_len)
    assert table[key] == [N_PLANTED, N_PLANTED // 4] and np.array_equal(D.expand(table, ref_len)[0], r.counts[:, 5])
    d = tmp_path
    (d / "ref.fas").write_text(">SYN_REF test\n" + ref + "\n")
    synth.write_bed(str(d / "p.bed"), primers)
    write_reads(str(d / "in.bam"), "wb", batch, ref_len)
    base = ["aio", "-i", str(d / "in.bam"), "-p", str(d / "p.bed"), "-r", str(d / "ref.fas"), "-ml", "30"]
    outs = lambda tag: ["-ot", str(d / (tag + ".bam")), "-ov", str(d / (tag + ".vcf")), "-oc", str(d / (tag + ".fas"))]
    run(monkeypatch, base + outs("plain"))
    run(monkeypatch, base + outs("del") + ["--deletions", "--del_out", str(d / "d.tsv.gz"), "--indel_vcf", str(d / "i.vcf")])
    read = lambda name: open(str(d / name), "rb").read()
    assert read("del.bam") == read("plain.bam") and read("del.fas") == read("plain.fas") and b"DEL_N" not in read("plain.vcf")
    want = deletion.Tables(D.as_array(table), r.counts, ref, amplipy.DEFAULTS["min_depth_variants"], amplipy.DEFAULTS["min_freq_variants"])
    # the default VCF
    text = read("del.vcf").decode()
    assert deletion.HEADER_LINES in text
    out, n_records, n_listed = [], 0, 0
    for line in text.replace(deletion.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-2:]] == list(deletion.KEYS) and kvs[-3].startswith("ALT_FREQ=")
            assert ";".join(kvs[-2:]) == want.info(int(f[1]) - 1, int(kvs[0].split("=")[1]))
            n_listed += kvs[-1] != "DEL=."
            f[7] = ";".join(kvs[:-2])
            line = "\t".join(f)
            n_records += 1
        out.append(line + "\n")
    assert "".join(out).encode() == read("plain.vcf") and n_records > 12 and n_listed >= 9
    assert ("DEL=%d-%d:%d:%d" % (key[0] + 1, key[0] + 9, N_PLANTED, N_PLANTED // 4)) in text
    # the event table
    f = io.StringIO()
    deletion.write_tsv(f, "SYN_REF", want)
    assert gzip.open(str(d / "d.tsv.gz"), "rt").read() == f.getvalue() and f.getvalue().count("\n") == len(table) + 1
    # the indel VCF: the planted deletion once, with the planted read count; every REF is the reference at its POS
    lines = [l.split("\t") for l in read("i.vcf").decode().splitlines() if not l.startswith("#")]
    hits = [l for l in lines if int(l[1]) == key[0] and len(l[3]) == 10]
    assert len(hits) == 1 and hits[0][3] == ref[key[0] - 1:key[0] + 9] and hits[0][4] == ref[key[0] - 1]
    assert hits[0][7].startswith("DP=%d;AD=%d;RV=%d;AF=" % (int(r.counts[key[0]].sum()), N_PLANTED, N_PLANTED // 4))
    assert all(ref[int(l[1]) - 1:int(l[1]) - 1 + len(l[3])] == l[3] and len(l[3]) != len(l[4]) for l in lines) and len(lines) >= 1
    assert [int(l[1]) for l in lines] == sorted(int(l[1]) for l in lines)
    assert sum(len(l[3]) > len(l[4]) for l in lines) == len(want.called())
    assert read("i.vcf").decode() == indel_text(want, deletion.insertion_rows(vcf_records(read("plain.vcf").decode())))
    # an existing output is refused before a read is looked at; a table that is too small ends the run with an error
    with pytest.raises(SystemExit):
        run(monkeypatch, base + outs("x") + ["--indel_vcf", str(d / "i.vcf")])
    with pytest.raises(RuntimeError) as e:
        run(monkeypatch, base + outs("y") + ["--del_out", str(d / "y.tsv"), "--del_capacity", "4"])
    assert "--del_capacity" in str(e.value)


def vcf_records(text):
    """The records of a default VCF as the call made them, as far as deletion.insertion_rows reads them."""
    from amplipy_amd import calling
    recs = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        info = dict(kv.split("=") for kv in f[7].split(";"))
        recs.append(calling.VariantRecord(int(f[1]) - 1, f[3], f[4].split(","), int(info["DP"]), int(info["REF_DP"]), info["ALT_DP"].split(","),
                                          float(info["REF_FREQ"]), info["ALT_FREQ"].split(","), ()))
    return recs


def indel_text(tables, insertions):
    import io
    from amplipy_amd import deletion
    f = io.StringIO()
    deletion.write_indel_vcf(f, "SYN_REF", tables, insertions, "amplipy_amd pinned")
    return f.getvalue()
