"""The read haplotypes on the device (amp_hap.hip: k_hap) through amp_process_batch and
amp_process_batch_device against the plain restatement of tests/hap_util.py on the ORACLE's counted alignments, with the
invariant of section 22 held wherever a table is read; and against what is already reference-pinned: one-position regions give
the count table's columns, and three sites inside a region give k_cooc's pattern cells.  Batch sizes round a wave and a tile; the
crafted edges; one key on a pile; more distinct keys than a wave has lanes; keys that start at one slot and keys that differ in
their last word alone; a table of 16 slots that wraps and one that is full; state across batches, reset, disable, another
capacity, other regions, amp_hap_add, a small array at amp_hap_get; the refusal of a pass without its results; all hooks at once.
Last, the command line: aio, variants and consensus with --haplotypes, one device codec route, the lost error, two ranks."""
import ctypes as C
import gzip
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, haplotype, lib, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import codon_util as CU
from tests import cooc_util as CO
from tests import hap_util as U
from tests import strand_util as S
from tests.test_gpu_del import G, PRIMERS, SWITCHES, dev_out, device_batch, write_reads

pytestmark = pytest.mark.gpu

MQ, WINDOW = 20, 4
SIZES = [1, 64, 65, 256, 257, 1500]
MESSAGE = "the read haplotypes need new_pos, new_ncig, new_cig and status of a trimming pass"
REF = U.reference(G)
REGIONS = U.regions_near(PRIMERS, G)

_STATE = {}


def state():
    """One engine on the 4,000-base reference, primers set; batches and what their tables must be, made once."""
    if not _STATE:
        tabs = oracle.find_overlapping_primers(G, PRIMERS, 0)
        eng = lib.Engine(G)
        eng.set_primers(*tabs)
        _STATE.update(eng=eng, tabs=tabs, batches={}, wants={})
    return _STATE


def planted():
    return [(e + 30, U.other(REF[e + 30]), 2) for _, e in PRIMERS if REF[e + 30] in "ACGT"]


def batch(n):
    """The seeded mix laid onto the reference: one base in a hundred changed, two planted variants, one quality in fifty low."""
    st = state()
    if n not in st["batches"]:
        st["batches"][n] = U.onto_reference(S.strand_batch(n, G, PRIMERS, 2000 + n), REF, 77 + n, rate=0.01, planted=planted(), low_rate=0.02)
    return st["batches"][n]


def want(n, do_trim=True, regions=None):
    """(table, tally, reads, counts) of batch n: the restatement on the oracle's counted alignments."""
    st = state()
    key = (n, do_trim, None if regions is None else tuple(regions))
    if key not in st["wants"]:
        b = batch(n)
        r = oracle.process(b, G, *st["tabs"], MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        t = U.tables(S.walked_segments(b, r.trim if do_trim else None), G, regions or REGIONS, REF, MQ)
        U.check_invariant(t[0], t[1])
        r.counts.setflags(write=False)
        st["wants"][key] = t + (r.counts,)
    return st["wants"][key]


def enable(eng, regions=None, ref=None, log2_capacity=0):
    regions = REGIONS if regions is None else regions
    eng.hap_enable([s for s, _ in regions], [e for _, e in regions], REF if ref is None else ref, log2_capacity)


def fresh(do_trim=True, log2_capacity=0, regions=None):
    eng = state()["eng"]
    eng.set_params(MQ, WINDOW, do_trim, True)
    eng.set_kernel_variant(0)
    eng.reset()
    enable(eng, regions, None, log2_capacity)
    return eng


def got(eng, capacity=1 << 20, lost=0):
    """(table, tally, reads) as the engine has them, the invariant and the order of the entries held."""
    ev, info, tally, reads = eng.hap_tables()
    assert info["used"] == len(ev) and info["capacity"] == capacity and info["lost"] == lost
    keys = [haplotype.entry_key(e) for e in ev]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    table = U.as_dict(ev)
    U.check_invariant(table, tally, lost)
    return table, tally, reads


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 1. the seeded mix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(n, do_trim, route):
    w = want(n, do_trim)
    eng = fresh(do_trim)
    if route == "host":
        eng.process(batch(n))
    else:
        d, out = device_batch(batch(n))
        eng.process_device(d.struct(), 0, dev_out(out, drop=("ref_len", "trim_flags")))        # (the hook needs neither)
        eng.sync()
    assert same(got(eng), w)
    assert np.array_equal(eng.counts(), w[3])
    assert eng.hap_last_ms() > 0
    if n >= 1500:
        table, tally, reads = w[:3]
        assert len(table) > 50 and tally[:, U.REF].sum() > 500 and tally[:, U.LOWQ].sum() > 50 and tally[:, U.EDGE].sum() > 0
        assert any(v[1] for v in table.values()) and any(v[0] > 20 for v in table.values()) and int(reads[1]) > 0


# ---- 2. crafted reads -----------------------------------------------------------------------------------------------------------
_EDGE = {}


def run_crafted(segs, regions, mq=MQ, do_trim=False, log2_capacity=0, lost=None):
    """Reads on the crafted reference through an engine of its own.  The oracle says which of them are counted (status 0) and
    how (the trimmed alignment with do_trim); the tables must be the restatement's on those.  -> (engine, wanted tables)"""
    ref_len = U.CRAFT_G
    b = ReadBatch.from_segments(segs)
    tabs = oracle.find_overlapping_primers(ref_len, U.CRAFT_PRIMERS, 0)
    r = oracle.process(b, ref_len, *(tabs if do_trim else (None, None, 0)), mq, WINDOW, do_trim=do_trim, do_count=True)
    counted = S.walked_segments(b, r.trim) if do_trim else [s for s, st in zip(segs, r.trim.status) if st == 0]
    w = U.tables(counted, ref_len, regions, U.CRAFT_REF, mq)
    if ref_len not in _EDGE:
        _EDGE[ref_len] = lib.Engine(ref_len)
        _EDGE[ref_len].set_primers(*tabs)
    eng = _EDGE[ref_len]
    eng.set_params(mq, WINDOW, do_trim, True)
    eng.reset()
    enable(eng, regions, U.CRAFT_REF, log2_capacity)
    res = eng.process(b)
    assert np.array_equal(res.status, r.trim.status) and np.array_equal(eng.counts(), r.counts)
    if lost is None:
        assert same(got(eng, 1 << (log2_capacity or 20)), w)
    return eng, w


_CRAFTED = U.crafted()


@pytest.mark.parametrize("case", _CRAFTED, ids=[c[0] for c in _CRAFTED])
def test_crafted_edges(case):
    name, regions, segs, mq, do_trim, expect = case
    eng, w = run_crafted(segs, regions, mq=mq, do_trim=do_trim)
    expect(*got(eng))


def test_one_key_on_a_pile_of_1500_reads():
    regions, segs, key = U.pile_case()
    eng, w = run_crafted(segs, regions)
    assert w[0] == {key: [1500, 500]} and w[1][0].tolist() == [1500, 0, 0, 0, 0, 0] and list(w[2]) == [1500, 0]


def test_more_distinct_keys_than_a_wave_has_lanes():
    regions, segs = U.distinct_keys_case()
    eng, w = run_crafted(segs, regions)
    assert len(w[0]) == 200 > 64 and all(v[0] == 1 for v in w[0].values())


def test_keys_that_start_at_one_slot_and_keys_that_differ_in_their_last_word():
    """The keys share head and twelve difference words and differ in the thirteenth -- the LAST key word, the last one claimed;
    among them three that start at one slot of a table of 256 and three that start at another, each carried by two reads."""
    region = (3300, 3400)
    variants = [(j, w) for j in range(30) for w in (1, 2, 3)]
    segs, keys = U.thirteen_diff_reads(region, variants)
    assert len({tuple(U.key_words(*k)[:13]) for k in keys}) == 1 and len({U.key_words(*k)[13] for k in keys}) == len(keys)
    by_slot = {}
    for k, key in enumerate(keys):
        by_slot.setdefault(U.slot_global(*key, 8), []).append(k)
    groups = [v[:3] for v in by_slot.values() if len(v) >= 3][:2]
    assert len(groups) == 2
    pick = [k for g in groups for k in g]
    reads = [segs[k] for k in pick] + [U.copy_of(segs[k], 0x10) for k in pick]
    eng, w = run_crafted(reads, [region], log2_capacity=8)
    assert w[0] == {keys[k]: [2, 1] for k in pick}


def test_a_table_of_16_slots_wraps_and_a_full_one_loses_whole_keys():
    region = (3300, 3400)
    variants = [(j, w) for j in range(20) for w in (1, 2, 3)]
    segs, keys = U.thirteen_diff_reads(region, variants)
    at15 = [k for k, key in enumerate(keys) if U.slot_global(*key, 4) == 15][:3]
    assert len(at15) == 3
    twelve = at15 + [k for k in range(60) if k not in at15][:9]
    eng, w = run_crafted([segs[k] for j, k in enumerate(twelve) for _ in range(j + 1)], [region], log2_capacity=4)
    assert [w[0][keys[k]][0] for k in twelve] == list(range(1, 13))               # (three keys of slot 15: probing wrapped)
    # 40 keys into 16 slots, filled in two batches: the second batch's new keys find a full table
    eng, w16 = run_crafted(segs[:16], [region], log2_capacity=4)
    assert len(w16[0]) == 16
    later = [segs[k] for k in range(8, 40) for _ in range(1 + k % 3)]
    eng.process(ReadBatch.from_segments(later))
    w2 = U.tables(later, U.CRAFT_G, [region], U.CRAFT_REF, MQ)
    lost = sum(v[0] for key, v in w2[0].items() if key not in w16[0])
    ev, info, tally, reads = eng.hap_tables()
    stored = U.as_dict(ev)
    assert info["used"] == 16 == len(stored) and info["capacity"] == 16 and info["lost"] == lost > 0
    both = U.add_tables(w16[0], w2[0])
    assert set(stored) == set(w16[0]) and all(stored[k] == both[k] for k in stored)          # every stored entry is exact: nothing merged
    U.check_invariant(stored, tally, lost)
    assert np.array_equal(tally, w16[1] + w2[1]) and np.array_equal(reads, w16[2] + w2[2])
    enable(eng, [region], U.CRAFT_REF, 0)                                                    # (the shared engine back on the default table)


# ---- 3. state -------------------------------------------------------------------------------------------------------------------
def add3(a, b):
    return U.add_tables(a[0], b[0]), a[1] + b[1], a[2] + b[2]


def test_batches_accumulate_reset_zeroes_disable_keeps_and_hap_add_sums():
    eng = fresh()
    eng.process(batch(257))
    eng.process(batch(1500))
    both = add3(want(257), want(1500))
    assert same(got(eng), both)
    eng.reset()
    t = got(eng)
    assert t[0] == {} and not t[1].any() and not t[2].any()
    eng.process(batch(257))
    eng.hap_disable()
    eng.process(batch(1500))
    assert same(got(eng), want(257))                    # readable, and nothing was added
    w = want(1500)
    big = np.array([2 ** 40 + 5, 0], np.uint64)
    eng.hap_add(U.as_array(w[0]), w[1], w[2] + big)     # another rank's tables: the per-key sum; a read count beyond 32 bits
    t = got(eng)
    assert t[0] == both[0] and np.array_equal(t[1], both[1]) and np.array_equal(t[2], both[2] + big)
    eng.hap_add(np.zeros(0, abi.HAP_ENTRY_DTYPE))
    assert got(eng)[0] == both[0]
    with pytest.raises(lib.AmpliHipError) as e:         # an entry of a region the engine does not have
        bad = U.as_array({(len(REGIONS), ((1, 0, 0),)): [1, 0]})
        eng.hap_add(bad)
    assert e.value.rc == -1
    enable(eng)                                         # on again: the tables start at zero
    assert got(eng)[0] == {}


def test_another_capacity_and_other_regions_lay_the_tables_out_again():
    eng = fresh()
    eng.process(batch(257))
    enable(eng, log2_capacity=12)
    assert got(eng, 1 << 12)[0] == {}
    eng.process(batch(257))
    assert same(got(eng, 1 << 12), want(257))
    for bad in (3, 29, -1):
        with pytest.raises(lib.AmpliHipError) as e:
            enable(eng, log2_capacity=bad)
        assert e.value.rc == -1
    assert same(got(eng, 1 << 12), want(257))
    other = [(70, 90), (70, 71), (450, 520), (3050, 3100)]
    enable(eng, other)
    eng.process(batch(1500))
    t = got(eng)
    assert t[1].shape == (4, 6) and same(t, want(1500, regions=other)) and t[0]
    enable(eng)


def test_bad_regions_are_refused():
    e = lib.Engine(500)
    ref = "ACGT" * 125
    for st, en in (([10, 5], [20, 15]), ([10], [10]), ([10], [9]), ([0], [4097]), ([-1], [5]), ([490], [501])):
        with pytest.raises(lib.AmpliHipError) as err:
            e.hap_enable(st, en, ref)
        assert err.value.rc == -1, (st, en)
    e.close()
    big = lib.Engine(70000)
    n = abi.HAP_MAX_REGIONS + 1
    with pytest.raises(lib.AmpliHipError) as err:           # one region more than 2^16
        big.hap_enable(np.arange(n), np.arange(n) + 1, "A" * 70000, 4)
    assert err.value.rc == -1
    big.hap_enable(np.arange(n - 1), np.arange(n - 1) + 1, "A" * 70000, 4)
    big.hap_enable([0, 0], [4096, 1], "A" * 70000, 4)       # equal starts in any order, the longest region
    big.close()


def test_get_with_a_small_array_says_how_many_and_before_the_first_enable_is_an_error():
    eng = fresh()
    eng.process(batch(1500))
    w = want(1500)
    ev = np.zeros(len(w[0]), abi.HAP_ENTRY_DTYPE)
    n = C.c_int64(-1)
    info = np.zeros(3, np.uint64); tally = np.zeros((len(REGIONS), 6), np.uint64); reads = np.zeros(2, np.uint64)
    rc = eng.L.amp_hap_get(eng.h, C.c_void_p(abi.ptr(ev)), C.c_int64(len(w[0]) - 1), C.byref(n), C.c_void_p(abi.ptr(info)), C.c_void_p(abi.ptr(tally)),
                           C.c_void_p(abi.ptr(reads)))
    assert rc == -1 and n.value == len(w[0]) and not ev["count"].any() and list(info) == [len(w[0]), 1 << 20, 0]
    assert np.array_equal(tally, w[1]) and np.array_equal(reads, w[2])
    rc = eng.L.amp_hap_get(eng.h, C.c_void_p(abi.ptr(ev)), C.c_int64(len(w[0])), C.byref(n), None, None, None)
    assert rc == 0 and n.value == len(w[0]) and U.as_dict(ev) == w[0]
    e = lib.Engine(500)
    for call in (e.hap_tables, e.hap_last_ms, lambda: e.hap_add(U.as_array({(0, ((1, 0, 0),)): [1, 0]}))):
        with pytest.raises(lib.AmpliHipError) as err:
            call()
        assert err.value.rc == -5
    e.hap_disable()             # off while off: nothing to do
    e.close()


def test_a_pass_without_its_results_is_refused_with_the_hook_s_message():
    eng = fresh()
    eng.process(batch(257))
    before = eng.counts()
    d, out = device_batch(batch(1500))
    for drop in (("status",), ("new_cig",), None):
        with pytest.raises(lib.AmpliHipError) as e:
            eng.process_device(d.struct(), 0, None if drop is None else dev_out(out, drop=drop))
        assert e.value.rc == -1 and MESSAGE in str(e.value)
        eng.sync()
        assert np.array_equal(eng.counts(), before) and same(got(eng), want(257))
        assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.set_params(MQ, WINDOW, False, True)                            # without trimming nothing of dev_out is needed
    eng.reset()
    eng.process_device(d.struct(), 0, None)
    eng.sync()
    assert same(got(eng), want(1500, do_trim=False))


def test_all_hooks_at_once_leave_the_others_alone():
    """On the example primer set, which has amplicons: every other hook's tables are the same bytes with the haplotypes on and
    off, and the haplotype tables are the restatement's."""
    from amplipy_amd import codon, errprof
    from tests import amplicon_util as A
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
    for with_hap in (False, True):
        eng.reset()
        eng.qc_enable(primers, 0, 60); eng.strand_enable(); amps.enable(eng); codon.enable(eng, cds); eng.del_enable(); eng.cooc_enable(*sets.arrays())
        errprof.enable(eng, ref, None)
        if with_hap:
            enable(eng, regions, ref)
        res = eng.process(b)
        t, ps, pe = eng.qc_read_tallies()
        snaps.append([np.array([t[k] for k in abi.QC_READ_FIELDS], np.uint64), ps, pe, *eng.strand_tables(), *eng.amplicon_tables(), *eng.codon_tables(),
                      eng.del_events()[0], *eng.cooc_tables(), *eng.errprof_tables(), eng.counts(), res.status, res.new_pos, res.new_ncig, res.new_cig])
    assert len(snaps[0]) == len(snaps[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(snaps[0], snaps[1]))
    assert all(np.frombuffer(snaps[0][k].tobytes(), np.uint8).any() for k in (0, 3, 5, 7, 9, 10, 12))
    r = oracle.process(b, amps.G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    w = U.tables(S.walked_segments(b, r.trim), amps.G, regions, ref, MQ)
    assert same(got(eng), w) and w[0] and w[1][:, U.REF].any()
    for h in ("qc", "strand", "amplicon", "codon", "del", "cooc", "errprof", "hap"):
        assert getattr(eng, h + "_last_ms")() > 0
    eng.close()


# ---- 4. pinned to the count table and to k_cooc -----------------------------------------------------------------------------------
_GOOD = {}


def good_batch():
    """1500 reads of the mix with a REGULAR CIGAR as they come in, every quality at or above min_quality, no base N; counted
    untrimmed.  -> (batch, segments, the oracle's counts)"""
    if not _GOOD:
        raw = S.strand_batch(2200, G, PRIMERS, 4242)
        keep = [i for i in range(raw.n) if CU.is_regular(raw.segment(i), G)][:1500]
        assert len(keep) == 1500
        b = U.onto_reference(synth.gather_rows(raw, np.array(keep)), REF, 99, rate=0.012, planted=planted())
        segs = []
        for i in range(b.n):
            s = b.segment(i)
            s.query_sequence = s.query_sequence.replace("N", "A")
            s.query_qualities = type(s.query_qualities)("B", [max(int(q), 25) for q in s.query_qualities])
            segs.append(s)
        b = ReadBatch.from_segments(segs)
        r = oracle.process(b, G, None, None, 0, MQ, WINDOW, do_trim=False, do_count=True)
        assert not r.trim.status.any() and all(min(s.query_qualities) >= MQ for s in segs)
        _GOOD.update(b=b, segs=segs, counts=r.counts)
    return _GOOD["b"], _GOOD["segs"], _GOOD["counts"]


def condition(segs, regions):
    """What makes the two pinned tests say something, asserted on the RESTATEMENT's numbers before the device is asked: at least
    half of the status-0 reads cover some region, and at least a quarter of the covering reads carry a non-reference signature."""
    cover, keyed = U.covering_and_non_ref(segs, G, regions, REF, MQ)
    assert cover * 2 >= len(segs) and keyed * 4 >= cover, (len(segs), cover, keyed)


def test_one_position_regions_give_the_count_table():
    b, segs, counts = good_batch()
    # one-position regions round every primer -- every position behind it, every third in front of it and further behind --
    # where the reference letter is among A C G T
    ps = set()
    for s, e in PRIMERS:
        ps |= set(range(e + 2, e + 34)) | set(range(max(s - 40, 0), s, 3)) | set(range(e + 34, e + 100, 3))
    regions = sorted((p, p + 1) for p in ps if REF[p].upper() in "ACGT")
    w = U.tables(segs, G, regions, REF, MQ)
    U.check_invariant(w[0], w[1])
    condition(segs, regions)
    eng = fresh(do_trim=False, regions=regions)
    eng.process(b)
    t = got(eng)
    assert same(t, w) and np.array_equal(eng.counts(), counts)
    table, tally, reads = t
    seen = 0
    for k, (s, en) in enumerate(regions):
        if en - s != 1:
            continue
        x = "ACGT".index(REF[s].upper())
        cols = [table.get((k, ((0, kind, 0),)), [0, 0])[0] for kind in range(5)]
        assert not any(key[0] == k and key[1][0][1] == U.KIND_DEL for key in table)
        cols[x] += int(tally[k, U.REF])
        assert cols == counts[s, :5].tolist() and int(tally[k, U.EDGE]) == int(counts[s, 5]), (s, cols, counts[s].tolist())
        assert not tally[k, U.LOWQ] and not tally[k, U.OVERFLOW]
        seen += sum(cols) - int(tally[k, U.REF])
    assert seen > 100 and tally[:, U.EDGE].sum() > 0


def test_three_sites_inside_a_region_give_the_cells_of_k_cooc():
    b, segs, counts = good_batch()
    e = PRIMERS[0][1]
    region = (e + 10, e + 50)
    # the reads that cover the region and are neither EDGE nor OVERFLOW there: k_cooc counts those too, the table cannot
    keep = []
    for i, s in enumerate(segs):
        tr = U.read_trials(s, G, [region], REF, MQ)
        if tr and tr[0][1] in (None, U.REF):
            keep.append(i)
    sub_b = synth.gather_rows(b, np.array(keep))
    sub_segs = [segs[i] for i in keep]
    w = U.tables(sub_segs, G, [region], REF, MQ)
    condition(sub_segs, [region])
    assert int(w[1][0, U.COVER]) == len(keep) > 300 and any(d[1] == U.KIND_DEL for key in w[0] for d in key[1])
    # three sites: the planted variant, and the two commonest other substitutions of the restatement's table
    tally_sub = {}
    for (k, diffs), (c, r) in w[0].items():
        for off, kind, ln in diffs:
            if kind < 4:
                tally_sub[(region[0] + off, kind)] = tally_sub.get((region[0] + off, kind), 0) + c
    sites = sorted(sorted(tally_sub, key=lambda x: (-tally_sub[x], x))[:3])
    assert len({p for p, _ in sites}) == 3
    eng = fresh(do_trim=False, regions=[region])
    eng.cooc_enable([0, 3], [p for p, _ in sites], [0, 0, 0], [kind for _, kind in sites])
    try:
        eng.process(sub_b)
        table, tally, reads = got(eng)
        assert same((table, tally, reads), w)
        cooc, cooc_reads = eng.cooc_tables()
    finally:
        eng.cooc_disable()
    cells = [0] * 65
    cells[0] = int(tally[0, U.REF])
    for (k, diffs), (c, r) in table.items():
        have = {(region[0] + off, kind) for off, kind, ln in diffs if kind < 4}
        cells[sum(1 << j for j, site in enumerate(sites) if site in have)] += c
    assert cooc[0].tolist() == cells and cells[64] == 0 and sum(1 for c in cells if c) >= 3


# ---- 5. the command line --------------------------------------------------------------------------------------------------------
N_CLI = 1500


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


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """The files of the job -- the mix of batch(1500) as a BAM, the reference, the primers, a region BED given OUT of start
    order -- and what the outputs must show: haplotype.Tables on the restatement's tables on the oracle's trim results."""
    d = tmp_path_factory.mktemp("hap_cli")
    b = batch(N_CLI)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + REF + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), [(s, e, "p%d" % k) for k, (s, e) in enumerate(PRIMERS)])
    rows = [(s, e, "r%d_%d" % (s, e - s)) for s, e in REGIONS]
    rows = rows[len(rows) // 2:] + rows[:len(rows) // 2]
    reg = d / "regions.bed"; reg.write_text("# regions\n" + "".join("SYN_REF\t%d\t%d\t%s\n" % r for r in rows))
    files = dict(ref=str(ref), bed=str(bed), regions=str(reg), bam=write_reads(str(d / "in.bam"), "wb", b, G))
    regions = haplotype.parse_regions(reg.read_text(), "SYN_REF", G)
    assert regions.order != list(range(regions.n)) and sorted(zip(regions.starts.tolist(), regions.ends.tolist())) == REGIONS
    dev_regions = [(int(s), int(e)) for s, e in zip(regions.starts, regions.ends)]
    return files, regions, dev_regions


def tables_for(regions, dev_regions, do_trim, v_min_freq=0.0, min_reads=2, min_freq=0.0):
    w = want(N_CLI, do_trim, regions=dev_regions)
    return haplotype.Tables(regions, REF, U.as_array(w[0]), w[1], w[2], 0, min_reads, min_freq, v_min_freq)


def check_vcf(with_keys, plain, tables):
    """Every record's last two keys are haplotype.Tables' words on the restatement; with the keys and their header lines stripped
    the file is ``plain``.  -> records with HAP_N > 0"""
    text = with_keys.decode()
    assert haplotype.HEADER_LINES in text
    out, hits = [], 0
    for line in text.replace(haplotype.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert kvs[-2].startswith("HAP_N=") and kvs[-1].startswith("HAP=")
            assert ";".join(kvs[-2:]) == tables.info(int(f[1]) - 1, f[3], f[4].split(",")), line
            hits += kvs[-2] != "HAP_N=0"
            f[7] = ";".join(kvs[:-2])
            line = "\t".join(f)
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    return hits


def tsv_of(tables):
    import io
    f = io.StringIO()
    haplotype.write_tsv(f, "SYN_REF", tables)
    return f.getvalue()


def test_aio_with_the_haplotype_flags_and_through_a_device_codec(tmp_path, job, monkeypatch, capfd):
    files, regions, dev_regions = job
    base = lambda tag: ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")), "-ov", str(tmp_path / (tag + ".vcf")),
                        "-oc", str(tmp_path / (tag + ".fas")), "-ml", "30", "-mfv", "0.05"]
    run(monkeypatch, base("plain"))
    capfd.readouterr()
    run(monkeypatch, base("hap") + ["--haplotypes", files["regions"], "--hap_out", str(tmp_path / "hap.tsv.gz"), "--hap_min_reads", "3"])
    log = capfd.readouterr().err
    tables = tables_for(regions, dev_regions, True, v_min_freq=0.05, min_reads=3)
    assert tables.summary_line() in log and "Output haplotype table" in log
    assert read(str(tmp_path / "hap.bam")) == read(str(tmp_path / "plain.bam")) and read(str(tmp_path / "hap.fas")) == read(str(tmp_path / "plain.fas"))
    assert b"HAP" not in read(str(tmp_path / "plain.vcf"))
    assert check_vcf(read(str(tmp_path / "hap.vcf")), read(str(tmp_path / "plain.vcf")), tables) > 3
    text = gzip.open(str(tmp_path / "hap.tsv.gz"), "rt").read()
    assert text == tsv_of(tables)
    lines = [l.split("\t") for l in text.splitlines()[1:]]
    assert list(dict.fromkeys(l[1] for l in lines)) == [name for _, _, name in regions.rows]            # the file's order of regions
    assert sum(l[4] == "ref" for l in lines) == regions.n and len(lines) > regions.n + 10 and all(int(l[5]) >= 3 for l in lines if l[4] != "ref")
    # the same run through the device codec for BAM input and output: identical files (but the BAM, whose blocks it cuts itself)
    capfd.readouterr()
    run(monkeypatch, base("dev") + ["--haplotypes", files["regions"], "--hap_out", str(tmp_path / "dev.tsv"), "--hap_min_reads", "3"], AMPLIPY_GPU_BAM=1, AMPLIPY_GPU_BAM_WRITE=1)
    log = capfd.readouterr().err
    assert "device" in log.lower()
    assert read(str(tmp_path / "dev.vcf")) == read(str(tmp_path / "hap.vcf")) and read(str(tmp_path / "dev.fas")) == read(str(tmp_path / "hap.fas"))
    assert read(str(tmp_path / "dev.tsv")).decode() == text
    # an existing --hap_out is refused like every other output; --hap_out without --haplotypes; --haplotypes on a run that only trims
    for argv in (base("x") + ["--haplotypes", files["regions"], "--hap_out", str(tmp_path / "dev.tsv")],
                 ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "y.vcf"), "--hap_out", str(tmp_path / "y.tsv")],
                 ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "z.bam"), "--haplotypes", files["regions"]]):
        with pytest.raises(SystemExit):
            run(monkeypatch, argv)
    assert read(str(tmp_path / "dev.tsv")).decode() == text


def test_variants_and_consensus_alone_and_the_lost_error(tmp_path, job, monkeypatch):
    files, regions, dev_regions = job
    tables = tables_for(regions, dev_regions, False, v_min_freq=amplipy.DEFAULTS["min_freq_variants"])       # (variants without -mf: the default threshold)
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "hap.vcf"), "--haplotypes", files["regions"], "--hap_out", str(tmp_path / "v.tsv")])
    assert check_vcf(read(str(tmp_path / "hap.vcf")), read(str(tmp_path / "plain.vcf")), tables) > 3
    text = read(str(tmp_path / "v.tsv")).decode()
    assert text == tsv_of(tables)
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "hap.fas"), "--haplotypes", files["regions"], "--hap_out", str(tmp_path / "c.tsv")])
    assert read(str(tmp_path / "hap.fas")) == read(str(tmp_path / "plain.fas")) and read(str(tmp_path / "c.tsv")).decode() == text
    with pytest.raises(RuntimeError) as e:                  # 16 slots for hundreds of haplotypes
        run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "lost.vcf"), "--haplotypes", files["regions"], "--hap_capacity", "4"])
    assert "--hap_capacity" in str(e.value) and "haplotype table was full" in str(e.value)


def test_two_ranks_give_the_one_process_files(tmp_path, job, monkeypatch):
    """Two ranks on one card (tests/rank_worker.py: a child process per rank, gloo, a time limit per child): --hap_out and the
    VCF equal the one-process run byte for byte."""
    from tests.test_gpu_ranks import run_ranks
    files, regions, dev_regions = job
    argv = lambda tag: ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", tag + ".bam", "-ov", tag + ".vcf", "-oc", tag + ".fas", "-ml", "30",
                        "--haplotypes", files["regions"], "--hap_out", tag + ".tsv"]
    monkeypatch.chdir(tmp_path)
    run(monkeypatch, argv("one"))
    status, logs = run_ranks(2, tmp_path, argv("two"), part_bytes=os.path.getsize(files["bam"]) // 4 + 1)
    assert status == [0, 0], logs
    shares = [int(x) for x in re.search(r"records \[(\d+), (\d+)\]", logs[0]).groups()]
    assert sum(shares) == N_CLI and min(shares) > 0
    for ext in (".vcf", ".tsv", ".fas"):
        assert read(str(tmp_path / ("two" + ext))) == read(str(tmp_path / ("one" + ext))), ext
    assert b"HAP_N=1" in read(str(tmp_path / "one.vcf")) or b"HAP_N=2" in read(str(tmp_path / "one.vcf"))
