"""The insertion-event chain on the device -- the read kernels' event list in eight shard regions, amp_aggregate_ins_events
(k_ins_hash, two radix sorts, k_ins_poskey, k_ins_heads, the scan, k_ins_runs: amp_ins.hip), amp_event_strings and
readloop._store_events -- against the plain tally of tests/ins_util.py over the CPU oracle's events: crafted allele shapes on
every read kernel at event counts around the 256-thread grid edges, lists with unused slots, batches in sequence with and
without drain and with read ids that wrap, the overflow report, and the call order.  Integers and text: the bar is equality.

No event reaches amp_event_strings or the aggregation before ins_util.assert_in_batch has held its read id and query range
against the batch: those calls hold q_to against nothing on the device."""
from collections import Counter

import numpy as np
import pytest

from amplipy_amd import lib, readloop, synth
from amplipy_amd.batch import ReadBatch
from amplipy_amd.insertions import EventStore
from tests import ins_util as U
from tests.gpu_util import EV_ORDER

pytestmark = pytest.mark.gpu

G = 2000
VARIANTS = [None, 7, 6, 4, 5, 2, 1, 3]
VARIANT_IDS = ["default", "fast_kernel_v7", "fast_kernel_v6", "fast_kernel", "fast_kernel_v5", "tile_kernel", "lane_kernel", "split_pipeline"]


class Dev:
    """An Engine without primers at ins_util.MQ / W whose table is a torch tensor, so that ins_at -- the events per position,
    the seventh column block behind the six count columns -- can be read."""

    def __init__(self, ref_len, variant=None):
        import torch
        self.torch = torch
        self.ref_len = ref_len
        self.table = torch.zeros(ref_len * 7, dtype=torch.int32, device="cuda:0")
        self.e = lib.Engine(ref_len)
        self.e.bind_counts(self.table.data_ptr())
        if variant is not None:
            self.e.set_kernel_variant(variant)
        self.e.set_primers(*U.no_primers(ref_len))
        self.e.set_params(U.MQ, U.W, True, True)

    def ins_at(self):
        self.e.sync()
        self.torch.cuda.synchronize()
        return self.table.cpu().numpy().view(np.uint32)[self.ref_len * 6:].copy()

    def close(self):
        self.e.close()


def sorted_events(ev):
    return np.sort(ev, order=EV_ORDER)


def check_list(dev, batch, want_events, read_base, ins_at_want, drain=False):
    """The device list against the oracle's events of the batch that is staged: events() sorted equal them; the runs summed by
    text equal their tally, one run per allele, ordered by (ref_pos, length), reserved 0, every representative an event of the
    list; per position, the summed run counts equal the oracle's; ins_at equals ``ins_at_want``.  -> (slots in use, events)."""
    e = dev.e
    n_slots = U.slots_in_use(e)
    ev = e.events()
    assert n_slots >= ev.size
    U.assert_in_batch(batch, ev, read_base)
    assert np.array_equal(sorted_events(ev), sorted_events(want_events)), "events() differs from the oracle's list"
    want = U.tally(batch, want_events, read_base)
    runs = e.aggregate_events(read_base=read_base, drain=drain)
    U.assert_in_batch(batch, U.run_rows(runs), read_base)
    U.check_runs(runs, batch, read_base, want, ev)                      # text on the host from the representatives
    assert runs.size == len(want), "one run per distinct allele"
    assert U._runs_as_counter(e, runs, read_base & 0xFFFFFFFF) == want               # text from the device
    per_pos = np.zeros(dev.ref_len, np.uint32)
    np.add.at(per_pos, runs["ref_pos"].astype(np.int64), runs["count"])
    assert np.array_equal(per_pos, U.per_position(want_events, dev.ref_len))
    assert np.array_equal(dev.ins_at(), ins_at_want)
    if drain:
        assert e.events().size == 0 and U.slots_in_use(e) == 0
    return n_slots, ev.size


@pytest.fixture(scope="module")
def edge_cases():
    """[(name, batch, oracle result)]: event counts 1, 255, 256, 257 and 2049, few alleles many times and all alleles distinct."""
    return [("%d %s" % (n, kind),) + U.batch_with_events(n, kind, G) for n in U.EVENT_COUNTS for kind in ("copies", "distinct")]


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_crafted_alleles_on_every_read_kernel(variant, edge_cases):
    """The crafted shapes (ins_util.crafted_segments: the empty allele, SEQ[a:None], position 0, a low quality inside the
    insertion, odd and even nibbles, IUPAC, lower case, the anchoring base, 200 bases, ...) with filler so that the list holds
    1, 255, 256, 257 and 2049 events.  The read with the trailing insertion stays in the batch: it has a status and no event."""
    dev = Dev(G, variant)
    try:
        for name, b, a in edge_cases:
            dev.e.reset()
            res = dev.e.process(b)
            assert np.array_equal(res.status, a.trim.status), name
            check_list(dev, b, a.events, 0, U.per_position(a.events, G))
            assert dev.e.error_reads() == int((a.trim.status != 0).sum()), name
    finally:
        dev.close()


def _status_zero(segs, ref_len):
    """The reads the reference accepts, by position -> (batch, oracle result)."""
    segs = sorted(segs, key=lambda s: s.reference_start)
    b = ReadBatch.from_segments(segs)
    a = U.oracle_events(b, ref_len)
    keep = np.nonzero(a.trim.status == 0)[0]
    if keep.size != b.n:
        b = ReadBatch.from_segments([segs[i] for i in keep])
        a = U.oracle_events(b, ref_len)
    assert not a.trim.status.any()
    return b, a


def test_unused_slots_are_really_present():
    """Lists with slots that were reserved and not used (ref_pos = -1: the granules of the many-op kernel and of the fast
    kernels, the slices of reads with very long CIGARs) between real events: 300 many-op reads, the shape that goes through
    k_long, and 2,000 reads of the mixed pool.  The same equalities; and the size query must have exceeded the exact count on
    one of the two at least (the many-op list: some 390,000 slots for 596 events), or this test no longer covers the -1 path."""
    from tests.test_gpu_parity import _long_read_segments
    g = synth.make_genome()
    _, amps = synth.make_artic_scheme()
    shapes = [("many ops", _long_read_segments(np.random.default_rng(120), 300, 60_000, 9000, 120), 60_000),
              ("mixed pool", synth.make_mixed_segments(g, amps, 2000, seed=3), int(g.size))]
    exceeded = {}
    for name, segs, ref_len in shapes:
        b, a = _status_zero(segs, ref_len)
        assert a.events.size > 100, name
        dev = Dev(ref_len)
        try:
            dev.e.process(b, read_base=7)
            a7 = U.oracle_events(b, ref_len, 7)
            n_slots, n_events = check_list(dev, b, a7.events, 7, U.per_position(a.events, ref_len))
            exceeded[name] = n_slots > n_events
            print("%s: %d slots in use, %d events" % (name, n_slots, n_events))
        finally:
            dev.close()
    assert exceeded["many ops"] or exceeded["mixed pool"], "no unused slot in either list: the -1 path is not covered"


@pytest.fixture(scope="module")
def slices():
    """Four batches in sequence: a handful of events, a few hundred, thousands, the crafted shapes.  [(batch, read_base, oracle
    result with that read_base)]."""
    rng = np.random.default_rng(8)
    parts = [U.distinct_segments(5, first=4000) + U.plain_segments(20, rng, G),
             U.copies_segments(300) + U.plain_segments(100, rng, G),
             U.distinct_segments(3000) + U.copies_segments(500, pos=300),
             [s for n, s in U.crafted_segments() if n != U.TRAILING] + U.copies_segments(50)]
    out, base = [], 2 ** 32 - 200                     # the ids wrap in the second batch
    for segs in parts:
        segs = [segs[i] for i in rng.permutation(len(segs))]
        b = ReadBatch.from_segments(segs)
        a = U.oracle_events(b, G, base)
        assert not a.trim.status.any()
        out.append((b, base, a))
        base += b.n
    assert out[0][2].events.size == 5 and out[2][2].events.size == 3500
    return out


def test_batches_without_drain(slices):
    """The list grows while it holds events (the first batch sizes it for a handful, the third brings thousands: grow_events
    lays the eight regions out again): events() is the union of the oracle's lists, ins_at their sum."""
    dev = Dev(G)
    try:
        union, ins_at = [], np.zeros(G, np.uint32)
        for b, base, a in slices:
            dev.e.process(b, read_base=base)
            union.append(a.events); ins_at += U.per_position(a.events, G)
            ev = dev.e.events()
            assert np.array_equal(sorted_events(ev), sorted_events(np.concatenate(union)))
            assert np.array_equal(dev.ins_at(), ins_at)
        assert dev.e.error_reads() == 0
    finally:
        dev.close()


def test_reservation_grows_under_a_full_shard(slices):
    """grow_events with a region that is more than half full: the smallest power of two that amp_reserve_events can be given
    for the 3,500-event batch without AMP_EOVERFLOW (so the fullest shard holds more than half of it), then a reservation four
    times as large while the events are in the list -- every region is copied whole to its new place -- then one more batch.
    A copy that is too short, or lands at the old stride, loses events here; in test_batches_without_drain the regions are
    sized by the library with room to spare and hold their events in their first few hundred slots."""
    b, base, a = slices[2]
    cap = 64
    while True:
        dev = Dev(G)
        dev.e.reserve_events(cap)
        dev.e.process(b, read_base=base)
        try:
            ev = dev.e.events()
            break
        except lib.AmpliHipError as err:
            assert "AMP_EOVERFLOW" in str(err)
            dev.close()
            cap *= 2
            assert cap <= 1 << 16, "3,500 events and the kernels' granules fit 65,536 slots a shard"
    try:
        assert cap > 64 and np.array_equal(sorted_events(ev), sorted_events(a.events))
        dev.e.reserve_events(4 * cap)
        assert np.array_equal(sorted_events(dev.e.events()), sorted_events(a.events))
        b2, base2, a2 = slices[3]
        dev.e.process(b2, read_base=base2)
        assert np.array_equal(sorted_events(dev.e.events()), sorted_events(np.concatenate([a.events, a2.events])))
        assert np.array_equal(dev.ins_at(), U.per_position(a.events, G) + U.per_position(a2.events, G))
    finally:
        dev.close()


def test_batches_with_drain(slices):
    """aggregate_events(drain=True) behind every batch: each batch's tally is exact -- nothing of the batch before is seen, whose
    slots still hold its events -- the list is empty after each drain, ins_at keeps adding up."""
    dev = Dev(G)
    try:
        ins_at = np.zeros(G, np.uint32)
        for b, base, a in slices:
            dev.e.process(b, read_base=base)
            ins_at += U.per_position(a.events, G)
            check_list(dev, b, a.events, base, ins_at, drain=True)
    finally:
        dev.close()


def test_read_base_near_2_32():
    """read_base = 2^32 - 3 on a 10-read batch: the ids wrap inside it.  readloop._store_events (aggregation, text of the
    representatives, drain) gives the tally, and amp_event_strings takes the ids modulo 2^32 like the aggregation."""
    base = 2 ** 32 - 3
    segs = [s for n, s in U.crafted_segments() if n in ("TT", "TTT", "anchor A", "anchor C", "lower case", "to the read's end")] + U.distinct_segments(4)
    b = ReadBatch.from_segments(segs)
    a = U.oracle_events(b, G, base)
    assert b.n == 10 and sorted(set(a.events["read"].tolist())) == sorted((base + i) & 0xFFFFFFFF for i in range(10))
    want = U.tally(b, a.events, base)
    dev = Dev(G)
    try:
        dev.e.process(b, read_base=base)
        ev = dev.e.events()
        U.assert_in_batch(b, ev, base)
        assert np.array_equal(sorted_events(ev), sorted_events(a.events))
        length, blob = dev.e.event_text(ev, read_base=base)                 # ids as recorded, not rebased by the caller
        raw = blob.tobytes(); off = np.cumsum(length) - length
        got = [(int(p), raw[int(o):int(o) + int(n)].decode("ascii")) for p, o, n in zip(ev["ref_pos"], off, length)]
        assert got == U.pairs(b, ev, base)
        store = EventStore()
        readloop._store_events(dev.e, store, base)
        assert Counter(store.pairs()) == want and len(store) == a.events.size
        assert dev.e.events().size == 0
        assert np.array_equal(dev.ins_at(), U.per_position(a.events, G))
    finally:
        dev.close()


def test_overflow_is_reported_and_nothing_else_is_hurt():
    """amp_reserve_events with too little room (8 slots per shard), then 4,096 reads with one insertion each: the event list and
    the aggregation answer AMP_EOVERFLOW; the count table and ins_at are exact (every store of an event is guarded by the
    capacity, the tally is added to whether or not the slot fits); no read has a status.  After reset() and a reservation
    that holds -- per shard, what launch_reads asks for: twice the batch's bound of 6 events a read, plus 64 slots per wave of
    the fast kernel (8 per CU) and of the many-op kernel (24 per CU) -- the same batch aggregates exactly."""
    rng = np.random.default_rng(12)
    segs = U.distinct_segments(2048) + U.copies_segments(2048)
    segs = [segs[i] for i in rng.permutation(len(segs))]
    b = ReadBatch.from_segments(segs)
    a = U.oracle_events(b, G)
    assert b.n == 4096 and a.events.size == 4096 and not a.trim.status.any()
    dev = Dev(G)
    try:
        dev.e.reserve_events(8)
        dev.e.process(b)
        with pytest.raises(lib.AmpliHipError, match="AMP_EOVERFLOW"):
            dev.e.events()
        with pytest.raises(lib.AmpliHipError, match="AMP_EOVERFLOW"):
            dev.e.aggregate_events()
        assert np.array_equal(dev.e.counts(), a.counts)
        assert np.array_equal(dev.ins_at(), U.per_position(a.events, G))
        assert dev.e.error_reads() == 0
        dev.e.reset()
        dev.e.reserve_events(2 * 6 * b.n + 64 * (8 + 24) * 256)
        dev.e.process(b)
        check_list(dev, b, a.events, 0, U.per_position(a.events, G))
        assert np.array_equal(dev.e.counts(), a.counts)
    finally:
        dev.close()


def test_aggregation_needs_a_batch_and_reset_empties_the_list():
    """On a ctx that has taken no batch amp_aggregate_ins_events with reads == NULL answers AMP_ESTATE, already to the size query
    (include/amplihip.h), as amp_event_strings does.  After reset() the list is empty and a new batch aggregates exactly."""
    dev = Dev(G)
    try:
        with pytest.raises(lib.AmpliHipError, match="AMP_ESTATE"):
            dev.e.aggregate_events()
        assert dev.e.events().size == 0
        b, a = U.batch_with_events(257, "copies", G)
        dev.e.process(b)
        check_list(dev, b, a.events, 0, U.per_position(a.events, G))
        dev.e.reset()
        assert dev.e.events().size == 0 and U.slots_in_use(dev.e) == 0 and dev.e.aggregate_events().size == 0
        assert not dev.ins_at().any()
        b2, a2 = U.batch_with_events(256, "distinct", G)
        dev.e.process(b2)
        check_list(dev, b2, a2.events, 0, U.per_position(a2.events, G))
    finally:
        dev.close()
