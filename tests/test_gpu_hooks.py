"""The three opt-in kernels behind the read pass -- the QC report, the strand tallies, the per-amplicon counts (DESIGN.md
section 9c) -- switched on TOGETHER on one engine.  What each computes alone is pinned by test_gpu_qc.py, test_gpu_strand.py and
test_gpu_amplicon.py; here: with all three on, each one's tables are bit for bit what an engine with only that one on gives for
the same batch, and trim results, count table and events are what an engine with none on gives; the three windowed tally
kernels (strand, amplicon, codon) on a batch whose last tile holds one read, with and without trimming; reset zeroes all three and a
disabled one is left out; a trimming pass without its results is refused by the first hook in run order that is on, before
anything ran; every hook's timer answers after a batch and answers ESTATE after an empty one; and, for each of the eight hooks
that keep tables, one life of its state: get before the first enable, add, reset, disable, and the next engine."""
import numpy as np
import pytest

from amplipy_amd import abi, lib
from oracle import oracle
from tests import amplicon_util as A
from tests import strand_util as S

pytestmark = pytest.mark.gpu

HOOKS = ("qc", "strand", "amplicon")          # the run order
MQ, WINDOW, MIN_LENGTH = 20, 4, 60
TRIM_FIELDS = ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")
EVENT_ORDER = ["ref_pos", "read", "q_from", "q_to"]
MESSAGES = {"qc": "the QC report needs new_pos, ref_len, trim_flags and status of a trimming pass",
            "strand": "the strand tallies need new_pos, new_ncig, new_cig and status of a trimming pass",
            "amplicon": "the amplicon tables need new_pos, new_ncig, new_cig and status of a trimming pass"}

_STATE = {}


def state():
    """One engine on the example amplicon set, primers set; the batches, made once."""
    if not _STATE:
        amps, rows = A.example_amps(), A.example_rows()
        primers = sorted((s, e) for s, e, _ in rows)
        eng = lib.Engine(amps.G)
        eng.set_primers(*oracle.find_overlapping_primers(amps.G, primers, 0))
        _STATE.update(amps=amps, primers=primers, eng=eng, batches={})
    return _STATE


def batch(n):
    st = state()
    if n not in st["batches"]:
        st["batches"][n] = S.strand_batch(n, st["amps"].G, st["primers"], 1000 + n)
    return st["batches"][n]


def fresh(on):
    """The engine with trimming and counting on, everything zero, and exactly the hooks ``on`` switched on."""
    st = state()
    eng = st["eng"]
    eng.set_params(MQ, WINDOW, True, True)
    eng.set_kernel_variant(0)
    eng.reset()
    switches = {"qc": (lambda: eng.qc_enable(st["primers"], 0, MIN_LENGTH), eng.qc_disable),
                "strand": (eng.strand_enable, eng.strand_disable),
                "amplicon": (lambda: st["amps"].enable(eng), eng.amplicon_disable)}
    for h in HOOKS:
        switches[h][0 if h in on else 1]()
    return eng


def snap(eng, hook):
    """The hook's tables as they stand, as a tuple of arrays."""
    if hook == "qc":
        t, ps, pe = eng.qc_read_tallies()
        return np.array([t[k] for k in abi.QC_READ_FIELDS], np.uint64), ps, pe
    return eng.strand_tables() if hook == "strand" else eng.amplicon_tables()


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def added(a, b):
    return tuple(x + y for x, y in zip(a, b))


def zero(a):
    return not any(x.any() for x in a)


def last_ms(eng, hook):
    return getattr(eng, hook + "_last_ms")()


def device_batch(b):
    import torch
    from amplipy_amd import synth_torch
    n = b.n
    d = synth_torch.DeviceBatch.from_host(b, "cuda:0")
    out = {k: torch.zeros(max(sz, 1), dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", d.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    return d, out


@pytest.mark.parametrize("n", [257, 1025])
def test_all_three_on_together_give_what_each_gives_alone(n):
    b = batch(n)
    eng = fresh(())
    off = eng.process(b)
    table_off = eng.counts()
    events_off = np.sort(eng.events(), order=EVENT_ORDER)
    alone = {}
    for h in HOOKS:
        eng = fresh((h,))
        eng.process(b)
        alone[h] = snap(eng, h)
        assert not zero(alone[h]), h
    eng = fresh(HOOKS)
    on = eng.process(b)
    for h in HOOKS:
        assert same(snap(eng, h), alone[h]), h
    for k in TRIM_FIELDS:
        assert getattr(on, k).tobytes() == getattr(off, k).tobytes(), k
    assert eng.counts().tobytes() == table_off.tobytes() and table_off.any()
    assert np.array_equal(np.sort(eng.events(), order=EVENT_ORDER), events_off)
    if n >= 1025:
        assert events_off.size > 0


@pytest.mark.parametrize("do_trim", [True, False])
def test_a_last_tile_of_one_read_with_and_without_trimming(do_trim):
    """257 reads: the second tile of the three windowed tally kernels (amp_tally.hpp) holds one live read and 255 lanes past n.
    Strand, amplicon and codon tables against their restatements, on the trimmed alignment and on the original one."""
    from amplipy_amd import codon
    from tests import codon_util as U
    st = state()
    b, amps = batch(257), st["amps"]
    cds = U.overlapping(amps.G)
    eng = fresh(("strand", "amplicon"))
    eng.set_params(MQ, WINDOW, do_trim, True)
    codon.enable(eng, cds)
    try:
        res = eng.process(b)
        assert not res.status.any()
        segs = S.walked_segments(b, res if do_trim else None)
        counts, rev, qsum = S.tables(segs, amps.G, MQ)
        assert np.array_equal(eng.counts(), counts) and counts.any()
        for hook, got, want in (("strand", eng.strand_tables(), (rev, qsum)),
                                ("amplicon", eng.amplicon_tables(), A.tables(b, res, amps, MQ, do_trim)[:2]),
                                ("codon", eng.codon_tables(), U.tables(segs, amps.G, cds.starts, MQ))):
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), hook
    finally:
        eng.codon_disable()


def test_reset_zeroes_all_three_and_a_disabled_hook_is_left_out():
    eng = fresh(HOOKS)
    eng.process(batch(257))
    a = {h: snap(eng, h) for h in HOOKS}
    assert not any(zero(a[h]) for h in HOOKS)
    eng.reset()
    assert all(zero(snap(eng, h)) for h in HOOKS)
    eng.process(batch(1025))
    b = {h: snap(eng, h) for h in HOOKS}
    eng.reset()
    eng.process(batch(257))
    eng.strand_disable()                        # the middle one
    eng.process(batch(1025))
    assert same(snap(eng, "qc"), added(a["qc"], b["qc"]))
    assert same(snap(eng, "strand"), a["strand"])               # readable, and nothing was added
    assert same(snap(eng, "amplicon"), added(a["amplicon"], b["amplicon"]))


def test_a_pass_without_its_results_is_refused_by_the_first_hook_that_is_on():
    eng = fresh(HOOKS)
    eng.process(batch(257))
    table = eng.counts()
    before = {h: snap(eng, h) for h in HOOKS}
    d, out = device_batch(batch(1025))
    for h in HOOKS:
        with pytest.raises(lib.AmpliHipError) as e:
            eng.process_device(d.struct(), 0, None)
        assert e.value.rc == -1 and MESSAGES[h] in str(e.value), h
        assert not any(m in str(e.value) for k, m in MESSAGES.items() if k != h), h
        eng.sync()
        assert np.array_equal(eng.counts(), table), h
        for k in HOOKS:
            assert same(snap(eng, k), before[k]), (h, k)
        assert not any(v.any().item() for v in out.values()), h         # nothing ran
        getattr(eng, h + "_disable")()
    eng.process_device(d.struct(), 0, None)                             # with all three off: as before the hooks existed
    eng.sync()
    assert not np.array_equal(eng.counts(), table)


def test_every_timer_answers_after_a_batch_and_not_after_an_empty_one():
    eng = fresh(HOOKS)
    eng.process(batch(1025))
    for h in HOOKS:
        assert last_ms(eng, h) > 0, h
    eng.process_device(abi.AmpDevReads(), 0, None)                      # no reads: nothing is enqueued, nothing was timed
    eng.sync()
    for h in HOOKS:
        with pytest.raises(lib.AmpliHipError) as e:
            last_ms(eng, h)
        assert e.value.rc == -5, h


# ---- the eight hooks that keep tables: one life of a state, the same for each ---------------------------------------------------
TABLE_HOOKS = ("strand", "amplicon", "codon", "del", "cooc", "errprof", "hap", "readpos")


def table_switches(eng):
    """hook -> (enable on the example set, disable) for ``eng``; the sets and the batch -- batch(257) with its match bases set
    onto a reference, so that the haplotype table gets keys -- are made once."""
    st = state()
    if "ref" not in st:
        from tests import codon_util, cooc_util, hap_util
        G = st["amps"].G
        ref = hap_util.reference(G, seed=3)
        st.update(ref=ref, cds=codon_util.overlapping(G), sets=cooc_util.mixed_sets(G), regions=hap_util.regions_near(st["primers"][:40], G),
                  on_ref=hap_util.onto_reference(batch(257), ref, 5, rate=0.01, low_rate=0.02))
    regions = st["regions"]
    return {"strand": (eng.strand_enable, eng.strand_disable),
            "amplicon": (lambda: st["amps"].enable(eng), eng.amplicon_disable),
            "codon": (lambda: eng.codon_enable(st["cds"].starts), eng.codon_disable),
            "del": (eng.del_enable, eng.del_disable),
            "cooc": (lambda: eng.cooc_enable(*st["sets"].arrays()), eng.cooc_disable),
            "errprof": (lambda: eng.errprof_enable(st["ref"]), eng.errprof_disable),
            "hap": (lambda: eng.hap_enable([s for s, _ in regions], [e for _, e in regions], st["ref"]), eng.hap_disable),
            "readpos": (eng.readpos_enable, eng.readpos_disable)}


def tables_of(eng, hook):
    """-> (the hook's arrays that add element-wise, its keyed records or None)"""
    if hook == "del":
        return (), eng.del_events()[0]
    if hook == "hap":
        ev, _, tally, reads = eng.hap_tables()
        return (tally, reads), ev
    t = getattr(eng, hook + "_tables")()
    return (t if isinstance(t, tuple) else (t,)), None


def same_tables(a, b):
    return same(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or a[1].tobytes() == b[1].tobytes())


def another_engine():
    st = state()
    e = lib.Engine(st["amps"].G)
    e.set_primers(*oracle.find_overlapping_primers(st["amps"].G, st["primers"], 0))
    e.set_params(MQ, WINDOW, True, True)
    return e


@pytest.mark.parametrize("hook", TABLE_HOOKS)
def test_a_hook_s_tables_from_before_the_first_enable_to_the_next_engine(hook):
    """Two tiles, the second with one live read.  Before the first enable a get answers ESTATE; after a batch every table holds
    something; adding the tables just got doubles every cell, and every count and rev of a keyed table; reset zeroes them; a
    disabled hook's tables stay readable and a further batch leaves them alone; an engine closed with every hook on takes
    nothing with it: the next engine's tables are the first one's."""
    other = another_engine()
    with pytest.raises(lib.AmpliHipError) as e:
        tables_of(other, hook)
    assert e.value.rc == -5
    eng = fresh(())
    sw = table_switches(eng)
    b = state()["on_ref"]
    for h in TABLE_HOOKS:
        sw[h][1]()
    sw[hook][0]()
    try:
        eng.process(b)
        once = tables_of(eng, hook)
        assert all(x.any() for x in once[0]) and (once[1] is None or (once[1].size > 0 and once[1]["count"].all()))
        if hook == "del":
            eng.del_add(once[1])
        elif hook == "hap":
            eng.hap_add(once[1], *once[0])
        else:
            getattr(eng, hook + "_add")(*once[0])
        twice = tables_of(eng, hook)
        assert same(twice[0], added(once[0], once[0]))
        if once[1] is not None:
            want = once[1].copy()
            want["count"] *= 2; want["rev"] *= 2
            assert twice[1].tobytes() == want.tobytes()
        eng.reset()
        cleared = tables_of(eng, hook)
        assert zero(cleared[0]) and (cleared[1] is None or cleared[1].size == 0)
        eng.process(b)
        assert same_tables(tables_of(eng, hook), once)
        sw[hook][1]()
        eng.process(b)
        assert same_tables(tables_of(eng, hook), once)
    finally:
        sw[hook][1]()
    sw_other = table_switches(other)
    other.qc_enable(state()["primers"], 0, MIN_LENGTH)
    for h in TABLE_HOOKS:
        sw_other[h][0]()
    other.process(b)
    assert same_tables(tables_of(other, hook), once)
    other.close()                               # ... with all nine states alive
    other = another_engine()
    table_switches(other)[hook][0]()
    other.process(b)
    assert same_tables(tables_of(other, hook), once)
    other.close()
