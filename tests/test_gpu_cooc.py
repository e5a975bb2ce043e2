"""k_cooc on the device (amplipy_amd/csrc/amp_cooc.hip) against the plain restatement in
tests/cooc_util.py, which tests/test_cooc_twin.py pins to the oracle's count table: the table on the device's own trim results at
sizes round the tile, sorted and shuffled, on overlapping, nested and shared sets; the crafted reads; the bit order; a pile; set
lists longer than the window; the state of the hook; every read kernel; device batches; the refusal; all six hooks together; and
the command line on a synthetic job that carries a linked double substitution, two unlinked ones and an in-frame deletion."""
import gzip
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, codon, cooc, lib, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import amplicon_util as A
from tests import codon_util as CU
from tests import cooc_util as U
from tests import strand_util as S

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
MQ, WINDOW = 20, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "amplipy_amd", "csrc", "amp_cooc.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


W = header_constant("CO_W")


def enable(eng, sets):
    eng.cooc_enable(*sets.arrays())


class PrimerSet:
    """One primer set: its engine and, per batch, the oracle's results, computed once."""

    def __init__(self, name):
        self.name = name
        if name == "example":
            self.rows = A.example_rows()
            self.G = 29903
        else:
            self.rows = [(100, 130, "l"), (400, 430, "r")]
            self.G = 2000
        self.primers = sorted((s, e) for s, e, _ in self.rows)
        self.tabs = oracle.find_overlapping_primers(self.G, self.primers, 0)
        self.sets = U.mixed_sets(self.G)
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(*self.tabs)
        self.batches, self.oracles = {}, {}

    def batch(self, n, seed=None):
        key = (n, seed)
        if key not in self.batches:
            self.batches[key] = S.strand_batch(n, self.G, self.primers, 2000 + n if seed is None else seed)
        return self.batches[key]

    def oracle(self, n, seed=None, mq=MQ, do_trim=True):
        key = (n, seed, mq, do_trim)
        if key not in self.oracles:
            r = oracle.process(self.batch(n, seed), self.G, *self.tabs, mq, WINDOW, do_trim=do_trim, do_count=True)
            assert not r.trim.status.any()
            r.counts.setflags(write=False)
            self.oracles[key] = r
        return self.oracles[key]

    def fresh(self, mq=MQ, do_trim=True, variant=0, sets=None):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(variant)
        self.eng.reset()
        enable(self.eng, sets or self.sets)
        return self.eng


_SETS = {}


def get_set(name):
    if name not in _SETS:
        _SETS[name] = PrimerSet(name)
    return _SETS[name]


@pytest.fixture(params=["one", "example"])
def pset(request):
    return get_set(request.param)


def want_tables(batch, res, G, sets, mq, do_trim):
    return U.tables(S.walked_segments(batch, res if do_trim else None), G, sets, mq)


def run_and_check(eng, batch, G, sets, oracle_counts, mq=MQ, do_trim=True, what=""):
    """One batch through the engine: the count table is the oracle's, the co-occurrence table is the restatement's on the
    device's own trim results.  -> (cooc, reads)."""
    res = eng.process(batch)
    assert np.array_equal(eng.counts(), oracle_counts), what
    want_c, want_r = want_tables(batch, res, G, sets, mq, do_trim)
    got_c, got_r = eng.cooc_tables()
    assert np.array_equal(got_r, want_r), what
    assert np.array_equal(got_c, want_c), what
    assert int(got_r.sum()) == batch.n - int((res.status != 0).sum())
    return got_c, got_r


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(pset, n, order):
    batch = pset.batch(n)
    if order == "shuffled" and n > 1:
        batch = synth.gather_rows(batch, np.random.default_rng(5).permutation(batch.n))
        assert n < 63 or (np.diff(batch.pos) < 0).any()
    eng = pset.fresh()
    c, r = run_and_check(eng, batch, pset.G, pset.sets, pset.oracle(n).counts, what=(pset.name, n, order))
    if n >= 1025:
        assert c[:, :64].any() and c[:, U.PARTIAL].any()
    if n:
        assert eng.cooc_last_ms() > 0


def test_single_site_sets_give_the_count_table():
    """The pin to the oracle on the device: single-site sets over the whole of the short reference."""
    s = get_set("one")
    sets = U.single_sites(0, s.G)
    eng = s.fresh(sets=sets)
    batch = s.batch(1025)
    res = eng.process(batch)
    c, r = eng.cooc_tables()
    segs = S.walked_segments(batch, res)
    U.check_single_sites(c, 0, s.G, s.oracle(1025).counts, U.all_regular(segs, s.G))
    assert int(r[1]) == sum(not CU.is_regular(x, s.G) for x in segs)


# ---- 2. crafted reads -----------------------------------------------------------------------------------------------------------
_EDGE = {}


def run_crafted(segs, sets, mq=MQ, do_trim=False, variant=0):
    G = U.CRAFT_G
    batch = ReadBatch.from_segments(segs)
    tabs = oracle.find_overlapping_primers(G, U.CRAFT_PRIMERS, 0)
    r = oracle.process(batch, G, *(tabs if do_trim else (None, None, 0)), mq, WINDOW, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    if G not in _EDGE:
        _EDGE[G] = lib.Engine(G)
        _EDGE[G].set_primers(*tabs)
    eng = _EDGE[G]
    eng.set_params(mq, WINDOW, do_trim, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    enable(eng, sets)
    out = run_and_check(eng, batch, G, sets, r.counts, mq=mq, do_trim=do_trim)
    eng.set_kernel_variant(0)
    return out


_CRAFTED = U.crafted()


@pytest.mark.parametrize("case", _CRAFTED, ids=[c[0] for c in _CRAFTED])
def test_crafted_reads(case):
    name, sets, segs, mq, do_trim, expect = case
    c, r = run_crafted(segs, sets, mq=mq, do_trim=do_trim)
    expect(c, r, sets)


# ---- 3. bit order, 4. pile -----------------------------------------------------------------------------------------------------
def test_bit_order():
    sets, segs = U.bit_order_case()
    c, r = run_crafted(segs, sets)
    assert c[0, :64].tolist() == list(range(1, 65)) and c[0, U.PARTIAL] == 0 and list(r) == [2080, 0]


def test_pile_of_identical_reads_is_counted_exactly():
    sets, segs = U.pile_case()
    c, r = run_crafted(segs, sets)
    assert c[0, 3] == 4096 and c[1, 3] == 3072 and c[1, 1] == 1024 and int(c.sum()) == 8192 and list(r) == [8192, 0]


# ---- 5. window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_more_sets_than_the_window_holds(pset, order):
    sets = U.many_sets(3 * W + 1, pset.G)
    assert sets.n_sets == 3 * W + 1
    batch = pset.batch(1025)
    if order == "shuffled":
        batch = synth.gather_rows(batch, np.random.default_rng(6).permutation(batch.n))
    eng = pset.fresh(sets=sets)
    c, r = run_and_check(eng, batch, pset.G, sets, pset.oracle(1025).counts)
    assert c.any()


# ---- 6. state -------------------------------------------------------------------------------------------------------------------
def test_tables_accumulate_reset_merge_and_follow_the_set_list():
    s = get_set("example")
    eng = s.fresh()
    res_a = eng.process(s.batch(257))
    res_b = eng.process(s.batch(1025))
    ta = want_tables(s.batch(257), res_a, s.G, s.sets, MQ, True)
    tb = want_tables(s.batch(1025), res_b, s.G, s.sets, MQ, True)
    c, r = eng.cooc_tables()
    assert np.array_equal(c, ta[0] + tb[0]) and np.array_equal(r, ta[1] + tb[1])
    eng.reset()
    c, r = eng.cooc_tables()
    assert not c.any() and not r.any()
    eng.process(s.batch(257))
    eng.cooc_disable()
    eng.process(s.batch(1025))
    c, r = eng.cooc_tables()                                    # what was tallied stays readable, nothing was added
    assert np.array_equal(c, ta[0]) and np.array_equal(r, ta[1])
    big = np.array([2 ** 40 + 5, 0], np.uint64)
    eng.cooc_add(tb[0], tb[1] + big)                            # another rank's tables, a read count beyond 32 bits
    c, r = eng.cooc_tables()
    assert np.array_equal(c, ta[0] + tb[0]) and np.array_equal(r, ta[1] + tb[1] + big)
    enable(eng, s.sets)                                         # on again: the tables start at zero
    c, r = eng.cooc_tables()
    assert not c.any() and not r.any()
    # two half-batches merged by cooc_add are the whole batch
    whole = s.batch(1025)
    halves = [synth.gather_rows(whole, np.arange(0, 512)), synth.gather_rows(whole, np.arange(512, 1025))]
    eng.process(halves[0])
    first = eng.cooc_tables()
    eng.reset()
    eng.process(halves[1])
    eng.cooc_add(*first)
    c, r = eng.cooc_tables()
    assert np.array_equal(c, tb[0]) and np.array_equal(r, tb[1])
    # another set list on an engine that had one: the tables are laid out again
    other = U.many_sets(7, s.G)
    enable(eng, other)
    res = eng.process(s.batch(257))
    want = want_tables(s.batch(257), res, s.G, other, MQ, True)
    c, r = eng.cooc_tables()
    assert c.shape[0] == 7 and np.array_equal(c, want[0]) and np.array_equal(r, want[1])


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.cooc_disable()
    off = eng.process(batch)
    table_off = eng.counts()
    events_off = np.sort(eng.events(), order=["ref_pos", "read", "q_from", "q_to"])
    never = lib.Engine(s.G)                                     # an engine that never had the hook
    never.set_primers(*s.tabs)
    never.set_params(MQ, WINDOW, True, True)
    clean = never.process(batch)
    assert never.counts().tobytes() == table_off.tobytes()
    never.close()
    eng = s.fresh()
    on = eng.process(batch)
    for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status"):
        assert getattr(on, k).tobytes() == getattr(off, k).tobytes(), k
        if k != "new_cig":
            assert getattr(clean, k).tobytes() == getattr(off, k).tobytes(), k
    # (new_cig has three spare words per read that no kernel writes: another engine's buffer is held to the ops alone)
    assert all(clean.cigar_ops(i) == off.cigar_ops(i) for i in range(batch.n))
    assert eng.counts().tobytes() == table_off.tobytes()
    assert np.array_equal(np.sort(eng.events(), order=["ref_pos", "read", "q_from", "q_to"]), events_off)
    assert events_off.size > 0


def test_tables_before_the_first_enable_and_bad_sets_are_errors():
    e = lib.Engine(500)
    with pytest.raises(lib.AmpliHipError) as err:
        e.cooc_tables()
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError):
        e.cooc_last_ms()
    with pytest.raises(lib.AmpliHipError) as err:
        e.cooc_add(np.zeros(0, np.uint32), np.zeros(2, np.uint64))
    assert err.value.rc == -5
    e.cooc_disable()            # off while off: nothing to do
    sub, dele = U.sub, U.dele
    bad = [[[sub(10, "A")], [sub(9, "A")]],                     # sets not sorted by first site
           [[sub(10, "A"), sub(10, "C")]],                      # two sites at one position
           [[dele(10, 3), sub(12, "A")]],                       # a site inside a deletion site
           [[sub(500, "A")]], [[dele(498, 3)]], [[sub(-1, "A")]],       # outside the reference
           [[sub(k, "A") for k in range(7)]]]                   # seven sites
    for sets in bad:
        off = np.cumsum([0] + [len(x) for x in sets]).astype(np.int32)
        flat = [site for x in sets for site in x]               # (as given: no sorting helper in between)
        with pytest.raises(lib.AmpliHipError) as err:
            e.cooc_enable(off, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat])
        assert err.value.rc == -1, sets
    with pytest.raises(lib.AmpliHipError) as err:               # an empty set
        e.cooc_enable([0, 0, 1], [5], [0], [0])
    assert err.value.rc == -1
    with pytest.raises(lib.AmpliHipError) as err:               # a base that is none of A C G T
        e.cooc_enable([0, 1], [5], [0], [4])
    assert err.value.rc == -1
    e.cooc_enable([0, 1, 3], [0, 0, 499], [0, 0, 0], [0, 1, 3])         # equal first sites, the last base of the reference
    e.close()
    big = lib.Engine(abi.COOC_MAX_SPAN + 100)
    with pytest.raises(lib.AmpliHipError) as err:               # a span above the limit
        big.cooc_enable([0, 2], [0, abi.COOC_MAX_SPAN + 1], [0, 0], [0, 0])
    assert err.value.rc == -1
    big.cooc_enable([0, 2], [0, abi.COOC_MAX_SPAN], [0, 0], [0, 0])
    n = abi.COOC_MAX_SETS + 1
    with pytest.raises(lib.AmpliHipError) as err:               # one set more than 2^16
        big.cooc_enable(np.arange(n + 1), np.arange(n), np.zeros(n), np.zeros(n))
    assert err.value.rc == -1
    big.close()


# ---- 7. every read kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 4, 5, 7, 2])
def test_every_read_kernel_feeds_the_same_table(variant):
    s = get_set("example")
    eng = s.fresh(variant=variant)
    run_and_check(eng, s.batch(1025), s.G, s.sets, s.oracle(1025).counts, what=variant)
    eng.set_kernel_variant(0)


# ---- 8. device batches, the refusal, all hooks ----------------------------------------------------------------------------------
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
    want = eng.cooc_tables()
    assert np.array_equal(want[0], want_tables(s.batch(1025), res, s.G, s.sets, MQ, True)[0])
    b, out = _device_batch(s.batch(1025))
    for drop in ((), ("ref_len", "trim_flags")):                # the hook needs neither ref_len nor trim_flags
        eng.reset()
        eng.process_device(b.struct(), 0, _dev_out(out, drop=drop))
        eng.sync()
        got = eng.cooc_tables()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_trimming_pass_without_new_cig_is_refused_before_it_runs():
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before, tables_before = eng.counts(), eng.cooc_tables()
    b, out = _device_batch(s.batch(1025))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, _dev_out(out, drop=("new_cig",)))
    assert e.value.rc == -1 and "the co-occurrence tallies need" in str(e.value)
    eng.sync()
    after = eng.cooc_tables()
    assert np.array_equal(eng.counts(), before) and np.array_equal(after[0], tables_before[0]) and np.array_equal(after[1], tables_before[1])
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.cooc_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the hook existed
    eng.sync()


def test_all_six_hooks_together_give_what_each_gives_alone():
    s = get_set("example")
    amps = A.example_amps()
    batch = s.batch(1025)
    regions = [(0, s.G), (1000, 2000)]
    cds = CU.overlapping(s.G)

    def engine(qc=False, strand=False, amplicon=False, cod=False, dele=False, co=False):
        eng = lib.Engine(s.G)
        eng.set_primers(*s.tabs)
        eng.set_params(MQ, WINDOW, True, True)
        if qc:
            eng.qc_enable(s.primers, 0, 30, False, regions, [1, 10, 100])
        if strand:
            eng.strand_enable()
        if amplicon:
            amps.enable(eng)
        if cod:
            codon.enable(eng, cds)
        if dele:
            eng.del_enable()
        if co:
            enable(eng, s.sets)
        eng.process(batch)
        return eng

    every = engine(True, True, True, True, True, True)
    alone = engine(qc=True)
    a, b = every.qc_read_tallies(), alone.qc_read_tallies()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    alone.close()
    alone = engine(strand=True)
    assert all(np.array_equal(x, y) for x, y in zip(every.strand_tables(), alone.strand_tables()))
    alone.close()
    alone = engine(amplicon=True)
    assert all(np.array_equal(x, y) for x, y in zip(every.amplicon_tables(), alone.amplicon_tables()))
    alone.close()
    alone = engine(cod=True)
    assert all(np.array_equal(x, y) for x, y in zip(every.codon_tables(), alone.codon_tables()))
    alone.close()
    alone = engine(dele=True)
    assert np.array_equal(every.del_events()[0], alone.del_events()[0]) and alone.del_events()[0].size > 0
    alone.close()
    alone = engine(co=True)
    assert all(np.array_equal(x, y) for x, y in zip(every.cooc_tables(), alone.cooc_tables()))
    assert every.cooc_tables()[0].any() and np.array_equal(every.counts(), alone.counts())
    alone.close()
    every.close()


# ---- 9. command line ------------------------------------------------------------------------------------------------------------
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST")
CLI_MIN_LENGTH = 30


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
    return build_job(tmp_path_factory.mktemp("cooc_cli"))


def build_job(d):
    """The files of the job (the synthetic job of the codon tests) and what the outputs must show: cooc.Tables on the
    restatement on the oracle's trim results."""
    j = CU.synthetic_job()
    g, batch = j["genome"], j["batch"]
    G = int(g.size)
    ref_seq = synth.genome_string(g)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + ref_seq + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), j["primers"])
    pa, pb, pc = j["pa"], j["pb"], j["pc"]
    one = lambda p: p + 1                                       # the file is 1-based
    far = pa + 20000 if pa + 20000 < G else 50                  # a set no read of the job reaches
    text = ("# name <tab> mutations, 1-based\n"
            "linked\tC%dA,G%dA\n" % (one(pa), one(pa + 1)) +
            "unlinked\tG%dA,C%dA\t# given out of order\n" % (one(pb + 1), one(pb)) +
            "del_and_sub\tdel%d-%d,C%dA\n" % (one(pc), one(pc + 2), one(pa)) +
            "nowhere\t%s%d%s\n" % (ref_seq[far], one(far), "A" if ref_seq[far] != "A" else "C"))
    sets_fn = d / "sets.tsv"; sets_fn.write_text(text)
    files = dict(ref=str(ref), bed=str(bed), sets=str(sets_fn), bam=write_reads(str(d / "in.bam"), "wb", batch, G))
    pr = sorted((s, e) for s, e, _ in j["primers"])
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    sets = cooc.parse_sets(text, ref_seq)
    dev = U.SetList([[(p, l, s) for _, p, l, s in muts] for _, muts in sets.sets])
    assert [np.array_equal(x, y) for x, y in zip(dev.arrays(), (sets.set_off, sets.site_pos, sets.site_len, sets.site_sym))] == [True] * 4
    want = {}
    for do_trim in (True, False):           # aio counts the trimmed reads; variants and consensus take the file as it is
        r = oracle.process(batch, G, *(tabs if do_trim else (None, None, 0)), MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        want[do_trim] = U.tables(S.walked_segments(batch, r.trim if do_trim else None), G, dev, MQ)
    return files, dict(sets=sets, ref=ref_seq, want=want, job=j), G


def run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    amplipy.main(argv)


def switches(monkeypatch, dist=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if dist:
        monkeypatch.setenv("AMPLIPY_FORCE_DIST", "1")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check_vcf(with_key, plain, tables):
    """Every record's last key is cooc.Tables' word on the restatement; with the key and its header line stripped the file is
    ``plain``.  -> {position: (alts, COOC)}."""
    text = with_key.decode()
    assert cooc.HEADER_LINES in text
    out, recs = [], {}
    for line in text.replace(cooc.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert kvs[-1].startswith("COOC=")
            pos, alts = int(f[1]) - 1, f[4].split(",")
            assert kvs[-1] == tables.info(pos, f[3], alts), line
            recs.setdefault(pos, (alts, kvs[-1][5:]))
            f[7] = ";".join(kvs[:-1])
            line = "\t".join(f)
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    return recs


def check_constructions(recs, tsv_text, want, tables):
    j = want["job"]
    pa, pb, pc = j["pa"], j["pb"], j["pc"]
    lines = tsv_text.splitlines()
    assert lines[0] == "#" + "\t".join(cooc.COLUMNS)
    rows = [l.split("\t") for l in lines[1:]]
    by = {(r[1], r[3]): r for r in rows}
    assert list(dict.fromkeys(r[1] for r in rows)) == ["linked", "unlinked", "del_and_sub", "nowhere"]      # the file's order
    # (a) the linked pair: pattern 11 at about the allele frequency (60 % of the reads carry both)
    r11 = by[("linked", "11")]
    assert int(r11[5]) > 200 and 0.5 < float(r11[6]) < 0.7 and int(r11[4]) == int(tables.cells(0)[3])
    assert int(by.get(("linked", "10"), [0] * 5)[4]) + int(by.get(("linked", "01"), [0] * 5)[4]) < 0.02 * int(r11[5])
    # (b) the unlinked pair: 10 and 01, and no 11.  The file names G(pb+1)A first: pattern "10" is the reads with that one only
    assert ("unlinked", "11") not in by and int(by[("unlinked", "10")][4]) > 50 and int(by[("unlinked", "01")][4]) > 50
    assert by[("unlinked", "10")][2].startswith("G%d" % (pb + 2))
    c = tables.cells(1)
    assert int(by[("unlinked", "10")][4]) == c[2] and int(by[("unlinked", "01")][4]) == c[1]          # (on the device C(pb)A is site 0)
    # (c) the deletion with a substitution: reported, the deletion on about half of the reads that span it
    both, only_del = int(by[("del_and_sub", "11")][4]), int(by[("del_and_sub", "10")][4])
    assert both > 50 and only_del > 20 and 0.3 < (both + only_del) / int(by[("del_and_sub", "11")][5]) < 0.7
    # a set nothing reaches: one row, the all-mutated pattern, no reads
    assert by[("nowhere", "1")][4:] == ["0", "0", "0", "0"]
    # the VCF: COOC on the records of the sets' substitutions, '.' elsewhere
    assert recs[pa][1].split("|") == ["linked:%d:%d" % (tables.cells(0)[3], sum(tables.cells(0)[:64])), "del_and_sub:%d:%d" % (tables.cells(2)[3], sum(tables.cells(2)[:64]))]
    assert recs[pa + 1][1] == "linked:%d:%d" % (tables.cells(0)[3], sum(tables.cells(0)[:64]))
    assert recs[pb][1].startswith("unlinked:0:") and recs[pb + 1][1].startswith("unlinked:0:")
    named = {pa, pa + 1, pb, pb + 1}
    assert all(v[1] == "." for p, v in recs.items() if p not in named) and len(recs) > len(named)


def test_aio_with_cooc_flags(tmp_path, job, monkeypatch, capfd):
    files, want, G = job
    switches(monkeypatch)
    c, rd = want["want"][True]
    tables = cooc.Tables(want["sets"], c, rd)
    got = {}
    extras = {"plain": [], "co": ["--cooc", files["sets"], "--cooc_out", str(tmp_path / "co.tsv")],
              "more": ["--strand", "--deletions"],
              "co_more": ["--strand", "--deletions", "--cooc", files["sets"], "--cooc_out", str(tmp_path / "co2.tsv.gz")]}
    for tag, extra in extras.items():
        base = ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        capfd.readouterr()
        run(monkeypatch, base + extra)
        log = capfd.readouterr().err
        assert ("Co-occurrence: %d reads tallied, %d irregular reads skipped; 4 mutation sets" % (int(rd[0]), int(rd[1])) in log) == ("co" in tag)
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".bam", ".vcf", ".fas")]
    for tag, base in (("co", "plain"), ("co_more", "more")):
        assert got[tag][0] == got[base][0] and got[tag][2] == got[base][2] and len(got[base][0]) > 30000
        assert b"COOC" not in got[base][1]
        recs = check_vcf(got[tag][1], got[base][1], tables)
    tsv_text = read(str(tmp_path / "co.tsv")).decode()
    assert gzip.open(str(tmp_path / "co2.tsv.gz"), "rt").read() == tsv_text
    check_constructions(recs, tsv_text, want, tables)
    # an existing --cooc_out is refused like every other output; --cooc_out without --cooc, and --cooc on a run that only trims
    for argv in (["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / "x.bam"), "-ov", str(tmp_path / "x.vcf"),
                  "-oc", str(tmp_path / "x.fas"), "--cooc", files["sets"], "--cooc_out", str(tmp_path / "co.tsv")],
                 ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "y.vcf"), "--cooc_out", str(tmp_path / "y.tsv")],
                 ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "z.bam"), "--cooc", files["sets"]]):
        with pytest.raises(SystemExit):
            run(monkeypatch, argv)
    assert read(str(tmp_path / "co.tsv")).decode() == tsv_text


def test_variants_and_consensus_alone(tmp_path, job, monkeypatch):
    files, want, G = job
    switches(monkeypatch)
    c, rd = want["want"][False]
    tables = cooc.Tables(want["sets"], c, rd)
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "co.vcf"), "--cooc", files["sets"],
                      "--cooc_out", str(tmp_path / "v.tsv")])
    recs = check_vcf(read(str(tmp_path / "co.vcf")), read(str(tmp_path / "plain.vcf")), tables)
    tsv_text = read(str(tmp_path / "v.tsv")).decode()
    check_constructions(recs, tsv_text, want, tables)
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "co.fas"), "--cooc", files["sets"],
                      "--cooc_out", str(tmp_path / "c.tsv")])
    assert read(str(tmp_path / "co.fas")) == read(str(tmp_path / "plain.fas"))
    assert read(str(tmp_path / "c.tsv")).decode() == tsv_text


def test_one_rank_through_rccl_gives_the_same_files(tmp_path, job, monkeypatch):
    files, want, G = job
    got = {}
    for tag, dist in (("plain", False), ("dist", True)):
        switches(monkeypatch, dist=dist)
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29553")
        run(monkeypatch, ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                          "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH),
                          "--cooc", files["sets"], "--cooc_out", str(tmp_path / (tag + ".tsv"))])
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".vcf", ".tsv", ".fas")]
    assert got["dist"] == got["plain"]
