"""k_codon on the device (amplipy_amd/csrc/amp_codon.hip) against the plain restatement in
tests/codon_util.py, which tests/test_codon_twin.py pins to the oracle's count table: the table on the oracle's trim results at
sizes round the tile, sorted and shuffled, on CDS sets with overlapping frames; the crafted reads; without trimming; every read
kernel; the state of the hook; device batches; the refusal; all four hooks together; and the command line on a synthetic job
that carries a linked double substitution, two unlinked ones and an in-frame deletion."""
import gzip
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, codon, lib, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import amplicon_util as A
from tests import codon_util as U
from tests import strand_util as S

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
MQ, WINDOW = 20, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "amplipy_amd", "csrc", "amp_codon.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


W, SLOTS, BLOCK = header_constant("CD_W"), header_constant("CD_SLOTS"), header_constant("CD_BLOCK")


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
        self.cds = U.overlapping(self.G)
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

    def fresh(self, mq=MQ, do_trim=True, variant=0, cds=None):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(variant)
        self.eng.reset()
        codon.enable(self.eng, cds or self.cds)
        return self.eng


_SETS = {}


def get_set(name):
    if name not in _SETS:
        _SETS[name] = PrimerSet(name)
    return _SETS[name]


@pytest.fixture(params=["one", "example"])
def pset(request):
    return get_set(request.param)


def want_tables(batch, res, G, cds, mq, do_trim):
    return U.tables(S.walked_segments(batch, res if do_trim else None), G, cds.starts, mq)


def run_and_check(eng, batch, G, cds, oracle_counts, mq=MQ, do_trim=True, what=""):
    """One batch through the engine: the count table is the oracle's, the codon table is the restatement's on the device's own
    trim results, and the invariants hold against the oracle's count table.  -> (codon, reads)."""
    res = eng.process(batch)
    assert np.array_equal(eng.counts(), oracle_counts), what
    want_c, want_r = want_tables(batch, res, G, cds, mq, do_trim)
    got_c, got_r = eng.codon_tables()
    assert np.array_equal(got_r, want_r), what
    assert np.array_equal(got_c, want_c), what
    U.check_at_most_counts(got_c, cds.starts, oracle_counts)
    assert int(got_r.sum()) == batch.n - int((res.status != 0).sum())
    return got_c, got_r


# ---- 1. the table against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(pset, n, order):
    batch = pset.batch(n)
    if order == "shuffled" and n > 1:
        batch = synth.gather_rows(batch, np.random.default_rng(5).permutation(batch.n))
        assert n < 63 or (np.diff(batch.pos) < 0).any()
    eng = pset.fresh()
    c, r = run_and_check(eng, batch, pset.G, pset.cds, pset.oracle(n).counts, what=(pset.name, n, order))
    if n >= 1025:
        assert c[:, :64].any() and c[:, U.BROKEN].any()
    if n:
        assert eng.codon_last_ms() > 0


@pytest.mark.parametrize("frames", ["one", "three"])
def test_frames(frames):
    s = get_set("one")
    cds = U.one_frame(s.G) if frames == "one" else U.three_frames(s.G)
    eng = s.fresh(cds=cds)
    run_and_check(eng, s.batch(1025), s.G, cds, s.oracle(1025).counts)


@pytest.mark.parametrize("frame", [0, 2])
def test_whole_codon_reads_give_the_count_table(frame):
    G = 2000
    rng = np.random.default_rng(40 + frame)
    segs = U.whole_codon_reads(800, G, frame, rng)
    cds = U.one_frame(G, frame)
    c, r = run_crafted(segs, G, cds)
    counts = _EDGE[G].counts()
    U.check_equal_counts(c, cds.starts, counts, counts.sum(axis=1) > 0)
    assert list(r) == [800, 0]


# ---- 2. crafted reads -----------------------------------------------------------------------------------------------------------
_EDGE = {}


def run_crafted(segs, G, cds, mq=MQ, variant=0):
    """The reads counted as they are (no trimming) -> the engine."""
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, G, None, None, 0, mq, WINDOW, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    if G not in _EDGE:
        _EDGE[G] = lib.Engine(G)
    eng = _EDGE[G]
    eng.set_params(mq, WINDOW, False, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    codon.enable(eng, cds)
    out = run_and_check(eng, batch, G, cds, r.counts, mq=mq, do_trim=False)
    eng.set_kernel_variant(0)
    return out


_CRAFTED = U.crafted(W, SLOTS, BLOCK)


@pytest.mark.parametrize("case", _CRAFTED, ids=[c[0] for c in _CRAFTED])
def test_crafted_reads(case):
    name, G, cds, segs, mq, expect = case
    c, r = run_crafted(segs, G, cds, mq=mq)
    expect(c, r, cds)


def test_without_trimming_the_read_is_counted_as_it_came_in():
    s = get_set("example")
    eng = s.fresh(do_trim=False)
    off = run_and_check(eng, s.batch(1025), s.G, s.cds, s.oracle(1025, do_trim=False).counts, do_trim=False)[0]
    eng = s.fresh()
    on = run_and_check(eng, s.batch(1025), s.G, s.cds, s.oracle(1025).counts)[0]
    assert not np.array_equal(on, off)


@pytest.mark.parametrize("variant", [0, 2, 5, 7])
def test_every_read_kernel_feeds_the_same_table(variant):
    s = get_set("example")
    eng = s.fresh(variant=variant)
    run_and_check(eng, s.batch(1025), s.G, s.cds, s.oracle(1025).counts, what=variant)
    eng.set_kernel_variant(0)


# ---- 3. state -------------------------------------------------------------------------------------------------------------------
def test_tables_accumulate_reset_stop_when_disabled_and_take_codon_add():
    s = get_set("example")
    eng = s.fresh()
    res_a = eng.process(s.batch(257))
    res_b = eng.process(s.batch(1025))
    ta = want_tables(s.batch(257), res_a, s.G, s.cds, MQ, True)
    tb = want_tables(s.batch(1025), res_b, s.G, s.cds, MQ, True)
    c, r = eng.codon_tables()
    assert np.array_equal(c, ta[0] + tb[0]) and np.array_equal(r, ta[1] + tb[1])
    eng.reset()
    c, r = eng.codon_tables()
    assert not c.any() and not r.any()
    eng.process(s.batch(257))
    eng.codon_disable()
    eng.process(s.batch(1025))
    c, r = eng.codon_tables()                                   # what was tallied stays readable, nothing was added
    assert np.array_equal(c, ta[0]) and np.array_equal(r, ta[1])
    big = np.array([2 ** 40 + 5, 0], np.uint64)
    eng.codon_add(tb[0], tb[1] + big)                           # another rank's tables, a read count beyond 32 bits
    c, r = eng.codon_tables()
    assert np.array_equal(c, ta[0] + tb[0]) and np.array_equal(r, ta[1] + tb[1] + big)
    codon.enable(eng, s.cds)                                    # on again: the tables start at zero
    c, r = eng.codon_tables()
    assert not c.any() and not r.any()
    # another set on an engine that had one: the tables are laid out again
    other = U.three_frames(s.G)
    codon.enable(eng, other)
    res = eng.process(s.batch(257))
    want = want_tables(s.batch(257), res, s.G, other, MQ, True)
    c, r = eng.codon_tables()
    assert c.shape[0] == other.n_slots and np.array_equal(c, want[0]) and np.array_equal(r, want[1])


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
    want = eng.codon_tables()
    assert np.array_equal(want[0], want_tables(s.batch(1025), res, s.G, s.cds, MQ, True)[0])
    b, out = _device_batch(s.batch(1025))
    for drop in ((), ("ref_len", "trim_flags")):                # the hook needs neither ref_len nor trim_flags
        eng.reset()
        eng.process_device(b.struct(), 0, _dev_out(out, drop=drop))
        eng.sync()
        got = eng.codon_tables()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.codon_disable()
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
        e.codon_tables()
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError):
        e.codon_last_ms()
    with pytest.raises(lib.AmpliHipError) as err:
        e.codon_add(np.zeros(0, np.uint32), np.zeros(2, np.uint64))
    assert err.value.rc == -5
    e.codon_disable()           # off while off: nothing to do
    for starts in ([10, 10], [10, 9], [-1, 5], [0, 498], [497, 498]):
        with pytest.raises(lib.AmpliHipError) as err:
            e.codon_enable(starts)
        assert err.value.rc == -1
    e.codon_enable([0, 497])
    e.close()
    big = lib.Engine(2 ** 20 + 8)           # one slot more than 2^20
    with pytest.raises(lib.AmpliHipError) as err:
        big.codon_enable(np.arange(2 ** 20 + 1, dtype=np.int32))
    assert err.value.rc == -1
    big.close()


# ---- 4. the refusal -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [None, "new_pos", "new_ncig", "new_cig", "status"])
def test_a_trimming_pass_without_its_results_is_refused_before_it_runs(drop):
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before, tables_before = eng.counts(), eng.codon_tables()
    b, out = _device_batch(s.batch(1025))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, None if drop is None else _dev_out(out, drop=(drop,)))
    assert e.value.rc == -1
    eng.sync()
    after = eng.codon_tables()
    assert np.array_equal(eng.counts(), before) and np.array_equal(after[0], tables_before[0]) and np.array_equal(after[1], tables_before[1])
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.codon_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the hook existed
    eng.sync()
    eng.set_params(MQ, WINDOW, False, True)                        # without trimming nothing of dev_out is needed
    eng.reset()
    codon.enable(eng, s.cds)
    eng.process_device(b.struct(), 0, None)
    eng.sync()
    want = want_tables(s.batch(1025), None, s.G, s.cds, MQ, False)
    got = eng.codon_tables()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 5. all four hooks together -------------------------------------------------------------------------------------------------
def test_all_four_hooks_together_give_what_each_gives_alone():
    s = get_set("example")
    amps = A.example_amps()
    batch = s.batch(1025)
    regions = [(0, s.G), (1000, 2000)]

    def engine(qc=False, strand=False, amplicon=False, cod=False):
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
            codon.enable(eng, s.cds)
        eng.process(batch)
        return eng

    every = engine(True, True, True, True)
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
    assert every.codon_tables()[0].any() and np.array_equal(every.counts(), alone.counts())
    alone.close()
    every.close()


# ---- 6. command line ------------------------------------------------------------------------------------------------------------
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
    """The files of the job and what the outputs must show: codon.Tables on the restatement on the oracle's trim results."""
    d = tmp_path_factory.mktemp("codon_cli")
    j = U.synthetic_job()
    g, batch = j["genome"], j["batch"]
    G = int(g.size)
    ref_seq = synth.genome_string(g)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + ref_seq + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), j["primers"])
    cds_fn = d / "cds.tsv"; cds_fn.write_text("".join("%s\t%d\t%d\t%s\n" % r for r in j["rows"]))
    files = dict(ref=str(ref), bed=str(bed), cds=str(cds_fn), bam=write_reads(str(d / "in.bam"), "wb", batch, G),
                 sam=write_reads(str(d / "in.sam"), "w", batch, G))
    pr = sorted((s, e) for s, e, _ in j["primers"])
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    cds = U.cds_set(j["rows"], G)
    want = {}
    for do_trim in (True, False):           # aio counts the trimmed reads; variants and consensus take the file as it is
        r = oracle.process(batch, G, *(tabs if do_trim else (None, None, 0)), MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        c, rd = U.tables(S.walked_segments(batch, r.trim if do_trim else None), G, cds.starts, MQ)
        U.check_at_most_counts(c, cds.starts, r.counts)
        want[do_trim] = (c, rd)
    return files, dict(cds=cds, ref=ref_seq, want=want, job=j), G


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


def info_of(line):
    f = line.split("\t")
    return int(f[1]) - 1, f[3], f[4].split(","), dict(kv.split("=", 1) for kv in f[7].split(";"))


def check_vcf(with_keys, plain, tables):
    """Every record's five keys are codon.Tables' word on the restatement; with the keys and their header lines stripped the
    file is ``plain``.  -> {position: (ref, alts, keys)}."""
    text = with_keys.decode()
    assert codon.HEADER_LINES in text
    out, recs = [], {}
    for line in text.replace(codon.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-5:]] == list(codon.KEYS)
            pos, ref, alts, keys = info_of(line)
            assert ";".join(kvs[-5:]) == tables.info(pos, ref, alts), line
            recs.setdefault(pos, (ref, alts, keys))
            f[7] = ";".join(kvs[:-5])
            line = "\t".join(f)
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    return recs


def check_constructions(recs, codon_text, aa_text, want, tables):
    j = want["job"]
    pa, pb, pc = j["pa"], j["pb"], j["pc"]
    rows = [l.split("\t") for l in codon_text.splitlines()[1:]]
    by = {(r[1], int(r[3]) - 1, r[6]): r for r in rows}                 # (cds, codon start, codon) -> line
    # (a) the linked pair: both records say R>K by CGG>AAG, at about the pair's depth, and --aa_out has the change
    ra, rb = recs[pa], recs[pa + 1]
    assert ra[1] == ["A"] and rb[1] == ["A"]
    num = (pa - j["rows"][0][1]) // 3 + 1
    for rec in (ra, rb):
        k = rec[2]
        assert k["CDS"].split("|")[0] == "orfA" and k["ALT_AA"].split("|")[0] == "R%dK" % num and k["ALT_CODON"].split("|")[0] == "CGG>AAG"
        dp, pair = int(k["CODON_DP"].split("|")[0]), int(k["ALT_CODON_DP"].split("|")[0])
        assert dp > 200 and 0.5 < pair / dp < 0.7
    assert ra[2]["ALT_CODON_DP"].split("|")[0] == rb[2]["ALT_CODON_DP"].split("|")[0] == by[("orfA", pa, "AAG")][8]
    aa = [l.split("\t") for l in aa_text.splitlines()[1:]]
    linked = [l for l in aa if l[1] == "orfA" and l[2] == "R%dK" % num]
    assert len(linked) == 1 and linked[0][6].split(",")[0] == "AAG:%s" % by[("orfA", pa, "AAG")][8]
    assert not [l for l in aa if l[1] == "orfA" and l[2] == "R%dQ" % num and float(l[5]) > 0.1]
    # (b) two substitutions on disjoint reads: different amino acids, and no double mutant
    numb = (pb - j["rows"][0][1]) // 3 + 1
    r1, r2 = recs[pb][2], recs[pb + 1][2]
    assert r1["ALT_AA"].split("|")[0] == "R%dR" % numb and r2["ALT_AA"].split("|")[0] == "R%dQ" % numb
    assert r1["ALT_CODON"].split("|")[0] == "CGG>AGG" and r2["ALT_CODON"].split("|")[0] == "CGG>CAG"
    assert ("orfA", pb, "AAG") not in by and int(by[("orfA", pb, "AGG")][8]) > 50 and int(by[("orfA", pb, "CAG")][8]) > 50
    assert int(tables.cells(pb)[U.cell_of("AAG")]) == 0
    # (c) the in-frame deletion breaks its codon in every frame that has one there
    assert int(tables.cells(pc)[U.BROKEN]) > 50 and int(by[("orfA", pc, synth.genome_string(j["genome"][pc:pc + 3]))][11]) > 50
    assert int(tables.cells(pc - 3)[U.BROKEN]) < 10                      # (the batch's own indels break a few)


_TSV = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_aio_with_codon_flags(tmp_path, job, monkeypatch, route, capfd):
    files, want, G = job
    name, inp, out, gpu_sam = route
    switches(monkeypatch, gpu_sam)
    c, rd = want["want"][True]
    tables = codon.Tables(want["cds"], want["ref"], c, rd, amplipy.DEFAULTS["min_depth_variants"], amplipy.DEFAULTS["min_freq_variants"])
    got = {}
    extras = {"plain": [], "cod": ["--codons", files["cds"], "--codon_out", str(tmp_path / "c.tsv"), "--aa_out", str(tmp_path / "aa.tsv")],
              "more": ["--strand"],
              "cod_more": ["--strand", "--codons", files["cds"], "--codon_out", str(tmp_path / "c2.tsv.gz")]}
    for tag, extra in extras.items():
        base = ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + "." + out)),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        capfd.readouterr()
        run(monkeypatch, base + extra)
        log = capfd.readouterr().err
        assert ("Codons: %d reads tallied, %d irregular reads skipped" % (int(rd[0]), int(rd[1])) in log) == ("cod" in tag)
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in ("." + out, ".vcf", ".fas")]
    for tag, base in (("cod", "plain"), ("cod_more", "more")):
        assert got[tag][0] == got[base][0] and got[tag][2] == got[base][2] and len(got[base][0]) > 30000
        assert b"CODON_DP" not in got[base][1]
        recs = check_vcf(got[tag][1], got[base][1], tables)
    codon_text = read(str(tmp_path / "c.tsv")).decode()
    aa_text = read(str(tmp_path / "aa.tsv")).decode()
    assert gzip.open(str(tmp_path / "c2.tsv.gz"), "rt").read() == codon_text
    check_constructions(recs, codon_text, aa_text, want, tables)
    _TSV[name] = (codon_text, aa_text)
    assert all(t == (codon_text, aa_text) for t in _TSV.values())        # the same files on every route run so far
    # an existing --codon_out or --aa_out is refused like every other output, before a read is looked at
    for flag, fn in (("--codon_out", "c.tsv"), ("--aa_out", "aa.tsv")):
        with pytest.raises(SystemExit):
            run(monkeypatch, ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / ("x." + out)),
                              "-ov", str(tmp_path / "x.vcf"), "-oc", str(tmp_path / "x.fas"), "--codons", files["cds"], flag, str(tmp_path / fn)])
    assert read(str(tmp_path / "c.tsv")).decode() == codon_text


def test_variants_and_consensus_alone(tmp_path, job, monkeypatch):
    files, want, G = job
    switches(monkeypatch)
    c, rd = want["want"][False]
    tables = codon.Tables(want["cds"], want["ref"], c, rd, amplipy.DEFAULTS["min_depth_variants"], amplipy.DEFAULTS["min_freq_variants"])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "cod.vcf"), "--codons", files["cds"],
                      "--codon_out", str(tmp_path / "v.tsv"), "--aa_out", str(tmp_path / "vaa.tsv")])
    recs = check_vcf(read(str(tmp_path / "cod.vcf")), read(str(tmp_path / "plain.vcf")), tables)
    codon_text = read(str(tmp_path / "v.tsv")).decode()
    check_constructions(recs, codon_text, read(str(tmp_path / "vaa.tsv")).decode(), want, tables)
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "cod.fas"), "--codons", files["cds"],
                      "--codon_out", str(tmp_path / "c.tsv")])
    assert read(str(tmp_path / "cod.fas")) == read(str(tmp_path / "plain.fas"))
    assert read(str(tmp_path / "c.tsv")).decode() == codon_text
    with pytest.raises(SystemExit):          # the amino-acid calls use the variant thresholds
        run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "x.fas"), "--codons", files["cds"],
                          "--aa_out", str(tmp_path / "x.tsv")])


def test_one_rank_through_rccl_gives_the_same_files(tmp_path, job, monkeypatch):
    files, want, G = job
    got = {}
    for tag, dist in (("plain", False), ("dist", True)):
        switches(monkeypatch, dist=dist)
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29551")
        run(monkeypatch, ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                          "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH),
                          "--codons", files["cds"], "--codon_out", str(tmp_path / (tag + ".tsv")), "--aa_out", str(tmp_path / (tag + ".aa.tsv"))])
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".vcf", ".tsv", ".aa.tsv", ".fas")]
    assert got["dist"] == got["plain"]
    if "host" in _TSV:
        assert got["plain"][1].decode() == _TSV["host"][0]
