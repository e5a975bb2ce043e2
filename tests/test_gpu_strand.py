"""The strand and base-quality tallies on the device (amp_strand.hip: k_strand) against the plain
restatement of tests/strand_util.py, applied to the batch and the ORACLE's trim results, and against the oracle's own two
constructions (the reverse reads alone, the sweep of quality thresholds).  Batch sizes around a wave, a tile and past a block's
first tile, on one primer and on the example BED, sorted and shuffled; crafted edges of the window and the slots; state across
batches, reset, disable, strand_add and the device-pointer form; the refusal of a pass without its results.  Last, the command
line: aio with --strand and --strand_out through the host codecs and a device-codec route, variants alone, one rank through
RCCL -- the fields equal the restatement, and with them stripped every output is byte for byte what the same command writes
without the flags."""
import gzip
import os
import re
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, lib, strand, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import helpers as H
from tests import qc_util as Q
from tests import strand_util as S

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
MQ, WINDOW = 20, 4


def header_constant(name):
    text = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "amplipy_amd", "csrc", "amp_strand.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


W, SLOTS = header_constant("ST_W"), header_constant("ST_SLOTS")


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
        """(counts, rev, qsum) of batch (n, seed); the restatement's count table is held to the oracle's on the way."""
        key = (n, seed, mq, do_trim)
        if key not in self.wants:
            b = self.batch(n, seed)
            r = oracle.process(b, self.G, *self.tabs, mq, WINDOW, do_trim=do_trim, do_count=True)
            assert not r.trim.status.any()
            t = S.tables(S.walked_segments(b, r.trim if do_trim else None), self.G, mq)
            assert np.array_equal(t[0], r.counts)
            for a in t:
                a.setflags(write=False)
            self.wants[key] = t
        return self.wants[key]

    def fresh(self, mq=MQ, do_trim=True):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(0)
        self.eng.reset()
        self.eng.strand_enable()
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
    counts, rev, qsum = want
    got_rev, got_qsum = eng.strand_tables()
    assert np.array_equal(eng.counts(), counts), what
    assert np.array_equal(got_rev, rev), what
    assert np.array_equal(got_qsum, qsum), what


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
    counts, rev, qsum = want
    assert (rev <= counts).all() and (qsum >= np.uint64(MQ) * counts[:, :5].astype(np.uint64)).all()
    if n >= 1025:           # both strands, deletions and quality sums are there
        assert rev.any() and (rev < counts).any() and rev[:, 5].any() and int(qsum.sum()) > MQ * n
    if n:
        assert eng.strand_last_ms() > 0


# ---- 2. the reverse-subset identity against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("strand_of", ["forward", "reverse", "mixed"])
def test_reverse_reads_alone_are_rev(strand_of):
    s = get_set("example")
    b = s.batch(3000, seed=21)
    flag = b.flag.copy()
    if strand_of == "forward":
        flag &= np.uint16(0xFFFF ^ 0x10)
    elif strand_of == "reverse":
        flag |= np.uint16(0x10)
    batch = ReadBatch(b.pos, flag, b.tlen, b.lseq, b.cig_off, b.cig, b.seq_off, b.seq, b.qual)
    rev_o, counts_o = S.oracle_rev(oracle.process, batch, s.G, s.tabs, MQ, WINDOW, True)
    eng = s.fresh()
    eng.process(batch)
    rev, _ = eng.strand_tables()
    assert np.array_equal(eng.counts(), counts_o) and np.array_equal(rev, rev_o)
    assert counts_o.any()
    if strand_of == "forward":
        assert not rev.any()
    elif strand_of == "reverse":
        assert np.array_equal(rev, counts_o)
    else:
        assert rev.any() and (rev < counts_o).any()


# ---- 3. the quality sweep -----------------------------------------------------------------------------------------------------
def test_quality_sweep_of_the_oracle_is_qsum():
    s = get_set("example")
    mq = 30
    batch = s.batch(3000, seed=22)
    r = oracle.process(batch, s.G, *s.tabs, mq, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    qsum_o, first = S.oracle_qsum(oracle.process, S.walked_batch(batch, r.trim), s.G, mq)
    assert np.array_equal(first, r.counts)
    eng = s.fresh(mq=mq)
    eng.process(batch)
    rev, qsum = eng.strand_tables()
    assert np.array_equal(eng.counts(), r.counts) and np.array_equal(qsum, qsum_o)
    assert int(qsum.sum()) > mq * 10000 and (qsum >= np.uint64(mq) * r.counts[:, :5].astype(np.uint64)).all()


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------
_EDGE = {}


def edge_engine(G):
    if G not in _EDGE:
        _EDGE[G] = lib.Engine(G)
    return _EDGE[G]


def run_crafted(segs, G, mq=MQ, variant=0):
    """The reads counted as they are (no trimming) -> the engine; the tables must be the restatement's, whose count table
    must be the oracle's."""
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, G, None, None, 0, mq, WINDOW, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    want = S.tables(segs, G, mq)
    assert np.array_equal(want[0], r.counts)
    eng = edge_engine(G)
    eng.set_params(mq, WINDOW, False, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    eng.strand_enable()
    eng.process(batch)
    assert_tables(eng, want)
    eng.set_kernel_variant(0)
    return want


def pile(rng, start, n, length=60):
    return [S.seg(start + int(rng.integers(0, 8)), [(0, length)], rng, 0x10 if k % 2 else 0) for k in range(n)]


@pytest.mark.parametrize("span", [W - 1, W, W + 1, 3 * W])
def test_tile_spans_around_the_window(span):
    rng = np.random.default_rng(span)
    segs = pile(rng, 5, 100, 40) + [S.seg(5 + span - 40, [(0, 40)], rng, 0x10), S.seg(5 + span - 41, [(0, 30), (2, 4), (0, 7)], rng, 0x10)]
    segs.sort(key=lambda g: g.reference_start)
    counts, rev, qsum = run_crafted(segs, 4 * W)
    assert rev[5 + span - 1].sum() == 2 and rev[5 + span:].sum() == 0


def test_more_segments_than_slots_soft_clips_and_a_deletion_across_the_edge():
    rng = np.random.default_rng(9)
    edge = 20 + W
    segs = pile(rng, 20, 300, 70)          # two tiles on one pile: the window stays
    segs += [S.seg(22, S.many_segment_cigar(SLOTS), rng, 0x10), S.seg(22, S.many_segment_cigar(SLOTS - 1), rng, 0), S.seg(23, S.many_segment_cigar(20), rng, 0x10),
             S.seg(24, [(5, 3), (4, 6), (0, 40), (1, 2), (0, 5), (4, 9), (5, 2)], rng, 0x10), S.seg(25, [(4, 7), (0, 33)], rng, 0, qual=[2] * 7 + [35] * 33),
             S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0x10), S.seg(edge - 21, [(0, 18), (3, 5), (0, 12)], rng, 0)]
    segs.sort(key=lambda g: g.reference_start)
    counts, rev, qsum = run_crafted(segs, 4 * W)
    assert list(rev[edge - 2:edge + 3, 5]) == [1] * 5 and counts[edge - 3:edge + 3, 5].sum() == 10


@pytest.mark.parametrize("mq", [0, 100])
def test_min_quality_zero_and_above_every_quality(mq):
    rng = np.random.default_rng(mq + 1)
    segs = pile(rng, 40, 70) + [S.seg(41, [(0, 20), (2, 3), (0, 20)], rng, 0x10), S.seg(42, [(0, 20), (1, 3), (0, 20)], rng, 0x10, qual=0),
                                S.seg(43, [(0, 9), (2, 2), (0, 9)], rng, 0)]
    counts, rev, qsum = run_crafted(segs, 3000, mq=mq)
    if mq == 0:
        assert int(counts[:, :5].sum()) == 70 * 60 + 40 + 40 + 18
    else:       # only '-' cells are left
        assert not counts[:, :5].any() and not qsum.any() and int(counts[:, 5].sum()) == 5 and int(rev[:, 5].sum()) == 3 and not rev[:, :5].any()


def test_without_trimming_the_read_is_walked_as_it_came_in():
    s = get_set("example")
    eng = s.fresh(do_trim=False)
    eng.process(s.batch(1025))
    want = s.want(1025, do_trim=False)
    assert_tables(eng, want)
    assert not np.array_equal(want[1], s.want(1025)[1])         # (trimming changes what is counted)


@pytest.mark.parametrize("variant", [0, 2, 5, 7])
def test_every_read_kernel_feeds_the_same_tables(variant):
    s = get_set("example")
    eng = s.fresh()
    eng.set_kernel_variant(variant)
    eng.process(s.batch(1025))
    assert_tables(eng, s.want(1025), variant)
    eng.set_kernel_variant(0)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def add(a, b):
    return tuple(x.astype(np.uint64) + y for x, y in zip(a, b))


def test_tables_accumulate_reset_stop_when_disabled_and_take_strand_add():
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    eng.process(s.batch(1025))
    both = add(s.want(257), s.want(1025))
    assert_tables(eng, both)
    eng.reset()
    rev, qsum = eng.strand_tables()
    assert not rev.any() and not qsum.any()
    eng.process(s.batch(257))
    assert_tables(eng, s.want(257))
    eng.strand_disable()
    eng.process(s.batch(1025))
    rev, qsum = eng.strand_tables()            # what was tallied stays readable, nothing was added
    assert np.array_equal(rev, s.want(257)[1]) and np.array_equal(qsum, s.want(257)[2])
    assert np.array_equal(eng.counts(), both[0])
    # strand_add: another rank's tables, with a sum beyond 32 bits
    big = np.zeros((s.G, 5), np.uint64); big[7, 2] = 2 ** 40 + 5
    eng.strand_add(s.want(1025)[1], s.want(1025)[2] + big)
    rev, qsum = eng.strand_tables()
    assert np.array_equal(rev, both[1]) and np.array_equal(qsum, both[2] + big)
    eng.strand_enable()                        # on again: the tables start at zero
    rev, qsum = eng.strand_tables()
    assert not rev.any() and not qsum.any()


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
    b, out = _device_batch(s.batch(1025))
    eng.process_device(b.struct(), 0, _dev_out(out))
    eng.sync()
    assert_tables(eng, s.want(1025))
    # the tallies need neither ref_len nor trim_flags
    eng.reset()
    eng.process_device(b.struct(), 0, _dev_out(out, drop=("ref_len", "trim_flags")))
    eng.sync()
    assert_tables(eng, s.want(1025))


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.strand_disable()
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


def test_tables_before_the_first_enable_are_an_error():
    e = lib.Engine(500)
    with pytest.raises(lib.AmpliHipError) as err:
        e.strand_tables()
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError):
        e.strand_last_ms()
    e.strand_disable()          # off while off: nothing to do
    e.close()


# ---- 6. the refusal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [None, "new_pos", "new_ncig", "new_cig", "status"])
def test_a_trimming_pass_without_its_results_is_refused_before_it_runs(drop):
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before = eng.counts()
    b, out = _device_batch(s.batch(1025))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, None if drop is None else _dev_out(out, drop=(drop,)))
    assert e.value.rc == -1
    eng.sync()
    assert np.array_equal(eng.counts(), before)
    assert_tables(eng, s.want(257))
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.strand_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the tallies existed
    eng.sync()
    eng.set_params(MQ, WINDOW, False, True)                        # without trimming nothing of dev_out is needed
    eng.reset()
    eng.strand_enable()
    eng.process_device(b.struct(), 0, None)
    eng.sync()
    assert_tables(eng, s.want(1025, do_trim=False))


# ---- 7. command line -----------------------------------------------------------------------------------------------------------
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
    """The files of the job and the tables the outputs must show: the restatement on the oracle's trim results (aio) and on
    the reads as they are (variants)."""
    d = tmp_path_factory.mktemp("strand_cli")
    g = synth.make_genome()
    G = int(g.size)
    primers, amps = synth.make_artic_scheme()
    pr = sorted((s, e) for s, e, _ in primers)
    batch = S.strand_batch(3000, G, pr, 31)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(g) + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), primers)
    files = dict(ref=str(ref), bed=str(bed), bam=write_reads(str(d / "in.bam"), "wb", batch, G), sam=write_reads(str(d / "in.sam"), "w", batch, G))
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    want = {}
    for do_trim in (True, False):
        r = oracle.process(batch, G, *tabs, MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        t = S.tables(S.walked_segments(batch, r.trim if do_trim else None), G, MQ)
        assert np.array_equal(t[0], r.counts)
        want[do_trim] = strand.Tables(*t)
    assert want[True].rev.any() and (want[True].rev < want[True].counts).any()
    return files, want, G


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


def check_vcf(with_keys, plain, tables):
    """Every record's five keys are the tables' word; with the keys and their header lines stripped the file is ``plain``."""
    text = with_keys.decode()
    assert strand.HEADER_LINES in text
    out = []
    n_records = n_two_strands = 0
    for line in text.replace(strand.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-5:]] == list(strand.KEYS) and kvs[-6].startswith("ALT_FREQ=")
            assert ";".join(kvs[-5:]) == tables.info(int(f[1]) - 1, f[3], f[4].split(","))
            n_two_strands += kvs[-1] not in ("SB=.", "SB=1")
            f[7] = ";".join(kvs[:-5])
            line = "\t".join(f)
            n_records += 1
        out.append(line + "\n")
    assert "".join(out).encode() == plain
    assert n_records > 12 and n_two_strands > 0
    return n_records


def tsv_text(ref_id, tables):
    import io
    f = io.StringIO()
    strand.write_tsv(f, ref_id, tables)
    return f.getvalue()


_TSV = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_aio_with_strand_flags(tmp_path, job, monkeypatch, route):
    files, want, G = job
    name, inp, out, gpu_sam = route
    switches(monkeypatch, gpu_sam)
    got = {}
    for tag in ("plain", "strand"):
        base = ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + "." + out)),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        run(monkeypatch, base + (["--strand", "--strand_out", str(tmp_path / "s.tsv")] if tag == "strand" else []))
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in ("." + out, ".vcf", ".fas")]
    assert got["strand"][0] == got["plain"][0] and got["strand"][2] == got["plain"][2] and len(got["plain"][0]) > 100000
    assert b"REF_RV" not in got["plain"][1]
    check_vcf(got["strand"][1], got["plain"][1], want[True])
    text = read(str(tmp_path / "s.tsv")).decode()
    assert text == tsv_text("SYN_REF", want[True])
    _TSV[name] = text
    assert all(t == text for t in _TSV.values())          # the same file on every route run so far
    # an existing --strand_out is refused like every other output, before a read is looked at
    with pytest.raises(SystemExit):
        run(monkeypatch, ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / ("x." + out)),
                          "-ov", str(tmp_path / "x.vcf"), "-oc", str(tmp_path / "x.fas"), "--strand_out", str(tmp_path / "s.tsv")])
    assert read(str(tmp_path / "s.tsv")).decode() == text


def test_variants_and_consensus_alone(tmp_path, job, monkeypatch):
    files, want, G = job
    switches(monkeypatch)
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "v.vcf"), "--strand", "--strand_out", str(tmp_path / "v.tsv.gz")])
    check_vcf(read(str(tmp_path / "v.vcf")), read(str(tmp_path / "plain.vcf")), want[False])
    assert gzip.open(str(tmp_path / "v.tsv.gz"), "rt").read() == tsv_text("SYN_REF", want[False])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "c.fas"), "--strand_out", str(tmp_path / "c.tsv")])
    assert read(str(tmp_path / "c.fas")) == read(str(tmp_path / "plain.fas"))
    assert read(str(tmp_path / "c.tsv")).decode() == tsv_text("SYN_REF", want[False])


def test_one_rank_through_rccl_gives_the_same_files(tmp_path, job, monkeypatch):
    files, want, G = job
    got = {}
    for tag, dist in (("plain", False), ("dist", True)):
        switches(monkeypatch, dist=dist)
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29548")
        run(monkeypatch, ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                          "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH),
                          "--strand", "--strand_out", str(tmp_path / (tag + ".tsv"))])
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".vcf", ".tsv", ".fas")]
    assert got["dist"] == got["plain"]
    assert got["plain"][1].decode() == tsv_text("SYN_REF", want[True])
