"""k_errprof on the device (amplipy_amd/csrc/amp_errprof.hip) against the plain restatement in
tests/errprof_util.py, which tests/test_errprof_twin.py pins to the oracle's count table: the three tables (exact integers) on the
device's own trim results at sizes round the tile, sorted and shuffled, masked and not; piles of one shape with one quality
throughout and with a different quality per base; strands and mates; the crafted edges; do_trim off; every read kernel; the state
of the hook; device batches; the refusal; all seven hooks together; and the command line -- the JSON report and the two VCF keys against the restatement -- through
the host codecs, both device codecs and one rank through RCCL.  The count table is held to the oracle's throughout."""
import gzip
import json
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, codon, errprof, lib, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import amplicon_util as A
from tests import codon_util as CU
from tests import cooc_util as CO
from tests import errprof_util as U
from tests import strand_util as S

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
MQ, WINDOW = 20, 4


class PrimerSet:
    """One primer set: its engine, its reference letters and, per batch, the oracle's results, computed once."""

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
        ref = list(U.seeded_ref(self.G, 8))
        for p in np.random.default_rng(9).integers(0, self.G, size=self.G // 40):
            ref[int(p)] = "acgtNRY"[int(p) % 7]
        self.ref = "".join(ref)
        self.mask = sorted(set(int(p) for p in np.random.default_rng(10).integers(0, self.G, size=self.G // 20)) | {0, 31, 32, self.G - 1})
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(*self.tabs)
        self.batches, self.oracles = {}, {}

    def batch(self, n, seed=None):
        key = (n, seed)
        if key not in self.batches:
            seed_ = 2000 + n if seed is None else seed
            self.batches[key] = U.with_mates(S.strand_batch(n, self.G, self.primers, seed_), seed_)
        return self.batches[key]

    def oracle(self, n, seed=None, mq=MQ, do_trim=True):
        key = (n, seed, mq, do_trim)
        if key not in self.oracles:
            r = oracle.process(self.batch(n, seed), self.G, *self.tabs, mq, WINDOW, do_trim=do_trim, do_count=True)
            assert not r.trim.status.any()
            r.counts.setflags(write=False)
            self.oracles[key] = r
        return self.oracles[key]

    def mask_array(self, masked):
        m = np.zeros(self.G, bool)
        if masked:
            m[self.mask] = True
        return m if masked else None

    def fresh(self, mq=MQ, do_trim=True, variant=0, masked=False):
        self.eng.set_params(mq, WINDOW, do_trim, True)
        self.eng.set_kernel_variant(variant)
        self.eng.reset()
        self.eng.errprof_enable(self.ref, self.mask_array(masked))
        return self.eng


_SETS = {}


def get_set(name):
    if name not in _SETS:
        _SETS[name] = PrimerSet(name)
    return _SETS[name]


@pytest.fixture(params=["one", "example"])
def pset(request):
    return get_set(request.param)


def run_and_check(eng, batch, ref, mask, oracle_counts, mq=MQ, do_trim=True, what=""):
    """One batch through the engine: the count table is the oracle's, the three tables and the read counters are the
    restatement's on the device's own trim results.  -> (cyc, qualt, sub, reads)."""
    res = eng.process(batch)
    assert np.array_equal(eng.counts(), oracle_counts), what
    assert do_trim or (res.status != 0).sum() <= 1              # (one crafted read has a status: QUAL '*' with the count table on)
    segs = S.walked_segments(batch, res) if do_trim else [batch.segment(i) for i in range(batch.n) if int(res.status[i]) == 0]
    want = U.tables(segs, ref, mask, mq)
    got = eng.errprof_tables()
    for g, w, name in zip(got, want, ("cyc", "qualt", "sub", "reads")):
        assert np.array_equal(g, w), (what, name)
    U.check_invariants(*got[:3])
    assert int(got[3].sum()) == batch.n - int((res.status != 0).sum())
    if mask is None and U.all_regular(segs, len(ref)):         # the identity with the count table, on the device's own numbers
        assert np.array_equal(got[2][:, :, 1].astype(np.int64).sum(axis=(0, 1)), U.by_letter(eng.counts(), ref)), what
    return got


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_match_restatement(pset, n, order):
    batch = pset.batch(n)
    if order == "shuffled" and n > 1:
        batch = synth.gather_rows(batch, np.random.default_rng(5).permutation(batch.n))
        assert n < 63 or (np.diff(batch.pos) < 0).any()
    masked = order == "shuffled"
    eng = pset.fresh(masked=masked)
    cyc, qualt, sub, reads = run_and_check(eng, batch, pset.ref, pset.mask if masked else None, pset.oracle(n).counts, what=(pset.name, n, order))
    if n >= 1025:
        assert cyc[..., 0].any() and cyc[..., 1].any() and all(sub[m, s].any() for m in range(2) for s in range(2)) and reads[1] > 0
    if n:
        assert eng.errprof_last_ms() > 0


# ---- 2. piles, strands and mates, crafted reads -----------------------------------------------------------------------------------
_EDGE = {}


def run_reads(segs, ref, mask=None, mq=MQ, variant=0):
    """Reads as they are (no trimming) through an engine of the reference's length.  -> the tables."""
    G = len(ref)
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, G, None, None, 0, mq, WINDOW, do_trim=False, do_count=True)
    if G not in _EDGE:
        _EDGE[G] = lib.Engine(G)
    eng = _EDGE[G]
    eng.set_params(mq, WINDOW, False, True)
    eng.set_kernel_variant(variant)
    eng.reset()
    m = None
    if mask is not None:
        m = np.zeros(G, bool); m[list(mask)] = True
    eng.errprof_enable(ref, m)
    out = run_and_check(eng, batch, ref, mask, r.counts, mq=mq, do_trim=False)
    eng.set_kernel_variant(0)
    return out


@pytest.mark.parametrize("equal", [True, False], ids=["one_quality", "a_quality_per_base"])
def test_pile_of_20000_reads_of_one_shape(equal):
    ref, segs = U.pile(20000, equal)
    cyc, qualt, sub, reads = run_reads(segs, ref)
    assert [int(x) for x in reads] == [20000, 0] and int(cyc.sum()) == 20000 * 150
    assert int((qualt.sum(axis=(0, 2)) > 0).sum()) == (1 if equal else 60)


@pytest.mark.parametrize("flags", [(0x0,), (0x10,), (0x1 | 0x40, 0x1 | 0x80), (0x1 | 0x80 | 0x10, 0x1 | 0x40), U.FLAGS], ids=["forward", "reverse", "r1_r2", "r2rev_r1", "all"])
def test_strand_and_mate_mixes(flags):
    rng = np.random.default_rng(31)
    ref = U.seeded_ref(1000, 3)
    segs = []
    for k in range(700):
        pos, L = int(rng.integers(0, 800)), int(rng.integers(20, 180))
        segs.append(U._read(pos, [(0, L)], U.noisy(ref, pos, L, rng), flag=flags[k % len(flags)], qual=rng.choice([2, 12, 23, 37], size=L).tolist()))
    cyc, qualt, sub, reads = run_reads(segs, ref)
    mates, strands = sorted({int(bool(f & 0x80)) for f in flags}), sorted({int(bool(f & 0x10)) for f in flags})
    assert [m for m in range(2) if cyc[m].any()] == mates and [s for s in range(2) if sub[:, s].any()] == strands


_CRAFTED = U.crafted(4)


@pytest.mark.parametrize("case", _CRAFTED, ids=[c[0] for c in _CRAFTED])
def test_crafted_edges(case):
    name, ref, mask, segs, mq, expect = case
    expect(*run_reads(segs, ref, mask=mask, mq=mq))


def test_a_read_longer_than_the_block_cells_take():
    from tests.test_errprof_twin import crafted_runs
    name, ref, mask, segs, mq, expect = crafted_runs(4)[-1]
    assert name == "longer_than_the_block_cells_take"
    expect(*run_reads(segs, ref, mq=mq))


def test_a_read_with_a_status_touches_nothing():
    s = get_set("one")
    batch = s.batch(257)
    bad = synth.gather_rows(batch, np.arange(batch.n))
    bad.pos = bad.pos.copy()
    bad.pos[::3] = s.G + 5                                      # past the reference: a status
    eng = s.fresh()
    res = eng.process(bad)
    assert (res.status[::3] != 0).all() and (res.status != 0).sum() == len(range(0, batch.n, 3))
    want = U.tables(S.walked_segments(bad, res), s.ref, None, MQ)
    got = eng.errprof_tables()
    assert U.same(got, want) and int(got[3].sum()) == batch.n - len(range(0, batch.n, 3))


# ---- 3. do_trim off, every read kernel --------------------------------------------------------------------------------------------
def test_without_trimming(pset):
    eng = pset.fresh(do_trim=False)
    run_and_check(eng, pset.batch(1025), pset.ref, None, pset.oracle(1025, do_trim=False).counts, do_trim=False)


@pytest.mark.parametrize("variant", [0, 2, 5, 7])
def test_every_read_kernel_feeds_the_same_tables(variant):
    s = get_set("example")
    eng = s.fresh(variant=variant)
    run_and_check(eng, s.batch(1025), s.ref, None, s.oracle(1025).counts, what=variant)
    eng.set_kernel_variant(0)


# ---- 4. state ---------------------------------------------------------------------------------------------------------------------
def test_tables_accumulate_reset_and_merge():
    s = get_set("example")
    eng = s.fresh()
    res_a = eng.process(s.batch(257))
    res_b = eng.process(s.batch(1025))
    ta = U.tables(S.walked_segments(s.batch(257), res_a), s.ref, None, MQ)
    tb = U.tables(S.walked_segments(s.batch(1025), res_b), s.ref, None, MQ)
    both = [x + y for x, y in zip(ta, tb)]
    assert U.same(eng.errprof_tables(), both)
    # two batches are one concatenated batch
    eng.reset()
    assert not any(t.any() for t in eng.errprof_tables())
    joined = ReadBatch.from_segments(s.batch(257).segments() + s.batch(1025).segments())
    eng.process(joined)
    assert U.same(eng.errprof_tables(), both)
    eng.reset()
    eng.process(s.batch(257))
    eng.errprof_disable()
    eng.process(s.batch(1025))
    assert U.same(eng.errprof_tables(), ta)                     # what was tallied stays readable, nothing was added
    big = np.array([2 ** 40 + 5, 0], np.uint64)
    huge = tb[0].copy(); huge[1, 511, 1] += np.uint64(2 ** 33)
    eng.errprof_add(huge, tb[1], tb[2], tb[3] + big)            # another rank's tables, counts beyond 32 bits
    got = eng.errprof_tables()
    assert np.array_equal(got[0], ta[0] + huge) and np.array_equal(got[1], both[1]) and np.array_equal(got[2], both[2]) and np.array_equal(got[3], both[3] + big)
    eng.errprof_enable(s.ref)                                   # on again: the tables start at zero
    assert not any(t.any() for t in eng.errprof_tables())
    eng.errprof_enable(s.ref, s.mask_array(True))               # another mask on an engine that had none
    res = eng.process(s.batch(257))
    assert U.same(eng.errprof_tables(), U.tables(S.walked_segments(s.batch(257), res), s.ref, s.mask, MQ))


def test_last_ms_after_an_empty_batch_and_errors_before_the_first_enable():
    s = get_set("one")
    eng = s.fresh()
    eng.process(s.batch(65))
    assert eng.errprof_last_ms() > 0
    b, out = _device_batch(s.batch(65))
    eng.process_device(b.struct(), 0, _dev_out(out))
    eng.sync()
    assert eng.errprof_last_ms() > 0
    empty = b.struct()
    empty.n_reads = 0                                           # a device batch without reads launches nothing: nothing to ask for
    eng.process_device(empty, 0, _dev_out(out))
    eng.sync()
    with pytest.raises(lib.AmpliHipError) as err:
        eng.errprof_last_ms()
    assert err.value.rc == -5
    e = lib.Engine(500)
    for call in (e.errprof_tables, e.errprof_last_ms, lambda: e.errprof_add(*[np.zeros(s_, np.uint64) for s_ in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE, 2)])):
        with pytest.raises(lib.AmpliHipError) as err:
            call()
        assert err.value.rc == -5
    e.errprof_disable()                                         # off while off: nothing to do
    with pytest.raises(lib.AmpliHipError) as err:               # on without the reference's letters
        e._chk(e.L.amp_errprof_enable(e.h, 1, None, None), "amp_errprof_enable")
    assert err.value.rc == -1
    with pytest.raises(ValueError):
        e.errprof_enable("ACGT")
    e.close()


def test_hook_changes_neither_trim_results_nor_table_nor_events():
    s = get_set("example")
    batch = s.batch(20011)
    eng = s.fresh()
    eng.errprof_disable()
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


# ---- 5. device batches, the refusal, all hooks ------------------------------------------------------------------------------------
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
    eng.process(s.batch(1025))
    want = eng.errprof_tables()
    assert want[0].any()
    b, out = _device_batch(s.batch(1025))
    for drop in ((), ("ref_len", "trim_flags")):                # the hook needs neither ref_len nor trim_flags
        eng.reset()
        eng.process_device(b.struct(), 0, _dev_out(out, drop=drop))
        eng.sync()
        assert U.same(eng.errprof_tables(), want)


def test_a_trimming_pass_without_new_cig_is_refused_before_it_runs():
    s = get_set("example")
    eng = s.fresh()
    eng.process(s.batch(257))
    before, tables_before = eng.counts(), eng.errprof_tables()
    b, out = _device_batch(s.batch(1025))
    with pytest.raises(lib.AmpliHipError) as e:
        eng.process_device(b.struct(), 0, _dev_out(out, drop=("new_cig",)))
    assert e.value.rc == -1 and "the error profile needs" in str(e.value)
    eng.sync()
    assert np.array_equal(eng.counts(), before) and U.same(eng.errprof_tables(), tables_before)
    assert not any(v.any().item() for v in out.values())           # nothing ran
    eng.errprof_disable()
    eng.process_device(b.struct(), 0, None)                        # as before the hook existed
    eng.sync()


def test_all_seven_hooks_together_give_what_each_gives_alone():
    s = get_set("example")
    amps = A.example_amps()
    batch = s.batch(1025)
    sets = CO.mixed_sets(s.G)

    def engine(every):
        eng = lib.Engine(s.G)
        eng.set_primers(*s.tabs)
        eng.set_params(MQ, WINDOW, True, True)
        if every:
            eng.qc_enable(s.primers, 0, 30, False, [(0, s.G), (1000, 2000)], [1, 10, 100])
            eng.strand_enable()
            amps.enable(eng)
            codon.enable(eng, CU.overlapping(s.G))
            eng.del_enable()
            eng.cooc_enable(*sets.arrays())
        eng.errprof_enable(s.ref)
        res = eng.process(batch)
        return eng, res

    every, res_every = engine(True)
    alone, res_alone = engine(False)
    never = lib.Engine(s.G)
    never.set_primers(*s.tabs)
    never.set_params(MQ, WINDOW, True, True)
    res_never = never.process(batch)
    assert U.same(every.errprof_tables(), alone.errprof_tables()) and every.errprof_tables()[0].any()
    assert every.counts().tobytes() == alone.counts().tobytes() == never.counts().tobytes()
    order = ["ref_pos", "read", "q_from", "q_to"]
    assert np.array_equal(np.sort(every.events(), order=order), np.sort(never.events(), order=order))
    for k in ("new_pos", "new_ncig", "ref_len", "trim_flags", "status"):
        assert getattr(res_every, k).tobytes() == getattr(res_alone, k).tobytes() == getattr(res_never, k).tobytes(), k
    assert all(res_every.cigar_ops(i) == res_never.cigar_ops(i) for i in range(batch.n))
    assert every.strand_tables()[0].any() and every.cooc_tables()[0].any() and every.del_events()[0].size > 0
    for e in (every, alone, never):
        e.close()


# ---- 6. command line --------------------------------------------------------------------------------------------------------------
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST")
CLI_MIN_LENGTH = 30


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """The files of the job (the synthetic job of the codon tests), a mask as BED and as VCF, and the restatement's tables on
    the oracle's trim results: [do_trim][masked]."""
    from tests.test_gpu_cooc import write_reads
    d = tmp_path_factory.mktemp("errprof_cli")
    j = CU.synthetic_job()
    g, batch = j["genome"], U.with_mates(j["batch"], 3)
    G = int(g.size)
    ref_seq = synth.genome_string(g)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + ref_seq + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), j["primers"])
    mask = sorted({j["pa"], j["pa"] + 1, j["pb"], j["pb"] + 1, j["pc"], j["pc"] + 1, j["pc"] + 2})
    mask_bed = d / "mask.bed"; mask_bed.write_text("".join("SYN_REF\t%d\t%d\n" % (p, p + 1) for p in mask))
    mask_vcf = d / "mask.vcf"
    mask_vcf.write_text("##fileformat=VCFv4.2\n" + "".join("SYN_REF\t%d\t.\t%s\tA\n" % (p + 1, ref_seq[p:p + 2]) for p in (j["pa"], j["pb"])) +
                        "SYN_REF\t%d\t.\t%s\tA\n" % (j["pc"] + 1, ref_seq[j["pc"]:j["pc"] + 3]))
    files = dict(ref=str(ref), bed=str(bed), mask_bed=str(mask_bed), mask_vcf=str(mask_vcf), bam=write_reads(str(d / "in.bam"), "wb", batch, G),
                 sam=write_reads(str(d / "in.sam"), "w", batch, G))
    pr = sorted((s, e) for s, e, _ in j["primers"])
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    want = {}
    for do_trim in (True, False):           # aio counts the trimmed reads; variants and consensus take the file as it is
        r = oracle.process(batch, G, *(tabs if do_trim else (None, None, 0)), MQ, WINDOW, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        segs = S.walked_segments(batch, r.trim if do_trim else None)
        want[do_trim] = {masked: (U.tables(segs, ref_seq, mask if masked else None, MQ), r.counts) for masked in (False, True)}
    return files, want, ref_seq, len(mask)


def run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    amplipy.main(argv)


def switches(monkeypatch, **on):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in on:
        monkeypatch.setenv(k, "1")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check_outputs(json_path, vcf, plain_vcf, tabs_counts, n_masked, with_p=True):
    """The JSON is errprof.Tables' report of the restatement's tables; every VCF record ends in the two keys as errprof.Tables
    gives them for the restatement; with the keys and their header lines stripped the VCF is ``plain_vcf``."""
    tabs, counts = tabs_counts
    t = errprof.Tables(*tabs, MQ, n_masked, counts)
    text = open(json_path).read()
    assert json.loads(text) == t.report() and list(json.loads(text)) == list(t.report())
    if vcf is None:
        return t
    body = vcf.decode()
    assert errprof.HEADER_LINES in body
    out, n_num = [], 0
    for line in body.replace(errprof.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert kvs[-2].startswith("ERR_RATE=") and kvs[-1].startswith("ERR_P=")
            assert ";".join(kvs[-2:]) == t.info(int(f[1]) - 1, f[3], f[4].split(",")), line
            n_num += kvs[-1] != "ERR_P=."
            f[7] = ";".join(kvs[:-2])
            line = "\t".join(f)
        out.append(line + "\n")
    assert "".join(out).encode() == plain_vcf and n_num > 3
    return t


def test_aio_with_the_error_profile(tmp_path, job, monkeypatch, capfd):
    files, want, ref_seq, n_masked = job
    switches(monkeypatch)
    got = {}
    extras = {"plain": [], "ep": ["--error_profile", str(tmp_path / "ep.json")],
              "more": ["--strand", "--deletions"],
              "ep_more": ["--strand", "--deletions", "--error_profile", str(tmp_path / "ep_more.json"), "--error_mask", files["mask_bed"]]}
    for tag, extra in extras.items():
        base = ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        capfd.readouterr()
        run(monkeypatch, base + extra)
        log = capfd.readouterr().err
        assert ("Error profile: " in log) == ("ep" in tag)
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in (".bam", ".vcf", ".fas")]
    for tag, base, masked in (("ep", "plain", False), ("ep_more", "more", True)):
        assert got[tag][0] == got[base][0] and got[tag][2] == got[base][2] and len(got[base][0]) > 30000
        assert b"ERR_RATE" not in got[base][1]
        t = check_outputs(str(tmp_path / (tag + ".json")), got[tag][1], got[base][1], want[True][masked], n_masked if masked else 0)
    assert t.reads[0] > 1000 and 0 < t.totals()["rate"] < 0.2
    # the VCF of a first run as the mask of a second gives the BED's tables
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "v.vcf"), "--error_profile", str(tmp_path / "v.json"),
                      "--error_mask", files["mask_vcf"]])
    check_outputs(str(tmp_path / "v.json"), None, None, want[False][True], n_masked)
    # an existing report is refused like every other output; a mask without the profile; the profile on a run that only trims
    for argv in (["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "x.vcf"), "--error_profile", str(tmp_path / "ep.json")],
                 ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "y.vcf"), "--error_mask", files["mask_bed"]],
                 ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "z.bam"), "--error_profile", str(tmp_path / "z.json")]):
        with pytest.raises(SystemExit):
            run(monkeypatch, argv)


@pytest.mark.parametrize("route", ["host", "gpu_sam", "gpu_bam", "rccl"])
def test_variants_and_consensus_through_every_codec(tmp_path, job, monkeypatch, route):
    files, want, ref_seq, n_masked = job
    reads_in = files["sam"] if route == "gpu_sam" else files["bam"]
    on = {"gpu_sam": {"AMPLIPY_GPU_SAM": 1}, "gpu_bam": {"AMPLIPY_GPU_BAM": 1}, "rccl": {"AMPLIPY_FORCE_DIST": 1}}.get(route, {})
    switches(monkeypatch, **on)
    if route == "rccl":
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29557")
    run(monkeypatch, ["variants", "-i", reads_in, "-r", files["ref"], "-o", str(tmp_path / "plain.vcf")])
    run(monkeypatch, ["variants", "-i", reads_in, "-r", files["ref"], "-o", str(tmp_path / "ep.vcf"), "--error_profile", str(tmp_path / "ep.json")])
    check_outputs(str(tmp_path / "ep.json"), read(str(tmp_path / "ep.vcf")), read(str(tmp_path / "plain.vcf")), want[False][False], 0)
    run(monkeypatch, ["consensus", "-i", reads_in, "-r", files["ref"], "-o", str(tmp_path / "plain.fas")])
    run(monkeypatch, ["consensus", "-i", reads_in, "-r", files["ref"], "-o", str(tmp_path / "ep.fas"), "--error_profile", str(tmp_path / "c.json.gz"),
                      "--error_mask", files["mask_bed"]])
    assert read(str(tmp_path / "ep.fas")) == read(str(tmp_path / "plain.fas"))
    t = errprof.Tables(*want[False][True][0], MQ, n_masked)
    assert json.loads(gzip.open(str(tmp_path / "c.json.gz"), "rt").read()) == t.report()
