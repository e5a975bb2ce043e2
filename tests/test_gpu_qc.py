"""The amplicon QC report on the device (amp_qc.hip: k_qc_reads, k_qc_depth, k_qc_regions) against the
plain restatement of tests/qc_util.py, applied to the batch and the DEVICE's own trim results.  Batch sizes around a wave, a
block and past the first trip of the kernel's grid-stride loop; a primer set of one, the example BED with its duplicate rows,
and 40,000 primers (more counters than a block keeps in LDS: the global path); piles on one primer and reads on a primer each;
state across batches, reset, disable, the device-pointer form and runs without trimming; depth and regions on seeded tables.
Last, the command line with --qc on one synthetic file of 3,000 reads through every I/O route of run_amplipy -- the host codecs
and the five combinations of the device-codec switches its docstring lists: the report is the same JSON on every route and equals
the restatement, and trimmed reads, VCF and FASTA are byte for byte what the same command writes without --qc; then trim and
variants alone, --qc_depth_out, and one rank through RCCL."""
import gzip
import json
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, bamio, lib, synth
from amplipy_amd.batch import SEQ_NT16, unpack_nibbles
from tests import helpers as H
from tests import qc_util as Q

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1023, 1025, 20011]
MIN_LENGTH = 60


def example_primers():
    bed = [l.rstrip("\r\n").split("\t") for l in open(H.GOLDEN + "/data/example_primers.bed") if l.strip()]
    return sorted((int(f[1]), int(f[2])) for f in bed)


class PrimerSet:
    """One primer set: its engine (primer tables set, trimming and counting on) and its owners by the restatement."""

    def __init__(self, name):
        self.name = name
        self.G, self.primers = {"one": lambda: (2000, [(100, 130)]), "example": lambda: (29903, example_primers()),
                                "many": lambda: (200003, Q.many_primers(40000, 200003, 3))}[name]()
        self.mn, self.mx, self.mpl = lib.find_overlapping_primers(self.G, self.primers, 0)
        self.owners = Q.primer_owners(self.G, self.primers, 0)
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(self.mn, self.mx, self.mpl)
        self.eng.set_params(20, 4, True, True)
        self.batches = {}

    def batch(self, n, seed=None):
        key = (n, seed)
        if key not in self.batches:
            self.batches[key] = Q.mixed_batch(n, self.G, self.primers, 1000 + n if seed is None else seed)
        return self.batches[key]

    def enable(self, include_no_primer=False, regions=(), depths=()):
        self.eng.qc_enable(self.primers, 0, MIN_LENGTH, include_no_primer, regions, depths)

    def expect(self, batch, res, do_trim=True, include_no_primer=False):
        return Q.read_tallies(batch, res, self.G, do_trim, MIN_LENGTH, include_no_primer, self.owners, len(self.primers))


_SETS = {}


@pytest.fixture(params=["one", "example", "many"])
def pset(request):
    if request.param not in _SETS:
        _SETS[request.param] = PrimerSet(request.param)
    s = _SETS[request.param]
    s.eng.set_params(20, 4, True, True)
    s.eng.reset()
    return s


def example_set():
    if "example" not in _SETS:
        _SETS["example"] = PrimerSet("example")
    s = _SETS["example"]
    s.eng.set_params(20, 4, True, True)
    s.eng.reset()
    return s


def assert_tallies(got, want, what=""):
    assert got[0] == want[0], what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


def test_example_bed_has_the_duplicates_the_owners_rule_is_about():
    pr = example_primers()
    assert len(pr) == 690 and len(set(pr)) < len(pr)
    assert 2 * 40000 > lib_lds_counters() >= 2 * 690


def lib_lds_counters():
    """QC_LDS_COUNTERS of amp_qc.hpp."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "amplipy_amd", "csrc", "amp_qc.hpp")).read()
    return int(re.search(r"constexpr int QC_LDS_COUNTERS = (\d+);", text).group(1))


# ---- 4. read tallies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_read_tallies(pset, n):
    batch = pset.batch(n)
    pset.enable()
    res = pset.eng.process(batch)
    want = pset.expect(batch, res)
    assert_tallies(pset.eng.qc_read_tallies(), want, (pset.name, n))
    t = want[0]
    assert t["rows"] == n and t["errors"] == (1 if n >= 8 else 0)       # the read past the reference, and only it
    assert t["kept"] + t["dropped_short"] + t["dropped_no_primer"] == n - t["errors"]
    if n >= 1023:           # the mix is there
        assert all(t[k] > 0 for k in abi.QC_READ_FIELDS if k != "primer_both" or pset.name != "one")
        assert int(want[1].sum()) == t["primer_start"] and int(want[2].sum()) == t["primer_end"]
        if pset.name != "one":
            assert int((want[1] > 0).sum()) > 100 and int((want[2] > 0).sum()) > 100
        ops = np.diff(batch.cig_off)
        assert ops.max() >= 40 and (batch.flag & 0x11 == 0x11).any()
        assert (res.trim_flags[(batch.flag & 0x11) == 0x11] & 1 == 0).all()          # the insert-size rule kept their start
    if n:
        assert pset.eng.qc_last_ms() > 0


def test_include_no_primer_moves_the_dropped_to_kept(pset):
    batch = pset.batch(1025)
    pset.enable(include_no_primer=True)
    res = pset.eng.process(batch)
    want = pset.expect(batch, res, include_no_primer=True)
    assert want[0]["dropped_no_primer"] == 0 and want[0]["primer_none"] > 0
    assert_tallies(pset.eng.qc_read_tallies(), want)


@pytest.mark.parametrize("kind", ["one_primer", "a_primer_each"])
def test_extreme_piles(kind):
    """20,000 reads that all start on one primer (every lane of every wave carries the same owner: one run per wave), and 20,000
    reads each on a primer of its own (no two neighbouring lanes agree: every lane is a run head), the latter on the 40,000
    primer set: the global path."""
    if kind == "one_primer":
        s = example_set()
        batch = Q.pile_batch(20000, [s.primers[40][0] + 2], 120, 7)
    else:
        if "many" not in _SETS:
            _SETS["many"] = PrimerSet("many")
        s = _SETS["many"]
        s.eng.reset()
        batch = Q.pile_batch(20000, [5 * k + 1 for k in range(20000)], 120, 8)
    s.enable()
    res = s.eng.process(batch)
    want = s.expect(batch, res)
    assert want[0]["primer_start"] == 20000
    assert int((want[1] > 0).sum()) == (1 if kind == "one_primer" else 20000)
    assert_tallies(s.eng.qc_read_tallies(), want)


def test_shuffled_batch_gives_the_same_tallies(pset):
    batch = pset.batch(20011)
    perm = np.random.default_rng(5).permutation(batch.n)
    shuffled = synth.gather_rows(batch, perm)
    pset.enable()
    pset.eng.process(batch)
    sorted_t = pset.eng.qc_read_tallies()
    pset.eng.reset()
    res = pset.eng.process(shuffled)
    assert (np.diff(shuffled.pos) < 0).any()
    assert_tallies(pset.eng.qc_read_tallies(), pset.expect(shuffled, res))
    assert_tallies(pset.eng.qc_read_tallies(), sorted_t)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def test_tallies_accumulate_reset_and_stop_when_disabled():
    s = example_set()
    s.enable()
    total = None
    for n in (65, 1025, 300):
        batch = s.batch(n)
        res = s.eng.process(batch)
        w = s.expect(batch, res)
        total = w if total is None else Q.add_tallies(total, w)
        assert_tallies(s.eng.qc_read_tallies(), total, n)
    s.eng.reset()
    t, ps, pe = s.eng.qc_read_tallies()
    assert not any(t.values()) and not ps.any() and not pe.any()
    batch = s.batch(300)
    res = s.eng.process(batch)
    once = s.expect(batch, res)
    assert_tallies(s.eng.qc_read_tallies(), once)
    s.eng.qc_disable()
    s.eng.process(s.batch(1025))
    s.eng.process(batch)
    assert_tallies(s.eng.qc_read_tallies(), once)          # what was tallied stays readable, nothing was added


def _device_run(s, batch):
    import torch
    from amplipy_amd import synth_torch
    n = batch.n
    b = synth_torch.DeviceBatch.from_host(batch, "cuda:0")
    out = {k: torch.zeros(max(sz, 1), dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", b.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    dev_out = abi.AmpTrimOut(*[out[k].data_ptr() for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")])
    s.eng.process_device(b.struct(), 0, dev_out)
    s.eng.sync()
    return b, {k: v.cpu().numpy() for k, v in out.items()}


def test_process_device_gives_the_same_tallies():
    s = example_set()
    batch = s.batch(1025)
    s.enable()
    res = s.eng.process(batch)
    host_form = s.eng.qc_read_tallies()
    assert_tallies(host_form, s.expect(batch, res))
    s.eng.reset()
    b, out = _device_run(s, batch)
    assert np.array_equal(out["trim_flags"], res.trim_flags) and np.array_equal(out["status"], res.status)
    assert_tallies(s.eng.qc_read_tallies(), host_form)
    # the report needs the pass's results: a trimming pass without them is refused before anything runs
    before = s.eng.counts()
    with pytest.raises(lib.AmpliHipError) as e:
        s.eng.process_device(b.struct(), 0, None)
    assert e.value.rc == -1
    s.eng.sync()
    assert np.array_equal(s.eng.counts(), before)
    assert_tallies(s.eng.qc_read_tallies(), host_form)
    s.eng.qc_disable()
    s.eng.process_device(b.struct(), 0, None)           # as before the report existed
    s.eng.sync()


def test_without_trimming_only_rows_errors_and_bases_in():
    s = example_set()
    s.eng.set_params(20, 4, False, True)
    batch = s.batch(1025)
    s.enable()
    res = s.eng.process(batch)
    want = s.expect(batch, res, do_trim=False)
    assert want[0]["errors"] == 1 and want[0]["ref_bases_in"] > 0
    assert all(want[0][k] == 0 for k in abi.QC_READ_FIELDS if k not in ("rows", "errors", "ref_bases_in"))
    assert not want[1].any() and not want[2].any()
    assert_tallies(s.eng.qc_read_tallies(), want)
    # ... and no primers at all: the report of a `variants` run
    s.eng.reset()
    s.eng.qc_enable((), 0, MIN_LENGTH, False, [(0, s.G)], [1])
    s.eng.process(batch)
    got = s.eng.qc_read_tallies()
    assert got[0] == want[0] and got[1].size == 0 and got[2].size == 0


def test_report_changes_neither_trim_results_nor_table():
    s = example_set()
    batch = s.batch(20011, seed=77)
    s.eng.qc_disable()
    off = s.eng.process(batch)
    table_off = s.eng.counts()
    events_off = np.sort(s.eng.events(), order=["ref_pos", "read", "q_from", "q_to"])
    s.eng.reset()
    s.enable(regions=[(0, s.G)], depths=[1, 10])
    on = s.eng.process(batch)
    for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status"):
        assert getattr(on, k).tobytes() == getattr(off, k).tobytes(), k
    assert s.eng.counts().tobytes() == table_off.tobytes()
    assert np.array_equal(np.sort(s.eng.events(), order=["ref_pos", "read", "q_from", "q_to"]), events_off)


def test_enable_needs_primers_when_trimming():
    e = lib.Engine(500)
    e.set_params(20, 4, True, False)
    with pytest.raises(lib.AmpliHipError) as err:
        e.qc_enable([(10, 30)], 0, 30, False)
    assert err.value.rc == -5
    with pytest.raises(lib.AmpliHipError):          # no report yet: nothing to read
        e.qc_read_tallies()
    e.close()


# ---- 6. depth and regions ---------------------------------------------------------------------------------------------------
def regions_for(G):
    rng = np.random.default_rng(G)
    r = [(0, G), (5, 5), (9, 3), (0, 1), (G - 1, G), (-10, 7), (G - 3, G + 50), (G, G + 5), (-20, -3)]
    for L in (1, 63, 64, 65):
        a = int(rng.integers(0, max(G - L, 1)))
        r.append((a, a + L))
    r += [(10, 200), (100, 300), (150, 160)]                       # overlapping
    while len(r) < 300:                                            # 300 regions: more than one trip per block is not needed, more than one block is
        a = int(rng.integers(-5, G)); r.append((a, a + int(rng.integers(0, 400))))
    return r


DEPTH_SETS = [[], [0], [1, 10, 100, 4294967295]]


@pytest.mark.parametrize("G", [1, 255, 256, 257, 70003])
def test_depth_and_regions(G):
    e = lib.Engine(G)
    e.set_params(20, 4, False, True)          # (a table alone: nothing trims)
    counts = Q.seeded_counts(G, G)
    e.add_counts(counts)
    want_depth = Q.depth_of(counts)
    for regions in ([(0, G)], regions_for(G)):
        for depths in DEPTH_SETS:
            e.qc_enable((), 0, 30, False, regions, depths)
            depth, got = e.qc_depth()
            assert np.array_equal(depth, want_depth)
            Q.assert_regions(got, Q.region_stats(want_depth, regions, depths), len(depths))
            assert np.array_equal(e.qc_depth(want_depth=False)[1], got)          # no atomics: the same bytes every time
    assert e.counts().tobytes() == counts.tobytes()
    e.close()


def test_depth_sum_beyond_32_bits():
    G = 70003
    e = lib.Engine(G)
    e.set_params(20, 4, False, True)
    counts = np.zeros((G, abi.NSYM), np.uint32)
    counts[:, :4] = 25000
    e.add_counts(counts)
    e.qc_enable((), 0, 30, False, [(0, G), (1, G - 1)], [100000, 100001])
    depth, got = e.qc_depth()
    assert (depth == 100000).all()
    assert int(got["depth_sum"][0]) == 100000 * G > 2 ** 32
    Q.assert_regions(got, Q.region_stats(Q.depth_of(counts), [(0, G), (1, G - 1)], [100000, 100001]), 2)
    assert [int(x) for x in got["covered"][0][:2]] == [G, 0]
    e.close()


# ---- 7. command line -----------------------------------------------------------------------------------------------------------
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST")
CLI_MIN_LENGTH, DEPTHS = 30, [1, 10, 100]
# (name, input, trimmed output, gpu_sam, gpu_bam, gpu_bam_write)
ROUTES = [("host", "bam", "bam", False, False, False), ("sam", "sam", "sam", True, False, False), ("sam_bam", "sam", "bam", True, False, True),
          ("bam", "bam", "bam", False, True, False), ("bam_bam", "bam", "bam", False, True, True), ("bam_sam", "bam", "sam", True, True, False)]


def write_reads(path, mode, hb, G):
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
    """The files of the job and what the report must say, by the restatement on the device's own trim results and table."""
    d = tmp_path_factory.mktemp("qc_cli")
    g = synth.make_genome()
    G = int(g.size)
    primers, amps = synth.make_artic_scheme()
    rows = sorted(primers, key=lambda p: (p[0], p[1]))
    pr = [(s, e) for s, e, _ in rows]
    batch = Q.mixed_batch(3000, G, pr, 31, bad_read=False)
    ref = d / "ref.fas"; ref.write_text(">SYN_REF test\n" + synth.genome_string(g) + "\n")
    bed = d / "p.bed"; synth.write_bed(str(bed), primers)
    regions = [(int(a[2]), int(a[3]), "insert%d" % k) for k, a in enumerate(amps[:12])] + [(G - 50, G + 70, "tail"), (40, 40, "empty")]
    rbed = d / "r.bed"; rbed.write_text("".join("SYN_REF\t%d\t%d\t%s\n" % r for r in regions))
    files = dict(ref=str(ref), bed=str(bed), rbed=str(rbed), bam=write_reads(str(d / "in.bam"), "wb", batch, G),
                 sam=write_reads(str(d / "in.sam"), "w", batch, G))
    # expectation
    mn, mx, mpl = lib.find_overlapping_primers(G, pr, 0)
    want = {}
    for do_trim in (True, False):
        e = lib.Engine(G)
        e.set_primers(mn, mx, mpl); e.set_params(20, 4, do_trim, True)
        res = e.process(batch)
        assert not res.status.any()
        t, ps, pe = Q.read_tallies(batch, res, G, do_trim, CLI_MIN_LENGTH, False, Q.primer_owners(G, pr, 0), len(pr))
        depth = Q.depth_of(e.counts())
        e.close()
        all_regions = [(0, G, "*")] + regions
        reg = [dict(name=name, start=w["start"], end=w["end"], length=w["length"], depth_sum=w["depth_sum"],
                    depth_mean=w["depth_sum"] / w["length"] if w["length"] else 0.0, depth_min=w["depth_min"], depth_max=w["depth_max"],
                    covered={str(k): c for k, c in zip(DEPTHS, w["covered"])})
               for (_, _, name), w in zip(all_regions, Q.region_stats(depth, [(s, e_) for s, e_, _ in all_regions], DEPTHS))]
        want[do_trim] = dict(reads=t if do_trim else {k: t[k] for k in ("rows", "errors", "ref_bases_in")}, depth=depth, regions=reg,
                             primers=[dict(name=name, start=s, end=e_, reads_start=int(a), reads_end=int(b)) for (s, e_, name), a, b in zip(rows, ps, pe)])
    assert want[True]["reads"]["kept"] > 1000 and sum(p["reads_start"] for p in want[True]["primers"]) > 1000
    return files, want, G


def run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])        # (@PG and ##source record the command line)
    amplipy.main(argv)


def switches(monkeypatch, gpu_sam=False, gpu_bam=False, gpu_bam_write=False, dist=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, on in (("AMPLIPY_GPU_SAM", gpu_sam), ("AMPLIPY_GPU_BAM", gpu_bam), ("AMPLIPY_GPU_BAM_WRITE", gpu_bam_write), ("AMPLIPY_FORCE_DIST", dist)):
        if on:
            monkeypatch.setenv(k, "1")


def read(path):
    with open(path, "rb") as f:
        return f.read()


_REPORTS = {}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_aio_with_qc_on_every_route(tmp_path, job, monkeypatch, route):
    files, want, G = job
    name, inp, out, gpu_sam, gpu_bam, gpu_bam_write = route
    switches(monkeypatch, gpu_sam, gpu_bam, gpu_bam_write)
    got = {}
    for tag in ("plain", "qc"):
        base = ["aio", "-i", files[inp], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + "." + out)),
                "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH)]
        run(monkeypatch, base + (["--qc", str(tmp_path / "qc.json"), "--qc_regions", files["rbed"]] if tag == "qc" else []))
        got[tag] = [read(str(tmp_path / (tag + ext))) for ext in ("." + out, ".vcf", ".fas")]
    assert got["qc"] == got["plain"]
    assert len(got["qc"][0]) > 100000 and got["qc"][1].count(b"\n") > 12
    text = read(str(tmp_path / "qc.json")).decode()
    rep = json.loads(text)
    assert list(rep) == ["amplipy_qc", "params", "reads", "primers", "regions"] and rep["amplipy_qc"] == 1
    assert rep["params"] == dict(primer_pos_offset=0, min_length=CLI_MIN_LENGTH, include_no_primer=False, depths=DEPTHS)
    w = want[True]
    assert rep["reads"] == w["reads"] and list(rep["reads"]) == list(Q.READ_FIELDS)
    assert rep["primers"] == w["primers"]
    assert rep["regions"] == w["regions"]
    assert list(rep["regions"][0]) == ["name", "start", "end", "length", "depth_sum", "depth_mean", "depth_min", "depth_max", "covered"]
    _REPORTS[name] = text
    assert all(t == text for t in _REPORTS.values())          # the same file on every route run so far


def test_trim_alone_has_no_regions_and_refuses_the_depth_file(tmp_path, job, monkeypatch, capsys):
    files, want, G = job
    switches(monkeypatch)
    run(monkeypatch, ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "t.bam"), "-ml", str(CLI_MIN_LENGTH),
                      "--qc", str(tmp_path / "t.json")])
    rep = json.load(open(str(tmp_path / "t.json")))
    assert list(rep) == ["amplipy_qc", "params", "reads", "primers"]
    assert rep["reads"] == want[True]["reads"] and rep["primers"] == want[True]["primers"]
    with pytest.raises(SystemExit):
        run(monkeypatch, ["trim", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-o", str(tmp_path / "t2.bam"),
                          "--qc_depth_out", str(tmp_path / "t2.tsv")])
    assert "no count table" in capsys.readouterr().err


@pytest.mark.parametrize("ext", [".tsv", ".tsv.gz"])
def test_variants_alone_has_no_primers_and_writes_the_depth_file(tmp_path, job, monkeypatch, ext):
    files, want, G = job
    switches(monkeypatch)
    dfn = str(tmp_path / ("d" + ext))
    run(monkeypatch, ["variants", "-i", files["bam"], "-r", files["ref"], "-o", str(tmp_path / "v.vcf"), "--qc", str(tmp_path / "v.json"),
                      "--qc_regions", files["rbed"], "--qc_depths", "1,10,100", "--qc_depth_out", dfn])
    rep = json.load(open(str(tmp_path / "v.json")))
    w = want[False]
    assert list(rep) == ["amplipy_qc", "params", "reads", "regions"] and rep["params"] == dict(depths=DEPTHS)
    assert rep["reads"] == w["reads"] and list(rep["reads"]) == ["rows", "errors", "ref_bases_in"]
    assert rep["regions"] == w["regions"]
    lines = (gzip.open(dfn, "rt") if ext.endswith(".gz") else open(dfn)).read().splitlines()
    assert lines == ["SYN_REF\t%d\t%d" % (p + 1, d) for p, d in enumerate(w["depth"].tolist())]


def test_one_rank_through_rccl_gives_the_same_report(tmp_path, job, monkeypatch):
    files, want, G = job
    texts = {}
    for tag, dist in (("plain", False), ("dist", True)):
        switches(monkeypatch, dist=dist)
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", "29547")
        run(monkeypatch, ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", str(tmp_path / (tag + ".bam")),
                          "-ov", str(tmp_path / (tag + ".vcf")), "-oc", str(tmp_path / (tag + ".fas")), "-ml", str(CLI_MIN_LENGTH),
                          "--qc", str(tmp_path / (tag + ".json")), "--qc_regions", files["rbed"]])
        texts[tag] = read(str(tmp_path / (tag + ".json")))
    assert texts["dist"] == texts["plain"]
    assert json.loads(texts["plain"])["reads"] == want[True]["reads"]
