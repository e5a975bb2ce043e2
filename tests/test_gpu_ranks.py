"""The command line under two and three ranks with every report on, on ONE card (amplipy.run_amplipy's multi-rank path: the
file cut by pieces or the text dealt out, the seams, one all-reduce of the count table and one per report, the object gathers,
the join of the ranks' trimmed BAMs, rank 0 writing every output).  Every rank is a fresh child process running
tests/rank_worker.py, which initialises torch.distributed with gloo -- ranks cannot share a card under RCCL -- and calls
amplipy.main; behind that everything is the product's own code on the real kernels.  RCCL with more than one rank stays
unmeasured.

Which all-reduce ran: the product's own.  This torch's gloo takes the device tensors that run_amplipy hands to
parallel.allreduce_table (every child of every case logged "gloo takes them"), so the worker replaced nothing; its stand-in
that sums a host copy has not run.  (a) asserts that all ranks of a run log the same arrangement.

The job is the synthetic job of the codon, co-occurrence and error-profile command-line tests (codon_util.synthetic_job with
errprof_util.with_mates(..., 3), written by test_gpu_cooc.write_reads; about 3000 reads in six piles on three amplicons) with
one more construction: at PI, 20 bases behind the deleted codon, about 40 % of the single-M reads that reach it carry the
insertion "GT", so that an insertion allele is called in a pile.  Three files hold it: ``plain`` (as generated, by coordinate),
``turned`` (the same reads, the last pile moved to the front: the middle of a two-rank run then lies in the pile with the
constructions, which is a sixth of the reads and cannot hold the cut of two ranks and a cut of three at once) and ``thin``
(every 15th read: one BGZF block).

THE REFERENCE of every multi-rank run is the one-process run (no WORLD_SIZE, no AMPLIPY_FORCE_DIST) of the same command on the
same files in the same session, in this process.  Its files are what each report's own command-line test pins against its
plain restatement; test_one_process_reference_is_the_restatements repeats that for the error-profile JSON and the --cooc_out
table of this job.  Text outputs are compared byte for byte, the joined BAM by its inflated bytes and its EOF block.

(a) test_every_report_bam_in_bam_out: aio, BAM in, BAM out, all nine reports and every table file; world 2 on ``turned`` and
    world 3 on ``plain`` with two pieces per rank, world 3 on ``plain`` with one piece per rank (AMPLIPY_PART_BYTES larger than
    the file: native_parts never makes fewer pieces than ranks, so every rank still has a third of the file).  Every child
    exits 0, no .partN.bam is left, the directory holds the one-process run's files and nothing else, and no rank but 0
    opened a file there for writing (the worker logs every such open).
(b) Reach conditions of (a), from the rank-0 log line "Shares of the N ranks: records [...]" and the input batch alone: every
    share is non-empty, the shares add up to the file, at least one cut falls inside a pile (the last read of rank r and the
    first of rank r+1 overlap on the reference), and the reads with A at PA (a called variant), with AAG at PA (a codon with
    ALT_AA), with the deletion (PC, 3), with the insertion at PI (an insertion-flagged position) and with both the deletion and
    A at PA (the complete pattern 11 of set del_and_sub) each lie on at least two ranks.  That the one-process outputs show each
    of the five is asserted too.
(c) test_text_in_world_2: the same command with -i in.sam; PythonDriver deals the reads out, every pile is split on every
    read.  VCF, FASTA and every report as one process; the trimmed reads are what the code does today: out.part0.bam and
    out.part1.bam, whose records together are the one-process out.bam's as a multiset, and no out.bam.
(d) test_variants_and_consensus_alone_world_2: the untrimmed BAM with --strand --deletions --readpos --codons --cooc --error_profile
    --haplotypes (consensus: the table files in place of the three VCF flags); do_trim is off and the hooks read the input CIGAR.  Reach:
    both shares non-empty.
(e) test_ranks_with_an_empty_share_world_3: ``thin`` has one block of records, so at world 3 two ranks run with every report
    on and never process a batch: a shares line with two zeros, exit 0 everywhere, the one-process files.  (The full job cannot
    give an empty share by a large AMPLIPY_PART_BYTES: that is (a)'s third case.)
(f) test_one_rank_fails_in_front_of_the_collective: a directory where rank 1's out.part1.bam should go, and -- once -- a joined
    out.bam that exists beforehand: both children end inside the limit with a non-zero status, both logs name the failing
    rank and its reason, rank 0 leaves no VCF record and no consensus behind.

The children: at most three, started with subprocess.Popen, waited for under ONE limit and killed behind it; nothing is tried
twice.  A child killed at the limit, or one that ends with 134, 139, -6 or -11, fails the test with its log, and no test of
the module starts a child after that.
"""
import collections
import contextlib
import gzip
import io
import json
import os
import re
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from amplipy_amd import amplipy, bam_native, bamio, cooc, errprof, synth
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import codon_util as CU
from tests import cooc_util as CO
from tests import errprof_util as U
from tests import strand_util as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rank_worker.py")
MQ, WINDOW, CLI_MIN_LENGTH = 20, 4, 30
# The one-process run of command (a) as a child process that, like every rank's child and like this session, has torch loaded
# and the device initialised by it before the run, took 2.32, 2.42 and 2.36 s on an MI355X machine (the bare command line
# imports no torch at all and took 0.62 and 0.47 s: ten times that would bound torch's import, not the run).  The children's
# limit and the collectives' timeout are ten times the middle figure; a world of three took 2.0 to 3.0 s.
ONE_PROCESS_SECONDS = 2.36
LIMIT = 10 * ONE_PROCESS_SECONDS
CRASHED = (134, 139, -6, -11)
CLEARED = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_FORCE_DIST", "AMPLIPY_PART_BYTES",
           "AMPLIPY_PYTHON_BAM", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
TEXT_OUTPUTS = ("out.vcf", "out.fas", "q.json", "d.tsv", "s.tsv", "a.tsv", "c.tsv", "aa.tsv", "del.tsv", "indel.vcf", "co.tsv", "ep.json", "hap.tsv", "rp.tsv")
_STOPPED = []                      # why no further children are started


# ---- the launcher ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def run_ranks(world, cwd, argv, part_bytes=None):
    """One job under ``world`` ranks in directory ``cwd`` -> ([exit status], [log])."""
    assert 1 < world <= 3
    if _STOPPED:
        pytest.fail("no further children: " + _STOPPED[0])
    env = {k: v for k, v in os.environ.items() if k not in CLEARED}
    port = _free_port()
    logs = [tempfile.TemporaryFile() for _ in range(world)]
    procs = []
    try:
        for rank in range(world):
            cmd = [sys.executable, WORKER, "--rank", str(rank), "--world", str(world), "--port", str(port), "--timeout", str(LIMIT)]
            cmd += ["--part-bytes", str(part_bytes)] if part_bytes is not None else []
            procs.append(subprocess.Popen(cmd + ["--"] + list(argv), cwd=str(cwd), env=env, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=logs[rank]))
        deadline = time.monotonic() + LIMIT
        for p in procs:
            try:
                p.wait(timeout=max(0.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                pass
    finally:
        late = [r for r, p in enumerate(procs) if p.poll() is None]
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    texts = []
    for f in logs:
        f.seek(0); texts.append(f.read().decode(errors="replace")); f.close()
    status = [p.returncode for p in procs]
    if late or any(s in CRASHED for s in status):
        _STOPPED.append("ranks %s of %s were killed at the limit of %.0f s, exit statuses %s" % (late, list(argv[:1]), LIMIT, status))
        pytest.fail(_STOPPED[0] + "".join("\n---- rank %d ----\n%s" % (r, t) for r, t in enumerate(texts)))
    return status, texts


def one_process(cwd, argv):
    """The reference: the same command in this process, with nothing of a multi-rank run in the environment.  -> its log."""
    saved = sys.argv, os.getcwd(), {k: os.environ.get(k) for k in CLEARED}
    log = io.StringIO()
    try:
        sys.argv = ["amplipy_amd", "pinned"]                  # (@PG and ##source record the command line)
        os.chdir(str(cwd))
        for k in CLEARED:
            os.environ.pop(k, None)
        with contextlib.redirect_stderr(log):
            amplipy.main(list(argv))
        return log.getvalue()
    finally:
        sys.argv = saved[0]
        os.chdir(saved[1])
        for k, v in saved[2].items():
            if v is not None:
                os.environ[k] = v


# ---- the job --------------------------------------------------------------------------------------------------------------------
INSERTED = "GT"


def _bases_at(seg, positions):
    """{reference position: the read's base there} for the match bases of ``seg`` at ``positions``."""
    return {r: seg.query_sequence[q] for q, r in seg.get_aligned_pairs() if q is not None and r in positions}


def _plant_insertion(batch, pi, seed):
    """The batch with INSERTED behind reference position ``pi`` on about 40 % of the single-M reads that reach 6 bases to either
    side of it; order, positions and flags stay."""
    rng = np.random.default_rng(seed)
    segs = []
    for i in range(batch.n):
        s = batch.segment(i)
        ops = s.cigartuples
        if rng.random() < 0.4 and len(ops) == 1 and s.reference_start <= pi - 6 and s.reference_start + ops[0][1] >= pi + 7:
            cut = pi + 1 - s.reference_start
            s.cigartuples = [(0, cut), (1, len(INSERTED)), (0, ops[0][1] - cut)]
            s.query_sequence = s.query_sequence[:cut] + INSERTED + s.query_sequence[cut:]
            quals = list(s.query_qualities)
            s.query_qualities = type(s.query_qualities)("B", quals[:cut] + [35] * len(INSERTED) + quals[cut:])
        segs.append(s)
    return ReadBatch.from_segments(segs)


def _carriers(batch, pa, pc, pi):
    """Per construction, which reads of the batch carry it (bool arrays in file order), from the reads alone."""
    kinds = {k: np.zeros(batch.n, bool) for k in ("variant", "codon", "deletion", "insertion", "pattern")}
    for i in np.nonzero((batch.pos.astype(np.int64) > pa - 400) & (batch.pos.astype(np.int64) <= pi))[0].tolist():
        s = batch.segment(i)
        at = _bases_at(s, {pa, pa + 1, pa + 2})
        r, dels, ins = s.reference_start, set(), set()
        for op, n in s.cigartuples:
            if op == 2:
                dels.add((r, n))
            if op == 1:
                ins.add(r - 1)
            if op in (0, 2, 3, 7, 8):
                r += n
        kinds["variant"][i] = at.get(pa) == "A"
        kinds["codon"][i] = [at.get(pa + k) for k in range(3)] == list("AAG")
        kinds["deletion"][i] = (pc, 3) in dels
        kinds["insertion"][i] = pi in ins
        kinds["pattern"][i] = (pc, 3) in dels and at.get(pa) == "A"
    return kinds


class Job:
    def __init__(self, d):
        from tests.test_gpu_cooc import write_reads
        j = CU.synthetic_job()
        self.pa, self.pb, self.pc = j["pa"], j["pb"], j["pc"]
        self.pi = self.pc + 20
        g = j["genome"]
        self.G = G = int(g.size)
        self.ref_seq = ref_seq = synth.genome_string(g)
        plain = U.with_mates(_plant_insertion(j["batch"], self.pi, 5), 3)
        pos = plain.pos.astype(np.int64)
        last_pile = int(np.searchsorted(pos, pos[-1] - 20))                 # the reverse reads of the third amplicon
        order = {"plain": np.arange(plain.n), "turned": np.concatenate([np.arange(last_pile, plain.n), np.arange(last_pile)]),
                 "thin": np.arange(0, plain.n, 15)}
        self.batch = {tag: plain if tag == "plain" else synth.gather_rows(plain, idx) for tag, idx in order.items()}
        carriers = _carriers(plain, self.pa, self.pc, self.pi)
        self.carriers = {tag: {k: m[idx] for k, m in carriers.items()} for tag, idx in order.items()}
        self.bam = {tag: write_reads(str(d / (tag + ".bam")), "wb", b, G) for tag, b in self.batch.items()}
        self.sam = write_reads(str(d / "plain.sam"), "w", plain, G)
        put = lambda name, text: (d / name).write_text(text) and str(d / name)
        self.ref = put("ref.fas", ">SYN_REF test\n" + ref_seq + "\n")
        self.bed = str(d / "p.bed"); synth.write_bed(self.bed, j["primers"])
        n_amp = len(j["primers"]) // 2
        self.pairs = put("amplicons.tsv", "".join("SYN_%d_LEFT\tSYN_%d_RIGHT\tSYN_%d\n" % (k, k, k) for k in range(1, n_amp + 1)))
        self.cds = put("cds.tsv", "".join("%s\t%d\t%d\t%s\n" % r for r in j["rows"]))
        _, amps = synth.make_artic_scheme()
        far = int(amps[11, 0]) + 200                          # inside the third amplicon only: no read shows it and PA together
        self.sets_text = ("del_and_sub\tdel%d-%d,C%dA\n" % (self.pc + 1, self.pc + 3, self.pa + 1) +
                          "two_amplicons\tC%dA,%s%d%s\n" % (self.pa + 1, ref_seq[far], far + 1, "A" if ref_seq[far] != "A" else "C"))
        self.sets = put("sets.tsv", self.sets_text)
        self.mask_positions = sorted({self.pa, self.pa + 1, self.pb, self.pb + 1, self.pc, self.pc + 1, self.pc + 2})
        self.mask = put("mask.bed", "".join("SYN_REF\t%d\t%d\n" % (p, p + 1) for p in self.mask_positions))
        regions = [(int(a[2]), int(a[3]), "insert%d" % k) for k, a in enumerate(amps[9:12])] + [(G - 50, G + 70, "tail"), (40, 40, "empty")]
        self.regions = put("r.bed", "".join("SYN_REF\t%d\t%d\t%s\n" % r for r in regions))
        # the regions of --haplotypes: the three inserts (no read spans one: their reads are "other reads") and 45 positions round
        # the deletion and the insertion, which whole reads cover
        self.hap_regions = put("h.bed", "".join("SYN_REF\t%d\t%d\t%s\n" % r for r in regions[:3] + [(self.pc - 20, self.pc + 25, "site")]))
        self.primers = sorted((s, e) for s, e, _ in j["primers"])
        self.dir = d
        self._refs, self.logs = {}, {}

    def aio(self, reads):
        return ["aio", "-i", reads, "-p", self.bed, "-r", self.ref, "-ot", "out.bam", "-ov", "out.vcf", "-oc", "out.fas", "-ml", str(CLI_MIN_LENGTH),
                "--qc", "q.json", "--qc_regions", self.regions, "--qc_depth_out", "d.tsv", "--strand", "--strand_out", "s.tsv",
                "--amplicons", self.pairs, "--amplicon_out", "a.tsv", "--codons", self.cds, "--codon_out", "c.tsv", "--aa_out", "aa.tsv",
                "--deletions", "--del_out", "del.tsv", "--indel_vcf", "indel.vcf", "--cooc", self.sets, "--cooc_out", "co.tsv",
                "--error_profile", "ep.json", "--error_mask", self.mask, "--haplotypes", self.hap_regions, "--hap_out", "hap.tsv",
                "--readpos", "--readpos_out", "rp.tsv"]

    def alone(self, command):
        """variants or consensus on the untrimmed BAM with every report such a run can have."""
        more = ["--codons", self.cds, "--codon_out", "c.tsv", "--cooc", self.sets, "--cooc_out", "co.tsv", "--error_profile", "ep.json", "--del_out", "del.tsv",
                "--strand_out", "s.tsv", "--haplotypes", self.hap_regions, "--hap_out", "hap.tsv", "--readpos_out", "rp.tsv"]
        if command == "variants":
            return ["variants", "-i", self.bam["plain"], "-r", self.ref, "-o", "out.vcf", "--strand", "--deletions", "--readpos"] + more
        return ["consensus", "-i", self.bam["plain"], "-r", self.ref, "-o", "out.fas"] + more

    def reference(self, tag, argv):
        """The directory of the one-process run of ``argv`` (run once)."""
        if tag not in self._refs:
            if _STOPPED:
                pytest.fail("nothing further on the GPU: " + _STOPPED[0])
            d = self.dir / ("one_" + tag)
            d.mkdir()
            self.logs[tag] = one_process(d, argv)
            self._refs[tag] = d
        return self._refs[tag]


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return Job(tmp_path_factory.mktemp("ranks"))


def read(path):
    with open(str(path), "rb") as f:
        return f.read()


def vcf_records(text):
    """{0-based position: (ALT list, INFO dict)} of a VCF's records."""
    recs = {}
    for line in text.splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            recs[int(f[1]) - 1] = (f[4].split(","), dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv))
    return recs


def shares_of(log, world):
    m = re.search(r"Shares of the (\d+) ranks: records \[([^\]]*)\]", log)
    assert m and int(m.group(1)) == world, log
    return [int(x) for x in m.group(2).split(",")]


def check_same_files(got, want, names):
    assert sorted(os.listdir(str(got))) == sorted(os.listdir(str(want))), "the directory of the ranks' run against the one-process run's"
    for name in names:
        assert read(got / name) == read(want / name), name


def summary_lines(log):
    """The reports' closing log lines, which carry the read counters that reach no file."""
    return re.findall(r"\] ((?:QC|Amplicons|Codons|Co-occurrence|Error profile|Haplotypes): .*)", log)


def check_same_summaries(log, want_log, n):
    assert summary_lines(log) == summary_lines(want_log) and len(summary_lines(log)) == n, (summary_lines(log), summary_lines(want_log))


def check_same_bam(got, want):
    joined, one = read(got), read(want)
    assert joined.endswith(bam_native.BGZF_EOF) and gzip.decompress(joined) == gzip.decompress(one) and len(one) > 3000


def check_only_rank_0_wrote(cwd, logs, at_least=len(TEXT_OUTPUTS)):
    opened = [[l.split(": ", 1)[1] for l in log.splitlines() if l.startswith("rank_worker: opens for writing: ")] for log in logs]
    inside = lambda paths: [p for p in paths if os.path.dirname(os.path.abspath(os.path.join(str(cwd), p))) == os.path.abspath(str(cwd))]
    assert len(inside(opened[0])) >= at_least, opened[0]             # (the worker does log them)
    for rank in range(1, len(logs)):
        assert inside(opened[rank]) == [], "rank %d opened an output" % rank


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def test_one_process_reference_is_the_restatements(job):
    """The one-process run of (a) on ``plain``: its error-profile JSON and its co-occurrence table are the restatements' on the
    oracle's trim results, and its outputs show the five constructions the reach conditions count carriers of."""
    d = job.reference("aio_plain", job.aio(job.bam["plain"]))
    batch, G = job.batch["plain"], job.G
    tabs = oracle.find_overlapping_primers(G, job.primers, 0)
    r = oracle.process(batch, G, *tabs, MQ, WINDOW, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim)
    t = errprof.Tables(*U.tables(segs, job.ref_seq, job.mask_positions, MQ), MQ, len(job.mask_positions), r.counts)
    text = read(d / "ep.json").decode()
    assert json.loads(text) == t.report() and list(json.loads(text)) == list(t.report()) and t.reads[0] > 1000
    sets = cooc.parse_sets(job.sets_text, job.ref_seq)
    dev = CO.SetList([[(p, l, s) for _, p, l, s in muts] for _, muts in sets.sets])
    f = io.StringIO()
    cooc.write_tsv(f, "SYN_REF", cooc.Tables(sets, *CO.tables(segs, G, dev, MQ)))
    assert read(d / "co.tsv").decode() == f.getvalue()
    rows = {(x[1], x[3]): x for x in (l.split("\t") for l in f.getvalue().splitlines()[1:])}
    assert int(rows[("del_and_sub", "11")][4]) > 50 and rows[("two_amplicons", "11")][4:7] == ["0", "0", "0"] and int(rows[("two_amplicons", "11")][7]) > 0
    # (no read reaches both amplicons' sites: nothing complete, the reads that show one of them partial)
    recs = vcf_records(read(d / "out.vcf").decode())
    assert "A" in recs[job.pa][0] and recs[job.pa][1]["ALT_AA"].strip(".,|") != ""
    assert any(len(a) > 1 for a in recs[job.pi][0])              # the planted insertion is called: the position was flagged
    dels = [l.split("\t") for l in read(d / "del.tsv").decode().splitlines()[1:]]
    assert [int(x[3]) > 50 for x in dels if (int(x[1]), int(x[2])) == (job.pc + 1, 3)] == [True]
    assert read(d / "out.bam").endswith(bam_native.BGZF_EOF)


def test_one_process_log_names_outputs_and_summaries_in_order(job):
    """The "Output ..." lines and the reports' closing lines of the one-process run of (a), by their text up to the first colon,
    against a list that does not come from the walk over reports.REGISTRY: it was written down from a run, with these arguments,
    of a run_amplipy that threaded every report by hand.  The deletion report's two files come first (they are written beside
    the VCF), then the other reports' in registry order, the QC report last; then the closing lines."""
    job.reference("aio_plain", job.aio(job.bam["plain"]))
    lines = [re.sub(r"^\[[^\]]*\] ", "", l) for l in job.logs["aio_plain"].splitlines()]
    heads = [l.split(":", 1)[0] for l in lines if l.startswith("Output ") or l in summary_lines(job.logs["aio_plain"])]
    assert heads == ["Output trimmed SAM/BAM", "Output variants VCF", "Output indel VCF", "Output deletion events", "Output strand tallies",
                     "Output per-amplicon counts", "Output codon table", "Output amino-acid calls", "Output co-occurrence table", "Output error profile",
                     "Output haplotype table", "Output read-position tallies", "Output QC report", "QC", "Amplicons", "Codons", "Co-occurrence",
                     "Error profile", "Haplotypes"]


# ---- (a), (b) -------------------------------------------------------------------------------------------------------------------
def check_reach(job, tag, shares):
    batch = job.batch[tag]
    print("shares", shares)
    assert all(n > 0 for n in shares) and sum(shares) == batch.n
    bounds = np.concatenate([[0], np.cumsum(shares)])
    ends = [job.batch[tag].segment(int(c) - 1).reference_end for c in bounds[1:-1]]
    assert any(int(batch.pos[int(c)]) < e for c, e in zip(bounds[1:-1], ends)), "no cut falls inside a pile"
    for kind, mask in job.carriers[tag].items():
        per_rank = [int(mask[a:b].sum()) for a, b in zip(bounds[:-1], bounds[1:])]
        print(kind, per_rank)
        assert sum(n > 0 for n in per_rank) >= 2, (kind, per_rank)


@pytest.mark.parametrize("world,tag,pieces", [(2, "turned", 2), (3, "plain", 2), (3, "plain", 1)], ids=["world2", "world3", "world3_one_piece_each"])
def test_every_report_bam_in_bam_out(job, tmp_path, world, tag, pieces):
    argv = job.aio(job.bam[tag])
    want = job.reference("aio_" + tag, argv)
    size = os.path.getsize(job.bam[tag])
    status, logs = run_ranks(world, tmp_path, argv, part_bytes=size // (pieces * world) + 1 if pieces > 1 else 4 * size)
    assert status == [0] * world, "\n".join(logs)
    assert not [n for n in os.listdir(str(tmp_path)) if ".part" in n]
    check_same_files(tmp_path, want, TEXT_OUTPUTS)
    check_same_bam(tmp_path / "out.bam", want / "out.bam")
    assert "Trimmed reads of %d ranks joined" % world in logs[0]
    check_same_summaries(logs[0], job.logs["aio_" + tag], 6)
    check_only_rank_0_wrote(tmp_path, logs)
    how = re.findall(r"rank_worker: all-reduce of device tensors: (.*)", "\n".join(logs))
    print("all-reduce of device tensors:", how)
    assert len(how) == world and len(set(how)) == 1
    check_reach(job, tag, shares_of(logs[0], world))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def test_text_in_world_2(job, tmp_path):
    argv = job.aio(job.sam)
    want = job.reference("aio_sam", argv)
    status, logs = run_ranks(2, tmp_path, argv)
    assert status == [0, 0], "\n".join(logs)
    for name in TEXT_OUTPUTS:
        assert read(tmp_path / name) == read(want / name), name
    check_same_summaries(logs[0], job.logs["aio_sam"], 6)
    # the trimmed reads of dealt-out text are NOT joined: one file per rank, together the one-process file's records
    assert sorted(set(os.listdir(str(tmp_path))) - set(TEXT_OUTPUTS)) == ["out.part0.bam", "out.part1.bam"]

    def records(path):
        rd = bamio.AlignmentReader(str(path), "rb")
        out = collections.Counter(bamio.bam_record_bytes(r, r.pos, r.cigar) for r in rd)
        rd.close()
        return out
    parts = [records(tmp_path / ("out.part%d.bam" % r)) for r in range(2)]
    one = records(want / "out.bam")
    assert parts[0] + parts[1] == one and sum(one.values()) > 1000 and all(sum(p.values()) > 0.4 * sum(one.values()) for p in parts)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("command", ["variants", "consensus"])
def test_variants_and_consensus_alone_world_2(job, tmp_path, command):
    argv = job.alone(command)
    want = job.reference(command, argv)
    size = os.path.getsize(job.bam["plain"])
    status, logs = run_ranks(2, tmp_path, argv, part_bytes=size // 4 + 1)
    assert status == [0, 0], "\n".join(logs)
    names = sorted(os.listdir(str(want)))
    assert names == sorted(["out.vcf" if command == "variants" else "out.fas", "c.tsv", "co.tsv", "ep.json", "del.tsv", "s.tsv", "hap.tsv", "rp.tsv"])
    check_same_files(tmp_path, want, names)
    check_same_summaries(logs[0], job.logs[command], 4)
    shares = shares_of(logs[0], 2)
    assert all(n > 0 for n in shares) and sum(shares) == job.batch["plain"].n
    check_only_rank_0_wrote(tmp_path, logs, at_least=len(names))
    if command == "variants":            # untrimmed: the constructions are there with the input's own CIGARs
        recs = vcf_records(read(want / "out.vcf").decode())
        assert "A" in recs[job.pa][0] and recs[job.pc][1]["DEL_N"] != "0"


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
def test_ranks_with_an_empty_share_world_3(job, tmp_path):
    argv = job.aio(job.bam["thin"])
    want = job.reference("aio_thin", argv)
    status, logs = run_ranks(3, tmp_path, argv, part_bytes=4 * os.path.getsize(job.bam["thin"]))
    assert status == [0, 0, 0], "\n".join(logs)
    shares = shares_of(logs[0], 3)
    assert sorted(shares) == [0, 0, job.batch["thin"].n], shares
    assert sum("Finished Processing -1 reads" in log for log in logs) == 2
    check_same_files(tmp_path, want, TEXT_OUTPUTS)
    check_same_bam(tmp_path / "out.bam", want / "out.bam")
    check_same_summaries(logs[0], job.logs["aio_thin"], 6)
    check_only_rank_0_wrote(tmp_path, logs)
    recs = vcf_records(read(want / "out.vcf").decode())
    assert "A" in recs[job.pa][0] and len(recs) > 5              # (the thin job still calls its variants)


# ---- (f) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["part_is_a_directory", "joined_file_exists"])
def test_one_rank_fails_in_front_of_the_collective(job, tmp_path, case):
    argv = job.aio(job.bam["plain"])
    if case == "part_is_a_directory":
        (tmp_path / "out.part1.bam").mkdir()                      # only rank 1 cannot open its output
        failing, reason = 1, "out.part1.bam"
    else:
        (tmp_path / "out.bam").write_bytes(b"kept")               # only rank 0 looks at the joined file's name
        failing, reason = 0, "File already exists: out.bam"
    t0 = time.monotonic()
    status, logs = run_ranks(2, tmp_path, argv, part_bytes=os.path.getsize(job.bam["plain"]) // 4 + 1)
    # well inside the limit: a rank left waiting would sit out the collective's timeout, which IS the limit
    assert time.monotonic() - t0 < LIMIT / 2 and all(s not in (0, None) for s in status), (status, logs)
    for log in logs:
        assert re.search(r"rank %d: \w+: .*%s" % (failing, re.escape(reason)), log), log
        assert "Shares of the" not in log
    if case == "joined_file_exists":
        assert read(tmp_path / "out.bam") == b"kept"
    vcf = tmp_path / "out.vcf"
    assert not vcf.exists() or [l for l in read(vcf).decode().splitlines() if not l.startswith("#")] == []
    assert not (tmp_path / "out.fas").exists()
