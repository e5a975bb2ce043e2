"""What run_amplipy's read loop and its choice of an I/O path do, without a GPU and without an engine: which driver and sink serve
which run (drivers.select against the table of run_amplipy's docstring and DESIGN.md sections 10-14), the progress lines
(AmpliPy.py:897-899), and "the reads in front of a failing one are written, then the run dies" (AmpliPy.py:907-911)."""
import io
import itertools
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from amplipy_amd import abi, bamio, drivers, readloop

ALL = ("", "S", "B", "W", "SB", "SW", "BW", "SBW")        # S, B, W: gpu_sam, gpu_bam, gpu_bam_write


def switches(combo):
    return dict(gpu_sam="S" in combo, gpu_bam="B" in combo, gpu_bam_write="W" in combo)


@pytest.fixture
def names(tmp_path, monkeypatch):
    """Input and output names of every kind the table has; only existence and extension matter to the selection."""
    monkeypatch.delenv("AMPLIPY_PYTHON_BAM", raising=False)
    monkeypatch.setattr(sys, "stdin", io.TextIOWrapper(io.BytesIO()))
    monkeypatch.setattr(sys, "stdout", io.TextIOWrapper(io.BytesIO()))
    n = SimpleNamespace(new_bam=str(tmp_path / "new.bam"), new_sam=str(tmp_path / "new.sam"), stdout="stdout", stdin="stdin")
    for key, name in (("bam", "in.bam"), ("bam_upper", "IN2.BAM"), ("sam", "in.sam"), ("old_bam", "old.bam"), ("old_sam", "old.sam")):
        setattr(n, key, str(tmp_path / name))
        open(getattr(n, key), "w").close()
    n.text_out = (n.stdout, "STDOUT", n.new_sam, str(tmp_path / "NEW2.SAM"))
    n.sam_in = (n.sam, n.stdin, "STDIN")
    n.bam_in = (n.bam, n.bam_upper)
    return n


def test_selection_table_trim_and_aio(names):
    n = names
    note = "BAM device codec: this run writes trimmed reads, the host codec reads the input"
    rows = [  # inputs, outputs, switch combinations, (driver, sink, note)
        (n.bam_in, [n.new_bam], ("BW", "SBW"), ("device_bam", "bam", None)),
        (n.bam_in, [n.new_bam], ("B", "SB"), ("native", None, note)),
        (n.bam_in, [n.new_bam], ("W", "SW", "", "S"), ("native", None, None)),
        (n.bam_in, n.text_out, ("SB", "SBW"), ("device_bam", "text", None)),
        (n.bam_in, n.text_out, ("B", "S", "", "W", "BW", "SW"), ("python", None, None)),
        (n.bam_in, [n.old_bam, n.old_sam], ALL, ("python", None, None)),
        (n.sam_in, n.text_out, ("S", "SB", "SW", "SBW"), ("device_sam", "text", None)),
        (n.sam_in, [n.new_bam], ("SW", "SBW"), ("device_sam", "bam", None)),
        (n.sam_in, [n.new_bam], ("S", "SB"), ("python", None, None)),
        (n.sam_in, list(n.text_out) + [n.new_bam, n.old_bam, n.old_sam], ("", "B", "W", "BW"), ("python", None, None)),
        (n.sam_in, [n.old_bam, n.old_sam], ALL, ("python", None, None)),
        ([n.new_bam, n.new_sam, None], [n.stdout, str(n.new_sam) + "2"], ALL, ("python", None, None)),      # no such input: the Python codec says so
    ]
    for inputs, outputs, combos, want in rows:
        for i, o, c in itertools.product(inputs, outputs, combos):
            assert tuple(drivers.select(i, o, True, **switches(c))) == want, (i, o, c)


def test_selection_table_variants_and_consensus(names):
    n = names
    for c in ALL:
        for i in n.bam_in:
            want = ("device_bam", None, None) if "B" in c else ("native", None, None)
            assert tuple(drivers.select(i, None, False, **switches(c))) == want, (i, c)
            assert tuple(drivers.select(i, n.new_bam, False, **switches(c))) == want, (i, c)      # (no trimmed reads are written: the name is not looked at)
        for i in n.sam_in:
            want = ("device_sam", None, None) if "S" in c else ("python", None, None)
            assert tuple(drivers.select(i, None, False, **switches(c))) == want, (i, c)


def test_selection_several_ranks_and_python_bam(names, monkeypatch):
    n = names
    off = {  # (run_trim, input, output): the route with every switch off
        (True, n.bam, n.new_bam): "native", (True, n.bam, n.stdout): "python", (True, n.bam, n.new_sam): "python", (True, n.bam, n.old_bam): "python",
        (True, n.sam, n.stdout): "python", (True, n.stdin, n.new_sam): "python", (True, n.sam, n.new_bam): "python",
        (False, n.bam, None): "native", (False, n.sam, None): "python", (False, n.stdin, None): "python"}
    for (trim, i, o), driver in off.items():
        for c in ALL:
            assert tuple(drivers.select(i, o, trim, several=True, **switches(c))) == (driver, None, None), (trim, i, o, c)
    monkeypatch.setenv("AMPLIPY_PYTHON_BAM", "1")
    for (trim, i, o), c, several in itertools.product(off, ALL, (False, True)):
        if i == n.bam:
            assert tuple(drivers.select(i, o, trim, several=several, **switches(c))) == ("python", None, None), (trim, i, o, c)
    # ... and standard streams without a binary layer are the Python codec's
    monkeypatch.delenv("AMPLIPY_PYTHON_BAM")
    monkeypatch.setattr(sys, "stdout", io.StringIO())
    monkeypatch.setattr(sys, "stdin", io.StringIO())
    assert drivers.select(n.bam, "stdout", True, **switches("SB")).driver == "python"
    assert drivers.select(n.sam, "stdout", True, **switches("S")).driver == "python"
    assert drivers.select("stdin", n.new_sam, True, **switches("S")).driver == "python"


# ---- the loop -----------------------------------------------------------------------------------------------------------------
class StubEngine:
    """process() answers ``result`` (or an all-clear of the batch's size); the event calls are recorded."""

    def __init__(self, result=None):
        self.result, self.batches, self.event_calls = result, [], 0

    def process(self, batch, read_base=0):
        self.batches.append((batch.n, read_base))
        return self.result or SimpleNamespace(status=np.zeros(batch.n, np.uint8))

    def aggregate_events(self, **kw):
        self.event_calls += 1
        return np.zeros(0, abi.INS_EVENT_DTYPE)


class StubCodec:
    def __init__(self):
        self.read_bases = []

    def process(self, read_base):
        self.read_bases.append(read_base)
        return -1, 0

    def dev_reads(self):
        return None


def rec(i, flag=0):
    return bamio.Rec("r%d" % i, flag, 0, 100 + i, 60, [(0, 8)], -1, -1, 0, "ACGTACGT", bytes([30] * 8))


def test_progress_lines_of_pieces_and_single_records(monkeypatch):
    """A:897-899: "Processed k reads..." in front of the record with index k, for every k that is a multiple of 50,000 but 0 --
    whether the records come in pieces of a device codec or one by one."""
    lines = []
    monkeypatch.setattr(readloop, "print_log", lines.append)
    eng, codec = StubEngine(), StubCodec()
    loop = readloop.ReadLoop(eng)
    assert loop.s_i is None
    for count in (49999, 1, 50000, 3):
        loop.device_piece(codec, SimpleNamespace(n_records=count, n_rows=count, n_bases=8 * count))
    assert lines == ["Processed 50000 reads...", "Processed 100000 reads..."]
    assert (loop.n_seen, loop.s_i, loop.read_base, loop.n_bases) == (100003, 100002, 100003, 8 * 100003)
    assert codec.read_bases == [0, 49999, 50000, 100000]
    unmapped = rec(0, flag=4)                                # (A:902: seen, not processed)
    loop.python_records(itertools.chain([rec(1)], itertools.repeat(unmapped, 49998), [rec(2), rec(3)]))
    assert lines == ["Processed 50000 reads...", "Processed 100000 reads...", "Processed 150000 reads..."]
    assert (loop.n_seen, loop.s_i) == (150004, 150003)
    assert eng.batches == [(3, 100003)] and loop.read_base == 100006 and not loop.pending
    # an empty piece is seen too (its records were all unmapped), and nothing is logged for record 0
    fresh = readloop.ReadLoop(eng)
    fresh.device_piece(codec, SimpleNamespace(n_records=2, n_rows=0, n_bases=0))
    assert (fresh.n_seen, fresh.s_i, fresh.read_base) == (2, 1, 0) and len(lines) == 3 and len(codec.read_bases) == 4


def test_rows_in_front_of_a_failing_read_are_written_then_the_run_dies():
    """A:907-911: row 2 has a status, row 1 is too short after trimming (A:910) -- row 0 alone is written, with the engine's POS and
    CIGAR, the exception is the reference's for that status, and the batch's events are not stored.  The mask the libampbam path
    hands its writer says the same."""
    status = 5
    result = SimpleNamespace(status=np.array([0, 0, status, 0, 0], np.uint8), ref_len=np.array([40, 29, 40, 40, 40], np.int32),
                             trim_flags=np.array([1, 2, 1, 3, 2], np.uint8), new_pos=np.array([200, 201, 202, 203, 204], np.int32),
                             cigar_ops=lambda k: [(4, 2), (0, 6 + k)])
    eng = StubEngine(result)
    written = []
    writer = SimpleNamespace(write=lambda r, pos=None, cigar=None: written.append((r.qname, pos, cigar)))
    loop = readloop.ReadLoop(eng, min_length=30, include_no_primer=False, run_trim=True, do_count=True)
    with pytest.raises(abi.READ_STATUS_EXC[status]) as e:
        loop.python_records([rec(i) for i in range(5)], writer)
    assert abi.READ_STATUS_NAMES[status] in str(e.value)
    assert written == [("r0", 200, [(4, 2), (0, 6)])]
    assert eng.batches == [(5, 0)] and eng.event_calls == 0 and loop.read_base == 0
    keep = readloop.keep_rows(result.ref_len, result.trim_flags, 30, False, first_bad=2)
    assert keep.tolist() == [True, False, False, False, False]
    # without the failing row the rule alone decides: A:910, and -e keeps reads without a primer
    flags = np.array([1, 2, 0, 3, 4], np.uint8)
    assert readloop.keep_rows(result.ref_len, flags, 30, False).tolist() == [True, False, False, True, False]
    assert readloop.keep_rows(result.ref_len, flags, 30, True).tolist() == [True, False, True, True, True]
    assert readloop.keep_rows(result.ref_len, flags, 29, None).tolist() == [True, True, False, True, False]
