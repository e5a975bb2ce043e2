"""The per-read and per-codon functions of the codon tallies (amplipy_amd/csrc/amp_codon.hpp) on the CPU:
tests/hostsim/codon_twin.cpp loops them over arrays in the kernel's order of steps, through the window and all-serial, built with
plain g++, and the table is held to the restatement in tests/codon_util.py -- which the two exact invariants pin to the
reference-pinned oracle's count table.  Inputs: the seeded mix of the strand tests with trim results from the oracle, sorted and
shuffled, with and without trimming; the reads of the golden named cases that have status 0; crafted reads.  The same source
runs once as a program of its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import codon_util as U
from tests import helpers as H
from tests import strand_util as S
from tests.test_strand_twin import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "codon_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("codon_twin") / "libcodon_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.twin_codon, L.twin_window, L.twin_slots, L.twin_block):
        f.restype = C.c_int
    return L


def twin_tables(L, walked, ref_len, starts, min_quality, force_serial=False):
    """-> (codon, reads, info) of the batch as it is counted."""
    starts = np.ascontiguousarray(starts, np.int32)
    codon = np.zeros((starts.size, U.CELLS), np.uint32); reads = np.zeros(2, np.uint64)
    info = np.zeros(4, np.int64)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    keep = [walked.pos, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    rc = L.twin_codon(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(ref_len), C.c_int32(min_quality), C.c_int32(starts.size),
                      p(starts), C.c_int32(int(force_serial)), p(codon), p(reads), p(info))
    assert rc == 0
    return codon, reads, [int(x) for x in info]


def check(L, segments, ref_len, starts, min_quality):
    """The twin on the reads against the restatement, through the window and all-serial.  -> (codon, reads, info)."""
    codon, reads = U.tables(segments, ref_len, starts, min_quality)
    walked = ReadBatch.from_segments(segments)
    got = twin_tables(L, walked, ref_len, starts, min_quality)
    assert np.array_equal(got[1], reads) and np.array_equal(got[0], codon)
    ser = twin_tables(L, walked, ref_len, starts, min_quality, force_serial=True)
    assert np.array_equal(ser[1], reads) and np.array_equal(ser[0], codon) and ser[2][0] == 0
    assert int(reads.sum()) == len(segments)
    return codon, reads, got[2]


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_G%d_s%d" % (c[0], c[1], c[4]))
def test_generator_batches_match_restatement(twin, case, do_trim, sort):
    n, G, primers, mq, seed = case
    batch = S.strand_batch(n, G, primers, seed, sort=sort)
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    r = oracle.process(batch, G, mn, mx, mpl, mq, 4, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim if do_trim else None)
    for cds in (U.one_frame(G), U.overlapping(G), U.three_frames(G)):
        codon, reads, info = check(twin, segs, G, cds.starts, mq)
        U.check_at_most_counts(codon, cds.starts, r.counts)         # against the ORACLE's count table
        assert int(reads.sum()) == n                                # rows minus reads with a status (none here)
        if n >= 700 and len(cds.rows) == 1:
            assert info[0] > 0 and info[1] > 0 and info[0] + info[1] == int(reads[0])
            if sort and len(primers) <= 5:
                assert info[0] > n // 2                             # piles on five primers: most reads take the window
            if not sort:
                assert info[1] > n // 4                             # a shuffled tile is wider than the window
            assert codon[:, :64].any() and codon[:, U.BROKEN].any()


@pytest.mark.parametrize("frame", [0, 1, 2])
def test_whole_codon_reads_give_the_count_table(twin, frame):
    """Invariant 2: single-M reads without N, every quality good, each covering whole codons of one frame -- the marginals of the
    codon table ARE the oracle's count table on every covered position, and cell 64 is zero everywhere."""
    G, mq = 2000, 20
    rng = np.random.default_rng(40 + frame)
    segs = U.whole_codon_reads(800, G, frame, rng)
    batch = ReadBatch.from_segments(segs)
    r = oracle.process(batch, G, None, None, 0, mq, 4, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    cds = U.one_frame(G, frame)
    codon, reads, info = check(twin, segs, G, cds.starts, mq)
    U.check_equal_counts(codon, cds.starts, r.counts, r.counts.sum(axis=1) > 0)
    U.check_at_most_counts(codon, cds.starts, r.counts)
    assert list(reads) == [800, 0] and int(codon.sum()) * 3 == int(r.counts.sum())
    # the other frames see the same reads with a codon less each, and nothing broken either
    other = U.one_frame(G, (frame + 1) % 3)
    codon, reads, info = check(twin, segs, G, other.starts, mq)
    U.check_at_most_counts(codon, other.starts, r.counts)
    assert not codon[:, U.BROKEN].any()


def test_named_cases_with_status_zero(twin):
    """The reads of the golden named cases with status 0, trimmed and as they came in, on every position as a codon start."""
    cases = H.load_json("named_cases.json")["cases"]
    n_ok = {True: 0, False: 0}
    n_irregular = 0
    for case in cases:
        G, mq = case["ref_len"], case["min_quality"]
        if G < 3:
            continue
        cds = U.three_frames(G)
        mn, mx, mpl = oracle.find_overlapping_primers(G, case["primers"], case["offset"])
        for do_trim in (True, False):
            for rd in case["reads"]:
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, G, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                if b.n != 1 or int(r.trim.status[0]) != 0:
                    continue
                codon, reads, info = check(twin, S.walked_segments(b, r.trim if do_trim else None), G, cds.starts, mq)
                U.check_at_most_counts(codon, cds.starts, r.counts)
                n_ok[do_trim] += 1
                n_irregular += int(reads[1])
    assert n_ok[True] >= 40 and n_ok[False] >= 40


def test_crafted_reads(twin):
    W, slots, block = twin.twin_window(), twin.twin_slots(), twin.twin_block()
    assert W * 3 >= 512 and W % 64 == 0
    seen = {}
    for name, G, cds, segs, mq, expect in U.crafted(W, slots, block):
        codon, reads, info = check(twin, segs, G, cds.starts, mq)
        expect(codon, reads, cds)
        batch = ReadBatch.from_segments(segs)
        r = oracle.process(batch, G, None, None, 0, mq, 4, do_trim=False, do_count=True)
        assert not r.trim.status.any()
        U.check_at_most_counts(codon, cds.starts, r.counts)
        seen[name] = info
    assert seen["more_entries_than_slots"][0] == 3 and seen["more_entries_than_slots"][1] == 1 and seen["more_entries_than_slots"][3] > 0
    # a tile of W - 1 or W slots fits the window; W + 1 and 3 W do not: the far reads go serially
    for span, fits in ((W - 1, True), (W, True), (W + 1, False), (3 * W, False)):
        info = seen["span_%d" % span]
        assert (info[1] == 0) == fits, (span, info)
        assert info[0] > block and info[0] + info[1] == 2 * block + 2      # (the middle tile holds both piles: its far reads are the ones that go serially)


def test_slots_the_engine_would_refuse_and_a_reference_without_room():
    """A reference of 2 bases has no slot (the host refuses the CDS file: tests/test_codon_host.py); the slot arrays are
    strictly increasing and end at G - 3."""
    for G in (3, 4, 600, 601, 602):
        st = U.three_frames(G).starts
        assert (np.diff(st) > 0).all() and st[0] == 0 and st[-1] == G - 3
    with pytest.raises(SystemExit):
        from amplipy_amd import codon
        codon.parse_cds("orf\t0\t2\n", 2)


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/codon_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches of
    regular and arbitrary CIGARs, reads in front of, inside and behind the reference, l_seq that disagrees with the CIGAR, QUAL
    '*', arrays in heap blocks of exactly their size; the window path and the serial path must agree.  It must finish clean."""
    exe = str(tmp_path / "codon_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DCODON_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "codon_twin ok" and not r.stderr
