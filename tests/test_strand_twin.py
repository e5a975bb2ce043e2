"""The per-read and per-base functions of the strand tallies (amplipy_amd/csrc/amp_strand.hpp) on the CPU:
tests/hostsim/strand_twin.cpp loops them over arrays in the kernel's order of steps, built with plain g++, and the tables are
held to the restatement in tests/strand_util.py -- which the two oracle constructions pin to the reference-pinned oracle first.
Inputs: the seeded mix with trim results from the oracle, the reads of the golden named cases that have status 0, and crafted
edges (more segments than slots, a deletion across the window's edge, a read at the last reference position, a reference of
one base).  The same source runs once as a program of its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import helpers as H
from tests import qc_util as Q
from tests import strand_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "strand_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("strand_twin") / "libstrand_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.twin_strand, L.twin_window, L.twin_slots):
        f.restype = C.c_int
    return L


def twin_tables(L, walked, ref_len, min_quality, force_serial=False):
    """-> (rev, qsum, info) of the batch as it is walked."""
    rev = np.zeros((ref_len, abi.NSYM), np.uint32); qsum = np.zeros((ref_len, S.QSUM_COLS), np.uint64)
    info = np.zeros(4, np.int64)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    keep = [walked.pos, walked.flag, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    rc = L.twin_strand(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(ref_len), C.c_int32(min_quality),
                       C.c_int32(int(force_serial)), p(rev), p(qsum), p(info))
    assert rc == 0
    return rev, qsum, [int(x) for x in info]


def check(L, segments, ref_len, min_quality):
    """The twin on the reads against the restatement, window and all-serial.  -> (counts, rev, qsum, info)."""
    counts, rev, qsum = S.tables(segments, ref_len, min_quality)
    walked = ReadBatch.from_segments(segments)
    got = twin_tables(L, walked, ref_len, min_quality)
    assert np.array_equal(got[0], rev) and np.array_equal(got[1], qsum)
    ser = twin_tables(L, walked, ref_len, min_quality, force_serial=True)
    assert np.array_equal(ser[0], rev) and np.array_equal(ser[1], qsum) and ser[2][0] == 0
    assert (rev <= counts).all() and (qsum >= np.uint64(min_quality) * counts[:, :5].astype(np.uint64)).all()
    return counts, rev, qsum, got[2]


CASES = [  # (reads, reference length, primers, min_quality, seed)
    (0, 500, [(10, 30)], 20, 1),
    (1, 500, [(10, 30)], 20, 2),
    (65, 500, [(10, 30)], 30, 3),
    (700, 4000, [(10, 30), (25, 60), (400, 420), (800, 830), (3000, 3030)], 20, 4),
    (1500, 9000, Q.many_primers(60, 9000, 25), 33, 5),
]


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
    counts, rev, qsum, info = check(twin, segs, G, mq)
    assert np.array_equal(counts, r.counts)                 # the restatement's own count table is the oracle's
    if n >= 700:
        assert info[0] > 0 and info[1] > 0 and info[0] + info[1] == n
        if sort and len(primers) <= 5:
            assert info[0] > n // 2                         # piles on five primers: most reads take the window; the 41-op reads and the far ones walk
        assert rev.any() and (rev < counts).any() and rev[:, 5].any()
        frac = float((batch.flag & 0x10 != 0).mean())
        assert 0.4 < frac < 0.75 and (batch.flag & 0x1).any() and (batch.flag & 0x1 == 0).any()
        if not sort:
            assert info[1] > n // 4                         # a shuffled tile is wider than the window


def test_oracle_constructions_agree_with_restatement():
    """The two ways the oracle alone speaks about the tables, on 3,000 reads of the mix on the example BED at min_quality 30."""
    bed = [l.rstrip("\r\n").split("\t") for l in open(H.GOLDEN + "/data/example_primers.bed") if l.strip()]
    primers = sorted((int(f[1]), int(f[2])) for f in bed)
    G, mq = 29903, 30
    batch = S.strand_batch(3000, G, primers, 11)
    tabs = oracle.find_overlapping_primers(G, primers, 0)
    rev_o, counts_o = S.oracle_rev(oracle.process, batch, G, tabs, mq, 4, True)
    res = S.oracle_counts(oracle.process, batch, G, tabs, mq, 4, True)[1]
    segs = S.walked_segments(batch, res)
    counts, rev, qsum = S.tables(segs, G, mq)
    assert np.array_equal(counts, counts_o) and np.array_equal(rev, rev_o)
    qsum_o, first = S.oracle_qsum(oracle.process, ReadBatch.from_segments(segs), G, mq)
    assert np.array_equal(first, counts_o) and np.array_equal(qsum, qsum_o)
    assert int(qsum.sum()) > 30 * 10000


def test_named_cases_with_status_zero(twin):
    """The reads of the golden named cases.  47 of the 49 come through trim_read without raising; with counting on, 44 have
    status 0 when trimmed and 44 when counted as they came in (three of the 47 raise in update_base_counts: such a read has a
    status, adds nothing, and leaves the tables unspecified).  Every read with status 0 is compared, under both settings."""
    cases = H.load_json("named_cases.json")["cases"]
    assert sum("error" not in exp["trim"] for case in cases for exp in case["expected"]) == 47
    n_ok = {True: 0, False: 0}
    for case in cases:
        G, mq = case["ref_len"], case["min_quality"]
        mn, mx, mpl = oracle.find_overlapping_primers(G, case["primers"], case["offset"])
        for do_trim in (True, False):
            for rd, exp in zip(case["reads"], case["expected"]):
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, G, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                golden_ok = "error" not in exp["count_raw"] if not do_trim else "error" not in exp["trim"] and "error" not in exp["count_trimmed"]
                assert (b.n == 1 and int(r.trim.status[0]) == 0) == golden_ok, (case["name"], rd["cigar"])
                if not golden_ok:
                    continue
                counts = check(twin, S.walked_segments(b, r.trim if do_trim else None), G, mq)[0]
                assert np.array_equal(counts, r.counts), (case["name"], rd["cigar"])
                n_ok[do_trim] += 1
    assert n_ok == {True: 44, False: 44}


def test_crafted_edges(twin):
    W, slots = twin.twin_window(), twin.twin_slots()
    rng = np.random.default_rng(3)
    G = 4 * W
    # more segments than slots: the read walks, its neighbours take the window
    segs = [S.seg(10, [(0, 50)], rng, 0x10), S.seg(12, S.many_segment_cigar(slots), rng, 0x10), S.seg(12, S.many_segment_cigar(slots - 1), rng, 0),
            S.seg(14, S.many_segment_cigar(1), rng, 0x10), S.seg(15, [(4, 3), (0, 40), (1, 2), (0, 5), (4, 6)], rng, 0x10)]
    info = check(twin, segs, G, 20)[3]
    assert info[0] == 4 and info[1] == 1 and info[3] > 0           # (a forward read's deletions take no slot: it fits)
    # a deletion across the window's edge: the read does not fit, walks, and adds on both sides of the edge
    edge = 10 + W
    segs = [S.seg(10, [(0, 30)], rng, 0x10), S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0x10), S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0)]
    counts, rev, qsum, info = check(twin, segs, G, 20)
    assert info[0] == 1 and info[1] == 2 and list(rev[edge - 2:edge + 3, 5]) == [1] * 5 and list(counts[edge - 2:edge + 3, 5]) == [2] * 5
    # tiles that span W - 1, W, W + 1 and 3 W positions
    for span in (W - 1, W, W + 1, 3 * W):
        segs = [S.seg(5, [(0, 40)], rng, 0x10), S.seg(5 + span - 40, [(0, 40)], rng, 0x10)]
        info = check(twin, segs, G, 20)[3]
        assert (info[0], info[1]) == ((2, 0) if span <= W else (1, 1)), span
    # a read at the last reference position, and a reference of one base
    check(twin, [S.seg(G - 1, [(0, 1)], rng, 0x10), S.seg(G - 3, [(0, 2), (2, 1)], rng, 0x10), S.seg(G - 40, [(4, 5), (0, 40)], rng, 0)], G, 20)
    counts, rev, qsum, info = check(twin, [S.seg(0, [(0, 1)], rng, 0x10, qual=37), S.seg(0, [(4, 2), (0, 1)], rng, 0, qual=30)], 1, 20)
    assert int(counts.sum()) == 2 and int(rev.sum()) == 1 and int(qsum.sum()) == 67
    # min_quality 0, and one above every quality: only '-' is left
    segs = [S.seg(30, [(0, 20), (2, 3), (0, 20)], rng, 0x10), S.seg(35, [(0, 20), (1, 3), (0, 20)], rng, 0x10, qual=0)]
    counts, rev, qsum, _ = check(twin, segs, G, 0)
    assert int(counts[:, :5].sum()) == 40 + 40
    counts, rev, qsum, _ = check(twin, segs, G, 200)
    assert int(counts[:, :5].sum()) == 0 and int(counts[:, 5].sum()) == 3 and np.array_equal(rev, counts) and not qsum.any()


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/strand_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches of
    regular and arbitrary CIGARs, reads in front of, inside and behind the reference, l_seq that disagrees with the CIGAR, QUAL
    '*', arrays in heap blocks of exactly their size; the window path and the all-serial walk must agree.  It must finish clean."""
    exe = str(tmp_path / "strand_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DSTRAND_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "strand_twin ok" and not r.stderr
