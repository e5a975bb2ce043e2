"""The per-read and per-base functions of the read-position tallies (amplipy_amd/csrc/amp_readpos.hpp) on the CPU:
tests/hostsim/readpos_twin.cpp loops them over arrays in the kernel's order of steps, built with plain g++, and the table is
held to the restatement in tests/readpos_util.py -- which the bin sums and the clip sweep pin to the reference-pinned oracle
first.  Inputs: the seeded mix with trim results from the oracle, the reads of the golden named cases that have status 0, and
crafted reads whose histogram is known in closed form.  The same source runs once as a program of its own under
-fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from oracle import oracle
from tests import helpers as H
from tests import qc_util as Q
from tests import readpos_util as RP
from tests import strand_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "readpos_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("readpos_twin") / "libreadpos_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.twin_readpos, L.twin_window, L.twin_slots, L.twin_flush_period, L.twin_rp_bin):
        f.restype = C.c_int
    return L


def twin_tables(L, walked, ref_len, min_quality, force_serial=False, status=None):
    """-> (hist, info) of the batch as it is walked; status: the reads' statuses (a read with one adds nothing)."""
    hist = np.zeros((ref_len, abi.NSYM, RP.BINS), np.uint32)
    info = np.zeros(5, np.int64)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    keep = [walked.pos, walked.flag, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    st = None if status is None else p(np.ascontiguousarray(status, np.uint8))
    rc = L.twin_readpos(C.c_int64(walked.n), *[p(a) for a in keep], st, C.c_int32(ref_len), C.c_int32(min_quality),
                        C.c_int32(int(force_serial)), p(hist), p(info))
    assert rc == 0
    return hist, [int(x) for x in info]


def check(L, segments, ref_len, min_quality):
    """The twin on the reads against the restatement, window and all-serial.  -> (counts, hist, info)."""
    counts, hist = RP.tables(segments, ref_len, min_quality)
    walked = ReadBatch.from_segments(segments)
    got = twin_tables(L, walked, ref_len, min_quality)
    assert np.array_equal(got[0], hist)
    ser = twin_tables(L, walked, ref_len, min_quality, force_serial=True)
    assert np.array_equal(ser[0], hist) and ser[1][0] == 0
    return counts, hist, got[1]


def example_primers():
    bed = [l.rstrip("\r\n").split("\t") for l in open(H.GOLDEN + "/data/example_primers.bed") if l.strip()]
    return sorted((int(f[1]), int(f[2])) for f in bed)


# ---- 1. the restatement against the oracle ------------------------------------------------------------------------------------
def test_bin_sums_and_clip_sweep_pin_the_restatement_to_the_oracle():
    """3,000 reads of the mix on the example BED at min_quality 30: the bin sums are the oracle's count table, and the oracle's
    count tables of the reads clipped by t = 0, 2, 4, ..., 64 more bases at each end give every bin of all six columns."""
    primers = example_primers()
    G, mq = 29903, 30
    batch = S.strand_batch(3000, G, primers, 11)
    tabs = oracle.find_overlapping_primers(G, primers, 0)
    counts_o, res = S.oracle_counts(oracle.process, batch, G, tabs, mq, 4, True)
    segs = S.walked_segments(batch, res)
    counts, hist = RP.tables(segs, G, mq)
    assert np.array_equal(counts, counts_o)
    hist_o, n_t = RP.sweep(oracle.process, segs, G, mq)
    assert np.array_equal(n_t[0], counts_o)
    for t, tab in zip(RP.EDGES, n_t):
        assert np.array_equal(tab, RP.at_least(segs, G, mq, t)), t
    assert np.array_equal(hist, hist_o)
    assert all(hist[:, :, b].any() for b in range(5)) and hist[:, 5, 1:].any()          # (bins up to d = 31; deletions off the ends)


# ---- 2. the twin against the restatement ----------------------------------------------------------------------------------------
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
    counts, hist, info = check(twin, segs, G, mq)
    assert np.array_equal(counts, r.counts)                 # the bin sums are the oracle's count table
    if n >= 700:
        assert info[0] > 0 and info[1] > 0 and info[0] + info[1] == n
        if sort and len(primers) <= 5:
            assert info[0] > n // 2
        assert hist[:, 5, :].any() and hist[:, :5, 0].any() and hist[:, :5, 1:].any()
        if not sort:
            assert info[1] > n // 4                         # a shuffled tile is wider than the window


def test_named_cases_with_status_zero(twin):
    """Every read of the golden named cases that has status 0, trimmed and as it came in (44 each, as for the strand tallies)."""
    cases = H.load_json("named_cases.json")["cases"]
    n_ok = {True: 0, False: 0}
    for case in cases:
        G, mq = case["ref_len"], case["min_quality"]
        mn, mx, mpl = oracle.find_overlapping_primers(G, case["primers"], case["offset"])
        for do_trim in (True, False):
            for rd, exp in zip(case["reads"], case["expected"]):
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, G, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                if int(r.trim.status[0]) != 0:
                    continue
                counts = check(twin, S.walked_segments(b, r.trim if do_trim else None), G, mq)[0]
                assert np.array_equal(counts, r.counts), (case["name"], rd["cigar"])
                n_ok[do_trim] += 1
    assert n_ok == {True: 44, False: 44}


def test_rp_bin_of_the_header_at_every_edge(twin):
    for d in range(0, 200):
        assert twin.twin_rp_bin(d) == RP.rp_bin(d)
    for b, lo in enumerate(RP.EDGES):
        assert twin.twin_rp_bin(lo) == b and (lo == 0 or twin.twin_rp_bin(lo - 1) == b - 1)
    assert twin.twin_rp_bin(2 ** 31 - 1) == 6


@pytest.mark.parametrize("clip", ["none", "left", "right", "both"])
def test_kept_spans_have_the_closed_form(twin, clip):
    rng = np.random.default_rng(17)
    G = 1000
    for L in RP.SPANS:
        cig = ([(4, 5)] if clip in ("left", "both") else []) + [(0, L)] + ([(4, 7)] if clip in ("right", "both") else [])
        counts, hist, info = check(twin, [RP.good(100, cig, rng)], G, 20)
        assert list(hist.sum(axis=(0, 1))) == RP.closed_form(L), L
        assert int(counts.sum()) == L and (counts[100:100 + L].sum(axis=1) == 1).all()
        # position by position: the base at offset k has d = min(k, L - 1 - k)
        for k in (0, L // 2, L - 1):
            assert hist[100 + k].sum(axis=0)[RP.rp_bin(min(k, L - 1 - k))] == 1


def test_insertions_and_deletions_at_the_ends_and_the_bin_edges(twin):
    rng = np.random.default_rng(5)
    G = 2000
    # an I op in front of the counted base: its bases count towards the distance from the left end
    counts, hist, _ = check(twin, [RP.good(50, [(0, 1), (1, 3), (0, 40)], rng)], G, 20)
    assert hist[51].sum(axis=0)[RP.rp_bin(4)] == 1 and hist[50].sum(axis=0)[0] == 1
    # a D one base from either end has d = 0; a D with e bases on its nearer side has d = e - 1
    for left in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65):
        for cig in ([(0, left), (2, 2), (0, 100)], [(0, 100), (3, 2), (0, left)]):
            counts, hist, _ = check(twin, [RP.good(300, cig, rng)], G, 20)
            assert list(hist[:, 5, :].sum(axis=0)) == [2 if b == RP.rp_bin(left - 1) else 0 for b in range(RP.BINS)], (left, cig)
    # soft clips do not count: the same D behind a clip
    counts, hist, _ = check(twin, [RP.good(300, [(4, 30), (0, 1), (2, 1), (0, 50), (4, 30)], rng)], G, 20)
    assert hist[301, 5, 0] == 1 and int(hist[:, 5].sum()) == 1


def test_crafted_edges(twin):
    W, slots = twin.twin_window(), twin.twin_slots()
    rng = np.random.default_rng(3)
    G = 4 * W
    # more segments than slots: the read walks, its neighbours take the window (deletions take slots on either strand)
    segs = [S.seg(10, [(0, 50)], rng, 0x10), S.seg(12, S.many_segment_cigar(slots // 2), rng, 0), S.seg(12, S.many_segment_cigar((slots - 1) // 2), rng, 0),
            S.seg(14, S.many_segment_cigar(1), rng, 0x10), S.seg(15, [(4, 3), (0, 40), (1, 2), (0, 5), (4, 6)], rng, 0x10), S.seg(16, S.many_segment_cigar(20), rng, 0)]
    info = check(twin, segs, G, 20)[2]
    assert 2 * (slots // 2) + 1 > slots and info[0] == 4 and info[1] == 2 and info[3] > 0
    # a deletion across the window's edge: the read does not fit, walks, and adds on both sides of the edge
    edge = 10 + W
    segs = [S.seg(10, [(0, 30)], rng, 0x10), S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0x10), S.seg(edge - 20, [(0, 18), (2, 5), (0, 12)], rng, 0)]
    counts, hist, info = check(twin, segs, G, 20)
    assert info[0] == 1 and info[1] == 2 and list(hist[edge - 2:edge + 3, 5, RP.rp_bin(11)]) == [2] * 5
    # tiles that span W - 1, W, W + 1 and 3 W positions
    for span in (W - 1, W, W + 1, 3 * W):
        segs = [S.seg(5, [(0, 40)], rng, 0x10), S.seg(5 + span - 40, [(0, 40)], rng, 0x10)]
        info = check(twin, segs, G, 20)[2]
        assert (info[0], info[1]) == ((2, 0) if span <= W else (1, 1)), span
    # a read at the last reference position, and a reference of one base
    check(twin, [S.seg(G - 1, [(0, 1)], rng, 0x10), S.seg(G - 3, [(0, 2), (2, 1)], rng, 0x10), S.seg(G - 40, [(4, 5), (0, 40)], rng, 0)], G, 20)
    counts, hist, info = check(twin, [S.seg(0, [(0, 1)], rng, 0x10, qual=37), S.seg(0, [(4, 2), (0, 1)], rng, 0, qual=30)], 1, 20)
    assert int(counts.sum()) == 2 and int(hist[0, :, 0].sum()) == 2
    # min_quality 0, and one above every quality: only '-' is left
    segs = [S.seg(30, [(0, 20), (2, 3), (0, 20)], rng, 0x10), S.seg(35, [(0, 20), (1, 3), (0, 20)], rng, 0x10, qual=0)]
    counts, hist, _ = check(twin, segs, G, 0)
    assert int(counts[:, :5].sum()) == 40 + 40
    counts, hist, _ = check(twin, segs, G, 200)
    assert int(counts[:, :5].sum()) == 0 and int(counts[:, 5].sum()) == 3 and int(hist[:, 5, RP.rp_bin(19)].sum()) == 3


def test_irregular_reads_walk_or_add_nothing(twin):
    """QUAL '*', a P op and a soft clip inside the core, each beside a plain neighbour: none takes the window.  A read the oracle
    counts (status 0) adds what the restatement says; a read the oracle gives a status adds nothing."""
    rng = np.random.default_rng(8)
    G = 600
    plain = RP.good(52, [(0, 30)], rng)
    odd = [Segment(flag=0, reference_start=40, cigar=[(0, 30)], query_sequence="ACGT" * 7 + "AC", query_qualities=None),
           RP.good(50, [(0, 20), (6, 2), (0, 20)], rng), RP.good(50, [(0, 20), (4, 3), (0, 20)], rng)]
    n_counted = n_status = 0
    for seg in odd:
        b = ReadBatch.from_segments([seg, plain])
        r = oracle.process(b, G, None, None, 0, 20, 4, do_trim=False, do_count=True)
        assert int(r.trim.status[1]) == 0
        if int(r.trim.status[0]) == 0:
            counts, hist, info = check(twin, [seg, plain], G, 20)
            assert info[0] == 1 and info[1] == 1 and np.array_equal(counts, r.counts)
            n_counted += 1
        else:
            want = RP.tables([plain], G, 20)[1]
            for serial in (False, True):
                hist, info = twin_tables(twin, b, G, 20, force_serial=serial, status=r.trim.status)
                assert np.array_equal(hist, want) and info[0] + info[1] == 1
            # without the status the header's functions still stay inside their bounds on the read (twin_tables asserts it)
            twin_tables(twin, b, G, 20)
            n_status += 1
    assert n_counted >= 1 and n_status >= 1


def test_a_pile_across_the_flush_period(twin):
    """4-base reads on one position for two tiles more than the flush period: no 16-bit half carries (the twin checks every
    half against a 32-bit shadow) and the table is the closed form times the reads."""
    period = twin.twin_flush_period()
    n = (period + 2) * 256
    one = RP.good(77, [(0, 4)], np.random.default_rng(1))
    b1 = ReadBatch.from_segments([one])
    reps = np.zeros(n, np.int64)
    from amplipy_amd import synth
    walked = synth.gather_rows(b1, reps)
    hist, info = twin_tables(twin, walked, 300, 20)
    want = RP.tables([one], 300, 20)[1].astype(np.uint64) * np.uint64(n)
    assert np.array_equal(hist, want.astype(np.uint32)) and int(hist.sum()) == 4 * n
    assert info[2] == 2 and info[4] == period * 256 and info[4] < 2 ** 16


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/readpos_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches of
    regular and arbitrary CIGAR words, reads in front of, inside and behind the reference, l_seq that disagrees with the CIGAR,
    QUAL '*', arrays in heap blocks of exactly their size; the window path and the all-serial walk must agree."""
    exe = str(tmp_path / "readpos_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DREADPOS_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "readpos_twin ok" and not r.stderr
