"""The per-read functions and the two table stages of the deletion events (amplipy_amd/csrc/amp_del.hpp) on the CPU:
tests/hostsim/del_twin.cpp loops them over arrays in the kernel's order of steps, built with plain g++, and the table is held to
the restatement in tests/del_util.py; ``expand`` of every table is held to column 5 of the reference-pinned oracle's count
table.  Inputs: the seeded mix with trim results from the oracle, the reads of the golden named cases that have status 0, and
crafted edges (merged deletions, the reference end, trimming through a deletion, more deletions than segment slots, irregular
CIGARs, keys that collide under either hash, more keys than the block's table or the list holds, a global table that is full).
The same source runs once as a program of its own under -fsanitize=address,undefined.  No GPU needed."""
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
from tests import del_util as D
from tests import helpers as H
from tests import qc_util as Q
from tests import strand_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "del_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]
INFO = ("regular", "walked", "list_full", "lds_past", "flush_full", "combined", "used", "lost", "qual_reads", "lds_inserts")
CONSTANTS = ("BLOCK", "LIST", "LDS_SLOTS", "LDS_PROBES", "LDS_FLUSH_AT", "GLOBAL_PROBES", "LOG2_DEFAULT", "LOG2_MIN", "LOG2_MAX", "ST_SLOTS")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("del_twin") / "libdel_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    L.twin_del.restype = C.c_int
    L.twin_del_constant.restype = C.c_int
    L.twin_del_key.restype = C.c_uint64
    L.twin_del_key.argtypes = [C.c_int32, C.c_int32]
    for f in (L.twin_del_slot_lds, L.twin_del_slot_global, L.twin_del_probes_global):
        f.restype = C.c_uint32
    L.twin_del_slot_lds.argtypes = [C.c_uint64]
    L.twin_del_slot_global.argtypes = [C.c_uint64, C.c_uint32]
    L.twin_del_probes_global.argtypes = [C.c_uint32]
    L.K = {name: L.twin_del_constant(k) for k, name in enumerate(CONSTANTS)}
    return L


class TwinTable:
    """A global table of the twin: run() adds a batch as it is walked."""

    def __init__(self, L, log2_capacity=12):
        self.L, self.log2 = L, log2_capacity
        self.keys = np.full(1 << log2_capacity, D.EMPTY, np.uint64)
        self.cnt = np.zeros((1 << log2_capacity, 2), np.uint32)

    def run(self, walked, ref_len, min_quality, force_serial=False):
        info = np.zeros(len(INFO), np.int64)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
        keep = [walked.pos, walked.flag, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
                np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
        rc = self.L.twin_del(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(ref_len), C.c_int32(min_quality),
                             C.c_uint32(self.log2), C.c_int32(int(force_serial)), p(self.keys), p(self.cnt), p(info))
        assert rc == 0
        return dict(zip(INFO, (int(x) for x in info)))

    def table(self):
        used = np.nonzero(self.keys != np.uint64(D.EMPTY))[0]
        assert not self.cnt[self.keys == np.uint64(D.EMPTY)].any()
        return {(int(self.keys[s]) >> 32, int(self.keys[s]) & 0xFFFFFFFF): [int(self.cnt[s, 0]), int(self.cnt[s, 1])] for s in used}


def oracle_dash(segments, ref_len, min_quality):
    """Column 5 of the oracle's count table for the reads as they are walked; every read must have status 0."""
    r = oracle.process(ReadBatch.from_segments(segments), ref_len, None, None, 0, min_quality, 4, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    return r.counts[:, 5]


def check(L, segments, ref_len, min_quality, log2_capacity=12, invariant=True):
    """The twin on the reads against the restatement, from the CIGAR words and all-serial, and the invariant.  -> (table, info)."""
    want = D.table(segments, min_quality, ref_len)
    walked = ReadBatch.from_segments(segments)
    t = TwinTable(L, log2_capacity)
    info = t.run(walked, ref_len, min_quality)
    assert t.table() == want and info["lost"] == 0 and info["used"] == len(want)
    ser = TwinTable(L, log2_capacity)
    info_ser = ser.run(walked, ref_len, min_quality, force_serial=True)
    assert ser.table() == want and info_ser["regular"] == 0 and info_ser["walked"] == len(segments)
    assert all(0 <= v[1] <= v[0] and v[0] > 0 for v in want.values())
    if invariant:
        dash, rev = D.expand(want, ref_len)
        assert np.array_equal(dash, oracle_dash(segments, ref_len, min_quality))
        rev_segs = [s for s in segments if s.flag & 0x10]
        assert np.array_equal(rev, oracle_dash(rev_segs, ref_len, min_quality) if rev_segs else np.zeros(ref_len, np.uint32))
    return want, info


def test_restated_hash_is_the_header_s(twin):
    rng = np.random.default_rng(1)
    for _ in range(300):
        s, l = int(rng.integers(0, 2 ** 31)), int(rng.integers(1, 2 ** 31))
        key = D.key_of(s, l)
        assert twin.twin_del_key(s, l) == key
        assert twin.twin_del_slot_lds(key) == D.slot_lds(key, twin.K["LDS_SLOTS"])
        for log2 in (4, 12, 20, 28):
            assert twin.twin_del_slot_global(key, log2) == D.slot_global(key, log2)
    assert twin.K["LDS_FLUSH_AT"] * 4 == twin.K["LDS_SLOTS"] * 3 and twin.K["LOG2_DEFAULT"] == abi.DEL_LOG2_DEFAULT == 20
    assert (twin.K["LOG2_MIN"], twin.K["LOG2_MAX"]) == (abi.DEL_LOG2_MIN, abi.DEL_LOG2_MAX) == (4, 28)
    assert twin.twin_del_probes_global(4) == 16 and twin.twin_del_probes_global(20) == twin.K["GLOBAL_PROBES"]


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
    want, info = check(twin, segs, G, mq, invariant=False)
    dash, rev = D.expand(want, G)
    assert np.array_equal(dash, r.counts[:, 5])                 # the invariant, against the oracle's own table of this batch
    assert np.array_equal(rev, S.tables(segs, G, mq)[1][:, 5])
    assert info["regular"] + info["walked"] == n
    if n >= 700:
        assert len(want) > 20 and info["regular"] > n // 4          # (41-op reads are regular here; a read trimmed down to soft clips walks)
        assert 0 < info["qual_reads"] <= info["regular"] < n + 1 and info["qual_reads"] < n // 2                  # only the reads with an event had a quality byte looked at


def test_named_cases_with_status_zero(twin):
    """The reads of the golden named cases that have status 0, trimmed and as they came in (44 each, as the strand twin counts)."""
    cases = H.load_json("named_cases.json")["cases"]
    n_ok = {True: 0, False: 0}
    n_events = 0
    for case in cases:
        G, mq = case["ref_len"], case["min_quality"]
        mn, mx, mpl = oracle.find_overlapping_primers(G, case["primers"], case["offset"])
        for do_trim in (True, False):
            for rd in case["reads"]:
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, G, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                if not (b.n == 1 and int(r.trim.status[0]) == 0):
                    continue
                want, _ = check(twin, S.walked_segments(b, r.trim if do_trim else None), G, mq, invariant=False)
                assert np.array_equal(D.expand(want, G)[0], r.counts[:, 5]), (case["name"], rd["cigar"])
                n_ok[do_trim] += 1
                n_events += len(want)
    assert n_ok == {True: 44, False: 44} and n_events > 0


def test_neighbouring_deletions_are_one_event(twin):
    rng = np.random.default_rng(3)
    G = 600
    for k, mid in enumerate(([(2, 2), (2, 3)], [(2, 2), (1, 1), (2, 3)], [(2, 2), (3, 3)], [(3, 5)], [(2, 2), (1, 4), (3, 1), (1, 2), (2, 2)])):
        segs = [S.seg(40, [(0, 20)] + mid + [(0, 20)], rng, 0x10 if k % 2 else 0)]
        want, info = check(twin, segs, G, 20)
        assert want == {(60, 5): [1, k % 2]} and info["regular"] == 1
    # a match between them, however short, keeps them apart; so does a low-quality base (it is still a position of its own)
    want, _ = check(twin, [S.seg(40, [(0, 20), (2, 2), (0, 1), (2, 3), (0, 20)], rng, 0, qual=[30] * 20 + [2] + [30] * 20)], G, 20)
    assert want == {(60, 2): [1, 0], (63, 3): [1, 0]}
    # a leading and a trailing deletion, soft and hard clips around the core
    want, _ = check(twin, [S.seg(40, [(5, 2), (4, 3), (2, 4), (0, 20), (3, 2), (4, 1), (5, 3)], rng, 0x10)], G, 20)
    assert want == {(40, 4): [1, 1], (64, 2): [1, 1]}


def test_reference_end(twin):
    rng = np.random.default_rng(4)
    # a deletion that ends at the last base and one on a reference of len + 1 bases: regular, whole
    want, info = check(twin, [S.seg(80, [(0, 10), (2, 10)], rng, 0x10)], 100, 20)
    assert want == {(90, 10): [1, 1]} and info["regular"] == 1
    want, info = check(twin, [S.seg(0, [(0, 1), (2, 7)], rng, 0)], 8, 20)
    assert want == {(1, 7): [1, 0]} and info["regular"] == 1
    want, info = check(twin, [S.seg(0, [(2, 7), (0, 1)], rng, 0)], 8, 20)
    assert want == {(0, 7): [1, 0]}
    # a deletion that runs past the reference end is cut where the walk stops.  (The reference raises there: such a read has
    # a status and is not counted, so the device never shows this; the functions still must stay inside the table.)
    segs = [S.seg(80, [(0, 10), (2, 15), (0, 5)], rng, 0x10)]
    want, info = check(twin, segs, 100, 20, invariant=False)
    assert want == {(90, 10): [1, 1]} and info["walked"] == 1
    want, info = check(twin, [S.seg(95, [(0, 10), (2, 3)], rng, 0)], 100, 20, invariant=False)
    assert want == {} and info["walked"] == 1


def test_trimming_cuts_through_a_deletion(twin):
    """A primer that ends inside a read's deletion: what is left of the deletion behind the trim is what the oracle counts."""
    rng = np.random.default_rng(5)
    G, primers, mq = 600, [(100, 130)], 20
    segs_in = [S.seg(100, [(0, 25), (2, 12), (0, 60)], rng, 0x10), S.seg(102, [(0, 20), (2, 20), (0, 60)], rng, 0), S.seg(100, [(0, 45), (2, 4), (0, 40)], rng, 0)]
    batch = ReadBatch.from_segments(segs_in)
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    r = oracle.process(batch, G, mn, mx, mpl, mq, 4, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim)
    want, _ = check(twin, segs, G, mq)
    assert np.array_equal(D.expand(want, G)[0], r.counts[:, 5])
    untrimmed = D.table(segs_in, mq, G)
    assert want != untrimmed and (145, 4) in want and (145, 4) in untrimmed         # the first two changed, the third did not
    assert sum(v[0] * k[1] for k, v in want.items()) < sum(v[0] * k[1] for k, v in untrimmed.items())


def test_more_deletions_than_segment_slots(twin):
    rng = np.random.default_rng(6)
    slots = twin.K["ST_SLOTS"]
    segs = [S.seg(12, S.many_segment_cigar(slots + 3), rng, 0x10), S.seg(12, S.many_segment_cigar(20), rng, 0), S.seg(12, S.many_segment_cigar(slots + 3), rng, 0)]
    want, info = check(twin, segs, 800, 20)
    assert info["regular"] == 3 and len(want) == 20 and want[(14, 1)] == [3, 1] and want[(14 + 3 * (slots + 2), 1)] == [3, 1]


def test_irregular_cigars_walk(twin):
    rng = np.random.default_rng(7)
    G = 600
    # 10M5S3D: a soft clip inside; the deletion behind it still counts (a deleted position counts whatever surrounds it)
    want, info = check(twin, [S.seg(40, [(0, 10), (4, 5), (2, 3)], rng, 0x10)], G, 20)
    assert info["walked"] == 1 and want == {(50, 3): [1, 1]}
    # a padding op between two deletions: walked; the positions are still consecutive.  (The reference raises on a P op: with
    # the hook behind the read pass such a read has a status and is not counted.)
    want, info = check(twin, [S.seg(40, [(0, 10), (2, 2), (6, 1), (2, 3), (0, 10)], rng, 0)], G, 20, invariant=False)
    assert info["walked"] == 1 and want == {(50, 5): [1, 0]}
    # QUAL '*': the walk ends at the first base, a deletion in front of it was counted; one quality byte said so
    seg = Segment(flag=0x10, reference_start=40, cigar=[(2, 3), (0, 10), (2, 2), (0, 5)], query_sequence="ACGTACGTACGTACG", query_qualities=None)
    walked = ReadBatch.from_segments([seg])
    assert walked.qual[int(walked.seq_off[0])] == 0xFF
    t = TwinTable(twin)
    info = t.run(walked, G, 20)
    assert info["walked"] == 1 and info["qual_reads"] == 1 and t.table() == {(40, 3): [1, 1]} == D.table([seg], 20, G)
    # ... and without a deletion nobody looks at the byte
    seg = Segment(flag=0, reference_start=40, cigar=[(0, 15)], query_sequence="ACGTACGTACGTACG", query_qualities=None)
    t = TwinTable(twin)
    info = t.run(ReadBatch.from_segments([seg]), G, 20)
    assert info["regular"] == 1 and info["qual_reads"] == 0 and t.table() == {}


def reads_with(keys, rng, flags=None):
    """One read per key (start, len): 6M, the deletion, 6M."""
    return [S.seg(s - 6, [(0, 6), (2, l), (0, 6)], rng, 0 if flags is None else flags[k]) for k, (s, l) in enumerate(keys)]


def test_keys_that_collide_under_either_hash(twin):
    rng = np.random.default_rng(8)
    G = 200000
    lds = D.colliding_keys(lambda k: D.slot_lds(k, twin.K["LDS_SLOTS"]), range(10, G - 20), 3)
    assert twin.twin_del_slot_lds(D.key_of(*lds[0])) == twin.twin_del_slot_lds(D.key_of(*lds[1]))
    glob = D.colliding_keys(lambda k: D.slot_global(k, 12), range(10, G - 20), 4)
    assert twin.twin_del_slot_global(D.key_of(*glob[0]), 12) == twin.twin_del_slot_global(D.key_of(*glob[1]), 12)
    assert twin.twin_del_slot_lds(D.key_of(*glob[0])) != twin.twin_del_slot_lds(D.key_of(*glob[1]))
    keys = [lds[0], lds[1], lds[0], glob[0], glob[1], glob[1], lds[1], lds[1]]
    flags = [0, 0x10, 0x10, 0, 0x10, 0, 0, 0x10]
    want, info = check(twin, reads_with(keys, rng, flags), G, 20)
    assert want == {lds[0]: [2, 1], lds[1]: [3, 2], glob[0]: [1, 0], glob[1]: [2, 1]}
    assert info["combined"] == 4 and info["lds_inserts"] == 4


def test_one_event_on_many_reads_is_combined(twin):
    rng = np.random.default_rng(9)
    segs = []
    for k in range(600):
        segs.append(S.seg(100, [(0, 30), (2, 9), (0, 30)], rng, 0x10 if k % 3 == 0 else 0) if k % 2 else S.seg(100 + k % 7, [(0, 60)], rng, 0x10 if k % 5 == 0 else 0))
    want, info = check(twin, segs, 1000, 20)
    assert want == {(130, 9): [300, 100]}
    assert info["lds_inserts"] == 5 and info["combined"] == 295          # 128, 128 and 44 entries on the lists of three tiles: 2 + 2 + 1 leaders
    # 70 distinct keys in the reads of one wave's worth of list entries and more
    keys = [(200 + 3 * k, 1 + k % 2) for k in range(70)]
    want, info = check(twin, reads_with(keys, rng), 1000, 20)
    assert len(want) == 70 and info["combined"] == 0 and info["lds_inserts"] == 70


def test_more_keys_than_the_block_s_table_and_the_list_hold(twin):
    rng = np.random.default_rng(10)
    G = 40000
    # 512 reads with four events each, all distinct: 2048 keys through a table of LDS_SLOTS
    cig = [(0, 3), (2, 1), (0, 3), (2, 2), (0, 3), (2, 1), (0, 3), (2, 3), (0, 3)]
    segs = [S.seg(10 + 40 * k, cig, rng, 0x10 if k % 2 else 0) for k in range(512)]
    want, info = check(twin, segs, G, 20)
    assert len(want) == 2048 > twin.K["LDS_SLOTS"] and info["flush_full"] >= 1 and info["lds_past"] > 0 and info["list_full"] == 0
    # 256 reads with five events each: the list has no room for the last 256 events
    cig5 = cig + [(2, 2), (0, 3)]
    segs = [S.seg(10 + 40 * k, cig5, rng, 0x10 if k % 2 else 0) for k in range(256)]
    want, info = check(twin, segs, G, 20)
    assert len(want) == 1280 and info["list_full"] == 1280 - twin.K["LIST"]


def test_a_small_global_table_wraps_and_a_full_one_loses_whole_events(twin):
    rng = np.random.default_rng(11)
    G = 100000
    last = [k for k in ((s, 2) for s in range(10, 5000)) if D.slot_global(D.key_of(*k), 4) == 15][:3]
    others = [k for k in ((s, 3) for s in range(10, 5000)) if D.slot_global(D.key_of(*k), 4) not in (15, 0, 1)][:9]
    keys12 = last + others
    reads = [k for j, k in enumerate(keys12) for _ in range(j + 1)]          # key j on j + 1 reads
    flags = [0x10 if j % 2 else 0 for j in range(len(reads))]
    want, info = check(twin, reads_with(reads, rng, flags), G, 20, log2_capacity=4)
    assert len(want) == 12 and [want[k][0] for k in keys12] == list(range(1, 13))
    t = TwinTable(twin, 4)
    t.run(ReadBatch.from_segments(reads_with(reads, rng, flags)), G, 20)
    assert all(int(t.keys[s]) != D.EMPTY for s in (15, 0, 1))                 # three keys of slot 15: two of them wrapped
    # 24 keys into 16 slots: 16 stored exactly, the reads of the other 8 lost, nothing merged
    keys24 = [(100 + 10 * j, 1 + j % 4) for j in range(24)]
    reads = [k for j, k in enumerate(keys24) for _ in range(j % 5 + 1)]
    segs = reads_with(reads, rng, [0x10 if j % 3 == 0 else 0 for j in range(len(reads))])
    want = D.table(segs, 20, G)
    t = TwinTable(twin, 4)
    info = t.run(ReadBatch.from_segments(segs), G, 20)
    got = t.table()
    assert info["used"] == 16 == len(got) and all(got[k] == want[k] for k in got)
    assert info["lost"] == sum(v[0] for k, v in want.items() if k not in got) > 0
    assert sum(v[0] for v in got.values()) + info["lost"] == sum(v[0] for v in want.values()) == len(reads)


def test_two_batches_accumulate(twin):
    rng = np.random.default_rng(12)
    a = reads_with([(100, 3), (100, 3), (200, 1)], rng, [0, 0x10, 0])
    b = reads_with([(100, 3), (300, 2)], rng, [0x10, 0x10])
    t = TwinTable(twin)
    t.run(ReadBatch.from_segments(a), 1000, 20)
    t.run(ReadBatch.from_segments(b), 1000, 20)
    assert t.table() == D.add_tables(D.table(a, 20, 1000), D.table(b, 20, 1000)) == {(100, 3): [3, 2], (200, 1): [1, 0], (300, 2): [1, 1]}


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/del_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches of
    regular and arbitrary CIGARs, piles that share one deletion, reads in front of, inside and behind the reference, l_seq that
    disagrees with the CIGAR, QUAL '*', arrays in heap blocks of exactly their size, global tables of 16 slots that fill up; the
    CIGAR-word path and the all-serial walk must agree.  It must finish clean."""
    exe = str(tmp_path / "del_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DDEL_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "del_twin ok" and not r.stderr
