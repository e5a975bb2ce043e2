"""The QC report's per-read and per-position functions (amplipy_amd/csrc/amp_qc.hpp) on the CPU: tests/hostsim/qc_twin.cpp loops
them over arrays, built with plain g++, and every number is held to the restatement in tests/qc_util.py -- on seeded batches
whose trim results come from the C restatement of the read pass (oracle.process, as the other twin tests do) and on seeded count
tables.  The same source runs once as a program of its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi, lib
from oracle import oracle
from tests import qc_util as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "qc_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("qc_twin") / "libqc_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    L.twin_read_tallies.restype = C.c_int
    L.twin_depth.restype = None
    L.twin_regions.restype = None
    return L


def twin_tallies(L, batch, res, ref_len, do_trim, min_length, include_no_primer, owners, n_primers):
    t = np.zeros(len(abi.QC_READ_FIELDS), np.uint64)
    ps = np.zeros(max(n_primers, 1), np.uint64); pe = np.zeros(max(n_primers, 1), np.uint64)
    off = np.ascontiguousarray(batch.cig_off, np.uint32)
    cig = batch.cig if batch.cig.size else np.zeros(1, np.uint32)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    rc = L.twin_read_tallies(C.c_int64(batch.n), p(batch.pos), p(off), p(cig), p(res.ref_len), p(res.trim_flags), p(res.status),
                             C.c_int32(ref_len), C.c_int32(int(do_trim)), C.c_int32(min_length), C.c_int32(int(include_no_primer)),
                             p(owners[0]), p(owners[1]), C.c_int32(n_primers), p(t), p(ps), p(pe))
    assert rc == 0
    return {k: int(v) for k, v in zip(abi.QC_READ_FIELDS, t)}, ps[:n_primers], pe[:n_primers]


def assert_same(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


CASES = [  # (reads, reference length, primers, offset, min_length, include_no_primer, seed)
    (0, 500, [(10, 30)], 0, 30, False, 1),
    (1, 500, [(10, 30)], 0, 30, False, 2),
    (65, 500, [(10, 30)], 3, 30, True, 3),
    (700, 4000, [(10, 30), (10, 30), (25, 60), (400, 420), (800, 830), (805, 812), (3000, 3030)], 0, 50, False, 4),
    (1500, 9000, Q.many_primers(60, 9000, 25), 5, 70, False, 5),
    (1500, 9000, Q.many_primers(60, 9000, 25), 0, 100, True, 6),
]


@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_G%d_p%d_s%d" % (c[0], c[1], len(c[2]), c[6]))
def test_read_tallies_match_restatement(twin, case, do_trim):
    n, G, primers, offset, min_length, inp, seed = case
    batch = Q.mixed_batch(n, G, primers, seed)
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, offset)
    res = oracle.process(batch, G, mn, mx, mpl, 20, 4, do_trim=do_trim, do_count=True).trim
    owners = Q.primer_owners(G, primers, offset)
    want = Q.read_tallies(batch, res, G, do_trim, min_length, inp, owners, len(primers))
    got = twin_tallies(twin, batch, res, G, do_trim, min_length, inp, lib.find_primer_owners(G, primers, offset), len(primers))
    assert_same(got, want)
    t = want[0]
    assert t["rows"] == n and t["errors"] == (1 if n >= 8 else 0)
    if do_trim:
        assert t["kept"] + t["dropped_short"] + t["dropped_no_primer"] == t["rows"] - t["errors"]
        if n >= 700:        # the mix is there: every tally moves
            quiet = {"primer_both"} if len(primers) < 60 else set()       # (few primers far apart: no read meets two)
            quiet |= {"dropped_no_primer"} if inp else set()
            assert all(t[k] > 0 for k in abi.QC_READ_FIELDS if k not in quiet)
            assert inp or t["dropped_no_primer"] > 0
            assert not inp or t["dropped_no_primer"] == 0
            assert t["primer_start"] == int(want[1].sum()) and t["primer_end"] == int(want[2].sum())
    else:
        assert all(t[k] == 0 for k in abi.QC_READ_FIELDS if k not in ("rows", "errors", "ref_bases_in"))


@pytest.mark.parametrize("G", [1, 255, 256, 257, 3001])
def test_depth_and_regions_match_restatement(twin, G):
    counts = Q.seeded_counts(G, G)
    depth = np.zeros(G, np.uint32)
    twin.twin_depth(C.c_void_p(abi.ptr(counts)), C.c_int32(G), C.c_void_p(abi.ptr(depth)))
    want_depth = Q.depth_of(counts)
    assert np.array_equal(depth, want_depth)
    regions = [(0, G), (5, 5), (7, 3), (0, 1), (G - 1, G), (-4, 9), (G - 2, G + 40), (G, G + 1), (10, 73), (10, 74), (10, 75), (100, 900), (300, 301)]
    for depths in ([], [0], [1, 10, 100, 4294967295], [int(want_depth.max()), int(want_depth.max()) + 1]):
        rs = np.array([r[0] for r in regions], np.int32); re_ = np.array([r[1] for r in regions], np.int32)
        dp = np.array(depths + [0], np.uint32)
        out = np.zeros(len(regions), abi.QC_REGION_DTYPE)
        twin.twin_regions(C.c_void_p(abi.ptr(depth)), C.c_int32(G), C.c_int32(len(regions)), C.c_void_p(abi.ptr(rs)), C.c_void_p(abi.ptr(re_)),
                          C.c_int32(len(depths)), C.c_void_p(abi.ptr(dp)), C.c_void_p(abi.ptr(out)))
        Q.assert_regions(out, Q.region_stats(want_depth, regions, depths), len(depths))


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/qc_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches with reads
    in front of, inside and behind the reference, reads without an op and with 40 ops and more, arrays in heap blocks of exactly
    their size.  It must finish clean."""
    exe = str(tmp_path / "qc_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DQC_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "qc_twin ok" and not r.stderr
