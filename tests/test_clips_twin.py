"""The clip table's per-read functions (amplipy_amd/csrc/amp_clip.hpp) on the CPU: tests/hostsim/clip_twin.cpp loops them over
arrays, built with plain g++, and every cell and scalar is held to the restatement in tests/clip_util.py -- on the crafted reads
of the rule's edges, on wave-shaped batches and on the QC tests' mix.  The same source runs once as a program of its own under
-fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from tests import clip_util as U
from tests import qc_util as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "clip_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("clip_twin") / "libclip_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    L.twin_clips.restype = C.c_int
    L.twin_clip_sizes.restype = C.c_int
    return L


def twin_tables(L, batch, G, clip_min, status=None):
    table = np.zeros((G + 1, 2, abi.CLIP_CELLS), np.uint32)
    scalars = np.zeros(abi.CLIP_SCALARS, np.uint64)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    cig = batch.cig if batch.cig.size else np.zeros(1, np.uint32)
    seq = batch.seq if batch.seq.size else np.zeros(1, np.uint8)
    coff = np.ascontiguousarray(batch.cig_off, np.uint32)            # (held here: p() takes addresses)
    soff8 = np.ascontiguousarray(batch.seq_off // 8, np.uint32)
    status = None if status is None else np.ascontiguousarray(status, np.uint8)
    rc = L.twin_clips(C.c_int64(batch.n), p(batch.pos), p(batch.flag), p(batch.lseq), p(coff), p(cig),
                      p(soff8), p(seq), None if status is None else p(status), C.c_int32(G),
                      C.c_int32(clip_min), p(table), p(scalars))
    assert rc == 0
    return table, scalars


def assert_same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]


def test_sizes_match_abi(twin):
    out = np.zeros(8, np.int32)
    assert twin.twin_clip_sizes(C.c_void_p(abi.ptr(out))) == 7
    assert out[:7].tolist() == [abi.CLIP_K, abi.CLIP_COLS, abi.CLIP_CELLS, abi.CLIP_SCALARS, abi.CLIP_MIN_MAX, abi.CLIP_LEFT, abi.CLIP_RIGHT]
    assert (U.K, U.COLS, U.CELLS) == (abi.CLIP_K, abi.CLIP_COLS, abi.CLIP_CELLS)


@pytest.mark.parametrize("clip_min", [1, 5, 10, 16, 17, 64])
def test_crafted_reads_match_restatement(twin, clip_min):
    G = 500
    batch = U.crafted_batch(G, clip_min)
    want = U.tables(batch, G, clip_min)
    assert_same(twin_tables(twin, batch, G, clip_min), want)
    table, (scanned, skipped, left, right) = want
    # the crafted cases are there: skipped reads of every kind (each twice: forward and reverse), sites at both ends of the table
    assert int(skipped) == 2 * 8 and int(scanned) == batch.n - 16
    if clip_min <= 20:
        assert table[G, U.RIGHT, 0] == 2 and table[0, U.LEFT, 0] == 2 and table[G, U.RIGHT, 1] == 1
        assert table[200, U.LEFT, 2:].reshape(U.K, U.COLS)[:, 4].sum() > 0       # N, = and IUPAC codes went to `other`
    assert int(table[:, :, 1].sum()) * 2 == int(table[:, :, 0].sum()) == int(left) + int(right)


def test_crafted_reads_with_statuses(twin):
    G, clip_min = 500, 10
    batch = U.crafted_batch(G, clip_min)
    status = (np.arange(batch.n) % 3 == 0).astype(np.uint8) * 4
    want = U.tables(batch, G, clip_min, status)
    assert_same(twin_tables(twin, batch, G, clip_min, status), want)
    assert int(want[1][0] + want[1][1]) == int((status == 0).sum())        # a row with a status adds to nothing


@pytest.mark.parametrize("kind", ["one_site", "distinct", "mixed", "left_only", "right_only", "none"])
def test_wave_batches_match_restatement(twin, kind):
    G = 3000
    batch = U.wave_batch(kind, 300, G, 5)
    want = U.tables(batch, G, 10)
    assert_same(twin_tables(twin, batch, G, 10), want)
    sites = (int((want[0][:, 0, 0] > 0).sum()), int((want[0][:, 1, 0] > 0).sum()))
    assert sites == {"one_site": (1, 1), "distinct": (300, 300), "left_only": sites[:1] + (0,), "right_only": (0,) + sites[1:],
                     "none": (0, 0)}.get(kind, sites)
    if kind == "mixed":
        assert sites[0] > 20 and int(want[0][:, 0, 0].max()) > 10


def test_mixed_qc_batch_matches_restatement(twin):
    G = 4000
    primers = [(10, 30), (400, 420), (800, 830), (3000, 3030)]
    batch = Q.mixed_batch(700, G, primers, 4)
    for clip_min in (1, 10):
        want = U.tables(batch, G, clip_min)
        assert_same(twin_tables(twin, batch, G, clip_min), want)
    assert int(want[1][1]) >= 1 and int(want[1][2]) > 0 and int(want[1][3]) > 0        # the read past the reference is skipped


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/clip_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded batches with reads
    in front of, inside and behind the reference, arbitrary CIGAR words, l_seq that disagrees with the CIGAR, arrays in heap blocks
    of exactly their size.  It must finish clean."""
    exe = str(tmp_path / "clip_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DCLIP_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-I", os.path.join(ROOT, "tests", "hostsim"), "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "clip_twin ok" and not r.stderr
