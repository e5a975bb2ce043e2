"""The per-read and per-set functions of the co-occurrence tallies (amplipy_amd/csrc/amp_cooc.hpp) on the CPU:
tests/hostsim/cooc_twin.cpp loops them over arrays in the kernel's order of steps, built with plain g++, and the table is held
to the restatement in tests/cooc_util.py -- which single-site sets pin to the reference-pinned oracle's count table.  Inputs:
the seeded mix of the strand tests with trim results from the oracle (both primer sets of tests/test_gpu_codon.py among them),
sorted and shuffled, with and without trimming; crafted reads.  The same source runs as a program of its own under
-fsanitize=address,undefined, on seeded batches and on the crafted cases.  No GPU needed."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import amplicon_util as A
from tests import cooc_util as U
from tests import strand_util as S
from tests.test_strand_twin import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "cooc_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]
PRIMER_SETS = {"one": (2000, [(100, 130), (400, 430)]), "example": (29903, sorted((s, e) for s, e, _ in A.example_rows()))}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cooc_twin") / "libcooc_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.twin_cooc, L.twin_cooc_plain, L.twin_window, L.twin_sites, L.twin_block):
        f.restype = C.c_int
    return L


def device_form(sets):
    """(first, set_off, site_pos, site_len, site_sym as int32, max_span) as amp_cooc_enable lays the sets out."""
    off, pos, ln, sym = sets.arrays()
    first = pos[off[:-1]]
    assert (np.diff(first) >= 0).all()
    span = int((pos[off[1:] - 1] - first).max())
    return [np.ascontiguousarray(a, np.int32) for a in (first, off, pos, ln, sym.astype(np.int32))], span


def twin_tables(L, walked, ref_len, sets, min_quality):
    """-> (cooc, reads, info) of the batch as it is counted; the windowed form and the plain one agree."""
    arrays, span = device_form(sets)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    keep = [walked.pos, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    out = []
    for fn, with_info in ((L.twin_cooc, True), (L.twin_cooc_plain, False)):
        cooc = np.zeros((sets.n_sets, U.CELLS), np.uint32); reads = np.zeros(2, np.uint64); info = np.zeros(3, np.int64)
        rc = fn(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(ref_len), C.c_int32(min_quality), C.c_int32(sets.n_sets),
                *[p(a) for a in arrays], C.c_int32(span), p(cooc), p(reads), *([p(info)] if with_info else []))
        assert rc == 0
        out.append((cooc, reads, [int(x) for x in info]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    return out[0]


def check(L, segments, ref_len, sets, min_quality):
    """The twin on the reads against the restatement.  -> (cooc, reads, info)."""
    cooc, reads = U.tables(segments, ref_len, sets, min_quality)
    got = twin_tables(L, ReadBatch.from_segments(segments), ref_len, sets, min_quality)
    assert np.array_equal(got[1], reads) and np.array_equal(got[0], cooc)
    assert int(reads.sum()) == len(segments)
    return got


def pinned_to_the_oracle(L, segs, G, counts, mq):
    """Single-site sets {(p, b)} for all p, b, a stretch of the reference at a time (a set list has at most 2^16 sets): the
    twin and the restatement agree and ARE the oracle's count table when every live read is regular -- which is asserted of
    the batch first -- and stay at or below it otherwise.  -> whether the batch gave the equality."""
    exact = U.all_regular(segs, G)
    step = abi.COOC_MAX_SETS // 4
    for lo in range(0, G, step):
        hi = min(lo + step, G)
        sets = U.single_sites(lo, hi)
        cooc, reads, info = check(L, segs, G, sets, mq)
        assert exact == (int(reads[1]) == 0)
        U.check_single_sites(cooc, lo, hi, counts, exact)
    return exact


_EXACT = []


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_G%d_s%d" % (c[0], c[1], c[4]))
def test_generator_batches_match_restatement_and_oracle(twin, case, do_trim, sort):
    n, G, primers, mq, seed = case
    batch = S.strand_batch(n, G, primers, seed, sort=sort)
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    r = oracle.process(batch, G, mn, mx, mpl, mq, 4, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim if do_trim else None)
    cooc, reads, info = check(twin, segs, G, U.mixed_sets(G), mq)
    assert int(reads.sum()) == n
    if n >= 700:
        assert cooc[:, :64].any() and cooc[:, U.PARTIAL].any()
    W = twin.twin_window()
    many = U.many_sets(3 * W + 1, G)
    cooc, reads, info = check(twin, segs, G, many, mq)
    if n >= 700:
        assert info[0] > 0 and (sort or info[1] > 0)       # a shuffled tile reaches sets past its window
    if pinned_to_the_oracle(twin, segs, G, r.counts, mq):
        _EXACT.append(n)


@pytest.mark.parametrize("name", sorted(PRIMER_SETS))
def test_both_primer_sets_of_the_device_tests(twin, name):
    G, primers = PRIMER_SETS[name]
    mq = 20
    tabs = oracle.find_overlapping_primers(G, primers, 0)
    for n, sort in ((1025, True), (257, False)):
        batch = S.strand_batch(n, G, primers, 2000 + n, sort=sort)
        r = oracle.process(batch, G, *tabs, mq, 4, do_trim=True, do_count=True)
        assert not r.trim.status.any()
        segs = S.walked_segments(batch, r.trim)
        cooc, reads, info = check(twin, segs, G, U.mixed_sets(G), mq)
        assert cooc.any()
        if pinned_to_the_oracle(twin, segs, G, r.counts, mq):
            _EXACT.append(n)


def test_some_batch_gave_the_equality_with_the_oracle():
    """The equality with the count table holds only on a batch without a non-regular live read: at least one of the batches
    above must have been one, or the pin is the inequality alone."""
    assert any(n >= 65 for n in _EXACT), _EXACT


def crafted_runs():
    """The crafted cases as they are counted: [(name, sets, segments, min_quality, expect)] with the oracle's trim results."""
    tabs = oracle.find_overlapping_primers(U.CRAFT_G, U.CRAFT_PRIMERS, 0)
    out = []
    for name, sets, segs, mq, do_trim, expect in U.crafted():
        batch = ReadBatch.from_segments(segs)
        r = oracle.process(batch, U.CRAFT_G, *(tabs if do_trim else (None, None, 0)), mq, 4, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any(), name
        out.append((name, sets, S.walked_segments(batch, r.trim if do_trim else None), mq, expect))
    bits, segs = U.bit_order_case()

    def expect(c, r, L):
        assert c[0, :64].tolist() == list(range(1, 65)) and c[0, U.PARTIAL] == 0 and int(r[0]) == 2080
    out.append(("bit_order", bits, segs, 20, expect))
    return out


def test_crafted_reads(twin):
    assert twin.twin_sites() == U.SITES == abi.COOC_SITES and twin.twin_block() == 256
    for name, sets, segs, mq, expect in crafted_runs():
        cooc, reads, info = check(twin, segs, U.CRAFT_G, sets, mq)
        expect(cooc, reads, sets)
    sets, segs = U.pile_case()
    cooc, reads, info = check(twin, segs, U.CRAFT_G, sets, 20)
    assert cooc[0, 3] == 4096 and cooc[1, 3] == 3072 and cooc[1, 1] == 1024 and int(cooc.sum()) == 8192


def _vec(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return struct.pack("<q", a.size) + a.tobytes()


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/cooc_twin.cpp with its own main under -fsanitize=address,undefined (host code only).  Without an argument:
    seeded batches of regular and arbitrary CIGARs, reads in front of, inside and behind the reference, l_seq that disagrees
    with the CIGAR, QUAL '*', set lists sparse, dense and longer than a window.  With a file: the crafted cases, from heap blocks
    of exactly their size, against the restatement's tables.  Both must finish clean."""
    exe = str(tmp_path / "cooc_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DCOOC_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "cooc_twin ok" and not r.stderr
    runs = crafted_runs()
    blob = [struct.pack("<i", len(runs))]
    for name, sets, segs, mq, expect in runs:
        cooc, reads = U.tables(segs, U.CRAFT_G, sets, mq)
        expect(cooc, reads, sets)
        w = ReadBatch.from_segments(segs)
        off, pos, ln, sym = sets.arrays()
        blob += [struct.pack("<ii", U.CRAFT_G, mq), _vec(w.pos, np.int32), _vec(w.lseq, np.uint32), _vec(w.cig_off, np.uint32), _vec(w.cig, np.uint32),
                 _vec(w.seq_off // 8, np.uint32), _vec(w.seq, np.uint8), _vec(w.qual, np.uint8), _vec(off, np.int32), _vec(pos, np.int32),
                 _vec(ln, np.int32), _vec(sym, np.int32), _vec(cooc, np.uint32), _vec(reads, np.uint64)]
    fn = tmp_path / "cases.bin"
    fn.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(fn)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "cooc_twin ok: %d cases" % len(runs) and not r.stderr
