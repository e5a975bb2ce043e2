"""The error profile (amplipy_amd/csrc/amp_errprof.hpp) on the CPU.  First the restatement in tests/errprof_util.py is pinned
to the reference-pinned oracle's count table: the count-table identity per mate and strand, the quality sweep, the cycle
spotlight, the mask.  Then tests/hostsim/errprof_twin.cpp -- the header's functions looped over arrays in the kernel's order
of steps, built with plain g++ -- is held to the restatement on the seeded mix of the strand tests (sorted and shuffled, trimmed
and not), the status-0 reads of the golden named cases and crafted edges.  The same source runs as a program of its own under
-fsanitize=address,undefined, where the segment path and an all-serial walk must agree on arbitrary CIGARs.  No GPU needed."""
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
from tests import errprof_util as U
from tests import helpers as H
from tests import strand_util as S
from tests.test_strand_twin import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "errprof_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]


def odd_ref(G, seed):
    """A seeded reference with a lower-case stretch, some N and some IUPAC letters."""
    ref = list(U.seeded_ref(G, seed))
    rng = np.random.default_rng(seed + 1)
    for p in rng.integers(0, G, size=max(G // 50, 1)):
        ref[int(p)] = "acgtNRY"[int(rng.integers(0, 7))]
    return "".join(ref)


# ---- the restatement and the oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_mix():
    """3,000 reads of the strand tests' mix on the example BED, trimmed by the oracle."""
    primers = sorted((s, e) for s, e, _ in A.example_rows())
    G, mq = 29903, 30
    batch = U.with_mates(S.strand_batch(3000, G, primers, 11), 11)
    tabs = oracle.find_overlapping_primers(G, primers, 0)
    r = oracle.process(batch, G, *tabs, mq, 4, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    return G, mq, batch, r, U.seeded_ref(G, 8)


@pytest.mark.parametrize("do_trim", [True, False])
def test_count_table_identity_per_mate_and_strand(example_mix, do_trim):
    G, mq, batch, r, ref = example_mix
    every = S.walked_segments(batch, r.trim if do_trim else None)
    segs = [s for s in every if U.CU.is_regular(s, G)]      # the identity is about a batch of regular reads (a read trimmed to soft clips alone is none)
    assert len(segs) > 0.7 * len(every) and U.all_regular(segs, G)
    cyc, qualt, sub, reads = U.tables(every, ref, None, mq)
    U.check_invariants(cyc, qualt, sub)
    assert [int(x) for x in reads] == [len(segs), len(every) - len(segs)]
    assert U.same(U.tables(segs, ref, None, mq)[:3], (cyc, qualt, sub))
    walked = ReadBatch.from_segments(segs)
    U.check_count_identity(oracle.process, walked, ref, sub, mq)
    whole = U.oracle_plain_counts(oracle.process, walked, G, mq)
    if do_trim and len(segs) == len(every):
        assert np.array_equal(whole, r.counts)
    assert np.array_equal(sub[:, :, 1].astype(np.int64).sum(axis=(0, 1)), U.by_letter(whole, ref))
    assert all(sub[m, s].any() for m in range(2) for s in range(2)) and sub[:, :, 0].any()


def test_quality_sweep(example_mix):
    G, mq, batch, r, ref = example_mix
    segs = [s for s in S.walked_segments(batch, r.trim) if U.CU.is_regular(s, G)][:600]
    cyc, qualt, sub, reads = U.tables(segs, ref, None, mq)
    U.check_quality_sweep(oracle.process, ReadBatch.from_segments(segs), ref, qualt)
    assert int((qualt.sum(axis=(0, 2)) > 0).sum()) > 10


def test_cycle_spotlight():
    rng = np.random.default_rng(5)
    G = 300
    ref = U.seeded_ref(G, 6)
    segs = []
    for k in range(60):
        L = (1, 7, 24)[k % 3]
        cig = [(0, L)] if k % 4 or L < 7 else [(4, 2), (0, 2), (2, 1), (0, L - 6), (4, 2)]
        pos = int(rng.integers(0, G - 30))
        segs.append(U._read(pos, cig, U.noisy(ref, pos, L, rng, rate=0.3), flag=U.FLAGS[k % len(U.FLAGS)]))
    cyc, qualt, sub, reads = U.tables_plain(segs, ref, None, 20)
    assert int(reads[0]) == 60 and U.same(U.tables(segs, ref, None, 20), (cyc, qualt, sub, reads))
    U.check_cycle_spotlight(oracle.process, segs, ref, cyc)
    assert cyc[:, :, 1].any() and cyc[:, 23].any()


def test_mask_leaves_the_oracles_rows_out(example_mix):
    G, mq, batch, r, ref = example_mix
    segs = [s for s in S.walked_segments(batch, r.trim) if U.CU.is_regular(s, G)]
    covered = np.nonzero(r.counts[:, :4].sum(axis=1))[0]
    mask = sorted(set(int(p) for p in covered[::7]) | {0, G - 1})
    cyc, qualt, sub, reads = U.tables(segs, ref, mask, mq)
    U.check_invariants(cyc, qualt, sub)
    U.check_count_identity(oracle.process, ReadBatch.from_segments(segs), ref, sub, mq, mask=mask)
    assert int(sub.sum()) < int(U.tables(segs, ref, None, mq)[2].sum())


# ---- the twin ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("errprof_twin") / "liberrprof_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.twin_errprof, L.twin_errprof_serial, L.twin_cells, L.twin_slots, L.twin_block, L.twin_lds_lseq, L.twin_cycles, L.twin_quals):
        f.restype = C.c_int
    L.twin_ref_codes.restype = None
    return L


def mask_bits(mask, G):
    bits = np.zeros((G + 31) // 32, np.uint32)
    for p in mask:
        bits[p >> 5] |= np.uint32(1 << (p & 31))
    return bits


def split(cells):
    n1, n2 = int(np.prod(abi.EP_CYC_SHAPE)), int(np.prod(abi.EP_QUAL_SHAPE))
    return cells[:n1].reshape(abi.EP_CYC_SHAPE), cells[n1:n1 + n2].reshape(abi.EP_QUAL_SHAPE), cells[n1 + n2:-2].reshape(abi.EP_SUB_SHAPE), cells[-2:]


def twin_tables(L, walked, ref_seq, mask, min_quality):
    """-> (cyc, qualt, sub, reads, info) of the batch as it is counted; the segment path and the all-serial walk agree."""
    G = len(ref_seq)
    p = lambda a: C.c_void_p(abi.ptr(a))            # (of arrays that outlive the call)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    ref = np.frombuffer(ref_seq.encode("ascii"), np.uint8)
    code = np.zeros(G, np.uint8)
    bits = mask_bits(mask, G) if mask is not None else None
    L.twin_ref_codes(p(ref), p(bits) if bits is not None else None, C.c_int32(G), p(code))
    keep = [walked.pos, walked.flag, walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    out = []
    for fn, with_info in ((L.twin_errprof, True), (L.twin_errprof_serial, False)):
        cells = np.zeros(L.twin_cells() + 2, np.uint64); info = np.zeros(5, np.int64)
        rc = fn(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(G), C.c_int32(min_quality), p(code), p(cells), *([p(info)] if with_info else []))
        assert rc == 0
        out.append((cells, [int(x) for x in info]))
    assert np.array_equal(out[0][0], out[1][0])
    return split(out[0][0]) + (out[0][1],)


def check(L, segments, ref_seq, mask, min_quality):
    """The twin on the reads against the restatement.  -> (cyc, qualt, sub, reads, info)."""
    want = U.tables(segments, ref_seq, mask, min_quality)
    got = twin_tables(L, ReadBatch.from_segments(segments), ref_seq, mask, min_quality)
    assert U.same(got[:4], want)
    U.check_invariants(*got[:3])
    assert int(got[3].sum()) == len(segments)
    return got


def test_constants_and_code_table(twin):
    assert twin.twin_cells() == sum(int(np.prod(s)) for s in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE))
    assert twin.twin_cycles() == abi.EP_CYCLES == U.CYCLES and twin.twin_quals() == abi.EP_QUALS == U.QUALS and twin.twin_block() == 256
    ref = "ACGTacgtNnRYKMSWBDHVUu-*@[`{" + "A" * 40
    G = len(ref)
    code = np.zeros(G, np.uint8)
    p = lambda a: C.c_void_p(abi.ptr(a))
    letters, bits = np.frombuffer(ref.encode("ascii"), np.uint8), mask_bits([0, 31, 32, G - 1], G)
    twin.twin_ref_codes(p(letters), None, C.c_int32(G), p(code))
    assert code.tolist() == [0, 1, 2, 3, 0, 1, 2, 3] + [0xFF] * 20 + [0] * 40
    twin.twin_ref_codes(p(letters), p(bits), C.c_int32(G), p(code))
    assert code.tolist() == [0xFF, 1, 2, 3, 0, 1, 2, 3] + [0xFF] * 20 + [0, 0, 0, 0xFF, 0xFF] + [0] * 34 + [0xFF]


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_G%d_s%d" % (c[0], c[1], c[4]))
def test_generator_batches_match_restatement(twin, case, do_trim, sort):
    n, G, primers, mq, seed = case
    batch = U.with_mates(S.strand_batch(n, G, primers, seed, sort=sort), seed)
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    r = oracle.process(batch, G, mn, mx, mpl, mq, 4, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim if do_trim else None)
    ref = odd_ref(G, seed)
    cyc, qualt, sub, reads, info = check(twin, segs, ref, None, mq)
    if n >= 700:
        assert info[0] > n // 4 and info[1] > 0 and cyc[..., 0].any() and cyc[..., 1].any() and all(sub[m, s].any() for m in range(2) for s in range(2))
    covered = np.nonzero(r.counts[:, :4].sum(axis=1))[0]
    check(twin, segs, ref, [int(p) for p in covered[::5]], mq)


def test_example_bed_mix(twin, example_mix):
    G, mq, batch, r, ref = example_mix
    segs = S.walked_segments(batch, r.trim)
    order = np.random.default_rng(2).permutation(len(segs))
    got = check(twin, segs, ref, None, mq)
    shuffled = check(twin, [segs[k] for k in order], ref, None, mq)
    assert U.same(got[:4], shuffled[:4])
    assert U.same(U.tables_plain(segs[:500], ref, None, mq), U.tables(segs[:500], ref, None, mq))


def test_named_cases_with_status_zero(twin):
    cases = H.load_json("named_cases.json")["cases"]
    n_ok = 0
    for case in cases:
        G, mq = case["ref_len"], case["min_quality"]
        mn, mx, mpl = oracle.find_overlapping_primers(G, case["primers"], case["offset"])
        ref = odd_ref(G, 3)
        for do_trim in (True, False):
            for rd in case["reads"]:
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, G, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                if b.n != 1 or int(r.trim.status[0]) != 0:
                    continue
                check(twin, S.walked_segments(b, r.trim if do_trim else None), ref, None, mq)
                n_ok += 1
    assert n_ok == 88


def crafted_runs(slots):
    """The crafted cases, and a read longer than the block's cells take: [(name, ref, mask, segments, min_quality, expect)]."""
    out = U.crafted(slots)
    rng = np.random.default_rng(4)
    L = 65536 + 40
    ref = U.seeded_ref(L + 100, 9)
    long_reads = [U._read(50, [(0, L)], U.noisy(ref, 50, L, rng, rate=0.01), flag=f, qual=30) for f in (0x0, 0x1 | 0x80 | 0x10)]

    def e(cyc, qualt, sub, reads):
        assert int(cyc.sum()) == 2 * L + 30 and int(cyc[:, U.CYCLES - 1].sum()) == 2 * (L - U.CYCLES + 1)
    out.append(("longer_than_the_block_cells_take", ref, None, long_reads + [U._read(60, [(0, 30)], ref[60:90])], 20, e))
    return out


def test_crafted_edges(twin):
    slots = twin.twin_slots()
    names = set()
    for name, ref, mask, segs, mq, expect in crafted_runs(slots):
        want = U.tables(segs, ref, mask, mq)
        expect(*want)
        if name != "longer_than_the_block_cells_take":
            assert U.same(U.tables_plain(segs, ref, mask, mq), want)       # the array form of the restatement is the plain one
        got = check(twin, segs, ref, mask, mq)
        expect(*got[:4])
        names.add(name)
        if name == "more_segments_than_slots":
            assert got[4][1] == len(U.FLAGS) and got[4][0] == 1
        if name == "longer_than_the_block_cells_take":
            assert got[4][2] == 2 and twin.twin_lds_lseq() == 65535
        if name == "64_equal_qualities":
            assert got[4][3] <= len(U.FLAGS) * (2 + 16)       # one or two quality keys and at most sixteen classes per wave
    assert len(names) == 7 + 13
    # a read with a status touches nothing
    segs = U.crafted(slots)[0][3]
    b = ReadBatch.from_segments(segs)
    # (twin_tables passes no status; here one is given: every other read has one)
    status = (np.arange(b.n) % 2).astype(np.uint8)
    want = U.tables(segs[::2], U.crafted(slots)[0][1], None, 20)
    p = lambda a: C.c_void_p(abi.ptr(a))
    ref = U.crafted(slots)[0][1]
    code = np.zeros(len(ref), np.uint8)
    letters, coff, soff = np.frombuffer(ref.encode("ascii"), np.uint8), b.cig_off.astype(np.uint32), (b.seq_off // 8).astype(np.uint32)
    twin.twin_ref_codes(p(letters), None, C.c_int32(len(ref)), p(code))
    cells = np.zeros(twin.twin_cells() + 2, np.uint64); info = np.zeros(5, np.int64)
    assert twin.twin_errprof(C.c_int64(b.n), p(b.pos), p(b.flag), p(b.lseq), p(coff), p(b.cig), p(soff), p(b.seq),
                             p(b.qual), p(status), C.c_int32(len(ref)), C.c_int32(20), p(code), p(cells), p(info)) == 0
    assert U.same(split(cells), want)


def test_a_pile_is_combined(twin):
    """2,000 reads of one shape, 150 bases in steps of 64, 64 and 22 lanes: with one quality throughout a step has one quality
    key (and up to eight substitution classes), with a different quality per base up to 60; either way the tables are the
    restatement's."""
    for equal in (True, False):
        ref, segs = U.pile(2000, equal)
        got = check(twin, segs, ref, None, 20)
        per_wave = got[4][3] / (2000 * 3)
        assert per_wave < 12 if equal else per_wave > 40


def _vec(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return struct.pack("<q", a.size) + a.tobytes()


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/errprof_twin.cpp with its own main under -fsanitize=address,undefined (host code only).  Without an
    argument: seeded batches of regular and arbitrary CIGARs, reads in front of, inside and behind the reference, l_seq that
    disagrees with the CIGAR, QUAL '*', masks, odd reference letters; the segment path and the all-serial walk must agree.  With
    a file: the crafted cases, from heap blocks of exactly their size, against the restatement's tables.  Both must finish clean."""
    exe = str(tmp_path / "errprof_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DERRPROF_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "errprof_twin ok" and not r.stderr
    runs = crafted_runs(4)
    blob = [struct.pack("<i", len(runs))]
    for name, ref, mask, segs, mq, expect in runs:
        cyc, qualt, sub, reads = U.tables(segs, ref, mask, mq)
        w = ReadBatch.from_segments(segs)
        blob += [struct.pack("<i", mq), _vec(w.pos, np.int32), _vec(w.flag, np.uint16), _vec(w.lseq, np.uint32), _vec(w.cig_off, np.uint32), _vec(w.cig, np.uint32),
                 _vec(w.seq_off // 8, np.uint32), _vec(w.seq, np.uint8), _vec(w.qual, np.uint8), _vec(np.frombuffer(ref.encode("ascii"), np.uint8), np.uint8),
                 _vec(mask_bits(mask, len(ref)) if mask is not None else np.zeros(0, np.uint32), np.uint32),
                 _vec(np.concatenate([a.reshape(-1) for a in (cyc, qualt, sub, reads)]), np.uint64)]
    fn = tmp_path / "cases.bin"
    fn.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(fn)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "errprof_twin ok: %d cases" % len(runs) and not r.stderr
