"""The functions of the read haplotypes (amplipy_amd/csrc/amp_hap.hpp) on the CPU: tests/hostsim/hap_twin.cpp loops them over
arrays in the kernel's order of steps, built with plain g++ -Wall -Werror, and the table, the tallies and the read counters are
held to the restatement in tests/hap_util.py -- with the 16-bases-at-once compare and with the one-base function, which must
agree.  The 16-at-once compare alone is held against the one-base function and against a count made here for every nibble
phase of the read offset crossed with every phase of the reference offset, and across a word boundary.  Inputs: the seeded mix
laid onto a reference, with trim results from the oracle; the reads of the golden named cases that have status 0; the crafted
edges.  The same source runs once as a program of its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import hap_util as U
from tests import helpers as H
from tests import strand_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hap_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]
G = 4000
PRIMERS = [(10, 30), (25, 60), (400, 420), (800, 830), (3000, 3030)]
MQ = 20


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hap_twin") / "libhap_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    L.twin_hap.restype = C.c_int
    L.twin_match_both.restype = C.c_int32
    L.twin_hash.restype = C.c_uint64
    L.twin_slot.restype = C.c_uint32
    L.twin_constants.restype = None
    return L


def p(a):
    return C.c_void_p(abi.ptr(np.ascontiguousarray(a)))


def twin_tables(L, walked, ref_seq, regions, min_quality, log2_capacity=12, fast=1):
    """-> (entries, info dict, tally, reads) of the batch as it is counted."""
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    keep = [walked.pos, np.ascontiguousarray(walked.flag, np.uint16), walked.lseq, np.ascontiguousarray(walked.cig_off, np.uint32), pad(walked.cig),
            np.ascontiguousarray(walked.seq_off // 8, np.uint32), pad(walked.seq), pad(walked.qual)]
    st = np.array([s for s, _ in regions], np.int32); en = np.array([e for _, e in regions], np.int32)
    ref = np.frombuffer(ref_seq.encode(), np.uint8)
    cap = 1 << log2_capacity
    ev = np.zeros(cap, abi.HAP_ENTRY_DTYPE); n = C.c_int64(0); info = np.zeros(4, np.uint64)
    tally = np.zeros((len(regions), U.TALLY_COLS), np.uint64); reads = np.zeros(2, np.uint64)
    rc = L.twin_hap(C.c_int64(walked.n), *[p(a) for a in keep], None, C.c_int32(len(ref_seq)), C.c_int32(min_quality), C.c_int32(len(regions)), p(st), p(en), p(ref),
                    C.c_int32(log2_capacity), C.c_int32(fast), p(ev), C.c_int64(cap), C.byref(n), p(info), p(tally), p(reads))
    assert rc == 0
    return ev[:n.value], dict(used=int(info[0]), capacity=int(info[1]), lost=int(info[2]), inserts=int(info[3])), tally, reads


def check(L, segments, ref_seq, regions, min_quality):
    """The twin on the reads, both compares, against the restatement.  -> (table, tally, reads, info)."""
    want = U.tables(segments, len(ref_seq), regions, ref_seq, min_quality)
    U.check_invariant(want[0], want[1])
    walked = ReadBatch.from_segments(segments)
    for fast in (1, 0):
        ev, info, tally, reads = twin_tables(L, walked, ref_seq, regions, min_quality, fast=fast)
        assert U.as_dict(ev) == want[0] and np.array_equal(tally, want[1]) and np.array_equal(reads, want[2]), fast
        assert ev.tobytes() == U.as_array(want[0]).tobytes()           # the order of amp_hap_get: by the 14 key words
        assert info["used"] == len(want[0]) and info["lost"] == 0
    assert int(want[2].sum()) == len(segments)
    return want + (info,)


def test_the_constants_are_the_header_s(twin):
    out = np.zeros(10, np.int32)
    twin.twin_constants(p(out))
    assert out.tolist() == [U.MAX_DIFFS, U.MAX_REGION, U.TALLY_COLS, U.KEY_WORDS, U.GLOBAL_PROBES, U.LOG2_DEFAULT, U.BLOCK, U.KIND_N, U.KIND_DEL, U.EMPTY & 0x7FFFFFFF]
    text = open(os.path.join(ROOT, "amplipy_amd", "csrc", "amp_hap.hpp")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+)[;,]" % name, text).group(1))
    assert (val("HP_MAX_DIFFS"), val("HP_MAX_REGION"), val("HP_TALLY_COLS"), val("HP_KEY_WORDS"), val("HP_GLOBAL_PROBES"), val("HP_LOG2_DEFAULT"), val("HP_BLOCK")) == \
        (U.MAX_DIFFS, U.MAX_REGION, U.TALLY_COLS, U.KEY_WORDS, U.GLOBAL_PROBES, U.LOG2_DEFAULT, U.BLOCK)
    assert "constexpr uint32_t HP_EMPTY = 0x%Xu;" % U.EMPTY in text
    head = open(os.path.join(ROOT, "include", "amplihip.h")).read()
    for name, v in (("AMP_HAP_MAX_DIFFS", U.MAX_DIFFS), ("AMP_HAP_MAX_REGION", U.MAX_REGION), ("AMP_HAP_TALLY_COLS", U.TALLY_COLS)):
        assert int(re.search(r"#define %s (\d+)" % name, head).group(1)) == v
    assert (abi.HAP_MAX_DIFFS, abi.HAP_MAX_REGION, abi.HAP_TALLY_COLS, abi.HAP_LOG2_DEFAULT) == (U.MAX_DIFFS, U.MAX_REGION, U.TALLY_COLS, U.LOG2_DEFAULT)
    assert (abi.HAP_COVER, abi.HAP_REF, abi.HAP_REF_REV, abi.HAP_LOWQ, abi.HAP_OVERFLOW, abi.HAP_EDGE) == (U.COVER, U.REF, U.REF_REV, U.LOWQ, U.OVERFLOW, U.EDGE)


def test_the_hash_restated(twin):
    rng = np.random.default_rng(1)
    for _ in range(200):
        n = int(rng.integers(1, 14))
        diffs = tuple(sorted((int(rng.integers(0, 4096)), int(rng.integers(0, 6)), int(rng.integers(0, 4095))) for _ in range(n)))
        region = int(rng.integers(0, 1 << 16))
        words = np.array(U.key_words(region, diffs), np.uint32)
        assert twin.twin_hash(p(words)) == U.mix(words.tolist())
        for log2 in (4, 12, 20, 28):
            assert twin.twin_slot(p(words), C.c_uint32(log2)) == U.slot_global(region, diffs, log2)


CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}


def _match(twin, seq_codes, quals, k0, ref, p0, n, mq=20):
    """twin_match_both on exactly the bytes that hold the bases; -> ([(position, code)], lowq), held to a count made here."""
    L = len(seq_codes)
    packed = np.zeros((L + 1) // 2, np.uint8)
    for k, c in enumerate(seq_codes):
        packed[k >> 1] |= c << (0 if k & 1 else 4)
    out = np.zeros(2 * n, np.int32); lowq = C.c_int32(0)
    qual_a = np.array(quals, np.uint8); ref_a = np.frombuffer(ref.encode(), np.uint8)          # (kept alive over the call)
    nd = twin.twin_match_both(p(packed), p(qual_a), C.c_uint64(k0), p(ref_a), C.c_int32(len(ref)),
                              C.c_int32(p0), C.c_int32(n), C.c_int32(mq), p(out), C.byref(lowq))
    assert nd >= 0, "the 16-at-once compare and the one-base function disagree"
    want, want_low = [], False
    for d in range(n):
        x = ref[p0 + d].upper()
        if x in "ACGT" and seq_codes[k0 + d] != CODE[x]:
            if quals[k0 + d] < mq:
                want_low = True
            else:
                want.append((p0 + d, seq_codes[k0 + d]))
    got = [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(nd)]
    assert got == want and bool(lowq.value) == want_low
    return got, want_low


def test_sixteen_at_once_against_one_base_for_every_phase(twin):
    rng = np.random.default_rng(2)
    letters = "ACGTNacgt"
    seen = 0
    for kq in range(16):
        for kr in range(16):
            for n in (1, 15, 16, 17, 33):
                ref = "".join(letters[k] for k in rng.integers(0, len(letters), size=kr + n))
                codes = [int(rng.choice([1, 2, 4, 8, 15])) for _ in range(kq)]
                for d in range(n):
                    x = ref[kr + d].upper()
                    codes.append(CODE[x] if rng.random() < 0.7 else int(rng.choice([1, 2, 4, 8, 15])))
                quals = [int(q) for q in np.where(rng.random(kq + n) < 0.2, 5, 30)]
                got, _ = _match(twin, codes, quals, kq, ref, kr, n)
                seen += len(got)
    assert seen > 500


def test_sixteen_at_once_across_a_word_boundary(twin):
    """A single difference at every position of three words, the rest the reference: each is found, alone, at its place --
    the last base of a word and the first of the next among them; and one at either end of a stretch that ends mid-word."""
    ref = ("ACGT" * 16)[:50]
    for k0 in (0, 1, 7):
        for at in range(48):
            codes = [1] * k0 + [CODE[c] for c in ref[:48]]
            codes[k0 + at] = 15 if at % 2 else (CODE[ref[at]] % 8) * 2 or 1
            got, low = _match(twin, codes, [30] * len(codes), k0, ref, 0, 48)
            assert got == [(at, codes[k0 + at])] and not low
        codes = [1] * k0 + [CODE[c] for c in ref[2:39]]
        codes[k0] = 15; codes[-1] = 15
        got, low = _match(twin, codes, [30] * (len(codes) - 1) + [3], k0, ref, 2, 37)
        assert got == [(2, 15)] and low


_BATCHES = {}


def mix_batch(n, seed=None):
    """The seeded mix on the 4,000-base reference: the reads ARE the reference but for one base in a hundred, two planted
    variants and one quality in fifty set low."""
    key = (n, seed)
    if key not in _BATCHES:
        ref = U.reference(G)
        planted = [(e + 30, U.other(ref[e + 30]), 2) for _, e in PRIMERS if ref[e + 30] in "ACGT"]
        _BATCHES[key] = U.onto_reference(S.strand_batch(n, G, PRIMERS, 2000 + n if seed is None else seed), ref, 77 + n, rate=0.01, planted=planted, low_rate=0.02)
    return _BATCHES[key]


@pytest.mark.parametrize("do_trim", [True, False])
@pytest.mark.parametrize("n", [1, 64, 65, 257, 1500])
def test_seeded_mix_matches_restatement(twin, n, do_trim):
    ref = U.reference(G)
    regions = U.regions_near(PRIMERS, G)
    batch = mix_batch(n)
    tabs = oracle.find_overlapping_primers(G, PRIMERS, 0)
    r = oracle.process(batch, G, *tabs, MQ, 4, do_trim=do_trim, do_count=True)
    assert not r.trim.status.any()
    segs = S.walked_segments(batch, r.trim if do_trim else None)
    table, tally, reads, info = check(twin, segs, ref, regions, MQ)
    if n >= 1500:
        assert len(table) > 50 and tally[:, U.REF].sum() > 500 and tally[:, U.LOWQ].sum() > 50 and tally[:, U.EDGE].sum() > 0
        assert any(v[1] for v in table.values()) and any(v[0] > 20 for v in table.values())
        assert info["inserts"] < sum(v[0] for v in table.values())          # the combine made one insert of many reads
        assert int(reads[0]) > n // 2 and int(reads[1]) > 0


def test_one_position_regions_give_the_oracle_s_count_table(twin):
    """The pin to what is reference-pinned: reads with a regular CIGAR, every quality at or above min_quality, counted untrimmed.
    A one-position region at p whose reference letter is among A C G T: the REF tally plus the entries by kind are columns
    A C G T N of the ORACLE's counts[p], and EDGE is its '-' column."""
    from amplipy_amd import synth
    from tests import codon_util as CU
    ref = U.reference(G)
    raw = S.strand_batch(900, G, PRIMERS, 4242)
    keep = [i for i in range(raw.n) if CU.is_regular(raw.segment(i), G)][:600]
    b = U.onto_reference(synth.gather_rows(raw, np.array(keep)), ref, 99, rate=0.012)
    segs = []
    for i in range(b.n):
        s = b.segment(i)
        s.query_qualities = type(s.query_qualities)("B", [max(int(q), 25) for q in s.query_qualities])
        segs.append(s)
    r = oracle.process(ReadBatch.from_segments(segs), G, None, None, 0, MQ, 4, do_trim=False, do_count=True)
    assert not r.trim.status.any()
    ps = set()
    for s, e in PRIMERS:
        ps |= set(range(e + 2, e + 34)) | set(range(max(s - 40, 0), s, 3)) | set(range(e + 34, e + 100, 3))
    regions = sorted((p_, p_ + 1) for p_ in ps if ref[p_].upper() in "ACGT")
    table, tally, reads, info = check(twin, segs, ref, regions, MQ)
    seen = 0
    for k, (s, e) in enumerate(regions):
        cols = [table.get((k, ((0, kind, 0),)), [0, 0])[0] for kind in range(5)]
        cols["ACGT".index(ref[s].upper())] += int(tally[k, U.REF])
        assert cols == r.counts[s, :5].tolist() and int(tally[k, U.EDGE]) == int(r.counts[s, 5]), (s, cols, r.counts[s].tolist())
        assert not tally[k, U.LOWQ] and not tally[k, U.OVERFLOW]
        seen += sum(cols) - int(tally[k, U.REF])
    assert seen > 50 and tally[:, U.EDGE].sum() > 0 and any(key[1][0][1] == U.KIND_N for key in table)


def test_named_cases_with_status_zero(twin):
    """The reads of the golden named cases that have status 0, trimmed and as they came in, on a reference of the case's
    length, a region every 7 positions."""
    cases = H.load_json("named_cases.json")["cases"]
    n_ok, n_trials = 0, 0
    for case in cases:
        Gc, mq = case["ref_len"], case["min_quality"]
        ref = U.reference(Gc, seed=5)
        regions = [(a, min(a + 1 + a % 23, Gc)) for a in range(0, Gc, 7)]
        mn, mx, mpl = oracle.find_overlapping_primers(Gc, case["primers"], case["offset"])
        for do_trim in (True, False):
            for rd in case["reads"]:
                b = ReadBatch.from_segments([H.seg_from_dict(rd)])
                r = oracle.process(b, Gc, mn, mx, mpl, mq, case["window"], do_trim=do_trim, do_count=True)
                if not (b.n == 1 and int(r.trim.status[0]) == 0):
                    continue
                table, tally, reads, info = check(twin, S.walked_segments(b, r.trim if do_trim else None), ref, regions, mq)
                n_ok += 1
                n_trials += int(tally[:, U.COVER].sum())
    assert n_ok == 88 and n_trials > 100


def crafted_runs():
    """The crafted cases as they are counted: [(name, regions, segments, min_quality, expect)] with the oracle's trim results."""
    tabs = oracle.find_overlapping_primers(U.CRAFT_G, U.CRAFT_PRIMERS, 0)
    out = []
    for name, regions, segs, mq, do_trim, expect in U.crafted():
        batch = ReadBatch.from_segments(segs)
        r = oracle.process(batch, U.CRAFT_G, *(tabs if do_trim else (None, None, 0)), mq, 4, do_trim=do_trim, do_count=True)
        walked = S.walked_segments(batch, r.trim) if do_trim else [s for s, st in zip(segs, r.trim.status) if st == 0]       # the reads with status 0
        out.append((name, regions, walked, mq, expect))
    return out


def test_crafted_edges(twin):
    for name, regions, segs, mq, expect in crafted_runs():
        table, tally, reads, info = check(twin, segs, U.CRAFT_REF, regions, mq)
        expect(table, tally, reads)


def test_pile_distinct_keys_and_keys_that_differ_in_the_last_word(twin):
    regions, segs, key = U.pile_case()
    table, tally, reads, info = check(twin, segs, U.CRAFT_REF, regions, MQ)
    assert table == {key: [1500, 500]} and info["inserts"] == (1500 + 63) // 64 and list(reads) == [1500, 0]
    regions, segs = U.distinct_keys_case()
    table, tally, reads, info = check(twin, segs, U.CRAFT_REF, regions, MQ)
    assert len(table) == 200 and all(v[0] == 1 for v in table.values())
    segs, keys = U.thirteen_diff_reads((3300, 3400), [(j, w) for j in range(4) for w in (1, 2, 3)] * 2, flag_of=lambda k: 0x10 if k >= 12 else 0)
    table, tally, reads, info = check(twin, segs, U.CRAFT_REF, [(3300, 3400)], MQ)
    assert len(table) == 12 and all(table[k] == [2, 1] for k in keys)
    assert len({tuple(U.key_words(*k)[:13]) for k in keys}) == 1 and len({U.key_words(*k)[13] for k in keys}) == 12       # they differ in the LAST word alone


def test_a_table_of_16_slots_wraps_and_a_full_one_loses_whole_keys(twin):
    region = (3300, 3400)
    variants = [(j, w) for j in range(20) for w in (1, 2, 3)]
    segs, keys = U.thirteen_diff_reads(region, variants)
    at15 = [k for k, key in enumerate(keys) if U.slot_global(*key, 4) == 15][:3]
    assert len(at15) == 3
    walked = ReadBatch.from_segments([segs[k] for k in at15] + [segs[k] for k in range(60) if k not in at15][:9])
    ev, info, tally, reads = twin_tables(twin, walked, U.CRAFT_REF, [region], MQ, log2_capacity=4)
    assert info["used"] == 12 and info["lost"] == 0 and all(keys[k] in U.as_dict(ev) for k in at15)       # three keys of slot 15: probing wrapped
    walked = ReadBatch.from_segments(segs[:40])
    want = U.tables(segs[:40], U.CRAFT_G, [region], U.CRAFT_REF, MQ)
    ev, info, tally, reads = twin_tables(twin, walked, U.CRAFT_REF, [region], MQ, log2_capacity=4)
    stored = U.as_dict(ev)
    assert info["used"] == 16 == len(stored) and all(stored[k] == want[0][k] for k in stored)             # nothing merged
    assert info["lost"] == sum(v[0] for k, v in want[0].items() if k not in stored) == 24
    U.check_invariant(stored, tally, lost=24)


def _vec(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return struct.pack("<q", a.size) + a.tobytes()


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/hap_twin.cpp with its own main under -fsanitize=address,undefined (host code only).  Without an argument:
    the phase sweep of the 16-at-once compare from heap blocks of exactly the bytes that hold the bases, then seeded batches of
    regular and arbitrary CIGARs, both compares, and a table of 16 slots.  With a file: the crafted cases, from heap blocks of
    exactly their size, against the restatement's tables.  Both must finish clean."""
    exe = str(tmp_path / "hap_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DHAP_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "hap_twin ok" and not r.stderr
    runs = crafted_runs()
    blob = [struct.pack("<i", len(runs))]
    for name, regions, segs, mq, expect in runs:
        table, tally, reads = U.tables(segs, U.CRAFT_G, regions, U.CRAFT_REF, mq)
        expect(table, tally, reads)
        w = ReadBatch.from_segments(segs)
        blob += [struct.pack("<i", mq), _vec(w.pos, np.int32), _vec(w.flag, np.uint16), _vec(w.lseq, np.uint32), _vec(w.cig_off, np.uint32), _vec(w.cig, np.uint32),
                 _vec(w.seq_off // 8, np.uint32), _vec(w.seq, np.uint8), _vec(w.qual, np.uint8), _vec([s for s, _ in regions], np.int32),
                 _vec([e for _, e in regions], np.int32), _vec(np.frombuffer(U.CRAFT_REF.encode(), np.uint8), np.uint8),
                 _vec(np.frombuffer(U.as_array(table).tobytes(), np.uint32), np.uint32), _vec(tally, np.uint64), _vec(reads, np.uint64)]
    fn = tmp_path / "cases.bin"
    fn.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(fn)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "hap_twin ok: %d cases" % len(runs) and not r.stderr
