"""The per-event functions of the insertion-event aggregation (amplipy_amd/csrc/amp_ins.hpp) on the CPU:
tests/hostsim/ins_twin.cpp loops them over host arrays in the order of steps of ins_aggregate (amp_ins.hip), built with plain
g++, and its runs are held to the plain tally of tests/ins_util.py -- a Counter of (ref_pos, text), the text by Python slicing
of the unpacked codes -- over events of the CPU oracle.  The twin takes a mask for the hash key, so that alleles of one
position and length collide and interleave (nobody can craft that for the device's 64 bits): a run is split then, never
mixed.  Layouts of the eight shard regions, unused slots, the grid edges of the 256-thread kernels, the allele shapes the
reference produces, read ids that wrap, and the host's EventStore on the same batches.  The same source runs once as a program
of its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from amplipy_amd import abi, calling
from amplipy_amd.batch import ReadBatch
from amplipy_amd.insertions import EventStore, event_strings
from tests import ins_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "ins_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]
G = 2000


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ins_twin") / "libins_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, SRC])
    L = C.CDLL(so)
    L.twin_ins_aggregate.restype = C.c_int
    L.twin_read_row.restype = C.c_int64
    L.twin_read_row.argtypes = [C.c_uint32, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def pool():
    """(batch, events): the crafted reads, 300 copies of three alleles, 1,900 distinct 6-base alleles of one position and plain
    reads, shuffled, through the oracle: 2,200 events and more, equal alleles far apart in the list."""
    rng = np.random.default_rng(5)
    segs = [s for _, s in U.crafted_segments()] + U.copies_segments(300) + U.distinct_segments(1900) + U.plain_segments(30, rng, G)
    segs = [segs[i] for i in rng.permutation(len(segs))]
    b = ReadBatch.from_segments(segs)
    a = U.oracle_events(b, G)
    assert a.events.size >= 2200 and int((a.trim.status != 0).sum()) == 1
    ev = a.events[rng.permutation(a.events.size)]
    ev.setflags(write=False)
    return b, ev


def test_header_compiles_without_hip(tmp_path):
    """amp_ins.hpp alone under plain g++ -std=c++17 -Wall -Werror: the two attributes are defined away, nothing of HIP is needed."""
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "amp_ins.hpp"\nint main() { return (int)amp::ins_run_of(0u, 1u); }\n')
    subprocess.check_call([GXX, "-std=c++17", "-Wall", "-Werror"] + INC + ["-o", str(tmp_path / "only_header"), str(src)])
    assert subprocess.run([str(tmp_path / "only_header")]).returncode == 0


def test_crafted_allele_shapes(twin):
    """Every shape of tests/ins_util.crafted_segments, their events the oracle's: the texts are the ones the reference builds,
    and the twin's runs give their tally under every mask.  The read with the trailing insertion has a status and no event."""
    named = U.crafted_segments()
    b = ReadBatch.from_segments([s for _, s in named])
    a = U.oracle_events(b, G)
    names = [n for n, _ in named]
    bad = names.index(U.TRAILING)
    assert [i for i in range(b.n) if a.trim.status[i]] == [bad] and bad not in a.events["read"].tolist()
    by_name = {}
    for e, (p, t) in zip(a.events.tolist(), U.pairs(b, a.events)):
        by_name.setdefault(names[e[1]], []).append((p, t, e[2], e[3]))
    assert by_name["empty allele"] == [(49, "", 9, 9)]
    assert by_name["to the read's end"] == [(63, "TTTACGT", 3, 10)]                       # 7 bases, to the read's end
    assert by_name["anchored at position 0"] == [(0, "GGA", 0, 3)]
    assert by_name["cut by a low quality"] == [(77, "TCC", 3, 6), (73, "CC", 6, 8)]      # ref_end - 1 first, the rest at the insertion
    assert by_name["odd nibble start"][0][2] % 2 == 1 and by_name["even nibble start"][0][2] % 2 == 0
    assert by_name["N and IUPAC codes"] == [(93, "TNRYKM", 3, 9)]
    assert by_name["lower case"] == by_name["upper case twin of it"] == [(103, "TGG", 3, 6)]
    assert by_name["anchor A"][0][:2] == (113, "ATT") and by_name["anchor C"][0][:2] == (113, "CTT")
    assert len(by_name["200 bases"][0][1]) == 201
    assert [by_name["equal up to the last base, " + c][0][1] for c in "CG"] == ["TACGTAC", "TACGTAG"]
    assert by_name["TT"][0][:2] == (143, "ATT") and by_name["TTT"][0][:2] == (143, "ATTT") and by_name["the same text elsewhere"][0][:2] == (153, "ATT")
    want = U.tally(b, a.events)
    assert want[(143, "ATT")] == 2 and want[(103, "TGG")] == 2 and len(want) == a.events.size - 2
    for where, rng in (("end", None), ("scattered", np.random.default_rng(1))):
        slots = U.slots_of(a.events, a.events.size + 7, where, rng)
        regions, shard_n = U.make_list(U.spread(slots, [1, 2, 6], np.random.default_rng(2)), 64)
        for mask in U.MASKS:
            U.check_twin(twin, regions, 64, shard_n, b, 0, mask)


@pytest.mark.parametrize("n_slots", U.SLOT_COUNTS)
def test_list_layouts(twin, pool, n_slots):
    """Where the events lie in the eight shard regions must not matter: every layout at every slot count, under every mask."""
    b, ev = pool
    rng = np.random.default_rng(n_slots)
    n_real = n_slots - (n_slots + 4) // 5      # a fifth of the slots unused, where the layout has unused slots
    layouts = []
    for s in range(8):                          # all events in one shard
        layouts.append(("shard %d" % s, U.spread(ev[:n_slots], [s]), n_slots))
    layouts.append(("shards 0 3 7", U.spread(ev[:n_slots], [0, 3, 7], rng), n_slots))
    layouts.append(("all eight", U.spread(ev[:n_slots], list(range(8)), rng), n_slots))
    layouts.append(("a large cap", U.spread(ev[:n_slots], [2, 5], rng), 40 * n_slots + 1000))
    for where in ("start", "middle", "end", "scattered"):
        layouts.append(("unused " + where, U.spread(U.slots_of(ev[:n_real], n_slots, where, rng), [4]), n_slots))
        layouts.append(("unused %s, eight shards" % where, U.spread(U.slots_of(ev[:n_real], n_slots, where, rng), list(range(8)), rng), n_slots))
    layouts.append(("only unused", U.spread(U.slots_of(ev[:0], n_slots, "end"), [0, 7], rng), n_slots))
    for name, shards, cap in layouts:
        regions, shard_n = U.make_list(shards, cap)
        assert int(shard_n.sum()) == n_slots, name
        for mask in U.MASKS:
            n_runs, n_distinct = U.check_twin(twin, regions, cap, shard_n, b, 0, mask)
            if name == "only unused":
                assert n_runs == 0 and n_distinct == 0


def test_empty_list(twin, pool):
    b, ev = pool
    for cap in (0, 1, 300):
        regions, shard_n = U.make_list([ev[:0]] * 8, cap)
        for mask in U.MASKS:
            runs, ros, n_events = U.run_twin(twin, regions, cap, shard_n, b, 0, mask)
            assert runs.size == 0 and ros.size == 0 and n_events == 0


def test_weak_masks_split_runs_and_never_mix(twin, pool):
    """Alleles of one position and length that collide in the (masked) key and interleave in the list: an allele then comes as
    several runs.  The seeded pool does that under the 1-bit mask -- asserted, so that this case cannot stop testing the split
    unnoticed -- and the tally by text is still exact (check_twin recomputes the text of every event of every run)."""
    b, ev = pool
    regions, shard_n = U.make_list(U.spread(ev, list(range(8)), np.random.default_rng(3)), ev.size)
    n = {mask: U.check_twin(twin, regions, ev.size, shard_n, b, 0, mask) for mask in U.MASKS}
    distinct = n[U.FULL][1]
    assert n[U.FULL][0] == distinct
    assert n[1][0] > distinct, "the 1-bit mask no longer splits a run: the collision path is untested"
    assert n[0][0] > distinct and n[0xF][0] >= distinct
    # ... and the consumer's side of the promise: rows of one allele are summed by text
    runs, _, _ = U.run_twin(twin, regions, ev.size, shard_n, b, 0, 1)
    rows = U.run_rows(runs)
    text = U.pairs(b, rows)
    st = EventStore()
    lens = (rows["q_to"] - rows["q_from"]).astype(np.int64)
    st.add_text(runs["ref_pos"], lens, np.frombuffer("".join(t for _, t in text).encode("ascii"), np.uint8), runs["count"])
    triples = st.counted_pairs()
    assert len(triples) == runs.size > distinct and len(st) == ev.size
    want = U.tally(b, ev)
    got = calling.tallies_from_runs(triples, {p for p, _ in want})
    assert {(p, s): c for p, d in got.items() for s, c in d.items()} == dict(want)
    assert Counter(st.pairs()) == want


def test_one_allele_five_thousand_times(twin):
    b = ReadBatch.from_segments(U.copies_segments(5000, alleles=("GATTAC",)))
    a = U.oracle_events(b, G)
    assert a.events.size == 5000
    regions, shard_n = U.make_list(U.spread(a.events, [0, 1, 2, 3, 4, 5, 6, 7], np.random.default_rng(4)), 5000)
    for mask in U.MASKS:
        assert U.check_twin(twin, regions, 5000, shard_n, b, 0, mask) == (1, 1)
    runs, _, _ = U.run_twin(twin, regions, 5000, shard_n, b, 0, U.FULL)
    assert runs["count"].tolist() == [5000]


@pytest.mark.parametrize("read_base", [0, 7, 2 ** 32 - 3])
def test_read_ids_relative_to_read_base_modulo_2_32(twin, read_base):
    """A 10-read batch whose ids start at read_base: with 2^32 - 3 they wrap inside the batch."""
    segs = [s for n, s in U.crafted_segments() if n in ("TT", "TTT", "anchor A", "anchor C", "lower case", "to the read's end")] + U.distinct_segments(4)
    b = ReadBatch.from_segments(segs)
    assert b.n == 10
    a = U.oracle_events(b, G, read_base)
    ids = sorted(set(a.events["read"].tolist()))
    assert ids == sorted((read_base + i) & 0xFFFFFFFF for i in range(10))
    for r in ids:
        assert twin.twin_read_row(r, read_base) == (r - read_base) % 2 ** 32 < 10
    want = U.tally(b, a.events, read_base)
    assert want == U.tally(b, U.oracle_events(b, G, 0).events, 0) and len(want) == 10
    regions, shard_n = U.make_list(U.spread(a.events, [0, 5], np.random.default_rng(6)), 16, read_base)
    for mask in U.MASKS:
        U.check_twin(twin, regions, 16, shard_n, b, read_base, mask)
    # the host's store takes the ids the same way
    st = EventStore()
    st.add(b, a.events, read_base)
    assert st.pairs() == U.pairs(b, a.events, read_base)


def test_event_store_on_the_same_batches(pool):
    """EventStore.add gives the pairs of event_strings; add_text with counts, then counted_pairs and tallies_from_runs, the tally."""
    b, ev = pool
    st = EventStore()
    st.add(b, ev, 0)
    assert st.pairs() == event_strings(b, ev, 0) and len(st) == ev.size
    named = U.crafted_segments()
    cb = ReadBatch.from_segments([s for _, s in named])
    ca = U.oracle_events(cb, G)
    st2 = EventStore()
    st2.add(cb, ca.events, 0)
    assert st2.pairs() == event_strings(cb, ca.events, 0) and ("", 49) in [(s, p) for p, s in st2.pairs()]
    assert st2.pairs([143]) == [(143, "ATT"), (143, "ATTT"), (143, "ATT")]


def test_twin_as_a_program_under_sanitizers(tmp_path):
    """tests/hostsim/ins_twin.cpp with its own main under -fsanitize=address,undefined (host code only): seeded lists -- shards
    empty and full, unused slots, zero-length alleles, ids that wrap, arrays in heap blocks of exactly their size, the slots
    beyond a region's fill naming no read -- under the four masks against a tally by text.  It must finish clean."""
    exe = str(tmp_path / "ins_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DINS_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ins_twin ok" and not r.stderr
