"""The per-event functions of the insertion evidence (amplipy_amd/csrc/amp_insev.hpp) on the CPU: tests/hostsim/insev_twin.cpp
loops them over arrays in k_insev's order of steps, built with plain g++, and the table is held to the restatement of
tests/insev_util.py on the crafted batches: every bin edge, insertions behind a soft clip and behind a trimmed primer, at the
read's end, at position 0, split by a low quality, alleles of length 0, 1 and 97, odd and even nibbles, two alleles that differ
in the last base, one allele on both strands, QUAL '*', do_trim off.  The event list is the oracle's, dealt to the eight shard
regions between unused slots and behind a cursor with stale entries in front of it.  The same source runs once as a program of
its own under -fsanitize=address,undefined.  No GPU needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from amplipy_amd import abi, insevidence
from oracle import py_restatement as R
from tests import insev_util as U

SRC, GXX, INC = U.TWIN_SRC, U.GXX, U.INC
INFO = ("slots", "unused", "guarded", "events", "inserts", "combined", "used", "lost")
SIDE_DTYPE = np.dtype([("qsum", "<u8"), ("noqual", "<u4"), ("bin", "<u4", (abi.INSEV_BINS,))])
EMPTY = (1 << 64) - 1


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return U.load_twin(tmp_path_factory.mktemp("insev_twin"))


def test_the_constants_python_uses_are_the_headers(twin):
    assert twin.K["BINS"] == abi.INSEV_BINS and twin.K["STRIDE"] == abi.INSEV_STRIDE == twin.K["BLOCK"] * twin.K["GRID"]
    assert (twin.K["LOG2_DEFAULT"], twin.K["LOG2_MIN"], twin.K["LOG2_MAX"]) == (abi.INSEV_LOG2_DEFAULT, abi.INSEV_LOG2_MIN, abi.INSEV_LOG2_MAX)
    assert twin.K["ENTRY_BYTES"] == abi.INSEV_ENTRY_DTYPE.itemsize and twin.K["SIDE_BYTES"] == SIDE_DTYPE.itemsize == 40


def test_distance_and_bin_at_every_edge(twin):
    for d in range(0, 200):
        assert twin.twin_insev_bin(d) == U.bin_of(d), d
    for q_from, q_to, qs, qe in [(5, 8, 5, 40), (4, 8, 5, 40), (10, 40, 0, 40), (10, 41, 0, 40), (7, 7, 0, 40), (0, 3, 0, 3)]:
        assert twin.twin_insev_d(q_from, q_to, qs, qe) == max(0, min(q_from - qs, qe - q_to))
    assert insevidence.END_EDGES == U.BIN_UPPER


def test_python_hash_is_the_twin_s_on_every_letter(twin):
    rng = np.random.default_rng(5)
    texts = ["", "A", U.NT16] + ["".join(U.NT16[k] for k in rng.integers(0, 16, int(rng.integers(1, 120)))) for _ in range(300)]
    for t in texts:
        assert U.twin_hash(twin, t) == insevidence.allele_hash(t), t
    assert len({insevidence.allele_hash(t) for t in texts}) == len(set(texts))
    assert all(insevidence.allele_hash(t) < (1 << 63) for t in texts)


class TwinTable:
    """A table of the twin: run() adds the events of one batch."""

    def __init__(self, L, log2_capacity=10):
        self.L, self.log2 = L, log2_capacity
        n = 1 << log2_capacity
        self.keys = np.full((n, 2), EMPTY, np.uint64)
        self.cnt = np.zeros((n, 2), np.uint32)
        self.side = np.zeros(n, SIDE_DTYPE)

    def run(self, batch, counted_cigars, events, read_base=0, status=None, cap=None, stale=3, unused_every=4):
        """``counted_cigars``: [(op, n)] per read, as the read was counted.  The events go to the eight regions in turn, an unused
        slot after every ``unused_every``-th, behind ``stale`` slots per region that the cursor has passed (events of a read of the
        batch at another position: tallied, they would show)."""
        cig_off = np.zeros(batch.n + 1, np.uint32)
        cig_off[1:] = np.cumsum([len(c) for c in counted_cigars])
        cig = np.array([(n << 4) | op for c in counted_cigars for op, n in c] or [0], np.uint32)
        shards = [[(599, read_base & 0xFFFFFFFF, 0, 1)] * stale for _ in range(8)]
        for k, (pos, read, lo, hi) in enumerate(events):
            s = shards[k % 8]
            s.append((pos, (read + read_base) & 0xFFFFFFFF, lo, hi))
            if unused_every and k % unused_every == 0:
                s.append((-1, 0, 0, 0))
        cap = cap or max(len(s) for s in shards) + 2
        regions = np.zeros(8 * cap, abi.INS_EVENT_DTYPE)
        regions["ref_pos"] = 598; regions["read"] = read_base & 0xFFFFFFFF; regions["q_to"] = 1        # (beyond the fill: never to be looked at)
        for s, slots in enumerate(shards):
            regions[s * cap:s * cap + len(slots)] = np.array(slots, abi.INS_EVENT_DTYPE)
        shard_n = np.array([len(s) for s in shards], np.uint64)
        cursor = np.full(8, stale, np.uint64)
        info = np.zeros(len(INFO), np.int64)
        p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
        keep = [np.ascontiguousarray(batch.flag, np.uint16), np.ascontiguousarray(batch.lseq, np.uint32), cig_off, cig,
                np.ascontiguousarray(batch.seq_off // 8, np.uint32), batch.seq, batch.qual]
        rc = self.L.twin_insev(C.c_int64(batch.n), *[p(a) for a in keep], p(status) if status is not None else None, C.c_uint64(read_base), p(regions),
                               C.c_longlong(cap), p(shard_n), p(cursor), C.c_uint32(self.log2), p(self.keys), p(self.cnt), p(self.side), p(info))
        assert rc == 0
        return dict(zip(INFO, (int(x) for x in info)))

    def table(self):
        used = np.nonzero(self.keys[:, 1] != np.uint64(EMPTY))[0]
        free = self.keys[:, 1] == np.uint64(EMPTY)
        assert (self.keys[free, 0] == np.uint64(EMPTY)).all() and not self.cnt[free].any() and not self.side[free]["bin"].any()
        out = {}
        for s in used.tolist():
            k0 = int(self.keys[s, 0])
            out[(k0 >> 32, k0 & 0xFFFFFFFF, int(self.keys[s, 1]))] = [int(self.cnt[s, 0]), int(self.cnt[s, 1]), int(self.side[s]["noqual"]), int(self.side[s]["qsum"])] + \
                [int(b) for b in self.side[s]["bin"]]
        return out


def oracle_run(case, do_trim=None):
    """(counted CIGARs, events) of a crafted case from the plain restatement of the read pass."""
    do_trim = case.do_trim if do_trim is None else do_trim
    _, events, trims = R.process_full(case.batch, case.G, *case.tabs, U.MQ, U.W, do_trim)
    return [cig for _, cig, _ in trims], events


@pytest.mark.parametrize("name", ["edges", "corners", "primer", "untrimmed"])
@pytest.mark.parametrize("read_base", [0, 0xFFFFFFFF - 3])
def test_crafted_batches_against_the_restatement(twin, name, read_base):
    case = U.crafted()[name]
    cigars, events = oracle_run(case)
    t = TwinTable(twin)
    info = t.run(case.batch, cigars, events, read_base)
    want = U.by_key(case.want())
    assert t.table() == want
    assert info["events"] == len(events) and info["guarded"] == 0 and info["lost"] == 0 and info["used"] == len(want)
    assert info["unused"] == len(range(0, len(events), 4)) and info["slots"] == info["events"] + info["unused"]
    # a second batch adds up
    t.run(case.batch, cigars, events, read_base)
    assert t.table() == U.scaled(want, 2)


def test_every_edge_distance_is_in_the_edge_case():
    ds = set(U.crafted()["edges"].restated()[1])
    assert ds == set(U.D_EDGES)
    want = U.crafted()["corners"].want()
    assert (49, "") in want and (0, "GGA") in want and {len(t) for _, t in want} >= {0, 1, 2, 97}
    # at the read's last kept base (M I S, and M I S H on a reverse read): q_to = qe, bin 0 from the RIGHT end; the allele of one base
    assert want[(309, "GTG")] == [1, 0, 0, 111, 1, 0, 0, 0, 0, 0, 0] and want[(298, "CAGC")][:2] == [1, 1] and want[(298, "CAGC")][4] == 1
    assert want[(294, "C")][:4] == [1, 0, 0, 37]
    events = {(e[0], e[1]): e for e in oracle_run(U.crafted()["corners"])[1]}
    batch = U.crafted()["corners"].batch
    assert events[(309, 18)][3] == int(batch.lseq[18]) - 5 and events[(298, 19)][3] == int(batch.lseq[19]) - 1
    assert events[(294, 20)][2:] == (int(batch.lseq[20]) - 1, int(batch.lseq[20]))
    assert want[(253, "ATT")][:2] == [3, 2] and want[(273, "TGGTT")][:4] == [2, 0, 1, 37 * 5]
    assert 0 in U.crafted()["primer"].restated()[1]


def test_trimming_changes_the_bins_not_the_counts():
    case = U.crafted()["primer"]
    on, off = case.want(True), case.want(False)
    assert set(on) < set(off)               # (the clip takes the insertions that touch the primer along)
    assert all(off[k][:4] == v[:4] for k, v in on.items()) and any(off[k] != v for k, v in on.items())
    ds_on, ds_off = case.restated(True)[1], case.restated(False)[1]
    assert {0, 1, 2} <= set(ds_on) and not {0, 1, 2} & set(ds_off[:len(U.primer_reads(np.random.default_rng(0)))])


def test_guards_and_status(twin):
    """Entries of a row outside the batch, of a read with a status, with an interval that leaves its read: never tallied."""
    case = U.crafted()["corners"]
    cigars, events = oracle_run(case)
    bad = [(10, case.batch.n, 0, 2), (10, case.batch.n + 7, 0, 2), (10, 0, 3, 2), (10, 0, 0, int(case.batch.lseq[0]) + 1), (10, 0, -1, 2)]
    status = np.zeros(case.batch.n, np.uint8)
    status[3] = 4
    t = TwinTable(twin)
    info = t.run(case.batch, cigars, events + bad, status=status)
    dropped = [e for e in events if e[1] == 3]
    assert info["guarded"] == len(bad) + len(dropped) and dropped
    want = U.by_key(U.restate_without(case, {3}))
    assert t.table() == want


def test_a_full_table_loses_whole_keys(twin):
    """More alleles than a table of 16 slots holds: used + lost account for every event, no key has a wrong count."""
    reads = U.distinct(40) + U.copies(9)
    case = U.Crafted("full", reads)
    cigars, events = oracle_run(case)
    t = TwinTable(twin, 4)
    info = t.run(case.batch, cigars, events)
    got, want = t.table(), U.by_key(case.want())
    assert info["used"] == 16 == len(got) and info["lost"] == len(events) - sum(v[0] for v in got.values()) > 0
    assert all(want[k] == v for k, v in got.items())


def test_the_twin_s_own_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "insev_twin")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-DINSEV_TWIN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + INC + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "insev_twin ok" in out.stdout, out.stdout + out.stderr
