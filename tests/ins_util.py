"""Insertion events under test: the plain reference tally, crafted reads, layouts of the device list, and the ctypes side of the
CPU twin (tests/hostsim/ins_twin.cpp).  Shared by tests/test_ins_twin.py (no GPU) and tests/test_gpu_ins.py.

The reference is a Counter of (ref_pos, text) with the text from amplipy_amd.insertions.event_strings -- Python slicing of the
unpacked base codes -- over the events of the CPU oracle."""
import ctypes as C
from collections import Counter

import numpy as np

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from amplipy_amd.insertions import event_strings
from amplipy_amd.segment import Segment
from oracle import oracle

FULL = 2 ** 64 - 1
MASKS = [0, 1, 0xF, FULL]                      # bits of the hash key the twin sorts by
SLOT_COUNTS = [1, 2, 255, 256, 257, 2049]      # one lane, two, a block of the k_ins_* kernels less one, exactly, plus one, several blocks
EVENT_COUNTS = [1, 255, 256, 257, 2049]
UNUSED = (-1, 0, 0, 0)
MQ, W = 20, 4


# ---- the reference ----------------------------------------------------------------------------------------
def rows_of(events, read_base):
    """The events with their read ids turned into rows of the batch: ids are 32-bit, relative to read_base modulo 2^32."""
    rows = np.array(events, abi.INS_EVENT_DTYPE)
    rows["read"] = ((events["read"].astype(np.int64) - (int(read_base) & 0xFFFFFFFF)) & 0xFFFFFFFF).astype(np.uint32)
    return rows


def assert_in_batch(batch, events, read_base=0):
    """Every event names a row of the batch and a query range inside that read.  The device calls that fetch allele bases hold
    q_to against nothing: nothing is handed to them before this has passed."""
    rows = rows_of(events, read_base)
    assert (rows["ref_pos"] >= 0).all()
    assert (rows["read"].astype(np.int64) < batch.n).all(), "an event names a read outside its batch"
    lseq = batch.lseq[rows["read"].astype(np.int64)].astype(np.int64)
    assert ((rows["q_from"] >= 0) & (rows["q_from"] <= rows["q_to"]) & (rows["q_to"].astype(np.int64) <= lseq)).all(), "an event's query range leaves its read"
    return rows


def pairs(batch, events, read_base=0):
    """[(ref_pos, text)] per event, in order."""
    return event_strings(batch, assert_in_batch(batch, events, read_base), 0)


def tally(batch, events, read_base=0):
    return Counter(pairs(batch, events, read_base))


def per_position(events, ref_len):
    """Events per reference position: what the device keeps in ins_at."""
    return np.bincount(events["ref_pos"].astype(np.int64), minlength=ref_len).astype(np.uint32)


def no_primers(ref_len):
    mn = np.full(ref_len, -1, np.int32)
    return mn, mn.copy(), 0


def oracle_events(batch, ref_len, read_base=0):
    """The CPU oracle on the batch without primers at MQ / W -> its result (events with ids read_base + row modulo 2^32)."""
    mn, mx, mpl = no_primers(ref_len)
    return oracle.process(batch, ref_len, mn, mx, mpl, MQ, W, read_base=read_base)


# ---- crafted reads ---------------------------------------------------------------------------------------------
def seg(pos, cigar, seq, qual=None, flag=0):
    q = [37] * len(seq) if qual is None else list(qual)
    assert len(q) == len(seq) and sum(n for op, n in Segment(cigar=cigar).cigartuples if op in (0, 1, 4, 7, 8)) == len(seq), cigar
    return Segment(flag=flag, reference_start=pos, cigar=cigar, template_length=0, query_sequence=seq, query_qualities=q)


TRAILING = "trailing insertion"


def crafted_segments():
    """[(name, Segment)]: the allele shapes the reference produces at the edges of SEQ[q_from:q_to] (A:730-748).  All but the
    trailing insertion have status 0; that one raises in the reference (the run reaches the end of the pairs, A:734) and records
    nothing."""
    lowq = [37] * 12; lowq[6] = 5
    return [
        ("empty allele", seg(50, "2I8M", "TTACGTACGT")),                         # SEQ[-1:2] = ''
        ("to the read's end", seg(60, "4M2I3D4M", "ACGTTTACGT")),                # insertion, then a deletion: SEQ[3:None]
        ("anchored at position 0", seg(0, "2I5M", "GGACGTA")),                   # r == 0: SEQ[0:3]
        ("cut by a low quality", seg(70, "4M4I4M", "ACGTCCCCACGT", lowq)),       # the first part lands on ref_end - 1
        ("odd nibble start", seg(80, "4M2I4M", "ACGTGGACGT")),                   # SEQ[3:6]
        ("even nibble start", seg(80, "5M2I3M", "ACGTAGGCGT")),                  # SEQ[4:7]
        ("N and IUPAC codes", seg(90, "4M5I4M", "ACGTNRYKMACGT")),
        ("lower case", seg(100, "4M2I4M", "acgtggacgt")),
        ("upper case twin of it", seg(100, "4M2I4M", "ACGTGGACGT")),
        ("anchor A", seg(110, "4M2I4M", "ACGATTCGTA")),
        ("anchor C", seg(110, "4M2I4M", "ACGCTTCGTA")),
        ("200 bases", seg(120, "4M200I4M", "ACGT" + "ACGGTCA" * 28 + "ACGT" + "ACGT")),
        ("equal up to the last base, C", seg(130, "4M6I4M", "ACGTACGTACACGT")),
        ("equal up to the last base, G", seg(130, "4M6I4M", "ACGTACGTAGACGT")),
        ("TT", seg(140, "4M2I4M", "ACGATTCGTA")),
        ("TTT", seg(140, "4M3I4M", "ACGATTTCGTA")),
        ("the same text elsewhere", seg(150, "4M2I4M", "ACGATTCGTA")),
        ("reverse strand", seg(140, "4M2I4M", "ACGATTCGTA", flag=16)),
        (TRAILING, seg(160, "4M3I", "ACGTGGG")),
    ]


def _digits(i, n=6):
    return "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(n))


def distinct_segments(n, pos=300, first=0):
    """n reads with one 6-base insertion each, all different, at one position behind one anchoring base: one event per read."""
    assert first + n <= 4096
    return [seg(pos, "20M6I20M", "ACGTACGTACGTACGTACGA" + _digits(first + i) + "CGTACGTACGTACGTACGTA") for i in range(n)]


def copies_segments(n, pos=400, alleles=("GATTAC", "GATTAG", "CATTAC")):
    """n reads with one 6-base insertion each, of few alleles in turn: one event per read."""
    return [seg(pos, "20M6I20M", "ACGTACGTACGTACGTACGA" + alleles[i % len(alleles)] + "CGTACGTACGTACGTACGTA") for i in range(n)]


def plain_segments(n, rng, ref_len):
    """Reads of 10 to 210 bases without an insertion: filler that records nothing."""
    out = []
    for _ in range(n):
        L = int(rng.integers(10, 211))
        out.append(seg(int(rng.integers(0, ref_len - L)), "%dM" % L, "".join(rng.choice(list("ACGT"), L))))
    return out


def batch_with_events(n_events, kind, ref_len, seed=0):
    """A batch whose oracle event list has exactly n_events entries: the crafted reads when they fit, plain filler, and reads of
    ``kind`` ("copies": few alleles many times, "distinct": all alleles different), shuffled.  -> (batch, oracle result)."""
    rng = np.random.default_rng(seed + n_events)
    crafted = [s for _, s in crafted_segments()]
    n_crafted = oracle_events(ReadBatch.from_segments(crafted), ref_len).events.size
    segs = (crafted if n_events > n_crafted else []) + plain_segments(min(n_events, 40), rng, ref_len)
    left = n_events - (n_crafted if n_events > n_crafted else 0)
    segs += distinct_segments(left) if kind == "distinct" else copies_segments(left)
    segs = [segs[i] for i in rng.permutation(len(segs))]
    b = ReadBatch.from_segments(segs)
    a = oracle_events(b, ref_len)
    assert a.events.size == n_events
    return b, a


# ---- layouts of the device list: eight regions of `cap` slots, shard_n[s] in use ---------------------------------
STALE_POS = 1999      # where the slots beyond a region's fill claim an event: no read of these tests has one there


def make_list(shards, cap, read_base=0):
    """shards: eight arrays of slots (INS_EVENT_DTYPE; ref_pos -1 = reserved and not used).  -> (regions [8 * cap], shard_n
    uint64[8]).  The slots beyond a region's fill are never to be looked at: they hold what a batch before might have left there,
    an event of row 0 at STALE_POS, so that a step that does look shows up as a wrong tally."""
    assert len(shards) == 8 and all(len(s) <= cap for s in shards)
    regions = np.zeros(8 * cap, abi.INS_EVENT_DTYPE)
    regions["ref_pos"] = STALE_POS; regions["read"] = int(read_base) & 0xFFFFFFFF; regions["q_to"] = 1
    for s, slots in enumerate(shards):
        regions[s * cap:s * cap + len(slots)] = slots
    return regions, np.array([len(s) for s in shards], np.uint64)


def slots_of(events, n_slots, where, rng=None):
    """n_slots slots that hold ``events`` and unused slots: where = "start" / "middle" / "end" / "scattered"."""
    n_un = n_slots - events.size
    assert n_un >= 0
    un = np.array([UNUSED] * n_un, abi.INS_EVENT_DTYPE)
    if where == "start":
        return np.concatenate([un, events])
    if where == "end":
        return np.concatenate([events, un])
    if where == "middle":
        h = events.size // 2
        return np.concatenate([events[:h], un, events[h:]])
    out = np.concatenate([events, un])
    return out[rng.permutation(out.size)]


def spread(slots, shards, rng=None):
    """The slots dealt to the given shards in uneven consecutive pieces (every named shard gets at least one when there are
    enough) -> the eight arrays."""
    out = [np.zeros(0, abi.INS_EVENT_DTYPE) for _ in range(8)]
    k = len(shards)
    if slots.size < k:
        cuts = [min(i, slots.size) for i in range(k + 1)]
    elif k == 1:
        cuts = [0, slots.size]
    else:
        inner = np.sort(rng.choice(np.arange(1, slots.size), k - 1, replace=False)) if slots.size > k else np.arange(1, k)
        cuts = [0] + [int(c) for c in inner] + [slots.size]
    for i, s in enumerate(shards):
        out[s] = slots[cuts[i]:cuts[i + 1]]
    return out


def flat_slots(regions, cap, shard_n):
    """The slots in use, concatenated shard by shard: the numbering the aggregation works in."""
    return np.concatenate([regions[s * cap:s * cap + int(shard_n[s])] for s in range(8)]) if int(shard_n.sum()) else np.zeros(0, abi.INS_EVENT_DTYPE)


# ---- the CPU twin --------------------------------------------------------------------------------------------
def run_twin(L, regions, cap, shard_n, batch, read_base, mask):
    """twin_ins_aggregate -> (runs INS_RUN_DTYPE[n_runs], run_of_slot uint32[n_slots], n_events)."""
    n = int(shard_n.sum())
    runs = np.zeros(max(n, 1), abi.INS_RUN_DTYPE); ros = np.zeros(max(n, 1), np.uint32)
    ne, nr = C.c_int64(-1), C.c_int64(-1)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    p = lambda a: C.c_void_p(abi.ptr(np.ascontiguousarray(a)))
    keep = [pad(np.ascontiguousarray(regions)), np.ascontiguousarray(shard_n, np.uint64), np.ascontiguousarray(batch.seq_off // 8, np.uint32), pad(batch.seq)]
    rc = L.twin_ins_aggregate(p(keep[0]), C.c_longlong(cap), p(keep[1]), p(keep[2]), p(keep[3]), C.c_uint64(int(read_base)), C.c_uint64(int(mask)),
                              p(runs), p(ros), C.byref(ne), C.byref(nr))
    assert rc == 0
    return runs[:int(nr.value)], ros[:n], int(ne.value)


def run_rows(runs):
    rows = np.zeros(runs.size, abi.INS_EVENT_DTYPE)
    for f in ("ref_pos", "read", "q_from", "q_to"):
        rows[f] = runs[f]
    return rows


def pos_keys(rows):
    return (rows["ref_pos"].astype(np.int64) << 32) | (rows["q_to"].astype(np.int64) - rows["q_from"].astype(np.int64))


def check_runs(runs, batch, read_base, want, events=None):
    """What every list of runs owes the tally ``want``: counts summed by (ref_pos, text) equal it, reserved is 0, position keys
    never decrease, and (events given: the plain event list) every representative is one of the events.  -> the runs' texts."""
    rows = run_rows(runs)
    text = pairs(batch, rows, read_base)
    got = Counter()
    for k, c in zip(text, runs["count"].tolist()):
        got[k] += c
    assert got == want
    assert (runs["count"] > 0).all() and not runs["reserved"].any()
    assert (np.diff(pos_keys(rows)) >= 0).all(), "runs are ordered by (ref_pos, length)"
    if events is not None:
        have = set(map(tuple, events.tolist()))
        assert all(tuple(r) in have for r in rows.tolist()), "a representative is no event of the list"
    return text


def check_twin(L, regions, cap, shard_n, batch, read_base, mask):
    """The twin on the list against the plain tally, for any mask.  -> (n_runs, n_distinct)."""
    slots = flat_slots(regions, cap, shard_n)
    real = slots[slots["ref_pos"] >= 0]
    want = tally(batch, real, read_base)
    runs, ros, n_events = run_twin(L, regions, cap, shard_n, batch, read_base, mask)
    assert n_events == real.size == int(runs["count"].sum())
    text = check_runs(runs, batch, read_base, want, real)
    # no run mixes texts: the text of EVERY event against that of the run it went to, and the representative among them
    used = slots["ref_pos"] >= 0
    assert (ros[~used] == 0xFFFFFFFF).all() and (ros[used] < runs.size).all()
    ev_text = pairs(batch, real, read_base)
    members = np.bincount(ros[used].astype(np.int64), minlength=runs.size)
    assert np.array_equal(members, runs["count"].astype(np.int64))
    rep_seen = np.zeros(runs.size, bool)
    rows = run_rows(runs)
    for e, t, r in zip(real.tolist(), ev_text, ros[used].tolist()):
        assert t == text[r], "a run mixes alleles"
        if tuple(e) == tuple(rows[r].tolist()):
            rep_seen[r] = True
    assert rep_seen.all(), "a representative is not an event of its run"
    if mask == FULL:
        assert runs.size == len(want)
    else:
        assert runs.size >= len(want)
    return runs.size, len(want)


# ---- the device side ------------------------------------------------------------------------------------------
def _runs_as_counter(e, runs, read_base):
    """{(ref_pos, allele text): events} of Engine.aggregate_events records (text of the representative events from the device)."""
    rows = np.zeros(runs.size, abi.INS_EVENT_DTYPE)
    for f in ("ref_pos", "q_from", "q_to"):
        rows[f] = runs[f]
    rows["read"] = runs["read"] - np.uint32(read_base)
    length, blob = e.event_text(rows, 0) if runs.size else (np.zeros(0, np.int64), np.zeros(0, np.uint8))
    raw = blob.tobytes(); off = np.cumsum(length) - length
    out = Counter()
    for k in range(runs.size):
        out[(int(runs["ref_pos"][k]), raw[int(off[k]):int(off[k]) + int(length[k])].decode("ascii"))] += int(runs["count"][k])
    return out


def slots_in_use(e):
    """The size query of amp_get_ins_events (buf == NULL): list slots in use, unused ones included."""
    n = C.c_int64(0)
    e._chk(e.L.amp_get_ins_events(e.h, C.byref(n), None, C.c_int64(0)), "amp_get_ins_events")
    return int(n.value)
