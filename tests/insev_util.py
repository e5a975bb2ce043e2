"""TEST INFRASTRUCTURE of the insertion evidence: a plain restatement -- the oracle's events of a batch
(oracle/py_restatement.process_full: the reference's event rules, read by read), and per event rev, qsum, noqual, d and the bin
from the TRIMMED CIGAR with plain loops, tallied per (position, allele text) -- written from the definition and from nothing
in amplipy_amd/csrc; the crafted batches of tests/test_insev_twin.py and tests/test_gpu_insev.py; and the two ways a device or
twin table becomes the restatement's shape.  Shared by the CPU and the GPU tests: a case's restatement is computed once."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

from amplipy_amd import abi, insevidence
from oracle import oracle
from oracle import py_restatement as R
from tests import readpass_craft as K
from tests.readpass_craft import D, H, I, M, S

NT16 = "=ACMGRSVTWYHKDBN"
MQ, W = 20, 4
BIN_UPPER = (2, 4, 8, 16, 32, 64)               # d < 2, 2-3, 4-7, 8-15, 16-31, 32-63, >= 64
D_EDGES = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64)


# ---- the CPU twin ----------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN_SRC = os.path.join(ROOT, "tests", "hostsim", "insev_twin.cpp")
GXX = shutil.which("g++") or "g++"
INC = ["-I", os.path.join(ROOT, "amplipy_amd", "csrc")]
TWIN_CONSTANTS = ("BLOCK", "GRID", "BINS", "LOG2_DEFAULT", "LOG2_MIN", "LOG2_MAX", "SIDE_BYTES", "ENTRY_BYTES", "STRIDE")


def load_twin(directory):
    """tests/hostsim/insev_twin.cpp built with plain g++ into ``directory`` and loaded."""
    so = os.path.join(str(directory), "libinsev_twin.so")
    subprocess.check_call([GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INC + ["-o", so, TWIN_SRC])
    L = C.CDLL(so)
    L.twin_insev.restype = C.c_int
    L.twin_insev_constant.restype = C.c_int
    L.twin_insev_allele_hash.restype = C.c_uint64
    L.twin_insev_d.restype = C.c_int32
    L.twin_insev_d.argtypes = [C.c_int32] * 4
    L.twin_insev_bin.restype = C.c_uint32
    L.twin_insev_bin.argtypes = [C.c_int32]
    L.K = {name: L.twin_insev_constant(k) for k, name in enumerate(TWIN_CONSTANTS)}
    return L


def twin_hash(L, text):
    codes = codes_of(text) if text else np.zeros(1, np.uint8)
    return L.twin_insev_allele_hash(C.c_void_p(abi.ptr(codes)), C.c_int32(len(text)))


# ---- the restatement --------------------------------------------------------------------------------------------------------
def bin_of(d):
    for b, hi in enumerate(BIN_UPPER):
        if d < hi:
            return b
    return len(BIN_UPPER)


def primer_tables(ref_len, primers, offset=0):
    if not primers:
        mn = np.full(ref_len, -1, np.int32)
        return mn, mn.copy(), 0
    return oracle.find_overlapping_primers(ref_len, list(primers), offset)


def restate(batch, ref_len, tabs, do_trim, mq=MQ, w=W, skip=()):
    """{(ref_pos, allele text): [count, rev, noqual, qsum, b0 .. b6]} of the batch, and the per-event d values in event order.
    ``skip``: rows whose events are left out (reads given a status)."""
    _, events, trims = R.process_full(batch, ref_len, *tabs, mq, w, do_trim)
    table, ds = {}, []
    for ref_pos, read, lo, hi in events:
        if read in skip:
            continue
        _, cig, _ = trims[read]
        lseq = int(batch.lseq[read])
        s0 = int(batch.seq_off[read])
        qs, qe = R.query_alignment_start(cig), R.query_alignment_end(cig, lseq)
        text = ""
        for q in range(lo, hi):
            byte = int(batch.seq[(s0 + q) // 2])
            text += NT16[byte & 15 if (s0 + q) & 1 else byte >> 4]
        d = max(0, min(lo - qs, qe - hi))
        ds.append(d)
        c = table.setdefault((ref_pos, text), [0] * (4 + abi.INSEV_BINS))
        c[0] += 1
        c[1] += 1 if int(batch.flag[read]) & 0x10 else 0
        if lseq > 0 and int(batch.qual[s0]) == 0xFF:
            c[2] += 1
        else:
            for q in range(lo, hi):
                c[3] += int(batch.qual[s0 + q])
        c[4 + bin_of(d)] += 1
    return table, ds


def restate_without(case, rows):
    return restate(case.batch, case.G, case.tabs, case.do_trim, skip=set(rows))[0]


def add_tables(*tables):
    out = {}
    for t in tables:
        for k, v in t.items():
            c = out.setdefault(k, [0] * len(v))
            for j, x in enumerate(v):
                c[j] += x
    return out


def scaled(table, k):
    return {key: [x * k for x in v] for key, v in table.items()}


def by_key(table):
    """The restatement's table under the device keys: {(ref_pos, len, hash): cells} -- the Python port of the allele hash."""
    out = {}
    for (pos, text), v in table.items():
        key = insevidence.key_of(pos, text)
        assert key not in out, "two alleles of the test share a key"
        out[key] = list(v)
    return out


def entries_dict(entries):
    """abi.INSEV_ENTRY_DTYPE rows -> {(ref_pos, len, hash): cells}."""
    out = {}
    for k in range(entries.size):
        e = entries[k]
        key = (int(e["ref_pos"]), int(e["len"]), int(e["hash"]))
        assert key not in out, "one key in two slots"
        out[key] = [int(e["count"]), int(e["rev"]), int(e["noqual"]), int(e["qsum"])] + [int(b) for b in e["bin"]]
    return out


def triples_of(table):
    """EventStore.counted_pairs rows of a restated table."""
    return [(pos, text, v[0]) for (pos, text), v in table.items()]


# ---- crafted batches --------------------------------------------------------------------------------------------------------
class Crafted:
    def __init__(self, name, reads, G=600, primers=(), do_trim=True):
        self.name, self.reads, self.G, self.primers, self.do_trim = name, reads, G, list(primers), do_trim

    @functools.cached_property
    def batch(self):
        return K.build_batch(self.reads)

    @functools.cached_property
    def tabs(self):
        return primer_tables(self.G, self.primers)

    @functools.lru_cache(maxsize=None)
    def restated(self, do_trim=None):
        return restate(self.batch, self.G, self.tabs, self.do_trim if do_trim is None else do_trim)

    def want(self, do_trim=None):
        return self.restated(do_trim)[0]

    @functools.lru_cache(maxsize=None)
    def status(self, do_trim=None):
        """The reference-pinned oracle's status per read: a read it refuses (QUAL '*' is one) records nothing on the device."""
        return oracle.process(self.batch, self.G, *self.tabs, MQ, W, do_trim=self.do_trim if do_trim is None else do_trim, do_count=True).trim.status

    @functools.lru_cache(maxsize=None)
    def want_accepted(self, do_trim=None):
        """The restatement over the reads the oracle accepts: what the device table holds behind the real read pass."""
        do_trim = self.do_trim if do_trim is None else do_trim
        refused = set(np.nonzero(self.status(do_trim))[0].tolist())
        return restate(self.batch, self.G, self.tabs, do_trim, skip=refused)[0] if refused else self.want(do_trim)


def codes_of(text):
    return np.array([NT16.index(c) for c in text], np.uint8)


def read(pos, cig, text=None, qual=None, flag=0, rng=None, q=37):
    L = K.query_len(cig)
    if text is None:
        text = "".join("ACGT"[k] for k in (rng or np.random.default_rng(L)).integers(0, 4, L))
    assert len(text) == L, (cig, len(text))
    return K.Read(pos, cig, codes_of(text), np.full(L, q, np.uint8) if qual is None else np.asarray(qual, np.uint8), flag)


def edge_reads(rng):
    """An insertion at every bin edge's distance from the read's left end and from its right end."""
    out = []
    for d in D_EDGES:
        out.append(read(100, [(M, d + 1), (I, 2), (M, 80)], rng=rng))                   # q_from = d: the anchor base
        if d:
            out.append(read(100, [(M, 80), (I, 2), (M, d)], rng=rng, flag=16))          # q_to = 82, qe = 82 + d
    return out


def corner_reads(rng):
    low = np.full(4 + 4 + 4, 37, np.uint8); low[6] = 5
    long97 = "".join("ACGT"[k] for k in rng.integers(0, 4, 97))
    star = np.full(12, 37, np.uint8); star[0] = 0xFF
    return [
        read(150, [(S, 5), (I, 2), (M, 30)], rng=rng),                      # directly behind a soft clip: the anchor lies in the clip
        read(150, [(S, 5), (M, 1), (I, 2), (M, 30)], rng=rng),              # one base behind it
        read(200, [(M, 10), (I, 2), (D, 3), (M, 10)], rng=rng),             # to the next base over a deletion
        read(0, [(I, 2), (M, 12)], "GGACGTACGTACGT"),                       # anchored at position 0: r == 0
        read(50, [(I, 2), (M, 8)], "TTACGTACGT"),                           # the empty allele: SEQ[-1:2]
        read(210, [(M, 4), (I, 4), (M, 4)], "ACGTCCCCACGT", low),           # split by a low quality
        read(220, [(M, 4), (I, 1), (M, 4)], "ACGTGACGT"),                   # a one-base insertion (an allele of two), odd nibble start
        read(220, [(M, 5), (I, 1), (M, 3)], "ACGTAGCGT"),                   # even nibble start
        read(230, [(M, 4), (I, 96), (M, 4)], "ACGT" + long97[1:] + "ACGT"),    # an allele of 97 bases
        read(240, [(M, 4), (I, 6), (M, 4)], "ACGTACGTACACGT"),              # equal up to the last base, C
        read(240, [(M, 4), (I, 6), (M, 4)], "ACGTACGTAGACGT"),              # ... G
        read(250, [(M, 4), (I, 2), (M, 4)], "ACGATTCGTA"),                  # one allele forward ...
        read(250, [(M, 4), (I, 2), (M, 4)], "ACGATTCGTA", flag=16),         # ... and reverse
        read(250, [(M, 4), (I, 2), (M, 4)], "ACGATTCGTA", flag=16),
        read(260, [(M, 4), (I, 4), (M, 4)], "ACGTNRYKACGT"),                # IUPAC codes
        read(270, [(M, 4), (I, 4), (M, 4)], "ACGTGGTTACGT", star),          # QUAL '*'
        read(270, [(M, 4), (I, 4), (M, 4)], "ACGTGGTTACGT"),                # the same allele with qualities
        read(280, [(H, 3), (S, 2), (M, 6), (I, 3), (M, 9), (S, 4), (H, 2)], rng=rng),
        read(290, [(M, 20), (I, 2), (S, 5)], rng=rng),                      # at the read's last kept base: q_to = qe, d = 0 from the right
        read(290, [(M, 9), (I, 3), (S, 1), (H, 4)], rng=rng, flag=16),      # ... in front of one clipped base and a hard clip
        read(295, [(I, 2), (D, 2), (M, 10)], "TTACGTACGTAC"),               # an allele of length 1: SEQ[-1:None], the read's last base
    ]


def primer_reads(rng):
    """Reads that start inside the primer [300, 330): the trim soft-clips up to the primer's end, so an insertion just behind it
    sits at the start of the kept span -- and one INSIDE the primer region loses its anchor to the clip."""
    return [
        read(300, [(M, 31), (I, 2), (M, 40)], rng=rng),                     # the clip takes an insertion that touches the primer along
        read(300, [(M, 30), (I, 2), (M, 40)], rng=rng),
        read(300, [(M, 32), (I, 2), (M, 40)], rng=rng),                     # anchor = the first kept bases: d = 0, 1, 2 where the
        read(300, [(M, 33), (I, 2), (M, 40)], rng=rng),                     # untrimmed read has 31, 32, 33
        read(300, [(M, 34), (I, 2), (M, 40)], rng=rng),
        read(300, [(M, 35), (I, 3), (M, 40)], rng=rng),
        read(310, [(M, 28), (I, 2), (M, 40)], rng=rng, flag=16),
        read(340, [(M, 20), (I, 2), (M, 40)], rng=rng),                     # no primer at its start
    ]


@functools.lru_cache(maxsize=None)
def crafted():
    """{name: Crafted}: every crafted batch, built once."""
    rng = np.random.default_rng(19)
    cases = [
        Crafted("edges", edge_reads(rng)),
        Crafted("corners", corner_reads(rng)),
        Crafted("primer", primer_reads(rng) + edge_reads(rng)[:6], primers=[(300, 330)]),
        Crafted("untrimmed", primer_reads(rng) + corner_reads(rng), primers=[(300, 330)], do_trim=False),
    ]
    return {c.name: c for c in cases}


# ---- the routes of the read pass (tests/readpass_craft.py has the selection rules) ----------------------------------------------
def short_reads(n, rng, G, every=3, alleles=("GA", "TTC", "G")):
    """Plain short reads, every ``every``-th with one insertion of few alleles: k_fast's shape ([S] M I M [S], <= 152 bases)."""
    out = []
    for k in range(n):
        pos = int(rng.integers(0, G - 200))
        L = int(rng.integers(40, 140))
        if k % every:
            out.append(read(pos, [(M, L)], rng=rng, flag=16 * int(rng.integers(0, 2))))
            continue
        a = alleles[(k // every) % len(alleles)]
        left = int(rng.integers(1, 30))
        body = "".join("ACGT"[j] for j in rng.integers(0, 4, L))
        text = body[:left] + a + body[left:]
        qual = rng.integers(21, 41, len(text)).astype(np.uint8)
        out.append(read(pos, [(M, left), (I, len(a)), (M, L - left)], text, qual, flag=16 * int(rng.integers(0, 2))))
    return K.by_pos(out)


def irregular_reads(n, rng, G):
    """Reads no fast kernel takes: two insertions, insertions beside deletions, clips on both sides, low qualities inside an
    insertion, a skipped region in front of an insertion -- the general pass and the second pass."""
    out = []
    for k in range(n):
        pos = int(rng.integers(0, G - 300))
        kind = k % 5
        if kind == 0:
            cig = [(S, 3), (M, 20), (I, 2), (M, 15), (I, 3), (M, 20), (S, 2)]
        elif kind == 1:
            cig = [(M, 12), (I, 2), (D, 2), (M, 12), (D, 1), (I, 1), (M, 12)]
        elif kind == 2:
            cig = [(H, 2), (M, 30), (I, 9), (M, 30)]                        # longer than a fast kernel's insertion
        elif kind == 3:
            cig = [(M, 10), (I, 4), (M, 200)]                               # longer than a fast kernel's read
        else:
            cig = [(M, 20), (K.N_, 5), (I, 2), (M, 20), (S, 6)]
        L = K.query_len(cig)
        qual = rng.integers(21, 41, L).astype(np.uint8)
        if kind == 0 and k % 2:
            qual[24] = 3                                                    # inside the second insertion's neighbourhood
        out.append(read(pos, cig, rng=rng, qual=qual, flag=16 * int(rng.integers(0, 2))))
    return K.by_pos(out)


def many_op_reads(n, rng, G, nops=40):
    """Reads of ``nops`` ops, insertions and deletions in turn: the wave-per-read path (k_long) when the batch's mean is >= 8 ops."""
    return K.by_pos([K.many_ops(rng, int(rng.integers(0, G - 400)), nops + (k % 3) * 2, lead_clip=bool(k % 2)) for k in range(n)])


@functools.lru_cache(maxsize=None)
def routes():
    rng = np.random.default_rng(23)
    G = 3000
    return {c.name: c for c in [
        Crafted("short", short_reads(400, rng, G), G, primers=[(500, 530), (1500, 1530)]),
        Crafted("irregular", short_reads(150, rng, G) + irregular_reads(90, rng, G), G, primers=[(500, 530)]),
        Crafted("many ops", many_op_reads(70, rng, G), G),
    ]}


def copies(n, allele="GATTACA"[:4], pos=100, flag=0):
    """n identical reads with one insertion: one key n times."""
    r = read(pos, [(M, 20), (I, len(allele)), (M, 20)], "ACGTACGTACGTACGTACGA" + allele + "CGTACGTACGTACGTACGTA", flag=flag)
    return [r] * n


def distinct(n, pos=100, first=0):
    """n reads with one 6-base insertion each, all different."""
    digits = lambda i: "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(6))
    return [read(pos, [(M, 20), (I, 6), (M, 20)], "ACGTACGTACGTACGTACGA" + digits(first + i) + "CGTACGTACGTACGTACGTA", flag=16 * (i & 1)) for i in range(n)]


def uniform_batch(n, allele="GATT", pos=100, L=20):
    """n identical reads with one insertion, built without a Python object per read (for counts past the kernel's stride)."""
    from amplipy_amd.batch import ReadBatch
    text = "ACGTACGTACGTACGTACGA"[:L] + allele + "CGTACGTACGTACGTACGTA"[:L]
    width = len(text)
    codes = np.broadcast_to(codes_of(text), (n, width))
    cig = np.tile(np.array([(L << 4) | M, (len(allele) << 4) | I, (L << 4) | M], np.uint32), n)
    return ReadBatch.from_uniform(np.full(n, pos, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.int32), width, np.arange(0, 3 * n + 1, 3, dtype=np.uint64),
                                  cig, codes, np.full((n, width), 37, np.uint8))
