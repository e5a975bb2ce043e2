"""Crafted chunks for the DEFLATE encoder (amplipy_amd/csrc/amp_deflate.hip: k_deflate and its phases): every case sits on a limit
of the encoder, and carries the facts that follow from the encoder's own constants or from RFC 1951 -- which distance a token must
have, which it must never have, which length must be seen, what the header has to say.  None of them comes from a device run.

Plain Python and numpy: no GPU.  tests/test_deflate_enc_craft.py runs the list through the encoder's phases compiled for the host
(-DAMPDF_HOSTSIM) and reads the streams token by token (tests/deflate_read.py); tests/test_gpu_deflate_edges.py asks the device for
byte-identical streams, which carries every token-level fact over to it.

The constants below restate amp_deflate.hip; the CPU test reads the same names out of the source and fails when they drift, so an
encoder change that moves a limit has to move the cases with it.
"""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests.deflate_craft import DIST_BASE, LEN_BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "amplipy_amd", "csrc", "amp_deflate.hip")

# ---- the encoder's constants ---------------------------------------------------------------------------------------------------
BS_MAX = 0xFF00         # bytes of a chunk at most
SEG = 124               # bytes of a segment: one lane inserts a segment and parses about one
KWIN = 32               # segments a look-up reads: the position's own and the 31 in front of it
ROW = 128               # table slots of a segment
SCOUT = 32              # bytes at a segment's end that the scout parses
NICE_MATCH = 64         # a match this long is taken without a look at the next position
MIN_MATCH = 4
TOK_MAX = 256           # token slots of a lane
THREADS = 576
PIECE_BLOCKS = 256      # chunks per launch of the host-pointer entry
N_SLOTS = 2             # pieces in flight there
SOURCE_CONSTANTS = dict(BS_MAX=BS_MAX, SEG=SEG, KWIN=KWIN, ROW=ROW, SCOUT=SCOUT, NICE_MATCH=NICE_MATCH, MIN_MATCH=MIN_MATCH,
                        TOK_MAX=TOK_MAX, THREADS=THREADS, PIECE_BLOCKS=PIECE_BLOCKS, N_SLOTS=N_SLOTS)

# what follows from them
LANE_BYTES = 2 * SEG - 1            # a lane parses from where the lane in front ended (its segment's first byte at the earliest) up
                                    # to SEG - 1 bytes into the next segment: no token is longer; see DESIGN.md section 9
LONGEST_TOKEN = 2 * SEG - 2         # what families A to E reach: the first byte of a run or of a chunk is a literal
WINDOW = KWIN * SEG                 # no distance of this many bytes or more
UNSEEN_FROM = KWIN * SEG + SEG - 1  # from this distance on no position of the copy shares a look-up with its source

ROOM = 65536 - 26                   # what a BGZF block leaves a stream
GUARD = 96
PATTERN = 0xA5


# ---- the phases on the host -------------------------------------------------------------------------------------------------------
_hostsim = None


def hostsim_library():
    """libampdf_hostsim.so -- amp_deflate.hip's phases compiled for the host, thread after thread, phase after phase -- built once
    per session into a directory of its own."""
    global _hostsim
    if _hostsim is None:
        d = tempfile.mkdtemp(prefix="ampdf_hostsim_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libampdf_hostsim.so")
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                               "-o", so, SOURCE])
        L = C.CDLL(so)
        L.ampdf_hostsim_blocks.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.ampdf_hostsim_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _hostsim = L
    return _hostsim


def encode(call, data, block_bytes=None, room=ROOM, skew=0):
    """``call(in, n_bytes, block_bytes, out, stride, room, out_len)`` -- ampdf_hostsim_blocks, or amp_deflate_blocks behind its
    device number -- on ``data`` placed ``skew`` bytes behind a dword boundary, between other bytes: [stream or None per chunk].
    The bytes behind every stream and behind every room must be untouched."""
    n = len(data)
    block_bytes = block_bytes or max(n, 1)
    nb = (n + block_bytes - 1) // block_bytes
    stride = room + GUARD
    buf = np.arange(n + 24, dtype=np.uint32).astype(np.uint8) ^ 0x5A
    at = (-buf.ctypes.data) % 4 + 8 + skew
    buf[at:at + n] = np.frombuffer(data, np.uint8)
    out = np.full(max(nb, 1) * stride, PATTERN, np.uint8)
    lens = np.full(max(nb, 1), 0xFFFFFFFF, np.uint32)
    rc = call(buf.ctypes.data + at, n, block_bytes, out.ctypes.data, stride, room, lens.ctypes.data)
    assert rc == 0, "return code %d" % rc
    streams = []
    for k in range(nb):
        ln = int(lens[k])
        assert ln <= room, "chunk %d: length %d beyond the room %d" % (k, ln, room)
        assert (out[k * stride + ln:(k + 1) * stride] == PATTERN).all(), "chunk %d: bytes behind the stream / the room were written" % k
        streams.append(out[k * stride:k * stride + ln].tobytes() if ln else None)
    return streams


def host_lengths(freq, max_bits):
    """ampdf_hostsim_lengths: the code lengths the phases give these frequencies."""
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.full(f.size + 8, PATTERN, np.uint8)
    rc = hostsim_library().ampdf_hostsim_lengths(f.ctypes.data, f.size, max_bits, out.ctypes.data)
    assert rc == 0 and (out[f.size:] == PATTERN).all()
    return [int(x) for x in out[:f.size]]


# ---- what RFC 1951 says, restated ---------------------------------------------------------------------------------------------------
def length_symbol_of(length):
    """The literal/length symbol of a match length, 258 as symbol 285 (3.2.5)."""
    return 285 if length == 258 else 257 + max(i for i in range(28) if LEN_BASE[i] <= length)


def distance_symbol_of(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def run_length_rule(lengths):
    """3.2.7 on the HLIT + HDIST lengths back to back, greedy: a run of zeros goes out as 18s of at most 138, then one 17 if three
    or more are left, then single zeros; a run of another length as the length itself, then 16s of at most 6 while three or more
    are left, then single lengths.  A run does not end where the literal/length lengths do."""
    seq, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        left = j - i
        if v == 0:
            while left >= 11:
                r = min(left, 138); seq.append((18, r)); left -= r
            if left >= 3:
                seq.append((17, left)); left = 0
        else:
            seq.append(v); left -= 1
            while left >= 3:
                r = min(left, 6); seq.append((16, r)); left -= r
        seq += [v] * left
        i = j
    return seq


def kraft(lengths, unit):
    """Sum of 2^-l in units of 2^-unit: 1 << unit for a complete code."""
    return sum(1 << (unit - l) for l in lengths if l)


def runs_of(lengths):
    """[(value, run)] of the maximal runs."""
    out = []
    for v in lengths:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(v, r) for v, r in out]


def covered(tokens, dist, lo, hi):
    """Bytes of [lo, hi) that tokens of distance exactly ``dist`` stand for."""
    at, n = 0, 0
    for t in tokens:
        if isinstance(t, int):
            at += 1
            continue
        if t[1] == dist:
            n += max(0, min(hi, at + t[0]) - max(lo, at))
        at += t[0]
    return n


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
class Chunk:
    """One crafted chunk.  ``expect`` holds what its stream must show:
      dist        a distance some token must have                 cover     (lo, hi, floor): tokens of that distance stand for at
      no_dist     a distance no token may have                              least ``floor`` bytes of [lo, hi)
      stored      True: a stored block; False: a dynamic one      length    a length some token must have
      no_match    no token is a match                             hdist     HDIST; dist_lengths: the distance code lengths
      only_dsym   the one distance symbol the tokens use          zero_runs / code_runs: maximal runs the literal/length lengths hold
      why         the rule the case stands on"""

    def __init__(self, name, data, room=ROOM, **expect):
        self.name, self.family, self.data, self.room, self.expect = name, name[0], bytes(data), int(room), expect
        assert 1 <= len(self.data) <= BS_MAX

    def __repr__(self):
        return "Chunk(%s, %d bytes)" % (self.name, len(self.data))


def _rand(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, n, dtype=np.uint8).tobytes()


# -- A: sizes and alignment
A_SIZES = sorted({1, 2, 3, 4, 5, 123, 124, 125, 247, 248, 249, 3 * SEG - 1, 3 * SEG, 3 * SEG + 1, 526 * SEG - 1, 526 * SEG, 526 * SEG + 1,
                  BS_MAX - 1, BS_MAX})
SKEWS = (0, 1, 2, 3)


def acgt_with_repeats(rng, n):
    """n bytes of a 4-letter alphabet with planted repeats of 8 to 59 bytes."""
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    for _ in range(n // 150 + 1):
        L = int(rng.integers(8, 60))
        if n < 2 * L + 2:
            continue
        src = int(rng.integers(0, n - 2 * L))
        dst = int(rng.integers(src + L, n - L))
        a[dst:dst + L] = a[src:src + L]
    return a.tobytes()


def _family_a():
    rng = np.random.default_rng(11)
    return [Chunk("A_n%d" % n, acgt_with_repeats(rng, n), why="len <= n + 5; a stored block is exactly n + 5 bytes") for n in A_SIZES]


# -- B: the match window
B_SEED = 3
B_FLOOR = 150                                                       # of the 200 bytes of the second R
B_NEAR = tuple(range(3700, 3918, 7))
B_PICKED = (200, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073)
B_FAR = (UNSEEN_FROM, UNSEEN_FROM + 1, 4200, 5000)
# both ends of every distance symbol 0 ... 23 (3.2.5)
B_SMALL = tuple(sorted({DIST_BASE[k] for k in range(24)} | {DIST_BASE[k + 1] - 1 for k in range(23)}))


def window_chunk(rng, d):
    """500 random bytes, a 200-byte random string R, d - 200 random bytes, R again, 300 random bytes: (bytes, where the second R
    starts)."""
    r = _rand(rng, 200)
    return _rand(rng, 500) + r + _rand(rng, d - 200) + r + _rand(rng, 300), 500 + d


def near_chunk(rng, d, length=40):
    """A copy at distance d < 200 that the table can give: the copy starts on a segment boundary (a look-up never finds a source
    in the position's own segment: the slot holds the last position with a hash, the position itself or a later one), so its
    source starts in the segment in front, or the one before that.  The background is 64 byte values: it compresses, and four
    bytes of it hardly ever come twice.  (bytes, where the copy starts)."""
    p = 5 * SEG
    a = bytearray(_rand(rng, p + length + 200, 64, 128))
    unit = bytes(rng.permutation(64)[:d].astype(np.uint8)) if d <= 64 else _rand(rng, d, 0, 64)
    a[p - d:p] = unit
    for i in range(length):
        a[p + i] = a[p + i - d]
    a[p + length] = 200                                             # closes the copy
    return bytes(a), p


def _family_b():
    rng = np.random.default_rng(B_SEED)
    out = []
    for d in B_PICKED + B_NEAR:
        data, at = window_chunk(rng, d)
        out.append(Chunk("B_d%d" % d, data, dist=d, cover=(at, at + 200, B_FLOOR), stored=False,
                         why="a source at most KWIN - 1 segments in front of the position is looked up"))
    for d in B_FAR:
        data, at = window_chunk(rng, d)
        out.append(Chunk("B_far_d%d" % d, data, no_dist=d, stored=True,
                         why="from KWIN * SEG + SEG - 1 bytes on no position of the copy sees its source: random bytes, a stored block"))
    for d in B_SMALL:
        if d < 200:                                                  # (floor: the lazy step may send the copy's first byte as a literal,
            data, at = near_chunk(rng, d)                            # and fewer than MIN_MATCH bytes at its end start no match)
            out.append(Chunk("B_small_d%d" % d, data, dist=d, cover=(at, at + 40, 36), stored=False,
                             why="a copy on a segment boundary sees a source in the segments in front, however near"))
        elif d not in B_PICKED:
            data, at = window_chunk(rng, d)
            out.append(Chunk("B_d%d" % d, data, dist=d, cover=(at, at + 200, B_FLOOR), stored=False, why="both ends of a distance symbol"))
    return out


# -- C: match lengths
C_LENGTHS = (4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 18, 19, 34, 35, 66, 67, 130, 131, 226, 227, 246)
C_RUNS = (257, 258, 259, 260, 261, 262, 263, 516, 517, 518, 65279, 65280)


def length_chunk(rng, length):
    """An L-byte copy closed by a differing byte, inside one lane's range: it starts on a segment boundary (where the lane in
    front, parsing literals, ends) and is at most 2 * SEG - 1 bytes long, so it ends at or in front of the lane's limit.  Its source
    starts on the last byte of a segment: a segment's ROW slots keep the last position of a hash value, and no later one is there
    to take the slot."""
    p, q = 6 * SEG, 2 * SEG - 1
    a = bytearray(_rand(rng, p + length + 300, 64, 128))
    a[q:q + length] = _rand(rng, length, 0, 64)
    a[q + length] = 201
    a[p:p + length] = a[q:q + length]
    a[p + length] = 202
    return bytes(a), p - q


def _family_c():
    rng = np.random.default_rng(17)
    out = []
    for L in C_LENGTHS:
        data, d = length_chunk(rng, L)
        out.append(Chunk("C_len%d" % L, data, length=L, dist=d, stored=False, why="an L-byte copy closed by a differing byte is one token"))
    for n in C_RUNS:
        out.append(Chunk("C_run%d" % n, b"a" * n, stored=False, only_dsym=0,
                         why="a run is a literal and matches of distance 1, none longer than 2 * SEG - 2"))
    return out


# -- D: Huffman codes and the header
def fibonacci_bytes():
    """Byte values with Fibonacci frequencies, shuffled: a Huffman tree of the BYTES would be 21 deep."""
    f = [1, 1]
    while sum(f) + f[-1] + f[-2] <= BS_MAX:
        f.append(f[-1] + f[-2])
    vals = np.concatenate([np.full(c, (7 * i + 3) & 0xFF, np.uint8) for i, c in enumerate(f)])
    np.random.default_rng(1).shuffle(vals)
    return vals.tobytes()


def no_match_bytes(rng, counts):
    """The byte values of {value: count} in an order that leaves nothing for a match of MIN_MATCH bytes: no byte five times in a
    row (distance 1), and no four bytes twice unless the chunk is one segment (a source is never found in the position's own)."""
    vals = np.concatenate([np.full(c, v, np.uint8) for v, c in sorted(counts.items())])
    for _ in range(2000):
        rng.shuffle(vals)
        b = vals.tobytes()
        grams = {b[i:i + 4] for i in range(len(b) - 3)}
        if not any(bytes([v]) * 5 in b for v in counts) and (len(b) <= SEG or len(grams) == len(b) - 3):
            return b
    raise AssertionError("no order without a match")


# Code lengths by construction: counts that are powers of two and sum to a power of two (the end-of-block code counts 1) leave a
# Huffman code no choice: length = log2(total / count).
D_RUNS_1 = [("code", 3), ("zero", 2), ("code", 4), ("zero", 3), ("code", 6), ("zero", 10), ("code", 7), ("zero", 11), ("code", 8), ("zero", 138)]
D_ZERO_RUNS = (2, 3, 10, 11, 138, 139)
D_CODE_RUNS = (3, 4, 6, 7, 8)


def _runs_case_1(rng):
    counts, v = {}, 0
    for kind, run in D_RUNS_1:                                       # 28 values of count 8: five bits each
        if kind == "code":
            for i in range(run):
                counts[v + i] = 8
        v += run
    assert v == 192 and len(counts) == 28
    counts.update({192: 1, 210: 2, 220: 4, 230: 8, 240: 16})        # with the end-of-block code: 224 + 31 + 1 = 256
    assert sum(counts.values()) == 255
    return no_match_bytes(rng, counts)


def _runs_case_2(rng):
    counts = {0: 32, 140: 16, 141: 8, 142: 4, 200: 2, 201: 1}        # values 1 ... 139 unused: a run of 139 zeros; total 63 + 1
    return no_match_bytes(rng, counts)


def _two_values(rng):
    while True:
        b = bytes(rng.integers(0, 2, 100, dtype=np.uint8) + 0x30)
        if b"\x30" * 5 not in b and b"\x31" * 5 not in b:
            return b


def _family_d():
    rng = np.random.default_rng(23)
    out = [Chunk("D_one_value", b"\x07" * 300, stored=False, only_dsym=0, hdist=2, dist_lengths=[1, 1]),
           Chunk("D_two_values", _two_values(rng), stored=False, no_match=True, hdist=2, dist_lengths=[1, 1],
                 why="one segment: no source in a segment in front, no run of five"),
           Chunk("D_all_values", bytes(np.concatenate([np.arange(256), rng.geometric(0.03, 3744).clip(0, 255)]).astype(np.uint8)),
                 stored=False, all_literals=True),
           Chunk("D_no_match", no_match_bytes(rng, {65 + i: 24 - 2 * i for i in range(8)}), stored=False, no_match=True, hdist=2,
                 dist_lengths=[1, 1], why="phase 4: a chunk without a match still sends two distance codes of one bit")]
    # exactly one distance used: symbol 0, 1 and 5 (phase 4 gives symbols 0 and 1 a count when fewer than two are used)
    out.append(Chunk("D_only_dsym0", _rand(rng, 150, 64, 128) + b"\x09" * 60 + _rand(rng, 100, 64, 128), stored=False, only_dsym=0, hdist=2,
                     dist_lengths=[1, 1]))
    for sym, d in ((1, 2), (5, 7)):
        data, _ = near_chunk(rng, d)
        want = [1, 1] if sym == 1 else [2, 2, 0, 0, 0, 1]
        out.append(Chunk("D_only_dsym%d" % sym, data, stored=False, only_dsym=sym, hdist=len(want), dist_lengths=want, dist=d))
    out.append(Chunk("D_runs_1", _runs_case_1(rng), stored=False, no_match=True, zero_runs=(2, 3, 10, 11, 138), code_runs=D_CODE_RUNS,
                     why="counts that are powers of two: five bits for 28 values laid out in runs"))
    out.append(Chunk("D_runs_2", _runs_case_2(rng), stored=False, no_match=True, zero_runs=(139,), why="values 1 ... 139 unused"))
    # (its repeats become matches and the literal counts flatten: the tree of its tokens is 14 deep, phase 8 has nothing to do)
    out.append(Chunk("D_fibonacci", fibonacci_bytes(), stored=False, why="byte values with Fibonacci counts"))
    return out


# -- E: room
def _family_e():
    """(name, bytes): three compressible chunks and an incompressible one; the rooms follow from the stream length the full room
    gives, so the test derives them (room_cases)."""
    rng = np.random.default_rng(29)
    return [Chunk("E_acgt", acgt_with_repeats(rng, 3000), stored=False),
            Chunk("E_text", b"".join(b"read%07d\tACGTACGTTTGACCA\tIIIIIIIIIIIIIII\n" % (i * 7919 % 100000) for i in range(200)), stored=False),
            Chunk("E_short", acgt_with_repeats(rng, 40), stored=False, why="40 + 5 bytes of a stored block hardly leave room"),
            Chunk("E_random", _rand(rng, 2000), stored=True)]


def room_cases(chunk, full_stream):
    """[(room, what must come back)] for a chunk of family E whose stream with the full room is ``full_stream``: 'same' (that
    stream), 'stored', or None (out_len 0)."""
    n, S = len(chunk.data), len(full_stream)
    if chunk.expect["stored"]:
        assert S == n + 5
        return [(n + 5, "stored"), (n + 4, None)]
    assert S < n + 5
    return [(S, "same"), (S - 1, "stored" if n + 5 <= S - 1 else None), (n + 5, "same"), (n + 4, "same")]


# -- X: beside the families: a copy of 2 * SEG - 1 bytes from a segment boundary on fills a lane's whole range
def _family_x():
    rng = np.random.default_rng(37)
    out = []
    for L in (LANE_BYTES, LANE_BYTES + 1, 258):
        data, d = length_chunk(rng, L)
        out.append(Chunk("X_len%d" % L, data, length=LANE_BYTES, dist=d, stored=False,
                         why="a lane's range is at most 2 * SEG - 1 bytes: a longer copy is cut there"))
    return out


FAMILY_A, FAMILY_B, FAMILY_C, FAMILY_D, FAMILY_E, FAMILY_X = _family_a(), _family_b(), _family_c(), _family_d(), _family_e(), _family_x()
CHUNKS = FAMILY_A + FAMILY_B + FAMILY_C + FAMILY_D + FAMILY_E + FAMILY_X
assert len({c.name for c in CHUNKS}) == len(CHUNKS)


# -- chunks in a row: for the paths that take several
def bam_like(rng, n):
    """n bytes that look like BAM records: a few binary fields, a name, packed bases, qualities."""
    out = bytearray()
    k = 0
    while len(out) < n:
        pos = 1000 + 37 * k
        out += np.array([180, 0, pos, 0x12004908, 0x00630001, 100, 0, pos + 150, 200], np.int32).tobytes()
        out += b"read%06d\0" % k
        out += rng.integers(0, 256, 50, dtype=np.uint8).tobytes() if k % 2 == 0 else bytes(rng.choice([0x11, 0x12, 0x24, 0x48, 0x88, 0x41], 50).astype(np.uint8))
        out += bytes(rng.choice([37, 37, 37, 25, 11, 2], 100).astype(np.uint8))
        k += 1
    return bytes(out[:n])


def unlike_chunks(rng, n_chunks, per_group, size=300):
    """Chunks of ``size`` bytes such that the chunks a workgroup takes one after the other (k, k + per_group, k + 2 per_group ...)
    are a long Huffman stream, then one byte value, then a stored block, and so on: what one leaves in LDS the next must not see."""
    out = []
    for k in range(n_chunks):
        kind = (k % per_group + k // per_group) % 3
        if kind == 0:
            out.append(acgt_with_repeats(rng, size))
        elif kind == 1:
            out.append(bytes([65 + k % 26]) * size)
        else:
            out.append(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    return b"".join(out)


# -- F: frequencies for build_lengths
def fibonacci_freq(n, total):
    """Fibonacci counts as far as ``total`` allows, then ones, over n symbols."""
    f = [1, 1]
    while len(f) < n and sum(f) + f[-1] + f[-2] + (n - len(f) - 1) <= total:
        f.append(f[-1] + f[-2])
    return f + [1] * (n - len(f))


def lengths_inputs():
    """[(name, frequencies, max_bits)].  The counts of a chunk's literal/length and distance symbols sum to at most BS_MAX + 1, those
    of its code-length symbols to at most 286 + 30; the named cases keep to that, and two leave it behind on purpose (the plain
    Fibonacci numbers over 19 and 30 symbols, which fit 32 bits)."""
    rng = np.random.default_rng(31)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    out = [("fibonacci_19_of_7", fib[:19], 7), ("fibonacci_19_of_7_in_316", fibonacci_freq(19, 316), 7),
           ("fibonacci_30_of_15", fib[:30], 15), ("fibonacci_30_of_15_in_chunk", fibonacci_freq(30, BS_MAX + 1), 15),
           ("fibonacci_286_of_15", fibonacci_freq(286, BS_MAX + 1), 15)]
    for n, bits, total in ((19, 7, 316), (30, 15, BS_MAX + 1), (286, 15, BS_MAX + 1)):
        tag = "%d_of_%d" % (n, bits)
        out.append(("equal_" + tag, [total // n] * n, bits))
        out.append(("ones_" + tag, [1] * n, bits))
        out.append(("heavy_" + tag, [1] * (n // 2) + [total - n + 1] + [1] * (n - n // 2 - 1), bits))
        out.append(("two_" + tag, [0] * (n - 2) + [1, total - 1] if n != 30 else [3] + [0] * 28 + [5], bits))
        out.append(("two_equal_" + tag, [7, 7] + [0] * (n - 2), bits))
        for k in range(200):
            kind = k % 4
            if kind == 0:                                            # a few heavy symbols over a floor of rare ones
                f = rng.integers(0, 3, n) + (rng.random(n) < 0.15) * rng.integers(1, total // 8, n)
            elif kind == 1:                                          # geometric: deep trees
                f = np.floor(total * 0.5 ** (np.arange(n) * rng.uniform(0.3, 1.2)) / 2).astype(np.int64)
                rng.shuffle(f)
            elif kind == 2:                                          # a random cut of the Fibonacci counts, some symbols unused
                f = np.array(fibonacci_freq(n, total)) * (rng.random(n) < 0.9)
                rng.shuffle(f)
            else:
                f = rng.integers(0, max(2, 2 * total // n), n)
            f = np.asarray(f, np.int64)
            if np.count_nonzero(f) < 2:
                f[:2] = 1
            while f.sum() > total:                                   # back inside what a chunk can count
                f = np.where(f > 1, f * 3 // 4, f)
            out.append(("random_%s_%d" % (tag, k), [int(x) for x in f], bits))
    return out


def optimal_limited_cost(freq, max_bits):
    """Bits of an optimal code no deeper than max_bits for the used symbols of ``freq``: package-merge (Larmore and Hirschberg 1990).
    Every used symbol is a coin of each width 2^-1 ... 2^-max_bits with its count as the cost; pairs of a width are packaged into
    coins of the next; the 2m - 2 cheapest coins of width 2^-1 are what a code of m symbols pays."""
    w = sorted(f for f in freq if f)
    m = len(w)
    assert m >= 2 and (1 << max_bits) >= m
    packages = []
    for _ in range(max_bits):
        merged = sorted(w + packages)
        packages = [merged[i] + merged[i + 1] for i in range(0, len(merged) - 1, 2)]
        last = merged
    return sum(last[:2 * m - 2])


def dump(path, items):
    """[(name, bytes, room)] into one file for tests/hostsim/deflate_enc_main.cpp: per item a line ``name n_bytes room`` and the
    bytes."""
    with open(path, "wb") as f:
        for name, data, room in items:
            f.write(b"%s %d %d\n" % (name.encode(), len(data), room))
            f.write(data)
