"""Crafted raw DEFLATE streams (RFC 1951) for the decoders of this project: a bit writer, stored / fixed / dynamic blocks written
from token lists and CHOSEN code lengths, the bytes those tokens stand for, and two fixed lists of cases -- VALID_CASES, which every
decoder here must inflate exactly, and REFUSED_CASES, which every decoder must refuse.  A generator, not a test: tests/
test_deflate_craft.py keeps it honest against zlib and tests/test_gpu_bam_edges.py feeds its streams to the device codec.

A token is an int (a literal byte), (length, distance), or (258, distance, 284): length 258 written as symbol 284 with 31 in its
extra bits, which inflate accepts like symbol 285.  Everything is deterministic: the random parts draw from seeded generators.
"""
import zlib

import numpy as np

# RFC 1951 3.2.5: base and extra bits of length symbols 257 ... 285 and of distance symbols 0 ... 29
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
PRE_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)                  # 3.2.7
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                                        # 3.2.6
FIXED_DIST = [5] * 32


class BitWriter:
    """Bits into bytes from the least significant bit up (3.1.1); Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc = self.n = 0

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical Huffman code of 3.2.2."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def length_symbol(length, codes, via284=False):
    """(symbol, extra bits, extra value).  258 is symbol 285, or 284 + 31 when asked for or when 285 has no code."""
    if length == 258 and not via284 and 285 in codes:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    assert length - LEN_BASE[k] < (1 << LEN_EXTRA[k])
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def distance_symbol(dist):
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    assert dist - DIST_BASE[k] < (1 << DIST_EXTRA[k])
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def play(tokens, start=b""):
    """The bytes the tokens stand for, behind ``start``."""
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= len(out) and dist <= 32768
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(start):])


def balanced(n):
    """Lengths of a complete code of n >= 2 symbols, as even as can be."""
    d = n.bit_length() - 1
    return [d] * ((2 << d) - n) + [d + 1] * (2 * n - (2 << d))


def run_length(lengths):
    """A plain code-length sequence for ``lengths``: ints 0 ... 15 and (16 | 17 | 18, repeat) items."""
    seq, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            seq.append((18, r) if r >= 11 else (17, r))
            i += r
        elif v and run >= 4:
            r = min(run - 1, 6)
            seq += [v, (16, r)]
            i += 1 + r
        else:
            seq.append(v)
            i += 1
    return seq


class Stream:
    """One raw DEFLATE stream under construction: blocks are appended, ``done()`` gives the bytes."""

    def __init__(self):
        self.w = BitWriter()

    def done(self):
        return self.w.done()

    def stored(self, data, final):
        w = self.w
        w.bits(1 if final else 0, 1); w.bits(0, 2)
        w.align()
        w.bits(len(data), 16); w.bits(len(data) ^ 0xFFFF, 16)
        w.raw(data)
        return self

    def _symbols(self, tokens, lit, dst):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*lit[t])
                continue
            sym, eb, ev = length_symbol(t[0], lit, len(t) > 2 and t[2] == 284)
            w.code(*lit[sym]); w.bits(ev, eb)
            sym, eb, ev = distance_symbol(t[1])
            w.code(*dst[sym]); w.bits(ev, eb)
        w.code(*lit[256])

    def fixed(self, tokens, final):
        self.w.bits(1 if final else 0, 1); self.w.bits(1, 2)
        self._symbols(tokens, canonical(FIXED_LITLEN), canonical(FIXED_DIST))
        return self

    def header(self, final, n_litlen, n_dist, code_length_sequence, pre_lengths=None, n_pre=None):
        """The header of a dynamic block as told, valid or not: HLIT, HDIST, HCLEN, the code-length code and the sequence."""
        w = self.w
        used = sorted({x if isinstance(x, int) else x[0] for x in code_length_sequence})
        if pre_lengths is None:
            if len(used) == 1:                                     # (a code-length code of one code is incomplete: a partner)
                used = sorted(set(used) | {0 if used[0] else 1})
            pre_lengths = [0] * 19
            for s, l in zip(used, balanced(len(used))):
                pre_lengths[s] = l
        if n_pre is None:
            n_pre = max(4, 1 + max(i for i, s in enumerate(PRE_ORDER) if pre_lengths[s]))
        w.bits(1 if final else 0, 1); w.bits(2, 2)
        w.bits(n_litlen - 257, 5); w.bits(n_dist - 1, 5); w.bits(n_pre - 4, 4)
        for s in PRE_ORDER[:n_pre]:
            w.bits(pre_lengths[s], 3)
        pre = canonical(pre_lengths)
        for x in code_length_sequence:
            if isinstance(x, int):
                w.code(*pre[x])
            else:
                sym, rep = x
                w.code(*pre[sym])
                w.bits(rep - (3 if sym < 18 else 11), {16: 2, 17: 3, 18: 7}[sym])
        return self

    def dynamic(self, tokens, litlen_lengths, dist_lengths, final, code_length_sequence=None):
        """HLIT = len(litlen_lengths), HDIST = len(dist_lengths).  code_length_sequence: the items of the code-length alphabet
        to write -- ints 0 ... 15 and (16 | 17 | 18, repeat) -- which must spell the two length lists back to back."""
        assert 257 <= len(litlen_lengths) <= 286 and 1 <= len(dist_lengths) <= 30 and litlen_lengths[256]
        both = list(litlen_lengths) + list(dist_lengths)
        seq = run_length(both) if code_length_sequence is None else code_length_sequence
        spelt = []
        for x in seq:
            if isinstance(x, int):
                spelt.append(x)
            else:
                assert (3 <= x[1] <= 6 and spelt) if x[0] == 16 else (3 <= x[1] <= 10) if x[0] == 17 else (11 <= x[1] <= 138)
                spelt += [spelt[-1] if x[0] == 16 else 0] * x[1]
        assert spelt == both
        self.header(final, len(litlen_lengths), len(dist_lengths), seq)
        self._symbols(tokens, canonical(litlen_lengths), canonical(dist_lengths))
        return self


def stored(data, final=True):
    return Stream().stored(data, final).done()


def fixed(tokens, final=True):
    return Stream().fixed(tokens, final).done()


def dynamic(tokens, litlen_lengths, dist_lengths, final=True, code_length_sequence=None):
    return Stream().dynamic(tokens, litlen_lengths, dist_lengths, final, code_length_sequence).done()


def random_complete_lengths(rng, n, n_symbols=None, keep=()):
    """Code lengths of a random COMPLETE code of n >= 16 codes with a leaf at depth 15, dealt at random over n_symbols symbols
    (the rest 0); the symbols of ``keep`` get a code."""
    assert n >= 16
    leaves = list(range(1, 16)) + [15]                              # a chain down to depth 15: complete
    while len(leaves) < n:
        k = int(rng.integers(0, len(leaves)))
        if leaves[k] < 15:
            leaves[k] += 1
            leaves.append(leaves[k])
    n_symbols = n if n_symbols is None else n_symbols
    keep = list(dict.fromkeys(keep))
    order = [int(x) for x in rng.permutation(n_symbols)]
    order = list(keep) + [s for s in order if s not in keep]
    perm = [int(x) for x in rng.permutation(n)]
    lengths = [0] * n_symbols
    for s, k in zip(order[:n], perm):
        lengths[s] = leaves[k]
    assert kraft(lengths) == 32768 and max(lengths) == 15
    return lengths


def random_tokens(rng, litlen_lengths, dist_lengths, n_out, matches=None):
    """Tokens of exactly n_out bytes that use only symbols with a code, every one of them about equally often (symbol 284 with
    all its extra bits set included: length 258 the long way).  matches: the share of tokens that are matches, where one fits."""
    lits = [s for s in range(256) if litlen_lengths[s]]
    lens = [s for s in range(257, min(len(litlen_lengths), 286)) if litlen_lengths[s]]
    dsts = [s for s in range(min(len(dist_lengths), 30)) if dist_lengths[s]]
    assert lits
    tokens, n = [], 0
    while n < n_out:
        s = int(rng.integers(0, len(lits) + len(lens))) if dsts and n else 0
        if matches is not None and lens and s:
            s = len(lits) + int(rng.integers(0, len(lens))) if rng.random() < matches else 0
        near = [x for x in dsts if DIST_BASE[x] <= n]
        if s < len(lits) or not near:
            tokens.append(lits[int(rng.integers(0, len(lits)))])
            n += 1
            continue
        k = lens[s - len(lits)] - 257
        length = LEN_BASE[k] + int(rng.integers(0, 1 << LEN_EXTRA[k]))
        if length > n_out - n:
            tokens.append(lits[int(rng.integers(0, len(lits)))])
            n += 1
            continue
        d = near[int(rng.integers(0, len(near)))]
        dist = DIST_BASE[d] + int(rng.integers(0, 1 << DIST_EXTRA[d]))
        if dist > n:
            dist = DIST_BASE[d]
        tokens.append((length, dist, 284) if length == 258 and k == 27 else (length, dist))
        n += length
    return tokens


# ---- members of a feed -------------------------------------------------------------------------------------------------------------
def member(payload, raw):
    """(raw, ISIZE, CRC-32) of a BGZF block whose stream is ``raw`` and whose bytes are ``payload``."""
    return raw, len(payload), zlib.crc32(payload) & 0xFFFFFFFF


def table(members):
    """(comp, tab): the members' streams back to back and the (n, 4) array of in_off, in_len, ISIZE, CRC that BamCodec.feed takes."""
    tab = np.zeros((len(members), 4), np.uint64)
    at = 0
    for k, (raw, isize, crc) in enumerate(members):
        tab[k] = (at, len(raw), isize, crc)
        at += len(raw)
    return b"".join(m[0] for m in members), tab


# ---- the valid cases ---------------------------------------------------------------------------------------------------------------
def _payloads():
    rng = np.random.default_rng(5)
    acgt = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000)) + bytes(rng.choice([37, 37, 37, 25, 11, 2], 2000).astype(np.uint8))
    return (("acgt", acgt), ("random", rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()), ("zeros", bytes(5000)))


def _valid_cases():
    rng = np.random.default_rng(1951)
    cases = []

    def add(name, raw, want):
        assert len(want) <= 65536 and len(raw) <= (65535 if name != "stored_65535" else 65540), name
        cases.append((name, raw, bytes(want)))

    # stored blocks
    add("stored_empty_final", stored(b"", True), b"")
    add("stored_empty_run", Stream().stored(b"", False).stored(b"", False).stored(b"", False).stored(b"", True).done(), b"")
    add("stored_empty_between", Stream().stored(b"", False).stored(b"ab", False).stored(b"", False).stored(b"c", True).done(), b"abc")
    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    add("stored_65535", stored(big, True), big)                     # (the one stream longer than a BGZF block can hold: 5 + 65,535)
    mids = (0, 1, 3, 6, 7, 8, 9, 20, 5, 2, 4, 300)
    for k in range(12):                                             # the fixed block ends at bit (2 + k % 8) % 8 of a byte
        lits = [int(x) for x in rng.integers(144, 256, k % 8)] + [int(x) for x in rng.integers(0, 144, k - k % 8)]
        mid = rng.integers(0, 256, mids[k], dtype=np.uint8).tobytes()
        back = [7]
        have = k + len(mid) + 1
        if len(mid):
            back.append((3 + k, min(len(mid) + 1, have)))           # reaches back over the stored bytes
            back.append((258, 1, 284))
        raw = Stream().fixed(lits, False).stored(mid, False).fixed(back, False).stored(b"", True).done()
        add("fixed_%d_stored_%d_fixed_stored" % (k, len(mid)), raw, play(lits + list(mid) + back))
    # one fixed block with every length symbol and every distance symbol, smallest and largest extra bits
    pre = [int(x) for x in rng.integers(0, 256, 32768)]
    toks = list(pre)
    for k in range(30):
        for top in (0, 1):
            lk = min(k, 28)
            length = LEN_BASE[lk] + (((1 << LEN_EXTRA[lk]) - 1) if top else 0)
            dist = DIST_BASE[k] + (((1 << DIST_EXTRA[k]) - 1) if top else 0)
            toks.append((length, dist, 284) if length == 258 and k == 27 else (length, dist))
    want = play(toks)
    assert len(want) < 65536 and any(t == (258, 32768) for t in toks if not isinstance(t, int))
    add("fixed_every_symbol", fixed(toks, True), want)
    # short distances, matches that end at or near the end of the output
    for dist in (1, 2, 3, 7, 8, 9, 15, 16):
        for length in (258, 3, 11):
            for tail in (0, 1, 7, 8, 9):
                toks = [int(x) for x in rng.integers(0, 256, 16)]
                toks.append((258, dist, 284) if length == 258 and tail in (1, 8) else (length, dist))
                toks += [int(x) for x in rng.integers(0, 256, tail)]
                add("fixed_d%d_l%d_t%d" % (dist, length, tail), fixed(toks, True), play(toks))
    # dynamic blocks: random complete codes with 15-bit leaves in both alphabets
    for k in range(64):
        n_out = 65536 if k in (8, 39) else (1, 100, 5000, 100, 700, 5000)[k % 6]
        hlit = (257, 258, 270, 285, 286)[k % 5]
        hdist = (29, 30, 16, 30, 22, 30, 19)[k % 7]
        lit = random_complete_lengths(rng, int(rng.integers(16, hlit + 1)), hlit, keep=(256, int(rng.integers(0, 256))))
        dst = random_complete_lengths(rng, int(rng.integers(16, hdist + 1)), hdist)
        toks = random_tokens(rng, lit, dst, n_out, 0.7 if n_out == 65536 else None)   # (15-bit literals alone would not fit a block)
        add("dynamic_random_%d_hlit%d_hdist%d_%d" % (k, hlit, hdist, n_out), dynamic(toks, lit, dst, True), play(toks))
    # HLIT x HDIST at their edges (short distance alphabets cannot hold a 15-bit leaf)
    small_dst = {1: [1], 2: [1, 1], 5: [1, 2, 3, 4, 4]}
    for hlit in (257, 258, 270, 285, 286):
        for hdist in (1, 2, 5, 29, 30):
            lit = random_complete_lengths(rng, min(hlit, 200), hlit, keep=(256, 65, hlit - 1))
            dst = small_dst[hdist] if hdist in small_dst else random_complete_lengths(rng, hdist, hdist)
            toks = random_tokens(rng, lit, dst, 100)
            add("dynamic_hlit%d_hdist%d" % (hlit, hdist), dynamic(toks, lit, dst, True), play(toks))
    # a one-code distance alphabet (distance 1 only), and HDIST = 1 with length 0: literals only
    lit = random_complete_lengths(rng, 120, 286, keep=(256, 0, 285, 284, 257))
    toks = [0, (258, 1), (258, 1, 284), (3, 1)] + random_tokens(rng, lit, [1], 3000)
    add("dynamic_one_distance_code", dynamic(toks, lit, [1], True), play(toks))
    lit = random_complete_lengths(rng, 150, 257, keep=(256,))
    toks = random_tokens(rng, lit, [0], 1000)
    add("dynamic_no_distance_code", dynamic(toks, lit, [0], True), play(toks))
    # the code-length alphabet: HCLEN field 4 (eight code-length codes: lengths 6 ... 9 and 0), the fewest codes a valid block can
    # have (five: 16 17 18 0 8), symbol 18 with 138 zeros, symbol 16 repeating across the boundary between the two alphabets
    lit = [6] * 10 + [7] * 20 + [8] * 100 + [9] * 152
    assert kraft(lit) == 32768
    toks = [int(x) for x in rng.integers(0, 256, 400)]
    raw = dynamic(toks, lit, [0], True, code_length_sequence=lit + [0])
    assert (raw[1] >> 5 | (raw[2] & 1) << 3) == 4
    add("dynamic_hclen_field_4", raw, play(toks))
    lit = [8] * 255 + [0, 8]
    toks = [int(x) for x in rng.integers(0, 255, 300)]
    raw = dynamic(toks, lit, [0], True, code_length_sequence=lit + [0])
    assert (raw[1] >> 5 | (raw[2] & 1) << 3) == 1
    add("dynamic_hclen_fewest", raw, play(toks))
    lit = [2, 2] + [0] * 138 + [3] + [0] * 115 + [3, 3, 3]           # symbols 0 1 | 140 | 256 257 258: complete
    assert kraft(lit) == 32768
    toks = [0, 1, 140, 140, 1, (3, 2), (4, 1), 0]
    add("dynamic_18_with_138_zeros", dynamic(toks, lit, [1, 1], True, code_length_sequence=[2, 2, (18, 138), 3, (18, 115), 3, 3, 3, 1, 1]),
        play(toks))
    lit = [1] + [0] * 255 + [5] * 16                                # the run of 5s goes on through the first 16 distance lengths
    dst = [5] * 16 + [4] * 8
    assert len(lit) == 272 and kraft(lit) == 32768 and kraft(dst) == 32768
    seq = [1, (18, 138), (18, 117), 5, (16, 6), (16, 6), (16, 6), (16, 6), (16, 4), (16, 3), 4, (16, 6), 4]
    toks = [0, 0, 0, 0, (3, 1), (10, 4), 0, (4, 9), (30, 3)]
    add("dynamic_16_across_the_alphabets", dynamic(toks, lit, dst, True, code_length_sequence=seq), play(toks))
    # two dynamic blocks and a fixed one in one stream: matches reach back over the block boundaries
    la = random_complete_lengths(rng, 100, 286, keep=(256,)); da = random_complete_lengths(rng, 20, 30)
    lb = random_complete_lengths(rng, 286, 286); db = random_complete_lengths(rng, 30, 30)
    ta = random_tokens(rng, la, da, 3000)
    tb = [(100, 2900)] + random_tokens(rng, lb, db, 2000)
    tc = [(258, 4000), 65, (3, 1), 66] + [int(x) for x in rng.integers(0, 256, 50)]
    raw = Stream().dynamic(ta, la, da, False).dynamic(tb, lb, db, False).fixed(tc, True).done()
    add("dynamic_dynamic_fixed", raw, play(ta + tb + tc))
    raw = Stream().fixed(tc[1:], False).dynamic(ta, la, da, False).fixed(tc[1:], False).stored(b"xyz", False).fixed([(5, 3)], True).done()
    add("fixed_dynamic_fixed_stored_fixed", raw, play(tc[1:] + ta + tc[1:] + list(b"xyz") + [(5, 3)]))
    # zlib: every level and strategy, a full flush in the middle
    for pname, data in _payloads():
        for level in range(10):
            for sname, strategy in (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY),
                                    ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
                half = len(data) // 2
                raw = co.compress(data[:half]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[half:]) + co.flush()
                add("zlib_%s_l%d_%s" % (pname, level, sname), raw, data)
    return cases


# ---- the refused cases -------------------------------------------------------------------------------------------------------------
def _refused_cases():
    """[(name, raw, ISIZE)]: zlib raises on each, or gives a length other than ISIZE -- and {name: the ISIZE bytes a decoder that
    skipped the failing check would leave}, where those are known: with their CRC-32 in the table only the decoder can refuse."""
    rng = np.random.default_rng(286)
    cases, lenient = [], {}
    data = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
    good = stored(data, True)
    cases.append(("stored_nlen_mismatch", good[:3] + bytes([good[3] ^ 1]) + good[4:], 100))
    lenient["stored_nlen_mismatch"] = data
    cases.append(("stored_len_beyond_input", good[:55], 100))
    cases.append(("stored_len_beyond_output", good, 60))
    lenient["stored_len_beyond_output"] = data[:60]
    lit = random_complete_lengths(rng, 200, 286, keep=(256,)); dst = random_complete_lengths(rng, 30, 30)
    toks = random_tokens(rng, lit, dst, 2000)
    dyn = dynamic(toks, lit, dst, True)
    cases.append(("output_one_byte_short", dyn, 1999))
    lenient["output_one_byte_short"] = play(toks)[:1999]
    cases.append(("output_one_byte_long", dyn, 2001))
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 29)
    cases.append(("block_type_3", w.done(), 10))
    cases.append(("distance_before_the_start", fixed([1, 2, 3, (3, 4)], True), 6))
    cases.append(("no_final_block", Stream().fixed([1, 2, 3], False).stored(b"abc", False).done(), 6))
    lenient["no_final_block"] = b"\x01\x02\x03abc"
    for name, put in (("fixed_length_symbol_286", lambda w: (w.code(0b11000110, 8), w.code(0, 5))),
                      ("fixed_distance_symbol_30", lambda w: (w.code(0b0000001, 7), w.code(30, 5)))):
        s = Stream()
        s.w.bits(1, 1); s.w.bits(1, 2)
        for c in (65, 66, 67, 68):
            s.w.code(0x30 + c, 8)
        put(s.w)
        s.w.code(0x30 + 69, 8); s.w.code(0, 7)
        cases.append((name, s.done(), 8))
    over = [8] * 257
    over[0] = 7; over[1] = 7                                            # 257 codes of 8 bits and two of 7: 2 / 256 too many
    over += [8]
    s = Stream().header(True, 258, 1, over + [0])
    for _ in range(12):
        s.w.bits(0, 8)
    cases.append(("oversubscribed_literal_code", s.done(), 12))
    no_eob = [8] * 256 + [0]
    s = Stream().header(True, 257, 1, no_eob + [0])
    for _ in range(12):
        s.w.bits(0, 8)
    cases.append(("no_end_of_block_code", s.done(), 12))
    s = Stream().header(True, 257, 1, [(16, 3)] + [8] * 253 + [8, 0])
    for _ in range(12):
        s.w.bits(0, 8)
    cases.append(("code_16_first", s.done(), 12))
    s = Stream().header(True, 257, 1, [8] * 255 + [0, 8, (17, 3)])
    for _ in range(12):
        s.w.bits(0, 8)
    cases.append(("repeat_past_hlit_hdist", s.done(), 12))
    cases.append(("stream_cut_in_half", dyn[:len(dyn) // 2], 2000))
    assert all(len(lenient[name]) == isize for name, _, isize in cases if name in lenient)
    return cases, lenient


VALID_CASES = _valid_cases()
REFUSED_CASES, LENIENT_BYTES = _refused_cases()


def replacement(isize, seed=0):
    """A valid member of ISIZE bytes: what stands in for a refused one when the host patches it."""
    data = np.random.default_rng(1000 + seed).integers(0, 256, isize, dtype=np.uint8).tobytes()
    return member(data, stored(data, True))


def valid_members():
    return [member(want, raw) for _, raw, want in VALID_CASES]


def feed_members(codec, members):
    """One feed of ``members`` to a BamCodec with no record index -- the first record starts behind the image: (info, image bytes)."""
    comp, tab = table(members)
    info = codec.feed(comp, tab, sum(m[1] for m in members), 1)
    return info, codec.image()[0].tobytes()


def refused_member(k):
    """REFUSED_CASES[k] as a member.  Its CRC is that of LENIENT_BYTES where there are any, so that a decoder which wrongly accepts
    the stream is not covered by the CRC check behind it; else 0."""
    name, raw, isize = REFUSED_CASES[k]
    return raw, isize, (zlib.crc32(LENIENT_BYTES[name]) & 0xFFFFFFFF) if name in LENIENT_BYTES else 0


def mixed_feed():
    """(members, indices of the refused ones, the same members with a valid one of the same ISIZE in place of each refused one):
    REFUSED_CASES between valid members of every kind."""
    valid = valid_members()
    step = len(valid) // len(REFUSED_CASES)
    members, bad, mended = [], [], []
    for k in range(len(REFUSED_CASES)):
        for m in valid[k * step:(k + 1) * step][:3]:
            members.append(m); mended.append(m)
        bad.append(len(members))
        members.append(refused_member(k))
        mended.append(replacement(REFUSED_CASES[k][2], k))
    members.append(valid[-1]); mended.append(valid[-1])
    return members, bad, mended


def spans(members):
    """[(start, end)] of every member's bytes in the image of one feed."""
    at, out = 0, []
    for _, isize, _ in members:
        out.append((at, at + isize))
        at += isize
    return out


def dump(path):
    """Every case into one file for tests/hostsim/bgzf_cases.cpp: per case a line ``name valid|refused n_raw n_out crc`` and the
    raw bytes, then the expected bytes of a valid one."""
    with open(path, "wb") as f:
        for name, raw, want in VALID_CASES:
            f.write(b"%s valid %d %d %d\n" % (name.encode(), len(raw), len(want), zlib.crc32(want) & 0xFFFFFFFF))
            f.write(raw); f.write(want)
        for name, raw, isize in REFUSED_CASES:
            f.write(b"%s refused %d %d 0\n" % (name.encode(), len(raw), isize))
            f.write(raw)
