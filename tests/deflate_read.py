"""A token reader for raw DEFLATE (RFC 1951): a plain Python inflate of ONE final block that keeps everything the block says --
for a stored block its length, for a dynamic block HLIT, HDIST, HCLEN, the 19 code-length-code lengths, the code-length symbols as
they were sent (with their repeat counts), the two lists of code lengths, the tokens and the bytes they stand for.  No speed, no
library: tests/test_deflate_enc_craft.py keeps it honest against zlib (never against the encoder it is used on) and then reads the
encoder's streams with it.
"""
from tests.deflate_craft import DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LITLEN, LEN_BASE, LEN_EXTRA, PRE_ORDER, canonical


class NotOneFinalBlock(ValueError):
    """The stream does not start with a final block, or goes on behind it."""


class Block:
    """kind: 'stored' | 'fixed' | 'dynamic'.  stored: ``length``.  dynamic: ``hlit``, ``hdist``, ``hclen`` (the counts, not the
    fields), ``pre_lengths`` (19, by symbol), ``sent`` (ints 0 ... 15 and (16 | 17 | 18, repeat)), ``litlen`` (hlit lengths),
    ``dist`` (hdist lengths).  fixed and dynamic: ``tokens`` (int for a literal, (length, distance) for a match), ``symbols``
    (the literal/length symbol of every token: 258 may come as 285 or as 284 with 31 in its extra bits), ``header_bits`` and
    ``n_bits``.  All: ``data``, the bytes replayed, and ``n_bytes``, the stream's length."""

    def __init__(self, kind):
        self.kind = kind
        self.tokens, self.symbols, self.data = [], [], b""


class _Bits:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            if self.at >> 3 >= len(self.raw):
                raise ValueError("the stream ends inside the block")
            v |= ((self.raw[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v

    def symbol(self, table):
        """One Huffman symbol: ``table`` is {(code, length): symbol}; codes come most significant bit first."""
        code = 0
        for length in range(1, 16):
            code = (code << 1) | self.bits(1)
            s = table.get((code, length))
            if s is not None:
                return s
        raise ValueError("a code that no symbol has")


def _decoder(lengths):
    return {cl: s for s, cl in canonical(list(lengths)).items()}


def read_block(raw):
    """The one final block that ``raw`` is.  Raises NotOneFinalBlock when it is not one, ValueError on anything invalid."""
    r = _Bits(raw)
    if r.bits(1) != 1:
        raise NotOneFinalBlock("BFINAL is 0")
    btype = r.bits(2)
    if btype == 3:
        raise ValueError("block type 3")
    if btype == 0:
        b = Block("stored")
        r.at = (r.at + 7) & ~7
        n, nn = r.bits(16), r.bits(16)
        if n ^ nn != 0xFFFF:
            raise ValueError("LEN and NLEN disagree")
        at = r.at >> 3
        if at + n > len(raw):
            raise ValueError("the stored bytes end behind the stream")
        if at + n != len(raw):
            raise NotOneFinalBlock("bytes behind the block")
        b.length, b.data, b.n_bytes = n, bytes(raw[at:at + n]), len(raw)
        return b
    b = Block("fixed" if btype == 1 else "dynamic")
    if btype == 1:
        litlen, dist = FIXED_LITLEN, FIXED_DIST
    else:
        b.hlit, b.hdist, b.hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
        b.pre_lengths = [0] * 19
        for s in PRE_ORDER[:b.hclen]:
            b.pre_lengths[s] = r.bits(3)
        pre = _decoder(b.pre_lengths)
        both, b.sent = [], []
        while len(both) < b.hlit + b.hdist:
            s = r.symbol(pre)
            if s < 16:
                both.append(s); b.sent.append(s)
                continue
            if s == 16 and not both:
                raise ValueError("symbol 16 first")
            rep = r.bits({16: 2, 17: 3, 18: 7}[s]) + (11 if s == 18 else 3)
            both += [both[-1] if s == 16 else 0] * rep
            b.sent.append((s, rep))
        if len(both) != b.hlit + b.hdist:
            raise ValueError("a repeat runs past HLIT + HDIST")
        litlen, dist = both[:b.hlit], both[b.hlit:]
        b.litlen, b.dist = litlen, dist
        if not litlen[256]:
            raise ValueError("no end-of-block code")
    b.header_bits = r.at
    lit, dst = _decoder(litlen), _decoder(dist)
    out = bytearray()
    while True:
        s = r.symbol(lit)
        if s == 256:
            break
        if s < 256:
            b.tokens.append(s); b.symbols.append(s); out.append(s)
            continue
        if s > 285:
            raise ValueError("length symbol %d" % s)
        length = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
        d = r.symbol(dst)
        if d > 29:
            raise ValueError("distance symbol %d" % d)
        distance = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
        if distance > len(out):
            raise ValueError("a distance before the start")
        b.tokens.append((length, distance)); b.symbols.append(s)
        for _ in range(length):
            out.append(out[-distance])
    b.n_bits = r.at
    if (r.at + 7) >> 3 != len(raw):
        raise NotOneFinalBlock("bytes behind the block")
    b.data, b.n_bytes = bytes(out), len(raw)
    return b
