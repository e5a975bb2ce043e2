"""The crafted chunks of tests/deflate_enc_craft.py through the DEFLATE encoder's phases on the host (amp_deflate.hip with
-DAMPDF_HOSTSIM), every stream read token by token (tests/deflate_read.py): which matches the encoder finds and which it must not,
which lengths it sends, what its Huffman codes and its header look like, what it does with the room it is given; build_lengths at
the limits no chunk reaches; and the same phases as a program of their own under AddressSanitizer / UBSan.  Every expectation comes
from the encoder's restated constants or from zlib and RFC 1951.  What passes here is what tests/test_gpu_deflate_edges.py asks of
the device, byte for byte.  No GPU needed."""
import heapq
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests import deflate_enc_craft as ec
from tests.deflate_read import NotOneFinalBlock, read_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    return ec.hostsim_library()


@pytest.fixture(scope="module")
def blocks(sim):
    """{name: (stream, what the reader says of it)} of every chunk with its own room, the source dword-aligned."""
    out = {}
    for c in ec.CHUNKS:
        s, = ec.encode(sim.ampdf_hostsim_blocks, c.data, room=c.room)
        assert s is not None, c.name
        out[c.name] = (s, read_block(s))
    return out


def matches(b):
    return [t for t in b.tokens if not isinstance(t, int)]


def round_trips(stream, data):
    d = zlib.decompressobj(-15)
    return d.decompress(stream) == data and d.eof and d.unused_data == b""


# ---- the reader and the constants ------------------------------------------------------------------------------------------------------------
def respell(b):
    """The stream that the reader's fields spell, written with tests/deflate_craft's bit writer."""
    s = dc.Stream()
    s.header(True, b.hlit, b.hdist, b.sent, pre_lengths=b.pre_lengths, n_pre=b.hclen)
    tokens = [(t[0], t[1], 284) if not isinstance(t, int) and sym == 284 and t[0] == 258 else t for t, sym in zip(b.tokens, b.symbols)]
    s._symbols(tokens, dc.canonical(b.litlen), dc.canonical(b.dist))
    return s.done()


def test_reader_agrees_with_zlib():
    """Against zlib, never against the encoder: the replayed bytes are zlib's, and the fields the reader returns spell the very
    stream it read."""
    seen = {"stored": 0, "dynamic": 0, "fixed": 0}
    streams = [(name, raw, want) for name, raw, want in dc.VALID_CASES]
    rng = np.random.default_rng(7)
    payloads = [ec.acgt_with_repeats(rng, 5000), bytes(rng.integers(0, 256, 40, dtype=np.uint8)) * 60, b"a" * 3000 + bytes(range(256)) * 4,
                bytes(rng.geometric(0.05, 6000).clip(0, 255).astype(np.uint8)),
                b"a" * 3000 + bytes(rng.geometric(0.1, 3000).clip(0, 255).astype(np.uint8)),
                b"".join(b"read%07d\tACGTACGTTTGACCA\tIIIIIIIIIIIIIII\n" % (i * 7919 % 100000) for i in range(150))]
    own = set()
    for k, data in enumerate(payloads):
        for level in (1, 6, 9):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            streams.append(("zlib_%d_l%d" % (k, level), co.compress(data) + co.flush(), data))
            own.add(streams[-1][0])
    zlib_dynamic = 0
    for name, raw, want in streams:
        try:
            b = read_block(raw)
        except NotOneFinalBlock:
            continue
        assert b.data == want == zlib.decompress(raw, -15), name
        assert b.n_bytes == len(raw)
        if b.kind == "stored":
            assert b.length == len(want) and raw[0] & 7 == 1, name
        elif b.kind == "dynamic":
            assert dc.play(b.tokens) == want, name
            assert len(b.pre_lengths) == 19 and len(b.litlen) == b.hlit and len(b.dist) == b.hdist, name
            spelt = []
            for x in b.sent:
                spelt += [x] if isinstance(x, int) else [spelt[-1] if x[0] == 16 else 0] * x[1]
            assert spelt == b.litlen + b.dist, name
            assert respell(b) == raw, name
            zlib_dynamic += name in own
        else:
            assert dc.play(b.tokens) == want, name
        seen[b.kind] += 1
    assert seen["stored"] >= 2 and seen["dynamic"] >= 90 and seen["fixed"] >= 6, seen       # (the crafted 15-bit codes are among them)
    assert zlib_dynamic == 12 and len(own) == 18, "zlib's levels 1, 6 and 9 gave fewer than twelve single dynamic blocks"
    for raw in (b"", b"\x07", dc.fixed([1, 2, 3], True)[:1]):
        with pytest.raises(ValueError):
            read_block(raw)
    for name, raw, _ in dc.REFUSED_CASES:
        if name not in ("output_one_byte_short", "output_one_byte_long", "stored_len_beyond_output"):     # (about ISIZE, not the stream)
            with pytest.raises(ValueError):
                read_block(raw)


def test_constants_are_the_sources():
    text = open(ec.SOURCE).read()
    for name, value in ec.SOURCE_CONSTANTS.items():
        m = re.search(r"^constexpr int(?:64_t)? (?:\w+ = \w+, )*%s = (0x[0-9A-Fa-f]+|\d+)\b" % name, text, re.M)
        assert m, "%s is not a constant of amp_deflate.hip any more" % name
        assert int(m.group(1), 0) == value, "%s is %s in amp_deflate.hip, %d here" % (name, m.group(1), value)
    assert "w - (KWIN - 1) + j" in text and "b1 + SEG - 1 < n ? b1 + SEG - 1 : n" in text      # the window and a lane's limit
    assert ec.UNSEEN_FROM == 4091 and ec.WINDOW == 3968 and ec.LANE_BYTES == 247 <= ec.TOK_MAX


# ---- every chunk ---------------------------------------------------------------------------------------------------------------------------------
def huffman_depth(counts):
    """Depth of a plain Huffman tree over the counts."""
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def check_header(name, b):
    """Family D's rules, for a dynamic block of any family."""
    assert ec.kraft(b.litlen, 15) == 1 << 15 and ec.kraft(b.dist, 15) == 1 << 15, "%s: a code is not complete" % name
    assert ec.kraft(b.pre_lengths, 7) == 1 << 7, "%s: the code-length code is not complete" % name
    assert max(b.litlen) <= 15 and max(b.dist) <= 15 and max(b.pre_lengths) <= 7, name
    assert b.sent == ec.run_length_rule(b.litlen + b.dist), "%s: the code lengths are not sent as RFC 1951 3.2.7, greedy" % name
    coded = [i for i, s in enumerate(dc.PRE_ORDER) if b.pre_lengths[s]]
    assert b.hclen == max(4, coded[-1] + 1), "%s: HCLEN %d" % (name, b.hclen)
    assert {x if isinstance(x, int) else x[0] for x in b.sent} <= {s for s in range(19) if b.pre_lengths[s]}
    assert (b.hlit == 257 or b.litlen[-1]) and (b.hdist == 1 or b.dist[-1]) and b.hlit <= 285, "%s: HLIT %d, HDIST %d" % (name, b.hlit, b.hdist)


def test_every_stream_and_every_header(blocks):
    """Families A to E: the stream is valid and no longer than a stored block, no distance reaches KWIN * SEG, no token is longer
    than 2 * SEG - 2, symbol 285 never occurs, and every dynamic block keeps the header rules of family D."""
    n_dynamic = 0
    deepest = {"literal/length": (0, ""), "distance": (0, ""), "code-length": (0, "")}
    for c in ec.CHUNKS:
        s, b = blocks[c.name]
        n = len(c.data)
        assert round_trips(s, c.data) and b.data == c.data, c.name
        assert len(s) <= n + 5, c.name
        assert (s[0] & 7 == 1) == (b.kind == "stored") and (b.kind != "stored" or len(s) == n + 5), c.name
        assert b.kind in ("stored", "dynamic") and (b.kind == "dynamic" or s[0] & 7 == 1), c.name
        if "stored" in c.expect:
            assert (b.kind == "stored") == c.expect["stored"], "%s: %s block (%s)" % (c.name, b.kind, c.expect.get("why", ""))
        if b.kind != "dynamic":
            continue
        n_dynamic += 1
        check_header(c.name, b)
        longest = ec.LANE_BYTES if c.family == "X" else ec.LONGEST_TOKEN
        for length, dist in matches(b):
            assert ec.MIN_MATCH <= length <= longest, "%s: a token of %d bytes" % (c.name, length)
            assert 1 <= dist < ec.WINDOW, "%s: distance %d" % (c.name, dist)
        assert 285 not in b.symbols and b.hlit <= 285, c.name
        # how deep a plain Huffman tree of the counts this block sent would be: deeper than 15 / 15 / 7 and a limit had to act
        lit, dst, pre = [0] * 286, [0] * 30, [0] * 19
        for sym in b.symbols + [256]:
            lit[sym] += 1
        for _, dist in matches(b):
            dst[ec.distance_symbol_of(dist)] += 1
        for x in b.sent:
            pre[x if isinstance(x, int) else x[0]] += 1
        for key, counts in (("literal/length", lit), ("distance", dst), ("code-length", pre)):
            if sum(1 for x in counts if x) > 1:
                deepest[key] = max(deepest[key], (huffman_depth(counts), c.name))
    print("deepest plain Huffman trees of the families' own counts:", deepest)
    assert n_dynamic >= len(ec.CHUNKS) - 15


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_sizes_and_alignment(sim, blocks):
    assert {len(c.data) for c in ec.FAMILY_A} == set(ec.A_SIZES) >= {1, 5, 123, 125, 247, 249, 371, 373, 65223, 65225, 0xFEFF, 0xFF00}
    n_dynamic = 0
    for c in ec.FAMILY_A:
        s0, b0 = blocks[c.name]
        n_dynamic += b0.kind == "dynamic"
        for skew in ec.SKEWS[1:]:
            s, = ec.encode(sim.ampdf_hostsim_blocks, c.data, skew=skew)
            assert round_trips(s, c.data), (c.name, skew)
            assert read_block(s).tokens == b0.tokens and s == s0, "%s: the stream depends on the source's misalignment (%d)" % (c.name, skew)
    assert n_dynamic >= len(ec.FAMILY_A) - 5                          # (1 to 5 bytes are stored blocks)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------------
def test_b_the_match_window(blocks):
    near = [c for c in ec.FAMILY_B if "cover" in c.expect]
    assert {c.expect["dist"] for c in near} >= set(ec.B_NEAR) | set(ec.B_PICKED) | set(ec.B_SMALL)
    assert len([d for d in ec.B_PICKED if d < 3700]) >= 6 and set(ec.B_NEAR) == set(range(3700, 3918, 7)) and min(ec.B_FAR) == 4091
    seen, low = set(), []
    for c in near:
        _, b = blocks[c.name]
        lo, hi, floor = c.expect["cover"]
        got = ec.covered(b.tokens, c.expect["dist"], lo, hi)
        low.append((got, c.name))
        assert got >= floor, "%s: tokens of distance %d cover %d of the %d bytes of the copy, the floor is %d (%s)" % (
            c.name, c.expect["dist"], got, hi - lo, floor, c.expect["why"])
        seen |= {ec.distance_symbol_of(t[1]) for t in matches(b)}
    print("family B: least cover", sorted(low)[:3])
    assert seen >= set(range(24)), "distance symbols never sent: %s" % sorted(set(range(24)) - seen)
    for c in ec.FAMILY_B:
        if "no_dist" in c.expect:
            s, b = blocks[c.name]
            assert b.kind == "stored" and not any(t[1] == c.expect["no_dist"] for t in matches(b)), c.name


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------------
def test_c_match_lengths(blocks):
    want = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 18, 19, 34, 35, 66, 67, 130, 131, 226, 227, 246}
    assert {c.expect["length"] for c in ec.FAMILY_C if "length" in c.expect} == want
    for c in ec.FAMILY_C + ec.FAMILY_X:
        _, b = blocks[c.name]
        if "length" in c.expect:
            assert (c.expect["length"], c.expect["dist"]) in matches(b), "%s: no token (%d, %d): %r" % (
                c.name, c.expect["length"], c.expect["dist"], matches(b)[:8])
        else:                                                           # a run: a literal, then distance 1 only
            assert b.tokens[0] == ord("a") and all(t[1] == 1 for t in matches(b)) and len(matches(b)) == len(b.tokens) - 1, c.name
            assert max(t[0] for t in matches(b)) <= ec.LONGEST_TOKEN
    assert {len(c.data) for c in ec.FAMILY_C if "length" not in c.expect} == {257, 258, 259, 260, 261, 262, 263, 516, 517, 518, 65279, 65280}
    # every length symbol but 285 is sent somewhere in the families
    sent = {s for name, (_, b) in blocks.items() if b.kind == "dynamic" for s in b.symbols if s > 256}
    assert sent >= {ec.length_symbol_of(L) for L in want} and 285 not in sent


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------------
def test_d_codes_and_header(blocks):
    zero_runs, code_runs = set(), set()
    for c in ec.FAMILY_D:
        _, b = blocks[c.name]
        e = c.expect
        m = matches(b)
        if e.get("no_match"):
            assert not m, "%s: %r" % (c.name, m[:5])
        if "only_dsym" in e:
            assert m and {ec.distance_symbol_of(t[1]) for t in m} == {e["only_dsym"]}, c.name
        if "dist" in e:
            assert any(t[1] == e["dist"] for t in m), c.name
        if "hdist" in e:
            assert b.hdist == e["hdist"] and b.dist == e["dist_lengths"], "%s: HDIST %d, lengths %r" % (c.name, b.hdist, b.dist)
        if e.get("all_literals"):
            assert all(b.litlen[v] for v in range(256)) and b.hlit >= 257, c.name
        runs = ec.runs_of(b.litlen)
        for r in e.get("zero_runs", ()):
            assert (0, r) in runs, "%s: no run of %d zeros in %r" % (c.name, r, runs)
            zero_runs.add(r)
        for r in e.get("code_runs", ()):
            assert any(v and k == r for v, k in runs), "%s: no run of %d equal lengths in %r" % (c.name, r, runs)
            code_runs.add(r)
    assert zero_runs == set(ec.D_ZERO_RUNS) and code_runs == set(ec.D_CODE_RUNS)
    one = blocks["D_one_value"][1]
    assert sum(1 for x in one.litlen[:256] if x) == 1
    assert len({t for t in blocks["D_two_values"][1].tokens}) == 2


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------------
def room_items(blocks):
    """[(name, chunk, room, what must come back)] of family E."""
    return [("%s_room%d" % (c.name, room), c, room, want) for c in ec.FAMILY_E for room, want in ec.room_cases(c, blocks[c.name][0])]


def test_e_room(sim, blocks):
    kinds = set()
    for name, c, room, want in room_items(blocks):
        s, = ec.encode(sim.ampdf_hostsim_blocks, c.data, room=room)           # (checks the bytes behind the room)
        full = blocks[c.name][0]
        if want == "same":
            assert s == full, name
        elif want == "stored":
            assert s is not None and s[0] == 1 and len(s) == len(c.data) + 5 <= room and round_trips(s, c.data), name
        else:
            assert s is None, name
        kinds.add((c.expect["stored"], want))
    # (a Huffman stream is shorter than its stored block, so one byte less than it needs never leaves room for that either)
    assert kinds == {(False, "same"), (False, None), (True, "stored"), (True, None)}


def test_a_chunk_does_not_depend_on_the_chunk_before(sim, blocks):
    """The host phases keep one LDS image from chunk to chunk, as a workgroup does: a long Huffman stream, one byte value and a
    stored block in a row give the streams each gives behind a chunk of another kind."""
    rng = np.random.default_rng(59)
    data = ec.unlike_chunks(rng, 12, 12)
    row = ec.encode(sim.ampdf_hostsim_blocks, data, block_bytes=300, room=320)
    assert [s[0] & 7 for s in row] == [5, 5, 1] * 4 and min(len(s) for s in row) < 30
    for k, s in enumerate(row):
        chunk = data[300 * k:300 * (k + 1)]
        for before in ("D_all_values", "C_run65280", "B_far_d5000"):
            ec.encode(sim.ampdf_hostsim_blocks, next(c for c in ec.CHUNKS if c.name == before).data)
            alone, = ec.encode(sim.ampdf_hostsim_blocks, chunk, room=320)
            assert alone == s and round_trips(s, chunk), "chunk %d behind %s" % (k, before)
    rng = np.random.default_rng(41)
    data = ec.bam_like(rng, 1300 * 64 - 17)
    kinds = [s[0] & 7 for s in ec.encode(sim.ampdf_hostsim_blocks, data, block_bytes=64, room=69)]
    print("64-byte chunks of BAM-like bytes: %d dynamic, %d stored" % (kinds.count(5), kinds.count(1)))
    assert kinds.count(5) > 1300 // 4 and kinds.count(1) > 1300 // 8


# ---- F ---------------------------------------------------------------------------------------------------------------------------------------------
def test_f_build_lengths_at_its_limits(sim, capsys):
    """ampdf_hostsim_lengths on frequencies no chunk gives: complete, no deeper than the limit, never longer for the more frequent
    symbol, and never cheaper than an optimal length-limited code (package-merge).  How far above the optimum it lands is printed,
    not gated (DESIGN.md section 9 has the figures)."""
    assert ec.optimal_limited_cost([1, 1, 2, 3, 5, 8, 13], 15) == sum(f * l for f, l in zip([1, 1, 2, 3, 5, 8, 13], [6, 6, 5, 4, 3, 2, 1]))
    assert ec.optimal_limited_cost([1, 1, 2, 3, 5, 8, 13], 3) == 3 * 20 + 2 * 13      # depth 3: the heaviest symbol gets two bits
    assert ec.optimal_limited_cost([5, 5, 5, 5], 2) == 40
    inputs = ec.lengths_inputs()
    assert sum(1 for x in inputs if x[0].startswith("random_")) == 600
    limited = {7: 0, 15: 0}
    excess = {}
    for name, freq, bits in inputs:
        lens = ec.host_lengths(freq, bits)
        used = [(f, l) for f, l in zip(freq, lens) if f]
        assert all(l == 0 for f, l in zip(freq, lens) if not f), name
        assert ec.kraft(lens, bits) == 1 << bits, "%s: not complete: %r" % (name, lens)
        assert 1 <= min(l for _, l in used) and max(l for _, l in used) <= bits, "%s: deeper than %d" % (name, bits)
        by_f = sorted(used)
        for (f0, l0), (f1, l1) in zip(by_f, by_f[1:]):
            assert f0 == f1 or l0 >= l1, "%s: count %d has %d bits, count %d has %d" % (name, f0, l0, f1, l1)
        cost, best = sum(f * l for f, l in used), ec.optimal_limited_cost(freq, bits)
        assert cost >= best, "%s: %d bits, below the optimum %d: the restatement is wrong" % (name, cost, best)
        acted = huffman_depth(freq) > bits
        limited[bits] += acted
        if acted:
            excess.setdefault((len(freq), bits), []).append((cost / best - 1, name))
    assert limited[7] >= 20 and limited[15] >= 20, limited
    with capsys.disabled():
        for (n, bits), xs in sorted(excess.items()):
            worst = max(xs)
            print("\nbuild_lengths, %d symbols, limit %d: the limit acted in %d inputs; bits above the optimal length-limited code: "
                  "mean %.2f %%, worst %.2f %% (%s)" % (n, bits, len(xs), 100 * sum(x for x, _ in xs) / len(xs), 100 * worst[0], worst[1]), end="")
        print()


# ---- the phases as a program under the sanitizers --------------------------------------------------------------------------------------------------
def test_phases_under_the_sanitizers(tmp_path, sim, blocks):
    """tests/hostsim/deflate_enc_main.cpp around amp_deflate.hip's phases, -fsanitize=address,undefined on the host code: every
    chunk of every family (and family E's rooms) at the four misalignments, source and destination in heap blocks of exactly the
    bytes the encoder may touch.  It must finish clean, and its streams are the shared library's."""
    exe, cases, got = str(tmp_path / "deflate_enc_main"), str(tmp_path / "cases.bin"), str(tmp_path / "streams.bin")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-x", "hip",
                           os.path.join(ROOT, "tests", "hostsim", "deflate_enc_main.cpp"), "-o", exe])
    items = [(c.name, c.data, c.room) for c in ec.CHUNKS] + [(name, c.data, room) for name, c, room, _ in room_items(blocks)]
    ec.dump(cases, items)
    r = subprocess.run([exe, cases, got], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "cases %d, streams %d" % (len(items), 4 * len(items)) in r.stdout
    raw, at = open(got, "rb").read(), 0
    for name, data, room in items:
        for skew in ec.SKEWS:
            end = raw.index(b"\n", at)
            head = raw[at:end].split()
            assert head[0].decode() == name and int(head[1]) == skew, (name, skew, head)
            n = int(head[2])
            stream = raw[end + 1:end + 1 + n]
            at = end + 1 + n
            want, = ec.encode(sim.ampdf_hostsim_blocks, data, room=room, skew=skew)
            assert stream == (want or b""), "%s, skew %d: the program's stream is not the library's" % (name, skew)
    assert at == len(raw)
