"""The device codec for BAM input (amp_bgzf.hip / bam_device.py) on its host twin: the kernels' lane
functions compiled with -DAMPBGZF_HOSTSIM and run lane after lane.  Inflate against zlib, CRC against zlib and libampbam, the
record index against a serial walk, the decoded batch against ampbam_decode of the same file opened whole -- pads and slack
included -- and the refused-block path.  No GPU needed."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, bam_native, synth
from tests.bam_util import (_assert_rows, _bgzf, _blocks_of, _check_file, _make_decoy_bam, _make_lseq0_bam, _make_repeated_bam, _run,
                            _whole)
from tests.test_bam_native import _make_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """A factory of codecs on the host twin."""
    so = bam_device.build_twin(str(tmp_path_factory.mktemp("twin") / "libampbgzf_twin.so"))
    return lambda: bam_device.BamCodec(twin=so)


@pytest.fixture(scope="module")
def lane_lib(tmp_path_factory):
    """inflate_block and the lane-combined CRC of amp_bgzf.hpp behind two C functions."""
    d = tmp_path_factory.mktemp("lanes")
    src = d / "lanes.cpp"
    src.write_text('#define BGZ_HD static inline\n#include "amp_bgzf.hpp"\n'
                   'extern "C" int t_inflate(const uint8_t *in, int64_t n_in, uint8_t *out, int64_t n_out) {\n'
                   '    static ampbgzf::Tables T; return ampbgzf::inflate_block(in, (size_t)n_in, out, (size_t)n_out, T) ? 0 : -3; }\n'
                   'extern "C" uint32_t t_crc(const uint8_t *p, uint32_t n) {\n'
                   '    uint32_t tab[256], reg = 0; for (uint32_t i = 0; i < 256; ++i) tab[i] = ampbgzf::crc_table_entry(i);\n'
                   '    for (uint32_t lane = 0; lane < 64; ++lane) reg ^= ampbgzf::crc_lane(p, n, lane, tab);\n'
                   '    return ~reg; }\n')
    so = str(d / "liblanes.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "amplipy_amd", "csrc"),
                           "-o", so, str(src)])
    L = C.CDLL(so)
    L.t_inflate.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.t_crc.restype = C.c_uint32
    L.t_crc.argtypes = [C.c_void_p, C.c_uint32]
    return L


def _inflate(L, raw, n_out, pad=64):
    out = np.full(n_out + 2 * pad, 0xA5, np.uint8)
    src = np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(1, np.uint8)
    rc = L.t_inflate(C.c_void_p(src.ctypes.data), C.c_int64(len(raw)), C.c_void_p(out.ctypes.data + pad), C.c_int64(n_out))
    assert (out[:pad] == 0xA5).all() and (out[pad + n_out:] == 0xA5).all(), "wrote outside the output range"
    return rc, out[pad:pad + n_out].tobytes()


def test_block_table_is_the_files(tmp_path):
    bam = str(tmp_path / "a.bam")
    _make_bam(bam, n=900)
    tab = bam_device.block_table(bam)
    raw = open(bam, "rb").read()
    assert len(tab) >= 3 and int(tab[-1, 2]) == 0                   # the EOF block is in the table
    image = b"".join(zlib.decompress(raw[int(o):int(o + n)], -15) for o, n, _, _ in tab)
    assert image == b"".join(zlib.decompress(raw[int(o) - 18:int(o + n) + 8], 31) for o, n, _, _ in tab)
    assert [int(x) for x in tab[:, 2]] == [len(zlib.decompress(raw[int(o):int(o + n)], -15)) for o, n, _, _ in tab]
    f = bam_native.BamFile(bam)
    text, refs, first = bam_device.read_header(bam, tab)
    assert text == f.header_text and refs == f.references
    l_text = struct.unpack_from("<I", image, 4)[0]
    o = 12 + l_text
    for _ in refs:
        o += 8 + struct.unpack_from("<I", image, o)[0]
    assert first == o
    open(str(tmp_path / "x.bam"), "wb").write(b"not a bam at all")
    with pytest.raises(bam_native.AmpBamError) as e1:
        bam_native.BamFile(str(tmp_path / "x.bam"))
    with pytest.raises(bam_native.AmpBamError) as e2:
        bam_device.block_table(str(tmp_path / "x.bam"))
    assert str(e1.value) == str(e2.value)


def test_inflate_equals_zlib(lane_lib, tmp_path):
    """Every zlib level and strategy (stored, fixed, dynamic, several DEFLATE blocks per stream, the empty stream), lengths
    0 ... 65,280; wrong ISIZE, truncated, bit-flipped and random input: refused or equal, never a byte outside the range."""
    rng = np.random.default_rng(17)

    def payloads():
        yield b""
        yield b"a"
        yield b"abc" * 5000
        yield bytes(60000)
        yield rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
        yield rng.integers(0, 4, 65280, dtype=np.uint8).tobytes()
        yield bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 40000)) + bytes(rng.choice([37, 37, 37, 25, 11, 2], 25000).astype(np.uint8))
        for n in (1, 2, 7, 8, 9, 255, 256, 257, 258, 259, 300, 4095, 32768, 32769, 65280):
            yield bytes(rng.integers(0, 3, n, dtype=np.uint8))

    n_ok = 0
    for data in payloads():
        for level in range(10):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
                half = len(data) // 2
                raw = co.compress(data[:half]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[half:]) + co.flush()
                rc, got = _inflate(lane_lib, raw, len(data))
                assert rc == 0 and got == data, (len(data), level, strategy)
                n_ok += 1
                if len(data) > 300 and level == 6 and strategy == zlib.Z_DEFAULT_STRATEGY:
                    assert _inflate(lane_lib, raw, len(data) - 1)[0] != 0 and _inflate(lane_lib, raw, len(data) + 1)[0] != 0
                    assert _inflate(lane_lib, raw[:len(raw) // 2], len(data))[0] != 0
                    for _ in range(40):
                        bad = bytearray(raw); k = int(rng.integers(0, len(bad))); bad[k] ^= 1 << int(rng.integers(0, 8))
                        rc2, got2 = _inflate(lane_lib, bytes(bad), len(data))
                        assert rc2 != 0 or got2 == data or zlib.crc32(got2) != zlib.crc32(data)
    assert n_ok > 1000
    for _ in range(300):
        raw = rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes()
        _inflate(lane_lib, raw, int(rng.integers(0, 65537)))
    # the blocks of files: written by the Python codec, by libampbam (libdeflate or zlib), and the fixed-Huffman EOF block
    p1 = str(tmp_path / "py.bam"); p2 = str(tmp_path / "nat.bam")
    _make_bam(p1, n=2500)
    f = bam_native.BamFile(p1)
    b, _ = f.decode(0, f.n_records, copy=True)
    w = bam_native.BamWriter(p2, f.header_text, f, level=6)
    w.write_batch(b)
    w.close(); f.close()
    kinds = set()
    for path in (p1, p2):
        for raw, isize, crc in _blocks_of(path):
            rc, got = _inflate(lane_lib, raw, isize)
            assert rc == 0 and got == zlib.decompress(raw, -15) and zlib.crc32(got) == crc
            kinds.add((raw[0] >> 1) & 3)
    assert {1, 2} <= kinds


def test_inflate_streams_of_the_device_encoder(lane_lib, tmp_path):
    """... and on the streams of the host twin of the device DEFLATE encoder (amp_deflate.hip with -DAMPDF_HOSTSIM)."""
    from amplipy_amd import build
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.isfile("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc: the encoder's twin cannot be built")
    so = str(tmp_path / "libampdf_hostsim.so")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-function", "-DAMPDF_HOSTSIM",
                           "-o", so, os.path.join(build.CSRC, "amp_deflate.hip")])
    sim = C.CDLL(so)
    bam = str(tmp_path / "a.bam")
    _make_bam(bam, n=2500)
    image = b"".join(zlib.decompress(raw, -15) for raw, _, _ in _blocks_of(bam))
    bs, room = 0xFF00, 0xFF00 + 64
    n = (len(image) + bs - 1) // bs
    src = np.frombuffer(image, np.uint8).copy()
    out = np.zeros(n * room, np.uint8); lens = np.zeros(n, np.uint32)
    rc = sim.ampdf_hostsim_blocks(C.c_void_p(src.ctypes.data), C.c_int64(src.size), C.c_int32(bs), C.c_void_p(out.ctypes.data),
                                C.c_int64(room), C.c_int32(room), C.c_void_p(lens.ctypes.data))
    assert rc == 0 and (lens > 0).all()
    for k in range(n):
        want = image[k * bs:(k + 1) * bs]
        rc, got = _inflate(lane_lib, out[k * room:k * room + int(lens[k])].tobytes(), len(want))
        assert rc == 0 and got == want, k


def test_inflate_and_crc_under_the_sanitizers(tmp_path):
    """tests/hostsim/bgzf_fuzz.cpp under -fsanitize=address,undefined (host code only): here 4,000 valid streams with 28,000 mutated
    and 4,000 random ones; at its default count (100,000 valid, 800,000 damaged) it ran clean when the codec was written."""
    exe = str(tmp_path / "bgzf_fuzz")
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "hostsim", "bgzf_fuzz.cpp"), "-lz"])
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "valid streams 4000 (failed 0)" in r.stdout


def test_crc_equals_zlibs(lane_lib):
    L = bam_native.load()
    rng = np.random.default_rng(9)
    buf = rng.integers(0, 256, 70000, dtype=np.uint8)
    lens = list(range(0, 301)) + [int(x) for x in rng.integers(301, 65537, 200)] + [65280, 65535, 65536]
    for n in lens:
        off = int(rng.integers(0, 17)) if n + 17 < buf.size else 0
        got = int(lane_lib.t_crc(C.c_void_p(buf.ctypes.data + off), C.c_uint32(n)))
        assert got == zlib.crc32(buf[off:off + n].tobytes()) & 0xFFFFFFFF, (n, off)
        assert got == int(L.ampbam_crc32(C.c_void_p(buf.ctypes.data + off), C.c_int64(n))) or n == 0


# ---- index and decode ---------------------------------------------------------------------------------------------------------------
def test_decode_equals_ampbam_decode(twin, tmp_path):
    """_make_bam files (aux tags, an unmapped record, a record without CIGAR, QUAL absent, odd l_seq) and one with l_seq 0, at
    pieces of one block, 64 KB, 1 MB and the whole file: records and their 36 fixed bytes straddle pieces."""
    bam = str(tmp_path / "a.bam")
    _make_bam(bam, n=4000)
    st = _check_file(twin, bam, (1, 65536, 1 << 20, 1 << 30))
    assert st[1]["pieces"] > 15 and st[1 << 30]["pieces"] == 1
    p2 = _make_lseq0_bam(str(tmp_path / "z.bam"))
    _check_file(twin, p2, (1, 4096, 1 << 30))


def test_decode_of_write_batch_and_compressible_files(twin, tmp_path):
    """Files written by ampbam_write_batch, and one of repeated records that compresses about 37 x (its pieces are cut by their
    ISIZE sum as well)."""
    from tools.e2e_legs import write_bam
    g = synth.make_genome(); primers, amps = synth.make_artic_scheme()
    p1 = str(tmp_path / "wb.bam")
    write_bam(p1, synth.make_amplicon_batch(g, amps, 20000, seed=5), int(g.size))
    st = _check_file(twin, p1, (65536, 1 << 20, 1 << 30))
    assert st[65536]["index_rounds"] == st[65536]["pieces"]            # one round per piece on an ordinary file
    p2 = _make_repeated_bam(str(tmp_path / "rep.bam"), p1)
    assert sum(isz for _, isz, _ in _blocks_of(p2)) > 20 * os.path.getsize(p2)
    _check_file(twin, p2, (4096, 1 << 30))


def test_index_ignores_decoys(twin, tmp_path):
    """The decoy file of test_record_index_ignores_decoy_records (runs of 70 plausible fake records inside quality bytes) and the
    decoy that ends with its host record (test_piece_walk_does_not_guess_record_starts): exactly the offsets of a serial walk.
    Records longer than one and than ten stretches; a file of one record; the rounds are reported."""
    bam = str(tmp_path / "d.bam"); one = str(tmp_path / "one.bam")
    _make_decoy_bam(bam, one)
    st = _check_file(twin, bam, (1, 300000, 1 << 30), ordinary=False)
    assert st[1 << 30]["index_rounds"] > 1 and st[1 << 30]["waits"] >= 1           # guesses inside decoys were overruled, and counted
    st = _check_file(twin, one, (1, 1 << 30))
    assert st[1 << 30]["records"] == 1 and st[1 << 30]["index_rounds"] == 1


def test_refused_blocks_go_through_the_host(twin, tmp_path):
    """A block the codec is told to refuse is inflated by the host and patched in: same rows, blocks_host == 1.  A flipped payload
    bit, a wrong CRC and a wrong ISIZE each raise what bam_native.BamFile raises for that file."""
    bam = str(tmp_path / "a.bam")
    _make_bam(bam, n=3000)
    f, want = _whole(bam)
    for pb in (1, 1 << 30):
        rows, _, st = _run(twin, bam, pb, refuse_block=3)
        assert st["blocks_host"] == 1 and st["records"] == f.n_records
        _assert_rows(rows, want)
    f.close()
    tab = bam_device.block_table(bam)
    raw = open(bam, "rb").read()
    k = 4
    o, n = int(tab[k, 0]), int(tab[k, 1])
    damaged = {"bit": (o + n // 2, 0x10), "crc": (o + n + 1, 0x01), "isize": (o + n + 4, 0x01)}
    for name, (at, mask) in damaged.items():
        p = str(tmp_path / ("bad_%s.bam" % name))
        b = bytearray(raw); b[at] ^= mask
        open(p, "wb").write(bytes(b))
        with pytest.raises(bam_native.AmpBamError) as host:
            bam_native.BamFile(p)
        with pytest.raises(bam_native.AmpBamError) as dev:
            _run(twin, p, 1 << 30)
        assert str(dev.value) == str(host.value), name
        with pytest.raises(bam_native.AmpBamError) as dev1:
            _run(twin, p, 1)
        assert str(dev1.value) == str(host.value), name
    # a file that ends inside a record, and one whose record says block_size 5
    image = b"".join(zlib.decompress(r, -15) for r, _, _ in _blocks_of(bam))
    _, _, first = bam_device.read_header(bam, tab)
    for name, img in (("cut", image[:len(image) - 7]), ("bs", image[:first] + struct.pack("<I", 5) + image[first + 4:])):
        p = str(tmp_path / ("bad_%s.bam" % name))
        with open(p, "wb") as out:
            for a in range(0, len(img), 60000):
                out.write(_bgzf(img[a:a + 60000]))
            out.write(bam_native.BGZF_EOF)
        with pytest.raises(bam_native.AmpBamError) as host:
            bam_native.BamFile(p)
        with pytest.raises(bam_native.AmpBamError) as dev:
            _run(twin, p, 65536)
        assert str(dev.value) == str(host.value), name
