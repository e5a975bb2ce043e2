"""The crafted DEFLATE streams of tests/deflate_craft.py on the CPU: the generator against zlib, then every case through the host
twin of the device codec for BAM input (one feed of all members, amp_bgzf.hip with -DAMPBGZF_HOSTSIM), through libampbam's own
decoder (ampbam_inflate_raw, amp_inflate.hpp) and, under AddressSanitizer / UBSan, through tests/hostsim/bgzf_cases.cpp.  What
passes here is what tests/test_gpu_bam_edges.py sends to the device.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, bam_native
from tests import deflate_craft as dc
from tests.deflate_craft import feed_members, mixed_feed, spans, valid_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = bam_device.build_twin(str(tmp_path_factory.mktemp("twin") / "libampbgzf_twin.so"))
    c = bam_device.BamCodec(twin=so)
    yield c
    c.close()


def host_inflate(raw, n_out, pad=64):
    """ampbam_inflate_raw between two guard zones: (return code, bytes)."""
    L = bam_native.load()
    out = np.full(n_out + 2 * pad, 0xA5, np.uint8)
    src = np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(1, np.uint8)
    rc = L.ampbam_inflate_raw(C.c_void_p(src.ctypes.data), C.c_int64(len(raw)), C.c_void_p(out.ctypes.data + pad), C.c_int64(n_out))
    assert (out[:pad] == 0xA5).all() and (out[pad + n_out:] == 0xA5).all(), "wrote outside the output range"
    return rc, out[pad:pad + n_out].tobytes()


def sanitizer_run(tmp_dir):
    """All cases through tests/hostsim/bgzf_cases.cpp built with -fsanitize=address,undefined (host code only): its answer."""
    exe = os.path.join(str(tmp_dir), "bgzf_cases"); cases = os.path.join(str(tmp_dir), "cases.bin")
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "hostsim", "bgzf_cases.cpp")])
    dc.dump(cases)
    return subprocess.run([exe, cases], capture_output=True, text=True)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def test_generator_agrees_with_zlib():
    names = [c[0] for c in dc.VALID_CASES] + [c[0] for c in dc.REFUSED_CASES]
    assert len(set(names)) == len(names)
    for name, raw, want in dc.VALID_CASES:
        assert zlib.decompress(raw, -15) == want, name
        assert len(want) <= 65536 and (len(raw) <= 65535 or name == "stored_65535"), name
    for name, raw, isize in dc.REFUSED_CASES:
        try:
            got = zlib.decompress(raw, -15)
        except zlib.error:
            continue
        assert len(got) != isize, name


def test_case_list_holds_what_it_promises():
    """Block types, bit phases, code depths and sizes are what the device tests rely on."""
    by = {name: (raw, want) for name, raw, want in dc.VALID_CASES}
    deep = [n for n in by if n.startswith("dynamic_random_")]
    assert len(deep) >= 60 and {len(by[n][1]) for n in deep} >= {1, 100, 5000, 65536}
    assert {int(n.split("hlit")[1].split("_")[0]) for n in by if n.startswith("dynamic_hlit")} == {257, 258, 270, 285, 286}
    assert {int(n.split("hdist")[1]) for n in by if n.startswith("dynamic_hlit")} == {1, 2, 5, 29, 30}
    assert len(by["stored_65535"][1]) == 65535 and by["stored_empty_final"][0] == b"\x01\0\0\xff\xff"
    assert sum(n.startswith("fixed_d") and "_l" in n for n in by) == 8 * 3 * 5 and sum(n.startswith("zlib_") for n in by) == 3 * 10 * 5
    phases = set()                                                     # bit phase at which the stored block's header starts
    for k in range(12):
        (name, (raw, want)), = [(n, v) for n, v in by.items() if n.startswith("fixed_%d_stored_" % k)]
        mid = want[k:k + int(name.split("_")[3])]                      # the stored bytes: found in the stream behind LEN and NLEN
        at = raw.index(len(mid).to_bytes(2, "little") + (len(mid) ^ 0xFFFF).to_bytes(2, "little") + mid)
        bits = 3 + sum(8 if b < 144 else 9 for b in want[:k]) + 7     # the fixed block in front: header, k literals, end of block
        assert at == (bits + 3 + 7) // 8, name                         # (the stored header's 3 bits, then up to the next byte)
        phases.add(bits % 8)
    assert phases == set(range(8))
    rng = np.random.default_rng(3)
    for n in (16, 17, 30, 100, 286):
        lens = dc.random_complete_lengths(rng, n)
        assert len(lens) == n and max(lens) == 15 and min(lens) >= 1 and dc.kraft(lens) == 32768
    assert dc.play([1, 2, (5, 2), 3]) == bytes([1, 2, 1, 2, 1, 2, 1, 3])
    # length 258 both ways
    assert dc.fixed([0, (258, 1)]) != dc.fixed([0, (258, 1, 284)])
    assert zlib.decompress(dc.fixed([0, (258, 1)]), -15) == zlib.decompress(dc.fixed([0, (258, 1, 284)]), -15) == bytes(259)
    assert len(dc.REFUSED_CASES) == 15


# ---- the decoders -------------------------------------------------------------------------------------------------------------------------
def test_valid_cases_through_the_twin(twin):
    members = valid_members()
    info, image = feed_members(twin, members)
    assert info.n_refused == 0 and twin.refused() == [] and info.n_blocks == len(members) and info.waits == 1
    for (name, _, want), (a, b) in zip(dc.VALID_CASES, spans(members)):
        assert image[a:b] == want, name
    assert len(image) == sum(len(w) for _, _, w in dc.VALID_CASES)


def test_valid_cases_through_the_host_codec():
    for name, raw, want in dc.VALID_CASES:
        rc, got = host_inflate(raw, len(want))
        assert rc == 0 and got == want, name


def test_refused_cases_are_refused(twin):
    for name, raw, isize in dc.REFUSED_CASES:
        assert host_inflate(raw, isize)[0] != 0, name
    for k, (name, raw, isize) in enumerate(dc.REFUSED_CASES):          # (its CRC is that of the bytes a lenient decoder would leave)
        info, _ = feed_members(twin, [dc.refused_member(k)])
        assert info.n_refused == 1 and twin.refused() == [0] and list(twin.verdicts()) == [1], name
    members, bad, mended = mixed_feed()
    info, image = feed_members(twin, members)
    assert info.n_refused == len(bad) == len(dc.REFUSED_CASES) and twin.refused() == bad
    assert [int(v) for v in twin.verdicts()] == [int(k in bad) for k in range(len(members))]     # by the decoder, not by the CRC
    want = b"".join(zlib.decompress(m[0], -15) for m in mended)
    for k, (a, b) in enumerate(spans(members)):
        assert k in bad or image[a:b] == want[a:b], k            # the valid members of the same feed are intact
    assert twin.patch_through_host(*dc.table(mended)) == len(bad)   # the host's patch of the mended copy
    assert twin.info.n_refused == 0 and twin.image()[0].tobytes() == want


def test_crafted_streams_under_the_sanitizers(tmp_path):
    r = sanitizer_run(tmp_path)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "valid %d, refused %d, failed 0" % (len(dc.VALID_CASES), len(dc.REFUSED_CASES)) in r.stdout
