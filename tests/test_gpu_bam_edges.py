"""The device codec for BAM input (amplipy_amd/csrc/amp_bgzf.hip) on the GPU, at the edges its host twin
cannot show and zlib's default streams do not reach: the crafted DEFLATE streams of tests/deflate_craft.py side by side in one
launch, more blocks than workgroups (the grid-stride loops and the reuse of one LDS Tables object), the CRC of short and odd
blocks, and the record index and the decode on the files that make them work hard -- lanes of one launch reading what other lanes
write.  One Engine and one BamCodec serve the module; each step runs once."""
import zlib

import numpy as np
import pytest

from amplipy_amd import bam_device, lib, synth
from tests import deflate_craft as dc
from tests.bam_util import _check_file, _make_decoy_bam, _make_lseq0_bam
from tests.test_bam_native import _make_bam
from tests.deflate_craft import feed_members, mixed_feed, spans, valid_members

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = lib.Engine(synth.make_genome().size)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def dev(engine):
    c = bam_device.BamCodec(engine)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin_so(tmp_path_factory):
    return bam_device.build_twin(str(tmp_path_factory.mktemp("twin") / "libampbgzf_twin.so"))


@pytest.fixture(scope="module")
def twin(twin_so):
    c = bam_device.BamCodec(twin=twin_so)
    yield c
    c.close()


@pytest.fixture(scope="module")
def on_twin(twin):
    """What the host twin makes of the two crafted feeds, for comparison.  The streams themselves are proved in the CPU suite
    (tests/test_deflate_craft.py: zlib, the twin, the host codec, the sanitizer run): that is the gate in front of the device.
    -> (image of the valid feed, image of the mixed one, its refused members, its verdicts)."""
    _, t_valid = feed_members(twin, valid_members())
    _, t_mixed = feed_members(twin, mixed_feed()[0])
    return t_valid, t_mixed, twin.refused(), [int(v) for v in twin.verdicts()]


def test_crafted_streams_inflate_on_the_device(dev, on_twin):
    """Every valid case as the members of ONE feed: stored, fixed and dynamic blocks, second-level tables, short distances and
    matches at the end of the output decode side by side."""
    members = valid_members()
    info, image = feed_members(dev, members)
    for (name, _, want), (a, b) in zip(dc.VALID_CASES, spans(members)):
        assert image[a:b] == want, name
    assert image == b"".join(w for _, _, w in dc.VALID_CASES) == on_twin[0]
    assert info.n_refused == 0 and dev.refused() == [] and info.waits == 1 and info.n_blocks == len(members)
    assert not dev.verdicts().any()


def test_refused_streams_are_refused_on_the_device(dev, on_twin):
    """The fixed list proved clean under the sanitizers in the CPU suite, each stream once, between valid members: exactly the bad
    ones are refused -- by the decoder (verdict 1), not by the CRC check behind it, which a wrongly accepted block could pass: where
    the bytes a lenient decoder would leave are known, the member carries their CRC.  Their neighbours are intact, and the host's
    patch of a mended copy completes the image."""
    members, bad, mended = mixed_feed()
    info, image = feed_members(dev, members)
    assert info.n_refused == len(bad) and dev.refused() == bad == on_twin[2]
    assert [int(v) for v in dev.verdicts()] == [int(k in bad) for k in range(len(members))] == on_twin[3]
    want = b"".join(zlib.decompress(m[0], -15) for m in mended)
    for k, (a, b) in enumerate(spans(members)):
        assert k in bad or (image[a:b] == want[a:b] == on_twin[1][a:b]), k
    assert dev.patch_through_host(*dc.table(mended)) == len(bad)
    assert dev.info.n_refused == 0 and dev.image()[0].tobytes() == want


@pytest.fixture(scope="module")
def tiny_members():
    """16,391 members of 0 ... 130 random bytes, zlib level 6."""
    rng = np.random.default_rng(3072)
    sizes = rng.integers(0, 131, 16384 + 7)
    data = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8).tobytes()
    out, at = [], 0
    for n in (int(x) for x in sizes):
        payload = data[at:at + n]; at += n
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        out.append(dc.member(payload, co.compress(payload) + co.flush()))
    return out


def test_more_blocks_than_workgroups(dev, tiny_members):
    """3,072 workgroups inflate and 4,096 x 4 waves check: 3,073 + 5 and 16,384 + 7 blocks are the fewest that make both kernels
    take a second turn -- with the LDS tables of the turn before."""
    for n in (3073 + 5, 16384 + 7):
        members = tiny_members[:n]
        info, image = feed_members(dev, members)
        assert info.n_blocks == n and info.n_refused == 0 and info.waits == 1
        assert image == b"".join(zlib.decompress(m[0], -15) for m in members), n
    members = list(tiny_members[:3080])
    for k in (3075, 2):
        raw, isize, crc = members[k]
        members[k] = (raw, isize, crc ^ 0x00010000)
    info, _ = feed_members(dev, members)
    assert info.n_refused == 2 and dev.refused() == [2, 3075]
    # ... and in the CRC kernel's own second turn, which only the larger feed has (770 workgroups serve 3,080 blocks in one)
    members = list(tiny_members)
    for k in (16388, 8200):
        raw, isize, crc = members[k]
        members[k] = (raw, isize, crc ^ 0x00010000)
    info, _ = feed_members(dev, members)
    assert info.n_refused == 2 and dev.refused() == [8200, 16388]


def test_crc_of_short_and_odd_blocks(dev):
    """Stored blocks, so the cost is the CRC's: every length 0 ... 130 (most lanes own an empty slice), the lengths around 256,
    4,096 and the block limit, and one of 131 bytes more so that the last workgroup has idle waves."""
    rng = np.random.default_rng(64)
    lengths = list(range(0, 131)) + [255, 256, 257, 4095, 4096, 4097, 65280, 65535, 65536] + [131]
    assert len(lengths) % 4 == 1
    members = []
    for n in lengths:
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        s = dc.Stream()
        if n > 65535:
            s.stored(payload[:65535], False).stored(payload[65535:], True)
        else:
            s.stored(payload, True)
        members.append(dc.member(payload, s.done()))
    info, image = feed_members(dev, members)
    assert info.n_refused == 0 and dev.refused() == [] and image == b"".join(zlib.decompress(m[0], -15) for m in members)
    flipped = [(raw, isize, crc ^ (1 << (k % 32))) for k, (raw, isize, crc) in enumerate(members)]
    info, _ = feed_members(dev, flipped)
    assert info.n_refused == len(members) and dev.refused() == list(range(len(members))) and (dev.verdicts() == 2).all()


def test_index_and_decode_edges_on_the_device(engine, twin_so, tmp_path):
    """The files of the twin suite on the card: records and their fixed bytes straddling one-block pieces, l_seq 0 and absent QUAL,
    decoy runs and records longer than ten stretches, a file of one record.  Offsets equal to the serial walk, rows equal to
    ampbam_decode's with pads and slack, no block through the host -- and rounds, records and pieces equal to the twin's: the
    marking reaches a fixed point that does not depend on the order of the lanes."""
    def on_device():
        return bam_device.BamCodec(engine)

    def on_twin():
        return bam_device.BamCodec(twin=twin_so)

    a = str(tmp_path / "a.bam"); z = str(tmp_path / "z.bam"); d = str(tmp_path / "d.bam"); one = str(tmp_path / "one.bam")
    _make_bam(a, n=4000)
    _make_lseq0_bam(z)
    _make_decoy_bam(d, one)
    for path, pieces, ordinary in ((a, (1, 65536, 1 << 30), True), (z, (1, 4096, 1 << 30), True), (d, (1, 300000, 1 << 30), False),
                                   (one, (1, 1 << 30), True)):
        got = _check_file(on_device, path, pieces, ordinary=ordinary)
        want = _check_file(on_twin, path, pieces, ordinary=ordinary)
        for pb in pieces:
            for key in ("index_rounds", "records", "pieces", "blocks_host"):
                assert got[pb][key] == want[pb][key], (path, pb, key, got[pb], want[pb])
            assert got[pb]["blocks_host"] == 0
