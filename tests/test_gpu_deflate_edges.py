"""The DEFLATE encoder on the device against its own phases on the host (amp_deflate.hip with -DAMPDF_HOSTSIM), byte for byte, where
the two could part: the crafted chunks of tests/deflate_enc_craft.py -- tests/test_deflate_enc_craft.py has read their host streams
token by token, so equality carries every one of those facts over -- and the paths only a device run takes: a second and a third
piece of the host-pointer entry and the reuse of its slots, workgroups that take several chunks of unlike content one after the
other, destinations and strides that are not dword-aligned, the four misalignments of the source, and the entry whose byte count
is read on the device."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import deflate_enc_craft as ec
from tests.test_gpu_deflate import _check_streams

pytestmark = pytest.mark.gpu

PATTERN = ec.PATTERN


@pytest.fixture(scope="module")
def libs():
    """(libamplihip, the host phases' library), argument types set."""
    from amplipy_amd import lib
    L = lib.load()
    L.amp_deflate_blocks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    L.amp_deflate_blocks_device.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.amp_deflate_blocks_device_counted.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                                    C.c_void_p, C.c_void_p]
    return L, ec.hostsim_library()


def on_device(L):
    return lambda *a: L.amp_deflate_blocks(0, *a)


def device_entry(L, data, block_bytes, room, stride, in_skew=0, out_skew=0, count=None, max_bytes=None):
    """amp_deflate_blocks_device (count is None) or amp_deflate_blocks_device_counted on torch tensors: the source ``in_skew`` bytes
    behind a dword boundary, the destination ``out_skew`` bytes behind one.  Returns ([stream or None per chunk that has one],
    out_len as it came back); every byte of the destination outside a stream must still hold the pattern."""
    import torch
    n = len(data) if max_bytes is None else max_bytes
    nb = (n + block_bytes - 1) // block_bytes
    src = np.full(len(data) + 16, 0x5A, np.uint8)
    src[4 + in_skew:4 + in_skew + len(data)] = np.frombuffer(data, np.uint8)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((out_skew + nb * stride + ec.GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    d_len = torch.full((nb + 1,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")       # 0xA5A5A5A5
    assert d_in.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    if count is None:
        rc = L.amp_deflate_blocks_device(0, d_in.data_ptr() + 4 + in_skew, n, block_bytes, d_out.data_ptr() + out_skew, stride, room,
                                         d_len.data_ptr(), None)
    else:
        d_n = torch.tensor([count], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = L.amp_deflate_blocks_device_counted(0, d_in.data_ptr() + 4 + in_skew, d_n.data_ptr(), n, block_bytes, d_out.data_ptr() + out_skew,
                                                 stride, room, d_len.data_ptr(), None)
    assert rc == 0 and L.amp_deflate_sync(0) == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    lens = d_len.cpu().numpy().view(np.uint32)
    assert lens[nb] == 0xA5A5A5A5
    done = nb if count is None else (min(count, n) + block_bytes - 1) // block_bytes
    streams, clean = [], np.ones(out.size, bool)
    for k in range(done):
        ln = int(lens[k])
        assert ln <= room, "chunk %d: length %d beyond the room %d" % (k, ln, room)
        at = out_skew + k * stride
        streams.append(out[at:at + ln].tobytes() if ln else None)
        clean[at:at + ln] = False
    assert (out[clean] == PATTERN).all(), "bytes outside the streams were written: at %r" % np.flatnonzero(clean & (out != PATTERN))[:8]
    assert (lens[done:] == 0xA5A5A5A5).all(), "out_len of chunks beyond the count was written"
    return streams


def host_streams(sim, data, block_bytes, room):
    return ec.encode(sim.ampdf_hostsim_blocks, data, block_bytes=block_bytes, room=room)


# ---- 1. the crafted chunks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E", "X"])
def test_crafted_chunks_are_the_host_phases_streams(libs, family):
    L, sim = libs
    n = 0
    for c in ec.CHUNKS:
        if c.family != family:
            continue
        want, = ec.encode(sim.ampdf_hostsim_blocks, c.data, room=c.room)
        rooms = [(c.room, want)]
        if family == "E":
            rooms += [(room, None) for room, _ in ec.room_cases(c, want)]
        for room, ref in rooms:
            if ref is None:
                ref, = ec.encode(sim.ampdf_hostsim_blocks, c.data, room=room)
            got, = ec.encode(on_device(L), c.data, room=room)
            assert got == ref, "%s, room %d: the device's stream is not the host phases'" % (c.name, room)
            _check_streams(c.data, [got], block_bytes=len(c.data), allow_none=True)
            n += 1
    assert n >= 3


def test_source_misalignments_on_the_device_entry(libs):
    """Family A at the four misalignments of the source: one stream each, the host phases'."""
    L, sim = libs
    for c in ec.FAMILY_A:
        want, = ec.encode(sim.ampdf_hostsim_blocks, c.data)
        for skew in ec.SKEWS:
            got, = device_entry(L, c.data, len(c.data), ec.ROOM, 65536, in_skew=skew)
            assert got == want, "%s: source misaligned by %d" % (c.name, skew)
        assert zlib.decompress(want, -15) == c.data


# ---- 2. pieces of the host-pointer entry ---------------------------------------------------------------------------------------------------
def test_pieces_and_slots_of_the_host_entry(libs):
    """block_bytes 64: 255 to 1300 chunks are one to six pieces of PIECE_BLOCKS chunks on N_SLOTS slots, call after call."""
    L, sim = libs
    rng = np.random.default_rng(41)
    bs, room = 64, 64 + 5
    assert ec.PIECE_BLOCKS == 256 and ec.N_SLOTS == 2
    for n_chunks in (1300, 255, 513, 256, 512, 257):
        data = ec.bam_like(rng, n_chunks * bs - 17)                      # (a short last chunk)
        got = ec.encode(on_device(L), data, block_bytes=bs, room=room)     # (checks the guard bytes)
        want = host_streams(sim, data, bs, room)
        assert len(got) == n_chunks
        for k in sorted({0, n_chunks - 1} | {b + d for b in range(ec.PIECE_BLOCKS, n_chunks, ec.PIECE_BLOCKS) for d in (-1, 0) if b + d < n_chunks}):
            assert got[k] == want[k], "%d chunks: chunk %d, next to a piece boundary" % (n_chunks, k)
            assert zlib.decompress(got[k], -15) == data[k * bs:(k + 1) * bs]
        assert got == want, "%d chunks: first difference at chunk %d" % (n_chunks, [a == b for a, b in zip(got, want)].index(False))
        assert sum(1 for s in got if s[0] & 7 == 5) > n_chunks // 4 and sum(1 for s in got if s[0] & 7 == 1) > n_chunks // 8


# ---- 3. the device entry ---------------------------------------------------------------------------------------------------------------------
def test_more_chunks_than_compute_units(libs):
    import torch
    L, sim = libs
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(43)
    for n_chunks in (n_cu + 1, 3 * n_cu + 5):                          # a workgroup takes 2, then 4 chunks
        data = ec.unlike_chunks(rng, n_chunks, n_cu)
        got = device_entry(L, data, 300, 320, 320)
        want = host_streams(sim, data, 300, 320)
        assert got == want, "%d chunks on %d CUs: first difference at chunk %d" % (n_chunks, n_cu, [a == b for a, b in zip(got, want)].index(False))
        assert {s[0] & 7 for s in got} == {1, 5} and min(len(s) for s in got) < 30
    _check_streams(data, got, block_bytes=300)


def test_unaligned_destination_and_stride(libs):
    L, sim = libs
    rng = np.random.default_rng(47)
    data = ec.unlike_chunks(rng, 41, 7)[:-123]
    room = 320
    want = host_streams(sim, data, 300, room)
    assert {s[0] & 7 for s in want} == {1, 5}
    for skew in (1, 2, 3):
        for extra in (1, 2, 3):
            got = device_entry(L, data, 300, room, room + extra, out_skew=skew)
            assert got == want, "destination misaligned by %d, stride %d" % (skew, room + extra)


def test_counted_entry(libs):
    """amp_deflate_blocks_device_counted: the byte count is read on the device; chunks beyond it are left alone."""
    L, sim = libs
    rng = np.random.default_rng(53)
    bs, room, max_bytes = 512, 512 + 5, 40 * 512
    data = ec.bam_like(rng, max_bytes)
    for count in (0, 1, 512, 513, 39 * 512 + 1, 40 * 512, 40 * 512 + 1000):
        got = device_entry(L, data, bs, room, room + 3, count=count, max_bytes=max_bytes)
        n = min(count, max_bytes)
        want = host_streams(sim, data[:n], bs, room) if n else []
        assert got == want, "count %d" % count
        if n:
            _check_streams(data[:n], got, block_bytes=bs)
