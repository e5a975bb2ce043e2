"""What the tests of the device codec for BAM input share (tests/test_bam_device_twin.py on the host twin, tests/test_gpu_bam.py and
tests/test_gpu_bam_edges.py on the device): a file's blocks, a BGZF block made by zlib, the serial walk over records, the walk of
run_amplipy over a codec made by a factory, the comparison with ampbam_decode's batch, and the files that make the record
index work hard.  A codec factory is ``lambda: BamCodec(twin=so)`` or ``lambda: BamCodec(engine)``."""
import struct
import zlib

import numpy as np

from amplipy_amd import bam_device, bam_native, bamio, synth


def _blocks_of(path):
    tab = bam_device.block_table(path)
    raw = open(path, "rb").read()
    return [(raw[int(o):int(o + n)], int(isz), int(crc)) for o, n, isz, crc in tab]


def _bgzf(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def _serial_walk(image, first):
    off = []
    o = first
    while o + 4 <= len(image):
        bs = struct.unpack_from("<I", image, o)[0]
        if o + 4 + bs > len(image):
            break
        off.append(o)
        o += 4 + bs
    return off, o


def _whole(path):
    f = bam_native.BamFile(path)                      # ampbam_open: the file opened whole, not walked in pieces
    want, _ = f.decode(0, f.n_records, copy=False)
    return f, want


def _run(factory, path, piece_bytes, refuse_block=None):
    """The walk of run_amplipy on the codec ``factory()`` makes: (rows of all pieces concatenated with the last piece's slack,
    record offsets in the file's inflated stream, stats)."""
    src = bam_device.DeviceBamInput(path, piece_bytes)
    c = factory()
    rows, offs, base, st = [], [], 0, None
    try:
        for info, st in bam_device.walk(c, src, refuse_block=refuse_block):
            img, off = c.image()
            offs.extend(int(x) + base - int(info.carry_in) for x in off)
            base += int(info.n_inflated)
            assert int(info.carry_out) <= int(info.image_bytes)
            if info.n_rows:
                rows.append(c.batch(slack=True))
    finally:
        c.close()
    return rows, offs, dict(st)


def _assert_rows(rows, want, f_n_records=None):
    """Equal to ampbam_decode's batch: scalars, offsets (piece-relative ones re-based), CIGAR words, bases and qualities with
    every pad, and 16 zero bytes of slack behind each piece's arrays."""
    for _, (cig_tail, seq_tail, qual_tail) in rows:
        assert cig_tail.size == 4 and not cig_tail.any() and seq_tail.size == 16 and not seq_tail.any() and qual_tail.size == 16 and not qual_tail.any()
    rows = [r for r, _ in rows]
    assert sum(r.n for r in rows) == want.n
    for name in ("pos", "flag", "tlen", "lseq", "src_index"):
        assert np.array_equal(np.concatenate([getattr(r, name) for r in rows]), getattr(want, name)), name
    assert np.array_equal(np.concatenate([r.cig[:int(r.cig_off[-1])] for r in rows]), want.cig)
    assert np.array_equal(np.concatenate([r.seq[:int(r.seq_off[-1]) // 2] for r in rows]), want.seq)
    assert np.array_equal(np.concatenate([r.qual[:int(r.seq_off[-1])] for r in rows]), want.qual)
    co, so, cb, sb = [], [], 0, 0
    for r in rows:
        co.append(r.cig_off[:-1] + np.uint64(cb)); so.append(r.seq_off[:-1] + np.uint64(sb))
        cb += int(r.cig_off[-1]); sb += int(r.seq_off[-1])
    assert np.array_equal(np.concatenate(co), want.cig_off[:-1]) and np.array_equal(np.concatenate(so), want.seq_off[:-1])
    assert cb == int(want.cig_off[-1]) and sb == int(want.seq_off[-1])


def _check_file(factory, path, piece_sizes, ordinary=True):
    f, want = _whole(path)
    image = b"".join(zlib.decompress(raw, -15) for raw, _, _ in _blocks_of(path))
    _, _, first = bam_device.read_header(path, bam_device.block_table(path))
    serial, end = _serial_walk(image, first)
    assert len(serial) == f.n_records and end == len(image)
    out = {}
    for pb in piece_sizes:
        rows, offs, st = _run(factory, path, pb)
        assert offs == serial, pb
        assert st["records"] == f.n_records and st["blocks_host"] == 0, (pb, st)
        if ordinary:                                  # one wait for the device per piece, one index round
            assert st["waits"] == st["pieces"] and st["index_rounds"] <= st["pieces"], (pb, st)
        _assert_rows(rows, want)
        out[pb] = st
    f.close()
    return out


# ---- files that make the index and the decode work hard -------------------------------------------------------------------------------
def _header():
    g = synth.make_genome()
    return g, bamio.Header("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:SYN_REF\tLN:%d\n" % g.size, [("SYN_REF", int(g.size))])


def _make_lseq0_bam(path):
    """3,000 records: every third with l_seq 0, lengths 0 ... 39 otherwise, every fifth without QUAL."""
    _, hdr = _header()
    w = bamio.AlignmentWriter(path, "wb", hdr)
    rng = np.random.default_rng(4)
    for i in range(3000):
        L = int(rng.integers(0, 40)) if i % 3 else 0
        seq = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, L))
        w.write(bamio.Rec("q%d" % i, 0, 0, 10 + i, 60, [(0, max(L, 1))], -1, -1, 0, seq if L else None,
                          bytes(rng.integers(0, 60, L).astype(np.uint8)) if L and i % 5 else None))
    w.close()
    return path


def _make_decoy_bam(path, one_path=None):
    """6,000 mixed records with runs of 70 plausible fake records inside quality bytes and of 80 inside an aux tag, and records longer
    than one and than ten stretches; ``one_path``: a file of the first record alone."""
    g, hdr = _header()
    _, amps = synth.make_artic_scheme()
    segs = synth.make_mixed_segments(g, amps, 6000, seed=3)
    fake = struct.pack("<iiiBBHHHIiii", 34, 0, 5, 2, 60, 4680, 0, 0, 0, -1, -1, 0) + b"A\0"
    decoy_q = bytes([30]) * 3 + fake * 70 + bytes([30]) * 40
    tag = b"zzBC" + struct.pack("<I", 80 * len(fake)) + fake * 80
    long_q = bytes([31]) * 50000                                       # a record longer than ten stretches
    recs = []
    for i, s in enumerate(segs):
        r = bamio.Rec("r%d" % i, s.flag, 0, s.reference_start, 60, s.cigartuples, 0, s.reference_start, s.template_length,
                      s.query_sequence, bytes(s.query_qualities))
        if i % 97 == 13:
            r.aux_bam = tag
        recs.append(r)
        if i % 150 == 75:
            L = len(decoy_q)
            recs.append(bamio.Rec("decoy%d" % i, 0, 0, 100 + i % 1000, 60, [(0, L)], -1, -1, 0, "ACGT" * (L // 4) + "A" * (L % 4), decoy_q))
        if i % 1500 == 700:
            L = len(long_q)
            recs.append(bamio.Rec("long%d" % i, 0, 0, 100, 60, [(0, L)], -1, -1, 0, "ACGT" * (L // 4), long_q))
    w = bamio.AlignmentWriter(path, "wb", hdr)
    for r in recs:
        w.write(r)
    w.close()
    if one_path:
        w = bamio.AlignmentWriter(one_path, "wb", hdr)
        w.write(recs[0])
        w.close()
    return path


def _make_repeated_bam(path, like_path):
    """One record 20,000 times through ampbam_write_batch (header and references of ``like_path``): compresses about 37 x."""
    g = synth.make_genome(); _, amps = synth.make_artic_scheme()
    one = synth.make_amplicon_batch(g, amps, 1, seed=1)
    f = bam_native.BamFile(like_path)
    w = bam_native.BamWriter(path, f.header_text, f, level=6)
    for _ in range(40):
        for k in range(500):
            w.write_batch(one, name_base=0)
    w.close(); f.close()
    return path
