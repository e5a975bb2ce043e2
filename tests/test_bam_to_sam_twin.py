"""Trimmed reads of a BAM input as SAM text on the device codec (amp_bam_text_check / amp_bam_format, amplipy_amd/csrc/amp_bamtext.hip;
DESIGN.md section 14) on its host twin: the lane functions compiled with -DAMPBGZF_HOSTSIM and run lane after lane.  The text
against bamio.AlignmentWriter(mode "w").write(rec, pos=, cigar=) of the Recs bamio.AlignmentReader yields, at several piece sizes;
the oddness rule; '%g' of float32 in integers; the routing function of run_amplipy.  No GPU needed."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from amplipy_amd import amplipy, bam_device, bamio, lib, synth
from tests import sam_util as U
from tests.test_bam_reencode_twin import G, AMPS, Results, _keep, _made_up_results, _oracle_results, twin        # noqa: F401 (twin: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("SYN_REF", int(G.size)), ("chr|2", 5000), ("third.ref", 77)]
HDR = bamio.Header("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@PG\tID:sim\tPN:sim\n", REFS)
PIECES = (1, 65536, 1 << 30)                          # one block, 64 KB, the whole file
ESTATE = -5
REASON = {n: k for k, n in enumerate(bam_device.ODD_REASONS)}


def write_raw(path, chunks, hdr=HDR):
    """A BAM file of ``chunks``: Recs (through the Python codec) or the bytes of records, block_size word included."""
    w = bamio.AlignmentWriter(path, "wb", hdr)
    for c in chunks:
        if isinstance(c, bytes):
            w._w.write(c)
        else:
            w.write(c)
    w.close()
    return path


def raw_record(name=b"q\0", flag=0, ref_id=0, pos=10, mapq=60, cigar=(0x80,), next_ref=-1, next_pos=-1, tlen=0, seq=b"\x12\x48", qual=b"\x1e" * 4,
               l_seq=None, aux=b"", l_name=None):
    """The bytes of one record, every field as given (nothing checked)."""
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) if l_name is None else l_name, mapq, 4681, len(cigar), flag,
                       len(qual) if l_seq is None else l_seq, next_ref, next_pos, tlen)
    body += name + struct.pack("<%dI" % len(cigar), *cigar) + seq + qual + aux
    return struct.pack("<i", len(body)) + body


def python_rows(path):
    """The Recs of the file that are rows (A:902), in order."""
    return [r for r in bamio.AlignmentReader(path, "rb") if not (r.flag & 4) and r.cigar is not None]


def python_text(rows, res, keep, hdr=HDR):
    out = io.StringIO()
    w = bamio.AlignmentWriter(None, "w", hdr, fileobj=out)
    start = out.tell()
    for k, r in enumerate(rows):
        if keep[k]:
            w.write(r, pos=int(res.new_pos[k]), cigar=[(int(v) & 15, int(v) >> 4) for v in res.words[k]])
    return out.getvalue()[start:].encode()


def twin_text(twin, path, res, piece_bytes, min_length, include_no_primer, first_bad=-1, hdr=HDR):
    """run_amplipy's walk on the twin with the results ``res`` of the whole file's rows: (the text of all formats, the check infos,
    the format infos).  Every piece is checked; one with an odd row answers AMP_ESTATE to format."""
    src = bam_device.DeviceBamInput(path, piece_bytes)
    c = bam_device.BamCodec(twin=twin)
    c.set_references([n for n, _ in hdr.refs])
    text, checks, formats, lo = [], [], [], 0
    for info, st in bam_device.walk(c, src):
        ti = c.text_check()
        assert ti.waits == (1 if info.n_rows else 0)
        checks.append((int(ti.first_odd_row), int(ti.odd_reason), lo))
        local_bad = -1
        if info.n_rows:
            b = c.batch()
            hi = lo + b.n
            local_bad = first_bad - lo if lo <= first_bad < hi else -1
            c.set_trim(res.rows(b, lo, hi), first_bad=local_bad)
            lo = hi
        if ti.first_odd_row >= 0:
            with pytest.raises(lib.AmpliHipError) as e:
                c.format(min_length, include_no_primer)
            assert e.value.rc == ESTATE
            continue
        retries = getattr(c, "text_retries", 0)
        t, fi = c.format(min_length, include_no_primer)
        assert fi.waits <= 2 + (getattr(c, "text_retries", 0) - retries) and fi.n_bytes == len(t) and t.count(b"\n") == fi.n_rows_written
        assert int(c.L.amp_bam_twin_text_guard(c.h)) == 0
        text.append(t); formats.append(fi)
        if local_bad >= 0:
            break
    c.close()
    return b"".join(text), checks, formats


def all_pieces(twin, path, res, min_length=30, include_no_primer=False, first_bad=-1, pieces=PIECES, hdr=HDR):
    rows = python_rows(path)
    want = python_text(rows, res, _keep(res, min_length, include_no_primer, first_bad), hdr)
    for pb in pieces:
        got, checks, formats = twin_text(twin, path, res, pb, min_length, include_no_primer, first_bad, hdr)
        assert all(c[0] == -1 for c in checks), (pb, [c for c in checks if c[0] >= 0][:3])
        assert got == want, (pb, first_difference(got, want))
    return want


def first_difference(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for k, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return k, x[:300], y[:300]
    return len(la), len(lb)


def pool_recs(segs, seed, prefix="r"):
    """Recs of the segments with up to five AUX_POOL fields, mates on any of the three references."""
    rng = np.random.default_rng(seed)
    recs = []
    for i, s in enumerate(segs):
        aux = [U.AUX_POOL[int(k)] for k in rng.choice(len(U.AUX_POOL), int(rng.integers(0, 6)), replace=False)]
        nref = int(rng.integers(-1, 3))
        recs.append(bamio.Rec("%s%d/%d" % (prefix, i, int(rng.integers(0, 1000))), s.flag, 0, s.reference_start, int(rng.integers(0, 61)), s.cigartuples,
                              nref, int(rng.integers(0, 29000)) if nref >= 0 else -1, s.template_length, s.query_sequence, bytes(s.query_qualities),
                              aux_sam=aux))
    return recs


def identity_results(want):
    old = np.diff(want.cig_off.astype(np.int64))
    words = [want.cig[int(want.cig_off[r]):int(want.cig_off[r + 1])].copy() for r in range(want.n)]
    return Results(want, want.pos.copy(), old.astype(np.uint32), words, np.full(want.n, 1 << 20, np.int32), np.zeros(want.n, np.uint8))


# ---- the text ------------------------------------------------------------------------------------------------------------------------------
def test_text_equals_the_python_codecs_on_seeded_reads(twin, tmp_path):
    """Amplicon, config-5 and many-op records with AUX_POOL aux; results from the oracle (CIGARs grow and shrink) and results that
    change nothing; include_no_primer both ways; rows behind a failing row; pieces of one block, 64 KB and whole (a record that
    spans two pieces among them)."""
    rng = np.random.default_rng(5)
    segs = synth.make_amplicon_batch(G, AMPS, 1500, seed=5).segments() + synth.make_mixed_segments(G, AMPS, 1500, seed=3) \
        + U.many_op_segments(rng, 600, G.size, max_len=600)
    recs = pool_recs(segs, 17)
    recs[700].aux_sam = ["XL:Z:" + "long" * 20000]                       # 80,000 bytes: the record spans two blocks, so two pieces
    for k in range(100, 3000, 211):                                      # records that are no rows between them
        recs.insert(k, bamio.Rec("u%d" % k, 4, -1, -1, 0, None, -1, -1, 0, "ACGT", bytes([30] * 4), aux_sam=["XX:i:1"]))
    path = write_raw(str(tmp_path / "seeded.bam"), recs)
    want, res = _oracle_results(path)
    old = np.diff(want.cig_off.astype(np.int64))
    assert (res.new_ncig.astype(np.int64) > old).any() and (res.new_ncig.astype(np.int64) < old).any()
    text = all_pieces(twin, path, res)
    assert text.count(b"\n") > 1000
    all_pieces(twin, path, res, include_no_primer=True, pieces=(65536,))
    part = all_pieces(twin, path, res, include_no_primer=True, first_bad=want.n // 2, pieces=(1, 1 << 30))
    whole = all_pieces(twin, path, identity_results(want), include_no_primer=True, pieces=(1, 1 << 30))
    assert whole.count(b"\n") == want.n and 0 < part.count(b"\n") < want.n
    none = all_pieces(twin, path, res, min_length=10 ** 6, include_no_primer=True, pieces=(1, 1 << 30))       # pieces without a kept row
    assert none == b""


B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
EDGES = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}


def b_array(tag, st, vals):
    return tag + b"B" + st.encode() + struct.pack("<I%d%s" % (len(vals), B_FMT[st]), len(vals), *vals)


def corner_recs():
    rng = np.random.default_rng(99)
    recs = []

    def rec(name="c", l_seq=20, qual=True, aux=b"", **kw):
        seq = "".join(rng.choice(list("=ACMGRSVTWYHKDBN"), l_seq)) if l_seq else None
        q = bytes(rng.integers(0, 94, l_seq, dtype=np.uint8)) if (l_seq and qual) else None
        d = dict(flag=int(rng.choice([0, 16, 99, 147])), ref_id=0, pos=100, mapq=int(rng.integers(0, 256)), cigar=[(0, max(l_seq, 1))], next_ref_id=0,
                 next_pos=50, tlen=-20)
        d.update(kw)
        recs.append(bamio.Rec("%s%d" % (name, len(recs)), d["flag"], d["ref_id"], d["pos"], d["mapq"], d["cigar"], d["next_ref_id"], d["next_pos"],
                              d["tlen"], seq, q, aux_bam=aux))
    for l_seq in (0, 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000):
        rec(l_seq=l_seq)
        rec(l_seq=l_seq, qual=False)                                     # QUAL 0xFF...
    rec(name="")
    recs[-1].qname = "n"                                                 # QNAME of 1 byte, and of 254
    rec(name="")
    recs[-1].qname = "".join(chr(33 + k % 94) for k in range(254))
    for n_aux in (0, 1, 63, 64, 65, 100):
        rec(aux=b"".join(b"%c%ci" % (65 + k // 26, 97 + k % 26) + struct.pack("<i", k * 1000003 - 50000000) for k in range(n_aux)))
    for n_z in (0, 7, 8, 9, 5000):
        body = bytes(32 + k % 95 for k in range(n_z))
        rec(aux=b"NMC\x07" + b"zzZ" + body + b"\0" + b"hhH" + body.hex().upper().encode()[:n_z] + b"\0" + b"XSA+")
    for st in "cCsSiIf":
        for n in (0, 1, 300):
            if st == "f":
                vals = [float(np.float32(v)) for v in rng.uniform(-1000, 1000, n)]
            else:
                lo, hi = EDGES[st]
                vals = [int(v) for v in rng.integers(lo, hi + 1, n)]
                vals[:2] = [lo, hi][:n]
            rec(aux=b"NMC\x01" + b_array(b"ba", st, vals) + b"XSA-")
    rec(aux=b"".join(b"e%c%c" % (48 + k, t.encode()[0]) + struct.pack("<" + B_FMT[t], EDGES[t][k % 2]) for k, t in enumerate("ccCCssSSiiII")))
    rec(aux=b"f0f" + struct.pack("<f", 0.25) + b"f1f" + struct.pack("<f", -0.0) + b"f2f" + struct.pack("<f", 0.0) + b"f3f" + struct.pack("<f", 1e6)
        + b"f4f" + struct.pack("<f", 123456.7) + b"f5f" + struct.pack("<f", -9.2e18) + b"f6f" + struct.pack("<f", 0.000123))
    rec(next_pos=2 ** 31 - 1, tlen=-2 ** 31, pos=2 ** 31 - 2)
    rec(next_pos=-1, tlen=2 ** 31 - 1, pos=0)
    rec(ref_id=-1, next_ref_id=-1)
    rec(ref_id=1, next_ref_id=1)                                         # RNEXT '='
    rec(ref_id=1, next_ref_id=2)
    rec(ref_id=2, next_ref_id=-1)
    rec(ref_id=-1, next_ref_id=2)
    rec(cigar=[(op, 1 + op) for op in range(10)], l_seq=30)              # every op code
    rec(cigar=[(0, 2 ** 28 - 1)], l_seq=3)
    return recs


def test_hand_written_corners(twin, tmp_path):
    """l_seq 0, 1, 2, 7, 8, 9, 63, 64, 65 and more with and without qualities; QNAME of 1 and 254 bytes; 0, 1, 63, 64, 65 and 100 aux
    fields; Z and H of 0, 7, 8, 9 and 5,000 bytes; B with 0, 1 and 300 elements of every subtype; every integer type at both
    edges; floats; next_pos 2^31 - 1 and tlen -2^31; ref_id -1; next_ref_id equal, different and -1; new_pos 0 and -1; a new CIGAR
    of 0 ops and of old + 3."""
    path = write_raw(str(tmp_path / "corners.bam"), corner_recs())
    rows = python_rows(path)
    f = bam_device.bam_native.BamFile(path)
    want, _ = f.decode(0, f.n_records, copy=True)
    f.close()
    assert want.n == len(rows)
    for seed in (1, 2):
        res = _made_up_results(want, seed, drop_runs=False)
        res.ref_len[:] = 100; res.trim_flags[:] = 1                      # every row kept
        old = np.diff(want.cig_off.astype(np.int64))
        assert (res.new_pos == 0).any() and (res.new_pos == -1).any() and (res.new_ncig == 0).any() and (res.new_ncig.astype(np.int64) == old + 3).any()
        text = all_pieces(twin, path, res)
        assert text.count(b"\n") == want.n
    ident = all_pieces(twin, path, identity_results(want), include_no_primer=True, pieces=(1 << 30,))
    assert b"\t=\t2147483648\t-2147483648\t" in ident and b"\t=\t0\t2147483647\t" in ident       # PNEXT in 64 bits; next_pos -1 gives 0
    assert b"\tf1:f:-0\tf2:f:0\tf3:f:1e+06\tf4:f:123457\tf5:f:-9.2e+18\tf6:f:0.000123\n" in ident
    assert b"\tba:B:c\tXS:A:-\n" in ident and b"\t1M2I3D4N5S6H7P8=9X10B\t" in ident


# ---- floats ------------------------------------------------------------------------------------------------------------------------------
LO_BITS, HI_BITS = 0x38D1B718, 0x5F000000              # the float32 behind 9.99999975e-05; 2^63


def float_patterns(n, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(LO_BITS, HI_BITS, n, dtype=np.uint32)
    per_exp = np.concatenate([(np.uint32(e) << np.uint32(23)) | rng.integers(0, 1 << 23, 100, dtype=np.uint32) for e in range(114, 190)])
    near = []
    for v in (1e-4, 1e-3, 1e5, 1e6, 999999.5, 99999.95, 1e7, 2.0 ** 62, 1.0, 10.0, 9.999995, 0.5):
        b = int(np.float32(v).view(np.uint32))
        near += list(range(b - 40, b + 41))
    near += list(range(LO_BITS, LO_BITS + 50)) + list(range(HI_BITS - 50, HI_BITS))
    all_ = np.concatenate([bits, per_exp, np.array([b for b in near if LO_BITS <= b < HI_BITS], np.uint32), np.zeros(4, np.uint32)])
    all_ = all_ | (rng.integers(0, 2, all_.size, dtype=np.uint32) << np.uint32(31))
    return all_


def float_carrier_recs(bits):
    """Records that carry the bit patterns 2,000 each in a B:f array (and the first twenty of each as f fields)."""
    recs = []
    for k in range(0, bits.size, 2000):
        chunk = bits[k:k + 2000]
        aux = b"flB" + b"f" + struct.pack("<I", chunk.size) + chunk.astype("<u4").tobytes() + b"".join(b"f%cf" % (65 + j) + chunk[j:j + 1].astype("<u4").tobytes()
                                                                                                      for j in range(min(20, chunk.size)))
        recs.append(bamio.Rec("f%d" % k, 0, 0, 10, 60, [(0, 4)], -1, -1, 0, "ACGT", bytes([30] * 4), aux_bam=aux))
    return recs


def percent_g_of_arrays(text):
    """The elements of the B:f array of every line (its first aux field, behind "fl:B:f,"), joined by commas."""
    return b",".join(line.split(b"\t")[11][7:] for line in text.split(b"\n")[:-1])


def test_floats_equal_percent_g(twin, tmp_path):
    """100,000 seeded in-set bit patterns, 100 per binary exponent, the neighbours of 1e-4, 1e6, 999999.5, 2^62 and 2^63, both
    zeros: carried in B:f arrays (and a few as f fields), compared with '%g' through the Python codec."""
    bits = float_patterns(100000, 7)
    assert bits.size >= 100000
    path = write_raw(str(tmp_path / "floats.bam"), float_carrier_recs(bits))
    f = bam_device.bam_native.BamFile(path)
    want, _ = f.decode(0, f.n_records, copy=True)
    f.close()
    text = all_pieces(twin, path, identity_results(want), include_no_primer=True, pieces=(1 << 30,))
    # the comparison above is with aux_bam_to_sam; this one with '%g' itself
    vals = bits.view(np.float32)
    assert percent_g_of_arrays(text) ==",".join("%g" % float(v) for v in vals).encode()


OUT_OF_SET_BITS = (LO_BITS - 1, HI_BITS, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x007FFFFF, 0x00800000, 0x80000001, 0x7F7FFFFF, 0x38D1B717 | 0x80000000)


def out_of_set_aux(b):
    """The bit pattern as an f field, and as the second element of a B:f array."""
    return b"xff" + struct.pack("<I", b), b"xfBf" + struct.pack("<III", 2, 0x3F800000, b)


def test_floats_outside_the_set_are_odd(twin, tmp_path):
    for k, b in enumerate(OUT_OF_SET_BITS):
        for aux in out_of_set_aux(b):
            path = write_raw(str(tmp_path / ("odd_%d_%d.bam" % (k, len(aux)))), [bamio.Rec("q", 0, 0, 10, 60, [(0, 4)], -1, -1, 0, "ACGT", bytes([30] * 4), aux_bam=aux)])
            _, checks, _ = twin_text(twin, path, Results(_Empty, *[np.zeros(1, t) for t in (np.int32, np.uint32)], [np.zeros(0, np.uint32)],
                                                         np.zeros(1, np.int32), np.zeros(1, np.uint8)), 1 << 30, 30, True)
            assert [c[:2] for c in checks] == [(0, REASON["AUX_FLOAT"])], hex(b)


class _Empty:
    """A batch of one row with one CIGAR word, for the Results of a one-record file."""
    n = 1
    cig_off = np.array([0, 1], np.uint64)


# ---- the oddness rule --------------------------------------------------------------------------------------------------------------------
ODD = {
    "QNAME": [raw_record(name=b"a b\0"), raw_record(name=b"a\x7f\0"), raw_record(name=b"", l_name=0), raw_record(name=b"\xc3\xa9\0")],
    "REF": [raw_record(ref_id=3), raw_record(next_ref=3), raw_record(ref_id=2 ** 31 - 1)],
    "CIGAR_OP": [raw_record(cigar=(0x4A,)), raw_record(cigar=(0x40, 0x1F))],
    "QUAL": [raw_record(qual=b"\x1e\x5e\x1e\x1e"), raw_record(qual=b"\x00" * 3 + b"\xff"), raw_record(seq=b"\x11" * 6, qual=b"\x1e" * 11 + b"\x80")],
    "AUX_TYPE": [raw_record(aux=b"xxQ\0"), raw_record(aux=b"NMC\1xxBZ\0\0\0\0"), raw_record(aux=b"xxz\0"), raw_record(aux=b"xxBd\0\0\0\0")],
    "AUX_TRUNC": [raw_record(aux=b"xxi\1\0\0"), raw_record(aux=b"xxA"), raw_record(aux=b"xxBs\3\0\0\0\1\0\2\0\3"), raw_record(aux=b"xxZabc"),
                  raw_record(aux=b"NMC\1x"), raw_record(aux=b"NMC\1xx"), raw_record(aux=b"xxBc\xff\xff\xff\xff\1"), raw_record(aux=b"xxBi\0\0\0"),
                  raw_record(aux=b"xxH")],
    "AUX_CHAR": [raw_record(aux=b"x C\1"), raw_record(aux=b"xxA "), raw_record(aux=b"xxZa\tb\0"), raw_record(aux=b"xxHa\x80\0"), raw_record(aux=b"\x80xC\1")],
    "AUX_FLOAT": [raw_record(aux=b"xxf\0\0\xc0\x7f"), raw_record(aux=b"xxBf\1\0\0\0\0\0\x80\x7f"), raw_record(aux=b"xxf\1\0\0\0")],
}


def test_every_odd_reason_first_in_the_middle_and_last(twin, tmp_path):
    """One odd row among nine, at each place; every variant of every reason.  The check names the row and the reason, and
    amp_bam_format answers AMP_ESTATE on the piece."""
    good = [raw_record(name=b"g%d\0" % k, aux=b"NMC\1XSZok\0") for k in range(9)]
    res = Results(type("B", (), {"n": 9, "cig_off": np.arange(10, dtype=np.uint64)}), np.zeros(9, np.int32), np.ones(9, np.uint32), [np.array([0x40], np.uint32)] * 9,
                  np.full(9, 100, np.int32), np.ones(9, np.uint8))
    n = 0
    for reason, variants in ODD.items():
        for v, bad in enumerate(variants):
            for place in (0, 4, 8):
                recs = list(good)
                recs[place] = bad
                path = write_raw(str(tmp_path / ("odd_%s_%d_%d.bam" % (reason, v, place))), recs)
                text, checks, _ = twin_text(twin, path, res, 1 << 30, 30, True)
                assert checks == [(place, REASON[reason], 0)], (reason, v, place, checks)
                assert text == b""
                n += 1
    assert n == 3 * sum(len(v) for v in ODD.values())
    # the smallest odd row wins, and of one row's faults the smallest number
    path = write_raw(str(tmp_path / "two.bam"), good[:3] + [ODD["AUX_FLOAT"][0], raw_record(name=b"a b\0", cigar=(0x4A,), aux=b"xxQ\0")] + good[5:])
    assert twin_text(twin, path, res, 1 << 30, 30, True)[1] == [(3, REASON["AUX_FLOAT"], 0)]
    path = write_raw(str(tmp_path / "three.bam"), [raw_record(name=b"a b\0", cigar=(0x4A,), aux=b"x Q\0")] + good[1:])
    assert twin_text(twin, path, res, 1 << 30, 30, True)[1] == [(0, REASON["QNAME"], 0)]


def test_an_odd_record_that_is_no_row_is_not_odd(twin, tmp_path):
    """Records the loop skips (A:902) are never written and never checked: an unmapped record with a bad aux, one without a CIGAR
    and a QNAME with a blank."""
    recs = [raw_record(name=b"g0\0"), raw_record(flag=4, aux=b"xxQ\0"), raw_record(name=b"a b\0", cigar=()), raw_record(name=b"g1\0", flag=16)]
    path = write_raw(str(tmp_path / "norow.bam"), recs)
    res = Results(type("B", (), {"n": 2, "cig_off": np.arange(3, dtype=np.uint64)}), np.array([5, 6], np.int32), np.ones(2, np.uint32),
                  [np.array([0x40], np.uint32)] * 2, np.full(2, 100, np.int32), np.ones(2, np.uint8))
    text, checks, formats = twin_text(twin, path, res, 1 << 30, 30, False)
    assert checks == [(-1, 0, 0)] and formats[0].n_rows_written == 2
    assert text == b"g0\t0\tSYN_REF\t6\t60\t4M\t*\t0\t0\tACGT\t????\ng1\t16\tSYN_REF\t7\t60\t4M\t*\t0\t0\tACGT\t????\n"


def test_format_needs_a_check_results_and_room(twin, tmp_path):
    path = write_raw(str(tmp_path / "s.bam"), [raw_record(name=b"g%d\0" % k) for k in range(5)])
    src = bam_device.DeviceBamInput(path)
    c = bam_device.BamCodec(twin=twin)
    (info, st), = list(bam_device.walk(c, src))
    with pytest.raises(lib.AmpliHipError) as e:
        c.text_check()                                                   # no name table yet
    assert e.value.rc == ESTATE
    c.set_references([n for n, _ in HDR.refs])
    res = identity_results(c.batch())
    c.set_trim(res)
    with pytest.raises(lib.AmpliHipError) as e:
        c.format(1, True)                                                # results, and no check yet
    assert e.value.rc == ESTATE
    (info, st), = list(bam_device.walk(c, bam_device.DeviceBamInput(path)))
    assert c.text_check().first_odd_row == -1
    with pytest.raises(lib.AmpliHipError) as e:
        c.format(1, True)                                                # a check, and no results yet
    assert e.value.rc == ESTATE
    c.set_trim(res)
    ti = bam_device.AmpBamTextInfo()
    buf = np.zeros(64, np.uint8)
    rc = c.L.amp_bam_format(c.h, 1, 1, buf.ctypes.data_as(bam_device.C.c_void_p), bam_device.C.c_int64(10), bam_device.C.byref(ti))
    assert rc == bam_device.OVERFLOW and ti.n_bytes == 5 * len(b"g0\t0\tSYN_REF\t11\t60\t8M\t*\t0\t0\tACGT\t????\n") and not buf.any()
    text, fi = c.format(1, True)
    assert len(text) == ti.n_bytes and fi.n_rows_written == 5 and fi.waits == 2
    c.close()


# ---- under the sanitizers -------------------------------------------------------------------------------------------------------------
def test_text_under_the_sanitizers(tmp_path):
    """tests/hostsim/bamtext_fuzz.cpp: the twin as a program under -fsanitize=address,undefined (host code only), guard bytes behind
    the text buffer: random records with damaged aux among them, random results and piece cuts; every piece is odd or its text
    equals a plain serial formatter's (snprintf("%g") for floats)."""
    exe = bam_device.build_twin(str(tmp_path / "bamtext_fuzz"), sanitize=True, main_source=os.path.join(ROOT, "tests", "hostsim", "bamtext_fuzz.cpp"))
    r = subprocess.run([exe, "40"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "files 40" in r.stdout and "mismatches 0" in r.stdout and "guard hits 0" in r.stdout
    pieces, odd = [int(r.stdout.split(key)[1].split()[0].rstrip(",")) for key in ("pieces ", "odd ")]
    assert pieces > 100 and 2 * odd <= pieces


# ---- routing ----------------------------------------------------------------------------------------------------------------------------
def test_routing_accepts_exactly_the_runs_of_section_14(tmp_path, monkeypatch):
    """open_device_bam_text: an existing .bam in (AMPLIPY_PYTHON_BAM unset), stdout with a .buffer or a new .sam file out, a header of
    ASCII text whose @SQ names fit the device's table -- and None for every other run, which the other codecs serve or refuse."""
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    monkeypatch.delenv("AMPLIPY_PYTHON_BAM", raising=False)
    recs = [bamio.Rec("r%d" % i, 0, 0, 10 + i, 60, [(0, 8)], -1, -1, 0, "ACGTACGT", bytes([30] * 8)) for i in range(20)]
    inp = write_raw(str(tmp_path / "in.bam"), recs)
    upper = write_raw(str(tmp_path / "IN2.BAM"), recs)
    opened = []

    def go(i, o):
        r = amplipy.open_device_bam_text(i, o)
        if r is not None:
            opened.append(r)
            r[1]._f.flush()
        return r
    # the runs it takes
    out = str(tmp_path / "new.sam")
    src, writer, outb = go(inp, out)
    outb.close()
    want_hdr = HDR.with_amplipy_pg(amplipy.VERSION, "amplipy_amd pinned").text
    assert open(out).read() == want_hdr and isinstance(src, bam_device.DeviceBamInput) and src.path == inp
    src, writer, outb = go(upper, str(tmp_path / "NEW2.SAM"))
    outb.close()
    fake = io.TextIOWrapper(io.BytesIO(), write_through=True)
    monkeypatch.setattr(sys, "stdout", fake)
    src, writer, outb = go(inp, "stdout")
    assert outb is fake.buffer and fake.buffer.getvalue().decode() == want_hdr
    src, writer, outb = go(inp, "STDOUT")
    assert outb is fake.buffer
    # ... and the runs it leaves alone
    monkeypatch.setattr(sys, "stdout", io.StringIO())                    # no .buffer
    assert go(inp, "stdout") is None
    monkeypatch.undo()
    monkeypatch.setattr(sys, "argv", ["amplipy_amd", "pinned"])
    sam_in = str(tmp_path / "in.sam")
    open(sam_in, "w").write(HDR.text)
    fresh = iter(str(tmp_path / ("o%d.sam" % k)) for k in range(100))
    for i in (None, "stdin", "STDIN", str(tmp_path / "missing.bam"), sam_in):
        assert go(i, next(fresh)) is None
    for o in (None, str(tmp_path / "o.bam"), out, str(tmp_path / "o.txt"), str(tmp_path / "o.sam.gz"), str(tmp_path / "o")):
        assert go(inp, o) is None
    monkeypatch.setenv("AMPLIPY_PYTHON_BAM", "1")
    assert go(inp, next(fresh)) is None
    monkeypatch.delenv("AMPLIPY_PYTHON_BAM")
    not_bam = str(tmp_path / "text.bam")
    open(not_bam, "w").write("not a BAM file\n")
    assert go(not_bam, next(fresh)) is None
    # headers the device's name table cannot take, or whose text is not ASCII
    def with_refs(tag, refs, text=None):
        text = text or "@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:sim\n"
        return write_raw(str(tmp_path / (tag + ".bam")), recs if refs else [], bamio.Header(text, refs))
    many = [("c%d" % k, 100) for k in range(65)]
    assert go(with_refs("r65", many), next(fresh)) is None
    assert go(with_refs("r64", many[:64]), next(fresh)) is not None
    assert go(with_refs("rlong", [("x" * 2049, 5), ("y" * 2048, 5)]), next(fresh)) is None
    assert go(with_refs("rfits", [("x" * 2048, 5), ("y" * 2048, 5)]), next(fresh)) is not None
    for k, name in enumerate(("*", "=", "a b", "caf\x7f")):
        assert go(with_refs("rname%d" % k, [(name, 100)]), next(fresh)) is None
    assert go(with_refs("utf8", [("ok", 100)], "@HD\tVN:1.6\n@SQ\tSN:ok\tLN:100\n@CO\tcafé\n@PG\tID:sim\n"), next(fresh)) is None
    assert go(with_refs("norefs", []), next(fresh)) is not None
    # a header without @PG raises what the Python codec raises -- unless that codec would refuse the output first
    nopg = with_refs("nopg", [("ok", 100)], "@HD\tVN:1.6\n@SQ\tSN:ok\tLN:100\n")
    with pytest.raises(KeyError):
        go(nopg, next(fresh))
    assert go(nopg, out) is None
    made = [p for p in os.listdir(str(tmp_path)) if p.startswith("o") and p.endswith(".sam")]
    assert len(made) == 3                                               # only the three runs it took here made a file
    for r in opened:
        if not r[2].closed and r[2] is not fake.buffer:
            r[2].close()
