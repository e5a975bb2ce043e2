"""BAM input through the device codec of libamplihip.so (amp_bam_*, amplipy_amd/csrc/amp_bgzf.hip),
trimmed BAM output from it (amp_bam_encode, amplipy_amd/csrc/amp_bamout.hip; section 12) and trimmed SAM text from it
(amp_bam_text_check / amp_bam_format, amplipy_amd/csrc/amp_bamtext.hip; section 14: AMPLIPY_GPU_SAM=1 as well, and stdout or a
new .sam file out).

Opt-in (AMPLIPY_GPU_BAM=1 or run_amplipy(gpu_bam=True)), for single-process runs that read an existing BAM file and write no
trimmed reads -- or, with AMPLIPY_GPU_BAM_WRITE=1 / gpu_bam_write=True as well, a new trimmed BAM file, whose records are
re-encoded, compressed and framed on the device too: the file is walked in pieces of whole BGZF blocks, the COMPRESSED bytes of a piece and its block table go to
the device, and inflate, CRC check, record index and decode into the packed batch all happen there; the read pass runs on
the batch where it lies.  A block the device refuses is inflated here (zlib), checked and patched in, and counted.

``BamCodec`` binds the C entry points; it also drives the host twin of the kernels (the same lane functions compiled with
-DAMPBGZF_HOSTSIM, ``build_twin``), which is how the codec is checked without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import abi, bam_native, devcodec

# Compressed bytes of a piece (AMPLIPY_GPU_BAM_PIECE_BYTES).  A CU holds twelve decoders (13,344 bytes of LDS each), the chip
# 3,072; a BGZF block of an amplicon BAM is 8-10 KB compressed, so 16 MB are about 1,800 blocks: one wave of work for more
# than half of the decoders, while the image (6.8 x: 110 MB) and everything sized by it (about 6 x the image) stay below a
# GB.  The sweep of tools/time_gpu_bam.py is in DESIGN.md section 11.
PIECE_BYTES = 16 << 20
IMAGE_LIMIT = 256 << 20            # AMP_BAM_IMAGE_LIMIT of amplihip.h
PIECE_ISIZE_LIMIT = 120 << 20      # ISIZE sum of a piece: with a carry of at most one record (2^27 + 4 bytes) the image fits
N_STAGES = 16                      # AMP_BAM_N_STAGES
OUT_BS = devcodec.OUT_BS
FORMAT_ERROR = -3                  # AMPBAM_EFORMAT

# the last run of run_amplipy that took this path
LAST_RUN_STATS = {"pieces": 0, "blocks_device": 0, "blocks_host": 0, "index_rounds": 0, "waits": 0, "records": 0,
                  "bytes_up": 0, "bytes_file": 0,
                  # a run that writes trimmed reads through amp_bam_encode (section 12)
                  "out_blocks_device": 0, "out_blocks_host": 0, "out_rows": 0, "bytes_down": 0, "bytes_out_file": 0,
                  # a run that writes trimmed reads as SAM text through amp_bam_format (section 14)
                  "text_pieces_device": 0, "text_pieces_python": 0, "text_rows": 0, "text_bytes": 0}
OUT_STATS = ("out_blocks_device", "out_blocks_host", "out_rows", "bytes_down", "bytes_out_file")
TEXT_STATS = ("text_pieces_device", "text_pieces_python", "text_rows", "text_bytes")
ODD_REASONS = ("NONE", "QNAME", "REF", "CIGAR_OP", "QUAL", "AUX_TYPE", "AUX_TRUNC", "AUX_CHAR", "AUX_FLOAT")       # AMP_BAM_ODD_*
OVERFLOW = -6                      # AMP_EOVERFLOW


def zeroed_stats():
    """The keys of LAST_RUN_STATS, all zero: a run's totals before its first piece."""
    return dict.fromkeys(LAST_RUN_STATS, 0)


class AmpBamBlock(C.Structure):
    _fields_ = [("in_off", C.c_uint32), ("in_len", C.c_uint32), ("out_len", C.c_uint32), ("crc", C.c_uint32)]


class AmpBamInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_blocks", "n_inflated", "image_bytes", "carry_in", "carry_out", "next_first", "n_records",
                                         "n_rows", "n_cig", "n_bases", "n_bases_padded", "n_refused", "index_rounds", "waits",
                                         "bytes_up")] + [("bad_record", C.c_int32), ("reserved", C.c_int32)]


class AmpBamTextInfo(C.Structure):
    _fields_ = [("first_odd_row", C.c_int64), ("odd_reason", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_int64) for n in ("n_rows_written", "n_bytes", "waits", "bytes_down")]


AmpBamOutInfo, TWIN_DEFLATE_FN, bgzf_block = devcodec.AmpBamOutInfo, devcodec.TWIN_DEFLATE_FN, devcodec.bgzf_block


def twin_sources():
    """amp_bgzf.hip (which includes amp_bamout.hip, the re-encoder's lanes and driver, and amp_bamtext.hip, the text stage's) and the
    lane functions' headers."""
    here = os.path.dirname(os.path.abspath(__file__))
    return tuple(os.path.join(here, "csrc", f) for f in ("amp_bgzf.hip", "amp_bgzf.hpp", "amp_bamout.hip", "amp_bamout.hpp", "amp_bamtext.hip", "amp_bamtext.hpp"))


def build_twin(out_path, sanitize=False, main_source=None):
    """The kernels' lane functions and a driver that runs them lane after lane, compiled for the host (no HIP needed): a shared
    library with the amp_bam_* entry points (without amp_bam_process), or, with ``main_source``, a program around the lane
    functions.  sanitize: -fsanitize=address,undefined (host code only)."""
    return devcodec.build_twin(twin_sources()[0], "AMPBGZF_HOSTSIM", out_path, sanitize, main_source)


def format_error(path):
    """What bam_native.BamFile raises for a file that is not a valid BGZF / BAM stream."""
    return bam_native.AmpBamError("%s: %s" % (path, bam_native.load().ampbam_strerror(FORMAT_ERROR).decode()))


def block_table(path):
    """ampbam_block_table: an (n, 4) uint64 array -- file offset and length of every block's raw DEFLATE stream, ISIZE, CRC-32.
    Raises what bam_native.BamFile raises for a file whose block headers are not BGZF."""
    L = bam_native.load()
    n = int(L.ampbam_block_table(os.fsencode(path), None, 0))
    if n < 0:
        raise bam_native.AmpBamError("%s: %s" % (path, L.ampbam_strerror(int(n)).decode()))
    tab = np.zeros((n, 4), np.uint64)
    m = int(L.ampbam_block_table(os.fsencode(path), C.c_void_p(tab.ctypes.data), n))
    if m != n:
        raise format_error(path)
    return tab


def read_header(path, table):
    """(header text, [(name, length)], offset of the first record in the inflated stream) from the file's first blocks, as
    libampbam reads them (the text without trailing NULs).  The offset follows from the header's own length fields."""
    have = bytearray()
    k = 0

    def need(upto):
        nonlocal k
        with open(path, "rb") as f:
            while len(have) < upto:
                if k >= len(table):
                    raise format_error(path)
                off, ln, isize, crc = (int(x) for x in table[k])
                k += 1
                f.seek(off)
                raw = f.read(ln)
                try:
                    out = zlib.decompress(raw, -15) if isize else b""
                except zlib.error:
                    raise format_error(path)
                if len(out) != isize or (isize and (zlib.crc32(out) & 0xFFFFFFFF) != crc):
                    raise format_error(path)
                have.extend(out)
    need(12)
    if bytes(have[:4]) != b"BAM\1":
        raise format_error(path)
    l_text = struct.unpack_from("<I", have, 4)[0]
    need(12 + l_text)
    text = bytes(have[8:8 + l_text]).rstrip(b"\0").decode("ascii", "replace")
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", have, o)[0]
    o += 4
    if n_ref < 0:
        raise format_error(path)
    refs = []
    for _ in range(n_ref):
        need(o + 4)
        l_name = struct.unpack_from("<I", have, o)[0]
        o += 4
        if l_name == 0:
            raise format_error(path)
        need(o + l_name + 4)
        refs.append((bytes(have[o:o + l_name - 1]).decode("ascii"), struct.unpack_from("<i", have, o + l_name)[0]))
        o += l_name + 4
    return text, refs, o


def cut_pieces(table, piece_bytes):
    """[(k_lo, k_hi)]: runs of whole blocks of about piece_bytes compressed bytes whose ISIZE sum stays below PIECE_ISIZE_LIMIT."""
    pieces = []
    n = len(table)
    k = 0
    while k < n:
        lo = k
        comp = isize = 0
        while k < n and (k == lo or (comp + int(table[k, 1]) + 26 <= piece_bytes and isize + int(table[k, 2]) <= PIECE_ISIZE_LIMIT)):
            comp += int(table[k, 1]) + 26
            isize += int(table[k, 2])
            k += 1
        pieces.append((lo, k))
    return pieces


class BamCodec(devcodec.DeviceCodec):
    """One amp_bam: on the device of ``engine`` (lib.Engine), or the host twin when ``twin`` is the path of its library."""

    def __init__(self, engine=None, twin=None):
        super().__init__("amp_bam", N_STAGES, engine, twin)

    def feed(self, comp, blocks, first_off, n_ref, rec_base=0):
        """amp_bam_feed: comp = the piece's bytes (numpy uint8 or bytes), blocks = (n, 4) array of in_off (relative to comp), in_len,
        ISIZE, CRC.  first_off None: the image starts with the carry of the piece before."""
        comp = np.frombuffer(comp, np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, np.uint8)
        tab = np.ascontiguousarray(np.asarray(blocks, np.uint64).reshape(-1, 4).astype(np.uint32))
        info = AmpBamInfo()
        rc = self.L.amp_bam_feed(self.h, C.c_void_p(abi.ptr(comp)), C.c_int64(comp.size), C.c_void_p(abi.ptr(tab)), C.c_int64(tab.shape[0]),
                                 C.c_int64(-1 if first_off is None else int(first_off)), C.c_int32(n_ref), C.c_int64(rec_base), C.byref(info))
        if rc == -6:
            raise bam_native.AmpBamError("AMPLIPY_GPU_BAM: a piece's image (carry + inflated blocks) would pass %d bytes" % IMAGE_LIMIT)
        self._chk(rc, "amp_bam_feed")
        self.info = info
        self._blocks = tab
        self._comp = comp
        return info

    def dev_refuse(self, k):
        self._chk(self.L.amp_bam_dev_refuse(self.h, C.c_int64(k)), "amp_bam_dev_refuse")

    def refused(self):
        n = C.c_int64(0)
        idx = np.zeros(max(int(self.info.n_refused), 1), np.int64)
        self._chk(self.L.amp_bam_refused(self.h, C.c_void_p(abi.ptr(idx)), C.c_int64(idx.size), C.byref(n)), "amp_bam_refused")
        return [int(x) for x in idx[:int(n.value)]]

    def verdicts(self):
        """amp_bam_verdicts: one byte per block of the last feed -- 0 accepted, 1 refused by the decoder, 2 by the CRC check."""
        v = np.zeros(max(int(self.info.n_blocks), 1), np.uint8)
        self._chk(self.L.amp_bam_verdicts(self.h, C.c_void_p(abi.ptr(v)), C.c_int64(v.size)), "amp_bam_verdicts")
        return v[:int(self.info.n_blocks)]

    def patch_through_host(self, comp=None, blocks=None):
        """Every refused block of the last feed through the host's inflate and CRC check: the number of blocks patched, or None
        when one of them is damaged (the caller raises what the host codec raises for the file).  Then the index again.
        comp, blocks: the host reads these instead of what was fed (same block count and ISIZEs; tests)."""
        if comp is None:
            comp, blocks = self._comp, self._blocks
        else:
            comp, blocks = np.frombuffer(comp, np.uint8), np.asarray(blocks, np.uint64).reshape(-1, 4)
        n = 0
        for k in self.refused():
            off, ln, isize, crc = (int(x) for x in blocks[k])
            out = b""
            if isize:
                try:
                    out = zlib.decompress(comp[off:off + ln].tobytes(), -15)
                except zlib.error:
                    return None
                if len(out) != isize or (zlib.crc32(out) & 0xFFFFFFFF) != crc:
                    return None
            buf = np.frombuffer(out, np.uint8) if out else np.zeros(1, np.uint8)
            self._chk(self.L.amp_bam_patch_block(self.h, C.c_int64(k), C.c_void_p(abi.ptr(buf)), C.c_int64(len(out))), "amp_bam_patch_block")
            n += 1
        info = AmpBamInfo()
        self._chk(self.L.amp_bam_reindex(self.h, C.byref(info)), "amp_bam_reindex")
        self.info = info
        return n

    def batch(self, slack=False):
        """The batch of the last feed as a host ReadBatch (src_index = the rows' record numbers).  slack: (the batch, the 16 spare
        bytes behind cig, seq and qual as three arrays) -- the tests check that they are zero like ampbam_decode's."""
        rb, tails = super().batch(slack=16)
        return (rb, tails) if slack else rb

    def set_trim(self, res, first_bad=-1):
        """Twin only (it has no read pass): the results of the last feed's rows -- new_pos, new_ncig, new_cig (row r's words at
        cig_off[r] + 3 r), ref_len, trim_flags as a lib.TrimResult holds them -- for the encode that follows."""
        self._trim = [np.ascontiguousarray(a, t) for a, t in ((res.new_pos, np.int32), (res.new_ncig, np.uint32), (res.new_cig, np.uint32),
                                                              (res.ref_len, np.int32), (res.trim_flags, np.uint8))]
        self._chk(self.L.amp_bam_twin_set_trim(self.h, *[C.c_void_p(abi.ptr(a)) for a in self._trim], C.c_int64(first_bad)), "amp_bam_twin_set_trim")

    def encode(self, min_length, include_no_primer, final=False):
        """amp_bam_encode + amp_bam_encoded_to_host: (the BGZF blocks of this call as they go into the file, info).  The kept rows
        of the last feed (A:910), behind what the call before left over; final: the last partial block too.  A block whose
        stream did not fit comes down raw and is compressed here (info.n_blocks_host counts it; never on real data)."""
        info = AmpBamOutInfo()
        rc = self.L.amp_bam_encode(self.h, C.c_int32(int(min_length)), C.c_int32(1 if include_no_primer else 0), C.c_int32(1 if final else 0), C.byref(info))
        if rc == -1:
            raise bam_native.AmpBamError("write: %s" % bam_native.load().ampbam_strerror(-1).decode())      # (what ampbam_write_rows answers)
        self._chk(rc, "amp_bam_encode")
        return self._encoded(info)

    # ---- trimmed reads as SAM text (section 14) ----------------------------------------------------------------------------------
    def text_check(self):
        """amp_bam_text_check behind a feed whose index stands: the info (first_odd_row -1: the device formats the piece)."""
        info = AmpBamTextInfo()
        self._chk(self.L.amp_bam_text_check(self.h, C.byref(info)), "amp_bam_text_check")
        self.text_info = info
        return info

    def format(self, min_length, include_no_primer):
        """amp_bam_format: (the lines of the kept rows of the last feed as bytes, info).  The buffer it copies into is kept; when it
        is short the call names the size, the buffer grows and the call is made again (info.waits has the wait of the short try
        too, ``self.text_retries`` counts them: pieces of a run have one size, so the first pieces at most)."""
        info = AmpBamTextInfo()
        room = max(2 * int(self.info.image_bytes), 1 << 16)             # (a line is at most about twice its record)
        if getattr(self, "_text", None) is None or self._text.size < room:
            self._text = np.empty(room, np.uint8)

        def call():
            return self.L.amp_bam_format(self.h, C.c_int32(int(min_length)), C.c_int32(1 if include_no_primer else 0),
                                         C.c_void_p(abi.ptr(self._text)), C.c_int64(self._text.size), C.byref(info))
        rc = call()
        waits = 0
        if rc == OVERFLOW and info.n_bytes < (1 << 32):
            waits = int(info.waits)
            self.text_retries = getattr(self, "text_retries", 0) + 1
            self._text = np.empty(int(info.n_bytes) + int(info.n_bytes) // 4, np.uint8)
            rc = call()
        self._chk(rc, "amp_bam_format")
        info.waits += waits
        self.text_info = info
        return self._text[:int(info.n_bytes)].tobytes(), info

    def image(self):
        """(the image of the last feed, the offsets of its records in it)."""
        img = np.zeros(max(int(self.info.image_bytes), 1), np.uint8)
        off = np.zeros(max(int(self.info.n_records), 1), np.uint32)
        self._chk(self.L.amp_bam_image_to_host(self.h, C.c_void_p(abi.ptr(img)), C.c_int64(img.size), C.c_void_p(abi.ptr(off)), C.c_int64(off.size)),
                  "amp_bam_image_to_host")
        return img[:int(self.info.image_bytes)], off[:int(self.info.n_records)]


class DeviceBamInput:
    """A BAM file as a sequence of pieces of whole BGZF blocks: (compressed bytes, block table relative to them, is it the last),
    read one piece ahead of the consumer on a helper thread.  Header text, references and the offset of the first record are
    read from the first blocks when the input is made."""

    def __init__(self, path, piece_bytes=None):
        self.path = path
        self.piece_bytes = max(1, int(piece_bytes or os.environ.get("AMPLIPY_GPU_BAM_PIECE_BYTES", PIECE_BYTES)))
        self.table = block_table(path)
        self.header_text, self.references, self.first_record = read_header(path, self.table)
        self.pieces = cut_pieces(self.table, self.piece_bytes)
        self.file_bytes = os.path.getsize(path)

    def _read(self):
        with open(self.path, "rb") as f:
            for n, (lo, hi) in enumerate(self.pieces):
                start = int(self.table[lo, 0])
                end = int(self.table[hi - 1, 0] + self.table[hi - 1, 1])
                comp = np.empty(end - start, np.uint8)
                f.seek(start)
                if f.readinto(memoryview(comp)) != comp.size:
                    raise bam_native.AmpBamError("%s: %s" % (self.path, bam_native.load().ampbam_strerror(-2).decode()))
                tab = self.table[lo:hi].copy()
                tab[:, 0] -= np.uint64(start)
                yield comp, tab, lo, n + 1 == len(self.pieces)

    def __iter__(self):
        return devcodec.read_ahead(self._read())


def walk(codec, src, refuse_block=None):
    """Feeds the pieces of ``src`` (DeviceBamInput) to ``codec`` and yields (info, stats) per piece once its index stands: refused
    blocks went through the host (counted), a damaged block or record raised what the host codec raises for the file.
    stats = the running totals (the keys of LAST_RUN_STATS).  refuse_block: development only -- that block of the file is
    treated as refused."""
    stats = zeroed_stats()
    stats["bytes_file"] = src.file_bytes
    n_ref = len(src.references)
    first = src.first_record
    for comp, tab, k_lo, last in src:
        if refuse_block is not None and k_lo <= refuse_block < k_lo + len(tab):
            codec.dev_refuse(refuse_block - k_lo)
        info = codec.feed(comp, tab, first, n_ref, rec_base=stats["records"])
        stats["bytes_up"] += int(info.bytes_up)
        n_host = 0
        if info.n_refused:
            n_host = codec.patch_through_host()
            if n_host is None:
                raise format_error(src.path)
            info = codec.info
        if info.bad_record:
            raise format_error(src.path)
        first = int(info.next_first) if info.next_first > 0 else None
        if last and (info.carry_out or info.next_first > 0):
            raise format_error(src.path)           # the file ends inside a record (or inside its header)
        stats["pieces"] += 1
        stats["blocks_device"] += int(info.n_blocks) - n_host
        stats["blocks_host"] += n_host
        stats["index_rounds"] += int(info.index_rounds)
        stats["waits"] += int(info.waits)
        stats["records"] += int(info.n_records)
        yield info, stats


class DeviceBamOutput:
    """The trimmed BAM of a run whose reads an amp_bam holds (section 12): header blocks and end-of-file block from the host codec
    (bam_native.BamWriter on the header alone), everything between them from ``codec.encode``.  ``stats``: the running totals of
    ``walk``, whose output keys and waits are counted up here."""

    def __init__(self, path, header_text, references, level=-1):
        self.writer = bam_native.BamWriter(path, header_text, None, level=level, references=references)
        self.path = path

    def encode(self, codec, stats, min_length, include_no_primer, final=False):
        return self._append(stats, *codec.encode(min_length, include_no_primer, final))

    def encode_bytes(self, codec, stats, data, final=False):
        """Record bytes made on the host through the same stream (sam_native.SamCodec.encode_bytes)."""
        return self._append(stats, *codec.encode_bytes(data, final))

    def _append(self, stats, blocks, info):
        self.writer.append_framed(blocks)
        stats["out_blocks_device"] += int(info.n_blocks) - int(info.n_blocks_host)
        stats["out_blocks_host"] += int(info.n_blocks_host)
        stats["out_rows"] += int(info.n_rows_written)
        stats["bytes_down"] += int(info.bytes_down)
        stats["bytes_out_file"] += int(blocks.size)
        stats["waits"] += int(info.waits)
        return info

    def close(self):
        self.writer.close()
