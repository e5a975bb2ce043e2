"""SAM text through the device codec of libamplihip.so (amp_sam_*, amplipy_amd/csrc/amp_sam.hip).

Opt-in (AMPLIPY_GPU_SAM=1 or run_amplipy(gpu_sam=True)): chunks of text go to the device, a packed batch is built there, the read
pass runs on it and the kept lines of a trimmed output come back as text -- no per-read Python object.  A chunk with a line
the device codec calls odd (one the Python codec might not give back byte for byte, or raises on) is handed to the Python codec
of ``bamio`` instead, so whatever that does with the line still happens.  With AMPLIPY_GPU_BAM_WRITE=1 (gpu_bam_write=True) as well
and a new .bam file as the trimmed output, the kept rows leave the device as framed BGZF blocks of BAM
records instead (``SamCodec.encode``), and the records the Python codec makes of an odd chunk go through the same stream
(``SamCodec.encode_bytes``).

``SamCodec`` binds the C entry points; it also drives the host twin of the kernels (the same lane functions compiled with
-DAMPSAM_HOSTSIM, ``build_twin``), which is how the codec is checked without a GPU.
"""
from __future__ import annotations

import ctypes as C
import io
import os
import sys

import numpy as np

from . import abi, devcodec

CHUNK_BYTES = 16 << 20             # text per device chunk (AMPLIPY_SAM_CHUNK_BYTES): see the sweep in DESIGN.md section 10
N_STAGES = 15                      # AMP_SAM_N_STAGES
OUT_TEXT, OUT_BAM = 0, 1           # AMP_SAM_OUT_*

ODD_REASONS = {0: "NONE", 1: "BYTE", 2: "INT", 3: "RANGE", 4: "RNAME", 5: "RNEXT", 6: "CIGAR", 7: "CIGAR_LEN", 8: "EMPTY",
               9: "QUAL_NO_SEQ", 10: "QUAL_LEN", 11: "QUAL_CHAR", 12: "LINES",
               # with BAM output only
               13: "QNAME", 14: "AUX_TAG", 15: "AUX_A", 16: "AUX_INT", 17: "AUX_INT_RANGE", 18: "AUX_B", 19: "AUX_B_RANGE", 20: "AUX_FLOAT",
               21: "CIGAR_OPS"}

# chunks of the last run of run_amplipy that took this path: by the device, and by the Python codec (odd chunks)
LAST_RUN_STATS = {"device_chunks": 0, "python_chunks": 0, "records": 0,
                  # a run that writes trimmed reads as BAM through amp_sam_encode (section 13): blocks made on the device / compressed
                  # by the host, rows the device encoded, device-to-host bytes, bytes of the file's record blocks, encodes, their waits
                  "out_blocks_device": 0, "out_blocks_host": 0, "out_rows": 0, "bytes_down": 0, "bytes_out_file": 0, "encodes": 0, "waits": 0}
OUT_STATS = ("out_blocks_device", "out_blocks_host", "out_rows", "bytes_down", "bytes_out_file", "encodes", "waits")


def zeroed_stats():
    """The keys of LAST_RUN_STATS, all zero: a run's totals before its first chunk."""
    return dict.fromkeys(LAST_RUN_STATS, 0)


class AmpSamInfo(C.Structure):
    _fields_ = [("n_lines", C.c_int64), ("n_records", C.c_int64), ("n_rows", C.c_int64), ("n_cig", C.c_int64),
                ("n_bases", C.c_int64), ("n_bases_padded", C.c_int64), ("first_odd_line", C.c_int64),
                ("odd_reason", C.c_int32), ("reserved", C.c_int32)]


def twin_sources():
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(here, "csrc", "amp_sam.hip"), os.path.join(here, "..", "include", "amplihip.h")


def build_twin(out_path, sanitize=False, main_source=None):
    """The kernels' lane functions and a driver that runs them lane after lane, compiled for the host (no HIP needed):
    a shared library with the amp_sam_* entry points (amp_sam_twin_set_results in place of amp_sam_process), or, with
    ``main_source``, a program around them.  sanitize: -fsanitize=address,undefined (host code only)."""
    return devcodec.build_twin(twin_sources()[0], "AMPSAM_HOSTSIM", out_path, sanitize, main_source)


class SamCodec(devcodec.DeviceCodec):
    """One amp_sam: on the device of ``engine`` (lib.Engine), or the host twin when ``twin`` is the path of its library."""

    def __init__(self, engine=None, twin=None):
        super().__init__("amp_sam", N_STAGES, engine, twin)
        self._out = np.zeros(1 << 16, np.uint8)

    def parse(self, text):
        """amp_sam_parse on bytes (whole lines): AmpSamInfo."""
        info = AmpSamInfo()
        buf = (C.c_char * len(text)).from_buffer_copy(text) if isinstance(text, (bytearray, memoryview)) else text
        self._chk(self.L.amp_sam_parse(self.h, buf, C.c_int64(len(text)), C.byref(info)), "amp_sam_parse")
        self.info = info
        return info

    def batch(self):
        """The batch of the last parse as a host ReadBatch (src_index = the rows' records)."""
        return super().batch(slack=0)[0]

    def twin_set_results(self, res):
        """(twin) the results the format stage works from: an abi.TrimResult-like of this batch's rows."""
        bad = C.c_int64(-1); st = C.c_uint8(0)
        arrs = [np.ascontiguousarray(x) for x in (res.new_pos, res.new_ncig, res.new_cig, res.ref_len, res.trim_flags, res.status)]
        self._chk(self.L.amp_sam_twin_set_results(self.h, *[C.c_void_p(abi.ptr(x)) for x in arrs], C.byref(bad), C.byref(st)),
                  "amp_sam_twin_set_results")
        return int(bad.value), int(st.value)

    def set_output(self, mode):
        """amp_sam_set_output: OUT_TEXT (the default) or OUT_BAM, before the first parse."""
        self._chk(self.L.amp_sam_set_output(self.h, C.c_int32(mode)), "amp_sam_set_output")

    def process(self, read_base=0, defer=False):
        """amp_sam_process.  defer: the pass is enqueued and nothing waited for -- ``encode`` (or ``verdict``) brings the first failing
        row down; returns None then."""
        if not defer:
            return super().process(read_base)
        self._chk(self.L.amp_sam_process(self.h, C.c_uint64(read_base), None, None), "amp_sam_process")
        self.first_bad = None
        return None

    def verdict(self):
        """amp_sam_first_bad: (first row with a non-zero status or -1, that status) of the last process, deferred or not."""
        bad = C.c_int64(-1); st = C.c_uint8(0)
        self._chk(self.L.amp_sam_first_bad(self.h, C.byref(bad), C.byref(st)), "amp_sam_first_bad")
        self.first_bad = int(bad.value)
        return int(bad.value), int(st.value)

    def waits(self):
        """Waits for the device since the codec was made."""
        self.L.amp_sam_waits.restype = C.c_int64
        return int(self.L.amp_sam_waits(self.h))

    def encode(self, min_length, include_no_primer, final=False):
        """amp_sam_encode + amp_sam_encoded_to_host: (the BGZF blocks of this call as they go into the file, info) -- the kept rows of
        the last parse (A:910) as BAM records behind what the call before left over; final: the last partial block too.  Same
        shape as bam_device.BamCodec.encode, the stored-block fallback included."""
        info = devcodec.AmpBamOutInfo()
        self._chk(self.L.amp_sam_encode(self.h, C.c_int32(int(min_length)), C.c_int32(1 if include_no_primer else 0), C.c_int32(1 if final else 0),
                                        C.byref(info)), "amp_sam_encode")
        return self._encoded(info)

    def encode_bytes(self, data, final=False):
        """amp_sam_encode_bytes: BAM record bytes made on the host (a chunk that went through the Python codec) through the same
        stream; (blocks, info) as ``encode``."""
        info = devcodec.AmpBamOutInfo()
        data = bytes(data)
        self._chk(self.L.amp_sam_encode_bytes(self.h, data, C.c_int64(len(data)), C.c_int32(1 if final else 0), C.byref(info)), "amp_sam_encode_bytes")
        return self._encoded(info)

    def format(self, min_length, include_no_primer):
        """amp_sam_format: (bytes of the kept lines, their number)."""
        nb = C.c_int64(0); nr = C.c_int64(0)
        for _ in range(2):
            rc = self.L.amp_sam_format(self.h, C.c_int32(min_length), C.c_int32(1 if include_no_primer else 0),
                                       C.c_void_p(abi.ptr(self._out)), C.c_int64(self._out.size), C.byref(nb), C.byref(nr))
            if rc != -6:
                break
            self._out = np.zeros(int(nb.value) + (int(nb.value) >> 2) + 4096, np.uint8)
        self._chk(rc, "amp_sam_format")
        return self._out[:int(nb.value)].tobytes(), int(nr.value)


# ---- the run's input -----------------------------------------------------------------------------------------------------------
def decode_text(raw):
    """Bytes -> str the way the text-mode reader of bamio does it: default encoding, universal newlines."""
    return io.TextIOWrapper(io.BytesIO(raw)).read()


class SamTextInput:
    """A SAM file or stdin read as bytes: the header lines, then chunks of about ``chunk_bytes`` cut behind their last newline
    (a final line without one is completed), read one chunk ahead of the consumer on a helper thread."""

    def __init__(self, path, chunk_bytes=None):
        self.chunk_bytes = int(chunk_bytes or os.environ.get("AMPLIPY_SAM_CHUNK_BYTES", CHUNK_BYTES))
        self._f = sys.stdin.buffer if path == "-" else open(path, "rb")
        head = []
        self._carry = b""
        while True:
            line = self._f.readline()
            if not line:
                break
            if not line.startswith(b"@"):
                self._carry = line
                break
            head.append(line)
        self.header_raw = b"".join(head)

    def header_is_plain(self):
        """True when the header is ASCII with LF / CRLF line ends only: what the device path takes the @SQ names from."""
        h = self.header_raw.replace(b"\r\n", b"\n")
        return b"\r" not in h and all(c < 128 for c in h)

    def header_text(self):
        text = decode_text(self.header_raw)
        return text if text.endswith("\n") or not text else text + "\n"

    def _chunks(self):
        buf = self._carry
        self._carry = b""
        while True:
            more = self._f.read(self.chunk_bytes)
            if not more:
                break
            buf += more
            cut = buf.rfind(b"\n") + 1
            if cut:
                yield buf[:cut]
                buf = buf[cut:]
        if buf:
            yield buf + b"\n"

    def __iter__(self):
        return devcodec.read_ahead(self._chunks())

    def close(self):
        if self._f is not sys.stdin.buffer:
            self._f.close()
