"""What the device codecs of libamplihip.so share on the Python side (sam_native / amp_sam_*, bam_device / amp_bam_*; the C
half is amplipy_amd/csrc/amp_codec.hpp and, for trimmed BAM out of either codec, amp_bamtail.hpp): the binding of the entry points
every codec has, the build of a host twin, and the thread that reads one piece ahead of the consumer."""
from __future__ import annotations

import ctypes as C
import os
import queue
import shutil
import struct
import subprocess
import threading
import zlib

import numpy as np

from . import abi
from .batch import ReadBatch


OUT_BS = 0xFF00                    # uncompressed bytes of a BGZF block of the trimmed output (the host writer's)
MAX_REFS = 64                      # AMP_SAM_MAX_REFS / AMP_SAM_MAX_REF_BYTES of amplihip.h: the name table of amp_*_set_references
MAX_REF_BYTES = 4096


def names_fit(names):
    """Can the device's name table take these reference names: at most MAX_REFS of them and MAX_REF_BYTES bytes, each printable
    ASCII without a blank and none of "", "*", "=" (what RNAME / RNEXT mean something else by)."""
    return len(names) <= MAX_REFS and sum(len(n) for n in names) <= MAX_REF_BYTES \
        and all(n not in ("", "*", "=") and all(33 <= ord(c) < 127 for c in n) for n in names)


class AmpBamOutInfo(C.Structure):
    """amp_bam_out_info: what amp_bam_encode and amp_sam_encode answer."""
    _fields_ = [(n, C.c_int64) for n in ("n_rows_written", "stream_bytes", "carry_in", "carry_out", "n_blocks", "file_bytes", "n_blocks_host",
                                         "waits", "bytes_down")]


# amp_bam_twin_deflate_fn of amp_bamout.hpp
TWIN_DEFLATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_uint32))


def bgzf_block(data, level=6):
    """One BGZF block of ``data`` (at most 0xFF00 bytes) made on the host: zlib's stream, the framing of flush_blocks."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def build_twin(source, define, out_path, sanitize=False, main_source=None):
    """``source``'s lane functions and a driver that runs them lane after lane, compiled for the host with -D``define`` (no HIP
    needed): a shared library with the codec's entry points, or, with ``main_source``, a program around them.
    sanitize: -fsanitize=address,undefined (host code only)."""
    cmd = [shutil.which("g++") or "g++", "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
           "-D" + define]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if main_source is None:
        cmd += ["-fPIC", "-shared", "-o", out_path, source]
    else:
        cmd += ["-I", os.path.dirname(source), "-o", out_path, main_source]
    subprocess.check_call(cmd)
    return out_path


def read_ahead(items):
    """The items of ``items`` (an iterable), produced one ahead of the consumer on a helper thread; what it raises there is raised
    here."""
    q = queue.Queue(maxsize=1)

    def run():
        try:
            for c in items:
                q.put(c)
            q.put(None)
        except Exception as e:          # surfaced by the consumer
            q.put(e)
    threading.Thread(target=run, daemon=True).start()
    while True:
        c = q.get()
        if c is None:
            return
        if isinstance(c, Exception):
            raise c
        yield c


class DeviceCodec:
    """One codec object of libamplihip.so (``prefix``: "amp_sam" / "amp_bam", with ``n_stages`` timed stages): on the device of
    ``engine`` (lib.Engine), or the host twin when ``twin`` is the path of its library.  ``self.info`` = the info struct of
    the last piece (n_rows, n_cig, n_bases_padded)."""

    def __init__(self, prefix, n_stages, engine=None, twin=None):
        if twin is not None:
            self.L = C.CDLL(twin); self.is_twin = True; ctx = None
        else:
            from . import lib
            self.L = lib.load(); self.is_twin = False; ctx = engine.h
        self.prefix, self.n_stages = prefix, n_stages
        self._fn("destroy").restype = None
        self._fn("destroy").argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        self._chk(self._fn("create")(ctx, C.byref(self.h)), prefix + "_create")
        self.info = None

    def _fn(self, name):
        return getattr(self.L, "%s_%s" % (self.prefix, name))

    def _chk(self, rc, where):
        if rc:
            from .lib import AmpliHipError
            raise AmpliHipError(rc, where)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_references(self, names):
        """amp_*_set_references: the names RNAME / RNEXT are read as or written from (the header's @SQ lines), once per run."""
        enc = [n.encode("ascii") for n in names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        self._chk(self._fn("set_references")(self.h, C.c_int32(len(enc)), arr), self.prefix + "_set_references")

    def dev_reads(self):
        rd = abi.AmpDevReads()
        self._chk(self._fn("reads")(self.h, C.byref(rd)), self.prefix + "_reads")
        return rd

    def batch(self, slack=0):
        """(the batch of the last piece as a host ReadBatch with src_index = the rows' records, the ``slack`` spare bytes behind
        cig, seq and qual as three arrays).  slack: what the codec's batch_to_host copies, 0 or 16."""
        n, nc, nb = int(self.info.n_rows), int(self.info.n_cig), int(self.info.n_bases_padded)
        sw, sb = slack // 4, slack
        a = dict(pos=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16), tlen=np.zeros(n, np.int32), lseq=np.zeros(n, np.uint32),
                 cig_off=np.zeros(n + 1, np.uint64), cig=np.full(nc + sw, 0xA5A5A5A5, np.uint32), seq_off=np.zeros(n + 1, np.uint64),
                 seq=np.full(nb // 2 + sb, 0xA5, np.uint8), qual=np.full(nb + sb, 0xA5, np.uint8))
        src = np.zeros(n, np.int64)
        st = abi.AmpReads(n, *[abi.ptr(a[k]) for k in ("pos", "flag", "tlen", "lseq", "cig_off", "cig", "seq_off", "seq", "qual")])
        self._chk(self._fn("batch_to_host")(self.h, C.byref(st), C.c_void_p(abi.ptr(src))), self.prefix + "_batch_to_host")
        tails = (a["cig"][nc:].copy(), a["seq"][nb // 2:].copy(), a["qual"][nb:].copy())
        rb = ReadBatch(a["pos"], a["flag"], a["tlen"], a["lseq"], a["cig_off"], a["cig"][:nc], a["seq_off"], a["seq"][:nb // 2], a["qual"][:nb],
                       src_index=src)
        return rb, tails

    def process(self, read_base=0):
        """amp_*_process: (first row with a non-zero status or -1, that status); the row is kept in ``self.first_bad`` as well."""
        bad = C.c_int64(-1); st = C.c_uint8(0)
        self._chk(self._fn("process")(self.h, C.c_uint64(read_base), C.byref(bad), C.byref(st)), self.prefix + "_process")
        self.first_bad = int(bad.value)
        return int(bad.value), int(st.value)

    # ---- trimmed BAM out of the codec (amp_bam_encode / amp_sam_encode and the tail they share) --------------------------------
    def set_deflater(self, fn):
        """Twin only: the DEFLATE encoder of its encodes -- the address of ampdf_hostsim_blocks (amp_deflate.hip's host phases), or a
        TWIN_DEFLATE_FN object."""
        self._deflater = fn
        self._chk(self._fn("twin_set_deflater")(self.h, fn), self.prefix + "_twin_set_deflater")

    def guards_ok(self):
        """Twin only: no encode so far wrote behind one of its buffers."""
        return int(self._fn("twin_guards")(self.h)) == 0

    def _encoded(self, info):
        """The BGZF blocks of the encode that answered ``info``, as they go into the file.  A block whose stream did not fit comes
        down raw and is compressed here (info.n_blocks_host counts it; never on real data)."""
        self.out_info = info
        out = np.empty(max(int(info.file_bytes), 1), np.uint8)
        if info.file_bytes:
            self._chk(self._fn("encoded_to_host")(self.h, C.c_void_p(abi.ptr(out)), C.c_int64(out.size)), self.prefix + "_encoded_to_host")
        out = out[:int(info.file_bytes)]
        if info.n_blocks_host:
            lens = np.zeros(int(info.n_blocks), np.uint32)
            self._chk(self._fn("encoded_blocks")(self.h, C.c_void_p(abi.ptr(lens)), C.c_int64(lens.size)), self.prefix + "_encoded_blocks")
            enc = int(info.stream_bytes) - int(info.carry_out)
            parts, at = [], 0
            for k, n in enumerate(int(x) for x in lens):
                if n:
                    parts.append(out[at:at + n].tobytes()); at += n
                else:
                    parts.append(bgzf_block(self.stream(k * OUT_BS, min(OUT_BS, enc - k * OUT_BS)).tobytes()))
                    info.bytes_down += min(OUT_BS, enc - k * OUT_BS)
            out = np.frombuffer(b"".join(parts), np.uint8)
        return out, info

    def stream(self, start=0, n=None):
        """Bytes [start, start + n) of the uncompressed stream [carry | new records] of the last encode (n None: to its end)."""
        n = int(self.out_info.stream_bytes) - start if n is None else n
        buf = np.zeros(max(n, 1), np.uint8)
        self._chk(self._fn("stream_to_host")(self.h, C.c_int64(start), C.c_int64(n), C.c_void_p(abi.ptr(buf))), self.prefix + "_stream_to_host")
        return buf[:n]

    def stage_ms(self, on=True, read=True):
        ms = (C.c_float * self.n_stages)(*([-1.0] * self.n_stages))
        self._chk(self._fn("stage_ms")(self.h, C.c_int(1 if on else 0), ms if read else None), self.prefix + "_stage_ms")
        return [float(x) for x in ms]
