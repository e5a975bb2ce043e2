"""ctypes binding of libamplihip.so (include/amplihip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``amplipy_amd.build``.  There is
no Python or CPU fallback: if the shared object is missing or no GPU is visible, the calls
below raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (development only -- AMPLIPY_DEV=1 AMPLIHIP_LIB=path: another build of the same library, for A/B timing by the tools under tools/;
#  the shipped package loads the library that lies next to this file and nothing else)
LIB_PATH = (os.environ.get("AMPLIHIP_LIB") if os.environ.get("AMPLIPY_DEV") == "1" else None) or os.path.join(_HERE, "libamplihip.so")
_LIB = None

EXPORTS = [
    "amp_version", "amp_strerror", "amp_last_error", "amp_read_status_exception", "amp_device_count",
    "amp_find_overlapping_primers", "amp_ctx_create", "amp_ctx_destroy", "amp_ctx_set_stream",
    "amp_ctx_bind_counts", "amp_set_primers", "amp_set_params", "amp_process_batch",
    "amp_process_batch_device", "amp_sync", "amp_last_kernel_ms", "amp_get_counts", "amp_add_counts",
    "amp_get_ins_events", "amp_counts_device_ptr", "amp_reduce", "amp_reset", "amp_error_reads",
    "amp_reserve_events", "amp_set_kernel_variant", "amp_set_reference", "amp_call_positions",
    "amp_event_strings", "amp_debug_counters", "amp_call_compact", "amp_debug_blocks", "amp_call_compact_view", "amp_set_timing", "amp_call_compact_begin", "amp_coordinate_helpers", "amp_drain_ins_events", "amp_set_cu_share", "amp_debug_second_grids", "amp_debug_last_second_grids", "amp_debug_event_capacity",
    "amp_aggregate_ins_events", "amp_fast_path_active", "amp_last_kernel_variant",
    "amp_deflate_blocks", "amp_deflate_blocks_device", "amp_deflate_blocks_device_counted", "amp_deflate_sync", "amp_deflate_blocks_cb",
    "amp_sam_create", "amp_sam_destroy", "amp_sam_set_references", "amp_sam_parse", "amp_sam_reads", "amp_sam_batch_to_host",
    "amp_sam_process", "amp_sam_format", "amp_sam_stage_ms",
    "amp_bam_create", "amp_bam_destroy", "amp_bam_feed", "amp_bam_dev_refuse", "amp_bam_refused", "amp_bam_verdicts", "amp_bam_patch_block", "amp_bam_reindex",
    "amp_bam_reads", "amp_bam_batch_to_host", "amp_bam_image_to_host", "amp_bam_process", "amp_bam_stage_ms",
    "amp_bam_encode", "amp_bam_encoded_to_host", "amp_bam_encoded_blocks", "amp_bam_stream_to_host",
    "amp_sam_set_output", "amp_sam_encode", "amp_sam_encode_bytes", "amp_sam_encoded_to_host", "amp_sam_encoded_blocks", "amp_sam_stream_to_host",
    "amp_sam_first_bad", "amp_sam_waits",
    "amp_bam_set_references", "amp_bam_text_check", "amp_bam_format",
    "amp_qc_find_primer_owners", "amp_qc_enable", "amp_qc_read_tallies", "amp_qc_depth", "amp_qc_last_ms",
    "amp_qc_clips_enable", "amp_qc_clips_get", "amp_qc_clips_add", "amp_qc_clips_last_ms",
    "amp_strand_enable", "amp_strand_get", "amp_strand_add", "amp_strand_last_ms",
    "amp_amplicon_enable", "amp_amplicon_get", "amp_amplicon_add", "amp_amplicon_last_ms",
    "amp_codon_enable", "amp_codon_get", "amp_codon_add", "amp_codon_last_ms",
    "amp_del_enable", "amp_del_get", "amp_del_add", "amp_del_last_ms",
    "amp_insev_enable", "amp_insev_get", "amp_insev_add", "amp_insev_last_ms",
    "amp_cooc_enable", "amp_cooc_get", "amp_cooc_add", "amp_cooc_last_ms",
    "amp_errprof_enable", "amp_errprof_get", "amp_errprof_add", "amp_errprof_last_ms",
    "amp_hap_enable", "amp_hap_get", "amp_hap_add", "amp_hap_last_ms",
    "amp_readpos_enable", "amp_readpos_get", "amp_readpos_add", "amp_readpos_last_ms",
]


class AmpliHipError(RuntimeError):
    def __init__(self, rc, where, detail=""):
        self.rc = rc
        super().__init__("%s: %s (%d)%s" % (where, abi.RC_NAMES.get(rc, "?"), rc, (": " + detail) if detail else ""))


def load():
    """Load libamplihip.so or raise -- never substitutes anything else."""
    global _LIB
    if _LIB is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); amplipy_amd has no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(L, name)  # AttributeError if the build is stale
        L.amp_strerror.restype = C.c_char_p
        L.amp_last_error.restype = C.c_char_p
        L.amp_last_error.argtypes = [C.c_void_p]
        L.amp_read_status_exception.restype = C.c_char_p
        L.amp_counts_device_ptr.restype = C.c_void_p
        L.amp_counts_device_ptr.argtypes = [C.c_void_p]
        L.amp_ctx_destroy.restype = None
        L.amp_ctx_destroy.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def find_overlapping_primers(ref_len, primers, offset):
    """find_overlapping_primers (AmpliPy.py:174-209) -> (min_start, max_end, max_primer_len);
    -1 stands for None."""
    L = load()
    ps = sorted((int(a), int(b)) for a, b in primers)
    st = np.array([p[0] for p in ps], np.int32); en = np.array([p[1] for p in ps], np.int32)
    mn = np.empty(ref_len, np.int32); mx = np.empty(ref_len, np.int32)
    mpl = C.c_int32(0)
    rc = L.amp_find_overlapping_primers(C.c_int32(ref_len), C.c_int32(len(ps)), C.c_void_p(abi.ptr(st)),
                                        C.c_void_p(abi.ptr(en)), C.c_int32(offset), C.c_void_p(abi.ptr(mn)),
                                        C.c_void_p(abi.ptr(mx)), C.byref(mpl))
    if rc:
        raise AmpliHipError(rc, "amp_find_overlapping_primers")
    return mn, mx, int(mpl.value)


def find_primer_owners(ref_len, primers, offset):
    """amp_qc_find_primer_owners -> (left_owner, right_owner), int32[ref_len] of indices into sorted(primers); -1: no primer
    covers the position.  left_owner[p] is the primer max_primer_end[p] comes from (A:450), right_owner[p] the one
    min_primer_start[p] comes from (A:451); ties go to the smallest index."""
    L = load()
    ps = sorted((int(a), int(b)) for a, b in primers)
    st = np.array([p[0] for p in ps], np.int32); en = np.array([p[1] for p in ps], np.int32)
    lo = np.empty(ref_len, np.int32); ro = np.empty(ref_len, np.int32)
    rc = L.amp_qc_find_primer_owners(C.c_int32(ref_len), C.c_int32(len(ps)), C.c_void_p(abi.ptr(st)), C.c_void_p(abi.ptr(en)),
                                     C.c_int32(offset), C.c_void_p(abi.ptr(lo)), C.c_void_p(abi.ptr(ro)))
    if rc:
        raise AmpliHipError(rc, "amp_qc_find_primer_owners")
    return lo, ro


class Engine:
    """One amp_ctx: the device-side state of a run (count table, insertion events)."""

    def __init__(self, ref_len, device=0):
        self.L = load()
        self.ref_len = int(ref_len)
        self.device = device
        h = C.c_void_p()
        rc = self.L.amp_ctx_create(C.byref(h), C.c_int(device), C.c_int32(ref_len))
        if rc:
            raise AmpliHipError(rc, "amp_ctx_create", "no usable MI355X device" if rc == -4 else "")
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.L.amp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc:
            raise AmpliHipError(rc, where, (self.L.amp_last_error(self.h) or b"").decode())

    # ---- configuration ---------------------------------------------------------------
    def set_primers(self, min_start, max_end, max_primer_len):
        mn = np.ascontiguousarray(min_start, np.int32); mx = np.ascontiguousarray(max_end, np.int32)
        assert mn.size == self.ref_len and mx.size == self.ref_len
        self._chk(self.L.amp_set_primers(self.h, C.c_void_p(abi.ptr(mn)), C.c_void_p(abi.ptr(mx)),
                                         C.c_int32(max_primer_len)), "amp_set_primers")

    def set_params(self, min_quality=20, window=4, do_trim=True, do_count=True):
        self._chk(self.L.amp_set_params(self.h, C.c_int32(min_quality), C.c_int32(window), C.c_int32(int(do_trim)),
                                        C.c_int32(int(do_count))), "amp_set_params")

    def fast_path_active(self):
        """True when runs with the current parameters take a fast kernel (windows of 1..8, min_quality <= 128)."""
        rc = self.L.amp_fast_path_active(self.h)
        if rc < 0:
            self._chk(rc, "amp_fast_path_active")
        return rc == 1

    def last_kernel_variant(self):
        """The kernel variant the last batch took (what the default, 0, resolved to)."""
        rc = self.L.amp_last_kernel_variant(self.h)
        if rc < 0:
            self._chk(rc, "amp_last_kernel_variant")
        return rc

    def set_kernel_variant(self, v):
        self._chk(self.L.amp_set_kernel_variant(self.h, C.c_int(v)), "amp_set_kernel_variant")

    def set_cu_share(self, divisor):
        """The fast kernel's grid for 1 / divisor of the CUs: for several engines in flight on different streams."""
        self._chk(self.L.amp_set_cu_share(self.h, C.c_int(divisor)), "amp_set_cu_share")

    def debug_second_grids(self, gen_blocks=0, heavy_blocks=0):
        """Development aid: blocks of the general pass / the heavy pass behind a fast kernel (0 = predicted from the last pass)."""
        self._chk(self.L.amp_debug_second_grids(self.h, C.c_int(gen_blocks), C.c_int(heavy_blocks)), "amp_debug_second_grids")

    def debug_last_second_grids(self):
        """(blocks of the general pass, blocks of the heavy pass) of the last pass behind a fast kernel."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.amp_debug_last_second_grids(self.h, C.byref(a), C.byref(b)), "amp_debug_last_second_grids")
        return int(a.value), int(b.value)

    def set_stream(self, hip_stream):
        self._chk(self.L.amp_ctx_set_stream(self.h, C.c_void_p(hip_stream)), "amp_ctx_set_stream")

    def bind_counts(self, dev_ptr):
        self._chk(self.L.amp_ctx_bind_counts(self.h, C.c_void_p(dev_ptr)), "amp_ctx_bind_counts")

    def set_timing(self, split):
        self._chk(self.L.amp_set_timing(self.h, C.c_int(1 if split else 0)), "amp_set_timing")

    def debug_event_capacity(self):
        """Slots per shard the insertion-event list has room for as it stands (amp_debug_event_capacity)."""
        n = C.c_int64(0)
        self._chk(self.L.amp_debug_event_capacity(self.h, C.byref(n)), "amp_debug_event_capacity")
        return int(n.value)

    def reserve_events(self, cap):
        self._chk(self.L.amp_reserve_events(self.h, C.c_int64(cap)), "amp_reserve_events")

    # ---- hot path --------------------------------------------------------------------
    def process(self, batch, read_base=0, want_trim=True):
        """amp_process_batch on a host ReadBatch; returns abi.TrimResult."""
        res = abi.TrimResult(batch)
        rd = abi.reads_struct(batch)
        out = res.struct()
        self._chk(self.L.amp_process_batch(self.h, C.byref(rd), C.c_uint64(read_base),
                                           C.byref(out) if want_trim else None), "amp_process_batch")
        return res

    def process_device(self, dev_reads, read_base=0, dev_out=None):
        """amp_process_batch_device: abi.AmpDevReads of device pointers; asynchronous."""
        self._chk(self.L.amp_process_batch_device(self.h, C.byref(dev_reads), C.c_uint64(read_base),
                                                  C.byref(dev_out) if dev_out is not None else None),
                  "amp_process_batch_device")

    def sync(self):
        self._chk(self.L.amp_sync(self.h), "amp_sync")

    def last_kernel_ms(self):
        t = C.c_float(0); s = C.c_float(0)
        self._chk(self.L.amp_last_kernel_ms(self.h, C.byref(t), C.byref(s)), "amp_last_kernel_ms")
        return float(t.value), float(s.value)

    # ---- state -----------------------------------------------------------------------
    def counts(self):
        c = np.empty((self.ref_len, abi.NSYM), np.uint32)
        self._chk(self.L.amp_get_counts(self.h, C.c_void_p(abi.ptr(c))), "amp_get_counts")
        return c

    def add_counts(self, counts):
        c = np.ascontiguousarray(counts, np.uint32)
        assert c.size == self.ref_len * abi.NSYM
        self._chk(self.L.amp_add_counts(self.h, C.c_void_p(abi.ptr(c))), "amp_add_counts")

    def counts_device_ptr(self):
        return self.L.amp_counts_device_ptr(self.h)

    def events(self):
        n = C.c_int64(0)
        self._chk(self.L.amp_get_ins_events(self.h, C.byref(n), None, C.c_int64(0)), "amp_get_ins_events")
        ev = np.zeros(int(n.value), abi.INS_EVENT_DTYPE)
        if n.value:
            self._chk(self.L.amp_get_ins_events(self.h, C.byref(n), C.c_void_p(abi.ptr(ev)), C.c_int64(ev.size)),
                      "amp_get_ins_events")
        return ev[:int(n.value)]          # the size query counts slots; a few may have been reserved and left unused

    def drain_events(self):
        """The events recorded since the last drain (or reset); the device list is empty afterwards."""
        n = C.c_int64(0)
        self._chk(self.L.amp_get_ins_events(self.h, C.byref(n), None, C.c_int64(0)), "amp_get_ins_events")
        ev = np.zeros(max(int(n.value), 1), abi.INS_EVENT_DTYPE)
        self._chk(self.L.amp_drain_ins_events(self.h, C.byref(n), C.c_void_p(abi.ptr(ev)), C.c_int64(ev.size)), "amp_drain_ins_events")
        return ev[:int(n.value)]

    def aggregate_events(self, dev_reads=None, read_base=0, drain=False):
        """amp_aggregate_ins_events: the insertion events recorded so far, sorted and run-length encoded ON THE DEVICE ->
        INS_RUN_DTYPE[n_runs], one record per (ref_pos, allele): a representative event and the number of events.
        dev_reads None = the batch of the last process() call (still staged on the device)."""
        n = C.c_int64(0)
        rdp = C.byref(dev_reads) if dev_reads is not None else None
        self._chk(self.L.amp_aggregate_ins_events(self.h, rdp, C.c_uint64(read_base), C.c_int(0), C.byref(n), None, C.c_int64(0)),
                  "amp_aggregate_ins_events")
        runs = np.zeros(max(int(n.value), 1), abi.INS_RUN_DTYPE)
        self._chk(self.L.amp_aggregate_ins_events(self.h, rdp, C.c_uint64(read_base), C.c_int(1 if drain else 0), C.byref(n),
                                                  C.c_void_p(abi.ptr(runs)), C.c_int64(runs.size)), "amp_aggregate_ins_events")
        return runs[:int(n.value)]

    def debug_blocks(self):
        out = np.zeros((4096, 4), np.uint32); nb = C.c_int(0)
        self._chk(self.L.amp_debug_blocks(self.h, C.c_void_p(abi.ptr(out)), C.c_int(4096), C.byref(nb)), "amp_debug_blocks")
        return out[:nb.value]

    def debug_counters(self):
        out = np.zeros(16, np.uint64)
        self._chk(self.L.amp_debug_counters(self.h, C.c_void_p(abi.ptr(out))), "amp_debug_counters")
        return out

    def error_reads(self):
        n = C.c_int64(0)
        self._chk(self.L.amp_error_reads(self.h, C.byref(n)), "amp_error_reads")
        return int(n.value)

    def reduce(self, comm=None, root=0):
        self._chk(self.L.amp_reduce(self.h, C.c_void_p(comm), C.c_int(root)), "amp_reduce")

    def reset(self):
        self._chk(self.L.amp_reset(self.h), "amp_reset")

    # ---- QC report -------------------------------------------------------------------
    def qc_enable(self, primers=(), primer_pos_offset=0, min_length=0, include_no_primer=False, regions=(), depths=()):
        """amp_qc_enable: the report on, its tallies zero.  primers: (start, end) pairs (sorted here like load_primers does);
        regions: (start, end) pairs, the caller's region 0 included; depths: up to 4 thresholds.  ``qc_disable`` turns it off."""
        ps = sorted((int(a), int(b)) for a, b in primers)
        st = np.array([p[0] for p in ps], np.int32); en = np.array([p[1] for p in ps], np.int32)
        rs = np.array([int(r[0]) for r in regions], np.int32); re_ = np.array([int(r[1]) for r in regions], np.int32)
        if len(depths) > abi.QC_MAX_DEPTHS:
            raise ValueError("at most %d depth thresholds" % abi.QC_MAX_DEPTHS)
        p = abi.AmpQcParams(len(ps), abi.ptr(st) if len(ps) else None, abi.ptr(en) if len(ps) else None, int(primer_pos_offset),
                            int(min_length), int(bool(include_no_primer)), rs.size, abi.ptr(rs) if rs.size else None,
                            abi.ptr(re_) if rs.size else None, len(depths))
        for k, d in enumerate(depths):
            p.depths[k] = int(d)
        self._chk(self.L.amp_qc_enable(self.h, C.byref(p)), "amp_qc_enable")
        self._qc_shape = (len(ps), int(rs.size))

    def qc_disable(self):
        self._chk(self.L.amp_qc_enable(self.h, None), "amp_qc_enable")

    def qc_read_tallies(self):
        """amp_qc_read_tallies -> (dict of the amp_qc_reads fields, reads_start uint64[n_primers], reads_end uint64[n_primers])."""
        n_primers = getattr(self, "_qc_shape", (0, 0))[0]
        t = np.zeros(len(abi.QC_READ_FIELDS), np.uint64)
        ps = np.zeros(max(n_primers, 1), np.uint64); pe = np.zeros(max(n_primers, 1), np.uint64)
        self._chk(self.L.amp_qc_read_tallies(self.h, C.c_void_p(abi.ptr(t)), C.c_void_p(abi.ptr(ps)), C.c_void_p(abi.ptr(pe))),
                  "amp_qc_read_tallies")
        return {k: int(v) for k, v in zip(abi.QC_READ_FIELDS, t)}, ps[:n_primers], pe[:n_primers]

    def qc_depth(self, want_depth=True):
        """amp_qc_depth on the table as it stands -> (depth uint32[ref_len] or None, QC_REGION_DTYPE[n_regions])."""
        depth = np.zeros(self.ref_len, np.uint32) if want_depth else None
        n_regions = getattr(self, "_qc_shape", (0, 0))[1]
        regions = np.zeros(max(n_regions, 1), abi.QC_REGION_DTYPE)
        self._chk(self.L.amp_qc_depth(self.h, C.c_void_p(abi.ptr(depth)), C.c_void_p(abi.ptr(regions))), "amp_qc_depth")
        return depth, regions[:n_regions]

    def _hook_last_ms(self, entry):
        """Milliseconds of a hook's kernel behind the last batch (``entry``: its amp_*_last_ms); ESTATE when none ran."""
        t = C.c_float(0)
        self._chk(getattr(self.L, entry)(self.h, C.byref(t)), entry)
        return float(t.value)

    def _tables(self, entry, specs, arrays=None, head=()):
        """The tables of a hook through ``entry``, one per (shape, dtype) of ``specs``, behind the arguments ``head``.
        ``arrays`` None: an amp_*_get into new arrays (a first dimension of 0 is 1 for the call) -> the list of them.
        Else an amp_*_add of ``arrays``, each made contiguous and held to the size of its shape; a None is left out."""
        if arrays is None:
            arrs = [np.zeros((max(shape[0], 1),) + tuple(shape[1:]), dt) for shape, dt in specs]
        else:
            arrs = [None if a is None else np.ascontiguousarray(a, dt) for a, (_, dt) in zip(arrays, specs)]
            assert all(a is None or a.size == int(np.prod(shape)) for a, (shape, _) in zip(arrs, specs))
        self._chk(getattr(self.L, entry)(self.h, *head, *[C.c_void_p(abi.ptr(a)) for a in arrs]), entry)
        return arrs if arrays is not None else [a[:shape[0]] for a, (shape, _) in zip(arrs, specs)]

    def _keyed_get(self, entry, dtype, info_fields, tail=()):
        """The two calls of a keyed table's amp_*_get: without an array for the size, then -- the table is not empty -- with
        one that holds it -> (dtype[used], the info dict).  ``tail``: the arguments behind info."""
        n = C.c_int64(0)
        info = np.zeros(len(info_fields), np.uint64)
        args = (C.byref(n), C.c_void_p(abi.ptr(info))) + tuple(tail)
        rc = getattr(self.L, entry)(self.h, None, C.c_int64(0), *args)
        ev = np.zeros(max(int(n.value), 1), dtype)
        if rc == -1 and n.value > 0:            # (AMP_EINVAL with the needed size: the table is not empty)
            rc = getattr(self.L, entry)(self.h, C.c_void_p(abi.ptr(ev)), C.c_int64(ev.size), *args)
        self._chk(rc, entry)
        return ev[:int(n.value)], {k: int(v) for k, v in zip(info_fields, info)}

    def qc_last_ms(self):
        return self._hook_last_ms("amp_qc_last_ms")

    # ---- QC report: soft-clip sites ----------------------------------------------------
    def qc_clips_enable(self, clip_min):
        """amp_qc_clips_enable: the clip sites of the QC report on (clip_min 1..64), their table zero; 0: off.  Needs a QC
        report, and has to be called again after every ``qc_enable``."""
        self._chk(self.L.amp_qc_clips_enable(self.h, C.c_int32(int(clip_min))), "amp_qc_clips_enable")

    def _clip_specs(self):
        return [((self.ref_len + 1, 2, abi.CLIP_CELLS), np.uint32), ((abi.CLIP_SCALARS,), np.uint64)]

    def qc_clips_tables(self):
        """amp_qc_clips_get -> (table uint32[ref_len + 1][2][CLIP_CELLS], scalars uint64[4]: abi.CLIP_SCALAR_FIELDS)."""
        return tuple(self._tables("amp_qc_clips_get", self._clip_specs()))

    def qc_clips_add(self, table, scalars):
        """amp_qc_clips_add: a host table and its scalars added element-wise (the merge of partial tables)."""
        self._tables("amp_qc_clips_add", self._clip_specs(), (table, scalars))

    def qc_clips_last_ms(self):
        return self._hook_last_ms("amp_qc_clips_last_ms")

    # ---- strand and base-quality tallies ---------------------------------------------
    def strand_enable(self):
        """amp_strand_enable(1): the tallies on, the tables zero.  ``strand_disable`` turns them off."""
        self._chk(self.L.amp_strand_enable(self.h, C.c_int(1)), "amp_strand_enable")

    def strand_disable(self):
        self._chk(self.L.amp_strand_enable(self.h, C.c_int(0)), "amp_strand_enable")

    def _strand_specs(self):
        return [((self.ref_len, abi.NSYM), np.uint32), ((self.ref_len, abi.STRAND_QSUM_COLS), np.uint64)]

    def strand_tables(self):
        """amp_strand_get -> (rev uint32[ref_len][6], qsum uint64[ref_len][5]) as they stand."""
        return tuple(self._tables("amp_strand_get", self._strand_specs()))

    def strand_add(self, rev, qsum):
        """amp_strand_add: host tables added element-wise (the merge of partial tables)."""
        self._tables("amp_strand_add", self._strand_specs(), (rev, qsum))

    def strand_last_ms(self):
        return self._hook_last_ms("amp_strand_last_ms")

    # ---- per-amplicon allele counts ---------------------------------------------------
    def amplicon_enable(self, lo, hi, amp_start, amp_end):
        """amp_amplicon_enable: the hook on for the amplicons with spans [lo[a], hi[a]) and the two owner tables
        (int32[ref_len], -1: none), the tables zero.  ``amplicon_disable`` turns it off."""
        lo = np.ascontiguousarray(lo, np.int32); hi = np.ascontiguousarray(hi, np.int32)
        st = np.ascontiguousarray(amp_start, np.int32); en = np.ascontiguousarray(amp_end, np.int32)
        if lo.size == 0 or lo.size != hi.size:
            raise ValueError("one span per amplicon, at least one amplicon")
        if st.size != self.ref_len or en.size != self.ref_len:
            raise ValueError("the owner tables have one entry per reference position")
        pad = lambda a: a if a.size else np.zeros(1, np.int32)          # (a reference of no bases: the pointers are still there)
        self._chk(self.L.amp_amplicon_enable(self.h, C.c_int32(lo.size), C.c_void_p(abi.ptr(lo)), C.c_void_p(abi.ptr(hi)),
                                             C.c_void_p(abi.ptr(pad(st))), C.c_void_p(abi.ptr(pad(en)))), "amp_amplicon_enable")
        self._amplicon_shape = (int(lo.size), int((hi.astype(np.int64) - lo).sum()))

    def amplicon_disable(self):
        self._chk(self.L.amp_amplicon_enable(self.h, C.c_int32(0), None, None, None, None), "amp_amplicon_enable")

    def _amplicon_specs(self):
        n_amp, cells = getattr(self, "_amplicon_shape", (0, 0))
        return [((cells, abi.NSYM), np.uint32), ((n_amp + 1,), np.uint64)]

    def amplicon_tables(self):
        """amp_amplicon_get -> (counts uint32[sum span][6], reads uint64[n_amp + 1]) as they stand."""
        return tuple(self._tables("amp_amplicon_get", self._amplicon_specs()))

    def amplicon_add(self, counts, reads):
        """amp_amplicon_add: host tables added element-wise (the merge of partial tables)."""
        self._tables("amp_amplicon_add", self._amplicon_specs(), (counts, reads))

    def amplicon_last_ms(self):
        return self._hook_last_ms("amp_amplicon_last_ms")

    # ---- codon tallies ----------------------------------------------------------------
    def codon_enable(self, starts):
        """amp_codon_enable: the hook on for the codon slots at ``starts`` (int32, strictly increasing), the tables zero
        (DESIGN.md section 18).  ``codon_disable`` turns it off."""
        st = np.ascontiguousarray(starts, np.int32)
        if st.size == 0:
            raise ValueError("at least one codon slot")
        self._chk(self.L.amp_codon_enable(self.h, C.c_int32(st.size), C.c_void_p(abi.ptr(st))), "amp_codon_enable")
        self._codon_slots = int(st.size)

    def codon_disable(self):
        self._chk(self.L.amp_codon_enable(self.h, C.c_int32(0), None), "amp_codon_enable")

    def _codon_specs(self):
        return [((getattr(self, "_codon_slots", 0), abi.CODON_CELLS), np.uint32), ((2,), np.uint64)]

    def codon_tables(self):
        """amp_codon_get -> (codon uint32[n_slots][65], reads uint64[2]: tallied, skipped) as they stand."""
        return tuple(self._tables("amp_codon_get", self._codon_specs()))

    def codon_add(self, codon, reads):
        """amp_codon_add: host tables added element-wise (the merge of partial tables)."""
        self._tables("amp_codon_add", self._codon_specs(), (codon, reads))

    def codon_last_ms(self):
        return self._hook_last_ms("amp_codon_last_ms")

    # ---- deletion events ---------------------------------------------------------------
    def del_enable(self, log2_capacity=0):
        """amp_del_enable: the hook on, the table zero, 2^log2_capacity slots (0: the default).
        ``del_disable`` turns it off; the table stays readable."""
        self._chk(self.L.amp_del_enable(self.h, C.c_int(1), C.c_int(int(log2_capacity))), "amp_del_enable")

    def del_disable(self):
        self._chk(self.L.amp_del_enable(self.h, C.c_int(0), C.c_int(0)), "amp_del_enable")

    def del_events(self):
        """amp_del_get -> (abi.DEL_EVENT_DTYPE[used] ordered by (start, len), {"used", "capacity", "lost"})."""
        return self._keyed_get("amp_del_get", abi.DEL_EVENT_DTYPE, abi.DEL_INFO_FIELDS)

    def del_add(self, events):
        """amp_del_add: host entries (abi.DEL_EVENT_DTYPE) through the kernel's insert path (the merge of partial tables)."""
        ev = np.ascontiguousarray(events, abi.DEL_EVENT_DTYPE)
        if ev.size:
            self._chk(self.L.amp_del_add(self.h, C.c_void_p(abi.ptr(ev)), C.c_int64(ev.size)), "amp_del_add")

    def del_last_ms(self):
        return self._hook_last_ms("amp_del_last_ms")

    # ---- insertion alleles: strand, quality and read-position evidence (the insertion half of the indel unit) ----
    def insev_enable(self, log2_capacity=0):
        """amp_insev_enable: the half on, the table zero, 2^log2_capacity slots (0: the default).
        ``insev_disable`` turns it off; the table stays readable.  The deletion half (``del_enable``) is not touched."""
        self._chk(self.L.amp_insev_enable(self.h, C.c_int(1), C.c_int(int(log2_capacity))), "amp_insev_enable")

    def insev_disable(self):
        self._chk(self.L.amp_insev_enable(self.h, C.c_int(0), C.c_int(0)), "amp_insev_enable")

    def insev_entries(self):
        """amp_insev_get -> (abi.INSEV_ENTRY_DTYPE[used] ordered by (ref_pos, len, hash), {"used", "capacity", "lost"})."""
        return self._keyed_get("amp_insev_get", abi.INSEV_ENTRY_DTYPE, abi.DEL_INFO_FIELDS)

    def insev_add(self, entries):
        """amp_insev_add: host entries (abi.INSEV_ENTRY_DTYPE) through the kernel's insert path (the merge of partial tables)."""
        ev = np.ascontiguousarray(entries, abi.INSEV_ENTRY_DTYPE)
        if ev.size:
            self._chk(self.L.amp_insev_add(self.h, C.c_void_p(abi.ptr(ev)), C.c_int64(ev.size)), "amp_insev_add")

    def insev_last_ms(self):
        return self._hook_last_ms("amp_insev_last_ms")

    # ---- co-occurrence of listed mutations ---------------------------------------------
    def cooc_enable(self, set_off, site_pos, site_len, site_sym):
        """amp_cooc_enable: the hook on for the sets given -- set s has the sites [set_off[s], set_off[s + 1]) of site_pos
        (0-based), site_len (0: a substitution) and site_sym (0..3 for A C G T); sorted by first site -- the tables zero
        (DESIGN.md section 20).  ``cooc_disable`` turns it off."""
        off = np.ascontiguousarray(set_off, np.int32)
        pos = np.ascontiguousarray(site_pos, np.int32); ln = np.ascontiguousarray(site_len, np.int32)
        sym = np.ascontiguousarray(site_sym, np.uint8)
        if off.size < 2:
            raise ValueError("at least one mutation set")
        if off[0] != 0 or not (pos.size == ln.size == sym.size) or (np.diff(off) < 0).any() or int(off[-1]) != pos.size:
            raise ValueError("set_off does not describe the site arrays")
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        self._chk(self.L.amp_cooc_enable(self.h, C.c_int32(off.size - 1), C.c_void_p(abi.ptr(off)), C.c_void_p(abi.ptr(pad(pos))),
                                         C.c_void_p(abi.ptr(pad(ln))), C.c_void_p(abi.ptr(pad(sym)))), "amp_cooc_enable")
        self._cooc_sets = int(off.size - 1)

    def cooc_disable(self):
        self._chk(self.L.amp_cooc_enable(self.h, C.c_int32(0), None, None, None, None), "amp_cooc_enable")

    def _cooc_specs(self):
        return [((getattr(self, "_cooc_sets", 0), abi.COOC_CELLS), np.uint32), ((2,), np.uint64)]

    def cooc_tables(self):
        """amp_cooc_get -> (cooc uint32[n_sets][65], reads uint64[2]: tallied, skipped) as they stand."""
        return tuple(self._tables("amp_cooc_get", self._cooc_specs()))

    def cooc_add(self, cooc, reads):
        """amp_cooc_add: host tables added element-wise (the merge of partial tables)."""
        self._tables("amp_cooc_add", self._cooc_specs(), (cooc, reads))

    def cooc_last_ms(self):
        return self._hook_last_ms("amp_cooc_last_ms")

    # ---- error profile -----------------------------------------------------------------
    def errprof_enable(self, ref_seq, mask=None):
        """amp_errprof_enable(1): the hook on for the reference letters ``ref_seq`` (str or bytes of ref_len letters), the
        tables zero.  ``mask``: bool[ref_len], True for a position that takes no part, or None.
        ``errprof_disable`` turns it off; the tables stay readable."""
        ref = np.frombuffer(ref_seq.encode("ascii") if isinstance(ref_seq, str) else bytes(ref_seq), np.uint8)
        if ref.size != self.ref_len:
            raise ValueError("the reference has %d letters, the engine %d positions" % (ref.size, self.ref_len))
        bits = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, bool)
            if mk.size != self.ref_len:
                raise ValueError("the mask has one entry per reference position")
            bits = np.zeros((self.ref_len + 31) // 32 + 1, np.uint32)
            p = np.nonzero(mk)[0]
            np.bitwise_or.at(bits, p >> 5, (np.uint32(1) << (p & 31).astype(np.uint32)).astype(np.uint32))
        pad = ref if ref.size else np.zeros(1, np.uint8)
        self._chk(self.L.amp_errprof_enable(self.h, C.c_int(1), C.c_void_p(abi.ptr(pad)), C.c_void_p(abi.ptr(bits))), "amp_errprof_enable")

    def errprof_disable(self):
        self._chk(self.L.amp_errprof_enable(self.h, C.c_int(0), None, None), "amp_errprof_enable")

    _ERRPROF_SPECS = [(s, np.uint64) for s in (abi.EP_CYC_SHAPE, abi.EP_QUAL_SHAPE, abi.EP_SUB_SHAPE, (2,))]

    def errprof_tables(self):
        """amp_errprof_get -> (cyc uint64[2][512][2], qualt uint64[2][94][2], sub uint64[2][2][2][4][4], reads uint64[2]:
        profiled, skipped) as they stand."""
        return tuple(self._tables("amp_errprof_get", self._ERRPROF_SPECS))

    def errprof_add(self, cyc, qualt, sub, reads):
        """amp_errprof_add: host tables added element-wise (the merge of partial tables)."""
        self._tables("amp_errprof_add", self._ERRPROF_SPECS, (cyc, qualt, sub, reads))

    def errprof_last_ms(self):
        return self._hook_last_ms("amp_errprof_last_ms")

    # ---- read haplotypes per region ----------------------------------------------------
    def hap_enable(self, starts, ends, ref_seq, log2_capacity=0):
        """amp_hap_enable: the hook on for the regions [starts[k], ends[k]) (0-based, sorted by start, 1 to 4096 positions each)
        and the reference letters ``ref_seq`` (str or bytes of ref_len letters), the tables zero, 2^log2_capacity slots (0: the
        default).  ``hap_disable`` turns it off; the tables stay readable."""
        st = np.ascontiguousarray(starts, np.int32); en = np.ascontiguousarray(ends, np.int32)
        if st.ndim != 1 or st.size != en.size or st.size == 0:
            raise ValueError("one start and one end per region, at least one region")
        ref = np.frombuffer(ref_seq.encode("ascii") if isinstance(ref_seq, str) else bytes(ref_seq), np.uint8)
        if ref.size != self.ref_len:
            raise ValueError("the reference has %d letters, the engine %d positions" % (ref.size, self.ref_len))
        pad = ref if ref.size else np.zeros(1, np.uint8)
        self._chk(self.L.amp_hap_enable(self.h, C.c_int32(st.size), C.c_void_p(abi.ptr(st)), C.c_void_p(abi.ptr(en)), C.c_void_p(abi.ptr(pad)),
                                        C.c_int(int(log2_capacity))), "amp_hap_enable")
        self._hap_regions = int(st.size)

    def hap_disable(self):
        self._chk(self.L.amp_hap_enable(self.h, C.c_int32(0), None, None, None, C.c_int(0)), "amp_hap_enable")

    def _hap_specs(self):
        return [((getattr(self, "_hap_regions", 0), abi.HAP_TALLY_COLS), np.uint64), ((2,), np.uint64)]

    def hap_tables(self):
        """amp_hap_get -> (abi.HAP_ENTRY_DTYPE[used] ordered by the 14 key words, {"used", "capacity", "lost"},
        tally uint64[n_regions][6]: COVER REF REF_REV LOWQ OVERFLOW EDGE, reads uint64[2]: covering, other) as they stand."""
        specs = self._hap_specs()
        tally, reads = (np.zeros((max(shape[0], 1),) + tuple(shape[1:]), dt) for shape, dt in specs)
        ev, info = self._keyed_get("amp_hap_get", abi.HAP_ENTRY_DTYPE, abi.HAP_INFO_FIELDS, (C.c_void_p(abi.ptr(tally)), C.c_void_p(abi.ptr(reads))))
        return ev, info, tally[:specs[0][0][0]], reads

    def hap_add(self, entries, tally=None, reads=None):
        """amp_hap_add: host entries (abi.HAP_ENTRY_DTYPE) through the kernel's insert path, tally and reads added element-wise
        (the merge of partial tables)."""
        ev = np.ascontiguousarray(entries, abi.HAP_ENTRY_DTYPE)
        self._tables("amp_hap_add", self._hap_specs(), (tally, reads), head=(C.c_void_p(abi.ptr(ev)) if ev.size else None, C.c_int64(ev.size)))

    def hap_last_ms(self):
        return self._hook_last_ms("amp_hap_last_ms")

    # ---- read-position tallies per allele ----------------------------------------------
    def readpos_enable(self):
        """amp_readpos_enable(1): the tallies on, the table zero.  ``readpos_disable`` turns them off."""
        self._chk(self.L.amp_readpos_enable(self.h, C.c_int(1)), "amp_readpos_enable")

    def readpos_disable(self):
        self._chk(self.L.amp_readpos_enable(self.h, C.c_int(0)), "amp_readpos_enable")

    def _readpos_specs(self):
        return [((self.ref_len, abi.NSYM, abi.RP_BINS), np.uint32)]

    def readpos_tables(self):
        """amp_readpos_get -> hist uint32[ref_len][6][7] as it stands."""
        return self._tables("amp_readpos_get", self._readpos_specs())[0]

    def readpos_add(self, hist):
        """amp_readpos_add: a host table added element-wise (the merge of partial tables)."""
        self._tables("amp_readpos_add", self._readpos_specs(), (hist,))

    def readpos_last_ms(self):
        return self._hook_last_ms("amp_readpos_last_ms")

    # ---- calling ---------------------------------------------------------------------
    def set_reference(self, ref_seq):
        ref = np.frombuffer(ref_seq.encode("ascii") if isinstance(ref_seq, str) else bytes(ref_seq), np.uint8)
        assert ref.size == self.ref_len
        self._chk(self.L.amp_set_reference(self.h, C.c_void_p(abi.ptr(ref))), "amp_set_reference")

    def call_positions(self, params):
        """amp_call_positions -> (structured array POS_CALL_DTYPE[ref_len], n_relevant)."""
        out = np.zeros(self.ref_len, abi.POS_CALL_DTYPE)
        nr = C.c_int64(0)
        self._chk(self.L.amp_call_positions(self.h, C.byref(params), C.c_void_p(abi.ptr(out)), C.byref(nr)),
                  "amp_call_positions")
        return out, int(nr.value)

    def coordinate_helpers(self, cigars, ref_start, ref_pos, query_pos):
        """get_pos_on_query / get_pos_on_ref / fix_cigar (AmpliPy.py:363-423) for a list of CIGARs [(op, len), ...] on the
        device -> (pos_on_query int32[n], pos_on_ref int32[n], [fixed cigar tuples], status uint8[n])."""
        n = len(cigars)
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(c) for c in cigars])
        words = np.array([(int(l) << 4) | int(op) for c in cigars for op, l in c], np.uint32)
        rs, rp, qp = (np.ascontiguousarray(x, np.int32) for x in (ref_start, ref_pos, query_pos))
        oq, orf = np.zeros(n, np.int32), np.zeros(n, np.int32)
        fx, fn, st = np.zeros(max(words.size, 1), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._chk(self.L.amp_coordinate_helpers(self.h, C.c_int64(n), C.c_void_p(abi.ptr(off)), C.c_void_p(abi.ptr(words) if words.size else None),
                                                C.c_void_p(abi.ptr(rs)), C.c_void_p(abi.ptr(rp)), C.c_void_p(abi.ptr(qp)),
                                                C.c_void_p(abi.ptr(oq)), C.c_void_p(abi.ptr(orf)), C.c_void_p(abi.ptr(fx)),
                                                C.c_void_p(abi.ptr(fn)), C.c_void_p(abi.ptr(st))), "amp_coordinate_helpers")
        fixed = [[(int(w & 15), int(w >> 4)) for w in fx[int(off[i]):int(off[i]) + int(fn[i])]] for i in range(n)]
        return oq, orf, fixed, st

    def call_compact_begin(self, params):
        """Enqueue the calling kernels now; the next call_compact with the same parameters only waits for them."""
        self._chk(self.L.amp_call_compact_begin(self.h, C.byref(params)), "amp_call_compact_begin")

    def call_compact(self, params):
        """amp_call_compact_view -> (consensus int8[G], VAR_REC_DTYPE[V], relevant int32[R]).  The arrays
        are views of host memory owned by the engine, valid until the next call_* on it."""
        G = self.ref_len
        if not hasattr(self, "_cv"):
            self._cv = [abi.AmpCallView(), None, None]
        st = self._cv
        v = st[0]
        rc = self.L.amp_call_compact_view(self.h, C.byref(params), C.byref(v))
        if rc:
            self._chk(rc, "amp_call_compact_view")
        key = (v.consensus, v.vars, v.relevant)
        if st[1] != key:   # (re)wrap the library's image once per allocation
            cons = np.frombuffer((C.c_int8 * G).from_address(v.consensus), np.int8)
            vars_ = np.frombuffer((C.c_uint8 * (G * abi.VAR_REC_DTYPE.itemsize)).from_address(v.vars), abi.VAR_REC_DTYPE)
            rel = np.frombuffer((C.c_int32 * G).from_address(v.relevant), np.int32)
            st[1] = key; st[2] = (cons, vars_, rel)
        cons, vars_, rel = st[2]
        return cons, vars_[:v.n_vars], rel[:v.n_relevant]

    def event_text(self, events, read_base=0, dev_reads=None):
        """(lengths int64[n], text uint8[sum]) of ``events``: the allele bytes back to back, no Python step per event.
        dev_reads None = the batch of the last process() call (still staged on the device)."""
        n = events.size
        lens = np.maximum(events["q_to"].astype(np.int64) - events["q_from"].astype(np.int64), 0)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        text = np.zeros(max(int(off[n]), 1), np.uint8)
        ev = np.ascontiguousarray(events)
        self._chk(self.L.amp_event_strings(self.h, C.byref(dev_reads) if dev_reads is not None else None, C.c_uint64(read_base), C.c_int64(n),
                                           C.c_void_p(abi.ptr(ev)), C.c_void_p(abi.ptr(off)), C.c_void_p(abi.ptr(text))),
                  "amp_event_strings")
        return lens, text[:int(off[n])]

    def event_strings_device(self, dev_reads, events, read_base=0):
        """Strings of ``events`` (INS_EVENT_DTYPE) taken from a device-resident batch."""
        n = events.size
        lens = (events["q_to"] - events["q_from"]).astype(np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        text = np.zeros(max(int(off[n]), 1), np.uint8)
        ev = np.ascontiguousarray(events)
        self._chk(self.L.amp_event_strings(self.h, C.byref(dev_reads), C.c_uint64(read_base), C.c_int64(n),
                                           C.c_void_p(abi.ptr(ev)), C.c_void_p(abi.ptr(off)), C.c_void_p(abi.ptr(text))),
                  "amp_event_strings")
        raw = text.tobytes()
        return [raw[int(off[k]):int(off[k + 1])].decode("ascii") for k in range(n)]
