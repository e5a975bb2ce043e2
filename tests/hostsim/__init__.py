"""Loader for the CPU simulation of the device per-read functions (test infrastructure)."""
import ctypes as C
import os
import subprocess

import numpy as np

from amplipy_amd import abi
from oracle import oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libhostsim.so")
        src = os.path.join(_HERE, "hostsim.hip")
        hdrs = [os.path.join(_HERE, "..", "..", "amplipy_amd", "csrc", h) for h in ("amp_read.hpp", "amp_bf.hpp", "amp_plan.hpp", "amp_call.hpp")]
        if not os.path.isfile(so) or os.path.getmtime(so) < max([os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]):
            subprocess.check_call(["hipcc", "-O1", "-fPIC", "-shared", "--offload-arch=gfx950", "-o", so, src])
        _LIB = C.CDLL(so)
        _LIB.sim_process_range.restype = C.c_int
        _LIB.sim_free.restype = None
    return _LIB


def process(batch, ref_len, mn, mx, mpl, mq, w, do_trim=True, do_count=True, **kw):
    L = lib()
    return oracle.process(batch, ref_len, mn, mx, mpl, mq, w, do_trim=do_trim, do_count=do_count,
                          _fn=L.sim_process_range, _free=L.sim_free, **kw)


def cig2_fuzz(seed, iters):
    """(mismatches, punted, compared) of the two-segment closed forms against the generic trim code."""
    L = lib()
    L.sim_cig2_fuzz.restype = C.c_long
    np_, nc = C.c_long(0), C.c_long(0)
    bad = L.sim_cig2_fuzz(C.c_uint64(seed), C.c_long(iters), C.byref(np_), C.byref(nc))
    return int(bad), int(np_.value), int(nc.value)


def bf_fuzz(seed, iters):
    """(mismatches, punted, compared) of the branch-free closed forms (amp_bf.hpp) against the branchy ones."""
    L = lib()
    L.sim_bf_fuzz.restype = C.c_long
    np_, nc = C.c_long(0), C.c_long(0)
    bad = L.sim_bf_fuzz(C.c_uint64(seed), C.c_long(iters), C.byref(np_), C.byref(nc))
    return int(bad), int(np_.value), int(nc.value)


def regops_fuzz(seed, iters):
    """(mismatches, events, error reads) of the op-by-op indel walk (count_regular_ops) against the exact pair walk."""
    L = lib()
    L.sim_regops_fuzz.restype = C.c_long
    ne, nr = C.c_long(0), C.c_long(0)
    bad = L.sim_regops_fuzz(C.c_uint64(seed), C.c_long(iters), C.byref(ne), C.byref(nr))
    return int(bad), int(ne.value), int(nr.value)


def call_positions(counts, ins_at, ref_seq, params):
    """The per-position decision of k_call (amp_call.hpp) on the CPU -> (POS_CALL_DTYPE[ref_len], n_relevant), the shape of
    Engine.call_positions.  ``ref_seq`` may be None when params.run_variants is 0."""
    L = lib()
    L.sim_call_positions.restype = C.c_int
    c = np.ascontiguousarray(counts, np.uint32); ia = np.ascontiguousarray(ins_at, np.uint32)
    G = ia.size
    assert c.size == G * abi.NSYM
    ref = None if ref_seq is None else np.frombuffer(ref_seq.encode("ascii"), np.uint8)
    assert ref is None or ref.size == G
    out = np.zeros(G, abi.POS_CALL_DTYPE); nr = C.c_int64(0)
    rc = L.sim_call_positions(C.c_void_p(abi.ptr(c)), C.c_void_p(abi.ptr(ia)), C.c_void_p(abi.ptr(ref)), C.c_int32(G),
                              C.byref(params), C.c_void_p(abi.ptr(out)), C.byref(nr))
    assert rc == 0
    return out, int(nr.value)
