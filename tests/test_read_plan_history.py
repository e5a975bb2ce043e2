"""The blocks of the kernels behind a fast kernel (amp_plan.hpp: ReadPlan::gen_blocks / heavy_blocks), on the CPU.

The general pass and the heavy pass are launched with twice the blocks the engine's previous pass would have kept busy, between
8 and their full grids for the engine's share of the CUs; a pass without history takes the full grids.  The segments of the
lists (gen_grid, heavy_grid) and the scratch layout do not depend on the history: tests/test_read_plan.py holds those.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "plan_history_shim.cpp")
_HDR = os.path.join(_HERE, "..", "amplipy_amd", "csrc", "amp_plan.hpp")
_SO = os.path.join(_HERE, "hostsim", "libplanhistory.so")

BENCH_READS = 1993533        # the 10k x batch: 31,149 tiles, 1,024 list segments and 512 heavy blocks on 256 CUs


def plan(n, n_cu, share, prev_list, prev_heavy):
    if not os.path.isfile(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", _SO, _SRC])
    L = C.CDLL(_SO)
    L.plan_history.restype = None
    a = np.array([n, n_cu, share, prev_list, prev_heavy], np.int64)
    out = np.full(7, -1, np.int64)
    L.plan_history(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert out[0] == 1 and out[1] == 4
    return dict(zip(("gen_grid", "heavy_grid", "gen_blocks", "heavy_blocks", "total"), out[2:].tolist()))


def test_no_history_takes_the_full_grids():
    p = plan(BENCH_READS, 256, 1, -1, -1)
    assert (p["gen_grid"], p["heavy_grid"]) == (1024, 512)
    assert (p["gen_blocks"], p["heavy_blocks"]) == (1024, 512)
    # one of the two unknown: that kernel alone takes its full grid
    q = plan(BENCH_READS, 256, 1, 0, -1)
    assert (q["gen_blocks"], q["heavy_blocks"]) == (8, 512)


def test_empty_lists_before_give_eight_blocks():
    p = plan(BENCH_READS, 256, 1, 0, 0)
    assert (p["gen_blocks"], p["heavy_blocks"]) == (8, 8)
    assert (p["gen_grid"], p["heavy_grid"]) == (1024, 512), "the segments do not follow the history"
    assert p["total"] == plan(BENCH_READS, 256, 1, -1, -1)["total"], "nor does the scratch buffer"


def test_a_full_batch_before_gives_the_full_grids():
    p = plan(BENCH_READS, 256, 1, BENCH_READS, BENCH_READS)
    assert (p["gen_blocks"], p["heavy_blocks"]) == (1024, 512)
    # lists far longer than any batch: still the full grids, never more
    p = plan(BENCH_READS, 256, 1, 0x3FFFFFFF, 0x3FFFFFFF)
    assert (p["gen_blocks"], p["heavy_blocks"]) == (1024, 512)


def test_cu_share_two_halves_the_clamp():
    whole, half = plan(BENCH_READS, 256, 1, BENCH_READS, BENCH_READS), plan(BENCH_READS, 256, 2, BENCH_READS, BENCH_READS)
    assert (half["gen_blocks"], half["heavy_blocks"]) == (whole["gen_blocks"] // 2, whole["heavy_blocks"] // 2) == (512, 256)
    none = plan(BENCH_READS, 256, 2, -1, -1)
    assert (none["gen_blocks"], none["heavy_blocks"]) == (512, 256)
    assert (half["gen_grid"], half["heavy_grid"]) == (1024, 512)
    assert plan(BENCH_READS, 256, 2, 0, 0)["gen_blocks"] == 8


def test_twice_what_the_list_before_would_fill():
    # 10,000 listed reads are 157 tiles, 8 a segment: 20 segments -> 40 blocks; 1,000 heavy entries are 4 rounds of 256 -> 8 blocks
    p = plan(BENCH_READS, 256, 1, 10000, 1000)
    assert (p["gen_blocks"], p["heavy_blocks"]) == (40, 8)
    p = plan(BENCH_READS, 256, 1, 10000, 5000)
    assert p["heavy_blocks"] == 40
    # a long list is cut into longer segments, as the device cuts it: 1,000,000 reads are 15,625 tiles, 16 a segment, 977 segments
    assert plan(BENCH_READS, 256, 1, 1000000, 0)["gen_blocks"] == 1024
    assert plan(BENCH_READS, 256, 1, 200000, 0)["gen_blocks"] == 2 * 391


def test_small_batches_never_get_more_blocks_than_segments():
    for n in (1, 64, 513, 4096):
        for hist in (-1, 0, 4096):
            p = plan(n, 256, 1, hist, hist)
            assert 1 <= p["gen_blocks"] <= p["gen_grid"] and 1 <= p["heavy_blocks"] <= p["heavy_grid"], (n, hist, p)
    assert plan(4096, 256, 1, 0, 0)["gen_blocks"] == 8 == plan(4096, 256, 1, 0, 0)["gen_grid"]
    assert plan(1, 256, 1, 0, 0)["gen_blocks"] == 1
