"""The host's plan for a batch of reads (amplipy_amd/csrc/amp_plan.hpp) against the rules it replaced, on the CPU.

The header is compiled alone with g++ (tests/hostsim/plan_shim.cpp): that it builds without hipcc is the proof that it holds
nothing of HIP.  Routing, grids and the size of the scratch buffer are restated below in numpy from the launch code as it was
before the plan existed (literal numbers, not the header's constants), and the layout is checked for what its consumers index.
Every test runs on the header as shipped and as -DAMP_DEV builds see it (k_fast's stamps need room in dcnt there).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "plan_shim.cpp")
_HDR = os.path.join(_HERE, "..", "amplipy_amd", "csrc", "amp_plan.hpp")
_SO = {False: os.path.join(_HERE, "hostsim", "libplanshim.so"), True: os.path.join(_HERE, "hostsim", "libplanshim_dev.so")}

AXES = {
    "n": [1, 63, 64, 65, 1000, 30000, 1993533, 8000000, 19935330, 0x3FFFFFFF],
    "ops": [1, 2, 3, 8, 40],
    "pad": [152, 160, 192, 200, 256, 304],
    "window": [1, 2, 3, 4, 5, 6, 7, 8, 9, 12],
    "mq": [0, 1, 20, 128, 129],
    "req": [0, 1, 2, 3, 4, 5, 6, 7],
    "n_cu": [1, 64, 256, 304],
    "share": [1, 2, 16],
    "give_cig": [0, 1],
    "give_pos": [0, 1],
    "give_ncig": [0, 1],
}
ROWS = 120000
REGIONS = ["pingpong", "dlist", "dcnt", "split", "new_pos", "new_ncig", "new_cig", "glist", "gcnt", "gdense", "geo", "segfirst",
           "llist", "lpos", "clist"]
HEAD = ["ok", "kv", "variant", "f5_waves", "f5_qrun", "fg_grid", "fg_rpb", "fast_waves", "tg_grid", "tg_tpb", "gen_grid", "heavy_grid",
        "long_kernel", "direct", "ev_fixed", "total", "fast_path_active"]


def _lib(dev=False):
    so = _SO[dev]
    if not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared"] + (["-DAMP_DEV"] if dev else [])
                              + ["-o", so, _SRC])
    L = C.CDLL(so)
    L.plan_rows.restype = None
    assert L.plan_in_cols() == 11 and L.plan_out_cols() == len(HEAD) + 2 * len(REGIONS) and L.plan_dev() == int(dev)
    return L


def _plan(L, cols):
    a = np.ascontiguousarray(np.stack(cols, axis=1).astype(np.int64))
    out = np.empty((a.shape[0], L.plan_out_cols()), np.int64)
    L.plan_rows(C.c_long(a.shape[0]), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    d = {k: out[:, i] for i, k in enumerate(HEAD)}
    for j, r in enumerate(REGIONS):
        d[r + "_off"] = out[:, len(HEAD) + 2 * j]
        d[r] = out[:, len(HEAD) + 2 * j + 1]
    return d


def _sample():
    """A seeded sample of the cross product of AXES in which every value of every axis occurs."""
    rng = np.random.default_rng(20240611)
    s = {}
    for k, vals in AXES.items():
        v = np.asarray(vals, np.int64)
        col = v[rng.integers(0, v.size, ROWS)]
        col[:v.size] = v
        s[k] = rng.permutation(col)
    for k, vals in AXES.items():
        assert set(np.unique(s[k]).tolist()) == set(vals)
    return s


def _cdiv(a, b):
    return (a + b - 1) // b


def _fast_grid(n, cus, waves):
    rpb = np.maximum(_cdiv(_cdiv(n, cus), 64) * 64, 2 * waves * 64)
    return _cdiv(n, rpb), rpb


@pytest.fixture(scope="module", params=[False, True], ids=["shipped", "dev"])
def planned(request):
    L = _lib(request.param)
    k = np.empty(10, np.int64)
    L.plan_constants(k.ctypes.data_as(C.c_void_p))
    # the literals of the restated rules below are the header's constants
    assert k.tolist() == [8, 8, 7, 64, 12, 64, 256, 0x3FFFFFFF, 64, 8]
    s = _sample()
    s["n_cig"] = np.minimum(s["n"] * s["ops"], 0xFFFFFFF0)
    s["n_bases"] = s["n"] * s["pad"]
    p = _plan(L, [s["n"], s["n_cig"], s["n_bases"], s["window"], s["mq"], s["req"], s["n_cu"], s["share"], s["give_pos"], s["give_ncig"],
                  s["give_cig"]])
    assert p["ok"].all()
    return request.param, s, p


def test_routing_is_the_rule_it_replaced(planned):
    _, s, p = planned
    n, w, mq, req = s["n"], s["window"], s["mq"], s["req"]
    mean_pad = _cdiv(s["n_bases"], n)
    waves = np.where((mean_pad <= 152) | (w != 4), 8, np.where(mean_pad <= 192, 6, 4))
    mixed = (waves != 8) & (s["n_cig"] >= 3 * n)
    kv0 = np.where(req != 0, req, np.where(mixed, 7, np.where((waves == 8) & (w != 8), 4, 5)))
    kv1 = np.where((kv0 >= 4) & ((w > 8) | (mq > 128)), 2, kv0)
    kv = np.where((kv1 == 6) & (mq < 1), 4, kv1)
    variant = np.where(kv >= 5, 4, kv)
    long_kernel = (variant == 4) & (s["n_cig"] >= 8 * n)
    assert np.array_equal(p["f5_waves"], waves)
    assert np.array_equal(p["f5_qrun"], np.where(waves == 8, 9728, np.where(waves == 6, 13312, 19456)))
    assert np.array_equal(p["kv"], kv)
    assert np.array_equal(p["variant"], variant)
    assert np.array_equal(p["long_kernel"], long_kernel)
    assert np.array_equal(p["direct"], ~long_kernel & (p["fg_grid"] <= 256))
    assert np.array_equal(p["fast_path_active"], np.isin(req, (0, 4, 5, 6, 7)) & (w <= 8) & (mq <= 128))
    # every branch is in the sample
    assert set(np.unique(kv).tolist()) == {1, 2, 3, 4, 5, 6, 7} and long_kernel.any() and (~long_kernel & (variant == 4)).any()
    assert ((variant == 4) & ~long_kernel & (p["fg_grid"] > 256)).any(), "direct switched off by the fast grid alone (more than 256 CUs)"


def _grids(s, p):
    n = s["n"]
    fast_cus = np.maximum(1, s["n_cu"] // s["share"])
    kv = p["kv"]
    waves = np.where(kv == 5, p["f5_waves"], np.where(kv == 7, 7, 8))
    grid, rpb = _fast_grid(n, fast_cus, waves)
    n_tiles = _cdiv(n, 64)
    tpb = np.maximum(_cdiv(_cdiv(n_tiles, 32 * s["n_cu"]), 8) * 8, 8)
    tg = _cdiv(n_tiles, tpb)
    gen_grid = np.minimum(np.minimum(tg, 4 * s["n_cu"]), 1024)
    return fast_cus, grid, rpb, n_tiles, tpb, tg, gen_grid


def test_grids_are_the_formulas_they_replaced(planned):
    _, s, p = planned
    fast_cus, grid, rpb, _, tpb, tg, gen_grid = _grids(s, p)
    assert np.array_equal(p["fg_grid"], grid) and np.array_equal(p["fg_rpb"], rpb)
    assert np.array_equal(p["tg_grid"], tg) and np.array_equal(p["tg_tpb"], tpb)
    assert np.array_equal(p["gen_grid"], gen_grid)
    assert np.array_equal(p["heavy_grid"], np.minimum(tg, 2 * s["n_cu"]))
    # event-list slots on top of the batch's bound: what was reserved before (k_fast's waves, whichever kernel ran), or the open
    # granules of the waves of the kernel that runs where those are more
    kv = p["kv"]
    waves = np.where(kv == 5, p["f5_waves"], np.where(kv == 7, 7, np.where(kv >= 4, 8, 0)))
    assert np.array_equal(p["fast_waves"], waves)
    long_term = 2 * s["n_cu"] * 12 * 64
    before = _fast_grid(s["n"], fast_cus, 8)[0] * 8 * 64 + long_term
    assert np.array_equal(p["ev_fixed"], np.maximum(_fast_grid(s["n"], fast_cus, 8)[0] * 8, grid * waves) * 64 + long_term)
    assert (p["ev_fixed"] >= before).all()
    # a block holds at least 128 reads per wave, so a grid has at most n / 128 + its waves per block (<= 8) waves, and k_fast's
    # grid at least n / 128: the two differ by fewer than eight granules
    assert (p["ev_fixed"] - before <= 8 * 64).all()
    assert (p["ev_fixed"] > before).any()


def test_layout(planned):
    dev, s, p = planned
    n = s["n"]
    _, grid, rpb, n_tiles, tpb, tg, gen_grid = _grids(s, p)
    slots = s["n_cig"] + 3 * n
    gen_tpb_max = _cdiv(_cdiv(n_tiles, gen_grid), 8) * 8
    dlist_words = np.maximum((tg + 1) * tpb, n_tiles + gen_tpb_max + 8) * 64
    kv, v4, lk = p["kv"], p["variant"] == 4, p["long_kernel"] != 0
    # every region inside the buffer, no two of them overlap (a region without words lies nowhere)
    for r in REGIONS:
        assert (p[r] >= 0).all() and (p[r + "_off"] >= 0).all() and (p[r + "_off"] + p[r] <= p["total"]).all(), r
    for i, a in enumerate(REGIONS):
        for b in REGIONS[i + 1:]:
            apart = (p[a + "_off"] + p[a] <= p[b + "_off"]) | (p[b + "_off"] + p[b] <= p[a + "_off"]) | (p[a] == 0) | (p[b] == 0)
            assert apart.all(), (a, b)
    # each at least as long as its consumers index
    zero = np.zeros_like(n)
    need = {
        "pingpong": slots,                                         # k_reads_lane, the heavy pass: a slot per read
        "dlist": dlist_words,
        # amp_debug_blocks / amp_debug_counters read it to 6 * grid + 64; in -DAMP_DEV builds k_fast gets dcnt + grid + 64 for its
        # stamps: eight words per block, and six per wave (eight a block) from word 2048 on (F_STAMP_OUT, amp_fast.hpp)
        "dcnt": np.maximum(6 * tg + 64, np.where(dev & (kv == 4), tg + 64 + np.maximum(8 * grid, 2048 + 6 * 8 * grid), 0)),
        "split": np.where(p["variant"] == 3, 4 * n, zero),
        "new_pos": np.where(s["give_pos"] == 0, n, zero),
        "new_ncig": np.where(s["give_ncig"] == 0, n, zero),
        "new_cig": np.where(s["give_cig"] == 0, slots, zero),
        "glist": np.where(v4, grid * rpb, zero),
        "gcnt": np.where(v4, grid * 8, zero),
        "gdense": np.where(v4, _cdiv(n, 4) * 4, zero),
        "geo": np.where(v4, 4, zero),
        "segfirst": np.where(v4, 1024, zero),
        "llist": np.where(lk, n, zero),
        "lpos": np.where(lk, n, zero),
        "clist": np.where(kv == 6, grid * rpb, np.where(kv == 7, 2 * grid * rpb, zero)),
    }
    for r in REGIONS:
        assert (p[r] >= need[r]).all(), r
    assert ((p["geo_off"] - p["gdense_off"])[v4] % 4 == 0).all()       # GenGeo: a multiple of four words behind the dense list, as before
    # never more than the one expression that sized the buffer before
    fast_words = np.where(v4, grid * rpb + grid * 8 + n + 64 + 1024 + np.where(lk, 2 * n, 0)
                          + np.where(kv == 6, grid * rpb, np.where(kv == 7, 2 * grid * rpb, 0)), 0)
    before = slots * np.where(s["give_cig"] != 0, 1, 2) + 7 * n + 6 * tg + 64 + dlist_words + fast_words
    # (a development build adds k_fast's stamps, which overran the buffer on small batches before; they are no part of the shipped size)
    assert (p["total"] <= before + np.where(dev & (kv == 4), 2048 + 6 * 8 * grid, 0)).all()
    assert (p["total"] == sum(p[r] for r in REGIONS)).all()          # and nothing in it that is not a region


def test_a_batch_over_the_index_limit_has_no_plan():
    L = _lib()
    for n in (0x40000000, 0x7FFFFFFF, 0x80000000, 1 << 40):
        one = [np.array([v], np.int64) for v in (n, n, n * 152, 4, 20, 0, 256, 1, 1, 1, 1)]
        assert _plan(L, one)["ok"][0] == 0
    one = [np.array([v], np.int64) for v in (0x3FFFFFFF, 0x3FFFFFFF, 0x3FFFFFFF * 152, 4, 20, 0, 256, 1, 1, 1, 1)]
    assert _plan(L, one)["ok"][0] == 1
