"""The crafted read-pass cases (tests/readpass_craft.py) on the CPU: the list is sound against the oracle, the device's per-read
functions (amp_read.hpp / amp_bf.hpp, executed by tests/hostsim) agree with the oracle on every case, and the constants and
routing rules the cases are built on are the headers'.  tests/test_gpu_readpass_edges.py runs the same list on the device."""
import os
import re
import shutil

import numpy as np
import pytest

from oracle import oracle
from tests import readpass_craft as RC

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "amplipy_amd", "csrc")
EV_ORDER = ["ref_pos", "read", "q_from", "q_to"]
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build hostsim")


def tables(case):
    if not case.primers:
        return None, None, 0
    return oracle.find_overlapping_primers(case.G, case.primers, case.offset)


def run(fn, case, batch, **kw):
    mn, mx, mpl = tables(case)
    return fn(batch, case.G, mn, mx, mpl, case.min_quality, case.window, do_trim=case.do_trim, **kw)


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_the_list_is_sound(case):
    b = case.batch()
    a = run(oracle.process, case, b)
    refused = np.nonzero(a.trim.status)[0].tolist()
    assert refused == case.fails, "the oracle refuses %r, the case names %r" % (refused[:20], case.fails[:20])
    assert len(case.fails) <= 0.02 * b.n
    assert case.reach is not None and case.reach(b), "the boundary the case is about is not in its batch"
    good = case.accepted()
    a = run(oracle.process, case, good)
    assert not a.trim.status.any()
    if hasattr(case, "events"):
        assert a.events.size == case.events
    if case.family == "B" and "ends_of_range" in case.name:
        assert a.events.size > sum(1 for r in case.reads if any(o == RC.I for o, _ in r.cig))       # several events from one insertion
    if case.family == "C" and "no_qualities" not in case.name:
        aligned = sum(k for r in case.reads for o, k in r.cig if o in (RC.M, RC.EQ, RC.X))
        counted = int(a.counts[:, :5].sum())
        assert counted > 0, "no base of the case is counted"
        if case.min_quality > 0:
            assert counted < aligned, "no base of the case is skipped"
    if case.family == "H":
        # every read of the pile is counted at one position: one packed byte takes an increment per lane
        assert int(a.counts.sum(axis=1).max()) == good.n and int(a.counts.max()) >= good.n // 2
        assert not a.counts[:300].any() and not a.counts[300 + case.pile["L"] + 1:].any()


@needs_hipcc
@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_device_read_functions_agree_with_the_oracle(case):
    from tests import hostsim
    b = case.batch()
    a, d = run(oracle.process, case, b), run(hostsim.process, case, b)
    assert np.array_equal(a.trim.status, d.trim.status)
    ok = a.trim.status == 0
    assert np.array_equal(a.trim.new_pos[ok], d.trim.new_pos[ok])
    assert np.array_equal(a.trim.ref_len, d.trim.ref_len)
    assert np.array_equal(a.trim.trim_flags, d.trim.trim_flags)
    assert np.array_equal(a.trim.new_ncig, d.trim.new_ncig)
    assert np.array_equal(a.trim.compact_cigars(), d.trim.compact_cigars())
    if case.fails:
        b = case.accepted()
        a, d = run(oracle.process, case, b), run(hostsim.process, case, b)
        assert not a.trim.status.any() and not d.trim.status.any()
    assert np.array_equal(a.counts, d.counts)
    assert np.array_equal(np.sort(a.events, order=EV_ORDER), np.sort(d.events, order=EV_ORDER))


def test_every_family_and_boundary_value_is_on_the_list():
    assert {c.family for c in RC.CASES} == set("ABCDEFGHIJ")
    names = " ".join(c.name for c in RC.CASES)
    for G in RC.D_REFLEN:
        assert "D_reference_of_%d " % G in names + " "
    for n in RC.E_SIZES:
        assert "E_batch_of_%d " % n in names + " "
    for mq in RC.C_MINQ:
        assert "C_minq%d_" % mq in names
    # the fast-path rule, both sides
    kv = {c.name: RC.route_variant(0, c.batch(), c.window, c.min_quality) for c in RC.CASES if c.family == "C"}
    assert kv["C_window9_minq20"] == 2 and kv["C_window8_minq129"] == 2 and kv["C_window8_minq128"] in (4, 5, 7)
    assert all((v == 2) == ("minq129" in k or "minq255" in k or "window9" in k) for k, v in kv.items())


def test_the_constants_are_the_headers():
    def text(h):
        with open(os.path.join(_CSRC, h)) as f:
            return f.read()
    for h, names in RC.HEADER_CONSTANTS.items():
        for name, want in names.items():
            m = re.search(r"constexpr int %s = (\d+);" % name, text(h))
            assert m, (h, name)
            assert int(m.group(1)) == want, (h, name, m.group(1), want)
    for h, names in RC.HEADER_UINTS.items():
        for name, want in names.items():
            m = re.search(r"constexpr uint32_t %s = (\d+);" % name, text(h))
            assert m and int(m.group(1)) == want, (h, name)
    for h, names in RC.HEADER_MACROS.items():
        for name, want in names.items():
            m = re.search(r"#define %s (\d+)" % name, text(h))
            assert m and int(m.group(1)) == want, (h, name)
            assert re.search(r"constexpr int \w+ = %s;" % name, text(h)), (h, name)
    # the tile kernel's two length limits are literals of amp_tile.hpp
    t = text("amp_tile.hpp")
    assert "sumlen >= %du" % RC.TILE_SUMLEN in t and "(uint32_t)lseq >= %du" % RC.TILE_MAXLSEQ in t
    assert "ncig + 3 > T_MAXOPS" in t


def test_the_routing_rules_are_the_plan_headers():
    """fast5_cfg, fast_path_active and route_variant as restated in readpass_craft.py against amp_plan.hpp (tests/hostsim/plan_shim.cpp),
    on every case and on rows around each threshold; the pile of family H fills the grid it is computed for."""
    from tests.test_read_plan import _lib, _plan
    L = _lib()
    rows, want = [], []
    for c in RC.CASES:
        b = c.batch()
        for req in RC.VARIANTS:
            rows.append((b.n, int(b.cig_off[b.n]), int(b.seq_off[b.n]), c.window, c.min_quality, req, 256, 1))
            want.append((RC.route_variant(req, b, c.window, c.min_quality),) + RC.fast5_cfg(b.n, int(b.seq_off[b.n]), c.window)
                        + (int(RC.fast_path_active(req, c.window, c.min_quality)),))
    for pad in (RC.F5_PAD_SHORT, RC.F5_PAD_SHORT + 8, RC.F5_PAD_MID, RC.F5_PAD_MID + 8):
        for w in (4, 8, 9):
            for mq in (128, 129):
                for ops in (1, 3):
                    for req in RC.VARIANTS:
                        n = 1000
                        rows.append((n, n * ops, n * pad, w, mq, req, 256, 1))
                        waves, run_ = RC.fast5_cfg(n, n * pad, w)
                        mixed = waves != 8 and ops >= 3
                        kv0 = req if req else (7 if mixed else 4 if (waves == 8 and w != 8) else 5)
                        kv = 2 if kv0 >= 4 and not RC.fast_path_active(kv0, w, mq) else kv0
                        want.append((kv, waves, run_, int(RC.fast_path_active(req, w, mq))))
    a = np.array(rows, np.int64)
    p = _plan(L, [a[:, k] for k in range(8)] + [np.ones(len(rows), np.int64)] * 3)
    got = list(zip(p["kv"].tolist(), p["f5_waves"].tolist(), p["f5_qrun"].tolist(), p["fast_path_active"].tolist()))
    assert got == want
    assert {RC.F5_RUN_SHORT, RC.F5_RUN_MID, RC.F5_RUN_LONG} == set(p["f5_qrun"].tolist())
    # the pile: with a sixteenth of the CUs every block of the fast kernel holds 2 F_FLUSH + 2 tiles per wave
    for n_cu in (256, 304, 64):
        for kv in (4, 5, 7):
            n = RC.pile_reads(n_cu, kv)
            one = [np.array([v], np.int64) for v in (n, n, n * 152, 4, 20, kv, n_cu, 16, 1, 1, 1)]
            q = _plan(L, one)
            assert q["kv"][0] == kv and q["fg_grid"][0] * q["fast_waves"][0] * (2 * RC.F_FLUSH + 2) * RC.TILE == n
    assert RC.pile_reads(256, 4) == 262144
