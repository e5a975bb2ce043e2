"""The crafted read-pass cases (tests/readpass_craft.py) on the device, under the engine's own routing (variant 0) and under each
kernel on its own (4: k_fast, 5: k_fast5, 7: k_fast7, 2: k_tile): statuses, trims, count table and insertion events equal the
oracle's, AND the pass took the route the kernels' constants say -- the resolved variant, the reads on the general list
(debug_counters()[7]), the heavy entries of the second pass ([0]) and all deferred reads ([3]).  A fast kernel that hands a class
of reads to the exact generic code, or stops taking reads it should take, passes every parity check and fails these.

Every expected number comes from tests/readpass_craft.py route_facts(), which restates the kernels' rules; none from a device run."""
import numpy as np
import pytest

from oracle import oracle
from tests import readpass_craft as RC
from tests.gpu_util import GpuRunner, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runners():
    rs = {v: GpuRunner(variant=v) for v in RC.VARIANTS}
    yield rs
    for r in rs.values():
        r.close()


def tables(case):
    if not case.primers:
        return None, None, 0
    return oracle.find_overlapping_primers(case.G, case.primers, case.offset)


def both(runner, case, batch, mn, mx, mpl):
    a = oracle.process(batch, case.G, mn, mx, mpl, case.min_quality, case.window, do_trim=case.do_trim)
    d = runner.process(batch, case.G, mn, mx, mpl, case.min_quality, case.window, do_trim=case.do_trim)
    return a, d


def check_route(case, eng, batch, variant, facts=None):
    facts = facts or RC.route_facts(case, batch, variant)
    why = "%s, variant %d: %s" % (case.name, variant, case.expect["why"])
    assert eng.last_kernel_variant() == facts["kv"], why
    dc = [int(x) for x in eng.debug_counters()]
    print("%s variant %d -> %d: list %d (expected %r), heavy %d (expected %r), deferred %d" %
          (case.name, variant, facts["kv"], dc[7], facts["list"], dc[0], facts["heavy"], dc[3]))
    if facts["list"] is not None:
        lo, hi = facts["list"]
        assert lo <= dc[7] <= hi, why
    lo, hi = facts["heavy"]
    assert lo <= dc[0] <= hi, why
    # every deferred read is a heavy entry or a light one (indels left to do) of a read the second pass was given at all
    assert dc[0] <= dc[3] <= (facts["list"][1] if facts["list"] is not None else facts["n"]), why


@pytest.mark.parametrize("variant", RC.VARIANTS, ids=lambda v: "variant%d" % v)
@pytest.mark.parametrize("case", [c for c in RC.CASES if c.pile is None], ids=lambda c: c.name)
def test_crafted_case(runners, case, variant):
    runner = runners[variant]
    if len(runner.engines) >= 8 and case.G not in runner.engines:
        runner.close()          # (the cases have dozens of reference lengths: no need to keep an engine for each)
    mn, mx, mpl = tables(case)
    if case.fails:
        # the statuses of the whole batch first, then everything on the reads the oracle accepts
        b = case.batch()
        a, d = both(runner, case, b, mn, mx, mpl)
        assert_same(a, d, b, check_counts=False)
    good = case.accepted()
    a, d = both(runner, case, good, mn, mx, mpl)
    assert_same(a, d, good)
    check_route(case, runner.engine(case.G), good, variant)


@pytest.mark.parametrize("variant", RC.VARIANTS, ids=lambda v: "variant%d" % v)
@pytest.mark.parametrize("case", [c for c in RC.CASES if c.pile is not None], ids=lambda c: c.name)
def test_pile_at_the_counters_overflow_bound(runners, case, variant):
    """Family H: a pile so deep that every wave of the fast kernel counts more than two fold intervals of tiles into one packed
    window.  A late fold carries from one packed byte into the next: a wrong neighbouring base in the table."""
    if variant == 2:
        pytest.skip("the tile kernel counts into 32-bit LDS words: it has no packed bytes to overflow")
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    runner = runners[variant]
    kv = 4 if variant == 0 else variant          # (150-base reads, window 4: the engine's own routing takes k_fast)
    b = case.batch(RC.pile_reads(n_cu, kv))
    a = oracle.process(b, case.G, None, None, 0, case.min_quality, case.window)
    eng = runner.engine(case.G)
    try:
        eng.set_cu_share(16)
        d = runner.process(b, case.G, None, None, 0, case.min_quality, case.window)
        assert_same(a, d, b)
        check_route(case, eng, b, variant, dict(kv=kv, list=(0, 0), heavy=(0, 0), n=b.n))
    finally:
        eng.set_cu_share(1)
