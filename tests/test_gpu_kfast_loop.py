"""k_fast's tile loop after its scalar spills and select chains were cut down (amp_fast.hpp): the arguments the loop reads late from
the kernarg page, the CIGAR emission, the first quality byte read from the staged run, the loop's edges.

Every batch is compared with the oracle on statuses, the six per-read outputs (CIGAR words included), the count table and the
insertion events, under kernel variant 4 (k_fast) and variant 2 (the general kernel alone, the second witness).  Expected numbers
come from the batches and the kernels' constants (tests/readpass_craft.py), none from a device run."""
import itertools

import numpy as np
import pytest

from amplipy_amd import abi
from oracle import oracle
from tests import readpass_craft as RC
from tests.gpu_util import EV_ORDER, GpuRunner, assert_same

pytestmark = pytest.mark.gpu

M, I, D, S = RC.M, RC.I, RC.D, RC.S
VARIANTS = (4, 2)
FIELDS = ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")


@pytest.fixture(scope="module")
def runners():
    rs = {v: GpuRunner(variant=v) for v in VARIANTS}
    yield rs
    for r in rs.values():
        r.close()


def run_both(runners, batch, G, primers=(), mq=20, w=4, do_trim=True, do_count=True, read_base=0, check_counts=True):
    """The oracle once, then both variants; returns the oracle's result and the engines' general-list lengths by variant."""
    mn, mx, mpl = oracle.find_overlapping_primers(G, list(primers), 0) if primers else (None, None, 0)
    a = oracle.process(batch, G, mn, mx, mpl, mq, w, do_trim=do_trim, do_count=do_count, read_base=read_base)
    listed = {}
    for v in VARIANTS:
        d = runners[v].process(batch, G, mn, mx, mpl, mq, w, do_trim=do_trim, do_count=do_count, read_base=read_base)
        assert_same(a, d, batch, check_counts=check_counts)
        eng = runners[v].engine(G)
        assert eng.last_kernel_variant() == v
        listed[v] = int(eng.debug_counters()[7])
    return a, listed


def mixed_reads(n, seed, ins_every=10, base=100):
    """n reads in coordinate order: one-op reads with one-insertion and one-deletion reads among them, both strands, low tails."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        pos = base + 280 * (i * 4 // max(n, 4)) + i % 3
        if i % ins_every == 0:
            cig = [(M, 30), (I, 2), (M, 118)] if i % (2 * ins_every) else [(M, 70), (D, 3), (M, 80)]
        else:
            cig = [(M, 150)]
        reads.append(RC.mk(rng, pos, cig, flag=16 * (i % 2), low_tail=(i % 7) * 2))
    return RC.by_pos(reads)


# ---- late-loaded arguments ---------------------------------------------------------------------------------------------------------
def _device_batch(b):
    import torch
    from amplipy_amd import synth_torch
    d = synth_torch.DeviceBatch.from_host(b, "cuda:0")
    n = b.n
    out = {k: torch.full((max(sz, 1),), 0x5A, dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", d.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    return d, out


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "variant%d" % v)
def test_every_combination_of_output_pointers(runners, variant):
    """200 reads through amp_process_batch_device with each of the 64 subsets of the six output pointers: the outputs that are
    given equal the oracle's, the ones that are not stay untouched, table and events are the same in every run."""
    import torch
    G = 1400
    b = RC.build_batch(mixed_reads(200, 11, ins_every=5))
    primers = [(100, 125), (380, 400), (660, 690)]
    mn, mx, mpl = oracle.find_overlapping_primers(G, primers, 0)
    a = oracle.process(b, G, mn, mx, mpl, 20, 4)
    assert not a.trim.status.any() and a.events.size > 10
    want_ev = np.sort(a.events, order=EV_ORDER)
    eng = runners[variant].engine(G)
    eng.set_primers(mn, mx, mpl)
    eng.set_params(20, 4, True, True)
    d, out = _device_batch(b)
    for r in range(7):
        for given in itertools.combinations(FIELDS, r):
            drop = tuple(k for k in FIELDS if k not in given)
            for t in out.values():
                t.fill_(0x5A)
            eng.reset()
            eng.process_device(d.struct(), 0, None if not given else
                               abi.AmpTrimOut(*[None if k in drop else out[k].data_ptr() for k in FIELDS]))
            eng.sync()
            why = "outputs given: %s" % (given,)
            assert np.array_equal(eng.counts(), a.counts), why
            assert np.array_equal(np.sort(eng.events(), order=EV_ORDER), want_ev), why
            got = abi.TrimResult(b)
            for k in FIELDS:
                h = out[k].cpu().numpy()
                if k in drop:
                    assert (h == 0x5A).all(), why + ": %s written though absent" % k
                else:
                    getattr(got, k)[:] = h[:getattr(got, k).size].view(getattr(got, k).dtype)
            for k in given:
                if k == "new_cig":
                    if "new_ncig" in given:
                        assert np.array_equal(got.compact_cigars(), a.trim.compact_cigars()), why
                else:
                    assert np.array_equal(getattr(got, k), getattr(a.trim, k)), why + ": " + k
            if "new_cig" in given and "new_ncig" not in given:       # the slots by the oracle's counts
                got.new_ncig[:] = a.trim.new_ncig
                assert np.array_equal(got.compact_cigars(), a.trim.compact_cigars()), why
    torch.cuda.synchronize()


def test_read_base_above_32_bits(runners):
    """read_base + i carries into the high word inside the batch: an event's read id is the sum's low word."""
    b = RC.build_batch(mixed_reads(200, 12, ins_every=4))
    a, _ = run_both(runners, b, 1400, read_base=(1 << 33) - 100)
    assert a.events.size > 20
    ids = a.events["read"].astype(np.int64)
    assert (ids >= (1 << 32) - 100).any() and (ids < 100).any()


def test_granule_refill(runners):
    """Sixteen tiles of 64 one-event insertions on a fresh engine (its event list at the default capacity): a wave that takes a second
    such tile has used its granule of F_EVGRAN slots up and reserves another; the list grows behind the pass."""
    rng = np.random.default_rng(13)
    reads = []
    for t in range(16):
        reads += RC._ins_tile(rng, 200 + t, [1] * 64)
    b = RC.build_batch(reads)
    assert b.n > RC.F_WAVES * RC.F_EVGRAN            # more events than one granule per wave of a block holds
    fresh = {v: GpuRunner(variant=v) for v in VARIANTS}
    try:
        a, listed = run_both(fresh, b, 600, read_base=(1 << 32) + 7)
    finally:
        for r in fresh.values():
            r.close()
    assert a.events.size == b.n and listed[4] == 0


# ---- CIGAR emission ----------------------------------------------------------------------------------------------------------------
EMIT_LANES = (0, 29, 63)


def _emission_reads(rng, lane_of_special):
    """Tiles of 64 plain reads with one crafted read each at the given lane.  The crafted reads: every input form
    [S a] M ([I|D k] M) [S c]; the same under a left primer (a clip made by the primer trim, through the first match op up to the
    indel and past it), under low tails of every length up to the whole read on either strand (clips made by the quality trim: in
    front of the indel, inside it, through it, the whole read)."""
    specials = []
    for kind in (None, I, D):
        for a, c in ((0, 0), (4, 0), (0, 5), (4, 5)):
            body = [(M, 90)] if kind is None else [(M, 40), (kind, 3), (M, 50)]
            cig = ([(S, a)] if a else []) + body + ([(S, c)] if c else [])
            for flag in (0, 16):
                specials.append(dict(cig=cig, flag=flag, low=0, primed=False))
                specials.append(dict(cig=cig, flag=flag, low=0, primed=True))
            if kind is not None:
                # aligned query bases: m1 = 40, the insertion 3, m2 = 50.  Low tails that end around the indel from the 3' end
                for low in (c + 49, c + 50, c + 51, c + 53, c + 54, c + 60, c + 92, 39 + a, 40 + a, 41 + a, 43 + a, 44 + a):
                    for flag in (0, 16):
                        specials.append(dict(cig=cig, flag=flag, low=low, primed=False))
            else:
                for low in (1, 30, 89, 90, 90 + a + c):
                    for flag in (0, 16):
                        specials.append(dict(cig=cig, flag=flag, low=low, primed=False))
    reads, where = [], []
    for k, sp in enumerate(specials):
        pos0 = 1000 if sp["primed"] else 300
        for lane in range(64):
            if lane == lane_of_special:
                L = RC.query_len(sp["cig"])
                q = np.full(L, 40, np.uint8)
                if sp["low"]:
                    n_low = min(sp["low"], L)
                    if sp["flag"] & 16:
                        q[:n_low] = 2
                    else:
                        q[L - n_low:] = 2
                where.append(len(reads))
                reads.append(RC.mk(rng, pos0, sp["cig"], flag=sp["flag"], qual=q))
            else:
                reads.append(RC.mk(rng, pos0, [(M, 100)]))
    order = sorted(range(len(reads)), key=lambda i: reads[i].pos)        # (stable: the tiles stay whole, the unprimed ones first)
    return [reads[i] for i in order], len(specials)


def _forms(trim, idx):
    ops = "MIDNSHP=X"
    return {"".join(ops[o] for o, _ in trim.cigar_ops(int(i))) for i in idx}


@pytest.mark.parametrize("lane", EMIT_LANES, ids=lambda l: "lane%d" % l)
def test_cigar_emission_every_combination_of_parts(runners, lane):
    rng = np.random.default_rng(20 + lane)
    reads, n_special = _emission_reads(rng, lane)
    b = RC.build_batch(reads)
    # left primers end 35, 40, 41, 43 and 60 bases into the primed reads (position 1000): in front of the indel, on it, inside, behind
    primers = [(990, 1034), (990, 1039), (990, 1040), (990, 1042), (990, 1059)]
    a, _ = run_both(runners, b, 1400, primers=primers)
    special = np.nonzero(np.arange(b.n) % 64 == lane)[0]
    forms = _forms(a.trim, special)
    print("emitted forms:", sorted(forms))
    # every subset of parts the shape family can leave behind, ncig 1 to 5, both indel kinds
    assert {"M", "SM", "MS", "SMS", "MIM", "MDM", "SMIM", "SMDM", "MIMS", "MDMS", "SMIMS", "SMDMS", "S"} <= forms
    # ... and the ones a clip leaves that ends on the indel: no first match op, or no second
    assert {"SIM", "SDM", "SIMS", "SDMS", "MIS", "MDS", "SMIS", "SMDS"} <= forms
    assert {1, 2, 3, 4, 5} <= set(a.trim.new_ncig[special].tolist())
    flags = a.trim.trim_flags[special]
    assert (flags & abi.TRIM_QUALITY).any() and (flags & abi.TRIM_PRIMER_START).any()


# ---- first quality byte ------------------------------------------------------------------------------------------------------------
FB_LENGTHS = (1, 8, 9, 16, 17, 137, 144, 145, 152)


def _first_byte_reads(with_star):
    """One tile per (length, lane): 64 plain reads, at `lane` a read of that length whose qualities are all 0xFF (QUAL '*'; left out
    without ``with_star``), at lane + 32 a read of that length whose first quality is low."""
    rng = np.random.default_rng(30)
    reads, stars = [], []
    t = 0
    for L in FB_LENGTHS:
        for lane in range(64):
            pos = 100 + t // 16
            for l in range(64):
                if l == lane:
                    if with_star:
                        stars.append(len(reads))
                        reads.append(RC.mk(rng, pos, [(M, L)], qual=np.full(L, 0xFF, np.uint8)))
                    else:
                        reads.append(RC.mk(rng, pos, [(M, 100)]))
                elif l == (lane + 32) % 64:
                    q = np.full(L, 40, np.uint8); q[0] = 2
                    reads.append(RC.mk(rng, pos, [(M, L)], flag=16 * (lane % 2), qual=q))
                else:
                    reads.append(RC.mk(rng, pos, [(M, 100)]))
            t += 1
    return reads, stars


def test_first_quality_byte_every_lane(runners):
    reads, stars = _first_byte_reads(True)
    assert len(stars) == len(FB_LENGTHS) * 64 and {i % 64 for i in stars} == set(range(64))
    b = RC.build_batch(reads)
    # the whole batch: the oracle refuses the reads without qualities and nothing else; k_fast lists exactly those
    a, listed = run_both(runners, b, 900, check_counts=False)
    assert np.array_equal(np.nonzero(a.trim.status)[0], stars)
    assert listed[4] == len(stars)
    # the same tiles with a plain read in the starred lane: the reads whose first quality is merely low stay with k_fast
    reads, _ = _first_byte_reads(False)
    a, listed = run_both(runners, RC.build_batch(reads), 900)
    assert listed[4] == 0 and not a.trim.status.any()


# ---- loop edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (64, 65, 128, 192, 576, 1088))
def test_blocks_of_few_tiles(runners, n):
    """1, 2, 3, 9 and 17 tiles (1,088 reads: two blocks), and 65 reads: a last tile with one live lane."""
    a, listed = run_both(runners, RC.build_batch(mixed_reads(n, 40 + n)), 1400, primers=[(100, 122), (940, 960)])
    assert listed[4] == 0 and a.events.size > 0


@pytest.mark.parametrize("do_trim,do_count", ((False, True), (True, False)), ids=("trim_off", "count_off"))
def test_trim_off_and_count_off(runners, do_trim, do_count):
    a, listed = run_both(runners, RC.build_batch(mixed_reads(192, 50)), 1400, primers=[(100, 122)], do_trim=do_trim, do_count=do_count)
    assert listed[4] == 0
    assert bool(a.counts.any()) == do_count and bool(a.trim.trim_flags.any()) == do_trim


@pytest.mark.parametrize("w", (1, 4, 7, 8))
def test_windows(runners, w):
    a, listed = run_both(runners, RC.build_batch(mixed_reads(192, 60)), 1400, primers=[(100, 122)], w=w)
    assert listed[4] == 0 and (a.trim.trim_flags & abi.TRIM_QUALITY).any()
