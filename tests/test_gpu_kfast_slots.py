"""k_fast after its trims were rewritten as arithmetic on the five lengths (amp_bf.hpp) and its tile loop lost scalar-side
instructions (amp_fast.hpp): the whole shape family [S a][M m1]([I|D k][M m2])[S c] at SHORT lengths -- reads of 24 to 40 bases, so
that every clip of a few bases lands on one of the family's edges -- with primer-table entries and low-quality tails that put the end
of a clip on each place around the indel.

Every batch is compared with the oracle on statuses, the six per-read outputs (CIGAR words included), the count table and the
insertion events, under kernel variant 4 (k_fast) and variant 2 (the general kernel alone, the second witness).  The primer tables
are written entry by entry (min_start / max_end per position), not derived from a primer list: every read gets the entry its case
asks for.  The general list's length is counted from the batch: the reads outside the family (tests/readpass_craft.py::shape_ok);
over whole trims the closed forms hand nothing else over -- a primer clip cannot end inside an insertion (get_pos_on_query maps
no reference position there), so no clip meets an indel that already touches the far clip (tests/hostsim/bf_forms_main.cpp walks
all trims of the small domain and finds no punted one).  Expected values come from the oracle and the batches, none from a device
run.  About 11,000 distinct reads, 18,000 with the quality batch's nine runs."""
import numpy as np
import pytest

from oracle import oracle
from tests import readpass_craft as RC
from tests.gpu_util import GpuRunner, assert_same

pytestmark = pytest.mark.gpu

M, I, D, S = RC.M, RC.I, RC.D, RC.S
VARIANTS = (4, 2)
MPL = 30                                   # max_primer_len of the crafted tables: |tlen| - MPL > l_seq is the test of A:452
CLIPS = (0, 1, 7)
INDELS = ((None, 0), (I, 1), (I, 2), (I, 8), (D, 1), (D, 2), (D, 16))
# unpaired; paired with the template-length test on (the far primer is left alone) and off; each on both strands
FLAGS = tuple((paired | strand, tlen) for strand in (0, 16) for paired, tlen in ((0, 0), (1, 200), (1, 40)))
Q_HI, Q_LO = 200, 0                        # good and low under every min_quality of the tests (1, 20, 128); 0xFF would be QUAL '*'


@pytest.fixture(scope="module")
def runners():
    rs = {v: GpuRunner(variant=v) for v in VARIANTS}
    yield rs
    for r in rs.values():
        r.close()


def run_both(runners, reads, G, mn=None, mx=None, mq=20, w=4):
    """The oracle once, then both variants; k_fast's general list holds exactly the reads outside the family."""
    b = RC.build_batch(reads)
    none = np.full(G, -1, np.int32)
    mn = none if mn is None else mn
    mx = none if mx is None else mx
    a = oracle.process(b, G, mn, mx, MPL, mq, w)
    assert not a.trim.status.any()
    off = int(RC.off_limit(b, RC.F_MAXLEN).sum())
    for v in VARIANTS:
        d = runners[v].process(b, G, mn, mx, MPL, mq, w)
        assert_same(a, d, b)
        eng = runners[v].engine(G)
        assert eng.last_kernel_variant() == v
        if v == 4:
            assert int(eng.debug_counters()[7]) == off, "general list: %d reads, %d outside the family" % (int(eng.debug_counters()[7]), off)
    return a, b


def shape(L, kind, k, a, c):
    """(cigar, m1, m2) of l_seq L: the indel in the middle of the aligned bases."""
    body = L - a - c - (k if kind == I else 0)
    assert body >= 10 and 24 <= L <= 40
    if kind is None:
        return ([(S, a)] if a else []) + [(M, body)] + ([(S, c)] if c else []), body, 0
    m1 = body // 2
    return ([(S, a)] if a else []) + [(M, m1), (kind, k), (M, body - m1)] + ([(S, c)] if c else []), m1, body - m1


def shapes():
    """The 63 shapes, lengths 24 to 40 in turn."""
    out = []
    for kind, k in INDELS:
        for a in CLIPS:
            for c in CLIPS:
                L = max(24 + len(out) % 17, a + c + (k if kind == I else 0) + 10)      # at least ten aligned bases
                cig, m1, m2 = shape(L, kind, k, a, c)
                out.append((cig, kind, k, a, c, m1, m2))
    return out


def off_family(rng, pos):
    """A read the closed forms do not take (two indels): it must come back through the general list."""
    return RC.mk(rng, pos, [(M, 10), (I, 1), (M, 8), (D, 2), (M, 9)], q=Q_HI)


def primer_places(kind, k, a, m1, m2):
    """Reference bases t = max_end + 1 - pos (mirrored: from the read's end) a primer covers, so that its clip ends: with `del'
    negative and 0, before the indel, on the last base of m1, exactly in front of the indel, inside the deletion and on its last base
    (an insertion holds no reference position), one base behind the indel, inside m2, on the last base of m2 and behind it."""
    kd = k if kind == D else 0
    t = {-a - 2, -a, max(m1 - 3, 1), m1 - 1, m1}
    if kind is not None:
        t |= {m1 + 1, m1 + kd, m1 + kd + 1, m1 + kd + m2 // 2, m1 + kd + m2 - 1}
    t |= {m1 + kd + m2, m1 + kd + m2 + 2}
    return sorted(t)


def primer_batch(right):
    """One start position (right: one end position) per shape and place, six reads on it: the entry of that position puts the
    clip where the case wants it.  Returns (reads, G, min_start, max_end)."""
    rng = np.random.default_rng(71 + right)
    cases = []
    for sh in shapes():
        cig, kind, k, a, c, m1, m2 = sh
        if right and kind is not None:                 # seen from the read's end
            a, c, m1, m2 = c, a, m2, m1
        elif right:
            a, c = c, a
        cases += [(sh, t) for t in primer_places(kind, k, a, m1, m2)]
    G = 40 + 2 * len(cases) + 80
    assert G <= 2000
    mn, mx = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    reads = []
    for n, ((cig, kind, k, a, c, m1, m2), t) in enumerate(cases):
        span = RC.ref_span(cig)
        if not right:
            pos = 40 + 2 * n
            mx[pos] = pos + t - 1                      # the left primer's last base: t bases of the read's reference span
        else:
            end = 40 + 60 + 2 * n                      # the read's last reference position
            pos = end - span + 1
            mn[end] = end - t + 1                      # the right primer's first base: t bases from the read's end
        assert pos >= 20 and pos + span + 2 < G and mx[pos] >= -1
        for flag, tlen in FLAGS:
            reads.append(RC.mk(rng, pos, cig, flag=flag, tlen=tlen, q=Q_HI))
        if n % 40 == 0:
            reads.append(off_family(rng, pos))
    assert (mx[mx >= 0] >= 0).all() and (mn >= -1).all()
    return RC.by_pos(reads), G, mn, mx


@pytest.mark.parametrize("right", (0, 1), ids=("left_primer", "right_primer"))
def test_primer_clip_on_every_place(runners, right):
    reads, G, mn, mx = primer_batch(right)
    a, b = run_both(runners, reads, G, mn, mx)
    flags = a.trim.trim_flags
    want = 2 if right else 1                           # AMP_TRIM_PRIMER_END / AMP_TRIM_PRIMER_START
    assert 0.3 < (flags & want).astype(bool).mean() < 0.9          # (the template-length test spares a third of the paired reads' far primers)
    assert {1, 2, 3, 4, 5} <= set(a.trim.new_ncig.tolist())
    assert a.events.size > 50 and b.n > 3500


def quality_batch():
    """Low tails at the 3' end of the read direction (forward: the right end, reverse: the left end) of every length from five bases
    in front of the indel to five behind it, one base, the whole aligned part less one and the whole of it."""
    rng = np.random.default_rng(73)
    reads = []
    for cig, kind, k, a, c, m1, m2 in shapes():
        if 1 in (a, c):
            continue
        L = RC.query_len(cig)
        ki = k if kind == I else 0
        aligned = L - a - c
        for flag in (0, 16):
            near = m1 if flag else (m2 if kind is not None else m1)
            lows = {1, aligned - 1, aligned} | set(range(max(near - 5, 1), min(near + ki + 5, aligned) + 1))
            for n_low in sorted(lows):
                q = np.full(L, Q_HI, np.uint8)
                if flag:
                    q[a:a + n_low] = Q_LO
                else:
                    q[L - c - n_low:L - c] = Q_LO
                reads.append(RC.mk(rng, 100 + (len(reads) * 5) % 700, cig, flag=flag, qual=q))
            if len(reads) % 7 == 0:
                reads.append(off_family(rng, 100 + (len(reads) * 5) % 700))
    return RC.by_pos(reads)


@pytest.fixture(scope="module")
def quality_reads():
    return quality_batch()


@pytest.mark.parametrize("mq", (1, 20, 128))
@pytest.mark.parametrize("w", (1, 4, 7))
def test_quality_clip_on_every_place(runners, quality_reads, w, mq):
    a, b = run_both(runners, quality_reads, 900, mq=mq, w=w)
    trimmed = (a.trim.trim_flags & 4).astype(bool)     # AMP_TRIM_QUALITY
    assert 0.5 < trimmed.mean() < 1.0
    assert b.n < 1000


def forms(trim, idx):
    ops = "MIDNSHP=X"
    return {"".join(ops[o] for o, _ in trim.cigar_ops(int(i))) for i in idx}


def test_quality_clip_leaves_every_form(runners, quality_reads):
    """Window 1 cuts exactly at the first good base: the clip ends on every place, the indel directly behind or in front of a clip
    included (the forms without a first or a second match op)."""
    a, _ = run_both(runners, quality_reads, 900, mq=20, w=1)
    got = forms(a.trim, range(a.trim.new_ncig.size))
    assert {"S", "M", "SM", "MS", "SMS", "MIM", "MDM", "SIM", "SDM", "MIS", "MDS", "SMIS", "SMDS", "SIMS", "SDMS", "SMIMS", "SMDMS"} <= got


@pytest.mark.parametrize("n", (1, 63, 64, 65, 2 * 8 * 64 - 1, 2 * 8 * 64 + 1))
def test_lanes_past_the_batch(runners, n):
    """Batches that end inside a tile, on its edge and one read behind it, one tile and two blocks' worth: primers on both sides
    and low tails at once, the reads of the left-primer batch with every third one's tail lowered."""
    reads, G, mn, mx = primer_batch(0)
    rng = np.random.default_rng(75)
    picked = [reads[i] for i in sorted(rng.choice(len(reads), n, replace=False).tolist())]
    for j, r in enumerate(picked):
        if j % 3 == 0:
            if r.flag & 16:
                r.qual[:5 + j % 9] = Q_LO
            else:
                r.qual[r.lseq - 5 - j % 9:] = Q_LO
        end = r.pos + RC.ref_span(r.cig) - 1
        if j % 4 == 0 and mn[end] < 0:
            mn[end] = end - 3
    a, b = run_both(runners, picked, G, mn, mx)
    assert b.n == n
