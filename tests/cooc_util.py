"""TEST INFRASTRUCTURE of the co-occurrence tallies: a plain restatement of the table, written from the
definitions and from nothing in amplipy_amd/csrc -- per read the aligned pairs of the counted CIGAR become a map
{reference position: (base, quality)} and a set of deleted positions, and the rules are applied with Python sets; the checks
that pin it to the reference-pinned oracle's count table; set lists and crafted reads the tests share."""
import numpy as np

from amplipy_amd.batch import ReadBatch
from tests import codon_util as CU
from tests import strand_util as S

CELLS = 65
PARTIAL = 64
SITES = 6
BASES = "ACGT"
MUT, NOT, NONE = "MUT", "NOT", "NONE"


def sub(p, b):
    """A substitution site: 0-based position, base letter."""
    return (int(p), 0, BASES.index(b))


def dele(p, n):
    """A deletion site: the positions [p, p + n)."""
    return (int(p), int(n), 0)


class SetList:
    """Sets of sites (p, len, sym) as the engine takes them: the sites of a set by position, the sets by their first site
    (equal ones in the order given).  ``sets``: the sorted list; the four arrays of lib.Engine.cooc_enable."""

    def __init__(self, sets):
        self.sets = sorted([sorted(s) for s in sets], key=lambda s: s[0][0])
        self.set_off = np.cumsum([0] + [len(s) for s in self.sets]).astype(np.int32)
        flat = [site for s in self.sets for site in s]
        self.site_pos = np.array([x[0] for x in flat], np.int32)
        self.site_len = np.array([x[1] for x in flat], np.int32)
        self.site_sym = np.array([x[2] for x in flat], np.uint8)
        self.at = {}                        # position of a site -> the sets that have one there
        for k, s in enumerate(self.sets):
            for p, _, _ in s:
                self.at.setdefault(p, set()).add(k)

    @property
    def n_sets(self):
        return len(self.sets)

    def arrays(self):
        return self.set_off, self.site_pos, self.site_len, self.site_sym

    def index(self, s):
        """The row of the (first) set equal to ``s``."""
        return self.sets.index(sorted(s))


# ---- the restatement --------------------------------------------------------------------------------------------------------
def alignment(seg):
    """-> ({reference position: (base, quality)}, deleted positions, pos, ref_end) of the read's counted CIGAR."""
    seq, qual = seg.query_sequence.upper(), seg.query_qualities
    base, deleted = {}, set()
    q, r = 0, seg.reference_start
    for op, n in seg.cigartuples:
        if op in (0, 7, 8):
            for k in range(n):
                base[r + k] = (seq[q + k], qual[q + k])
            q += n; r += n
        elif op in (1, 4):
            q += n
        elif op in (2, 3):
            deleted.update(range(r, r + n))
            r += n
    return base, deleted, seg.reference_start, r


def site_state(site, base, deleted, pos, end, min_quality):
    p, n, sym = site
    if n == 0:
        if p in deleted:
            return NOT
        if p in base and base[p][0] in BASES and base[p][1] >= min_quality:
            return MUT if base[p][0] == BASES[sym] else NOT
        return NONE
    if not (pos <= p - 1 < end and pos <= p + n < end):
        return NONE
    if set(range(p, p + n)) <= deleted and (p - 1) not in deleted and (p + n) not in deleted:
        return MUT
    return NOT


def read_adds(seg, ref_len, setlist, min_quality):
    """[(set, cell)] of a read with status 0, or None when the read is not regular."""
    if not CU.is_regular(seg, ref_len):
        return None
    base, deleted, pos, end = alignment(seg)
    near = set()                            # a site that is not NONE lies inside [pos, end)
    for r in range(pos, end):
        near |= setlist.at.get(r, set())
    out = []
    for k in sorted(near):
        states = [site_state(site, base, deleted, pos, end, min_quality) for site in setlist.sets[k]]
        if all(s != NONE for s in states):
            out.append((k, sum(1 << j for j, s in enumerate(states) if s == MUT)))
        elif any(s != NONE for s in states):
            out.append((k, PARTIAL))
    return out


def tables(segments, ref_len, setlist, min_quality):
    """(cooc uint32[n_sets][65], reads uint64[2]) of reads with status 0, Python integers all the way."""
    cooc = [[0] * CELLS for _ in setlist.sets]
    reads = [0, 0]
    for seg in segments:
        adds = read_adds(seg, ref_len, setlist, min_quality)
        reads[adds is None] += 1
        for k, cell in adds or ():
            cooc[k][cell] += 1
    return np.array(cooc, np.uint32).reshape(len(setlist.sets), CELLS), np.array(reads, np.uint64)


def all_regular(segments, ref_len):
    return all(CU.is_regular(s, ref_len) for s in segments)


# ---- the oracle's word on the table -----------------------------------------------------------------------------------------
def single_sites(lo, hi):
    """{(p, b)} for every p in [lo, hi) and every b: set 4 (p - lo) + b."""
    return SetList([[(p, 0, b)] for p in range(lo, hi) for b in range(4)])


def check_single_sites(cooc, lo, hi, counts, exact):
    """Single-site sets over [lo, hi): the reads that show b at p are counts[p][b] of the ORACLE's table, and those that show
    anything there -- a good base among A C G T, or a deletion -- its A + C + G + T + '-'.  ``exact``: every live read of the
    batch is regular (else the table may fall short of the oracle's, never exceed it)."""
    c = np.asarray(cooc).astype(np.int64).reshape(hi - lo, 4, CELLS)
    assert not c[:, :, 2:].any()            # one site: patterns 0 and 1 only, and never partial
    cnt = counts[lo:hi].astype(np.int64)
    shown = cnt[:, [0, 1, 2, 3, 5]].sum(axis=1)
    if exact:
        assert np.array_equal(c[:, :, 1], cnt[:, :4])
        assert np.array_equal(c[:, :, 0] + c[:, :, 1], np.repeat(shown[:, None], 4, axis=1))
    else:
        assert (c[:, :, 1] <= cnt[:, :4]).all() and (c[:, :, 0] + c[:, :, 1] <= shown[:, None]).all()


# ---- set lists --------------------------------------------------------------------------------------------------------------
def mixed_sets(ref_len, n_anchor=40, seed=3):
    """Round ``n_anchor`` anchors spread over the reference: a single site, pairs that share it, nested sets of three to six
    sites with a deletion among them, sets with equal first positions, a set wider than a read."""
    rng = np.random.default_rng(seed)
    b = lambda: BASES[int(rng.integers(0, 4))]
    sets = []
    step = max(ref_len // n_anchor, 1)
    for a in range(2, ref_len - 1, step):
        room = ref_len - a
        cand = [[sub(a, b())]]
        if room > 12:
            cand += [[sub(a, b()), sub(a + 5, b())], [sub(a + 5, b()), sub(a + 9, b())], [dele(a + 6, 2), sub(a + 9, b())],
                     [sub(a, b()), dele(a + 2, 3), sub(a + 5, b())]]
        if room > 130:
            cand += [[sub(a, b()), sub(a + 5, b()), sub(a + 40, b()), dele(a + 60, 1)],
                     [sub(a + 1, b()), sub(a + 5, b()), dele(a + 20, 4), sub(a + 40, b()), sub(a + 90, b()), sub(a + 120, b())],
                     [dele(a + 1, 1), sub(a + 120, b())]]
        if room > 700:
            cand += [[sub(a, b()), sub(a + 650, b())]]
        sets += cand
    return SetList(sets)


def many_sets(n_sets, ref_len, seed=4):
    """``n_sets`` two-site sets spread evenly over the reference (more than a window holds)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_sets):
        a = 1 + (ref_len - 40) * k // n_sets
        out.append([sub(a, BASES[int(rng.integers(0, 4))]), sub(a + 1 + int(rng.integers(1, 30)), BASES[int(rng.integers(0, 4))])])
    return SetList(out)


# ---- crafted reads ----------------------------------------------------------------------------------------------------------
def _read(pos, cigar, seq, qual=35, flag=0):
    from amplipy_amd.segment import Segment
    return Segment(flag=flag, reference_start=pos, cigar=cigar, query_sequence=seq, query_qualities=[qual] * len(seq) if isinstance(qual, int) else qual)


CRAFT_G = 2000
CRAFT_PRIMERS = [(100, 130), (400, 430)]
M, I, D = 0, 1, 2


def crafted():
    """[(name, SetList, segments, min_quality, do_trim, expect)] on a reference of CRAFT_G bases with CRAFT_PRIMERS:
    ``expect(cooc, reads, setlist)`` asserts what the case is about on a table (the restatement's, the twin's, the device's)."""
    out = []

    def case(name, sets, segs, expect, mq=20, do_trim=False):
        out.append((name, SetList(sets), segs, mq, do_trim, expect))

    def only(c, L, want):
        """The table holds exactly ``want``: {(set as given, cell): count}."""
        got = {(k, cell): int(c[k, cell]) for k in range(c.shape[0]) for cell in range(CELLS) if c[k, cell]}
        assert got == {(L.index(s), cell): n for (s, cell), n in want.items()}, got

    def reads_are(r, want):
        assert [int(x) for x in r] == want, r

    T = lambda *sites: tuple(sites)
    ten = _read(600, [(M, 10)], "ACGTACGTAC")            # [600, 610)

    # a site on the first and on the last base of the read
    a, b_ = T(sub(600, "A"), sub(609, "C")), T(sub(600, "C"), sub(609, "C"))
    case("first_and_last_base", [a, b_], [ten], lambda c, r, L: (only(c, L, {(a, 3): 1, (b_, 2): 1}), reads_are(r, [1, 0])))

    # a site one position outside: partial; both outside: nothing
    s1, s2, s3, s4 = T(sub(599, "A"), sub(600, "A")), T(sub(609, "C"), sub(610, "A")), T(sub(598, "A"), sub(599, "A")), T(sub(610, "A"), sub(611, "A"))
    case("one_position_outside", [s1, s2, s3, s4], [ten], lambda c, r, L: only(c, L, {(s1, PARTIAL): 1, (s2, PARTIAL): 1}))

    # a substitution site inside the primer-trimmed part: NONE -- the trimmed alignment is the one used
    p1 = T(sub(110, "A"), sub(150, "A"))
    case("inside_the_trimmed_primer", [p1], [_read(100, [(M, 80)], "A" * 80)], lambda c, r, L: only(c, L, {(p1, PARTIAL): 1}), do_trim=True)
    case("the_same_read_untrimmed", [p1], [_read(100, [(M, 80)], "A" * 80)], lambda c, r, L: only(c, L, {(p1, 3): 1}))

    # low quality and base N: NONE
    q1, q2, q3 = T(sub(600, "A"), sub(603, "T")), T(sub(600, "A"), sub(606, "G")), T(sub(603, "T"),)
    lowq = _read(600, [(M, 10)], "ACGTACNTAC", qual=[35, 35, 35, 5, 35, 35, 35, 35, 35, 35])
    case("low_quality_and_n", [q1, q2, q3], [lowq], lambda c, r, L: only(c, L, {(q1, PARTIAL): 1, (q2, PARTIAL): 1}))
    case("quality_at_the_threshold", [q1], [_read(600, [(M, 10)], "ACGTACGTAC", qual=[20] * 10), _read(600, [(M, 10)], "ACGTACGTAC", qual=[19] * 10)],
         lambda c, r, L: only(c, L, {(q1, 3): 1}))

    # a substitution site under a deletion: NOT
    d4 = _read(600, [(M, 4), (D, 3), (M, 4)], "ACGT" "ACGT")          # [600, 611), 604..606 deleted
    u1 = T(sub(602, "G"), sub(605, "A"))
    case("substitution_under_a_deletion", [u1], [d4], lambda c, r, L: only(c, L, {(u1, 1): 1}))

    # a deletion site whose flank is the read's edge or beyond: NONE; its flank the read's first base: informative
    e1, e2, e3, e4 = T(dele(600, 2)), T(sub(602, "G"), dele(609, 2)), T(dele(601, 2)), T(dele(604, 3))
    case("deletion_flank_at_the_edge", [e1, e2, e3, e4], [d4], lambda c, r, L: only(c, L, {(e2, PARTIAL): 1, (e3, 0): 1, (e4, 1): 1}))

    # a deletion exactly matched by 3D2D: MUT; one longer, one shorter, shifted by one either way: NOT
    dd = _read(600, [(M, 4), (D, 3), (D, 2), (M, 4)], "ACGT" "ACGT")  # 604..608 deleted
    x0, x1, x2, x3, x4 = T(dele(604, 5)), T(dele(604, 6)), T(dele(604, 4)), T(dele(605, 5)), T(dele(603, 5))
    case("deletion_3D2D_and_near_misses", [x0, x1, x2, x3, x4], [dd, _read(600, [(M, 4), (D, 5), (M, 4)], "ACGT" "ACGT")],
         lambda c, r, L: only(c, L, {(x0, 1): 2, (x1, 0): 2, (x2, 0): 2, (x3, 0): 2, (x4, 0): 2}))

    # an insertion between two sites: the second site's base comes from behind the inserted bases
    i1, i2 = T(sub(603, "T"), sub(604, "C")), T(sub(603, "T"), sub(605, "A"))
    case("insertion_between_two_sites", [i1, i2], [_read(600, [(M, 4), (I, 2), (M, 4)], "ACGT" "TT" "CAGA")], lambda c, r, L: only(c, L, {(i1, 3): 1, (i2, 3): 1}))

    # a soft clip in front: its bases are not the alignment's
    case("soft_clip_in_front", [i1], [_read(600, [(4, 3), (M, 6)], "GGG" "ACGTCA")], lambda c, r, L: only(c, L, {(i1, 3): 1}))

    # a set wider than any read: only partial
    w1 = T(sub(590, "A"), sub(700, "A"))
    case("set_wider_than_any_read", [w1], [_read(580, [(M, 20)], "A" * 20), _read(690, [(M, 20)], "C" * 20), _read(620, [(M, 20)], "A" * 20)],
         lambda c, r, L: only(c, L, {(w1, PARTIAL): 2}))

    # a live read that is not regular (a soft clip inside the alignment) is counted as skipped and adds nothing
    case("non_regular_live_read", [a], [ten, _read(600, [(M, 4), (4, 2), (M, 4)], "ACGT" "TT" "ACAC")],
         lambda c, r, L: (only(c, L, {(a, 3): 1}), reads_are(r, [1, 1])))
    return out


def bit_order_case():
    """One set of six sites; pattern m is carried by exactly m + 1 reads.  -> (SetList, segments)."""
    sites = [sub(600 + 2 * j, "A") for j in range(SITES)]
    segs = []
    for m in range(64):
        seq = ["C"] * 12
        for j in range(SITES):
            if (m >> j) & 1:
                seq[2 * j] = "A"
        segs += [_read(600, [(M, 12)], "".join(seq)) for _ in range(m + 1)]
    order = np.random.default_rng(9).permutation(len(segs))
    return SetList([sites]), [segs[k] for k in order]


def pile_case():
    """4,096 identical reads on one two-site set, then 4,096 split 3 : 1 over two patterns of another.  -> (SetList, segments)."""
    s1, s2 = [sub(700, "A"), sub(705, "G")], [sub(900, "A"), sub(905, "G")]
    segs = [_read(698, [(M, 12)], "CCACCCCGCCCC") for _ in range(4096)]
    segs += [_read(898, [(M, 12)], "CCACCCCGCCCC" if k % 4 else "CCACCCCTCCCC") for k in range(4096)]
    return SetList([s1, s2]), segs
