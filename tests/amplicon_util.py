"""TEST INFRASTRUCTURE of the per-amplicon allele counts: a plain restatement of the amplicon set, the
assignment of a read and the tables, written from the definitions and from nothing in amplipy_amd/csrc; the seeded piles the
amplicon tests share; the pair list of the example BED; and the construction that pins the restatement to the reference-pinned
oracle -- the oracle's count table of the sub-batch of reads assigned to one amplicon is that amplicon's rows."""
import numpy as np

from amplipy_amd import abi, synth
from tests import helpers as H
from tests import qc_util as Q
from tests import strand_util as S

REF_OPS = (0, 2, 3, 7, 8)


# ---- the amplicon set -------------------------------------------------------------------------------------------------------
class Amps:
    """pairs: [(left name, right name, amplicon name or None)]; rows: [(start, end, name)] of the primer BED in ascending
    (start, end), file order among equals.  A name stands for every row that carries it."""

    def __init__(self, pairs, rows, offset, ref_len, owners=Q.primer_owners):
        self.G, self.offset = ref_len, offset
        self.names = []
        role = {}
        for left, right, amp in pairs:
            amp = left if amp is None else amp
            if amp not in self.names:
                self.names.append(amp)
            a = self.names.index(amp)
            for pname, side in ((left, 0), (right, 1)):
                assert any(n == pname for _, _, n in rows) and role.setdefault(pname, (a, side)) == (a, side)
        self.left = [(s, e, role[n][0]) for s, e, n in rows if n in role and role[n][1] == 0]
        self.right = [(s, e, role[n][0]) for s, e, n in rows if n in role and role[n][1] == 1]
        self.lo = [max(0, min(s for s, e, x in self.left if x == a) - offset) for a in range(len(self.names))]
        self.hi = [min(ref_len, max(e for s, e, x in self.right if x == a) + offset) for a in range(len(self.names))]
        assert all(l < h for l, h in zip(self.lo, self.hi))
        self.off = [0]
        for l, h in zip(self.lo, self.hi):
            self.off.append(self.off[-1] + h - l)
        # amp_start: the left-role primer that covers p with the largest end; amp_end: the right-role one with the smallest start
        lmap = np.array([a for _, _, a in self.left] + [-1], np.int32)
        rmap = np.array([a for _, _, a in self.right] + [-1], np.int32)
        self.amp_start = lmap[owners(ref_len, [(s, e) for s, e, _ in self.left], offset)[0]]
        self.amp_end = rmap[owners(ref_len, [(s, e) for s, e, _ in self.right], offset)[1]]

    @property
    def n(self):
        return len(self.names)

    @property
    def cells(self):
        return self.off[-1]

    def assign(self, p, e):
        """The amplicon of a read that came in at [p, e), -1: none."""
        cands = []
        if 0 <= p < self.G:
            cands.append(int(self.amp_start[p]))
        if 0 < e <= self.G:
            cands.append(int(self.amp_end[e - 1]))
        for a in cands:
            if a >= 0 and self.lo[a] <= p and e <= self.hi[a]:
                return a
        return -1

    def enable(self, eng):
        eng.amplicon_enable(self.lo, self.hi, self.amp_start, self.amp_end)


def simple_amps(ref_len, primer_pairs, offset=0):
    """Amplicons from [((left start, left end), (right start, right end))]: primers L<k> / R<k>."""
    rows = []
    for k, (l, r) in enumerate(primer_pairs):
        rows += [(l[0], l[1], "L%d" % k), (r[0], r[1], "R%d" % k)]
    rows.sort(key=lambda x: (x[0], x[1]))
    return Amps([("L%d" % k, "R%d" % k, None) for k in range(len(primer_pairs))], rows, offset, ref_len), rows


def example_rows():
    bed = [l.rstrip("\r\n").split("\t") for l in open(H.GOLDEN + "/data/example_primers.bed") if l.strip()]
    rows = [(int(f[1]), int(f[2]), f[3]) for f in bed]
    rows.sort(key=lambda r: (r[0], r[1]))
    return rows


def example_pairs(rows):
    """A name ending in F pairs with the same name ending in R; in BED order of the F primer, each pair once."""
    names = [n for _, _, n in rows]
    out = []
    for n in names:
        if n.endswith("F") and n[:-1] + "R" in names and (n, n[:-1] + "R", None) not in out:
            out.append((n, n[:-1] + "R", None))
    return out


_EXAMPLE = {}


def example_amps(offset=0):
    if offset not in _EXAMPLE:
        rows = example_rows()
        _EXAMPLE[offset] = Amps(example_pairs(rows), rows, offset, 29903)
    return _EXAMPLE[offset]


# ---- the restatement --------------------------------------------------------------------------------------------------------
def assignment(batch, amps, status=None):
    """int array: the amplicon of every read, -1: none, -2: the read has a status."""
    out = np.full(batch.n, -2, np.int64)
    for i in range(batch.n):
        if status is not None and int(status[i]) != 0:
            continue
        ops = batch.cig[int(batch.cig_off[i]):int(batch.cig_off[i + 1])]
        p = int(batch.pos[i])
        out[i] = amps.assign(p, p + sum(int(w) >> 4 for w in ops if (int(w) & 15) in REF_OPS))
    return out


def tables(batch, res, amps, min_quality, do_trim):
    """(amp_counts uint32[cells][6], amp_reads uint64[A + 1], assignment) of one batch and its trim results ``res``
    (abi.TrimResult: new_pos, new_cig, status; None: every read has status 0 and nothing was trimmed)."""
    asg = assignment(batch, amps, None if res is None else res.status)
    counts = [[0] * abi.NSYM for _ in range(amps.cells)]
    reads = [0] * (amps.n + 1)
    for i in range(batch.n):
        a = int(asg[i])
        if a == -2:
            continue
        reads[a if a >= 0 else amps.n] += 1
        if a < 0:
            continue
        s = batch.segment(i)
        if do_trim:
            s.reference_start = int(res.new_pos[i])
            s.cigartuples = res.cigar_ops(i)
        for r, c, _ in S.read_adds(s, min_quality):
            assert amps.lo[a] <= r < amps.hi[a]          # the counted alignment lies inside the original one, hence inside the span
            counts[amps.off[a] + r - amps.lo[a]][c] += 1
    return np.array(counts, np.uint32).reshape(amps.cells, abi.NSYM), np.array(reads, np.uint64), asg


def scatter(amp_counts, amps):
    """The sum over the amplicons back at reference positions: uint64[G][6]."""
    out = np.zeros((amps.G, abi.NSYM), np.uint64)
    for a in range(amps.n):
        out[amps.lo[a]:amps.hi[a]] += amp_counts[amps.off[a]:amps.off[a + 1]]
    return out


def check_invariants(amp_counts, amp_reads, asg, counts, amps):
    """The exact invariants of section 17 that need no oracle run."""
    back = scatter(amp_counts, amps)
    assert (back <= counts).all()
    if not (asg == -1).any():
        assert np.array_equal(back, counts)
    assert int(amp_reads.sum()) == int((asg != -2).sum())
    assert [int(x) for x in amp_reads] == [int((asg == a).sum()) for a in range(amps.n)] + [int((asg == -1).sum())]


def oracle_sub_batches(process, batch, asg, amps, tabs, amp_counts, min_quality, window, do_trim, only=None):
    """For each amplicon a (``only``: these), the oracle's count table of the sub-batch of reads assigned to a equals a's rows
    on [lo_a, hi_a) and is zero outside.  -> the amplicons that had reads."""
    seen = []
    for a in (range(amps.n) if only is None else only):
        rows = np.nonzero(asg == a)[0]
        block = amp_counts[amps.off[a]:amps.off[a + 1]]
        if rows.size == 0:
            assert not block.any()
            continue
        want = S.oracle_counts(process, synth.gather_rows(batch, rows), amps.G, tabs, min_quality, window, do_trim)[0]
        assert np.array_equal(want[amps.lo[a]:amps.hi[a]], block), a
        assert not want[:amps.lo[a]].any() and not want[amps.hi[a]:].any(), a
        seen.append(a)
    return seen


# ---- piles ------------------------------------------------------------------------------------------------------------------
def pile(amps, which, n, seed, read_len=150, overrun=0.1, interleave=True):
    """``n`` reads drawn from the amplicons ``which``, read by read in turn (interleave) or amplicon after amplicon: forward
    reads from the left primer, reverse reads ending in the right primer, fragments inside, and a share that overruns the span
    by one base and more.  Sorted by position unless interleaved draws are asked for as they come."""
    rng = np.random.default_rng(seed)
    segs = []
    for k in range(n):
        a = which[k % len(which)] if interleave else which[min(k * len(which) // max(n, 1), len(which) - 1)]
        lo, hi = amps.lo[a], amps.hi[a]
        span = hi - lo
        L = int(min(span, read_len - int(rng.integers(0, 30))))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            pos, flag = lo, 0
        elif kind == 1:
            pos, flag = hi - L, 0x10
        else:
            L = max(L // 2, 1)
            pos, flag = lo + int(rng.integers(0, span - L + 1)), 0x10 if k % 2 else 0
        if rng.random() < overrun:
            over = 1 if rng.random() < 0.5 else int(rng.integers(2, 12))
            if kind == 1 or (kind == 2 and k % 2):
                pos = min(hi + over, amps.G) - L
            else:
                pos = max(lo - over, 0)
        shape = int(rng.integers(0, 6))
        if shape == 0 and L > 20:
            d = int(rng.integers(5, L - 10))
            cig = [(0, d), (2, 2), (0, L - d - 2)]
        elif shape == 1 and L > 20:
            d = int(rng.integers(5, L - 10))
            cig = [(0, d), (1, 3), (0, L - d)]
        elif shape == 2:
            cig = [(4, 4), (0, L), (4, 2)]
        else:
            cig = [(0, L)]
        segs.append(S.seg(pos, cig, rng, flag))
    return segs


# ---- the seven INFO keys from tables ----------------------------------------------------------------------------------------
def keys(pos, ref, alts, amps, rows, counts, amp_counts, p_value):
    """{key: text} of a record at 0-based ``pos``.  rows: the primer BED [(start, end, name)] in ascending (start, end);
    counts: the count table; p_value(a, b, c, d): the two-sided Fisher exact test the caller holds AMP_P to."""
    listed = [a for a in range(amps.n) if amps.lo[a] <= pos < amps.hi[a]]
    cells = [[int(v) for v in amp_counts[amps.off[a] + pos - amps.lo[a]]] for a in listed]
    dps = [sum(c) for c in cells]
    out = {"AMP": ",".join(amps.names[a] for a in listed) if listed else ".",
           "AMP_DP": ",".join(str(d) for d in dps) if listed else ".",
           "AMP_NA_DP": str(sum(int(v) for v in counts[pos]) - sum(dps))}
    out["AMP_REF_DP"] = ",".join(str(c["ACGTN".index(ref)]) for c in cells) if listed and ref in tuple("ACGTN") else "."
    order = sorted(range(len(listed)), key=lambda k: (-dps[k], k))          # largest AMP_DP first, the earlier among equals
    pair = order[:2] if len([d for d in dps if d > 0]) >= 2 else None
    alt_dp, alt_p = [], []
    for s in alts:
        if s not in tuple("ACGTN-"):                                        # an insertion allele
            alt_dp.append("."); alt_p.append(".")
            continue
        c = "ACGTN-".index(s)
        alt_dp.append("|".join(str(x[c]) for x in cells) if listed else ".")
        alt_p.append("%.4g" % p_value(cells[pair[0]][c], dps[pair[0]] - cells[pair[0]][c], cells[pair[1]][c], dps[pair[1]] - cells[pair[1]][c])
                     if pair else ".")
    out["AMP_ALT_DP"], out["AMP_P"] = ",".join(alt_dp), ",".join(alt_p)
    names = []
    for s, e, n in rows:
        if s <= pos < e and n not in names:
            names.append(n)
    out["PRIMER"] = ",".join(names) if names else "."
    return out


KEY_ORDER = ("AMP", "AMP_DP", "AMP_REF_DP", "AMP_ALT_DP", "AMP_NA_DP", "AMP_P", "PRIMER")


def info_text(k):
    return ";".join("%s=%s" % (n, k[n]) for n in KEY_ORDER)
