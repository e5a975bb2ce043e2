"""Crafted batches for the read pass (k_fast, k_fast5, k_fast7, k_tile<LIST>, k_deferred_heavy, k_long): every case sits on a limit
of those kernels, and carries the route facts that follow from the kernels' own constants -- which reads a fast kernel must hand to
the general pass, which the general pass must hand on, which kernel the engine's own routing picks.

Plain Python and numpy: no GPU, no library.  tests/test_readpass_craft.py runs the list on the CPU (oracle, tests/hostsim, the
constants against the headers), tests/test_gpu_readpass_edges.py on the device with the route checks.

The constants below restate amp_fast.hpp, amp_fast5.hpp, amp_plan.hpp and amp_wave.hpp; the CPU test reads the same names out of
the headers and fails when they drift, so a kernel change that moves a limit has to move the cases with it.
"""
import numpy as np

from amplipy_amd.batch import ALIGN, ReadBatch, pack_nibbles

# ---- the kernels' constants --------------------------------------------------------------------------------------------------
F_MAXLEN = 152          # longest read k_fast takes
F5_MAXLEN = 304         # ... k_fast5 / k_fast7
F_MAXINS = 8            # longest insertion / deletion of a read a fast kernel takes
F_MAXDEL = 16
F_PW = 256              # positions of a wave's packed window
F_BW = 512              # ... of the block's 32-bit window
F_FLUSH = 15            # tiles between two folds of a packed window
F_STAGE = 10240         # bytes of k_fast's staging buffer: the longest run of quality bytes a tile may span
F_EVGRAN = 64           # event-list slots a wave reserves at a time
TILE = 64
F_WAVES = 8
F7_WAVES = 7
T_MAXOPS = 18           # the tile kernel takes reads of up to T_MAXOPS - 3 input ops
L_MAXOPS = 160          # k_long: up to L_MAXOPS - 4
WV_MAXOPS = 512         # the heavy pass's wave path: up to WV_MAXOPS - 4
F5_PAD_SHORT, F5_PAD_MID = 152, 192                 # fast5_cfg: mean padded read length up to which a build is chosen ...
F5_RUN_SHORT, F5_RUN_MID, F5_RUN_LONG = 9728, 13312, 19456      # ... and its run of quality bytes per tile
FAST_MAX_WINDOW = 8     # fast_path_active: window <= 8 and min_quality <= 128
FAST_MAX_MINQ = 128
TILE_SUMLEN = 4096      # the tile kernel keeps op lengths in 12 bits: reads whose op lengths sum to this go to the heavy pass
TILE_MAXLSEQ = 65536    # ... and reads of this many bases

HEADER_CONSTANTS = {
    "amp_fast.hpp": dict(F_MAXLEN=F_MAXLEN, F_MAXINS=F_MAXINS, F_MAXDEL=F_MAXDEL, F_PW=F_PW, F_STAGE=F_STAGE, F_FLUSH=F_FLUSH),
    "amp_fast5.hpp": dict(F5_MAXLEN=F5_MAXLEN),
    "amp_plan.hpp": dict(TILE=TILE, T_MAXOPS=T_MAXOPS, L_MAXOPS=L_MAXOPS),
    "amp_wave.hpp": dict(WV_MAXOPS=WV_MAXOPS),
}
# constants a header defines through a macro default (`#define AMP_X v` ... `constexpr int X = AMP_X`) or as another type
HEADER_MACROS = {
    "amp_fast.hpp": dict(AMP_F_BW=F_BW),
    "amp_plan.hpp": dict(AMP_F_WAVES=F_WAVES, AMP_F7_NWAVES=F7_WAVES),
}
HEADER_UINTS = {"amp_plan.hpp": dict(F_EVGRAN=F_EVGRAN)}

M, I, D, N_, S, H, P, EQ, X = range(9)          # CIGAR op codes
A_, C_, G_, T_, NN = 1, 2, 4, 8, 15              # 4-bit base codes; R (A or G) is an IUPAC code the pile-up has no column for
R_ = 5
VARIANTS = (0, 4, 5, 7, 2)


class Read:
    __slots__ = ("pos", "flag", "tlen", "cig", "codes", "qual")

    def __init__(self, pos, cig, codes, qual, flag=0, tlen=0):
        self.pos, self.flag, self.tlen, self.cig = int(pos), int(flag), int(tlen), [(int(o), int(k)) for o, k in cig]
        self.codes, self.qual = np.asarray(codes, np.uint8), np.asarray(qual, np.uint8)
        assert self.codes.size == self.qual.size == query_len(self.cig)

    @property
    def lseq(self):
        return self.codes.size


def query_len(cig):
    return sum(k for o, k in cig if o in (M, I, S, EQ, X))


def ref_span(cig):
    return sum(k for o, k in cig if o in (M, D, N_, EQ, X))


def build_batch(reads):
    """A ReadBatch of the reads in the order given (rows start on multiples of 8 bases, pad bytes are zero)."""
    n = len(reads)
    lseq = np.array([r.lseq for r in reads], np.int64)
    stride = lseq + (-lseq) % ALIGN
    seq_off = np.zeros(n + 1, np.uint64); seq_off[1:] = np.cumsum(stride)
    cig_off = np.zeros(n + 1, np.uint64); cig_off[1:] = np.cumsum([len(r.cig) for r in reads])
    codes = np.zeros(int(seq_off[n]), np.uint8); qual = np.zeros(int(seq_off[n]), np.uint8)
    for r, o in zip(reads, seq_off[:-1].astype(np.int64)):
        codes[o:o + r.lseq] = r.codes; qual[o:o + r.lseq] = r.qual
    cig = np.array([(k << 4) | o for r in reads for o, k in r.cig], np.uint32)
    return ReadBatch([r.pos for r in reads], [r.flag for r in reads], [r.tlen for r in reads], lseq, cig_off, cig, seq_off,
                     pack_nibbles(codes), qual)


class Case:
    """One crafted batch.  ``fails`` names the reads the oracle must refuse (at most 2 % of the batch); ``reach`` says, given the
    batch, whether the boundary the case is about is really in it; ``expect`` holds the route facts:
      slack      reads that MAY be on the general list on top of those that must be ('indel': a primer clip that runs through the
                 first match op of a one-indel read leaves a shape the closed forms hand over -- Bf::punt, amp_bf.hpp -- which depends
                 on the primer table, not on a constant; 'iupac': a piece with a code outside A C G T N is redone base by base and
                 asks for the exact status when such a base is counted)
      why        the rule of the kernels the case stands on (quoted when a route check fails)
    Everything else -- the variant the engine's own routing resolves to, the list length per fast kernel, the heavy entries -- is
    computed from the batch by route_facts()."""

    def __init__(self, name, reads=None, G=0, primers=(), offset=0, mq=20, w=4, do_trim=True, fails=(), reach=None, slack=None,
                 why="", pile=None):
        self.name, self.family = name, name[0]
        self.reads, self.G, self.primers, self.offset = reads, int(G), list(primers), int(offset)
        self.min_quality, self.window, self.do_trim = int(mq), int(w), bool(do_trim)
        self.fails = sorted(set(fails))
        self.reach = reach
        self.expect = dict(slack=slack, why=why)
        self.pile = pile
        self._batch = None

    def batch(self, n=None):
        if self.pile is not None:
            return pile_batch(n if n is not None else 2048, **self.pile)
        if self._batch is None:
            self._batch = build_batch(self.reads)
        return self._batch

    def accepted(self):
        """The batch without the reads named in ``fails``."""
        if not self.fails:
            return self.batch()
        bad = set(self.fails)
        return build_batch([r for i, r in enumerate(self.reads) if i not in bad])

    def __repr__(self):
        return "Case(%s)" % self.name


# ---- the route facts of a batch ----------------------------------------------------------------------------------------------
def shape_ok(cig, lseq, maxlen):
    """bf_from_words5 (amp_bf.hpp) and the length limit of geometry(): [S a] M ([I|D k] M) [S c], at most five ops."""
    n = len(cig)
    if not (1 <= n <= 5 and 1 <= lseq <= maxlen):
        return False
    lead = cig[0][0] == S
    v = cig[1:] if lead else cig
    m = len(v)
    if not 1 <= m <= 4 or (lead and cig[0][1] <= 0):
        return False
    o0, m1 = v[0]
    if o0 not in (M, EQ, X) or m1 <= 0:
        return False
    has3 = m >= 3
    if has3:
        (o1, k), (o2, m2) = v[1], v[2]
        if o1 not in (I, D) or o2 != o0 or k <= 0 or m2 <= 0:
            return False
        if (o1 == I and k > F_MAXINS) or (o1 == D and k > F_MAXDEL):
            return False
    if (m == 4) if has3 else (m == 2):
        ot, c = v[3] if has3 else v[1]
        if ot != S or c <= 0:
            return False
    elif has3 and m != 3:
        return False
    return query_len(cig[:n]) == lseq


def regular(cig, lseq):
    """classify() of amp_tile.hpp: H* S* (M|=|X|I|D|N)* S* H* whose query length is l_seq.  Any other CIGAR is the exact code's."""
    phase, q = 0, 0
    for op, k in cig:
        if op == H:
            if phase == 0:
                continue
            if phase >= 2:
                phase = 4; continue
            return False
        elif op == S:
            if phase <= 1:
                phase = 1
            elif phase <= 3:
                phase = 3
            else:
                return False
            q += k
        elif op in (M, EQ, X, I, D, N_):
            if phase > 2:
                return False
            phase = 2
            q += k if op in (M, EQ, X, I) else 0
        else:
            return False
    return q == lseq


def fast5_cfg(n_reads, n_bases_padded, window):
    """(waves per block, run bytes) of k_fast5 -- amp_plan.hpp."""
    mean_pad = -(-n_bases_padded // n_reads) if n_reads else 0
    if mean_pad <= F5_PAD_SHORT or window != 4:
        return 8, F5_RUN_SHORT
    if mean_pad <= F5_PAD_MID:
        return 6, F5_RUN_MID
    return 4, F5_RUN_LONG


def fast_path_active(requested, window, min_quality):
    return (requested == 0 or requested >= 4) and window <= FAST_MAX_WINDOW and min_quality <= FAST_MAX_MINQ


def route_variant(requested, batch, window, min_quality):
    """amp_plan.hpp route_variant for variants 0, 2, 4, 5, 7."""
    n, n_cig = batch.n, int(batch.cig_off[batch.n])
    waves, _ = fast5_cfg(n, int(batch.seq_off[n]), window)
    mixed = waves != 8 and n_cig >= 3 * n
    kv0 = requested if requested else (7 if mixed else 4 if (waves == 8 and window != 8) else 5)
    return 2 if (kv0 >= 4 and not fast_path_active(kv0, window, min_quality)) else kv0


def _cigars(batch):
    co = batch.cig_off.astype(np.int64)
    return [[(int(v) & 15, int(v) >> 4) for v in batch.cig[co[i]:co[i + 1]]] for i in range(batch.n)]


def _run_misfits(batch, kv, window):
    """Lanes whose bytes do not fit the run of their tile (geometry() of amp_fast.hpp / F5Sorted of amp_fast5.hpp): a tile is 64
    consecutive reads, its run starts at its first read, and the lanes from the first that does not fit on go to the general pass
    (all 64 when the first read alone is too long: `solo`).  k_fast7 gathers rows one by one and has no run."""
    n = batch.n
    out = np.zeros(n, bool)
    if kv == 7:
        return out
    o8 = (batch.seq_off[:-1] // 8).astype(np.int64)
    hl = np.minimum(batch.lseq.astype(np.int64), 0xFFFF)
    nch8 = ((hl + 7) >> 3) * 8
    if kv == 4:
        cap, extra = F_STAGE, np.where((hl >= 1) & (hl <= F_MAXLEN), 8, 0)
    else:
        cap, extra = fast5_cfg(n, int(batch.seq_off[n]), window)[1], 0
    for t0 in range(0, n, TILE):
        sl = slice(t0, min(n, t0 + TILE))
        row = (o8[sl] - o8[t0]) * 8
        fits = (o8[sl] - o8[t0] <= cap // 8) & (row + nch8[sl] + (extra[sl] if kv == 4 else 0) <= cap)
        bad = np.nonzero(~fits)[0]
        if bad.size:
            out[sl] = True if bad[0] == 0 else (np.arange(fits.size) >= bad[0])
    return out


def route_facts(case, batch, requested):
    """What the engine must report after one pass over ``batch`` (reads the oracle accepts) with kernel variant ``requested``:
      kv       Engine.last_kernel_variant()
      list     (lo, hi) of debug_counters()[7], the reads on the general list (None: the variant keeps no list)
      heavy    (lo, hi) of debug_counters()[0], heavy entries of the second pass
    lo == hi wherever the constants fix the number."""
    kv = route_variant(requested, batch, case.window, case.min_quality)
    cigs = _cigars(batch)
    lseq = batch.lseq.astype(np.int64)
    nops = np.array([len(c) for c in cigs])
    sumlen = np.array([sum(k for _, k in c) for c in cigs])
    # (the tile kernel judges the TRIMMED CIGAR; a trim leaves a regular CIGAR regular, and the cases with others trim nothing)
    heavy_shape = (nops + 3 > T_MAXOPS) | (lseq >= TILE_MAXLSEQ) | (sumlen >= TILE_SUMLEN) | \
        np.array([not regular(c, int(l)) for c, l in zip(cigs, lseq)])
    star = np.array([batch.qual[int(o)] == 0xFF for o in batch.seq_off[:-1]]) & (lseq > 0)
    facts = dict(kv=kv, list=None, heavy=None, n=batch.n)
    if kv == 2:
        # k_tile over the whole batch: heavy = the reads it cannot hold (a read without qualities is reported by the exact code, too)
        facts["heavy"] = (int(heavy_shape.sum()), int((heavy_shape | star).sum()))
        return facts
    maxlen = F_MAXLEN if kv == 4 else F5_MAXLEN
    shaped = np.array([shape_ok(c, int(l), maxlen) for c, l in zip(cigs, lseq)])
    must = ~shaped | star | _run_misfits(batch, kv, case.window)
    may = np.zeros(batch.n, bool)
    if case.expect["slack"] == "indel" and case.do_trim and case.primers:
        may = ~must & np.array([len(c) >= 3 for c in cigs])
    elif case.expect["slack"] == "iupac":
        co = unpack_codes(batch)
        may = ~must & np.array([bool(np.isin(co[int(o):int(o) + int(l)], (A_, C_, G_, T_, NN), invert=True).any())
                                for o, l in zip(batch.seq_off[:-1], lseq)])
    facts["list"] = (int(must.sum()), int((must | may).sum()))
    facts["listed"] = must
    long_kernel = int(batch.cig_off[batch.n]) >= 8 * batch.n
    hv = must & heavy_shape
    if long_kernel:
        # k_long takes list entries of 16 .. L_MAXOPS - 4 ops off the tile kernel's hands (and may hand some back): only the reads
        # with more ops than its rows hold are heavy entries for certain
        facts["heavy"] = (int((hv & (nops > L_MAXOPS - 4)).sum()), int(hv.sum()) + int(may.sum()))
    else:
        facts["heavy"] = (int(hv.sum()), int(hv.sum()) + (int(may.sum()) if case.expect["slack"] == "iupac" else 0))
    return facts


def off_limit(batch, maxlen=F5_MAXLEN):
    """Reads no fast kernel that takes ``maxlen`` bases can take, by their CIGAR and length alone."""
    return np.array([not shape_ok(c, int(l), maxlen) for c, l in zip(_cigars(batch), batch.lseq)])


def unpack_codes(batch):
    out = np.empty(batch.seq.size * 2, np.uint8)
    out[0::2] = batch.seq >> 4; out[1::2] = batch.seq & 15
    return out


# ---- building blocks ---------------------------------------------------------------------------------------------------------
_ACGT = np.array([A_, C_, G_, T_], np.uint8)


def mk(rng, pos, cig, flag=0, tlen=0, q=40, qual=None, codes=None, low_tail=0):
    L = query_len(cig)
    if codes is None:
        codes = _ACGT[rng.integers(0, 4, L)]
    if qual is None:
        qual = np.full(L, q, np.uint8)
        if low_tail and L > low_tail:
            if flag & 16:
                qual[:low_tail] = 2
            else:
                qual[L - low_tail:] = 2
    return Read(pos, cig, codes, qual, flag, tlen)


def by_pos(reads):
    return sorted(reads, key=lambda r: r.pos)


def many_ops(rng, pos, nops, seg=3, lead_clip=False):
    """A regular CIGAR of exactly ``nops`` ops: match ops of ``seg`` bases around one-base insertions and deletions in turn."""
    cig = [(S, 4)] if lead_clip else []
    k = 0
    while len(cig) < nops:
        if (len(cig) - (1 if lead_clip else 0)) % 2 == 0:
            cig.append((M, seg))
        else:
            cig.append((I if k % 2 == 0 else D, 1)); k += 1
    if cig[-1][0] != M:                 # (an even body: close it with a clip, which keeps the count)
        cig[-1] = (S, 2)
    assert len(cig) == nops
    return mk(rng, pos, cig)


def pile_batch(n, L=150, shift=False):
    """n identical one-op reads (same position, same bases, quality 40), every second one a position further when ``shift``."""
    rng = np.random.default_rng(L)
    codes = np.broadcast_to(_ACGT[rng.integers(0, 4, L)], (n, L))
    pos = np.full(n, 300, np.int32)
    if shift:
        pos[1::2] += 1          # (pairs of tiles stay in coordinate order within a position: the kernels do not rely on more)
    return ReadBatch.from_uniform(pos, np.zeros(n, np.uint16), np.zeros(n, np.int32), L, np.arange(n + 1, dtype=np.uint64),
                                  np.full(n, (L << 4) | M, np.uint32), codes, np.full((n, L), 40, np.uint8))


def pile_reads(n_cu, kv, cu_share=16):
    """Reads of a pile in which a wave of the fast kernel sees more than two fold intervals of tiles in one window:
    (fast blocks for that share) x (waves per block) x (2 F_FLUSH + 2) x 64."""
    waves = F7_WAVES if kv == 7 else F_WAVES
    return max(1, n_cu // cu_share) * waves * (2 * F_FLUSH + 2) * TILE


# ---- the families ------------------------------------------------------------------------------------------------------------
A_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 143, 144, 145, 151, 152, 153, 160, 296, 297, 303, 304, 305)
A_STARTS = (0, 7, 8, 15)


def _family_a():
    cases = []
    for w in (1, 4, 8):
        rng = np.random.default_rng(100 + w)
        reads = []
        for rep in range(4):
            for L in A_LENGTHS:
                for st in A_STARTS:
                    reads.append(mk(rng, 320 + 16 * ((rep * 7 + L) % 40) + st, [(M, L)], flag=16 if (L + rep) % 2 else 0,
                                    low_tail=3 if rep % 2 else 0))
        cases.append(Case("A_lengths_w%d" % w, by_pos(reads), G=1600, w=w,
                          reach=lambda b: set(A_LENGTHS) <= set(b.lseq.tolist()) and {0, 7, 8, 15} <= set((b.pos % 16).tolist()),
                          why="one-op reads at every length limit: the list is exactly the reads longer than the kernel's limit"))
    rng = np.random.default_rng(110)
    # tile 0 starts with a read longer than any staging run: the whole tile is the general pass's; tile 1 is plain
    reads = [mk(rng, 100, [(M, 10300)])] + [mk(rng, 100 + k, [(M, 150)]) for k in range(1, 128)]
    cases.append(Case("A_solo_first_read", reads, G=12000, reach=lambda b: int(b.lseq[0]) > F_STAGE and _run_misfits(b, 4, 4)[:64].all(),
                      why="geometry(): first read of a tile longer than the run -> `solo`, all 64 lanes handed over"))
    # lane 20 holds a long read: 400 bases still leave room for the 152-base rows behind it in k_fast's 10,240 bytes (the last two
    # lanes fall off k_fast5's 9,728); 1,000 bases in the second tile push lanes off k_fast's run as well.  (Four tiles of short
    # reads behind them keep the batch's mean padded length under 152, so that k_fast5 runs its 9,728-byte build.)
    reads = []
    for t, long_len in enumerate((400, 1000)):
        for lane in range(64):
            reads.append(mk(rng, 500 + 64 * t + lane, [(M, long_len if lane == 20 else 152)]))
    reads += [mk(rng, 640 + i, [(M, 100)]) for i in range(256)]
    cases.append(Case("A_ntake_long_read_in_lane_20", reads, G=2000,
                      reach=lambda b: fast5_cfg(b.n, int(b.seq_off[b.n]), 4)[1] == F5_RUN_SHORT and _run_misfits(b, 4, 4)[64:128].sum() > 0
                      and _run_misfits(b, 5, 4)[:64].sum() == 2 and not _run_misfits(b, 4, 4)[:64].any(),
                      why="geometry(): the lanes behind a long read that no longer fit the run (`ntake`) go to the general pass"))
    return cases


B_INS = (1, 7, 8, 9)
B_DEL = (1, 8, 9, 15, 16, 17)
B_OFFSETS = (1, 7, 8, 9, 15, 16, 17, -2)


def _indel_cig(L, kind, k, off, a, c):
    """[S a] m1 M, k I|D, m2 M [S c] of l_seq L with the indel ``off`` aligned bases into the read (-2: one base before its end)."""
    body = L - a - c - (k if kind == I else 0)
    m1 = off if off > 0 else body - 1
    m2 = body - m1
    assert m1 >= 1 and m2 >= 1
    return ([(S, a)] if a else []) + [(M, m1), (kind, k), (M, m2)] + ([(S, c)] if c else [])


def _family_b():
    cases = []
    rng = np.random.default_rng(200)
    reads = []
    for L in (F_MAXLEN, F5_MAXLEN):
        for kind, ks in ((I, B_INS), (D, B_DEL)):
            for k in ks:
                for off in B_OFFSETS:
                    for a, c in ((0, 0), (5, 0), (0, 6), (5, 6)):
                        cig = _indel_cig(L, kind, k, off, a, c)
                        r = mk(rng, 200 + (len(reads) * 3) % 190, cig, flag=16 if len(reads) % 3 == 0 else 0)
                        if kind == I and k >= 7:        # low bases inside the insertion: several events from one insertion
                            q0 = a + cig[1 if a else 0][1]
                            r.qual[q0 + 1:q0 + k:2] = 2
                        reads.append(r)
    def reach_b1(b):
        cg = _cigars(b)
        ins = {k for c in cg for o, k in c if o == I}; dl = {k for c in cg for o, k in c if o == D}
        return set(B_INS) <= ins and set(B_DEL) <= dl and {F_MAXLEN, F5_MAXLEN} <= set(b.lseq.tolist())
    cases.append(Case("B_one_indel_ends_of_range", by_pos(reads), G=1200, reach=reach_b1,
                      why="no primers: no clip can leave a punted shape, so the list is exactly the reads with an insertion of 9, "
                          "a deletion of 17 or more bases than the kernel takes"))
    # the 4-, 5- and 6-op forms
    rng = np.random.default_rng(201)
    forms = [[(S, 4), (M, 40), (I, 3), (M, 50)], [(S, 4), (M, 40), (D, 16), (M, 50), (S, 7)], [(H, 3), (S, 4), (M, 40), (D, 5), (M, 50), (S, 7)],
             [(M, 40), (I, 8), (M, 50), (S, 7)], [(H, 3), (M, 90)], [(M, 90)], [(S, 3), (EQ, 60), (D, 2), (EQ, 30)], [(M, 30), (D, 2), (EQ, 30)],
             [(M, 40), (N_, 5), (M, 40)], [(S, 4), (M, 40), (S, 3), (M, 2), (S, 1)]]
    reads = [mk(rng, 100 + (i * 7) % 150, forms[i % len(forms)], flag=16 * (i % 2)) for i in range(300)]
    cases.append(Case("B_four_five_six_op_forms", by_pos(reads), G=1000,
                      reach=lambda b: {1, 2, 3, 4, 5, 6} <= set(np.diff(b.cig_off.astype(np.int64)).tolist()),
                      why="six ops are outside the five CIGAR words a fast kernel loads; hard clips, N ops and mixed match ops are no shape"))
    # primer clips that end one base before the indel, on it, inside it and one base behind it, from either side, both strands
    rng = np.random.default_rng(202)
    reads, primers = [], []
    base = 100
    for kind, k in ((I, 3), (I, 8), (D, 3), (D, 16), (I, 9), (D, 17)):
        for d in (-2, -1, 0, 1, 2, k, k + 1):
            for side in (0, 1):
                kd = k if kind == D else 0
                if side == 0:       # left primer ending around the indel at reference base + 40
                    cig, primers_g = [(M, 30), (kind, k), (M, 60)], (base, base + 40 + d)
                else:               # right primer starting around the indel at reference base + 70
                    cig, primers_g = [(M, 60), (kind, k), (M, 30)], (base + 70 + d, base + 112 + kd)
                primers.append(primers_g)
                for flag in (0, 16):
                    reads.append(mk(rng, base + 10, cig, flag=flag, low_tail=2 if d == 0 else 0))
                    reads.append(mk(rng, base + 10, [(S, 3)] + cig + [(S, 2)], flag=flag))
                base += 300
    cases.append(Case("B_primer_clips_around_the_indel", by_pos(reads), G=base + 300, primers=primers, slack="indel",
                      reach=lambda b: b.n == 6 * 7 * 2 * 4,
                      why="bound: a primer clip through the first match op of an indel read leaves a punted shape (Bf::punt), which "
                          "depends on the table: at least the reads past a limit, at most those plus the indel reads"))
    return cases


C_MINQ = (0, 1, 2, 127, 128, 129, 255)


def _family_c():
    cases = []
    for mq in C_MINQ:
        values = sorted({v for v in (0, mq - 1, mq, mq + 1, 126, 127, 128, 129, 200, 254) if 0 <= v <= 254})
        # (1) trimming on: one low byte among 254s, so that every window of 4 / 8 passes while single bases fail
        if mq <= 129:
            for w in (4, 8):
                rng = np.random.default_rng(300 + mq + w)
                reads = []
                for i in range(192):
                    r = mk(rng, 50 + i % 100, [(M, 100)] if i % 4 else [(M, 40), (I, 4), (M, 56)], flag=16 * (i % 2), q=254)
                    r.qual[[9 + i % 7, 33 + i % 5, 57, 80 + i % 11]] = values[i % len(values)]
                    reads.append(r)
                cases.append(Case("C_minq%d_w%d_low_bytes_among_high" % (mq, w), by_pos(reads), G=400, mq=mq, w=w,
                                  reach=lambda b, values=values: set(values) <= set(b.qual.tolist()),
                                  why="fast_path_active: min_quality <= 128 and window <= 8 stay on the fast kernels, 129 takes variant 2"))
        # (2) trimming off: every byte of the set anywhere (255 as well, behind the first byte, so that min_quality 255 counts something)
        rng = np.random.default_rng(350 + mq)
        pool = np.array(values + [255], np.uint8)
        reads = []
        for i in range(192):
            r = mk(rng, 50 + i % 100, [(M, 100)] if i % 4 else [(M, 40), (D, 4), (M, 60)], flag=16 * (i % 2))
            r.qual[:] = pool[rng.integers(0, pool.size, r.lseq)]
            r.qual[0] = values[i % len(values)]
            reads.append(r)
        cases.append(Case("C_minq%d_untrimmed_every_byte" % mq, by_pos(reads), G=400, mq=mq, do_trim=False,
                          reach=lambda b, values=values: set(values) | {255} <= set(b.qual.tolist()),
                          why="ok_bits4 / the star test: a quality byte of 128 ... 255 anywhere behind the first is a good base, no hand-over"))
    # the window rule
    for w, mq in ((8, 128), (9, 20), (8, 129)):
        rng = np.random.default_rng(380 + w)
        reads = [mk(rng, 50 + i % 100, [(M, 120)], flag=16 * (i % 2), q=200, low_tail=i % 12) for i in range(192)]
        cases.append(Case("C_window%d_minq%d" % (w, mq), by_pos(reads), G=400, mq=mq, w=w, reach=lambda b: True,
                          why="window 9 / min_quality 129 report variant 2, window 8 with min_quality 128 a fast kernel"))
    # QUAL '*'
    rng = np.random.default_rng(390)
    # k_fast finds a read's first quality byte among its rotated piece slots.  Reads of 90 / 96 bases in lanes 7, 14 and 35 (pieces
    # start 8 bases early there, and lane % pieces == 0): the byte 8 of their last piece lies behind the row, in the next read
    star = {5: 100, 7: 90, 14: 90, 64 + 35: 96, 128 + 63: 100}
    reads = [mk(rng, 50 + i, [(M, star.get(i, 100))]) for i in range(320)]
    for i in star:
        reads[i].qual[:] = 0xFF
    cases.append(Case("C_no_qualities", reads, G=500, fails=sorted(star), reach=lambda b: int((b.qual == 0xFF).sum()) == 476,
                      why="a read whose first quality byte is 0xFF goes to the exact code, which refuses it: the statuses must be the oracle's"))
    return cases


D_REFLEN = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def _family_d():
    cases = []
    for G in D_REFLEN:
        rng = np.random.default_rng(400 + G)
        shapes = []
        for L in sorted({1, min(G, 7), min(G, 8), min(G, 16), min(G, 100), min(G, 152), min(G, 304)}):
            shapes.append((0, [(M, L)])); shapes.append((G - L, [(M, L)]))
        if G >= 17:
            span = min(G, 120)
            shapes.append((G - span, [(M, 5), (D, 2), (M, span - 7)]))                 # second segment ends on G - 1
            shapes.append((G - span, [(M, 5), (I, 3), (M, span - 5)]))
            shapes.append((0, [(M, 4), (D, min(16, G - 8)), (M, 4)]))
        if G >= 64:
            shapes.append((G - 40, [(S, 5), (M, 20), (D, 16), (M, 4), (S, 3)]))
        reads = [mk(rng, p, c, flag=16 * (i % 2)) for i in range(6) for p, c in shapes]
        reads = by_pos(reads)
        fails = []
        if G >= 300:
            reads.append(mk(rng, G - 99, [(M, 100)]))       # one base past the end
            reads = by_pos(reads)
            fails = [i for i, r in enumerate(reads) if r.pos + ref_span(r.cig) > G]
        cases.append(Case("D_reference_of_%d" % G, reads, G=G, fails=fails,
                          reach=lambda b, G=G: int(b.pos.min()) == 0 and any(int(p) + ref_span(c) == G for p, c in zip(b.pos, _cigars(b))),
                          why="pw_lim: packed and block windows wider than the reference"))
    return cases


E_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 895, 896, 897, 1023, 1024, 1025, 2047, 2048, 2049)


def _family_e():
    cases = []
    for n in E_SIZES:
        rng = np.random.default_rng(500 + n)
        reads = []
        for i in range(n):
            amp = 100 + 280 * (i * 8 // max(n, 8))               # eight piles of reads, in coordinate order
            kind = i % 10
            cig = [(M, 150)] if kind else ([(M, 30), (I, 2), (M, 118)] if i % 20 else [(M, 70), (D, 3), (M, 80)])
            reads.append(mk(rng, amp + i % 3, cig, flag=16 * (i % 2), low_tail=(i % 7) * 2))
        cases.append(Case("E_batch_of_%d" % n, by_pos(reads), G=2600, reach=lambda b, n=n: b.n == n,
                          why="all reads are shapes every fast kernel takes: an empty general list at every tile edge"))
    return cases


F_STEPS = (47, 48, 63, 64, 65, 255, 256, 257)


def _family_f():
    cases = []
    rng = np.random.default_rng(600)
    reads = []
    base = 100
    for step in F_STEPS:
        # the eight waves of a block draw tiles in turn: tiles 8 r .. 8 r + 7 share a position, the next eight lie `step` further
        for rnd in range(2):
            for t in range(8):
                for lane in range(64):
                    cig = [(M, 150)] if lane % 8 else [(M, 60), (D, 16), (M, 74)]
                    reads.append(mk(rng, base + rnd * step, cig))
        base += 1500
    cases.append(Case("F_window_steps", reads, G=base + 500,
                      reach=lambda b: set(F_STEPS) <= set(np.diff(b.pos[::512].astype(np.int64)).tolist()),
                      why="a piece that leaves the packed window is redone base by base, never handed over: the list stays empty"))
    reads = []
    for span, p0 in ((5, 100), (10, 1000)):         # a tile over 5 * 63 + 150 > 256 positions, one over 10 * 63 + 150 > 512
        for rep in range(2):
            reads += [mk(rng, p0 + span * lane, [(M, 150)] if lane % 5 else [(M, 100), (I, 8), (M, 42)]) for lane in range(64)]
    cases.append(Case("F_tiles_wider_than_the_windows", reads, G=2200,
                      reach=lambda b: int(b.pos[63] - b.pos[0]) + 150 > F_PW and int(b.pos[191] - b.pos[128]) + 150 > F_BW))
    reads = [mk(rng, 900 - 12 * (i // 16), [(M, 140)] if i % 6 else [(M, 50), (D, 9), (M, 90)]) for i in range(640)]
    reads += [mk(rng, 40 + i, [(M, 150)]) for i in range(64)]
    cases.append(Case("F_steps_backwards_unsorted", reads, G=1400, reach=lambda b: bool((np.diff(b.pos.astype(np.int64)) < 0).any())))
    return cases


def _family_g():
    cases = []
    rng = np.random.default_rng(700)
    reads, fails = [], []
    spots = (0, 7, 8, 15, 16, 23, 24, 31)          # bases 0, 7, 8, 15 of a piece for both early starts (phi = 0 and 8)
    for i in range(512):
        L = (97, 103, 100, 150)[i % 4]
        r = mk(rng, 60 + i // 4, [(M, L)], flag=16 * (i % 2))
        spot = spots[(i // 4) % 8]
        kind = (i // 32) % 4
        if kind == 0:
            r.codes[spot] = NN                                      # N, counted
        elif kind == 1:
            r.codes[spot] = NN; r.qual[spot] = 19                   # N below min_quality, between good bases (the windows pass)
        elif kind == 2:
            r.codes[L - 1] = NN                                     # N as the last base: l_seq % 8 of 1 and 7 reach the pad-nibble rewrite
        else:
            r.codes[spot] = R_; r.qual[spot] = 19                   # an IUPAC code that is skipped
        if i % 64 == 0:
            r.codes[:32] = NN                                       # first read of a tile: the 16 bytes behind the run before it
        reads.append(r)
    r = mk(rng, 60 + 200, [(M, 100)]); r.codes[40] = R_            # an IUPAC code at min_quality: refused (no column for it)
    reads.append(r)
    reads = by_pos(reads)
    fails = [i for i, r in enumerate(reads) if any(c == R_ and q >= 20 for c, q in zip(r.codes, r.qual))]
    cases.append(Case("G_codes_outside_acgt", reads, G=500, fails=fails, slack="iupac",
                      reach=lambda b: {97 % 8, 103 % 8} == {1, 7} and NN in unpack_codes(b) and R_ in unpack_codes(b),
                      why="N has a column: counted by the careful loop, never handed over.  Bound for the IUPAC reads: their piece is "
                          "redone base by base and asks for the exact status only when such a base is counted"))
    return cases


def _family_h():
    return [Case("H_pile_of_150", G=600, pile=dict(L=150), reach=lambda b: True,
                 why="16 increments per tile and a fold every F_FLUSH tiles: 240 of 255 per packed byte"),
            Case("H_pile_of_150_every_second_shifted", G=600, pile=dict(L=150, shift=True), reach=lambda b: True),
            Case("H_pile_of_151", G=600, pile=dict(L=151), reach=lambda b: True)]


def _ins_tile(rng, pos, pattern):
    """64 reads 40M 8I 40M; pattern[lane] = number of events the lane's insertion yields (0: a plain read)."""
    quals = {1: [40] * 8, 2: [40, 40, 40, 2, 40, 40, 40, 40], 4: [40, 2, 40, 2, 40, 2, 40, 2]}
    out = []
    for lane in range(64):
        if pattern[lane] == 0:
            out.append(mk(rng, pos, [(M, 88)]))
        else:
            r = mk(rng, pos, [(M, 40), (I, 8), (M, 40)], flag=16 * (lane % 2))
            r.qual[40:48] = quals[pattern[lane]]
            out.append(r)
    return out


def _family_i():
    rng = np.random.default_rng(900)
    tiles = {63: [1] * 63 + [0], 64: [1] * 64, 65: [1] * 63 + [2], 256: [4] * 64}
    cases = [Case("I_tile_of_%d_events" % ev, _ins_tile(rng, 200, pat), G=600,
                  reach=lambda b, pat=pat: int((np.diff(b.cig_off.astype(np.int64)) == 3).sum()) == sum(1 for p in pat if p), why="an F_EVGRAN granule of %d slots against %d events" % (F_EVGRAN, ev)) for ev, pat in tiles.items()]
    for c, ev in zip(cases, tiles):
        c.events = ev
    reads = []
    for t in range(32):           # four tiles per wave of a block, 256 events each: every wave refills its granule tile after tile
        reads += _ins_tile(rng, 200 + t, tiles[256])
    c = Case("I_tiles_of_256_events_back_to_back", reads, G=600, reach=lambda b: b.n == 32 * TILE and not off_limit(b, F_MAXLEN).any())
    c.events = 32 * 256
    return cases + [c]


def _family_j():
    cases = []
    rng = np.random.default_rng(1000)
    plain = lambda p: mk(rng, p, [(M, 150)])
    off = lambda p: mk(rng, p, [(M, 60), (D, 17), (M, 90)])            # past F_MAXDEL: on the list of every fast kernel
    cases.append(Case("J_nobody_on_the_list", [plain(100 + i // 4) for i in range(320)], G=600, reach=lambda b: not off_limit(b, F_MAXLEN).any()))
    cases.append(Case("J_everybody_on_the_list", [mk(rng, 100 + i // 4, [(H, 2), (S, 3), (M, 60), (D, 4), (M, 80), (S, 2)]) for i in range(320)],
                      G=600, reach=lambda b: off_limit(b).all()))
    cases.append(Case("J_odd_reads_on_the_list", [off(100 + i // 4) if i % 2 else plain(100 + i // 4) for i in range(320)], G=600,
                      reach=lambda b: np.array_equal(off_limit(b), np.arange(b.n) % 2 == 1)))
    cases.append(Case("J_last_read_on_the_list", [plain(100 + i // 4) for i in range(319)] + [off(180)], G=600,
                      reach=lambda b: np.array_equal(np.nonzero(off_limit(b))[0], [b.n - 1])))
    # op counts at the tile kernel's limit, between plain reads
    lim = T_MAXOPS - 3
    reads = []
    for i in range(256):
        reads.append(many_ops(rng, 100 + i, lim + (i // 4) % 2, lead_clip=(i // 8) % 2 == 1) if i % 4 == 0 else plain(100 + i))
    cases.append(Case("J_ops_%d_and_%d" % (lim, lim + 1), reads, G=700,
                      reach=lambda b, lim=lim: {lim, lim + 1} <= set(np.diff(b.cig_off.astype(np.int64)).tolist()),
                      why="T_MAXOPS - 3 input ops stay with k_tile<LIST>, one more is a heavy entry"))
    # k_long's limit: eight ops a read on average switch it on
    lim = L_MAXOPS - 4
    reads = [many_ops(rng, 100 + i, (lim, lim + 1, 21, 40)[i % 4], seg=2) for i in range(192)]
    cases.append(Case("J_ops_%d_and_%d_long_kernel" % (lim, lim + 1), reads, G=900,
                      reach=lambda b, lim=lim: {lim, lim + 1} <= set(np.diff(b.cig_off.astype(np.int64)).tolist()) and int(b.cig_off[b.n]) >= 8 * b.n,
                      why="bound on the heavy entries: k_long takes entries of up to L_MAXOPS - 4 ops and may hand reads back"))
    # the wave path's limit, with k_long off (few such reads among many plain ones) and on
    lim = WV_MAXOPS - 4
    for name, n_plain in (("", 700), ("_long_kernel", 40)):
        reads = [plain(100 + i % 300) for i in range(n_plain)] + [many_ops(rng, 150 + 20 * i, lim + i % 2, seg=2) for i in range(4)]
        cases.append(Case("J_ops_%d_and_%d%s" % (lim, lim + 1, name), by_pos(reads), G=2000,
                          reach=lambda b, on=bool(name), lim=lim: {lim, lim + 1} <= set(np.diff(b.cig_off.astype(np.int64)).tolist())
                          and (int(b.cig_off[b.n]) >= 8 * b.n) == on,
                          why="WV_MAXOPS - 4 ops fit a wave's CIGAR row, one more takes the serial path"))
    # op lengths summing to 4095 and 4096
    reads = []
    for i in range(192):
        reads.append(mk(rng, 100 + i, [(M, 2000), (D, 5), (M, 2090 + (i // 16) % 2)]) if i % 16 == 0 else plain(100 + i))
    cases.append(Case("J_op_lengths_of_4095_and_4096", reads, G=4700,
                      reach=lambda b: {4095, 4096} <= {sum(k for _, k in c) for c in _cigars(b)},
                      why="16-bit CIGAR columns: lengths summing to 4096 are a heavy entry, 4095 are not"))
    reads = [plain(100 + i) for i in range(130)]
    reads[40] = mk(rng, 140, [(M, 65535)]); reads[100] = mk(rng, 200, [(M, 65536)])
    cases.append(Case("J_reads_of_65535_and_65536", reads, G=66000, reach=lambda b: {65535, 65536} <= set(b.lseq.tolist())))
    return cases


def _all():
    cases = []
    for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h, _family_i, _family_j):
        cases += fam()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = _all()
BY_NAME = {c.name: c for c in CASES}
