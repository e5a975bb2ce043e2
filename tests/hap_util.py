"""TEST INFRASTRUCTURE of the read haplotypes: a plain restatement over Segments, written from the
definition in the header comment of amplipy_amd/csrc/amp_hap.hpp position by position, and from none of its functions; the
kernel's constants as Python values (tests/test_hap_twin.py holds them to the header); the key and the hash restated, for the
tests that craft colliding keys; a generator of reads that ARE the reference but for a seeded rate of substitutions and a
few planted variants (the QC mix draws bases at random: against a reference nearly every trial would overflow); and the
crafted edges the twin and the device test share."""
import numpy as np

from amplipy_amd import abi
from amplipy_amd.batch import ReadBatch
from amplipy_amd.segment import Segment
from tests import codon_util as CU

MAX_DIFFS, MAX_REGION, TALLY_COLS, KEY_WORDS = 13, 4096, 6, 14
GLOBAL_PROBES, LOG2_DEFAULT, BLOCK = 4096, 20, 256
COVER, REF, REF_REV, LOWQ, OVERFLOW, EDGE = range(6)
KIND_N, KIND_DEL = 4, 5
EMPTY = 0xFFFFFFFF
M64 = (1 << 64) - 1
BASES = "ACGT"


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


def judge(base, deleted, start, end, ref_seq, min_quality):
    """One trial: -> (column or None, differences): EDGE, LOWQ, OVERFLOW, REF, or None with the read's differences."""
    if start in deleted or end - 1 in deleted:
        return EDGE, None
    differs = lambda p: ref_seq[p].upper() in BASES and base[p][0] != ref_seq[p].upper()
    if any(p not in deleted and differs(p) and base[p][1] < min_quality for p in range(start, end)):
        return LOWQ, None
    diffs = []
    p = start
    while p < end:
        if p in deleted:
            q = p
            while q in deleted:
                q += 1
            assert start < p and q < end        # (behind the EDGE test: both flanks lie inside)
            diffs.append((p - start, KIND_DEL, q - p))
            p = q
            continue
        if differs(p):
            diffs.append((p - start, BASES.index(base[p][0]) if base[p][0] in BASES else KIND_N, 0))
        p += 1
    if len(diffs) > MAX_DIFFS:
        return OVERFLOW, None
    if not diffs:
        return REF, None
    return None, tuple(diffs)


def read_trials(seg, ref_len, regions, ref_seq, min_quality):
    """[(region, column or None, differences)] of a read with status 0, or None when the read is not regular."""
    if not CU.is_regular(seg, ref_len):
        return None
    base, deleted, pos, end = alignment(seg)
    out = []
    for k, (s, e) in enumerate(regions):
        if pos <= s and e <= end:
            out.append((k,) + judge(base, deleted, s, e, ref_seq, min_quality))
    return out


def tables(segments, ref_len, regions, ref_seq, min_quality):
    """({(region, differences): [count, rev]}, tally uint64[n_regions][6], reads uint64[2]) of reads with status 0."""
    table = {}
    tally = [[0] * TALLY_COLS for _ in regions]
    reads = [0, 0]
    for seg in segments:
        trials = read_trials(seg, ref_len, regions, ref_seq, min_quality)
        reads[0 if trials else 1] += 1
        rev = 1 if seg.flag & 0x10 else 0
        for k, col, diffs in trials or ():
            tally[k][COVER] += 1
            if col is None:
                c = table.setdefault((k, diffs), [0, 0])
                c[0] += 1; c[1] += rev
            else:
                tally[k][col] += 1
                if col == REF:
                    tally[k][REF_REV] += rev
    return table, np.array(tally, np.uint64).reshape(len(regions), TALLY_COLS), np.array(reads, np.uint64)


def add_tables(a, b):
    out = {k: list(v) for k, v in a.items()}
    for k, v in b.items():
        c = out.setdefault(k, [0, 0])
        c[0] += v[0]; c[1] += v[1]
    return out


def check_invariant(table, tally, lost=0):
    """COVER == REF + LOWQ + OVERFLOW + EDGE + the counts of the region's entries (+ the lost reads, known for the job only)."""
    tally = np.asarray(tally).astype(np.int64)
    held = np.zeros(len(tally), np.int64)
    for (k, _), (c, r) in table.items():
        assert 0 <= r <= c
        held[k] += c
    rest = tally[:, COVER] - tally[:, [REF, LOWQ, OVERFLOW, EDGE]].sum(axis=1) - held
    assert (rest >= 0).all() and int(rest.sum()) == lost, (rest, lost)
    assert (tally[:, REF_REV] <= tally[:, REF]).all()


# ---- keys, entries and the hash, restated -----------------------------------------------------------------------------------
def diff_word(off, kind, length):
    return off | (kind << 12) | (length << 15)


def key_words(region, diffs):
    return [region | (len(diffs) << 16)] + [diff_word(*d) for d in diffs] + [0] * (MAX_DIFFS - len(diffs))


def as_array(table):
    """The table as amp_hap_get gives it: abi.HAP_ENTRY_DTYPE ordered by the 14 key words."""
    rows = sorted((key_words(*k), v) for k, v in table.items())
    out = np.zeros(len(rows), abi.HAP_ENTRY_DTYPE)
    for j, (w, v) in enumerate(rows):
        out[j] = (w[0], w[1:], v[0], v[1])
    return out


def as_dict(entries):
    out = {}
    for e in entries:
        head = int(e["head"])
        n = head >> 16
        words = [int(w) for w in e["diff"]]
        assert 1 <= n <= MAX_DIFFS and not any(words[n:]) and all(w >> 28 == 0 for w in words)
        key = (head & 0xFFFF, tuple((w & 0xFFF, (w >> 12) & 7, (w >> 15) & 0x1FFF) for w in words[:n]))
        assert key not in out
        out[key] = [int(e["count"]), int(e["rev"])]
    return out


def mix(words):
    h = 0x9e3779b97f4a7c15
    for w in words:
        h = ((h ^ w) * 0xff51afd7ed558ccd) & M64
        h ^= h >> 32
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 33
    return h


def slot_global(region, diffs, log2_capacity):
    return (mix(key_words(region, diffs)) >> 32) & ((1 << log2_capacity) - 1)


# ---- a reference, and reads that are the reference but for a few bases --------------------------------------------------------
def reference(ref_len, seed=1):
    """Seeded A C G T with a lower-case stretch every 500 bases and an N every 97."""
    rng = np.random.default_rng(seed)
    ref = [BASES[k] for k in rng.integers(0, 4, size=ref_len)]
    for a in range(230, ref_len, 500):
        ref[a:a + 30] = [c.lower() for c in ref[a:a + 30]]
    for a in range(41, ref_len, 97):
        ref[a] = "N"
    return "".join(ref)


def onto_reference(batch, ref_seq, seed, rate=0.01, planted=(), low_rate=0.0):
    """The batch with every match base set to the reference's letter, then: each base changed with probability ``rate`` (one in
    ten of those to N); ``planted``: [(position, base, one read in how many)]; low_rate: the share of bases whose quality is
    set to 5 (0: the mix's own qualities stay).  Inserted and clipped bases stay as drawn."""
    rng = np.random.default_rng(seed)
    segs = []
    for i in range(batch.n):
        s = batch.segment(i)
        seq = list(s.query_sequence)
        qual = list(s.query_qualities) if s.query_qualities is not None else None
        q, r = 0, s.reference_start
        for op, n in s.cigartuples:
            if op in (0, 7, 8):
                for k in range(n):
                    if 0 <= r + k < len(ref_seq):
                        c = ref_seq[r + k].upper()
                        if rng.random() < rate:
                            c = "N" if rng.random() < 0.1 else BASES[(BASES.find(c) + 1 + int(rng.integers(0, 3))) % 4]
                        for p, b, every in planted:
                            if p == r + k and i % every == 0:
                                c = b
                        seq[q + k] = c
                        if qual is not None and low_rate and rng.random() < low_rate:
                            qual[q + k] = 5
                q += n; r += n
            elif op in (1, 4):
                q += n
            elif op in (2, 3):
                r += n
        s.query_sequence = "".join(seq)
        if qual is not None:
            s.query_qualities = type(s.query_qualities)("B", qual)
        segs.append(s)
    return ReadBatch.from_segments(segs)


def regions_near(primers, ref_len):
    """Regions of 1, 2, 16, 17, 40 and 100 positions behind every primer, overlapping ones and ones with equal starts among them,
    sorted by start."""
    out = []
    for s, e in primers:
        for a, n in ((e + 5, 1), (e + 5, 2), (e + 8, 16), (e + 8, 17), (e + 10, 40), (e + 20, 40), (e + 12, 100), (s + 2, 30), (e + 45, 1)):
            if a + n <= ref_len:
                out.append((a, a + n))
    return sorted(out)


# ---- crafted reads ----------------------------------------------------------------------------------------------------------
CRAFT_G = 5000
CRAFT_PRIMERS = [(100, 130), (400, 430)]


def _craft_reference():
    """Seeded upper-case A C G T but for one N at 1650 and a lower-case stretch [1730, 1760): the crafted cases know where."""
    rng = np.random.default_rng(2)
    ref = [BASES[k] for k in rng.integers(0, 4, size=CRAFT_G)]
    ref[1650] = "N"
    ref[1730:1760] = [c.lower() for c in ref[1730:1760]]
    return "".join(ref)


CRAFT_REF = _craft_reference()
M_, I_, D_, N_, S_ = 0, 1, 2, 3, 4


def other(c, k=1):
    """A base that is not ``c`` (upper-cased)."""
    return BASES[(BASES.find(c.upper()) + k) % 4] if c.upper() in BASES else "A"


def rd(pos, cigar, edits=None, qual=35, low=(), flag=0, ref_seq=None):
    """A read that is the reference over its match ops (a reference N is read as A); edits: {reference position: base};
    low: reference positions whose base has quality 5; qual None: QUAL '*'."""
    ref_seq = CRAFT_REF if ref_seq is None else ref_seq
    edits = edits or {}
    seq, quals = [], []
    r = pos
    for op, n in cigar:
        if op in (0, 7, 8):
            for k in range(n):
                c = ref_seq[r + k].upper()
                seq.append(edits.get(r + k, c if c in BASES else "A"))
                quals.append(5 if r + k in low else qual)
            r += n
        elif op in (1, 4):
            seq += ["G"] * n; quals += [qual] * n
        elif op in (2, 3):
            r += n
    return Segment(flag=flag, reference_start=pos, cigar=cigar, query_sequence="".join(seq), query_qualities=None if qual is None else quals)


def ok(cond):
    assert cond


def copy_of(seg, flag):
    """The same read with another FLAG."""
    return Segment(flag=flag, reference_start=seg.reference_start, cigar=seg.cigartuples, query_sequence=seg.query_sequence,
                   query_qualities=list(seg.query_qualities), template_length=seg.template_length)


def covering_and_non_ref(segments, ref_len, regions, ref_seq, min_quality):
    """(reads that cover some region, those of them with a keyed trial: a non-reference signature) of reads with status 0."""
    cover = keyed = 0
    for seg in segments:
        trials = read_trials(seg, ref_len, regions, ref_seq, min_quality)
        if trials:
            cover += 1
            keyed += any(col is None for _, col, _ in trials)
    return cover, keyed


def sub(region_start, pos, base):
    return (pos - region_start, BASES.index(base) if base in BASES else KIND_N, 0)


def crafted():
    """[(name, regions, segments, min_quality, do_trim, expect)] on CRAFT_REF with CRAFT_PRIMERS: ``expect(table, tally, reads)``
    asserts what the case is about on the restatement's, the twin's and the device's tables alike."""
    out = []
    R = CRAFT_REF
    plain = lambda p: R[p].upper() in BASES and R[p].isupper()

    def case(name, regions, segs, expect, mq=20, do_trim=False):
        assert regions == sorted(regions, key=lambda x: x[0])
        out.append((name, regions, segs, mq, do_trim, expect))

    def cols(tally, k):
        return [int(x) for x in tally[k]]

    # regions of 1, 2, 16, 17 and 4096 positions; a difference at offset 0 and at the last offset (4095: the top offset bit)
    a, z = 600, 600 + 4095
    assert plain(a) and plain(z)
    regs = [(a, a + 1), (a, a + 2), (a, a + 16), (a, a + 17), (a, a + 4096)]
    ea, ez = other(R[a]), other(R[z], 2)
    segs = [rd(590, [(M_, 4200)], {a: ea, z: ez}), rd(590, [(M_, 4200)]), rd(590, [(M_, 4200)], flag=0x10)]

    def sizes(t, tally, reads):
        want = {(k, (sub(a, a, ea),)): [1, 0] for k in range(4)}
        want[(4, (sub(a, a, ea), sub(a, z, ez)))] = [1, 0]
        assert t == want and all(cols(tally, k) == [3, 2, 1, 0, 0, 0] for k in range(5)) and list(reads) == [3, 0]
    case("region_sizes_and_the_last_offset", regs, segs, sizes)

    # a region equal to [pos, ref_end) exactly, and one position longer on either side (not covered)
    case("exact_cover", [(699, 800), (700, 800), (700, 801)], [rd(700, [(M_, 100)])],
         lambda t, tally, reads: ok(t == {} and [cols(tally, k) for k in range(3)] == [[0] * 6, [1, 1, 0, 0, 0, 0], [0] * 6] and list(reads) == [1, 0]))

    # regions that overlap, regions with equal starts; reads that cover 0, 1 and 5 regions
    regs = [(1000, 1010), (1000, 1020), (1005, 1015), (1005, 1030), (1012, 1040), (2000, 2010)]
    segs = [rd(1500, [(M_, 60)]), rd(1000, [(M_, 12)]), rd(995, [(M_, 50)], {1013: other(R[1013])}), rd(995, [(M_, 50)], flag=0x10)]
    assert plain(1013)

    def overlap(t, tally, reads):
        e = other(R[1013])
        assert t == {(1, (sub(1000, 1013, e),)): [1, 0], (2, (sub(1005, 1013, e),)): [1, 0], (3, (sub(1005, 1013, e),)): [1, 0], (4, (sub(1012, 1013, e),)): [1, 0]}
        assert [cols(tally, k)[:3] for k in range(6)] == [[3, 3, 1], [2, 1, 1], [2, 1, 1], [2, 1, 1], [2, 1, 1], [0, 0, 0]] and list(reads) == [3, 1]
    case("overlapping_and_equal_starts", regs, segs, overlap)

    # exactly 13 differences and exactly 14 (OVERFLOW)
    ps = [p for p in range(1100, 1160) if plain(p)][:14]
    e13 = {p: other(R[p]) for p in ps[:13]}
    e14 = {p: other(R[p]) for p in ps}

    def thirteen(t, tally, reads):
        assert t == {(0, tuple(sub(1100, p, e13[p]) for p in ps[:13])): [2, 1]} and cols(tally, 0) == [3, 0, 0, 0, 1, 0]
    case("thirteen_and_fourteen_differences", [(1100, 1160)], [rd(1090, [(M_, 100)], e13), rd(1090, [(M_, 100)], e13, flag=0x10), rd(1090, [(M_, 100)], e14)], thirteen)

    # a deletion run of 1, and of 4094 inside a region of 4096 (the length bits)
    case("deletion_runs_of_1_and_4094", [(600, 4696), (610, 620)], [rd(600, [(M_, 1), (D_, 4094), (M_, 1)]), rd(605, [(M_, 10), (D_, 1), (M_, 10)], flag=0x10)],
         lambda t, tally, reads: ok(t == {(0, ((1, KIND_DEL, 4094),)): [1, 0], (1, ((5, KIND_DEL, 1),)): [1, 1]} and list(reads) == [2, 0]))

    # a deleted first position and a deleted last position: EDGE, tested in front of LOWQ
    assert plain(1205)
    segs = [rd(1190, [(M_, 10), (D_, 3), (M_, 30)], {1205: other(R[1205])}, low={1205}),      # 1200..1202 deleted, a low-quality mismatch at 1205
            rd(1190, [(M_, 18), (D_, 4), (M_, 20)]),                                           # 1208..1211 deleted
            rd(1190, [(M_, 11), (D_, 2), (M_, 30)], {1205: other(R[1205])}, low={1205})]       # 1201..1202 deleted: inside; the mismatch decides
    case("edge_in_front_of_lowq", [(1200, 1210)], segs, lambda t, tally, reads: ok(t == {} and cols(tally, 0) == [3, 0, 0, 1, 0, 2]))

    # 3D2D as one run; a D op with an insertion behind it, then another D: one run; a D, an insertion, a match: the run ends
    segs = [rd(1290, [(M_, 15), (D_, 3), (D_, 2), (M_, 20)]), rd(1290, [(M_, 15), (D_, 3), (I_, 2), (N_, 2), (M_, 20)], flag=0x10),
            rd(1290, [(M_, 15), (D_, 5), (I_, 4), (M_, 20)]), rd(1290, [(M_, 15), (D_, 3), (I_, 1), (M_, 22)])]
    case("neighbouring_deletions_are_one_run", [(1300, 1320)], segs,
         lambda t, tally, reads: ok(t == {(0, ((5, KIND_DEL, 5),)): [3, 1], (0, ((5, KIND_DEL, 3),)): [1, 0]} and cols(tally, 0) == [4, 0, 0, 0, 0, 0]))

    # an insertion inside the region is ignored: with and without it the reads fall together
    assert plain(1410)
    e = other(R[1410])
    segs = [rd(1390, [(M_, 50)]), rd(1390, [(M_, 15), (I_, 3), (M_, 35)]), rd(1390, [(M_, 50)], {1410: e}), rd(1390, [(M_, 25), (I_, 1), (M_, 25)], {1410: e}, flag=0x10)]
    case("insertions_are_ignored", [(1400, 1420)], segs,
         lambda t, tally, reads: ok(t == {(0, (sub(1400, 1410, e),)): [2, 1]} and cols(tally, 0) == [4, 2, 0, 0, 0, 0]))

    # a low-quality mismatch: LOWQ; a low-quality match: REF; quality at the threshold counts
    assert plain(1505)
    e5 = other(R[1505])
    segs = [rd(1490, [(M_, 40)], {1505: e5}, low={1505}), rd(1490, [(M_, 40)], low={1505, 1506}), rd(1490, [(M_, 40)], {1505: e5}, qual=20), rd(1490, [(M_, 40)], {1505: e5}, qual=19)]
    case("low_quality", [(1500, 1510)], segs, lambda t, tally, reads: ok(t == {(0, (sub(1500, 1505, e5),)): [1, 0]} and cols(tally, 0) == [4, 1, 0, 2, 0, 0]))

    # QUAL '*': the count walk gives the read a status (it adds nothing at all); an irregular CIGAR (a soft clip inside): reads[1]
    segs = [rd(1490, [(M_, 40)], qual=None), rd(1490, [(M_, 10), (S_, 2), (M_, 28)]), rd(1490, [(M_, 40)])]
    case("no_qual_and_irregular", [(1500, 1510)], segs, lambda t, tally, reads: ok(t == {} and cols(tally, 0) == [1, 1, 0, 0, 0, 0] and list(reads) == [1, 1]))

    # a reference letter N is never a difference; a lower-case letter is one like its upper-case twin
    n_at = next(p for p in range(1600, 1700) if R[p] == "N")
    lc = next(p for p in range(1700, 2300) if R[p].islower())
    segs = [rd(n_at - 20, [(M_, 40)], {n_at: "C"}), rd(n_at - 20, [(M_, 40)], {n_at: "C"}, low={n_at}), rd(lc - 20, [(M_, 40)], {lc: other(R[lc])}), rd(lc - 20, [(M_, 40)], {lc: R[lc].upper()})]
    case("reference_n_and_lower_case", [(n_at - 5, n_at + 5), (lc - 5, lc + 5)], segs,
         lambda t, tally, reads: ok(t == {(1, (sub(lc - 5, lc, other(R[lc])),)): [1, 0]} and cols(tally, 0) == [2, 2, 0, 0, 0, 0] and cols(tally, 1) == [2, 1, 0, 0, 0, 0]))

    # a read base N at good quality: kind 4; a reverse read: rev
    assert plain(2405)
    segs = [rd(2390, [(M_, 40)], {2405: "N"}), rd(2390, [(M_, 40)], {2405: "N"}, flag=0x10), rd(2390, [(M_, 40)], {2405: "N"}, flag=0x10 | 0x1)]
    case("read_base_n_and_reverse", [(2400, 2410)], segs, lambda t, tally, reads: ok(t == {(0, ((5, KIND_N, 0),)): [3, 2]}))

    # a trim that moves pos past a region's start: not covered; the same read untrimmed covers it
    segs = [rd(105, [(M_, 100)])]
    case("trimmed_past_the_start", [(120, 150), (140, 150)], segs, lambda t, tally, reads: ok(cols(tally, 0)[0] == 0 and cols(tally, 1)[:2] == [1, 1] and list(reads) == [1, 0]), do_trim=True)
    case("the_same_read_untrimmed", [(120, 150), (140, 150)], segs, lambda t, tally, reads: ok(cols(tally, 0)[:2] == [1, 1] and cols(tally, 1)[:2] == [1, 1]))

    # a read with a status (it lies past the reference) adds nothing at all
    segs = [rd(2390, [(M_, 40)]), Segment(flag=0, reference_start=CRAFT_G + 5, cigar=[(M_, 40)], query_sequence="A" * 40, query_qualities=[35] * 40)]
    case("a_read_with_a_status", [(2400, 2410)], segs, lambda t, tally, reads: ok(cols(tally, 0)[:2] == [1, 1] and list(reads) == [1, 0]), do_trim=True)
    return out


def pile_case(n=1500):
    """``n`` reads that carry ONE non-reference haplotype on one region (every third reverse).  -> (regions, segments, key)"""
    R = CRAFT_REF
    ps = [p for p in range(3005, 3030) if R[p] in BASES][:3]
    edits = {p: other(R[p]) for p in ps}
    segs = [rd(2990, [(M_, 40), (D_, 2), (M_, 40)], edits, flag=0x10 if k % 3 == 0 else 0) for k in range(n)]
    diffs = tuple(sorted([sub(3000, p, edits[p]) for p in ps] + [(30, KIND_DEL, 2)]))
    return [(3000, 3050)], segs, (0, diffs)


def distinct_keys_case(n_keys=200):
    """One read per key, ``n_keys`` keys on one region: more distinct keys than a wave has lanes.  -> (regions, segments)"""
    R = CRAFT_REF
    ps = [p for p in range(3100, 3200) if R[p] in BASES]
    segs = []
    for k in range(n_keys):
        a, b = ps[k % 50], ps[50 + (k // 50) % 30]
        segs.append(rd(3090, [(M_, 130)], {a: other(R[a], 1 + k // 50 % 3), b: other(R[b])}, flag=0x10 if k % 2 else 0))
    return [(3100, 3200)], segs


def thirteen_diff_reads(region, variants, flag_of=lambda k: 0):
    """Reads over ``region`` = (start, end) of CRAFT_REF with 13 differences each: the first twelve the same, the thirteenth (the
    LAST key word) one of ``variants``: [(position index, which other base)].  -> (segments, keys)"""
    R = CRAFT_REF
    s, e = region
    ps = [p for p in range(s, e) if R[p] in BASES]
    fixed = {p: other(R[p]) for p in ps[:12]}
    segs, keys = [], []
    for k, (j, which) in enumerate(variants):
        p = ps[12 + j]
        edits = dict(fixed); edits[p] = other(R[p], which)
        segs.append(rd(s - 10, [(M_, e - s + 20)], edits, flag=flag_of(k)))
        keys.append((0, tuple(sub(s, q, edits[q]) for q in sorted(edits))))
    return segs, keys
