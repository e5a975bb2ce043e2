"""The insertion evidence on the device (k_insev, amp_insev.hip) behind the real read pass, against the
plain restatement of tests/insev_util.py: the crafted batches under do_trim on and off and on the three routes of the read pass;
event counts round the wave and one more than the grid takes in a stride; one key in 64 lanes and 64 keys; reserved slots left
unused; every drain pattern; the switch turned on over a list that holds events; read ids that wrap; amp_reset; an event list
that grows; a table that is full; amp_insev_add; the two halves of the indel unit apart and together, beside all nine hooks;
and the command line, one process and two ranks.  Integers and bytes: the bar is equality."""
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from amplipy_amd import abi, amplipy, insevidence, lib
from amplipy_amd.batch import ReadBatch
from oracle import oracle
from tests import insev_util as U
from tests import readpass_craft as K
from tests.ins_util import slots_in_use
from tests.readpass_craft import I, M

pytestmark = pytest.mark.gpu

MQ, W = U.MQ, U.W


def engine(G, tabs, do_trim=True, log2=0, insev=True):
    eng = lib.Engine(G)
    eng.set_primers(*tabs)
    eng.set_params(MQ, W, do_trim, True)
    if insev:
        eng.insev_enable(log2)
    return eng


def got(eng, lost=0):
    entries, info = eng.insev_entries()
    assert info["used"] == entries.size and info["lost"] == lost
    order = np.lexsort((entries["hash"], entries["len"], entries["ref_pos"]))
    assert np.array_equal(order, np.arange(entries.size)), "amp_insev_get orders by (ref_pos, len, hash)"
    return U.entries_dict(entries)


def simple(reads, G=600):
    return U.Crafted("simple", reads, G)


# ---- 1. the crafted batches through the real read pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("do_trim", [True, False], ids=["trim", "no_trim"])
@pytest.mark.parametrize("name", ["edges", "corners", "primer", "untrimmed"])
def test_crafted_batches(name, do_trim):
    case = U.crafted()[name]
    eng = engine(case.G, case.tabs, do_trim)
    try:
        res = eng.process(case.batch)
        assert np.array_equal(res.status, case.status(do_trim)) and int((res.status != 0).sum()) == (name in ("corners", "untrimmed"))     # (QUAL '*')
        assert got(eng) == U.by_key(case.want_accepted(do_trim))
        assert eng.insev_last_ms() > 0
        with pytest.raises(lib.AmpliHipError):
            eng.del_last_ms()                   # (k_del did not run: the deletion half is off)
    finally:
        eng.close()


@pytest.mark.parametrize("do_trim", [True, False], ids=["trim", "no_trim"])
@pytest.mark.parametrize("name", ["short", "irregular", "many ops"])
def test_routes_of_the_read_pass(name, do_trim):
    """Plain short reads (the fast kernel alone), irregular reads beside them (the general pass and the second pass), reads of
    forty ops (the wave-per-read path): the route is looked at, then the table."""
    case = U.routes()[name]
    eng = engine(case.G, case.tabs, do_trim)
    try:
        res = eng.process(case.batch)
        assert not res.status.any() and not case.status(do_trim).any()
        kv, listed = eng.last_kernel_variant(), int(eng.debug_counters()[7])
        off = int(K.off_limit(case.batch).sum())
        print("%s: kernel variant %d, %d reads on the general list, %d off a fast kernel's limits" % (name, kv, listed, off))
        assert kv >= 4
        if name == "short":
            assert off == 0
        elif name == "irregular":
            assert off >= 50 and listed >= 90           # (the 90 irregular reads: all on the list, most of them off every fast kernel's limits)
        else:
            assert int(case.batch.cig_off[case.batch.n]) >= 8 * case.batch.n and listed == off == case.batch.n
            assert slots_in_use(eng) > eng.events().size, "no slot was reserved and left unused: the -1 path is not covered"
        assert got(eng) == U.by_key(case.want(do_trim))
    finally:
        eng.close()


# ---- 2. counts round the wave and the stride; one key and many ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, abi.INSEV_STRIDE + 1])
def test_event_counts(n):
    """n reads with one and the same insertion beside 40 without: the restatement of ONE read, n times."""
    one = simple(U.copies(1)).want()
    rng = np.random.default_rng(n % 1000)
    plain = [U.read(100, [(M, 44)], rng=rng) for _ in range(40)]
    if n <= 65:
        b = K.build_batch(plain + U.copies(n))
    else:
        b = U.uniform_batch(n)
    eng = engine(600, U.primer_tables(600, ()))
    try:
        eng.process(b)
        assert eng.events().size == n
        assert got(eng) == U.by_key(U.scaled(one, n) if n else {})
    finally:
        eng.close()


def test_64_lanes_one_key_and_64_lanes_64_keys():
    for reads in (U.copies(64), U.distinct(64), U.distinct(64) + U.copies(64) + U.distinct(64, first=64)):
        case = simple(reads)
        eng = engine(case.G, case.tabs)
        try:
            eng.process(case.batch)
            assert got(eng) == U.by_key(case.want())
        finally:
            eng.close()


# ---- 3. which events count ---------------------------------------------------------------------------------------------------------
def two_batches():
    a = simple(U.distinct(70) + U.copies(30))
    b = simple(U.distinct(50, first=40) + U.copies(9, "GATC"[:3]) + [r for r in U.corner_reads(np.random.default_rng(19)) if r.qual[0] != 0xFF])
    return a, b


def test_drain_between_batches_or_not():
    a, b = two_batches()
    want = U.by_key(U.add_tables(a.want(), b.want()))
    tables = []
    for pattern in ("drain", "aggregate drain", "none"):
        eng = engine(600, a.tabs)
        try:
            eng.process(a.batch, read_base=5)
            if pattern == "drain":
                assert eng.drain_events().size == 100
            elif pattern == "aggregate drain":
                eng.aggregate_events(read_base=5, drain=True)
            eng.process(b.batch, read_base=5 + a.batch.n)
            tables.append(got(eng))
        finally:
            eng.close()
    assert tables[0] == tables[1] == tables[2] == want


def test_switch_turned_on_over_a_list_that_holds_events():
    a, b = two_batches()
    eng = engine(600, a.tabs, insev=False)
    try:
        eng.process(a.batch)
        assert eng.events().size == 100
        eng.insev_enable()
        eng.process(b.batch, read_base=a.batch.n)
        assert got(eng) == U.by_key(b.want())
        eng.insev_disable()                     # off: the table stays readable and takes no more
        eng.process(a.batch, read_base=a.batch.n + b.batch.n)
        assert got(eng) == U.by_key(b.want())
    finally:
        eng.close()


def test_read_ids_that_wrap_inside_the_batch():
    a, _ = two_batches()
    eng = engine(600, a.tabs)
    try:
        eng.process(a.batch, read_base=(1 << 32) - 37)
        assert got(eng) == U.by_key(a.want())
    finally:
        eng.close()


def test_reset_between_batches():
    a, b = two_batches()
    eng = engine(600, a.tabs)
    try:
        eng.process(a.batch)
        eng.reset()
        assert got(eng) == {}
        eng.process(b.batch)
        assert got(eng) == U.by_key(b.want())
    finally:
        eng.close()


def test_an_event_list_that_grows_between_two_undrained_batches():
    small, big = simple(U.copies(5)), simple(U.distinct(3000) + U.copies(2000))
    eng = engine(600, small.tabs)
    try:
        eng.process(small.batch)
        cap_small = eng.debug_event_capacity()
        eng.process(big.batch, read_base=small.batch.n)
        cap_big = eng.debug_event_capacity()
        assert 0 < cap_small < cap_big, "the list did not grow between the batches: grow_events is not covered"
        assert eng.events().size == 5005
        assert got(eng) == U.by_key(U.add_tables(small.want(), big.want()))
    finally:
        eng.close()


# ---- 4. the table --------------------------------------------------------------------------------------------------------------------
def test_a_table_of_16_slots_offered_49_alleles():
    case = simple(U.distinct(48) + U.copies(9) + U.distinct(48))
    want = U.by_key(case.want())
    eng = engine(case.G, case.tabs, log2=abi.INSEV_LOG2_MIN)
    try:
        eng.process(case.batch)
        entries, info = eng.insev_entries()
        held = U.entries_dict(entries)
        assert info["used"] == 16 == len(held) and info["capacity"] == 16
        assert info["lost"] + sum(v[0] for v in held.values()) == sum(v[0] for v in want.values()) and info["lost"] > 0
        assert all(want[k] == v for k, v in held.items()), "a key of a full table has a wrong cell"
    finally:
        eng.close()
    for bad in (abi.INSEV_LOG2_MIN - 1, abi.INSEV_LOG2_MAX + 1):
        eng = engine(case.G, case.tabs, insev=False)
        with pytest.raises(lib.AmpliHipError) as e:
            eng.insev_enable(bad)
        assert "insertion evidence table" in str(e.value)
        eng.close()


def test_insev_add_of_a_table_onto_itself_doubles_every_cell():
    case = U.crafted()["corners"]
    eng = engine(case.G, case.tabs)
    try:
        with pytest.raises(lib.AmpliHipError):
            lib.Engine(case.G).insev_entries()          # before the first enable
        eng.process(case.batch)
        entries, _ = eng.insev_entries()
        eng.insev_add(entries)
        assert got(eng) == U.by_key(U.scaled(case.want_accepted(), 2))
        eng.insev_enable(10)                            # another capacity: laid out again, zero
        assert got(eng) == {}
        eng.insev_add(entries)
        # ... and a partial table of another rank with a read without qualities (the read pass refuses QUAL '*': the cell fills
        # through amp_insev_add alone)
        more = np.zeros(1, abi.INSEV_ENTRY_DTYPE)
        more[0] = (273, 5, insevidence.allele_hash("TGGTT"), 1, 0, 1, 0, [0, 1, 0, 0, 0, 0, 0])
        eng.insev_add(more)
        assert got(eng) == U.by_key(case.want()) != U.by_key(case.want_accepted())
    finally:
        eng.close()


# ---- 5. the two halves of the indel unit ---------------------------------------------------------------------------------------------
def indel_case():
    """540 reads: 300 with a deletion on both strands, 40 with insertions of their own, 200 with one and the same."""
    rng = np.random.default_rng(3)
    dels = [U.read(100 + k % 7, [(M, 20), (K.D, 3 + k % 2), (M, 30)], rng=rng, flag=16 * (k & 1)) for k in range(300)]
    return simple(K.by_pos(dels + U.distinct(40, pos=104) + U.copies(200, pos=103)))


def test_either_half_alone_and_both():
    """The deletion table's bytes are the same with the insertion half on beside it; the insertion table is the same with the
    deletion half beside it; amp_del_enable(0) switches the deletion half off only."""
    case = indel_case()
    snaps = {}
    for halves in ("del", "ins", "both"):
        eng = engine(case.G, case.tabs, insev=halves != "del")
        try:
            if halves != "ins":
                eng.del_enable()
            eng.process(case.batch)
            snaps[halves] = (eng.del_events()[0].tobytes() if halves != "ins" else None, got(eng) if halves != "del" else None, eng.counts().tobytes())
            if halves == "ins":
                with pytest.raises(lib.AmpliHipError):
                    eng.del_events()                    # (as before the first amp_del_enable)
            if halves == "both":
                assert eng.del_last_ms() > 0 and eng.insev_last_ms() > 0
                eng.del_disable()
                eng.process(case.batch, read_base=case.batch.n)
                assert eng.del_events()[0].tobytes() == snaps["both"][0] and got(eng) == U.by_key(U.scaled(case.want(), 2))
        finally:
            eng.close()
    assert snaps["del"][0] == snaps["both"][0] and len(snaps["del"][0]) >= 2 * abi.DEL_EVENT_DTYPE.itemsize
    assert snaps["ins"][1] == snaps["both"][1] == U.by_key(case.want())
    assert snaps["del"][2] == snaps["ins"][2] == snaps["both"][2]


@pytest.mark.parametrize("first", ["insev", "del"])
def test_the_two_slots_are_independent(first):
    """In either enable order and with both tables filled: an enable of one unit at another capacity empties its own table and
    leaves the other's bytes; amp_reset empties both; a batch behind all that fills both to the restatements' values."""
    from tests import del_util
    case = indel_case()
    b = case.batch
    dels = del_util.table([b.segment(i) for i in range(b.n)], MQ, case.G)
    want_ins, want_del, want_del2 = U.by_key(case.want()), del_util.as_array(dels).tobytes(), del_util.as_array(del_util.add_tables(dels, dels)).tobytes()
    assert len(dels) >= 2 and len(want_ins) >= 41
    eng = engine(case.G, case.tabs, insev=False)
    try:
        for unit in (first, "del" if first == "insev" else "insev"):
            getattr(eng, unit + "_enable")()
        ins_bytes = lambda: eng.insev_entries()[0].tobytes()
        del_bytes = lambda: eng.del_events()[0].tobytes()
        eng.process(b)
        filled = ins_bytes()
        assert got(eng) == want_ins and del_bytes() == want_del
        eng.del_enable(12)                      # another capacity: the deletion table alone starts over
        assert del_bytes() == b"" and eng.del_events()[1]["capacity"] == 1 << 12 and ins_bytes() == filled
        eng.process(b, read_base=b.n)
        assert del_bytes() == want_del and got(eng) == U.by_key(U.scaled(case.want(), 2))
        eng.insev_enable(12)                    # ... and the converse
        assert ins_bytes() == b"" and eng.insev_entries()[1]["capacity"] == 1 << 12 and del_bytes() == want_del
        eng.process(b, read_base=2 * b.n)
        assert got(eng) == want_ins and del_bytes() == want_del2
        eng.reset()
        assert ins_bytes() == b"" and del_bytes() == b""
        eng.process(b)
        assert got(eng) == want_ins and ins_bytes() == filled and del_bytes() == want_del
    finally:
        eng.close()


def test_all_nine_hooks_beside_the_new_kernel():
    """Every other hook's tables are the same bytes with the insertion half on and off."""
    from amplipy_amd import codon, errprof
    from tests import amplicon_util as A
    from tests import codon_util as CU
    from tests import cooc_util as CO
    from tests import hap_util as HU
    from tests import strand_util as S
    amps, rows = A.example_amps(), A.example_rows()
    primers = sorted((s, e) for s, e, _ in rows)
    ref = HU.reference(amps.G, seed=3)
    regions = HU.regions_near(primers[:40], amps.G)
    tabs = oracle.find_overlapping_primers(amps.G, primers, 0)
    b = HU.onto_reference(S.strand_batch(1025, amps.G, primers, 2025), ref, 5, rate=0.01, low_rate=0.02)
    cds, sets = CU.overlapping(amps.G), CO.mixed_sets(amps.G)
    eng = lib.Engine(amps.G)
    eng.set_primers(*tabs)
    eng.set_params(MQ, W, True, True)
    snaps = []
    for with_insev in (False, True):
        eng.reset()
        eng.qc_enable(primers, 0, 60); eng.strand_enable(); amps.enable(eng); codon.enable(eng, cds); eng.del_enable(); eng.cooc_enable(*sets.arrays())
        errprof.enable(eng, ref, None)
        eng.hap_enable([s for s, _ in regions], [e for _, e in regions], ref, 0)
        eng.readpos_enable()
        if with_insev:
            eng.insev_enable()
        res = eng.process(b)
        t, ps, pe = eng.qc_read_tallies()
        h_ev, _, h_tally, h_reads = eng.hap_tables()
        snaps.append([np.array([t[k] for k in abi.QC_READ_FIELDS], np.uint64), ps, pe, *eng.strand_tables(), *eng.amplicon_tables(), *eng.codon_tables(),
                      eng.del_events()[0], *eng.cooc_tables(), *eng.errprof_tables(), h_ev, h_tally, h_reads, eng.readpos_tables(), eng.counts(),
                      res.status, res.new_pos, res.new_ncig, res.new_cig])
    assert len(snaps[0]) == len(snaps[1]) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(snaps[0], snaps[1]))
    # ... and the insertion table is the restatement's
    r = oracle.process(b, amps.G, *tabs, MQ, W, do_trim=True, do_count=True)
    assert not r.trim.status.any()
    want = U.restate(b, amps.G, tabs, True)[0]
    assert got(eng) == U.by_key(want) and sum(v[0] for v in want.values()) == r.events.size
    for h in ("qc", "strand", "amplicon", "codon", "del", "cooc", "errprof", "hap", "readpos", "insev"):
        assert getattr(eng, h + "_last_ms")() > 0
    eng.close()


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------
N_PLANTED = 240
ALLELE = "GATTA"


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """A small synthetic BAM: the seeded mix, 240 reads on both strands that carry one and the same insertion, 30 that carry
    insertions of their own -> (files, {do_trim: restated table}, reference, primer rows)."""
    from amplipy_amd import synth
    from tests import ins_util
    from tests import strand_util as S
    from tests.test_gpu_del import write_reads
    g = synth.make_genome()
    G, ref = int(g.size), synth.genome_string(g)
    primers, amps = synth.make_artic_scheme()
    pr = sorted((s, e) for s, e, _ in primers)
    a0 = int(amps[40][0])
    rng = np.random.default_rng(91)
    body = lambda n: "".join("ACGT"[k] for k in rng.integers(0, 4, n))
    left, right = body(70), body(60)
    planted = [ins_util.seg(a0 + 40 + k % 3, "%dM%dI60M" % (70 - k % 3, len(ALLELE) - 1), left[k % 3:] + ALLELE[1:] + right, flag=16 if k % 4 == 0 else 0)
               for k in range(N_PLANTED)]
    own = [ins_util.seg(a0 + 200 + k, "50M3I50M", body(103), flag=16 * (k & 1)) for k in range(30)]
    mix = S.strand_batch(800, G, pr, 41, sort=False)
    segs = sorted([mix.segment(i) for i in range(mix.n)] + planted + own, key=lambda s: s.reference_start)
    batch = ReadBatch.from_segments(segs)
    d = tmp_path_factory.mktemp("insev_cli")
    (d / "ref.fas").write_text(">SYN_REF test\n" + ref + "\n")
    synth.write_bed(str(d / "p.bed"), primers)
    files = dict(ref=str(d / "ref.fas"), bed=str(d / "p.bed"), bam=write_reads(str(d / "in.bam"), "wb", batch, G))
    tabs = oracle.find_overlapping_primers(G, pr, 0)
    want = {}
    for do_trim in (True, False):
        r = oracle.process(batch, G, *tabs, MQ, W, do_trim=do_trim, do_count=True)
        assert not r.trim.status.any()
        want[do_trim] = (U.restate(batch, G, tabs, do_trim)[0], r.counts)
        assert sum(v[0] for v in want[do_trim][0].values()) == r.events.size
    key = (a0 + 40 + 69, left[-1] + ALLELE[1:])
    assert want[False][0][key][:2] == [N_PLANTED, N_PLANTED // 4]
    return files, want, ref, key


def entries_of(table):
    out = np.zeros(len(table), abi.INSEV_ENTRY_DTYPE)
    for k, ((pos, text), v) in enumerate(sorted(table.items())):
        out[k] = insevidence.key_of(pos, text) + (v[0], v[1], v[2], v[3], v[4:])
    return out


def wanted_tables(want, min_freq, end):
    table, counts = want
    return insevidence.Tables(entries_of(table), U.triples_of(table), counts, min_freq, end)


def cli(monkeypatch, argv):
    from tests.test_gpu_del import run
    run(monkeypatch, argv)


def read_file(path):
    with (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")) as f:
        return f.read()


def check_vcf(with_keys, plain, tables, n_front=0):
    """Every record's last two keys are the tables' word; with them and their header lines stripped the file is ``plain``."""
    text = with_keys.decode()
    assert insevidence.HEADER_LINES in text
    out, n_records, n_listed = [], 0, 0
    for line in text.replace(insevidence.HEADER_LINES, "").splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            kvs = f[7].split(";")
            assert [kv.split("=")[0] for kv in kvs[-2:]] == list(insevidence.KEYS)
            assert ";".join(kvs[-2:]) == tables.info(int(f[1]) - 1, int(kvs[0].split("=")[1])), line
            n_listed += kvs[-1] != "INS=."
            f[7] = ";".join(kvs[:-2])
            line = "\t".join(f)
            n_records += 1
        out.append(line + "\n")
    assert "".join(out).encode() == plain and n_records > 12 and n_listed >= 1
    return text


def test_variants_with_the_insertion_flags(tmp_path, job, monkeypatch):
    files, want, ref, key = job
    d = tmp_path
    base = ["variants", "-i", files["bam"], "-r", files["ref"]]
    cli(monkeypatch, base + ["-o", str(d / "plain.vcf"), "--indel_vcf", str(d / "plain_i.vcf")])
    cli(monkeypatch, base + ["-o", str(d / "ins.vcf"), "--indel_vcf", str(d / "ins_i.vcf"), "--insertions", "--ins_out", str(d / "i.tsv.gz"), "--ins_end", "16"])
    tables = wanted_tables(want[False], amplipy.DEFAULTS["min_freq_variants"], 16)
    text = check_vcf(read_file(d / "ins.vcf"), read_file(d / "plain.vcf"), tables)
    a = [x for x in tables.at(key[0]) if x.text == key[1]][0]
    assert ("%s:%d:%d:%s:%d" % (key[1], N_PLANTED, N_PLANTED // 4, a.mean_qual(), a.near_end(16))) in text
    f = io.StringIO()
    insevidence.write_tsv(f, "SYN_REF", tables)
    assert read_file(d / "i.tsv.gz").decode() == f.getvalue() and f.getvalue().count("\n") == len(want[False][0]) + 1
    # the indel VCF: numeric RV on the insertion rows, and nothing else changes
    on, off = read_file(d / "ins_i.vcf").decode(), read_file(d / "plain_i.vcf").decode()
    assert "(deletions only)" in off and "(deletions only)" not in on
    rows_on, rows_off = [l for l in on.splitlines() if not l.startswith("#")], [l for l in off.splitlines() if not l.startswith("#")]
    assert len(rows_on) == len(rows_off) and [l for l in on.splitlines() if l.startswith("#")] == [l for l in off.replace(" (deletions only)", "").splitlines() if l.startswith("#")]
    n_ins = 0
    for x, y in zip(rows_on, rows_off):
        fx, fy = x.split("\t"), y.split("\t")
        if len(fx[4]) > len(fx[3]):
            n_ins += 1
            assert "RV=.;" in fy[7] and fy[7].replace("RV=.;", "RV=%d;" % tables.rev_of(int(fx[1]) - 1, fx[4])) == fx[7] and fx[:7] == fy[:7]
        else:
            assert x == y
    hit = [l.split("\t") for l in rows_on if l.split("\t")[1] == str(key[0] + 1) and l.split("\t")[4] == key[1]]
    assert n_ins >= 1 and len(hit) == 1 and (";AD=%d;RV=%d;" % (N_PLANTED, N_PLANTED // 4)) in hit[0][7]
    # --ins_out alone on consensus; a table that is too small ends the run with an error; an existing output is refused
    cli(monkeypatch, ["consensus", "-i", files["bam"], "-r", files["ref"], "-o", str(d / "c.fas"), "--ins_out", str(d / "c.tsv")])
    f = io.StringIO()
    insevidence.write_tsv(f, "SYN_REF", wanted_tables(want[False], 0, 8))
    assert read_file(d / "c.tsv").decode() == f.getvalue()
    with pytest.raises(RuntimeError) as e:
        cli(monkeypatch, base + ["-o", str(d / "y.vcf"), "--insertions", "--ins_capacity", "4"])
    assert "--ins_capacity" in str(e.value)
    with pytest.raises(SystemExit):
        cli(monkeypatch, base + ["-o", str(d / "z.vcf"), "--ins_out", str(d / "c.tsv")])


def test_two_ranks_give_the_one_process_files(tmp_path, job, monkeypatch):
    """aio with every flag of the indel unit, one process and two ranks on one card (tests/rank_worker.py takes the flags as
    they are): every output of rank 0 equals the one-process run's byte for byte, and the keys are the restatement's."""
    import re
    from tests.test_gpu_ranks import run_ranks
    files, want, ref, key = job
    argv = lambda tag: ["aio", "-i", files["bam"], "-p", files["bed"], "-r", files["ref"], "-ot", tag + ".bam", "-ov", tag + ".vcf", "-oc", tag + ".fas",
                        "-ml", "30", "--deletions", "--insertions", "--ins_out", tag + ".tsv", "--indel_vcf", tag + "_i.vcf", "--del_out", tag + "_d.tsv"]
    monkeypatch.chdir(tmp_path)
    cli(monkeypatch, argv("one"))
    status, logs = run_ranks(2, tmp_path, argv("two"), part_bytes=os.path.getsize(files["bam"]) // 4 + 1)
    assert status == [0, 0], logs
    shares = [int(x) for x in re.search(r"records \[(\d+), (\d+)\]", logs[0]).groups()]
    assert min(shares) > 0
    for ext in (".vcf", ".tsv", ".fas", "_i.vcf", "_d.tsv"):
        assert read_file(tmp_path / ("two" + ext)) == read_file(tmp_path / ("one" + ext)), ext
    tables = wanted_tables(want[True], amplipy.DEFAULTS["min_freq_variants"], 8)
    f = io.StringIO()
    insevidence.write_tsv(f, "SYN_REF", tables)
    assert read_file(tmp_path / "one.tsv").decode() == f.getvalue()
    text = read_file(tmp_path / "one.vcf").decode()
    assert "DEL_N=" in text and ";INS_N=" in text and text.index(deletion_header()) < text.index(insevidence.HEADER_LINES)


def deletion_header():
    from amplipy_amd import deletion
    return deletion.HEADER_LINES
