"""What the co-occurrence tallies cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases,
built on the device by synth_torch) through process_device with every per-read output, all on ONE engine and ONE batch.  A
round is a process of its own in which, in turn:

  * the read pass with every hook off (amp_last_kernel_ms);
  * the read pass and k_codon (amp_codon_last_ms) with the codon tallies on, one frame over the whole reference;
  * the read pass and k_cooc (amp_cooc_last_ms) with the co-occurrence tallies on, one two-site set per synthetic amplicon
    (two substitution sites 40 bases apart inside the amplicon, between its primers);
  * k_cooc once more on a long list: a two-site set every 15 positions of the reference, more than ten windows' worth.

20 launches per figure after 5 warm-up launches; every sample is kept next to its median.  The last launch's table is checked
against the count table with the invariant that needs no restatement: per site, the reads of the complete patterns that
carry the site's base are at most the count table's count of that base there.

  python tools/time_cooc.py [--rounds 3] [--out profiles/cooc.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_hooks
from tools.time_hooks import LAUNCHES


def two_site_sets(firsts, G, gap=40):
    """One set {(p, A), (p + gap, C)} per first position -> the arrays of cooc_enable."""
    import numpy as np
    firsts = np.array(sorted(int(p) for p in firsts if 0 <= p and p + gap < G), np.int32)
    n = firsts.size
    pos = np.stack([firsts, firsts + gap], axis=1).reshape(-1)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int32), pos.astype(np.int32), np.zeros(2 * n, np.int32), np.tile(np.array([0, 1], np.uint8), n)


def invariant(cooc, pos, sym, counts):
    """Two-site sets: the complete reads with site j's base (patterns with bit j) are at most counts[p_j][b_j]."""
    import numpy as np
    c = cooc.astype(np.int64)
    with0, with1 = c[:, 1] + c[:, 3], c[:, 2] + c[:, 3]
    p, b = pos.reshape(-1, 2).astype(np.int64), sym.reshape(-1, 2).astype(np.int64)
    return bool((with0 <= counts[p[:, 0], b[:, 0]]).all() and (with1 <= counts[p[:, 1], b[:, 1]]).all() and not c[:, 4:64].any())


def leg():
    """One process: all samples and their medians."""
    import numpy as np
    s = time_hooks.Setup()
    e, G, launches = s.eng, s.G, s.launches
    med = statistics.median
    off = launches()[0]
    res = {"reads": s.n, "pass_off_ms": med(off), "pass_off_samples": off}
    e.codon_enable(np.arange(0, G - 2, 3, dtype=np.int32))
    ps, ks = launches(e.codon_last_ms)
    res.update(pass_codon_on_ms=med(ps), codon_ms=med(ks), codon_samples=ks)
    e.codon_disable()
    lists = (("per_amplicon", [int(a[2]) + 60 for a in s.amps]), ("every_15", range(1, G - 41, 15)))
    for name, firsts in lists:
        off_, pos, ln, sym = two_site_sets(firsts, G)
        e.cooc_enable(off_, pos, ln, sym)
        ps, ks = launches(e.cooc_last_ms)
        cooc, reads = e.cooc_tables()
        res.update({"sets_" + name: int(off_.size - 1), "pass_cooc_on_ms_" + name: med(ps), "pass_cooc_on_samples_" + name: ps,
                    "cooc_ms_" + name: med(ks), "cooc_samples_" + name: ks,
                    "complete_" + name: int(cooc[:, :64].sum(dtype="uint64")), "partial_" + name: int(cooc[:, 64].sum(dtype="uint64")),
                    "invariant_holds_" + name: invariant(cooc, pos, sym, e.counts())})
        res["reads_tallied"], res["reads_skipped"] = int(reads[0]), int(reads[1])
        e.cooc_disable()
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cooc.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "rounds": []}
    for k in range(a.rounds):                 # a process each
        r = time_hooks.child(__file__, ["--leg"])
        assert r["invariant_holds_per_amplicon"] and r["invariant_holds_every_15"]
        res["rounds"].append(r)
    med = lambda key: statistics.median(r[key] for r in res["rounds"])
    res["reads"] = res["rounds"][0]["reads"]
    for key in ("pass_off_ms", "codon_ms", "cooc_ms_per_amplicon", "cooc_ms_every_15", "pass_cooc_on_ms_per_amplicon"):
        res[key + "_median"] = med(key)
    res["cooc_over_codon_per_amplicon"] = med("cooc_ms_per_amplicon") / med("codon_ms")
    res["cooc_over_pass_per_amplicon"] = med("cooc_ms_per_amplicon") / med("pass_off_ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
