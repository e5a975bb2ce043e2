"""What the read haplotypes cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on
the device by synth_torch) through process_device with every per-read output, all on ONE engine and ONE batch.  A round is a
process of its own in which, in turn:

  * the read pass with every hook off (amp_last_kernel_ms);
  * the read pass and k_cooc (amp_cooc_last_ms) with the co-occurrence tallies on, one two-site set per synthetic amplicon, as
    tools/time_cooc.py times it;
  * the read pass and k_errprof (amp_errprof_last_ms) with the error profile on, no mask, as tools/time_errprof.py times it;
  * the read pass and k_hap (amp_hap_last_ms) with the haplotypes on, one region of 100 positions per synthetic amplicon;
  * k_hap once more with regions of 100 positions tiling the whole reference.

20 launches per figure after 5 warm-up launches; every sample is kept next to its median.  The last launch's tables are checked
against the invariant that needs no restatement: per region COVER is REF + LOWQ + OVERFLOW + EDGE + the counts of the region's
entries, no read lost.

  python tools/time_hap.py [--rounds 3] [--out profiles/hap.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_hooks
from tools.time_cooc import two_site_sets
from tools.time_hooks import LAUNCHES

REGION = 100


def invariant(entries, info, tally):
    import numpy as np
    t = tally.astype(np.int64)
    held = np.zeros(len(t), np.int64)
    np.add.at(held, (entries["head"] & 0xFFFF).astype(np.int64), entries["count"].astype(np.int64))
    return bool(info["lost"] == 0 and (t[:, 0] == t[:, 1] + t[:, 3] + t[:, 4] + t[:, 5] + held).all() and (t[:, 2] <= t[:, 1]).all())


def leg():
    """One process: all samples and their medians."""
    import numpy as np
    from amplipy_amd import errprof, synth
    s = time_hooks.Setup()
    e, G, launches = s.eng, s.G, s.launches
    ref_seq = synth.genome_string(synth.make_genome())
    med = statistics.median
    off = launches()[0]
    res = {"reads": s.n, "pass_off_ms": med(off), "pass_off_samples": off}
    off_, pos, ln, sym = two_site_sets([int(a[2]) + 60 for a in s.amps], G)
    e.cooc_enable(off_, pos, ln, sym)
    ps, ks = launches(e.cooc_last_ms)
    res.update(cooc_sets=int(off_.size - 1), cooc_ms=med(ks), cooc_samples=ks)
    e.cooc_disable()
    errprof.enable(e, ref_seq, None)
    ps, ks = launches(e.errprof_last_ms)
    res.update(errprof_ms=med(ks), errprof_samples=ks)
    e.errprof_disable()
    lists = (("per_amplicon", sorted(int(a[2]) + 20 for a in s.amps if int(a[2]) + 20 + REGION <= G)), ("tiling", range(0, G - REGION + 1, REGION)))
    for name, starts in lists:
        st = np.array(list(starts), np.int32)
        e.hap_enable(st, st + REGION, ref_seq)
        ps, ks = launches(e.hap_last_ms)
        entries, info, tally, reads = e.hap_tables()
        res.update({"regions_" + name: int(st.size), "pass_hap_on_ms_" + name: med(ps), "pass_hap_on_samples_" + name: ps, "hap_ms_" + name: med(ks),
                    "hap_samples_" + name: ks, "haplotypes_" + name: int(info["used"]), "lost_" + name: int(info["lost"]),
                    "tally_" + name: [int(x) for x in tally.sum(axis=0)], "reads_covering_" + name: int(reads[0]), "reads_other_" + name: int(reads[1]),
                    "invariant_holds_" + name: invariant(entries, info, tally)})
        e.hap_disable()
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "region_positions": REGION, "rounds": []}
    for k in range(a.rounds):                 # a process each
        r = time_hooks.child(__file__, ["--leg"])
        assert r["invariant_holds_per_amplicon"] and r["invariant_holds_tiling"]
        res["rounds"].append(r)
    med = lambda key: statistics.median(r[key] for r in res["rounds"])
    res["reads"] = res["rounds"][0]["reads"]
    for key in ("pass_off_ms", "cooc_ms", "errprof_ms", "hap_ms_per_amplicon", "hap_ms_tiling", "pass_hap_on_ms_per_amplicon"):
        res[key + "_median"] = med(key)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
