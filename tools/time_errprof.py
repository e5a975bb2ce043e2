"""What the error profile costs, on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built
on the device by synth_torch) through process_device with every per-read output, all on ONE engine and ONE batch.  A round is
a process of its own in which, in turn:

  * the read pass with every hook off (amp_last_kernel_ms);
  * the read pass and k_strand (amp_strand_last_ms) with the strand tallies on -- the kernel that reads the same bytes through
    a window;
  * the read pass and k_errprof (amp_errprof_last_ms) with the error profile on, the reference being the synthetic genome, with
    the generator's qualities;
  * k_strand and k_errprof once more with every quality of the batch set to one value (the combine loop's shortest case).

20 launches per figure after 5 warm-up launches; every sample is kept next to its median.  The last launch's tables are checked
with the invariants that need no restatement: per mate the three tables hold the same number of bases, and when no live read
was skipped the substitution table at or above min_quality, summed by reference letter, is the count table summed likewise.

  python tools/time_errprof.py [--rounds 3] [--out profiles/errprof.json]
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


def invariants(tabs, counts, ref_seq):
    import numpy as np
    cyc, qualt, sub, reads = tabs
    same = all(int(cyc[m].sum()) == int(qualt[m].sum()) == int(sub[m].sum()) for m in range(2))
    if int(reads[1]) != 0:
        return same, None
    letters = np.frombuffer(ref_seq.upper().encode("ascii"), np.uint8)
    by_letter = np.stack([counts[letters == ord(X)][:, :4].astype(np.int64).sum(axis=0) for X in "ACGT"])
    return same, bool(np.array_equal(sub[:, :, 1].astype(np.int64).sum(axis=(0, 1)), by_letter))


def leg():
    """One process: all samples and their medians."""
    from amplipy_amd import synth
    s = time_hooks.Setup()
    e, launches = s.eng, s.launches
    ref_seq = synth.genome_string(synth.make_genome())
    med = statistics.median
    off = launches()[0]
    res = {"reads": s.n, "pass_off_ms": med(off), "pass_off_samples": off}
    for name in ("generated_qualities", "one_quality"):
        if name == "one_quality":
            s.batch.qual.fill_(37)
        e.strand_enable()
        ps, ks = launches(e.strand_last_ms)
        res.update({"strand_ms_" + name: med(ks), "strand_samples_" + name: ks})
        e.strand_disable()
        e.errprof_enable(ref_seq)
        ps, ks = launches(e.errprof_last_ms)
        tabs = e.errprof_tables()
        same, identity = invariants(tabs, e.counts(), ref_seq)
        res.update({"pass_errprof_on_ms_" + name: med(ps), "pass_errprof_on_samples_" + name: ps, "errprof_ms_" + name: med(ks), "errprof_samples_" + name: ks,
                    "bases_" + name: int(tabs[0].sum()), "mismatches_" + name: int(tabs[0][:, :, 1].sum()),
                    "quality_bins_" + name: int((tabs[1].sum(axis=(0, 2)) > 0).sum()),
                    "tables_agree_" + name: same, "count_table_identity_" + name: identity})
        res["reads_profiled"], res["reads_skipped"] = int(tabs[3][0]), int(tabs[3][1])
        e.errprof_disable()
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errprof.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "rounds": []}
    for k in range(a.rounds):                 # a process each
        r = time_hooks.child(__file__, ["--leg"])
        assert r["tables_agree_generated_qualities"] and r["tables_agree_one_quality"]
        assert r["count_table_identity_generated_qualities"] is not False and r["count_table_identity_one_quality"] is not False
        res["rounds"].append(r)
    med = lambda key: statistics.median(r[key] for r in res["rounds"])
    res["reads"] = res["rounds"][0]["reads"]
    for key in ("pass_off_ms", "strand_ms_generated_qualities", "errprof_ms_generated_qualities", "strand_ms_one_quality", "errprof_ms_one_quality",
                "pass_errprof_on_ms_generated_qualities"):
        res[key + "_median"] = med(key)
    for name in ("generated_qualities", "one_quality"):
        res["errprof_over_strand_" + name] = med("errprof_ms_" + name) / med("strand_ms_" + name)
        res["errprof_over_pass_" + name] = med("errprof_ms_" + name) / med("pass_off_ms")
        res["errprof_below_strand_" + name] = med("errprof_ms_" + name) < med("strand_ms_" + name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
