"""What the read-position tallies cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases,
built on the device by synth_torch) through process_device with every per-read output:

  * the read pass with every hook OFF (amp_last_kernel_ms, 20 launches after 5 warm-ups) -- and, with --parent-lib, the same with
    another build of the library (the commit before the tallies existed) in processes of their own, the two builds taking turns,
    so that what is held to the box's run-to-run spread is measured in one job on one box;
  * the read pass with k_strand alone (amp_strand_last_ms), then with k_readpos alone (amp_readpos_last_ms), 20 launches each,
    in the same process on the same engine and batch: k_strand is the yardstick.

  python tools/time_readpos.py [--parent-lib PATH/libamplihip.so] [--out profiles/readpos.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_hooks
from tools.time_hooks import LAUNCHES, WARMUP


def leg(with_tallies):
    """One process, one build of the library: medians over LAUNCHES launches."""
    from amplipy_amd import lib
    if not with_tallies:           # (a build from before the tallies has none of their entry points)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_readpos_")]
    s = time_hooks.Setup()
    e, n = s.eng, s.n
    res = {"reads": n, "pass_off_ms": statistics.median(s.launches()[0])}
    if with_tallies:
        e.strand_enable()
        ps, ks = s.launches(e.strand_last_ms)
        res.update(pass_strand_ms=statistics.median(ps), strand_ms=statistics.median(ks))
        e.strand_disable()
        e.readpos_enable()
        ps, ks = s.launches(e.readpos_last_ms)
        res.update(pass_on_ms=statistics.median(ps), readpos_ms=statistics.median(ks), readpos_ms_min=min(ks), readpos_ms_max=max(ks))
        hist = e.readpos_tables()
        counts = e.counts()
        # the last launch's table against the count table: the invariant that needs no restatement
        res["counted_last_launch"] = int(counts.sum(dtype="uint64"))
        res["bin_sums_are_the_count_table"] = bool((hist.sum(axis=2, dtype="uint64") == counts).all())
        res["bins_last_launch"] = [int(x) for x in hist.sum(axis=(0, 1), dtype="uint64")]
    e.close()
    print("LEG " + json.dumps(res))


def child(lib_path, with_tallies):
    return time_hooks.child(__file__, ["--leg", "tallies" if with_tallies else "pass"], lib_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["pass", "tallies"])
    ap.add_argument("--parent-lib", help="libamplihip.so of the commit before the tallies: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readpos.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "tallies")
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "warmup_launches": WARMUP, "parent_pass_ms": [], "this_pass_off_ms": [],
           "this_pass_on_ms": [], "strand_ms": [], "readpos_ms": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["parent_pass_ms"].append(child(a.parent_lib, False)["pass_off_ms"])
        r = child(None, True)
        res["reads"] = r["reads"]
        for key, src in (("this_pass_off_ms", "pass_off_ms"), ("this_pass_on_ms", "pass_on_ms"), ("strand_ms", "strand_ms"), ("readpos_ms", "readpos_ms")):
            res[key].append(r[src])
        res["counted"] = r["counted_last_launch"]; res["bins"] = r["bins_last_launch"]
        assert r["bin_sums_are_the_count_table"]
    med = statistics.median
    if a.parent_lib:
        res["parent_pass_median_ms"] = med(res["parent_pass_ms"])
        res["tallies_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
    res["this_pass_off_median_ms"] = med(res["this_pass_off_ms"])
    res["strand_median_ms"] = med(res["strand_ms"])
    res["readpos_median_ms"] = med(res["readpos_ms"])
    res["readpos_over_strand"] = med(res["readpos_ms"]) / med(res["strand_ms"])
    res["readpos_over_pass"] = med(res["readpos_ms"]) / med(res["this_pass_on_ms"])
    res["pass_on_vs_off"] = med(res["this_pass_on_ms"]) / med(res["this_pass_off_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
