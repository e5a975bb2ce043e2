"""What the strand and base-quality tallies cost, on the benchmark's 10k x batch (1,993,533 reads of 150
bases, built on the device by synth_torch) through process_device with every per-read output:

  * the read pass with the tallies OFF (amp_last_kernel_ms, 20 launches) -- and, with --parent-lib, the same with another build
    of the library (the commit before the tallies existed) in processes of their own, the two builds taking turns, so that what
    is held to the box's run-to-run spread is measured in one job on one box;
  * the read pass and k_strand (amp_strand_last_ms) with the tallies ON, 20 launches each, in the same process.

  python tools/time_strand.py [--parent-lib PATH/libamplihip.so] [--out profiles/strand.json]
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


def leg(with_tallies):
    """One process, one build of the library: medians over LAUNCHES launches."""
    from amplipy_amd import lib
    if not with_tallies:           # (a build from before the tallies has none of their entry points)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_strand_")]
    s = time_hooks.Setup()
    e, n = s.eng, s.n
    res = {"reads": n, "pass_off_ms": statistics.median(s.launches()[0])}
    if with_tallies:
        e.strand_enable()
        ps, ks = s.launches(e.strand_last_ms)
        res.update(pass_on_ms=statistics.median(ps), strand_ms=statistics.median(ks), strand_ms_min=min(ks), strand_ms_max=max(ks))
        rev, qsum = e.strand_tables()
        counts = e.counts()
        # the last launch's tables against the count table: the invariants that need no restatement
        res["counted_bases_last_launch"] = int(counts[:, :5].sum(dtype="uint64"))
        res["invariants_hold"] = bool((rev <= counts).all() and (qsum >= 20 * counts[:, :5].astype("uint64")).all() and
                                      (qsum <= 255 * counts[:, :5].astype("uint64")).all() and ((qsum > 0) == (counts[:, :5] > 0)).all())
        res["reverse_share"] = float(rev.sum(dtype="uint64")) / max(float(counts.sum(dtype="uint64")), 1.0)
    e.close()
    print("LEG " + json.dumps(res))


def child(lib_path, with_tallies):
    return time_hooks.child(__file__, ["--leg", "tallies" if with_tallies else "pass"], lib_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["pass", "tallies"])
    ap.add_argument("--parent-lib", help="libamplihip.so of the commit before the tallies: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strand.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "tallies")
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "parent_pass_ms": [], "this_pass_off_ms": [],
           "this_pass_on_ms": [], "strand_ms": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["parent_pass_ms"].append(child(a.parent_lib, False)["pass_off_ms"])
        r = child(None, True)
        res["reads"] = r["reads"]
        res["this_pass_off_ms"].append(r["pass_off_ms"]); res["this_pass_on_ms"].append(r["pass_on_ms"]); res["strand_ms"].append(r["strand_ms"])
        res["counted_bases"] = r["counted_bases_last_launch"]; res["reverse_share"] = r["reverse_share"]
        assert r["invariants_hold"]
    med = statistics.median
    if a.parent_lib:
        res["parent_pass_median_ms"] = med(res["parent_pass_ms"])
        res["tallies_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
    res["this_pass_off_median_ms"] = med(res["this_pass_off_ms"])
    res["strand_median_ms"] = med(res["strand_ms"])
    res["strand_over_pass"] = med(res["strand_ms"]) / med(res["this_pass_on_ms"])
    res["pass_on_vs_off"] = med(res["this_pass_on_ms"]) / med(res["this_pass_off_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
