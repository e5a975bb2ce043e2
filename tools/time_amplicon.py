"""What the per-amplicon allele counts cost, on the benchmark's 10k x batch (1,993,533 reads of 150
bases, built on the device by synth_torch) through process_device with every per-read output:

  * the read pass with the hook OFF (amp_last_kernel_ms, 20 launches) -- and, with --parent-lib, the same with another build
    of the library (the commit before the hook existed) in processes of their own, the two builds taking turns, so that what
    is held to the box's run-to-run spread is measured in one job on one box;
  * the read pass and k_amplicon (amp_amplicon_last_ms) with the hook ON, and next to it k_strand (amp_strand_last_ms) on the
    same batch in the same process, 20 launches each.

The synthetic primer set is paired into amplicons here: SYN_<k>_LEFT with SYN_<k>_RIGHT.

  python tools/time_amplicon.py [--parent-lib PATH/libamplihip.so] [--out profiles/amplicon.json]
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


def leg(with_hook):
    """One process, one build of the library: medians over LAUNCHES launches."""
    import numpy as np
    from amplipy_amd import amplicon, lib
    if not with_hook:              # (a build from before the hook has none of its entry points)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_amplicon_")]
    s = time_hooks.Setup()
    e, n, launches = s.eng, s.n, s.launches
    res = {"reads": n, "pass_off_ms": statistics.median(launches()[0])}
    if with_hook:
        aset = s.amplicon_set()
        e.strand_enable()
        ps, ks = launches(e.strand_last_ms)
        res.update(strand_ms=statistics.median(ks))
        e.strand_disable()
        amplicon.enable(e, aset)
        ps, ks = launches(e.amplicon_last_ms)
        res.update(pass_on_ms=statistics.median(ps), amplicon_ms=statistics.median(ks), amplicon_ms_min=min(ks), amplicon_ms_max=max(ks),
                   amplicons=aset.n, span_positions=aset.cells)
        a_counts, a_reads = e.amplicon_tables()
        counts = e.counts().astype(np.uint64)
        # the last launch's tables against the count table: the invariants that need no restatement
        back = np.zeros_like(counts)
        for k in range(aset.n):
            back[int(aset.lo[k]):int(aset.hi[k])] += a_counts[aset.rows_of(k)]
        res["invariants_hold"] = bool((back <= counts).all() and int(a_reads.sum()) == n)
        res["reads_assigned_share"] = float(a_reads[:-1].sum()) / n
        res["bases_assigned_share"] = float(back.sum()) / max(float(counts.sum()), 1.0)
    e.close()
    print("LEG " + json.dumps(res))


def child(lib_path, with_hook):
    return time_hooks.child(__file__, ["--leg", "hook" if with_hook else "pass"], lib_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["pass", "hook"])
    ap.add_argument("--parent-lib", help="libamplihip.so of the commit before the hook: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amplicon.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "hook")
    res = {"batch": "10k x depth, 150-base reads (synth_torch, seed 1000)", "launches_per_figure": LAUNCHES, "parent_pass_ms": [], "this_pass_off_ms": [],
           "this_pass_on_ms": [], "amplicon_ms": [], "strand_ms": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["parent_pass_ms"].append(child(a.parent_lib, False)["pass_off_ms"])
        r = child(None, True)
        for key in ("reads", "amplicons", "span_positions", "reads_assigned_share", "bases_assigned_share"):
            res[key] = r[key]
        res["this_pass_off_ms"].append(r["pass_off_ms"]); res["this_pass_on_ms"].append(r["pass_on_ms"])
        res["amplicon_ms"].append(r["amplicon_ms"]); res["strand_ms"].append(r["strand_ms"])
        assert r["invariants_hold"]
    med = statistics.median
    if a.parent_lib:
        res["parent_pass_median_ms"] = med(res["parent_pass_ms"])
        res["hook_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
    res["this_pass_off_median_ms"] = med(res["this_pass_off_ms"])
    res["amplicon_median_ms"] = med(res["amplicon_ms"])
    res["strand_median_ms"] = med(res["strand_ms"])
    res["amplicon_over_strand"] = med(res["amplicon_ms"]) / med(res["strand_ms"])
    res["amplicon_over_pass"] = med(res["amplicon_ms"]) / med(res["this_pass_on_ms"])
    res["pass_on_vs_off"] = med(res["this_pass_on_ms"]) / med(res["this_pass_off_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
