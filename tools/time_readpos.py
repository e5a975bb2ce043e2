"""What the read-position tallies cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases,
built on the device by synth_torch) through process_device with every per-read output.  A leg is one process with one build of
the library, one engine and one batch:

  * the read pass with every hook OFF (amp_last_kernel_ms, 20 launches after 5 warm-ups);
  * the read pass with k_strand alone (amp_strand_last_ms), then with k_readpos alone (amp_readpos_last_ms), 20 launches each:
    k_strand is the yardstick;
  * a hash of the three tables of the last launch.

With --parent-lib the same leg runs with another build of the library (the parent commit) in processes of their own, the two
builds taking turns, so that what is held to the box's run-to-run spread is measured in one job on one box: the tables must be
the same bytes, and a kernel of this build is `within` when its median over the rounds is at most the parent's median times
1 + the parent's own spread, (max - min) / median over its rounds.

  python tools/time_readpos.py [--parent-lib PATH/libamplihip.so] [--rounds 5] [--out profiles/readpos.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_hooks
from tools.time_hooks import LAUNCHES, WARMUP


def leg():
    """One process, one build of the library: medians over LAUNCHES launches, and a hash of the last launch's tables."""
    s = time_hooks.Setup()
    e, n = s.eng, s.n
    res = {"reads": n, "pass_off_ms": statistics.median(s.launches()[0])}
    sha = hashlib.sha256()
    e.strand_enable()
    ps, ks = s.launches(e.strand_last_ms)
    res.update(pass_strand_ms=statistics.median(ps), strand_ms=statistics.median(ks))
    for t in e.strand_tables():
        sha.update(t.tobytes())
    e.strand_disable()
    e.readpos_enable()
    ps, ks = s.launches(e.readpos_last_ms)
    res.update(pass_on_ms=statistics.median(ps), readpos_ms=statistics.median(ks), readpos_ms_min=min(ks), readpos_ms_max=max(ks))
    hist = e.readpos_tables()
    sha.update(hist.tobytes())
    res["tables_sha256"] = sha.hexdigest()     # integer sums: the same bytes whatever the order of the atomics
    counts = e.counts()
    # the last launch's table against the count table: the invariant that needs no restatement
    res["counted_last_launch"] = int(counts.sum(dtype="uint64"))
    res["bin_sums_are_the_count_table"] = bool((hist.sum(axis=2, dtype="uint64") == counts).all())
    res["bins_last_launch"] = [int(x) for x in hist.sum(axis=(0, 1), dtype="uint64")]
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib", help="libamplihip.so of the parent commit: its read pass and its two kernels are timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readpos.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "warmup_launches": WARMUP, "parent_pass_ms": [], "parent_strand_ms": [],
           "parent_readpos_ms": [], "this_pass_off_ms": [], "this_pass_on_ms": [], "strand_ms": [], "readpos_ms": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            r = time_hooks.child(__file__, ["--leg"], a.parent_lib)
            for key, src in (("parent_pass_ms", "pass_off_ms"), ("parent_strand_ms", "strand_ms"), ("parent_readpos_ms", "readpos_ms")):
                res[key].append(r[src])
            parent_sha = r["tables_sha256"]
        r = time_hooks.child(__file__, ["--leg"])
        res["reads"] = r["reads"]
        for key, src in (("this_pass_off_ms", "pass_off_ms"), ("this_pass_on_ms", "pass_on_ms"), ("strand_ms", "strand_ms"), ("readpos_ms", "readpos_ms")):
            res[key].append(r[src])
        res["counted"] = r["counted_last_launch"]; res["bins"] = r["bins_last_launch"]; res["tables_sha256"] = r["tables_sha256"]
        assert r["bin_sums_are_the_count_table"]
        assert not a.parent_lib or parent_sha == r["tables_sha256"], "the two builds' tables differ"
    med = statistics.median
    if a.parent_lib:
        res["parent_pass_median_ms"] = med(res["parent_pass_ms"])
        res["tallies_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
        res["tables_identical_to_parent"] = True
        # a kernel of this build is `within` when its median is at most the parent's times 1 + the parent's own spread over its rounds
        for name in ("strand", "readpos"):
            v = res["parent_%s_ms" % name]
            spread = (max(v) - min(v)) / med(v)
            res["parent_%s_median_ms" % name] = med(v)
            res["parent_%s_spread" % name] = spread
            res["%s_within" % name] = med(res["%s_ms" % name]) <= med(v) * (1 + spread)
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
