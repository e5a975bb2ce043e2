"""What the insertion evidence costs.  A leg is one process with one build of the library and one engine:

  * the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on the device by synth_torch) through process_device with
    every per-read output -- the SPARSE load: the insertion events that batch happens to hold.  The read pass with every hook
    off (amp_last_kernel_ms), then k_del alone (amp_del_last_ms), then k_insev alone (amp_insev_last_ms), then both hooks of
    the indel unit (HOOK_DEL and HOOK_INSEV, amp_hook.hpp) together;
  * the HOT-SPOT load: as many reads as the batch has, all on one amplicon, every one with the same four-base insertion, through
    process (the host form): every slot of the list holds one and the same key.  k_insev, k_del and the read pass itself
    (which piles the same reads onto one stretch of the count table) in the same launches.

20 launches per figure after 5 warm-up launches (8 after 2 on the hot spot, whose batch is staged anew every time), medians.  With --parent-lib both builds are
timed, taking turns, a fresh process each (tools/time_hooks.py's child): the read pass with every switch off and -- when the
parent has the unit -- the same figures as this build.  `hook_off_ratio` is this build's median over the parent's, next to the
parent's own run-to-run spread (max / min over its rounds) from the same session; `vs_parent` holds the same for k_insev
(sparse and hot spot) and k_del: both medians, the ratio, the parent's spread, and whether this build's median lies inside the
parent's range.

  python tools/time_insev.py [--parent-lib PATH/libamplihip.so] [--rounds 5] [--out profiles/insev.json]
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

HOT_ALLELE, HOT_ARM = "GATT", 70
HOT_WARMUP, HOT_LAUNCHES = 2, 8            # (a host batch is staged anew at every launch: fewer of them)


def hot_batch(n, pos):
    """n identical reads of 2 * HOT_ARM + 4 bases with one insertion, quality 37."""
    import numpy as np
    from amplipy_amd.batch import ReadBatch
    rng = np.random.default_rng(7)
    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    arm = lambda: [int(c) for c in np.array([1, 2, 4, 8])[rng.integers(0, 4, HOT_ARM)]]
    codes = np.array(arm() + [code[c] for c in HOT_ALLELE] + arm(), np.uint8)
    cig = np.tile(np.array([(HOT_ARM << 4) | 0, (len(HOT_ALLELE) << 4) | 1, (HOT_ARM << 4) | 0], np.uint32), n)
    return ReadBatch.from_uniform(np.full(n, pos, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.int32), codes.size, np.arange(0, 3 * n + 1, 3, dtype=np.uint64),
                                  cig, np.broadcast_to(codes, (n, codes.size)), np.full((n, codes.size), 37, np.uint8))


def leg(this):
    from amplipy_amd import lib
    with open(lib.LIB_PATH, "rb") as f:        # (looked for in the file: loading the library here would bring HIP up in front of torch)
        with_insev = this or b"amp_insev_enable" in f.read()
    if not with_insev:             # (a build from before the unit has none of its entry points, nor the getter that came with it)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_insev_") and n != "amp_debug_event_capacity"]
    s = time_hooks.Setup()
    e, med = s.eng, statistics.median
    res = {"reads": s.n, "pass_off_ms": med(s.launches()[0])}
    if with_insev:
        e.del_enable()
        res["sparse_del_ms"] = med(s.launches(e.del_last_ms)[1])
        e.del_disable()
        e.insev_enable()
        res["sparse_insev_ms"] = med(s.launches(e.insev_last_ms)[1])
        entries, info = e.insev_entries()
        res.update(sparse_events=int(entries["count"].sum()), sparse_alleles=info["used"], sparse_lost=info["lost"])
        e.del_enable()
        both = [s.launches(lambda: (e.del_last_ms(), e.insev_last_ms()))[1]][0]
        res["sparse_both_del_ms"], res["sparse_both_insev_ms"] = med([b[0] for b in both]), med([b[1] for b in both])
        # the hot spot, through the host form (the staging is not part of either kernel's time)
        hb = hot_batch(s.n, int(s.amps[40][0]) + 40)
        d_ms, i_ms, p_ms = [], [], []
        for it in range(HOT_WARMUP + HOT_LAUNCHES):
            e.reset(); e.process(hb, want_trim=False)
            if it >= HOT_WARMUP:
                d_ms.append(e.del_last_ms()); i_ms.append(e.insev_last_ms()); p_ms.append(e.last_kernel_ms()[0])
        entries, info = e.insev_entries()
        res.update(hot_del_ms=med(d_ms), hot_insev_ms=med(i_ms), hot_pass_ms=med(p_ms), hot_events=int(entries["count"].sum()), hot_alleles=info["used"], hot_lost=info["lost"])
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("this", "parent"))
    ap.add_argument("--parent-lib", help="libamplihip.so of the parent commit: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insev.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "this")
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "warmup_launches": WARMUP, "rounds": {"parent": [], "this": []}}
    for _ in range(a.rounds):                  # the builds take turns, a process each
        if a.parent_lib:
            res["rounds"]["parent"].append(time_hooks.child(__file__, ["--leg", "parent"], a.parent_lib, timeout=400))
        res["rounds"]["this"].append(time_hooks.child(__file__, ["--leg", "this"], timeout=400))
    med = statistics.median
    for key in sorted(res["rounds"]["this"][0]):
        res[key] = med([r[key] for r in res["rounds"]["this"]])
    if a.parent_lib:
        p = [r["pass_off_ms"] for r in res["rounds"]["parent"]]
        res["parent_pass_off_ms"] = {"median": med(p), "min": min(p), "max": max(p)}
        res["hook_off_ratio"] = res["pass_off_ms"] / med(p)
        res["parent_spread_ratio"] = max(p) / min(p)
        res["hook_off_within_parent_spread"] = min(p) / med(p) <= res["hook_off_ratio"] <= max(p) / med(p)
        res["vs_parent"] = {}
        for key in ("sparse_insev_ms", "hot_insev_ms", "sparse_del_ms"):
            p = [r[key] for r in res["rounds"]["parent"] if key in r]
            if p:
                res["vs_parent"][key] = {"this": res[key], "parent": med(p), "parent_min": min(p), "parent_max": max(p), "ratio": res[key] / med(p),
                                         "parent_spread_ratio": max(p) / min(p), "within_parent_range": min(p) <= res[key] <= max(p)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
