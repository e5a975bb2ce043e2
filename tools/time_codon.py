"""What the codon tallies cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on the
device by synth_torch) through process_device with every per-read output, all on ONE engine and ONE batch:

  * the read pass with every hook off (amp_last_kernel_ms);
  * the read pass and k_strand (amp_strand_last_ms) with the strand tallies on -- the hook of the same shape;
  * the read pass and k_codon (amp_codon_last_ms) with the codon tallies on, for a CDS set of one frame over the whole reference
    (a third of the positions start a codon) and for three overlapping frames (every position does).

20 launches per figure after 5 warm-up launches, medians; --rounds processes of their own take turns.

  python tools/time_codon.py [--rounds 3] [--out profiles/codon.json]
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


def leg():
    """One process: medians over LAUNCHES launches."""
    import numpy as np
    s = time_hooks.Setup()
    e, n, G, launches = s.eng, s.n, s.G, s.launches
    res = {"reads": n, "pass_off_ms": statistics.median(launches()[0])}
    e.strand_enable()
    ps, ks = launches(e.strand_last_ms)
    res.update(pass_strand_on_ms=statistics.median(ps), strand_ms=statistics.median(ks))
    e.strand_disable()
    counts = None
    for name, starts in (("one_frame", np.arange(0, G - 2, 3, dtype=np.int32)), ("three_frames", np.arange(0, G - 2, dtype=np.int32))):
        e.codon_enable(starts)
        ps, ks = launches(e.codon_last_ms)
        res.update({"pass_codon_on_ms_" + name: statistics.median(ps), "codon_ms_" + name: statistics.median(ks),
                    "codon_ms_min_" + name: min(ks), "codon_ms_max_" + name: max(ks)})
        codon, reads = e.codon_tables()
        counts = e.counts()
        # the last launch's table against the count table: the invariant that needs no restatement
        c = codon[:, :64].astype("uint64").reshape(-1, 4, 4, 4)
        marg = [c.sum(axis=(2, 3)), c.sum(axis=(1, 3)), c.sum(axis=(1, 2))]
        res["invariant_holds_" + name] = bool(all((marg[k] <= counts[starts.astype("int64") + k, :4]).all() for k in range(3)))
        res["triplets_" + name] = int(codon[:, :64].sum(dtype="uint64")); res["broken_" + name] = int(codon[:, 64].sum(dtype="uint64"))
        res["reads_tallied"], res["reads_skipped"] = int(reads[0]), int(reads[1])
        e.codon_disable()
    e.close()
    print("LEG " + json.dumps(res))


def child():
    return time_hooks.child(__file__, ["--leg"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codon.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": LAUNCHES, "rounds": []}
    for k in range(a.rounds):                 # a process each
        r = child()
        assert r["invariant_holds_one_frame"] and r["invariant_holds_three_frames"]
        res["rounds"].append(r)
    med = lambda key: statistics.median(r[key] for r in res["rounds"])
    res["reads"] = res["rounds"][0]["reads"]
    for key in ("pass_off_ms", "strand_ms", "codon_ms_one_frame", "codon_ms_three_frames", "pass_codon_on_ms_one_frame"):
        res[key + "_median"] = med(key)
    res["codon_over_strand_one_frame"] = med("codon_ms_one_frame") / med("strand_ms")
    res["codon_over_strand_three_frames"] = med("codon_ms_three_frames") / med("strand_ms")
    res["codon_over_pass_one_frame"] = med("codon_ms_one_frame") / med("pass_off_ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
