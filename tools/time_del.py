"""What the deletion events cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on
the device by synth_torch; one read in twenty carries a deletion of 1 to 3 bases at a random offset) through process_device
with every per-read output.  ONE process, one engine, one batch; the figures take turns, round after round:

  * the read pass with every hook off (amp_last_kernel_ms);
  * k_strand alone (amp_strand_last_ms): the kernel k_del is held against -- it reads every base and quality of the batch,
    k_del the CIGAR words;
  * k_del alone (amp_del_last_ms).

20 launches per figure and round after 5 warm-up launches; the median of a round, then the median over the rounds (at least
five).  Also: the distinct events the batch produces (what the default capacity of the device table, 2^20 slots, is to be
judged by), `lost`, and the invariant on the last launch's table -- per position, the events that cover it add up to the '-'
column of the count table.

  python tools/time_del.py [--rounds 5] [--out profiles/del.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log2-capacity", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "del.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five rounds")
    import numpy as np
    s = time_hooks.Setup()
    e, med = s.eng, statistics.median
    res = {"batch": time_hooks.BATCH, "reads": s.n, "launches_per_figure_and_round": LAUNCHES, "warmup_launches": WARMUP, "rounds": a.rounds,
           "pass_off_ms": [], "strand_ms": [], "del_ms": []}
    for _ in range(a.rounds):
        res["pass_off_ms"].append(med(s.launches()[0]))
        e.strand_enable()
        res["strand_ms"].append(med(s.launches(e.strand_last_ms)[1]))
        e.strand_disable()
        e.del_enable(a.log2_capacity)
        res["del_ms"].append(med(s.launches(e.del_last_ms)[1]))
        e.del_disable()
    events, info = e.del_events()          # the last launch's table (every launch starts from amp_reset)
    counts = e.counts()
    dash = np.zeros(s.G + 1, np.int64)
    np.add.at(dash, events["start"], events["count"].astype(np.int64))
    np.add.at(dash, events["start"] + events["len"], -events["count"].astype(np.int64))
    res.update(pass_off_median_ms=med(res["pass_off_ms"]), strand_median_ms=med(res["strand_ms"]), del_median_ms=med(res["del_ms"]),
               distinct_events=info["used"], capacity=info["capacity"], lost=info["lost"],
               reads_with_an_event=int(events["count"].sum(dtype=np.uint64)), longest_event=int(events["len"].max()) if events.size else 0,
               most_reads_on_one_event=int(events["count"].max()) if events.size else 0,
               invariant_holds=bool(np.array_equal(np.cumsum(dash)[:s.G], counts[:, 5].astype(np.int64))))
    res["del_over_strand"] = res["del_median_ms"] / res["strand_median_ms"]
    res["del_not_above_strand"] = res["del_median_ms"] <= res["strand_median_ms"]
    res["table_load"] = info["used"] / info["capacity"]
    e.close()
    assert res["lost"] == 0 and res["invariant_holds"], res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
