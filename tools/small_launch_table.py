"""Reduces a rocprofv3 --kernel-trace of one plain `bench.py` run to the table kept as profiles/small_launches_*.json:
   python3 tools/small_launch_table.py <kernel_trace.csv> <out.json> [steps]

For a dozen consecutive steps from the middle of the timed region (the last `steps` full-grid k_fast launches of the run, 200
by default): every kernel of the step with its place in the enqueue order (Dispatch_Id: the kernel trace carries no enqueue
stamp), queue, grid, start and end in microseconds from the start of the window; when the next k_fast on the same queue started;
and for the window the time during which 0, 1, 2 and more k_fast ran, with the gaps of fewer than two.  Over the whole timed
region: count, mean and maximum duration of every kernel, and the time it spent between the end of its predecessor on its
stream (the k_fast of its own step for the kernels behind the pass) and its own start."""
import collections
import csv
import json
import sys

SMALL = ("k_reset", "k_tile", "k_deferred_heavy", "k_call_compact", "k_call_fused", "k_call")


def short(name):
    n = name.split("(")[0].replace("void ", "").replace("amp::", "")
    return n.split("<")[0]


def main():
    path, out = sys.argv[1], sys.argv[2]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    rows = []
    for r in csv.DictReader(open(path)):
        k = short(r["Kernel_Name"])
        if k == "k_fast" or k in SMALL:
            rows.append({"kernel": k, "dispatch": int(r["Dispatch_Id"]), "queue": int(r.get("Queue_Id") or 0), "stream": int(r.get("Stream_Id") or 0),
                         "grid": int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["dispatch"])
    # a step: the launches of one engine from its k_reset to the last kernel before the next k_reset of the same stream
    by_stream = collections.defaultdict(list)
    for r in rows:
        by_stream[r["stream"] or r["queue"]].append(r)
    all_steps = []
    for s, rs in by_stream.items():
        cur = None
        for r in rs:
            if r["kernel"] == "k_reset":
                cur = [r]
                all_steps.append(cur)
            elif cur is not None:
                cur.append(r)
    gmax = max(r["grid"] for r in rows if r["kernel"] == "k_fast")
    all_steps = [st for st in all_steps if any(r["kernel"] == "k_fast" and r["grid"] == gmax for r in st)]
    all_steps.sort(key=lambda st: st[0]["dispatch"])
    timed = all_steps[-steps:]
    mid = len(timed) // 2
    window = timed[mid:mid + 12]
    w0 = min(r["t0"] for st in window for r in st)
    us = lambda t: round((t - w0) / 1e3, 2)
    fast_all = sorted((r for st in timed for r in st if r["kernel"] == "k_fast"), key=lambda r: r["t0"])

    table = []
    for st in window:
        fast = next(r for r in st if r["kernel"] == "k_fast")
        nxt = [r for r in fast_all if r["queue"] == fast["queue"] and r["dispatch"] > fast["dispatch"]]
        nxt.sort(key=lambda r: r["dispatch"])
        table.append({"queue": fast["queue"], "stream": fast["stream"],
                      "next_k_fast_same_queue_start_us": us(nxt[0]["t0"]) if nxt else None,
                      "kernels": [{"kernel": r["kernel"], "enqueue_order": r["dispatch"], "queue": r["queue"], "blocks": r["grid"], "start_us": us(r["t0"]),
                                   "end_us": us(r["t1"]), "dur_us": round((r["t1"] - r["t0"]) / 1e3, 2)} for r in st]})

    # k_fast concurrency over the window
    a, b = w0, max(r["t1"] for st in window for r in st if r["kernel"] == "k_fast")
    ev = []
    for r in fast_all:
        if r["t1"] > a and r["t0"] < b:
            ev += [(max(r["t0"], a), 1), (min(r["t1"], b), -1)]
    ev.sort()
    running, last, share, gaps = 0, a, collections.Counter(), []
    for t, d in ev:
        if t > last:
            share[min(running, 3)] += t - last
            if running < 2:
                if gaps and gaps[-1]["end_us"] == us(last) and gaps[-1]["k_fast_running"] == running:
                    gaps[-1]["end_us"] = us(t)
                else:
                    gaps.append({"start_us": us(last), "end_us": us(t), "k_fast_running": running})
            last = t
        running += d
    conc = {"window_us": round((b - a) / 1e3, 2), "us_with_0_k_fast": round(share[0] / 1e3, 2), "us_with_1_k_fast": round(share[1] / 1e3, 2),
            "us_with_2_k_fast": round(share[2] / 1e3, 2), "us_with_3_or_more_k_fast": round(share[3] / 1e3, 2),
            "gaps_with_fewer_than_two": [g for g in gaps if g["end_us"] - g["start_us"] >= 0.5]}

    # the whole timed region
    dur, wait = collections.defaultdict(list), collections.defaultdict(list)
    for st in timed:
        prev = None
        for r in st:
            dur[r["kernel"]].append((r["t1"] - r["t0"]) / 1e3)
            if prev is not None:
                wait[r["kernel"]].append((r["t0"] - prev["t1"]) / 1e3)
            prev = r
    stat = lambda v: {"n": len(v), "mean_us": round(sum(v) / len(v), 2), "max_us": round(max(v), 2)} if v else None
    region = {k: {"duration": stat(dur[k]), "start_after_predecessor_end": stat(wait[k])} for k in dur}
    span = (max(r["t1"] for st in timed for r in st) - min(r["t0"] for st in timed for r in st)) / 1e3
    json.dump({"note": "rocprofv3 --kernel-trace of one plain `python bench.py` (no counters, no other tracing); times in microseconds from the start "
                       "of the 12-step window taken from the middle of the timed region; enqueue_order is the trace's Dispatch_Id (the kernel "
                       "trace has no enqueue stamp); start_after_predecessor_end is the time between the end of the kernel in front on the same "
                       "stream and the kernel's own start",
               "timed_steps": len(timed), "gpu_span_of_timed_steps_us": round(span, 1), "gpu_span_per_step_us": round(span / max(1, len(timed)), 2),
               "timed_region": region, "k_fast_concurrency": conc, "steps": table}, open(out, "w"), indent=1)
    print(json.dumps({"timed_region": region, "k_fast_concurrency": {k: v for k, v in conc.items() if k != "gaps_with_fewer_than_two"},
                      "gpu_span_per_step_us": round(span / max(1, len(timed)), 2)}, indent=1))


if __name__ == "__main__":
    main()
