"""What the amplicon QC report costs, on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on
the device by synth_torch) through process_device with every per-read output:

  * the read pass with the report OFF (amp_last_kernel_ms, 20 launches) -- and, with --parent-lib, the same with another build of
    the library (the commit before the report existed) in processes of their own, the two builds taking turns, so that what is
    held to the box's run-to-run spread is measured in one job on one box;
  * the read pass and k_qc_reads (amp_qc_last_ms) with the report ON, 20 launches each.

  python tools/time_qc.py [--parent-lib PATH/libamplihip.so] [--out profiles/qc.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAUNCHES, WARMUP = 20, 5


def leg(with_report):
    """One process, one build of the library: medians over LAUNCHES launches."""
    import torch
    from amplipy_amd import abi, lib, synth, synth_torch
    if not with_report:            # (a build from before the report has none of its entry points)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_qc_")]
    g = synth.make_genome(); primers, amps = synth.make_artic_scheme(); G = int(g.size)
    pr = sorted((s, e) for s, e, _ in primers)
    n = synth.reads_for_depth(10000)
    mn, mx, mpl = lib.find_overlapping_primers(G, pr, 0)
    b = synth_torch.make_amplicon_batch_device(g, amps, n, 1000, "cuda:0"); torch.cuda.synchronize()
    rd = b.struct()
    out = {k: torch.zeros(sz, dtype=dt, device="cuda:0") for k, sz, dt in
           (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", b.n_cig + 3 * n, torch.int32),
            ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
    dev_out = abi.AmpTrimOut(*[out[k].data_ptr() for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")])
    e = lib.Engine(G); e.set_primers(mn, mx, mpl); e.set_params(20, 4, True, True); e.reserve_events(1 << 22)

    def launches(qc_on):
        ps, qs = [], []
        for it in range(WARMUP + LAUNCHES):
            e.reset(); e.process_device(rd, 0, dev_out); e.sync()
            if it >= WARMUP:
                ps.append(e.last_kernel_ms()[0])
                if qc_on:
                    qs.append(e.qc_last_ms())
        return ps, qs
    res = {"reads": n, "pass_off_ms": statistics.median(launches(False)[0])}
    if with_report:
        e.qc_enable(pr, 0, 30, False, [(0, G)], [1, 10, 100])
        ps, qs = launches(True)
        res.update(pass_on_ms=statistics.median(ps), qc_reads_ms=statistics.median(qs), qc_reads_ms_min=min(qs), qc_reads_ms_max=max(qs))
        t = e.qc_read_tallies()[0]
        res["rows_tallied_last_launch"] = t["rows"]
    e.close()
    print("LEG " + json.dumps(res))


def child(lib_path, with_report):
    env = dict(os.environ)
    if lib_path:
        env.update(AMPLIPY_DEV="1", AMPLIHIP_LIB=lib_path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "report" if with_report else "pass"], env=env, capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("leg failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["pass", "report"])
    ap.add_argument("--parent-lib", help="libamplihip.so of the commit before the report: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "report")
    res = {"batch": "10k x depth, 150-base reads (synth_torch, seed 1000)", "launches_per_figure": LAUNCHES, "parent_pass_ms": [], "this_pass_off_ms": [],
           "this_pass_on_ms": [], "qc_reads_ms": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["parent_pass_ms"].append(child(a.parent_lib, False)["pass_off_ms"])
        r = child(None, True)
        res["reads"] = r["reads"]
        res["this_pass_off_ms"].append(r["pass_off_ms"]); res["this_pass_on_ms"].append(r["pass_on_ms"]); res["qc_reads_ms"].append(r["qc_reads_ms"])
        assert r["rows_tallied_last_launch"] == r["reads"]
    med = statistics.median
    if a.parent_lib:
        res["report_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
    res["qc_reads_share_of_pass"] = med(res["qc_reads_ms"]) / med(res["this_pass_off_ms"])
    res["pass_on_vs_off"] = med(res["this_pass_on_ms"]) / med(res["this_pass_off_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
