"""What the clip sites of the QC report cost, on the benchmark's 10k x batch (1,993,533 reads of 150 bases,
built on the device by synth_torch) through process_device with every per-read output.  k_qc_clips (amp_qc_clips_last_ms) beside
k_qc_reads (amp_qc_last_ms) in the same launches, on three inputs:

  a  the batch as it is: no read is clipped;
  b  every read given a 20-base clip at both ends (20S110M20S at pos + 20): the sites form piles, the pre-trimmed case;
  c  the same reads, read i at position i mod (G - 200): the 64 reads of a wave have 64 sites of their own on either side.

And the read pass with every switch OFF -- with --parent-lib, against another build of the library (the parent commit) in
processes of their own, the two builds taking turns, so that what is held to the box's run-to-run spread is measured in one job
on one box.

  python tools/time_clips.py [--parent-lib PATH/libamplihip.so] [--out profiles/qc_clips.json]
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
CLIP, CLIP_MIN = 20, 10


def leg(with_clips):
    """One process, one build of the library: medians over LAUNCHES launches."""
    import torch
    from amplipy_amd import abi, lib, synth, synth_torch
    if not with_clips:            # (the parent build has none of the new entry points)
        lib.EXPORTS[:] = [n for n in lib.EXPORTS if not n.startswith("amp_qc_clips_")]
    g = synth.make_genome(); primers, amps = synth.make_artic_scheme(); G = int(g.size)
    pr = sorted((s, e) for s, e, _ in primers)
    n = synth.reads_for_depth(10000)
    mn, mx, mpl = lib.find_overlapping_primers(G, pr, 0)
    b = synth_torch.make_amplicon_batch_device(g, amps, n, 1000, "cuda:0"); torch.cuda.synchronize()
    e = lib.Engine(G); e.set_primers(mn, mx, mpl); e.set_params(20, 4, True, True); e.reserve_events(1 << 22)

    def outputs(batch):
        out = {k: torch.zeros(sz, dtype=dt, device="cuda:0") for k, sz, dt in
               (("new_pos", n, torch.int32), ("new_ncig", n, torch.int32), ("new_cig", batch.n_cig + 3 * n, torch.int32),
                ("ref_len", n, torch.int32), ("trim_flags", n, torch.uint8), ("status", n, torch.uint8))}
        return out, abi.AmpTrimOut(*[out[k].data_ptr() for k in ("new_pos", "new_ncig", "new_cig", "ref_len", "trim_flags", "status")])

    def clipped(pos):
        """Every read of b as 20S110M20S at ``pos``; bases, qualities and flags stay."""
        L = 150
        ops = torch.tensor([(CLIP << 4) | 4, ((L - 2 * CLIP) << 4) | 0, (CLIP << 4) | 4], dtype=torch.int32, device="cuda:0")
        return synth_torch.DeviceBatch(n, pos.to(torch.int32).contiguous(), b.flag, b.tlen, b.lseq, (3 * torch.arange(n + 1, device="cuda:0")).to(torch.int32),
                                       ops.repeat(n).contiguous(), b.seq_off8, b.seq, b.qual, 3 * n, b.n_bases_padded)

    def launches(batch, clips_on):
        keep, dev_out = outputs(batch)
        rd = batch.struct()
        ps, qs, cs = [], [], []
        for it in range(WARMUP + LAUNCHES):
            e.reset(); e.process_device(rd, 0, dev_out); e.sync()
            if it >= WARMUP:
                ps.append(e.last_kernel_ms()[0])
                if clips_on:
                    qs.append(e.qc_last_ms()); cs.append(e.qc_clips_last_ms())
        del keep
        return ps, qs, cs
    med = statistics.median
    res = {"reads": n, "pass_off_ms": med(launches(b, False)[0])}
    if with_clips:
        e.qc_enable(pr, 0, 30, False, [(0, G)], [1, 10, 100])
        e.qc_clips_enable(CLIP_MIN)
        inputs = {"a": b, "b": clipped(b.pos + CLIP), "c": clipped(torch.arange(n, device="cuda:0") % (G - 200) + CLIP)}
        for name, batch in inputs.items():
            ps, qs, cs = launches(batch, True)
            table, scalars = e.qc_clips_tables()          # of the last launch
            res[name] = dict(pass_ms=med(ps), qc_reads_ms=med(qs), qc_clips_ms=med(cs), qc_clips_ms_min=min(cs), qc_clips_ms_max=max(cs),
                             scanned=int(scalars[0]), skipped=int(scalars[1]), left=int(scalars[2]), right=int(scalars[3]),
                             left_sites=int((table[:, 0, 0] > 0).sum()), right_sites=int((table[:, 1, 0] > 0).sum()))
            assert int(scalars[0]) + int(scalars[1]) <= n and int(table[:, :, 0].sum()) == int(scalars[2]) + int(scalars[3])
            if name != "a":
                assert int(scalars[2]) == int(scalars[3]) == int(scalars[0])
    e.close()
    print("LEG " + json.dumps(res))


def child(lib_path, with_clips):
    env = dict(os.environ)
    if lib_path:
        env.update(AMPLIPY_DEV="1", AMPLIHIP_LIB=lib_path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "clips" if with_clips else "pass"], env=env, capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("leg failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["pass", "clips"])
    ap.add_argument("--parent-lib", help="libamplihip.so of the parent commit: its read pass is timed in turn with this build's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc_clips.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == "clips")
    med = statistics.median
    res = {"batch": "10k x depth, 150-base reads (synth_torch, seed 1000)", "launches_per_figure": LAUNCHES, "clip_min": CLIP_MIN,
           "inputs": {"a": "as it is: no clips", "b": "20S110M20S at pos + 20: piles (the pre-trimmed case)",
                      "c": "20S110M20S at i mod (G - 200): every read of a wave a site of its own"},
           "parent_pass_ms": [], "this_pass_off_ms": [], "rounds": []}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["parent_pass_ms"].append(child(a.parent_lib, False)["pass_off_ms"])
        r = child(None, True)
        res["reads"] = r["reads"]
        res["this_pass_off_ms"].append(r["pass_off_ms"])
        res["rounds"].append({name: r[name] for name in ("a", "b", "c")})
    for name in ("a", "b", "c"):
        res[name] = {k: med([rd[name][k] for rd in res["rounds"]]) for k in ("pass_ms", "qc_reads_ms", "qc_clips_ms")}
        res[name].update({k: res["rounds"][-1][name][k] for k in ("scanned", "skipped", "left", "right", "left_sites", "right_sites")})
    spread = lambda v: (max(v) - min(v)) / med(v)
    res["this_pass_off_spread"] = spread(res["this_pass_off_ms"])
    if a.parent_lib:
        res["parent_pass_spread"] = spread(res["parent_pass_ms"])
        res["switches_off_vs_parent"] = med(res["this_pass_off_ms"]) / med(res["parent_pass_ms"])
        res["within_parent_spread"] = min(res["parent_pass_ms"]) <= med(res["this_pass_off_ms"]) <= max(res["parent_pass_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
