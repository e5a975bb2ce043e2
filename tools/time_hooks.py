"""What the read pass and the three windowed tally kernels behind it cost (k_strand, k_amplicon, k_codon),
on the benchmark's 10k x batch (1,993,533 reads of 150 bases, built on the device by synth_torch) through process_device with
every per-read output.  A leg is one process with one build of the library, ONE engine and ONE batch:

  * the read pass with every hook off (amp_last_kernel_ms);
  * then each hook on alone: amp_strand_last_ms, amp_amplicon_last_ms (the synthetic primer set paired into amplicons), and
    amp_codon_last_ms (one frame over the whole reference).

20 launches per figure after 5 warm-up launches, medians.  With --parent-lib the two builds take turns, a fresh process each
(AMPLIPY_DEV=1 AMPLIHIP_LIB=path picks the library), so that both are measured in one job on one box; a figure of this build
is `within` when its median over the rounds is at most the parent's median plus the parent's own spread (max - min) over its
rounds.  The set-up and the child process here are what tools/time_strand.py, time_amplicon.py and time_codon.py use as well.

  python tools/time_hooks.py [--parent-lib PATH/libamplihip.so] [--rounds 5] [--out profiles/hooks_shared.json]
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
BATCH = "10k x depth, 150-base reads (synth_torch, seed 1000)"
FIGURES = ("pass_off_ms", "strand_ms", "amplicon_ms", "codon_ms")


class Setup:
    """The benchmark's batch on the device, the buffers of a trimming pass's results, and an engine that trims and counts."""

    def __init__(self):
        import torch
        from amplipy_amd import abi, lib, synth, synth_torch
        g = synth.make_genome()
        self.primers, self.amps = synth.make_artic_scheme()
        self.G = int(g.size)
        self.n = synth.reads_for_depth(10000)
        mn, mx, mpl = lib.find_overlapping_primers(self.G, sorted((s, e) for s, e, _ in self.primers), 0)
        self.batch = synth_torch.make_amplicon_batch_device(g, self.amps, self.n, 1000, "cuda:0")
        torch.cuda.synchronize()
        self.rd = self.batch.struct()
        fields = (("new_pos", self.n, torch.int32), ("new_ncig", self.n, torch.int32), ("new_cig", self.batch.n_cig + 3 * self.n, torch.int32),
                  ("ref_len", self.n, torch.int32), ("trim_flags", self.n, torch.uint8), ("status", self.n, torch.uint8))
        self.out = {k: torch.zeros(sz, dtype=dt, device="cuda:0") for k, sz, dt in fields}
        self.dev_out = abi.AmpTrimOut(*[self.out[k].data_ptr() for k, _, _ in fields])
        self.eng = lib.Engine(self.G)
        self.eng.set_primers(mn, mx, mpl)
        self.eng.set_params(20, 4, True, True)
        self.eng.reserve_events(1 << 22)

    def launches(self, timer=None):
        """WARMUP + LAUNCHES batches -> (the read pass's ms, the timer's ms) of the last LAUNCHES."""
        e, ps, ks = self.eng, [], []
        for it in range(WARMUP + LAUNCHES):
            e.reset(); e.process_device(self.rd, 0, self.dev_out); e.sync()
            if it >= WARMUP:
                ps.append(e.last_kernel_ms()[0])
                if timer is not None:
                    ks.append(timer())
        return ps, ks

    def amplicon_set(self):
        """The synthetic primer set paired into amplicons: SYN_<k>_LEFT with SYN_<k>_RIGHT."""
        from amplipy_amd import amplicon
        rows = sorted(self.primers, key=lambda r: (r[0], r[1]))
        pairs = [("SYN_%d_LEFT" % k, "SYN_%d_RIGHT" % k, "SYN_%d" % k) for k in range(1, len(self.primers) // 2 + 1)]
        return amplicon.build_amplicons(pairs, rows, 0, self.G)


def child(script, args, lib_path=None, timeout=300):
    """A fresh process for one leg, under a time limit -> what its 'LEG ' line holds."""
    env = dict(os.environ)
    if lib_path:
        env.update(AMPLIPY_DEV="1", AMPLIHIP_LIB=os.path.abspath(lib_path))
    r = subprocess.run([sys.executable, os.path.abspath(script)] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("leg failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])


def leg():
    import numpy as np
    from amplipy_amd import amplicon
    s = Setup()
    e, med = s.eng, statistics.median
    res = {"reads": s.n, "pass_off_ms": med(s.launches()[0])}
    e.strand_enable()
    res["strand_ms"] = med(s.launches(e.strand_last_ms)[1])
    e.strand_disable()
    amplicon.enable(e, s.amplicon_set())
    res["amplicon_ms"] = med(s.launches(e.amplicon_last_ms)[1])
    e.amplicon_disable()
    e.codon_enable(np.arange(0, s.G - 2, 3, dtype=np.int32))
    res["codon_ms"] = med(s.launches(e.codon_last_ms)[1])
    e.codon_disable()
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib", help="libamplihip.so of the parent commit: timed in turn with this build")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hooks_shared.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    if a.parent_lib and a.rounds < 5:
        ap.error("a comparison takes at least five rounds")
    res = {"batch": BATCH, "launches_per_figure": LAUNCHES, "rounds": {"parent": [], "this": []}}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["rounds"]["parent"].append(child(__file__, ["--leg"], a.parent_lib))
        res["rounds"]["this"].append(child(__file__, ["--leg"]))
    for key in FIGURES:
        row = {}
        for who, rounds in res["rounds"].items():
            v = [r[key] for r in rounds]
            if v:
                row[who] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        if "parent" in row:
            p = row["parent"]
            row["within"] = row["this"]["median"] <= p["median"] + (p["max"] - p["min"])
        res[key] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in FIGURES}, indent=1))


if __name__ == "__main__":
    main()
