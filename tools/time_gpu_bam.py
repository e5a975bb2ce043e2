"""What the opt-in device codec for BAM input (AMPLIPY_GPU_BAM=1) is worth on the bench's own e2e file
(tools/e2e_legs.py: the first 1.5 M rows of the bench batch as a BAM of distinct records): the whole `variants` command with the
switch off (libampbam inflates, indexes and decodes on 16 host threads: the code path of every earlier commit) and on, every run a
process of its own, the legs interleaved, `--reps` runs each after a dropped first one (median, all samples kept); the stages of
the on leg from HIP events (copy up, inflate, CRC, record index, decode, read pass), the inflate kernel's rate, and a sweep of the
piece size.  --kernel-stats FILE adds the kernels' times from a `rocprofv3 --kernel-trace --stats` run of its own
(`rocprofv3 ... -- python tools/time_gpu_bam.py --one on --inp ...`).  Prints one JSON line (stored as profiles/gpu_bam.json).
Needs a GPU.

usage: python tools/time_gpu_bam.py [--reps 7] [--reads 1500000] [--depth 10000] [--keep DIR] [--kernel-stats FILE]"""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = (4 << 20, 16 << 20, 64 << 20)


def one_run(args):
    """A child: one `variants` run in this fresh process; prints its wall time and the codec's counters."""
    from amplipy_amd import amplipy, bam_device
    if args.one == "on":
        os.environ["AMPLIPY_GPU_BAM"] = "1"
    else:
        os.environ.pop("AMPLIPY_GPU_BAM", None)
    log = sys.stderr
    sys.stderr = open(os.devnull, "w")
    try:
        t0 = time.perf_counter()
        amplipy.main(["variants", "-i", args.inp, "-r", args.ref, "-o", args.out])
        dt = time.perf_counter() - t0
    finally:
        sys.stderr.close()
        sys.stderr = log
    print(json.dumps({"ms": round(dt * 1e3, 1), "stats": dict(bam_device.LAST_RUN_STATS) if args.one == "on" else None}))


def child(leg, inp, ref, out, piece_bytes=None):
    env = dict(os.environ)
    env.pop("AMPLIPY_GPU_BAM", None); env.pop("AMPLIPY_GPU_BAM_PIECE_BYTES", None)
    if piece_bytes:
        env["AMPLIPY_GPU_BAM_PIECE_BYTES"] = str(piece_bytes)
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg, "--inp", inp, "--ref", ref, "--out", out], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the %s leg failed (%d): %s" % (leg, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def stages(inp, G, piece_bytes, reps):
    """The on leg's stages per file from HIP events, summed over the pieces: median over reps of each sum."""
    from amplipy_amd import bam_device, lib
    eng = lib.Engine(G); eng.set_params(20, 4, False, True)
    codec = bam_device.BamCodec(eng)
    codec.stage_ms(on=True, read=False)
    names = ("copy_up", "inflate", "crc", "index", "decode", "wait_and_host", "read_pass")
    samples = {k: [] for k in names}
    inflated = blocks = 0
    for rep in range(reps + 1):
        src = bam_device.DeviceBamInput(inp, piece_bytes)
        tot = [0.0] * len(names)
        inflated = blocks = 0
        rb = 0
        for info, st in bam_device.walk(codec, src):
            if info.n_rows:
                codec.process(rb)
                rb += int(info.n_rows)
            ms = codec.stage_ms(on=True, read=True)
            tot = [a + max(b, 0.0) for a, b in zip(tot, ms)]
            inflated += int(info.n_inflated); blocks += int(info.n_blocks)
        eng.reset()
        if rep:
            for k, v in zip(names, tot):
                samples[k].append(round(v, 3))
    codec.close(); eng.close()
    med = {k: statistics.median(v) for k, v in samples.items()}
    return {"piece_bytes": piece_bytes, "ms_median": med, "samples": samples, "inflated_bytes": inflated, "blocks": blocks,
            "inflate_GB_per_s_of_output": round(inflated / med["inflate"] / 1e6, 2) if med["inflate"] > 0 else None,
            "inflate_blocks_per_s": round(blocks / (med["inflate"] / 1e3), 1) if med["inflate"] > 0 else None}


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name") or ""
            if "k_bgzf" in name or "k_bam" in name:
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1500000)
    ap.add_argument("--depth", type=int, default=10000)
    ap.add_argument("--keep", default=None, help="directory that keeps the input file for a profiler run")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--one", choices=("on", "off"), default=None)
    ap.add_argument("--inp"); ap.add_argument("--ref"); ap.add_argument("--out")
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    import torch
    from amplipy_amd import bam_device, bam_native, synth, synth_torch
    from tools.e2e_legs import write_bam
    dev = "cuda:0"
    torch.cuda.set_device(0)
    genome = synth.make_genome()
    primers, amps = synth.make_artic_scheme()
    G = int(genome.size)
    batch = synth_torch.make_amplicon_batch_device(genome, amps, synth.reads_for_depth(args.depth), seed=1000, device=dev)
    nb = min(batch.n, args.reads)
    tmp = args.keep or tempfile.mkdtemp(prefix="amp_gpubam_")
    os.makedirs(tmp, exist_ok=True)
    out = {"metric": "gpu_bam", "reads": nb, "reps": args.reps}
    try:
        seed = os.path.join(tmp, "seed.bam")
        if os.path.exists(seed):
            os.remove(seed)
        write_bam(seed, batch.to_host(0, 64), G)
        inp = os.path.join(tmp, "in.bam")
        if os.path.exists(inp):
            os.remove(inp)
        sf = bam_native.BamFile(seed)
        w = bam_native.BamWriter(inp, sf.header_text, sf, level=6)
        w.write_batch(batch.to_host(0, nb))
        w.close(); sf.close()
        del batch
        ref = os.path.join(tmp, "ref.fas")
        with open(ref, "w") as f:
            f.write(">SYN_REF\n" + synth.genome_string(genome) + "\n")
        tab = bam_device.block_table(inp)
        out["input_bam_bytes"] = os.path.getsize(inp)
        out["input_inflated_bytes"] = int(tab[:, 2].sum())
        out["input_blocks"] = int(len(tab))
        # ---- the whole command, a process per run, legs interleaved ----
        legs = {"off": [], "on": []}
        stats = None
        vcf = {}
        for rep in range(args.reps + 1):                     # rep 0 (page cache, code objects on disk) is dropped
            for leg in ("off", "on"):
                o = os.path.join(tmp, "%s.vcf" % leg)
                r = child(leg, inp, ref, o)
                if rep:
                    legs[leg].append(r["ms"])
                if leg == "on":
                    stats = r["stats"]
                with open(o, "rb") as f:
                    vcf[leg] = f.read()
        out["variants_ms"] = {k: {"median": statistics.median(v), "samples": v} for k, v in legs.items()}
        out["variants_reads_per_s"] = {k: round(nb / (statistics.median(v) / 1e3), 1) for k, v in legs.items()}
        out["vcf_identical"] = vcf["on"] == vcf["off"]
        out["on_leg_counters"] = stats
        out["bytes_up_over_file_bytes"] = round(stats["bytes_up"] / stats["bytes_file"], 5)
        # ---- the piece size ----
        sweep = {}
        for pb in SWEEP:
            v = []
            for rep in range(4):
                r = child("on", inp, ref, os.path.join(tmp, "sweep.vcf"), piece_bytes=pb)
                if rep:
                    v.append(r["ms"])
            sweep[str(pb)] = {"median": statistics.median(v), "samples": v, "pieces": r["stats"]["pieces"]}
        out["piece_sweep_variants_ms"] = sweep
        # ---- the stages of the on leg ----
        out["stages"] = stages(inp, G, bam_device.PIECE_BYTES, args.reps)
        out["stages_one_piece"] = stages(inp, G, 1 << 30, 3)
        if args.kernel_stats:
            out["kernel_trace"] = kernel_stats(args.kernel_stats)
        out["note"] = ("variants = the whole command in a fresh process, time taken inside it around amplipy.main (interpreter start and "
                       "imports left out, HIP start-up included); legs interleaved, first repetition dropped; off = libampbam on 16 host "
                       "threads, the code path of the commits before the switch; stages = sums over the pieces of a file from HIP events")
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
