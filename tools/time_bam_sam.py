"""What BAM in, trimmed SAM text out on the device codec (AMPLIPY_GPU_BAM=1 AMPLIPY_GPU_SAM=1) is worth on the
bench's own e2e file (tools/e2e_legs.py: the first 1.5 M rows of the bench batch as a BAM of distinct records).  Two legs of
`trim -i e2e.bam -o out.sam`, every run a process of its own, the legs interleaved, `--reps` runs each after a dropped first one
(median, all samples kept):
  off     both switches off: the Python codec of bamio reads the BAM and writes the text (the code path of every earlier commit;
          the baseline)
  device  both switches on: compressed input up, the kept reads' lines and 24 bytes of counters per piece down
and for the device leg the stages from HIP events summed over the pieces (copy up ... read pass, text check, sizes and lines,
copy down), the counters of the run, and whether the two files are equal.  Writes profiles/gpu_bam_sam.json and prints it.  The
kernels' times come from a `rocprofv3 --kernel-trace --stats` run of its own on the kept input, merged into the file afterwards:
  python tools/time_bam_sam.py --keep DIR [--input-only]
  AMPLIPY_GPU_BAM=1 AMPLIPY_GPU_SAM=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR/prof -- python tools/time_bam_sam.py --one device --inp DIR/in.bam --bed DIR/p.bed --ref DIR/ref.fas --cwd DIR/run
  python tools/time_bam_sam.py --merge-kernel-stats DIR/prof/.../..._kernel_stats.csv
Needs a GPU.

usage: python tools/time_bam_sam.py [--reps 5] [--reads 1500000] [--depth 10000] [--keep DIR [--input-only]] [--out FILE]"""
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

LEGS = {"off": {}, "device": {"AMPLIPY_GPU_BAM": "1", "AMPLIPY_GPU_SAM": "1"}}
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_GPU_BAM_PIECE_BYTES", "AMPLIPY_PYTHON_BAM")
STAGES = {"copy_up": 0, "inflate": 1, "crc": 2, "index": 3, "decode": 4, "read_pass": 6, "text_check": 12, "sizes_and_lines": 14, "copy_down": 15}


def one_run(args):
    """A child: one `trim` run in this fresh process (its switches are in the environment, its output goes to the working directory
    under the same name in every leg: the @PG line records the command); prints its wall time and the codec's counters."""
    from amplipy_amd import amplipy, bam_device
    os.makedirs(args.cwd, exist_ok=True)
    os.chdir(args.cwd)
    if os.path.exists("out.sam"):
        os.remove("out.sam")
    log = sys.stderr
    sys.stderr = open(os.devnull, "w")
    sys.argv = ["amplipy_amd", "time_bam_sam"]
    try:
        t0 = time.perf_counter()
        amplipy.main(["trim", "-i", args.inp, "-p", args.bed, "-r", args.ref, "-o", "out.sam"])
        dt = time.perf_counter() - t0
    finally:
        sys.stderr.close()
        sys.stderr = log
    print(json.dumps({"ms": round(dt * 1e3, 1), "stats": dict(bam_device.LAST_RUN_STATS) if args.one == "device" else None}))


def child(leg, inp, bed, ref, cwd):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(LEGS[leg])
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg, "--inp", inp, "--bed", bed, "--ref", ref, "--cwd", cwd], env=env,
                       capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        raise RuntimeError("the %s leg failed (%d): %s" % (leg, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def stages(inp, G, primers, reps):
    """The device leg's stages per file from HIP events, summed over the pieces: median over reps of each sum."""
    from amplipy_amd import bam_device, lib
    eng = lib.Engine(G)
    eng.set_primers(*lib.find_overlapping_primers(G, [(s, e) for s, e, _ in primers], 0))
    eng.set_params(20, 4, True, False)
    codec = bam_device.BamCodec(eng)
    codec.stage_ms(on=True, read=False)
    samples = {k: [] for k in STAGES}
    pieces = text = 0
    for rep in range(reps + 1):
        src = bam_device.DeviceBamInput(inp)
        codec.set_references([n for n, _ in src.references])
        tot = {k: 0.0 for k in STAGES}
        rb = pieces = text = 0
        for info, st in bam_device.walk(codec, src):
            if codec.text_check().first_odd_row >= 0:
                raise RuntimeError("a piece of the bench's file is odd")
            if info.n_rows:
                codec.process(rb)
                rb += int(info.n_rows)
                text += len(codec.format(30, False)[0])
            ms = codec.stage_ms(on=True, read=True)
            for k, i in STAGES.items():
                tot[k] += max(ms[i], 0.0)
            pieces += 1
        eng.reset()
        if rep:
            for k in STAGES:
                samples[k].append(round(tot[k], 3))
    codec.close(); eng.close()
    return {"ms_median": {k: statistics.median(v) for k, v in samples.items()}, "samples": samples, "pieces": pieces, "text_bytes": text}


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name") or ""
            if any(k in name for k in ("k_bgzf", "k_bam", "k_fast", "DeviceScan")):
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1500000)
    ap.add_argument("--depth", type=int, default=10000)
    ap.add_argument("--keep", default=None, help="directory that keeps the input file for a profiler run")
    ap.add_argument("--input-only", action="store_true", help="with --keep: write the input files and stop")
    ap.add_argument("--merge-kernel-stats", default=None, help="a kernel_stats.csv of rocprofv3: its rows are added to the file of --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_bam_sam.json"))
    ap.add_argument("--one", choices=tuple(LEGS), default=None)
    ap.add_argument("--inp"); ap.add_argument("--bed"); ap.add_argument("--ref"); ap.add_argument("--cwd")
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    if args.merge_kernel_stats:
        out = json.load(open(args.out))
        out["kernel_trace"] = kernel_stats(args.merge_kernel_stats)
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
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
    tmp = args.keep or tempfile.mkdtemp(prefix="amp_bamsam_")
    os.makedirs(tmp, exist_ok=True)
    out = {"metric": "gpu_bam_sam", "reads": nb, "reps": args.reps}
    try:
        seed = os.path.join(tmp, "seed.bam")
        inp = os.path.join(tmp, "in.bam")
        for p in (seed, inp):
            if os.path.exists(p):
                os.remove(p)
        write_bam(seed, batch.to_host(0, 64), G)
        sf = bam_native.BamFile(seed)
        w = bam_native.BamWriter(inp, sf.header_text, sf, level=6)
        w.write_batch(batch.to_host(0, nb))
        w.close(); sf.close()
        del batch
        ref = os.path.join(tmp, "ref.fas")
        with open(ref, "w") as f:
            f.write(">SYN_REF\n" + synth.genome_string(genome) + "\n")
        bed = os.path.join(tmp, "p.bed")
        with open(bed, "w") as f:
            f.write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(primers)))
        if args.input_only:
            return
        out["input_bam_bytes"] = os.path.getsize(inp)
        out["input_inflated_bytes"] = int(bam_device.block_table(inp)[:, 2].sum())
        # ---- the whole command, a process per run, legs interleaved ----
        legs = {k: [] for k in LEGS}
        stats = None
        for rep in range(args.reps + 1):                     # rep 0 (page cache, code objects on disk) is dropped
            for leg in LEGS:
                r = child(leg, inp, bed, ref, os.path.join(tmp, leg))
                print("rep %d %s: %.0f ms" % (rep, leg, r["ms"]), file=sys.stderr, flush=True)
                if rep:
                    legs[leg].append(r["ms"])
                if leg == "device":
                    stats = r["stats"]
        out["trim_ms"] = {k: {"median": statistics.median(v), "samples": v} for k, v in legs.items()}
        out["trim_reads_per_s"] = {k: round(nb / (statistics.median(v) / 1e3), 1) for k, v in legs.items()}
        out["device_over_off"] = round(out["trim_ms"]["off"]["median"] / out["trim_ms"]["device"]["median"], 3)
        out["output_sam_bytes"] = {k: os.path.getsize(os.path.join(tmp, k, "out.sam")) for k in LEGS}
        with open(os.path.join(tmp, "device", "out.sam"), "rb") as a, open(os.path.join(tmp, "off", "out.sam"), "rb") as b:
            out["files_equal"] = a.read() == b.read()
        out["device_leg_counters"] = stats
        out["bytes_up_over_input_file"] = round(stats["bytes_up"] / stats["bytes_file"], 5)
        out["bytes_down_over_output_file"] = round(stats["bytes_down"] / out["output_sam_bytes"]["device"], 5)
        # ---- the stages of the device leg ----
        out["stages"] = stages(inp, G, primers, args.reps)
        out["note"] = ("trim = the whole command in a fresh process, time taken inside it around amplipy.main (interpreter start and imports left "
                       "out, HIP start-up included); legs interleaved, first repetition dropped; off = the Python codec of bamio for input and "
                       "output, the code path of the commits before the switch; stages = sums over the pieces of a file from HIP events")
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
