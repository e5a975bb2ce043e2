"""What keeping `aio` on the device codec end to end (AMPLIPY_GPU_BAM=1 AMPLIPY_GPU_BAM_WRITE=1) is worth on the
bench's own e2e file (tools/e2e_legs.py: the first 1.5 M rows of the bench batch as a BAM of distinct records).  Three legs of the
whole `aio` command, every run a process of its own, the legs interleaved, `--reps` runs each after a dropped first one (median,
all samples kept):
  off      both switches off: libampbam reads and writes on host threads (the code path of every earlier commit; the baseline)
  deflate  the host codec with AMPLIPY_GPU_DEFLATE=1: the writer's blocks are compressed on the device (section 9)
  device   both switches on: compressed input up, compressed output down
and for the device leg the stages from HIP events summed over the pieces (copy up ... read pass, re-encode, DEFLATE, CRC and
framing, copy down), the bytes up and down, and whether the three trimmed BAMs hold the same records.  --kernel-stats FILE adds
the kernels' times from a `rocprofv3 --kernel-trace --stats` run of its own
(`rocprofv3 ... -- python tools/time_gpu_bam_write.py --one device --inp ...`).  Prints one JSON line (stored as
profiles/gpu_bam_write.json).  Needs a GPU.

usage: python tools/time_gpu_bam_write.py [--reps 7] [--reads 1500000] [--depth 10000] [--keep DIR] [--kernel-stats FILE]"""
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

LEGS = {"off": {}, "deflate": {"AMPLIPY_GPU_DEFLATE": "1"}, "device": {"AMPLIPY_GPU_BAM": "1", "AMPLIPY_GPU_BAM_WRITE": "1"}}
SWITCHES = ("AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_GPU_BAM_PIECE_BYTES")
STAGES = ("copy_up", "inflate", "crc", "index", "decode", "wait_and_host", "read_pass", "wait_and_host_2", "reencode", "deflate", "crc_and_framing",
          "copy_down")


def one_run(args):
    """A child: one `aio` run in this fresh process (its switches are in the environment); prints its wall time and the codec's
    counters."""
    from amplipy_amd import amplipy, bam_device
    log = sys.stderr
    sys.stderr = open(os.devnull, "w")
    try:
        t0 = time.perf_counter()
        amplipy.main(["aio", "-i", args.inp, "-p", args.bed, "-r", args.ref, "-ot", args.out + ".bam", "-ov", args.out + ".vcf", "-oc", args.out + ".fas"])
        dt = time.perf_counter() - t0
    finally:
        sys.stderr.close()
        sys.stderr = log
    print(json.dumps({"ms": round(dt * 1e3, 1), "stats": dict(bam_device.LAST_RUN_STATS) if args.one == "device" else None}))


def child(leg, inp, bed, ref, out):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(LEGS[leg])
    for ext in (".bam", ".vcf", ".fas"):
        if os.path.exists(out + ext):
            os.remove(out + ext)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg, "--inp", inp, "--bed", bed, "--ref", ref, "--out", out], env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("the %s leg failed (%d): %s" % (leg, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def stages(inp, G, primers, reps):
    """The device leg's stages per file from HIP events, summed over the pieces: median over reps of each sum."""
    from amplipy_amd import bam_device, lib
    eng = lib.Engine(G)
    eng.set_primers(*lib.find_overlapping_primers(G, [(s, e) for s, e, _ in primers], 0))
    eng.set_params(20, 4, True, True)
    codec = bam_device.BamCodec(eng)
    codec.stage_ms(on=True, read=False)
    samples = {k: [] for k in STAGES}
    for rep in range(reps + 1):
        src = bam_device.DeviceBamInput(inp)
        tot = [0.0] * len(STAGES)
        rb = 0
        n = len(src.pieces)
        for k, (info, st) in enumerate(bam_device.walk(codec, src)):
            if info.n_rows:
                codec.process(rb)
                rb += int(info.n_rows)
                codec.encode(30, False, final=k + 1 == n)
            ms = codec.stage_ms(on=True, read=True)
            tot = [a + max(b, 0.0) for a, b in zip(tot, ms)]
        eng.reset()
        if rep:
            for k, v in zip(STAGES, tot):
                samples[k].append(round(v, 3))
    codec.close(); eng.close()
    return {"ms_median": {k: statistics.median(v) for k, v in samples.items()}, "samples": samples}


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name") or ""
            if any(k in name for k in ("k_bgzf", "k_bam", "k_deflate", "k_fast", "DeviceScan")):
                rows.append(row)
    return rows


def records_of(path):
    from amplipy_amd import bam_native
    f = bam_native.BamFile(path)
    b, _ = f.decode(0, f.n_records, copy=True)
    out = (f.n_records, f.header_text, bytes(b.pos), bytes(b.cig), bytes(b.seq), bytes(b.qual))
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1500000)
    ap.add_argument("--depth", type=int, default=10000)
    ap.add_argument("--keep", default=None, help="directory that keeps the input file for a profiler run")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--one", choices=tuple(LEGS), default=None)
    ap.add_argument("--inp"); ap.add_argument("--bed"); ap.add_argument("--ref"); ap.add_argument("--out")
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
    tmp = args.keep or tempfile.mkdtemp(prefix="amp_gpubamw_")
    os.makedirs(tmp, exist_ok=True)
    out = {"metric": "gpu_bam_write", "reads": nb, "reps": args.reps}
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
        bed = os.path.join(tmp, "p.bed")
        with open(bed, "w") as f:
            f.write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(primers)))
        tab = bam_device.block_table(inp)
        out["input_bam_bytes"] = os.path.getsize(inp)
        out["input_inflated_bytes"] = int(tab[:, 2].sum())
        # ---- the whole command, a process per run, legs interleaved ----
        legs = {k: [] for k in LEGS}
        stats = None
        for rep in range(args.reps + 1):                     # rep 0 (page cache, code objects on disk) is dropped
            for leg in LEGS:
                r = child(leg, inp, bed, ref, os.path.join(tmp, leg))
                if rep:
                    legs[leg].append(r["ms"])
                if leg == "device":
                    stats = r["stats"]
        out["aio_ms"] = {k: {"median": statistics.median(v), "samples": v} for k, v in legs.items()}
        out["aio_reads_per_s"] = {k: round(nb / (statistics.median(v) / 1e3), 1) for k, v in legs.items()}
        out["device_over_off"] = round(out["aio_ms"]["off"]["median"] / out["aio_ms"]["device"]["median"], 3)
        out["output_bam_bytes"] = {k: os.path.getsize(os.path.join(tmp, k + ".bam")) for k in LEGS}
        recs = {k: records_of(os.path.join(tmp, k + ".bam")) for k in LEGS}
        out["trimmed_records"] = recs["device"][0]
        out["records_identical"] = recs["device"] == recs["off"] == recs["deflate"]
        with open(os.path.join(tmp, "device.bam"), "rb") as a, open(os.path.join(tmp, "deflate.bam"), "rb") as b:
            out["device_file_equals_deflate_file"] = a.read() == b.read()
        out["vcf_identical"] = open(os.path.join(tmp, "device.vcf"), "rb").read() == open(os.path.join(tmp, "off.vcf"), "rb").read()
        out["device_leg_counters"] = stats
        out["bytes_up_over_input_file"] = round(stats["bytes_up"] / stats["bytes_file"], 5)
        out["bytes_down_over_output_file"] = round(stats["bytes_down"] / out["output_bam_bytes"]["device"], 5)
        # ---- the stages of the device leg ----
        out["stages"] = stages(inp, G, primers, args.reps)
        if args.kernel_stats:
            out["kernel_trace"] = kernel_stats(args.kernel_stats)
        out["note"] = ("aio = the whole command in a fresh process, time taken inside it around amplipy.main (interpreter start and imports left "
                       "out, HIP start-up included); legs interleaved, first repetition dropped; off = libampbam on host threads for input and "
                       "output, the code path of the commits before the switch; stages = sums over the pieces of a file from HIP events")
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
