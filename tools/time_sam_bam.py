"""What SAM text in, trimmed BAM out on the device codec (AMPLIPY_GPU_SAM=1 AMPLIPY_GPU_BAM_WRITE=1) is worth on the
bench's own e2e records (tools/e2e_legs.py: the first rows of the bench batch) written as one SAM file.  Three legs of the whole
`aio` command, every run a process of its own, the legs interleaved, `--reps` runs each after a dropped first one (median, all
samples kept):
  off     both switches off: the Python codec of bamio reads the text and writes the BAM (the code path of every earlier commit;
          the baseline)
  sam     AMPLIPY_GPU_SAM=1 alone: as off -- the device codec for text does not serve a BAM output on its own
  device  both switches on: text up, framed BGZF blocks and 128 bytes of counters per encode down
and for the device leg the stages from HIP events summed over the chunks (copy up ... read pass, records, DEFLATE, CRC and
framing, copy down), the counters of the run, and whether the three trimmed BAMs inflate to the same bytes.  Writes
profiles/gpu_sam_bam.json and prints it.  The kernels' times come from a `rocprofv3 --kernel-trace --stats` run of its own on the
kept input, merged into the file afterwards:
  python tools/time_sam_bam.py --keep DIR
  rocprofv3 --kernel-trace --stats -d DIR/prof -- python tools/time_sam_bam.py --one device --inp DIR/in.sam --bed DIR/p.bed --ref DIR/ref.fas --cwd DIR/run
  python tools/time_sam_bam.py --merge-kernel-stats DIR/prof/.../..._kernel_stats.csv
Needs a GPU.

usage: python tools/time_sam_bam.py [--reps 5] [--reads 100000] [--depth 10000] [--keep DIR] [--out FILE]"""
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

LEGS = {"off": {}, "sam": {"AMPLIPY_GPU_SAM": "1"}, "device": {"AMPLIPY_GPU_SAM": "1", "AMPLIPY_GPU_BAM_WRITE": "1"}}
SWITCHES = ("AMPLIPY_GPU_SAM", "AMPLIPY_GPU_BAM", "AMPLIPY_GPU_BAM_WRITE", "AMPLIPY_GPU_DEFLATE", "AMPLIPY_SAM_CHUNK_BYTES")
STAGES = {"copy_up": 0, "scan_ranks": 1, "lines_tabs": 2, "records_rows_aux": 3, "pack": 4, "read_pass": 6, "bam_records": 11, "deflate": 12,
          "crc_and_framing": 13, "copy_down": 14}


def one_run(args):
    """A child: one `aio` run in this fresh process (its switches are in the environment, its outputs go to the working
    directory under the same names in every leg: the @PG line records the command); prints its wall time and the codec's counters."""
    from amplipy_amd import amplipy, sam_native
    os.makedirs(args.cwd, exist_ok=True)
    os.chdir(args.cwd)
    for name in ("t.bam", "v.vcf", "c.fas"):
        if os.path.exists(name):
            os.remove(name)
    log = sys.stderr
    sys.stderr = open(os.devnull, "w")
    sys.argv = ["amplipy_amd", "time_sam_bam"]
    try:
        t0 = time.perf_counter()
        amplipy.main(["aio", "-i", args.inp, "-p", args.bed, "-r", args.ref, "-ot", "t.bam", "-ov", "v.vcf", "-oc", "c.fas"])
        dt = time.perf_counter() - t0
    finally:
        sys.stderr.close()
        sys.stderr = log
    print(json.dumps({"ms": round(dt * 1e3, 1), "stats": dict(sam_native.LAST_RUN_STATS) if args.one == "device" else None}))


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
    """The device leg's stages per file from HIP events, summed over the chunks: median over reps of each sum."""
    from amplipy_amd import lib, sam_native
    eng = lib.Engine(G)
    eng.set_primers(*lib.find_overlapping_primers(G, [(s, e) for s, e, _ in primers], 0))
    eng.set_params(20, 4, True, True)
    codec = sam_native.SamCodec(eng)
    codec.set_references(["SYN_REF"])
    codec.set_output(sam_native.OUT_BAM)
    codec.stage_ms(on=True, read=False)
    samples = {k: [] for k in STAGES}
    chunks = text = 0
    for rep in range(reps + 1):
        src = sam_native.SamTextInput(inp)
        tot = {k: 0.0 for k in STAGES}
        rb = chunks = text = 0
        for chunk in src:
            info = codec.parse(chunk)
            if info.n_rows:
                codec.process(rb, defer=True)
                rb += int(info.n_rows)
                codec.encode(30, False)
            ms = codec.stage_ms(on=True, read=True)
            for k, i in STAGES.items():
                tot[k] += max(ms[i], 0.0)
            chunks += 1; text += len(chunk)
        codec.encode_bytes(b"", final=True)
        src.close()
        eng.reset()
        if rep:
            for k in STAGES:
                samples[k].append(round(tot[k], 3))
    codec.close(); eng.close()
    return {"ms_median": {k: statistics.median(v) for k, v in samples.items()}, "samples": samples, "chunks": chunks, "text_bytes": text}


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name") or ""
            if any(k in name for k in ("k_sam", "k_out_", "k_deflate", "k_fast", "DeviceScan")):
                rows.append(row)
    return rows


def inflated(path):
    from amplipy_amd import bamio
    with open(path, "rb") as f:
        return b"".join(bamio.bgzf_blocks(f))


def write_sam(path, hb, G):
    """The rows of the packed host batch as SAM text (the records tools/e2e_legs.py writes as BAM)."""
    import numpy as np
    from amplipy_amd import bamio
    from amplipy_amd.batch import SEQ_NT16, unpack_nibbles
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % G, [("SYN_REF", G)])
    w = bamio.AlignmentWriter(path, "w", hdr)
    lut = np.frombuffer(SEQ_NT16.encode(), np.uint8)
    for i in range(hb.n):
        o = int(hb.seq_off[i]); L = int(hb.lseq[i])
        seq = lut[unpack_nibbles(hb.seq[o // 2:(o + L + 1) // 2], L)].tobytes().decode()
        a, c = int(hb.cig_off[i]), int(hb.cig_off[i + 1])
        w.write(bamio.Rec("r%d" % i, int(hb.flag[i]), 0, int(hb.pos[i]), 60, [(int(v) & 15, int(v) >> 4) for v in hb.cig[a:c]], 0,
                          int(hb.pos[i]), int(hb.tlen[i]), seq, bytes(hb.qual[o:o + L]), aux_sam=["NM:i:1", "AS:i:290"]))
    w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--depth", type=int, default=10000)
    ap.add_argument("--keep", default=None, help="directory that keeps the input file for a profiler run")
    ap.add_argument("--merge-kernel-stats", default=None, help="a kernel_stats.csv of rocprofv3: its rows are added to the file of --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_sam_bam.json"))
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
    from amplipy_amd import synth, synth_torch
    dev = "cuda:0"
    torch.cuda.set_device(0)
    genome = synth.make_genome()
    primers, amps = synth.make_artic_scheme()
    G = int(genome.size)
    batch = synth_torch.make_amplicon_batch_device(genome, amps, synth.reads_for_depth(args.depth), seed=1000, device=dev)
    nb = min(batch.n, args.reads)
    tmp = args.keep or tempfile.mkdtemp(prefix="amp_sambam_")
    os.makedirs(tmp, exist_ok=True)
    out = {"metric": "gpu_sam_bam", "reads": nb, "reps": args.reps}
    try:
        inp = os.path.join(tmp, "in.sam")
        write_sam(inp, batch.to_host(0, nb), G)
        del batch
        ref = os.path.join(tmp, "ref.fas")
        with open(ref, "w") as f:
            f.write(">SYN_REF\n" + synth.genome_string(genome) + "\n")
        bed = os.path.join(tmp, "p.bed")
        with open(bed, "w") as f:
            f.write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(primers)))
        out["input_sam_bytes"] = os.path.getsize(inp)
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
        out["sam_over_off"] = round(out["aio_ms"]["off"]["median"] / out["aio_ms"]["sam"]["median"], 3)
        out["output_bam_bytes"] = {k: os.path.getsize(os.path.join(tmp, k, "t.bam")) for k in LEGS}
        payload = {k: inflated(os.path.join(tmp, k, "t.bam")) for k in LEGS}
        out["output_inflated_bytes"] = len(payload["device"])
        out["bams_inflate_to_the_same_bytes"] = payload["device"] == payload["off"] == payload["sam"]
        out["vcf_and_fasta_identical"] = all(open(os.path.join(tmp, "device", n), "rb").read() == open(os.path.join(tmp, "off", n), "rb").read()
                                             for n in ("v.vcf", "c.fas"))
        out["device_leg_counters"] = stats
        out["bytes_down_over_output_file"] = round(stats["bytes_down"] / out["output_bam_bytes"]["device"], 5)
        # ---- the stages of the device leg ----
        out["stages"] = stages(inp, G, primers, args.reps)
        out["note"] = ("aio = the whole command in a fresh process, time taken inside it around amplipy.main (interpreter start and imports left "
                       "out, HIP start-up included); legs interleaved, first repetition dropped; off = the Python codec of bamio for input and "
                       "output, the code path of the commits before the switch; stages = sums over the chunks of a file from HIP events")
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
