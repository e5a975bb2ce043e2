"""What the opt-in device DEFLATE encoder of the BAM writer (AMPLIPY_GPU_DEFLATE=1) is worth on the bench's own
e2e file (tools/e2e_legs.py: the first 1.5 M rows of the bench batch as a BAM of distinct records): the stage "re-encode + DEFLATE +
write" alone and the whole `aio` command for the host codec at its shipped level (-1), the host codec at level 1 and the device
encoder; the encoder kernel alone on the trimmed file's inflated bytes; the size of each trimmed file.  The legs are run
interleaved, `--reps` times each (median, all samples kept).  Prints one JSON line (stored as profiles/gpu_deflate.json).  Needs a GPU.

usage: python tools/time_gpu_deflate.py [--reps 7] [--reads 1500000] [--depth 10000]"""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = (("host_level_default", {"AMPLIPY_BAM_LEVEL": "-1"}), ("host_level_1", {"AMPLIPY_BAM_LEVEL": "1"}),
        ("gpu_deflate", {"AMPLIPY_BAM_LEVEL": "-1", "AMPLIPY_GPU_DEFLATE": "1"}))


def _set_env(env):
    for k in ("AMPLIPY_BAM_LEVEL", "AMPLIPY_GPU_DEFLATE"):
        os.environ.pop(k, None)
    os.environ.update(env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1500000)
    ap.add_argument("--depth", type=int, default=10000)
    args = ap.parse_args()
    import torch
    from amplipy_amd import amplipy, bam_native, lib, synth, synth_torch
    from tools.e2e_legs import write_bam
    dev = "cuda:0"
    torch.cuda.set_device(0)
    genome = synth.make_genome()
    primers, amps = synth.make_artic_scheme()
    G = int(genome.size)
    batch = synth_torch.make_amplicon_batch_device(genome, amps, synth.reads_for_depth(args.depth), seed=1000, device=dev)
    nb = min(batch.n, args.reads)
    tmp = tempfile.mkdtemp(prefix="amp_gpudeflate_")
    out = {"metric": "gpu_deflate", "reads": nb, "reps": args.reps}
    try:
        # ---- the bench's e2e input file ----
        seed = os.path.join(tmp, "seed.bam")
        write_bam(seed, batch.to_host(0, 64), G)
        inp = os.path.join(tmp, "in.bam")
        sf = bam_native.BamFile(seed)
        hbb = batch.to_host(0, nb)
        w = bam_native.BamWriter(inp, sf.header_text, sf, level=6)
        w.write_batch(hbb)
        w.close(); sf.close()
        del hbb, batch
        with open(os.path.join(tmp, "ref.fas"), "w") as f:
            f.write(">SYN_REF\n" + synth.genome_string(genome) + "\n")
        with open(os.path.join(tmp, "p.bed"), "w") as f:
            f.write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(primers)))
        out["input_bam_bytes"] = os.path.getsize(inp)
        # ---- the stage alone: one write_rows of the whole file + close ----
        mn, mx, mpl = lib.find_overlapping_primers(G, [(s, e) for s, e, _ in primers], 0)
        src = bam_native.BamFile(inp)
        bb, _ = src.decode(0, src.n_records)
        eng = lib.Engine(G); eng.set_primers(mn, mx, mpl); eng.set_params(20, 4, True, True)
        res = eng.process(bb)
        keep = (res.ref_len >= 30) & ((res.trim_flags & 3) != 0)
        slot = bb.cig_off[:-1] + np.uint64(3) * np.arange(bb.n, dtype=np.uint64)
        stage = {k: [] for k, _ in LEGS}
        sizes, blocks = {}, {}
        stage_path = os.path.join(tmp, "stage.bam")
        for rep in range(args.reps + 1):                     # rep 0 warms every leg up (buffers, the device's staging) and is dropped
            for leg, env in LEGS:
                if os.path.exists(stage_path):
                    os.remove(stage_path)
                wr = bam_native.BamWriter(stage_path, src.header_text, src, level=int(env["AMPLIPY_BAM_LEVEL"]), gpu_deflate="AMPLIPY_GPU_DEFLATE" in env)
                t0 = time.perf_counter()
                wr.write_rows(None, bb.src_index, keep, res.new_pos, res.new_ncig, slot, res.new_cig)
                st = wr.deflater_stats()
                wr.close()
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    stage[leg].append(round(dt, 1))
                sizes[leg] = os.path.getsize(stage_path); blocks[leg] = st
                if leg == "gpu_deflate" and rep == 0:
                    shutil.copy(stage_path, os.path.join(tmp, "gpu_stage.bam"))
        eng.close(); src.close()
        out["stage_reencode_deflate_write_ms"] = {k: {"median": statistics.median(v), "samples": v} for k, v in stage.items()}
        out["trimmed_bam_bytes"] = sizes
        out["gpu_leg_blocks_device_host_failed"] = list(blocks["gpu_deflate"])
        # ---- the kernel alone, on the inflated bytes of the trimmed file ----
        img = gzip.open(os.path.join(tmp, "gpu_stage.bam")).read()
        out["trimmed_inflated_bytes"] = len(img)
        out["ratio"] = {k: round(len(img) / v, 3) for k, v in sizes.items()}
        L = lib.load()
        L.amp_deflate_blocks_device.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        BS, stride, room = 0xFF00, 65536, 65536 - 26
        nblk = (len(img) + BS - 1) // BS
        d_in = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(dev)
        d_out = torch.empty(nblk * stride, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(nblk, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()                                # (the default stream's handle is NULL, which means the library's own stream)
        s.wait_stream(torch.cuda.current_stream())
        ks = []
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rc = L.amp_deflate_blocks_device(0, d_in.data_ptr(), len(img), BS, d_out.data_ptr(), stride, room, d_len.data_ptr(), C.c_void_p(s.cuda_stream))
            e1.record(s)
            s.synchronize()
            assert rc == 0
            if rep:
                ks.append(round(e0.elapsed_time(e1), 3))
        kmed = statistics.median(ks)
        out["kernel_ms"] = {"median": kmed, "samples": ks, "blocks": nblk, "input_GB_per_s": round(len(img) / kmed / 1e6, 2),
                            "stream_bytes": int(d_len.sum().item())}
        del d_in, d_out, d_len, img
        # ---- the whole command ----
        aio = {k: [] for k, _ in LEGS}
        log = sys.stderr
        sys.stderr = open(os.devnull, "w")                   # the commands log progress lines like the reference does
        try:
            for rep in range(args.reps + 1):
                for leg, env in LEGS:
                    _set_env(env)
                    outs = [os.path.join(tmp, "%s_%d.%s" % (leg, rep, ext)) for ext in ("bam", "vcf", "fas")]
                    t0 = time.perf_counter()
                    amplipy.main(["aio", "-i", inp, "-p", os.path.join(tmp, "p.bed"), "-r", os.path.join(tmp, "ref.fas"),
                                  "-ot", outs[0], "-ov", outs[1], "-oc", outs[2]])
                    dt = time.perf_counter() - t0
                    if rep:
                        aio[leg].append(round(dt * 1e3, 1))
                    for p in outs:
                        os.remove(p)
        finally:
            sys.stderr.close()
            sys.stderr = log
            _set_env({})
        out["aio_ms"] = {k: {"median": statistics.median(v), "samples": v} for k, v in aio.items()}
        out["aio_reads_per_s"] = {k: round(nb / (statistics.median(v) / 1e3), 1) for k, v in aio.items()}
        out["note"] = ("legs interleaved, first repetition of each dropped; host_level_default is the writer as shipped (the code path is unchanged "
                       "when the switch is off); stage = one write_rows of the whole file + close, 16 host threads")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
