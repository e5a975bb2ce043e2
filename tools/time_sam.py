"""Timing of the opt-in device codec for SAM text (AMPLIPY_GPU_SAM=1) -> profiles/gpu_sam.json.

  python tools/time_sam.py [--reads N] [--reps R] [--out profiles/gpu_sam.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_sam.py --kernels-only     (a run of its own for the kernel times)
  python tools/time_sam.py --merge-kernel-stats DIR/.../kernel_stats.csv --out profiles/gpu_sam.json

Legs: ``aio`` (SAM in; SAM, VCF and FASTA out) and ``variants`` (the trimmed SAM in, VCF out) on one synthetic file, switch on
and switch off interleaved in one process, the first repetition of each dropped, all samples kept.  Switch off is the code as it
was before the codec existed (the path is not entered): the baseline.  Then the stages of the on leg alone (HIP events around
the copies and kernels, wall clock around the file reads and writes), a three-point sweep of the chunk size, and for context
the same records as a BAM file through the native BAM path."""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from amplipy_amd import amplipy, bamio, lib, sam_native, synth  # noqa: E402

HBM_BYTES_PER_S = 8e12            # MI355X peak HBM bandwidth
LINK_BYTES_PER_S = 63e9           # the host link's specification (PCIe 5.0 x16, one direction)


def make_files(d, n_reads, seed=1):
    g = synth.make_genome()
    primers, amps = synth.make_artic_scheme()
    ref = os.path.join(d, "ref.fas"); open(ref, "w").write(">SYN_REF\n" + synth.genome_string(g) + "\n")
    bed = os.path.join(d, "p.bed"); open(bed, "w").write("".join("SYN_REF\t%d\t%d\tp%d\n" % (s, e, i) for i, (s, e, _) in enumerate(primers)))
    hdr = bamio.Header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:SYN_REF\tLN:%d\n@PG\tID:sim\tPN:sim\n" % g.size, [("SYN_REF", g.size)])
    batch = synth.make_amplicon_batch(g, amps, n_reads, seed=seed)
    sam, bam = os.path.join(d, "in.sam"), os.path.join(d, "in.bam")
    ws, wb = bamio.AlignmentWriter(sam, "w", hdr), bamio.AlignmentWriter(bam, "wb", hdr)
    for i in range(batch.n):
        s = batch.segment(i)
        r = bamio.Rec("read%d" % i, s.flag, 0, s.reference_start, 60, s.cigartuples, 0, s.reference_start, s.template_length, s.query_sequence,
                      bytes(s.query_qualities), aux_sam=["NM:i:1", "AS:i:290"])
        ws.write(r); wb.write(r)
    ws.close(); wb.close()
    return g, primers, ref, bed, sam, bam


def quiet(fn, *a, **kw):
    err = sys.stderr
    sys.stderr = io.StringIO()
    try:
        return fn(*a, **kw)
    finally:
        sys.stderr = err


def aio(inp, d, ref, bed, tag, on, ext="sam"):
    outs = [os.path.join(d, "%s_%s" % (tag, x)) for x in ("t." + ext, "v.vcf", "c.fas")]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    t0 = time.perf_counter()
    quiet(amplipy.run_amplipy, untrimmed_reads_fn=inp, primer_fn=bed, reference_fn=ref, trimmed_reads_fn=outs[0], variants_fn=outs[1], consensus_fn=outs[2],
          primer_pos_offset=0, min_length=30, min_quality=20, sliding_window_width=4, min_freq_consensus=0.5, min_freq_variants=0.03, min_depth_consensus=10,
          min_depth_variants=1, unknown_symbol="N", include_no_primer=False, run_trim=True, run_variants=True, run_consensus=True, gpu_sam=on)
    return (time.perf_counter() - t0) * 1e3, outs


def variants(inp, d, ref, tag, on):
    out = os.path.join(d, "%s_var.vcf" % tag)
    if os.path.exists(out):
        os.remove(out)
    t0 = time.perf_counter()
    quiet(amplipy.run_amplipy, trimmed_reads_fn=inp, reference_fn=ref, variants_fn=out, min_quality=20, min_freq_variants=0.03, min_depth_variants=1,
          run_variants=True, gpu_sam=on)
    return (time.perf_counter() - t0) * 1e3, out


def med(samples):
    return {"median": round(statistics.median(samples), 2), "samples": [round(x, 2) for x in samples]}


def stages(sam, g, primers, chunk_bytes, d):
    """The on leg's stages alone, summed over the chunks of the file: ms."""
    pr = [(s, e) for s, e, _ in primers]
    mn, mx, mpl = lib.find_overlapping_primers(g.size, pr, 0)
    eng = lib.Engine(g.size); eng.set_primers(mn, mx, mpl); eng.set_params(20, 4, True, True)
    codec = sam_native.SamCodec(eng); codec.set_references(["SYN_REF"])
    out = {k: 0.0 for k in ("read", "copy_up", "scan_ranks", "lines_tabs", "records_rows", "pack", "read_pass", "format_kernels", "copy_down", "write",
                            "parse_call_wall", "process_call_wall", "format_call_wall")}
    acc = {"text_bytes": 0, "seq_qual_text_bytes": 0, "packed_bytes": 0, "out_bytes": 0, "chunks": 0}
    for rep in range(2):                      # the first pass grows the buffers; the second is the one reported
        for k in out:
            out[k] = 0.0
        for k in acc:
            acc[k] = 0
        codec.stage_ms(on=True, read=False)
        src = sam_native.SamTextInput(sam, chunk_bytes)
        it = src._chunks()
        f = open(os.path.join(d, "stages_out.sam"), "wb")
        read_base = 0
        while True:
            t0 = time.perf_counter()
            chunk = next(it, None)
            out["read"] += (time.perf_counter() - t0) * 1e3
            if chunk is None:
                break
            t0 = time.perf_counter(); info = codec.parse(chunk); t1 = time.perf_counter()
            codec.process(0); t2 = time.perf_counter()
            text, _ = codec.format(30, False); t3 = time.perf_counter()
            f.write(text); t4 = time.perf_counter()
            ms = codec.stage_ms(on=True)
            for name, k in (("copy_up", 0), ("scan_ranks", 1), ("lines_tabs", 2), ("records_rows", 3), ("pack", 4), ("read_pass", 6), ("format_kernels", 8), ("copy_down", 9)):
                out[name] += ms[k]
            out["parse_call_wall"] += (t1 - t0) * 1e3; out["process_call_wall"] += (t2 - t1) * 1e3; out["format_call_wall"] += (t3 - t2) * 1e3
            out["write"] += (t4 - t3) * 1e3
            acc["text_bytes"] += len(chunk); acc["seq_qual_text_bytes"] += 2 * int(info.n_bases)
            acc["packed_bytes"] += int(info.n_bases_padded) * 3 // 2; acc["out_bytes"] += len(text); acc["chunks"] += 1
            read_base += int(info.n_rows)
            eng.aggregate_events(dev_reads=codec.dev_reads(), read_base=0, drain=True)
        f.close(); src.close()
    codec.close(); eng.close()
    res = {"chunk_bytes": chunk_bytes, "ms": {k: round(v, 3) for k, v in out.items()}, **acc}
    pk, fm = out["pack"] / 1e3, out["format_kernels"] / 1e3
    res["pack_text_bytes_per_s"] = round(acc["seq_qual_text_bytes"] / pk) if pk > 0 else None
    res["format_out_bytes_per_s"] = round(acc["out_bytes"] / fm) if fm > 0 else None
    res["copy_up_bytes_per_s"] = round(acc["text_bytes"] / (out["copy_up"] / 1e3)) if out["copy_up"] > 0 else None
    res["copy_down_bytes_per_s"] = round(acc["out_bytes"] / (out["copy_down"] / 1e3)) if out["copy_down"] > 0 else None
    res["of_hbm_peak"] = {"pack": res["pack_text_bytes_per_s"] and round(res["pack_text_bytes_per_s"] / HBM_BYTES_PER_S, 4),
                          "format": res["format_out_bytes_per_s"] and round(res["format_out_bytes_per_s"] / HBM_BYTES_PER_S, 4)}
    res["of_link_spec"] = {"copy_up": res["copy_up_bytes_per_s"] and round(res["copy_up_bytes_per_s"] / LINK_BYTES_PER_S, 3),
                           "copy_down": res["copy_down_bytes_per_s"] and round(res["copy_down_bytes_per_s"] / LINK_BYTES_PER_S, 3)}
    return res


def merge_kernel_stats(path, out):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_sam_" in name or "DeviceScan" in name or "scan" in name.lower() and "rocprim" in name:
                rows.append({k: r[k] for k in r if k in ("Name", "KernelName", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs")})
    res = json.load(open(out))
    res["rocprofv3_kernel_stats"] = {"note": "a run of its own (rocprofv3 --kernel-trace --stats -- python tools/time_sam.py --kernels-only): one aio on the same file, switch on",
                                     "kernels": rows}
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_sam.json"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-kernel-stats")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)
    sys.argv = ["amplipy_amd", "time_sam"]
    os.environ.pop("AMPLIPY_GPU_SAM", None)
    with tempfile.TemporaryDirectory() as d:
        g, primers, ref, bed, sam, bam = make_files(d, a.reads)
        if a.kernels_only:
            aio(sam, d, ref, bed, "warm", True)
            ms, _ = aio(sam, d, ref, bed, "prof", True)
            print("aio, switch on: %.1f ms" % ms)
            return
        res = {"metric": "gpu_sam", "records": a.reads, "sam_bytes": os.path.getsize(sam), "bam_bytes": os.path.getsize(bam), "reps": a.reps,
               "default_chunk_bytes": sam_native.CHUNK_BYTES}
        legs = {"aio_off": [], "aio_on": [], "variants_off": [], "variants_on": [], "aio_bam_native": []}
        trimmed = None
        for rep in range(a.reps):
            for on in (False, True):
                ms, outs = aio(sam, d, ref, bed, "on" if on else "off", on)
                legs["aio_on" if on else "aio_off"].append(ms)
                trimmed = outs[0] if not on else trimmed
            same = all(open(os.path.join(d, "on_" + x), "rb").read() == open(os.path.join(d, "off_" + x), "rb").read() for x in ("t.sam", "v.vcf", "c.fas"))
            assert same, "switch on and switch off wrote different files"
            for on in (False, True):
                ms, _ = variants(trimmed, d, ref, "on" if on else "off", on)
                legs["variants_on" if on else "variants_off"].append(ms)
            assert open(os.path.join(d, "on_var.vcf"), "rb").read() == open(os.path.join(d, "off_var.vcf"), "rb").read()
            ms, _ = aio(bam, d, ref, bed, "bam", False, ext="bam")
            legs["aio_bam_native"].append(ms)
        res["device_chunks_python_chunks_of_last_on_run"] = [sam_native.LAST_RUN_STATS["device_chunks"], sam_native.LAST_RUN_STATS["python_chunks"]]
        res["legs_ms"] = {k: med(v[1:]) for k, v in legs.items()}
        res["records_per_s"] = {k: round(a.reads / (res["legs_ms"][k]["median"] / 1e3)) for k in legs}
        res["speedup_on_over_off"] = {k: round(res["legs_ms"][k + "_off"]["median"] / res["legs_ms"][k + "_on"]["median"], 2) for k in ("aio", "variants")}
        sweep = {}
        for cb in (4 << 20, 16 << 20, 64 << 20):
            os.environ["AMPLIPY_SAM_CHUNK_BYTES"] = str(cb)
            sweep[str(cb)] = med([aio(sam, d, ref, bed, "sweep", True)[0] for _ in range(4)][1:])
        os.environ.pop("AMPLIPY_SAM_CHUNK_BYTES", None)
        res["aio_on_ms_by_chunk_bytes"] = sweep
        res["stages_on_leg"] = stages(sam, g, primers, sam_native.CHUNK_BYTES, d)
        res["note"] = ("legs interleaved in one process, first repetition of each dropped; switch off runs the code as it was before the codec (the path is "
                       "not entered): the baseline; aio_bam_native = the same records as a BAM file through libampbam (BAM in, BAM out), for context; stages: "
                       "HIP events on the ctx stream summed over the chunks (second pass over the file), read / write / *_call_wall by the wall clock; "
                       "pack_text_bytes_per_s = SEQ and QUAL text bytes over the pack kernel's time, format_out_bytes_per_s = output bytes over the format "
                       "kernels' time; HBM peak 8 TB/s, host link 63 GB/s by its specification")
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({k: res[k] for k in ("records", "sam_bytes", "records_per_s", "speedup_on_over_off", "aio_on_ms_by_chunk_bytes")}))
        print(json.dumps(res["stages_on_leg"]))


if __name__ == "__main__":
    main()
