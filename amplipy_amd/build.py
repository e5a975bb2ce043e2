"""In-tree build of libamplihip.so with hipcc for gfx950 (cross-compiles without a GPU) and of the
host-side BAM codec libampbam.so (g++, zlib)."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# translation units of libamplihip.so: the C ABI with the context, the calling kernels and the small ones; the read pass (every
# kernel that trims and counts reads, and launch_reads: most of the compile time, and a unit of its own so that an edit of the
# host code beside it compiles none of them); the insertion-event aggregation (its sort headers triple the compile time of
# whatever includes them, so it is built -- and cached -- on its own), the DEFLATE encoder of the BAM writer, and
# the codecs for SAM text and for BAM (input, and trimmed records out), the QC report, the strand tallies, the per-amplicon counts, and
# the codon tallies, the deletion events, the insertion evidence, the co-occurrence tallies, the error profile, the read haplotypes, the read-position tallies
UNITS = ["amplihip.hip", "amp_readpass.hip", "amp_ins.hip", "amp_deflate.hip", "amp_sam.hip", "amp_bgzf.hip", "amp_qc.hip", "amp_strand.hip", "amp_amplicon.hip",
         "amp_codon.hip", "amp_del.hip", "amp_insev.hip", "amp_cooc.hip", "amp_errprof.hip", "amp_hap.hip", "amp_readpos.hip"]
HEADERS = [os.path.join(_HERE, "..", "include", "amplihip.h")] + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp"))
# what a unit includes, as `hipcc -MM` reports it (tests/test_build_deps.py holds every list to that): a unit is recompiled
# when one of these is newer than its object.  amp_ctx.hpp (the context) is private to the first two.
UNIT_DEPS = {"amplihip.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in
                              ("amp_ctx.hpp", "amp_read.hpp", "amp_plan.hpp", "amp_hook.hpp", "amp_call.hpp", "amp_ins.hpp", "amp_codec.hpp")],
             "amp_readpass.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in
                                  ("amp_ctx.hpp", "amp_read.hpp", "amp_plan.hpp", "amp_hook.hpp", "amp_tile.hpp", "amp_bf.hpp", "amp_fast.hpp",
                                   "amp_fast5.hpp", "amp_fast6.hpp", "amp_fast7.hpp", "amp_wave.hpp", "amp_heavy.hpp")],
             "amp_ins.hip": [os.path.join(_HERE, "..", "include", "amplihip.h"), os.path.join(CSRC, "amp_ins.hpp")],
             "amp_deflate.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")],
             # (amp_hook.hpp: the host shell the ten hooks behind the read pass share; amp_tally.hpp: the device skeleton of the four
             # windowed tally kernels, and the whole loop of k_strand and k_readpos; amp_keyed.hpp: the keyed table of del, insev and hap)
             # (amp_clip.hpp: the clip sites of the QC report; amp_tally.hpp for the wave combine its kernel shares with the tally kernels)
             "amp_qc.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_qc.hpp", "amp_clip.hpp", "amp_strand.hpp", "amp_tally.hpp")],
             "amp_strand.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_tally.hpp")],
             "amp_amplicon.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_amplicon.hpp", "amp_tally.hpp")],
             "amp_codon.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_codon.hpp", "amp_tally.hpp")],
             "amp_del.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_del.hpp", "amp_keyed.hpp", "amp_tally.hpp")],
             # (the insertion evidence: it reads the event list -- amp_ins.hpp -- and takes rp_bin from amp_readpos.hpp)
             "amp_insev.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_insev.hpp", "amp_keyed.hpp", "amp_ins.hpp", "amp_readpos.hpp", "amp_tally.hpp")],
             "amp_cooc.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_cooc.hpp", "amp_tally.hpp")],
             "amp_errprof.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_errprof.hpp", "amp_tally.hpp")],
             "amp_hap.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_hap.hpp", "amp_keyed.hpp", "amp_tally.hpp")],
             "amp_readpos.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in ("amp_hook.hpp", "amp_strand.hpp", "amp_readpos.hpp", "amp_tally.hpp")],
             "amp_sam.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in
                             ("amp_codec.hpp", "amp_bgzf.hpp", "amp_bamout.hpp", "amp_bamtail.hpp")],
             # (amp_bamout.hip, the re-encoder of trimmed records, and amp_bamtext.hip, trimmed records as SAM text, are part of
             # amp_bgzf.hip's unit: they are included there)
             "amp_bgzf.hip": [os.path.join(_HERE, "..", "include", "amplihip.h")] + [os.path.join(CSRC, f) for f in
                              ("amp_codec.hpp", "amp_bgzf.hpp", "amp_bamout.hpp", "amp_bamtail.hpp", "amp_bamout.hip", "amp_bamtext.hpp", "amp_bamtext.hip")]}
DEPS = [os.path.join(CSRC, u) for u in UNITS] + [os.path.join(CSRC, f) for f in ("amp_bamout.hip", "amp_bamtext.hip")] + HEADERS
OUT = os.path.join(_HERE, "libamplihip.so")
OBJ_DIR = os.path.join(_HERE, "build")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]


def needs_build():
    if not os.path.isfile(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force=False, verbose=False, extra_flags=()):
    if not force and not needs_build():
        return OUT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = []
    for u in UNITS:
        src = os.path.join(CSRC, u)
        obj = os.path.join(OBJ_DIR, u.replace(".hip", ".o"))
        stale = force or extra_flags or not os.path.isfile(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in [src] + UNIT_DEPS[u])
        if stale:
            cmd = [hipcc] + FLAGS + list(extra_flags) + ["-c", "-o", obj, src]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", OUT] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return OUT


BAM_SRC = os.path.join(_HERE, "csrc", "ampbam.cpp")
BAM_DEPS = [BAM_SRC, os.path.join(_HERE, "csrc", "amp_inflate.hpp"), os.path.join(_HERE, "..", "include", "ampbam.h")]
BAM_OUT = os.path.join(_HERE, "libampbam.so")


def build_bam(force=False, verbose=False):
    if not force and os.path.isfile(BAM_OUT) and all(os.path.getmtime(d) <= os.path.getmtime(BAM_OUT) for d in BAM_DEPS):
        return BAM_OUT
    cmd = [shutil.which("g++") or "g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", BAM_OUT, BAM_SRC, "-lz", "-ldl", "-pthread"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return BAM_OUT


if __name__ == "__main__":
    build(force=True, verbose=True)
    build_bam(force=True, verbose=True)
