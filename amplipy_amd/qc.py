"""The amplicon QC report of the command line (--qc): loaders for its inputs, the merge of the ranks'
tallies, the report as a dict, and its writers.  The numbers themselves come from the engine (lib.Engine.qc_read_tallies,
qc_depth): nothing here looks at a read."""
from __future__ import annotations

import gzip
import json
from os.path import isfile

import numpy as np

from . import abi
from .readloop import error

DEFAULT_DEPTHS = (1, 10, 100)
WHOLE = "*"                       # the name of region 0, the whole reference


def parse_depths(text):
    """'1,10,100' -> [1, 10, 100]: at most abi.QC_MAX_DEPTHS thresholds, each an integer >= 0 (and below 2^32)."""
    try:
        depths = [int(x) for x in str(text).split(",")]
    except ValueError:
        error("Invalid QC depth thresholds (comma-separated integers): %s" % text)
    if len(depths) > abi.QC_MAX_DEPTHS:
        error("At most %d QC depth thresholds: %s" % (abi.QC_MAX_DEPTHS, text))
    if any(d < 0 or d >= 2 ** 32 for d in depths):
        error("QC depth thresholds must be non-negative: %s" % text)
    return depths


def load_primer_rows(primer_fn):
    """The primer BED as [(start, end, name)] in the order load_primers sorts it: ascending (start, end), rows with the same
    interval in file order (the first of them is the one that owns positions)."""
    rows = []
    with open(primer_fn) as f:
        for l in f.read().strip().splitlines():
            parts = l.split("\t")
            rows.append((int(parts[1]), int(parts[2]), parts[3]))
    rows.sort(key=lambda r: (r[0], r[1]))
    return rows


def load_regions(regions_fn):
    """A region BED (ref, start, end[, name]) -> [(start, end, name)], half-open, as written: the engine clamps them to the
    reference, and a region that is empty after that reports zeros.  An empty file gives no region."""
    if not isfile(regions_fn):
        error("File not found: %s" % regions_fn)
    out = []
    with open(regions_fn) as f:
        for l in f.read().splitlines():
            if not l.strip():
                continue
            parts = l.split("\t")
            try:
                if len(parts) < 3:
                    raise ValueError
                s, e = int(parts[1]), int(parts[2])
                if not (-2 ** 31 <= s < 2 ** 31 and -2 ** 31 <= e < 2 ** 31):
                    raise ValueError
            except ValueError:
                error("Invalid region BED line: %s" % l)
            out.append((s, e, parts[3] if len(parts) > 3 and parts[3] else "region%d" % (len(out) + 1)))
    return out


def open_new(fn):
    """A text file for one of the report's outputs (.gz: compressed); an existing file is refused like every other output."""
    if isfile(fn):
        error("File already exists: %s" % fn)
    return gzip.open(fn, "wt") if fn.lower().endswith(".gz") else open(fn, "w")


def merge_read_tallies(parts):
    """Element-wise sum of the ranks' (tallies dict, reads_start, reads_end)."""
    parts = list(parts)
    tallies = {k: sum(int(p[0][k]) for p in parts) for k in abi.QC_READ_FIELDS}
    starts = np.sum([np.asarray(p[1], np.uint64) for p in parts], axis=0, dtype=np.uint64)
    ends = np.sum([np.asarray(p[2], np.uint64) for p in parts], axis=0, dtype=np.uint64)
    return tallies, starts, ends


def build_report(params, tallies, run_trim, primers=None, reads_start=None, reads_end=None, region_names=None, regions=None, depths=()):
    """The report as a dict, keys in the order the file has them.  primers: [(start, end, name)] with reads_start / reads_end
    from the engine (a run that trims); regions: abi.QC_REGION_DTYPE records with region_names (a run with a count table)."""
    rep = {"amplipy_qc": 1, "params": dict(params)}
    fields = abi.QC_READ_FIELDS if run_trim else ("rows", "errors", "ref_bases_in")
    rep["reads"] = {k: int(tallies[k]) for k in fields}
    if run_trim:
        rep["primers"] = [{"name": name, "start": int(s), "end": int(e), "reads_start": int(a), "reads_end": int(b)}
                          for (s, e, name), a, b in zip(primers, reads_start, reads_end)]
    if regions is not None:
        rep["regions"] = []
        for name, r in zip(region_names, regions):
            length = int(r["end"]) - int(r["start"])
            rep["regions"].append({"name": name, "start": int(r["start"]), "end": int(r["end"]), "length": length,
                                   "depth_sum": int(r["depth_sum"]), "depth_mean": int(r["depth_sum"]) / length if length else 0.0,
                                   "depth_min": int(r["depth_min"]), "depth_max": int(r["depth_max"]),
                                   "covered": {str(d): int(c) for d, c in zip(depths, r["covered"])}})
    return rep


def write_json(f, report):
    json.dump(report, f, indent=1)
    f.write("\n")


def write_depth(f, ref_id, depth):
    """One line ``ref_id <tab> pos + 1 <tab> depth`` per position, every position."""
    pos = np.arange(1, len(depth) + 1)
    f.write("".join(["%s\t%d\t%d\n" % (ref_id, p, d) for p, d in zip(pos.tolist(), np.asarray(depth).tolist())]))


def summary_line(report):
    """kept / rows, primers without a read, regions below the first threshold."""
    r = report["reads"]
    parts = ["%s of %d reads kept" % (r["kept"], r["rows"]) if "kept" in r else "%d reads" % r["rows"]]
    if "primers" in report:
        parts.append("%d of %d primers with zero reads" % (sum(1 for p in report["primers"] if p["reads_start"] + p["reads_end"] == 0),
                                                          len(report["primers"])))
    if "regions" in report and report["regions"] and report["regions"][0]["covered"]:
        first = next(iter(report["regions"][0]["covered"]))
        low = sum(1 for g in report["regions"] if g["covered"][first] < g["length"])
        parts.append("%d of %d regions below depth %s somewhere" % (low, len(report["regions"]), first))
    return "QC: " + "; ".join(parts)
