"""All nine kernels behind the read pass in one leg, for a comparison of two builds of the library: the workloads of
tools/time_hooks.py (strand, amplicon, codon), time_qc.py, time_del.py, time_cooc.py and time_hap.py (their per-amplicon lists),
time_errprof.py and time_readpos.py, each hook on alone on time_hooks.Setup's engine and batch, 20 launches after 5 warm-up
launches, medians; and a hash over every table the hook returns after its last launch.  With --parent-lib the two builds take
turns, a fresh process each; a figure of this build is `within` when its median over the rounds is at most the parent's median
plus the parent's own spread (max - min) over its rounds.

  python tools/time_hook_tables.py [--parent-lib PATH/libamplihip.so] [--rounds 5] [--out profiles/hook_tables.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_hooks
from tools.time_cooc import two_site_sets

HOOKS = ("qc", "strand", "amplicon", "codon", "del", "cooc", "errprof", "hap", "readpos")
REGION = 100


def digest(tables):
    import numpy as np
    m = hashlib.sha256()
    for t in tables:
        m.update(np.ascontiguousarray(t).tobytes())
    return m.hexdigest()[:16]


def leg():
    import numpy as np
    from amplipy_amd import amplicon, synth
    s = time_hooks.Setup()
    e, G, med = s.eng, s.G, statistics.median
    ref_seq = synth.genome_string(synth.make_genome())
    hap_starts = np.array(sorted(int(a[2]) + 20 for a in s.amps if int(a[2]) + 20 + REGION <= G), np.int32)
    life = {"qc": (lambda: e.qc_enable(sorted((a, b) for a, b, _ in s.primers), 0, 30, False, [(0, G)], [1, 10, 100]), e.qc_disable,
                   lambda: [np.array(list(e.qc_read_tallies()[0].values()), np.uint64)] + list(e.qc_read_tallies()[1:])),
            "strand": (e.strand_enable, e.strand_disable, e.strand_tables),
            "amplicon": (lambda: amplicon.enable(e, s.amplicon_set()), e.amplicon_disable, e.amplicon_tables),
            "codon": (lambda: e.codon_enable(np.arange(0, G - 2, 3, dtype=np.int32)), e.codon_disable, e.codon_tables),
            "del": (e.del_enable, e.del_disable, lambda: [e.del_events()[0]]),
            "cooc": (lambda: e.cooc_enable(*two_site_sets([int(a[2]) + 60 for a in s.amps], G)), e.cooc_disable, e.cooc_tables),
            "errprof": (lambda: e.errprof_enable(ref_seq), e.errprof_disable, e.errprof_tables),
            "hap": (lambda: e.hap_enable(hap_starts, hap_starts + REGION, ref_seq), e.hap_disable, lambda: [t for k, t in enumerate(e.hap_tables()) if k != 1]),
            "readpos": (e.readpos_enable, e.readpos_disable, lambda: [e.readpos_tables()])}
    res = {"reads": s.n, "pass_off_ms": med(s.launches()[0])}
    for h in HOOKS:
        on, off, tables = life[h]
        on()
        res[h + "_ms"] = med(s.launches(getattr(e, h + "_last_ms"))[1])
        res[h + "_tables"] = digest(tables())
        off()
    e.close()
    print("LEG " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib", help="libamplihip.so of the parent commit: timed in turn with this build")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hook_tables.json"))
    a = ap.parse_args()
    if a.leg:
        return leg()
    res = {"batch": time_hooks.BATCH, "launches_per_figure": time_hooks.LAUNCHES, "rounds": {"parent": [], "this": []}}
    for k in range(a.rounds):                 # the builds take turns, a process each
        if a.parent_lib:
            res["rounds"]["parent"].append(time_hooks.child(__file__, ["--leg"], a.parent_lib))
        res["rounds"]["this"].append(time_hooks.child(__file__, ["--leg"]))
    legs = res["rounds"]["parent"] + res["rounds"]["this"]
    for key in ("pass_off_ms",) + tuple(h + "_ms" for h in HOOKS):
        row = {who: {"median": statistics.median(v), "min": min(v), "max": max(v)} for who, v in ((w, [r[key] for r in rs]) for w, rs in res["rounds"].items()) if v}
        if "parent" in row:
            p = row["parent"]
            row["spread_percent"] = round(100 * (p["max"] - p["min"]) / p["median"], 2)
            row["within"] = row["this"]["median"] <= p["median"] + (p["max"] - p["min"])
        res[key] = row
    res["tables_identical"] = {h: len({r[h + "_tables"] for r in legs}) == 1 for h in HOOKS}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
