#!/usr/bin/env python3
"""GPU box: rate of the HOST-pointer drop-in path (PCIe copies + sync included), for DESIGN.md.

    python tools/host_path_rate.py                                   T30, nb = 1 .. 6144, printed
    python tools/host_path_rate.py --res t30,t63 --sizes 1,8,48 --op-sizes 8 --repeats 2 --label this --json runs.jsonl
    python tools/host_path_rate.py --summarise runs.jsonl --json profiles/host_call_parent_vs_this.json

Rows: grid_to_spec + spec_to_grid host-form round trips of nb fields (--sizes), and uvspec then vds of nb spectra (--op-sizes), on
the default route settings; the rate is fields through the pair of calls per second, over a window of about --seconds (first
calls warm the shape up and size the window).  --json appends one line per process, so that
two libraries ($SPDY_LIB) can be run in alternating processes into one file; --summarise turns such a file into the median and the
range of every row per label, and says for every row whether the label "this" has its median within or above the range of "parent"."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
RESOLUTIONS = {"t30": (30, 96, 48), "t63": (63, 192, 96)}   # trunc, ix, il


def measure(a):
    import numpy as np, synth, speedy_f90_amd as s
    sizes, ops = [int(x) for x in a.sizes.split(",") if x], [int(x) for x in a.op_sizes.split(",") if x]
    rows = {}
    for res in a.res.split(","):
        trunc, ix, il = RESOLUTIONS[res]
        sp = s.Spectral(res, kx=8, max_batch=max(sizes + ops), device=0)
        for kind, nb in [("transforms", n) for n in sizes] + [("operators", n) for n in ops]:
            G = synth.grids(min(nb, 64), ix, il); G = np.tile(G, ((nb + 63) // 64, 1, 1))[:nb].copy()
            S = sp.grid_to_spec(G)
            pair = (lambda: sp.spec_to_grid(sp.grid_to_spec(G), 1)) if kind == "transforms" else (lambda: sp.vds(*sp.uvspec(S, S)))
            t0 = time.perf_counter()
            for _ in range(3):
                pair()
            reps = max(3, int(a.seconds / ((time.perf_counter() - t0) / 3)))      # a window of about a.seconds
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(reps):
                    pair()
                dt = time.perf_counter() - t0
                rows.setdefault("%s %s nb=%d" % (res, kind, nb), []).append(nb * reps / dt)
                print("host-pointer path  %s %-10s nb=%5d : %10.0f round trips/s  (%.1f us per call pair)"
                      % (res, kind, nb, nb * reps / dt, dt / reps * 1e6), flush=True)
        sp.close()
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps({"label": a.label, "library": s.LIB_PATH, "rates": rows}) + "\n")


def summarise(a):
    arms = {}
    with open(a.summarise) as f:
        for line in f:
            run = json.loads(line)
            for row, rates in run["rates"].items():
                arms.setdefault(run["label"], {}).setdefault(row, []).extend(rates)
    out = {"unit": "fields through the pair of calls per second", "rows": {}}
    for row in arms[next(iter(arms))]:
        out["rows"][row] = {label: {"median": statistics.median(r[row]), "min": min(r[row]), "max": max(r[row]), "samples": len(r[row])}
                            for label, r in arms.items()}
        if "parent" in arms and "this" in arms:
            out["rows"][row]["this_median_within_or_above_parent_range"] = out["rows"][row]["this"]["median"] >= out["rows"][row]["parent"]["min"]
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="t30")
    ap.add_argument("--sizes", default="1,8,48,512,6144")
    ap.add_argument("--op-sizes", default="")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--label", default="this")
    ap.add_argument("--json")
    ap.add_argument("--summarise", metavar="RUNS")
    args = ap.parse_args()
    summarise(args) if args.summarise else measure(args)
