#!/usr/bin/env python3
"""Cost of the column physics as ONE launch (csrc/spdy_column_chain.hip, plan option "physics_fused" 1) against its five calls
(option 0), and of a whole captured time step with the whole physics in it.

(a) spdy_column_physics_dev on gridded states, plain launches, with and without shortwave: T30 L8 at nb 1 / 64, T63 L16 at nb 1 / 16.
(b) the captured step of tests/modelstep.py (inverse batch, grid tendencies, [geopotential + spdy_physics_dev], direct
    batch + spectral step): adiabatic, with the physics as five calls, with the physics in one launch.
Timing as tools/surface_rate.py: HIP events, 10 warm-up calls, the median of --repeats timings of --reps calls with the range.
The forms compared are interleaved repeat by repeat in one process, so that clock and thermal drift fall on all of them alike.

    python tools/physics_step_rate.py [--reps 100] [--repeats 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import modelstep  # noqa: E402
import moist  # noqa: E402
import physstep  # noqa: E402
import radiation  # noqa: E402
import support  # noqa: E402
import surface  # noqa: E402
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
from conftest import VARIANTS  # noqa: E402

TEND = ("utend", "vtend", "ttend", "qtend")


def time_interleaved(fns, reps, repeats):
    """fns: name -> callable.  Returns name -> (median, min, max) microseconds per call."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[n].append(a.elapsed_time(b) * 1e3 / reps)
    return {n: (float(np.median(v)), min(v), max(v)) for n, v in us.items()}


def report(rows, res, kx, nb, what, t):
    for n, (med, lo, hi) in t.items():
        rows.append({"res": res, "kx": kx, "nb": nb, "what": what, "form": n, "us": round(med, 2), "us_min": round(lo, 2),
                     "us_max": round(hi, 2)})
        print(json.dumps(rows[-1]), flush=True)


def gridded(res, kx, nbs, reps, repeats, rows):
    plans = {}
    for form, opt in (("one_launch", 1), ("five_calls", 0)):
        sp = s.Spectral(res, kx=kx, max_batch=max(nbs), device=0)
        if kx == 16:
            sp.set_sigma(synth.SIGMA_L16)
        sp.radiation_set_date(radiation.DATES[0])
        sp.set_option("physics_fused", opt)
        plans[form] = sp
    sp = plans["one_launch"]
    il, ix = sp.il, sp.ix
    tab = moist.tables(moist.HSG[kx])
    zon = radiation.zonal_columns({n: sp.table(n) for n in physstep.ZON}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    c = surface.columns(tab, il * ix, 1, zon, sqcoa)
    for p in plans.values():
        p.surface_set_orography(c["phis0"].reshape(il, ix))
        p.column_physics_workspace()
    dev = lambda a: torch.from_numpy(radiation.grids(a, 1, il, ix)).cuda()
    one = {n: dev(c[n]) for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "albsfc") + TEND + surface.BOUNDARY}
    for nb in nbs:
        d = {n: x.expand((nb,) + tuple(x.shape[1:])).contiguous() for n, x in one.items()}
        st = {f: torch.zeros(nb * sp.radiation_state_size(), dtype=torch.float64, device="cuda") for f in plans}
        tend = {f: [d[n].clone() for n in TEND] for f in plans}

        def call(f, sw):
            return lambda: plans[f].column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"],
                                                       st[f], *tend[f])
        for f in plans:
            call(f, True)()
        for sw in (True, False):
            report(rows, res, kx, nb, "column physics, %s shortwave" % ("with" if sw else "no"),
                   time_interleaved({f: call(f, sw) for f in plans}, reps, repeats))
    for p in plans.values():
        p.close()


def step(tag, reps, repeats, rows):
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    sp = support.plan(tag, 4 * kx + 4)
    case = physstep.Case(tag, sp, o)
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    sp.physics_workspace()
    W, P, D = modelstep.Workspace(sp), modelstep.physics_buffers(sp, case.bnd, 0.0), modelstep.device_state(case.st)
    modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, True))     # a shortwave step first: the radiation state is whole
    sp.synchronize()
    graphs = {}
    for name, opt, phys, sw in (("adiabatic", None, False, False), ("five_calls_sw", 0, True, True), ("five_calls", 0, True, False),
                                ("one_launch_sw", 1, True, True), ("one_launch", 1, True, False)):
        if opt is not None:
            sp.set_option("physics_fused", opt)
        # every graph steps its own copy of the state, re-armed below so that no run drifts out of range
        Dg = {n: D[n].clone() for n in D}
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            modelstep.step(sp, Dg, W, dt, physics=modelstep.whole_physics(P, sw) if phys else None)
        graphs[name] = (g, Dg)
    print("graph nodes:", {n: g.num_nodes() for n, (g, _) in graphs.items()}, flush=True)
    fns = {}
    for n, (g, Dg) in graphs.items():
        fns[n] = g.launch
        for k in Dg:          # every form starts from the same state; it then moves with each replay (reps steps per timing)
            Dg[k].copy_(D[k])
    torch.cuda.synchronize()
    t = time_interleaved(fns, reps, repeats)
    report(rows, VARIANTS[tag][0], kx, 1, "captured step", t)
    for g, _ in graphs.values():
        g.close()
    sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []
    gridded("t30", 8, [1, 64], a.reps, a.repeats, rows)
    gridded("t63", 16, [1, 16], a.reps, a.repeats, rows)
    with torch.cuda.stream(torch.cuda.Stream()):      # the plan follows torch's stream: captures are legal, the events sit on it
        step("t30", a.reps, a.repeats, rows)
        step("t63k16", a.reps, a.repeats, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
