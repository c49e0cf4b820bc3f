#!/usr/bin/env python3
"""Cost of the surface models on the device (csrc/spdy_surfmodel.hip), by the method of tools/physics_step_rate.py:
HIP events, 10 warm-up calls, the median of --repeats timings of --reps calls with the range, the forms interleaved repeat by
repeat in one process.  For T30 L8 and T63 L16:

(a) spdy_surface_model_couple_dev and spdy_surface_model_forcing_dev alone, plain launches;
(b) the captured step of tests/modelstep.py with the whole physics (no shortwave): as the parent commit has it
    (caller-owned boundary arrays, no flux outputs), reading the surface model's arrays and writing hfluxn / shf / evap / ssrd,
    and the same with couple_dev as the graph's last node;
(c) a model day: 36 replays of the step with couple_dev, one spdy_surface_model_set_date and one forcing_dev, against 36 replays
    of the parent's step.

    python tools/surface_model_rate.py [--reps 100] [--repeats 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import longrun  # noqa: E402
import modelstep  # noqa: E402
import physstep  # noqa: E402
import support  # noqa: E402
import surfmodel as sm  # noqa: E402
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
from conftest import VARIANTS  # noqa: E402
from physics_step_rate import report, time_interleaved  # noqa: E402


def run(tag, reps, repeats, rows):
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    sp = support.plan(tag, 4 * kx + 4)
    case = physstep.Case(tag, sp, o)
    il, ix = sp.il, sp.ix
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    sp.physics_workspace()
    c = sm.climatology(case.phis0, longrun.latitudes(sp.table("sia_half")))
    M = s.SurfaceModel(sp, {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + (il, ix)) for k, v in c.items()}, sm.DELT)
    date = sm.Date(1982, 1, 15)
    W, D = modelstep.Workspace(sp), modelstep.device_state(case.st)
    out = sp.column_outputs(1, ("sfc", "rad"), names=("hfluxn", "shf", "evap", "ssrd"))
    F = dict(out["sfc"], **out["rad"])
    bnd, albsfc = M.boundary()
    Pp = modelstep.physics_buffers(sp, case.bnd, 0.0)                            # the parent's step: caller-owned arrays
    Pm = {"bnd": dict(bnd, albsfc=albsfc), "rad": modelstep.radiation_state(sp, 0.0)}
    step = lambda D_, P, sw, o_=None: modelstep.step(sp, D_, W, dt, physics=modelstep.whole_physics(P, sw, o_))
    torch.cuda.synchronize()
    M.set_date(date.imont1, date.tmonth, date.tyear)
    M.couple_dev(0)
    M.forcing_dev(D["qcorh"])
    step(D, Pp, True)                                  # a shortwave step first on each radiation state
    step(D, Pm, True, out)
    sp.synchronize()
    couple = lambda: M.couple_dev(1, F["hfluxn"], F["shf"], F["evap"], F["ssrd"])
    # (a)
    report(rows, VARIANTS[tag][0], kx, 1, "surface model, plain launch",
           time_interleaved({"couple_dev": couple, "forcing_dev": lambda: M.forcing_dev(D["qcorh"])}, reps, repeats))
    # (b)
    graphs = {}
    for name, P, o_, last in (("parent_step", Pp, None, False), ("step", Pm, out, False), ("step_couple", Pm, out, True)):
        Dg = {n: D[n].clone() for n in D}              # every graph steps its own copy of the state
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            step(Dg, P, False, o_)
            if last:
                couple()
        graphs[name] = g
    nodes = {n: g.num_nodes() for n, g in graphs.items()}
    print("graph nodes:", nodes, flush=True)
    report(rows, VARIANTS[tag][0], kx, 1, "captured step, whole physics", time_interleaved({n: g.launch for n, g in graphs.items()}, reps, repeats))
    # (c)

    def day_parent():
        for _ in range(sm.NSTEPS):
            graphs["parent_step"].launch()

    def day_coupled():
        M.forcing_dev(D["qcorh"])
        for _ in range(sm.NSTEPS - 1):
            graphs["step_couple"].launch()
        graphs["step"].launch()                        # the day's last step: the date changes before its couple
        M.set_date(date.imont1, date.tmonth, date.tyear)
        couple()
    report(rows, VARIANTS[tag][0], kx, 1, "model day of 36 steps", time_interleaved({"parent": day_parent, "coupled": day_coupled},
                                                                                   max(1, reps // 20), repeats))
    rows.append({"res": VARIANTS[tag][0], "kx": kx, "what": "graph nodes", **nodes})
    for g in graphs.values():
        g.close()
    M.close()
    sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []
    with torch.cuda.stream(torch.cuda.Stream()):      # the plan follows torch's stream: captures are legal, the events sit on it
        run("t30", a.reps, a.repeats, rows)
        run("t63k16", a.reps, a.repeats, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
