#!/usr/bin/env python3
"""Cost of SPPT on the device: the pattern's advance alone (captured: noise + AR(1), inverse transform, clip) and
the captured time step of tests/modelstep.py with the whole physics, without SPPT (spdy_physics_dev: the path as it was) and
with it ({advance; spdy_physics_sppt_dev}), the physics as five calls and in one launch; T30 L8 and T63 L16, no shortwave.
Timing as tools/physics_step_rate.py: HIP events, 10 warm-up calls, the median of --repeats timings of --reps calls with the
range, the forms interleaved repeat by repeat in one process.

    python tools/sppt_rate.py [--reps 100] [--repeats 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import modelstep  # noqa: E402
import physstep  # noqa: E402
import support  # noqa: E402
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
from conftest import VARIANTS  # noqa: E402
from physics_step_rate import report, time_interleaved  # noqa: E402


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
    sp.physics_sppt_workspace()
    W, P, D = modelstep.Workspace(sp), modelstep.physics_buffers(sp, case.bnd, 0.0), modelstep.device_state(case.st)
    pat = s.Sppt(sp, 36, np.clip(np.linspace(-0.5, 1.5, kx), 0.0, 1.0), seed=1)
    modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, True))     # a shortwave step first: the radiation state is whole
    sp.synchronize()
    graphs = {}
    with sp.graph_capture() as g:
        pat.advance_dev()
    graphs["advance"] = (g, {})
    for name, opt, sppt in (("five_calls", 0, False), ("five_calls_sppt", 0, True), ("one_launch", 1, False), ("one_launch_sppt", 1, True)):
        sp.set_option("physics_fused", opt)
        Dg = {n: D[n].clone() for n in D}           # every graph steps its own copy of the state
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            modelstep.step(sp, Dg, W, dt, physics=modelstep.sppt_physics(P, False, pat) if sppt else modelstep.whole_physics(P, False))
        graphs[name] = (g, Dg)
    print("graph nodes:", {n: g.num_nodes() for n, (g, _) in graphs.items()}, flush=True)
    torch.cuda.synchronize()
    t = time_interleaved({n: g.launch for n, (g, _) in graphs.items()}, reps, repeats)
    report(rows, VARIANTS[tag][0], kx, 1, "captured step", t)
    print("draws:", pat.draws(), flush=True)
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
    with torch.cuda.stream(torch.cuda.Stream()):      # the plan follows torch's stream: captures are legal, the events sit on it
        step("t30", a.reps, a.repeats, rows)
        step("t63k16", a.reps, a.repeats, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
