#!/usr/bin/env python3
"""Cost of check_diagnostics on the device (csrc/spdy_diagnostics.hip), by the method of
tools/physics_step_rate.py: HIP events, 10 warm-up calls, the median of --repeats timings of --reps replays with the range, the
forms interleaved repeat by repeat in one process.  For T30 L8 and T63 L16: the captured adiabatic step of tests/modelstep.py
(form "composite") as it is, the same with spdy_diagnostics_check_dev on time level 2 as the graph's last node, and the captured
check alone.  The yardstick is the step WITHOUT the node: --without-guard times that arm alone and needs nothing of the
diagnostics, so the same file runs on the parent commit.

    python tools/diagnostics_cost.py [--reps 1000] [--repeats 5] [--without-guard] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import dynstep  # noqa: E402
import modelstep  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
import support  # noqa: E402
from conftest import VARIANTS  # noqa: E402
from physics_step_rate import report, time_interleaved  # noqa: E402


def run(tag, reps, repeats, rows, guard):
    kx = VARIANTS[tag][3]
    sp = support.plan(tag, 4 * kx + 4)
    dt = 2400.0 if tag == "t30" else 1200.0
    sp.initialize_implicit(dt)
    st = dynstep.state(sp, 8000)
    for n in ("vor", "div", "t", "tr", "ps"):          # replayed thousands of times without physics: a state that does not move
        st[n] = st[n] * (1e-6 if n != "t" else 1.0)
    st["t"][:, :, 1:, :] = 0.0
    st["t"][:, :, 0, 1:] = 0.0
    d = s.Diagnostics(sp, capacity=64) if guard else None
    graphs = {}
    for name in ("step", "step_check", "check") if guard else ("step",):
        D, W = modelstep.device_state(st), modelstep.Workspace(sp)
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            if name != "check":
                modelstep.step(sp, D, W, dt, form="composite")
            if name != "step":
                d.check_dev(D["vor"][1], D["div"][1], D["t"][1])
        graphs[name] = (g, D, W)
    nodes = {n: g.num_nodes() for n, (g, _, _) in graphs.items()}
    print("graph nodes:", nodes, flush=True)
    t = time_interleaved({n: g.launch for n, (g, _, _) in graphs.items()}, reps, repeats)
    report(rows, VARIANTS[tag][0], kx, 1, "captured adiabatic step", t)
    if guard:
        extra = t["step_check"][0] - t["step"][0]
        rows.append({"res": VARIANTS[tag][0], "kx": kx, "what": "check_dev as the last node", "extra_us": round(extra, 2),
                     "alone_us": round(t["check"][0], 2), **{"nodes_" + n: v for n, v in nodes.items()}})
        print(json.dumps(rows[-1]), flush=True)
        print("status after the run:", {k: v for k, v in d.status().items() if k != "bad_row"}, flush=True)
        d.close()
    for g, _, _ in graphs.values():
        g.close()
    sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--without-guard", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []
    with torch.cuda.stream(torch.cuda.Stream()):      # the plan follows torch's stream: captures are legal, the events sit on it
        for tag in ("t30", "t63k16"):
            run(tag, a.reps, a.repeats, rows, not a.without_guard)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
