#!/usr/bin/env python3
"""Rate of the moist-physics column kernel (spdy_moist_columns_dev, csrc/spdy_physics.hip) at T30 L8 and T63 L16 over nb states,
timed with HIP events on the plan's stream, against the byte model of DESIGN.md (per column: reads 5 kx + 1 doubles -- tg, qg,
phig, ttend, qtend and pslg -- writes 5 kx + 3 doubles and 2 ints with every optional output requested), and the extra time of a
captured model step with the block in it (geopotential + inverse launch + column kernel) over the adiabatic step.

    python tools/moist_rate.py [--reps 200] [--json out.json]"""
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
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
from dynstep import state as dyn_state  # noqa: E402

HBM = 8.0e12


def bytes_per_state(kx, ncol):
    return ncol * ((5 * kx + 1 + 5 * kx + 3) * 8 + 2 * 4)


def time_fn(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps      # us


def kernel_rates(res, kx, nbs, reps):
    sp = s.Spectral(res, kx=kx, max_batch=max(nbs), device=0)
    if kx == 16:
        sp.set_sigma(synth.SIGMA_L16)
    il, ix = sp.il, sp.ix
    tab = moist.tables(moist.HSG[kx])
    one = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in moist.grid_inputs(tab, (1, il, ix), 1)]
    rows = []
    for nb in nbs:
        tg, qg, phig, pslg, tt, qt = [x.expand((nb,) + tuple(x.shape[1:])).contiguous() for x in one]
        out = sp.column_outputs(nb, "moist")
        us = time_fn(lambda: sp.moist_columns_dev(tg, qg, phig, pslg, tt, qt, out), reps)
        bw = bytes_per_state(kx, il * ix) * nb / (us * 1e-6)
        rows.append({"res": res, "kx": kx, "nb": nb, "us": round(us, 2), "bytes": bytes_per_state(kx, il * ix) * nb,
                     "TB_s": round(bw / 1e12, 3), "frac_8TBs": round(bw / HBM, 3)})
        print(json.dumps(rows[-1]), flush=True)
    sp.close()
    return rows


def step_extra(res, kx, reps):
    sp = s.Spectral(res, kx=kx, max_batch=4 * kx + 4, device=0)
    if kx == 16:
        sp.set_sigma(synth.SIGMA_L16)
    dt = 2400.0
    sp.initialize_implicit(dt)
    D, W = modelstep.device_state(dyn_state(sp, 8000)), modelstep.Workspace(sp)
    sp.moist_workspace()
    sp.use_own_stream()
    res_ = {}
    for physics in (False, True):
        with sp.graph_capture() as g:
            modelstep.step(sp, D, W, dt, physics=modelstep.moist_physics() if physics else None)
        # the state evolves under replay; a few hundred adiabatic / moist steps stay finite at these amplitudes
        res_["with" if physics else "without"] = {"us": round(time_fn(g.launch, reps), 2), "nodes": g.num_nodes()}
        g.close()
    res_["extra_us"] = round(res_["with"]["us"] - res_["without"]["us"], 2)
    row = {"res": res, "kx": kx, "captured_step": res_}
    print(json.dumps(row), flush=True)
    sp.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"kernel": kernel_rates("t30", 8, [1, 16, 64, 256, 512], a.reps) + kernel_rates("t63", 16, [1, 16, 64], a.reps),
           "step": [step_extra("t30", 8, a.reps), step_extra("t63", 16, a.reps)]}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
