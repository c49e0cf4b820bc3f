#!/usr/bin/env python3
"""Rate of the surface-flux and boundary-layer kernels (spdy_surface_fluxes_dev / spdy_pbl_dev, csrc/spdy_surface.hip) and of the
whole column-physics chain (spdy_column_physics_dev, plain and captured, with and without shortwave) at T30 L8 over nb = 1, 64,
512 states and T63 L16 over nb = 1, 16, 64, timed with HIP events on the plan's stream, against the byte model of DESIGN.md §12.
Per column, in doubles (icnv is an int), required outputs only (what the chain asks for):
  surface_fluxes_kernel  reads 6 level values + 3 + 7 boundary + 2 plan fields = 18   writes 6                    (24)
  pbl_kernel             reads 6 kx + 7.5 (se rh qsat phig ttend qtend; qg(kx), pslg, icnv, 4 fluxes, utend(kx), vtend(kx))
                         writes 2 kx + 2                                                                           (8 kx + 9.5)
The chain's bytes are the sum of its five calls' models (tools/moist_rate.py, tools/radiation_rate.py with no optional output but
the intermediates the next call reads).  Each figure is the median of --repeats timings of --reps calls, with the range.

    python tools/surface_rate.py [--reps 100] [--repeats 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import moist  # noqa: E402
import radiation  # noqa: E402
import surface  # noqa: E402
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402

HBM = 8.0e12


def bytes_sfc(kx, ncol):
    return ncol * 24 * 8


def bytes_pbl(kx, ncol):
    return ncol * (8 * kx * 8 + 9 * 8 + 4)


def bytes_chain(kx, ncol, sw):
    """moist (reads 3 kx + 1 + 2 kx, writes 2 kx + 3 kx + 2 + 2 ints), radiation without optional outputs but ssrd / slrd
    (tools/radiation_rate.py less its optional outputs), surface, boundary layer"""
    moist_b = (5 * kx + 1 + 5 * kx + 2) * 8 + 8
    down = 5 * kx * 8 + (kx + 5) * 8 + 8 + (((2 * kx + 7) * 8 + 4 + (5 * kx + 3) * 8) if sw else 0)
    up = ((8 * kx + 10) + kx) * 8
    return ncol * (moist_b + down + up) + bytes_sfc(kx, ncol) + bytes_pbl(kx, ncol)


def time_fn(fn, reps, repeats):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(us)), min(us), max(us)


def rates(res, kx, nbs, reps, repeats):
    sp = s.Spectral(res, kx=kx, max_batch=max(nbs), device=0)
    if kx == 16:
        sp.set_sigma(synth.SIGMA_L16)
    sp.radiation_set_date(radiation.DATES[0])
    il, ix = sp.il, sp.ix
    ncol = il * ix
    tab = moist.tables(moist.HSG[kx])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ("fsol", "ozone", "ozupp", "zenit", "stratz")}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    c = surface.columns(tab, ncol, 1, zon, sqcoa)
    sp.surface_set_orography(c["phis0"].reshape(il, ix))
    sp.column_physics_workspace()
    r, _ = surface.chain(tab, c, zon, sqcoa)
    dev = lambda a, dt=np.float64: torch.from_numpy(radiation.grids(a, 1, il, ix).astype(dt)).cuda()
    one = {n: dev(c[n]) for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend", "qtend", "albsfc") + surface.BOUNDARY}
    one.update(ssrd=dev(r["ssrd"]), slrd=dev(r["down"]["slrd"]), icnv=dev(r["moist"]["icnv"], np.int32))
    one.update({n: dev(r["moist"][n]) for n in ("se", "rh", "qsat")})
    one["flux3"] = torch.from_numpy(np.stack([radiation.grids(f, 1, il, ix)[0] for f in r["flux3"]])[None]).cuda()
    S = sp.radiation_state_size()
    rows = []
    for nb in nbs:
        d = {n: x.expand((nb,) + tuple(x.shape[1:])).contiguous() for n, x in one.items()}
        st = torch.zeros(nb * S, dtype=torch.float64, device="cuda")
        ts, fsfcu = torch.zeros_like(d["pslg"]), torch.zeros_like(d["pslg"])
        flux3 = torch.zeros_like(d["flux3"])
        tend = [d[n].clone() for n in ("utend", "vtend", "ttend", "qtend")]

        def chain(sw):
            sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], st, *tend)
        chain(True)
        graphs = {}
        for sw in (True, False):
            with sp.graph_capture() as g:
                chain(sw)
            graphs[sw] = g
        calls = (("surface", lambda: sp.surface_fluxes_dev(d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d["ssrd"],
                                                          d["slrd"], d, ts, fsfcu, flux3), bytes_sfc(kx, ncol)),
                 ("pbl", lambda: sp.pbl_dev(d["qg"], d["phig"], d["pslg"], d["se"], d["rh"], d["qsat"], d["icnv"], d["flux3"], *tend),
                  bytes_pbl(kx, ncol)),
                 ("chain_sw", lambda: chain(True), bytes_chain(kx, ncol, True)),
                 ("chain_nosw", lambda: chain(False), bytes_chain(kx, ncol, False)),
                 ("chain_sw_graph", graphs[True].launch, bytes_chain(kx, ncol, True)),
                 ("chain_nosw_graph", graphs[False].launch, bytes_chain(kx, ncol, False)))
        for name, fn, nbytes in calls:
            us, lo, hi = time_fn(fn, reps, repeats)
            bw = nbytes * nb / (us * 1e-6)
            rows.append({"res": res, "kx": kx, "nb": nb, "call": name, "us": round(us, 2), "us_min": round(lo, 2),
                         "us_max": round(hi, 2), "bytes": nbytes * nb, "TB_s": round(bw / 1e12, 3), "frac_8TBs": round(bw / HBM, 3)})
            print(json.dumps(rows[-1]), flush=True)
        for g in graphs.values():
            g.close()
    sp.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = rates("t30", 8, [1, 64, 512], a.reps, a.repeats) + rates("t63", 16, [1, 16, 64], a.reps, a.repeats)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
