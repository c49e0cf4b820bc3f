#!/usr/bin/env python3
"""What weight interpolation of the ensemble analysis costs in accuracy (include/spdy.h, "ensemble analysis"): a
property of the method, computed on the CPU with the NumPy restatement (tests/letkf.py, tests/letkfinterp.py), no device needed.

The set-up of tools/ensemble_rate.py --letkf: T30 L8, E = 16, the network of 416 columns (26 x 16) that observes u, v, t, q at every
level and ps, 13 728 observations, each with the members' spread at its place as error and a value one such error around their
mean; sigma_v = 0.1, rho = 1.1; members = a seeded state plus a hundredth of the differences to other seeded states, brought to the
grid by the oracle's transforms.  For every --sigma-h (km) the full analysis is solved at every grid column once; for every stride
the transforms of its coarse columns are interpolated to all columns, and the increments are compared with the full analysis':
the largest and the root-mean-square difference per variable as fractions of that variable's largest increment.

The local sums are formed by matrix products here, not in the definition's order: the figures are differences of 1e-3 and more.

    python tools/letkf_interp_accuracy.py [--sigma-h 500 1000] [--json profiles/letkf_interp_accuracy.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ensemblestep  # noqa: E402
import letkf as lk  # noqa: E402
import letkfinterp as li  # noqa: E402
import support  # noqa: E402
import synth  # noqa: E402
from conftest import VARIANTS  # noqa: E402

STRIDES = [(2, 2), (3, 3), (4, 4)]


def grids(o, sts):
    """time level 1 of the member states on the grid by the oracle's transforms: true wind, t, q, ps"""
    x = {v: [] for v in lk.VARS}
    for st in sts:
        uv = [o.uvspec(st["vor"][0, k], st["div"][0, k]) for k in range(o.kx)]
        x["u"].append(np.stack([o.spec_to_grid(a, 2) for a, _ in uv]))
        x["v"].append(np.stack([o.spec_to_grid(b, 2) for _, b in uv]))
        x["t"].append(np.stack([o.spec_to_grid(st["t"][0, k], 1) for k in range(o.kx)]))
        x["q"].append(np.stack([o.spec_to_grid(st["tr"][0, k], 1) for k in range(o.kx)]))
        x["ps"].append(o.spec_to_grid(st["ps"][0], 1))
    return {v: np.stack(a) for v, a in x.items()}


def all_transforms(g, x, obs, sigma_h, sigma_v, rho, chunk=256):
    """T (ncol, kx, E, E) at every grid column, the local sums as matrix products over the observations in range of a chunk"""
    E, ncol = x["ps"].shape[0], g.ix * g.il
    s = lk.obs_space(g, x, obs)
    Y, d, ounit = s["y"], s["departure"], lk.unit(obs["lon"], obs["lat"])
    rinv = 1.0 / (obs["error"] * obs["error"])
    YY, Yd = (Y[:, :, None] * Y[:, None, :]).reshape(len(d), E * E), Y * d[:, None]
    T = np.zeros((ncol, g.kx, E, E))
    for c0 in range(0, ncol, chunk):
        cols = np.arange(c0, min(c0 + chunk, ncol))
        near = np.nonzero(lk.distance(g.colunit[cols], ounit).min(axis=0) < 2.0 * sigma_h * np.sqrt(10.0 / 3.0))[0]
        r = (lk.weights(g, ounit[near], s["obs_lnsigma"][near], cols, sigma_h, sigma_v) * rinv[near][None, None, :]).reshape(-1, len(near))
        C, b = (r @ YY[near]).reshape(-1, E, E), r @ Yd[near]
        T[cols] = lk.transform(C, b, E, rho)[0].reshape(len(cols), g.kx, E, E)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma-h", nargs="+", type=float, default=[500.0, 1000.0], help="km")
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--json")
    a = ap.parse_args()
    from oracle.pyoracle import Oracle, build
    build()
    tag, E = "t30", a.members
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    sp = support.plan(tag, E * (2 * kx + 1), device=-1)
    g = lk.Geometry(sp)
    ms = ensemblestep.member_states(sp, E + 1)
    x = grids(o, [{n: ms[0][n] + 0.01 * (ms[e + 1][n] - ms[0][n]) for n in ("vor", "div", "t", "tr", "ps")} for e in range(E)])
    lon, lat = np.meshgrid((np.arange(26) + 0.5) * (360.0 / 26), -75.0 + 10.0 * np.arange(16))
    var, lev = np.concatenate([np.repeat(np.arange(4), kx), [4]]), np.concatenate([np.tile(np.arange(kx), 4), [0]])
    nloc, per = lon.size, var.size
    obs = lk.make_obs(np.tile(var, nloc), np.tile(lev, nloc), np.repeat(lon.ravel(), per), np.repeat(lat.ravel(), per),
                      np.zeros(nloc * per), np.ones(nloc * per))
    hx = lk.observe(g, x, obs)[0]
    hxmean = lk.couple(g, obs, hx)["hxmean"]
    obs["error"] = hx.std(axis=1, ddof=1) + 1e-300
    obs["value"] = hxmean + obs["error"] * np.random.default_rng(0).standard_normal(nloc * per)
    allcols = np.arange(g.ix * g.il)
    km_lon, km_lat = 2.0 * np.pi * lk.REARTH / g.ix / 1e3, np.pi * lk.REARTH / g.il / 1e3
    rows = []
    for sh in a.sigma_h:
        T = all_transforms(g, x, obs, sh * 1e3, 0.1, 1.1)
        full = li.increments(g, x, T, allcols)
        top = {v: float(np.max(np.abs(full[v]))) for v in lk.VARS}
        for si, sj in STRIDES:
            idx, wgt = li.stencils(g, si, sj)
            coarse = li.coarse_columns(g, si, sj)
            got = li.increments(g, x, li.interpolate(T[coarse], np.arange(len(coarse)), idx, wgt, allcols), allcols)
            row = {"size": tag, "members": E, "observations": nloc * per, "sigma_h_km": sh, "stride": [si, sj],
                   "coarse_spacing_km_at_equator": [round(si * km_lon), round(sj * km_lat)], "coarse_columns": int(len(coarse)),
                   "max_fraction": {v: float("%.3g" % (np.max(np.abs(got[v] - full[v])) / top[v])) for v in lk.VARS},
                   "rms_fraction": {v: float("%.3g" % (np.sqrt(np.mean((got[v] - full[v]) ** 2)) / top[v])) for v in lk.VARS}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    sp.close()


if __name__ == "__main__":
    main()
