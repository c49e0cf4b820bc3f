#!/usr/bin/env python3
"""Rate of the radiation kernels (spdy_radiation_down_dev / spdy_radiation_up_dev, csrc/spdy_radiation.hip) at T30 L8 over
nb = 1, 64, 512 states and T63 L16 over nb = 1, 16, 64, for both compute_sw values, timed with HIP events on the plan's stream,
against the byte model of DESIGN.md §11 (every optional output requested).  Per column, in doubles (icltop and iptop are ints):
  shortwave launch (compute_sw only)  reads 2 kx + 7 (+ iptop)    writes 6 kx + 7 (+ icltop)
  longwave-down launch                reads 5 kx                  writes kx + 6
  up launch                           reads 8 kx + 10             writes 2 kx + 2

    python tools/radiation_rate.py [--reps 200] [--json out.json]"""
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
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402

HBM = 8.0e12


def bytes_down(kx, ncol, sw):
    b = 5 * kx * 8 + (kx + 6) * 8
    if sw:
        b += (2 * kx + 7) * 8 + 4 + (6 * kx + 7) * 8 + 4
    return ncol * b


def bytes_up(kx, ncol):
    return ncol * ((8 * kx + 10) + (2 * kx + 2)) * 8


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


def rates(res, kx, nbs, reps):
    sp = s.Spectral(res, kx=kx, max_batch=max(nbs), device=0)
    if kx == 16:
        sp.set_sigma(synth.SIGMA_L16)
    sp.radiation_set_date(radiation.DATES[0])
    il, ix = sp.il, sp.ix
    ncol = il * ix
    tab = moist.tables(moist.HSG[kx])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ("fsol", "ozone", "ozupp", "zenit", "stratz")}, 1, il, ix)
    c = radiation.columns(tab, ncol, 1, zon)
    one = {n: torch.from_numpy(radiation.grids(c[n], 1, il, ix)).cuda() for n in c if n != "iptop"}
    one["iptop"] = torch.from_numpy(radiation.grids(c["iptop"], 1, il, ix).astype(np.int32)).cuda()
    S = sp.radiation_state_size()
    rows = []
    for nb in nbs:
        d = {n: x.expand((nb,) + tuple(x.shape[1:])).contiguous() for n, x in one.items()}
        st = torch.zeros(nb * S, dtype=torch.float64, device="cuda")
        out = sp.column_outputs(nb, "rad")
        T = d["ttend_m"].clone()

        def down(sw):
            sp.radiation_down_dev(sw, d["tg"], d["qg"], d["phig"], d["pslg"], d["rh"], d["precnv"], d["precls"], d["iptop"],
                                  d["fmask"], d["albsfc"], st, out)
        down(True)
        for name, fn, nbytes in (("down_sw", lambda: down(True), bytes_down(kx, ncol, True)),
                                 ("down_nosw", lambda: down(False), bytes_down(kx, ncol, False)),
                                 ("up", lambda: sp.radiation_up_dev(d["tg"], d["pslg"], d["ts"], d["fsfcu"], st, T, out),
                                  bytes_up(kx, ncol))):
            us = time_fn(fn, reps)
            bw = nbytes * nb / (us * 1e-6)
            rows.append({"res": res, "kx": kx, "nb": nb, "call": name, "us": round(us, 2), "bytes": nbytes * nb,
                         "TB_s": round(bw / 1e12, 3), "frac_8TBs": round(bw / HBM, 3)})
            print(json.dumps(rows[-1]), flush=True)
    sp.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = rates("t30", 8, [1, 64, 512], a.reps) + rates("t63", 16, [1, 16, 64], a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
