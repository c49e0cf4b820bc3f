#!/usr/bin/env python3
"""Regenerate tests/golden/ref_physrun.npz: the REAL reference's column physics on columns that a model run produced (build
container only).

tests/golden/ref_surface.npz pins the NumPy restatements of the physics (tests/surface.py: chain) to the flang-built reference on
columns drawn to order.  This fixture pins them on columns the model itself made: the full (ix, il) grids of the two-day "wind"
run with the whole physics (tests/physstep.py: reference_run, T30 L8) before leapfrog step 70, a shortwave step, and before step
72, a step without shortwave on the radiation state the run holds -- inversions, humidities clamped after spectral ringing,
convection in some tens of columns.

The reference build is make_golden_surface.build() (flang -O2 of the reference's own modules and of its blocks cut from
physics.f90, in a temporary directory that is deleted afterwards; nothing of the reference is written into the repository).  The
reference keeps the shortwave part of its radiation state in module variables, so it runs the grids of step 70 with shortwave and
then those of step 72 without, which is the state the run holds at step 72 (step 71 computes no shortwave either); ssrd and tt_rsw
pass from the first call to the second as the shim's arguments.

Stored, for a column sample chosen by make_golden_surface's rule with smaller numbers (NUNIFORM uniform + up to NBRANCH per
branch of each grid, one sample for both grids; with that rule's 40 + 4 the file would be twice the size of ref_surface.npz,
because here the inputs are stored for every column of the sample): THE INPUTS THEMSELVES -- grids, incoming tendencies, boundary and zonal fields, sqcoa, and for step 72 the incoming radiation state of
the NumPy run -- and physstep.chain_outputs of the reference; the branch counts of each whole grid.  The test runs surface.chain
on the stored columns only.

    python tests/golden/make_golden_physrun.py
"""
import ctypes
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import make_golden_moist as mg  # noqa: E402
import make_golden_radiation as mr  # noqa: E402
import make_golden_surface as ms  # noqa: E402
import longrun  # noqa: E402
import physstep  # noqa: E402
import radiation  # noqa: E402
import support  # noqa: E402
import surface  # noqa: E402
from dynstep import ROB, oracle_dynamics_step  # noqa: E402

P = mg.P
TAG = "t30"
NUNIFORM, NBRANCH = 12, 2


def reference_chain(lib, c, sw, held, kx, il, ix):
    """the reference's chain on the grids c ([.., il * ix]), as make_golden_surface.run drives it; held: ssrd, ssr, tsr, tt_rsw,
    cloudc, clstr, icltop of the last shortwave call (None on a shortwave call).  Returns (outputs by name, held)"""
    G = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, il, ix).squeeze(0) if np.ndim(a) == 1
                                       else np.asarray(a, np.float64).reshape(-1, il, ix))
    a = {n: G(c[n]).copy() for n in ("tg", "qg", "phig", "pslg", "ttend", "qtend", "utend", "vtend")}
    m = {n: np.zeros((il, ix)) for n in ("precnv", "precls", "cbmf")}
    m.update({n: np.zeros((il, ix), np.int32) for n in ("iptop", "icnv")})
    m.update({n: np.zeros((kx, il, ix)) for n in ("qsat", "rh", "se")})
    lib.moist_run(*[P(a[n]) for n in ("tg", "qg", "phig", "pslg", "ttend", "qtend")],
                  *[P(m[n]) for n in ("precnv", "precls", "cbmf", "iptop", "icnv", "qsat", "rh", "se")])
    if held is None:
        held = {n: np.zeros((il, ix)) for n in ("cloudc", "clstr", "ssrd", "ssr", "tsr")}
        held.update(icltop=np.zeros((2, il, ix), np.int32), tt_rsw=np.zeros((kx, il, ix)))
    o = {n: np.zeros((il, ix)) for n in ("slrd", "slr", "olr")}
    o["tt_rlw"] = np.zeros((kx, il, ix))
    lib.rad_down(ctypes.c_int(1 if sw else 0), P(a["tg"]), P(a["qg"]), P(a["phig"]), P(a["pslg"]), P(m["se"]), P(m["rh"]),
                 P(m["precnv"]), P(m["precls"]), P(m["iptop"]), P(G(c["fmask"])), P(G(c["albsfc"])), P(held["icltop"]),
                 P(held["cloudc"]), P(held["clstr"]), P(held["ssrd"]), P(held["ssr"]), P(held["tsr"]), P(held["tt_rsw"]),
                 P(o["slrd"]), P(o["tt_rlw"]))
    s = {n: np.zeros((3, il, ix)) for n in surface.SFC_3}
    s["hfluxn"] = np.zeros((2, il, ix))
    s.update({n: np.zeros((il, ix)) for n in surface.SFC_2D})
    lib.sfc_run(P(G(c["ug"])), P(G(c["vg"])), P(a["tg"]), P(a["qg"]), P(m["rh"]), P(a["phig"]), P(a["pslg"]), P(G(c["phis0"])),
                *[P(G(c[n])) for n in surface.BOUNDARY], P(held["ssrd"]), P(o["slrd"]),
                *[P(s[n]) for n in surface.SFC_3 + ("hfluxn",) + surface.SFC_2D])
    lib.rad_up(P(a["tg"]), P(a["pslg"]), P(s["ts"]), P(o["slrd"]), P(s["slru"]), P(o["slr"]), P(o["olr"]), P(held["tt_rsw"]),
               P(o["tt_rlw"]), P(a["ttend"]))
    b = {n: np.zeros((kx, il, ix)) for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")}
    lib.pbl_run(P(a["qg"]), P(a["phig"]), P(a["pslg"]), P(m["se"]), P(m["rh"]), P(m["qsat"]), P(m["icnv"]),
                *[P(s[n]) for n in surface.FLUX3], *[P(a[n]) for n in ("utend", "vtend", "ttend", "qtend")],
                *[P(b[n]) for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")])
    assert not b["ut_pbl"][:-1].any() and not b["vt_pbl"][:-1].any()       # zero above level kx
    out = dict(s, ssrd=held["ssrd"].copy(), slrd=o["slrd"], ut_pbl=b["ut_pbl"][-1], vt_pbl=b["vt_pbl"][-1], tt_pbl=b["tt_pbl"],
               qt_pbl=b["qt_pbl"], utend=a["utend"][-1], vtend=a["vtend"][-1], ttend=a["ttend"], qtend=a["qtend"], icnv=m["icnv"],
               iptop=m["iptop"], precnv=m["precnv"], precls=m["precls"], cbmf=m["cbmf"], slr=o["slr"], olr=o["olr"])
    return out, held


def run(lib):
    from oracle.pyoracle import Oracle, build
    from conftest import VARIANTS
    build()
    ix, il, kx = support.grid(TAG)
    ncol = il * ix
    o = Oracle(*VARIANTS[TAG])
    sp = support.plan(TAG, 4 * kx + 4, device=-1)
    case = physstep.run_case(sp, o, "wind")
    tab = case.tab
    # the reference's own initialisation, as in make_golden_surface.run
    f = lambda a: np.asfortranarray(a, np.float64)
    lib.moist_init(ctypes.c_int(0), P(f(tab["hsg"])), P(f(tab["dhs"])), P(f(tab["fsg"])))
    lib.rad_tables(P(np.zeros((4, 301))))
    t = {"vd_scalars": np.zeros(6)}
    t.update({n: np.zeros(kx) for n in ms.TABLES[1:]})
    lib.sfc_tables(*[P(t[n]) for n in ms.TABLES])
    coa = np.zeros(il)
    lib.sfc_coa(P(coa))
    assert synth_close(np.repeat(np.sqrt(coa), ix), case.sqcoa)
    z = {n: np.zeros((il, ix)) for n in mr.ZON}
    lib.rad_date(ctypes.c_double(radiation.DATES[0]), *[P(z[n]) for n in mr.ZON])
    for n in mr.ZON:
        assert synth_close(z[n].reshape(-1), case.zon[n]), n
    forog = np.zeros((il, ix))
    lib.sfc_orog(P(np.ascontiguousarray(case.phis0)), P(forog))

    _, log, pre = physstep.reference_run(case, physstep.PHYSRUN_STEPS)       # leaves o.tail_init(2 delt) in place
    per, held = {}, None
    for n in physstep.PHYSRUN_STEPS:
        sw, st = physstep.shortwave_step(n), pre[n]["st"]
        tend = {}

        def grab(o_, s_, ut, vt, tt, qt):         # the tendencies of the dynamics, as the physics receive them
            tend.update(ut=ut.copy(), vt=vt.copy(), tt=tt.copy(), qt=qt.copy())
        oracle_dynamics_step(o, st, 2, 2.0 * longrun.DELT, ROB, physics=grab)
        c = physstep.columns_of(physstep.grids_of(o, st), case.bnd, case.phis0, tend["ut"], tend["vt"], tend["tt"], tend["qt"])
        rs = {k: v.copy() for k, v in pre[n]["rs"].items()}
        r, _ = surface.chain(tab, c, case.zon, case.sqcoa, sw, {k: v.copy() for k, v in rs.items()})
        margin = float(r["margin"].min())
        assert margin >= physstep.RUN_MARGIN, margin
        ref, held = reference_chain(lib, c, sw, None if sw else held, kx, il, ix)
        ref["forog"] = forog
        assert np.array_equal(ref["icnv"].reshape(-1), r["moist"]["icnv"]), "moist icnv: restatement differs"
        br = dict(surface.branch_cols(r), **{"moist_" + k: v for k, v in r["moist"]["branch_cols"].items()})
        print("step %d (shortwave %d): min margin %.2e; %s" % (n, sw, margin, {k: int(v.sum()) for k, v in sorted(br.items())}))
        per[n] = dict(c=c, rs=rs, r=r, ref=ref, br=br, sw=sw, margin=margin)
    # the sample: NUNIFORM uniform + up to NBRANCH per branch of either grid
    pick = [np.linspace(0, ncol - 1, NUNIFORM).astype(np.int64)]
    for n in per:
        for mask in per[n]["br"].values():
            idx = np.nonzero(mask)[0]
            if idx.size:
                pick.append(idx[np.linspace(0, idx.size - 1, min(NBRANCH, idx.size)).astype(np.int64)])
    sub = np.unique(np.concatenate(pick))
    d = {"sub": sub}
    cut = lambda a: np.ascontiguousarray(np.asarray(a).reshape(-1, ncol)[:, sub].squeeze())
    for n, e in per.items():
        p = "s%d_" % n
        names = set(physstep.chain_outputs(e["r"], e["c"]))
        assert names == set(e["ref"]), names ^ set(e["ref"])
        for k in names:
            d[p + "out_" + k] = cut(e["ref"][k])
        for k in physstep.PHYSRUN_INPUTS:
            d[p + "in_" + k] = cut(e["c"][k])
        d[p + "in_sqcoa"] = cut(case.sqcoa)
        for k in physstep.ZON:
            d[p + "zon_" + k] = cut(case.zon[k])
        if not e["sw"]:
            for k in physstep.RAD_STATE:
                a = e["rs"][k]
                d[p + "rs_" + k] = np.ascontiguousarray(a[..., sub])
        d[p + "sw"] = np.bool_(e["sw"])
        names = sorted(e["br"])
        d[p + "branch_names"] = np.array(names)
        d[p + "branch_counts"] = np.array([int(e["br"][k].sum()) for k in names], np.int64)
        d[p + "min_margin"] = np.float64(e["margin"])
    return d


def synth_close(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) <= 1e-13 * max(1.0, float(np.max(np.abs(b))))


def save(path, d):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same file"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_physrun: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    tmp = tempfile.mkdtemp(prefix="spdy_physrun_")
    d = {}

    def work():
        d.update(run(ms.build(TAG, tmp)))
    # the reference's (ix, il, kx) work arrays are automatic arrays: a large stack
    import threading
    threading.stack_size(256 << 20)
    th = threading.Thread(target=work)
    try:
        th.start()
        th.join()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not d:
        sys.exit("make_golden_physrun: failed")
    out = os.path.join(HERE, "ref_physrun.npz")
    save(out, d)
    print("wrote %s (%.2f MB, %d columns)" % (out, os.path.getsize(out) / 1e6, d["sub"].size))


if __name__ == "__main__":
    main()
