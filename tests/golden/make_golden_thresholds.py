#!/usr/bin/env python3
"""Regenerate tests/golden/ref_thresholds.npz from the REAL reference's column physics (build container only).

Built exactly like make_golden_surface.py (its build(): the reference modules compiled by flang -O2 where they lie, with the
params / geometry variants, into a mktemp directory that is deleted afterwards; the committed shims moist_shim.f90, rad_shim.f90
and sfc_shim.f90 are the bind(C) entries).  Nothing from the reference is committed: the only output is the npz.

Two things are recorded.
  * For T30 L8 and T30 L5 (thresholds.TAGS) the reference's own chain -- moist block, radiation down, surface fluxes, radiation
    up, boundary layer -- on tests/thresholds.py's state, whose constructed columns sit exactly ON the class-(i) thresholds of
    thresholds.INVENTORY and one ulp to either side: a call with shortwave at the first date of radiation.DATES, then a call
    without shortwave on thresholds.second()'s inputs with the radiation state held (tau2, stratc, flux in the reference's
    modules; tt_rsw and ssrd here).  Kept: every output of both calls on the constructed columns and a few plain ones, and a digest
    of every input array (the tests regenerate the inputs from the seed).  The generator asserts that every class-(i) row is hit
    on every side it names, and that the restatement's integers equal the reference's.
    Of the call without shortwave the moist block's own outputs are left out (its inputs are those of the first call) and of
    utend, vtend only level kx is kept (the levels above are untouched).
  * For the four variants the zonal forcing of get_zonal_average_fields at TYEARS: fsol, ozone, ozupp, zenit, stratz [il], whole
    for t30 and t63k16; t30k5 and t30k7 (the same grid as t30) are asserted equal to t30 bit for bit and keep a digest.

    python tests/golden/make_golden_thresholds.py
"""
import ctypes
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden_moist as mg  # noqa: E402
import make_golden_radiation as mr  # noqa: E402
import make_golden_surface as ms  # noqa: E402
import moist  # noqa: E402
import physlevels  # noqa: E402
import radiation  # noqa: E402
import surface  # noqa: E402
import synth  # noqa: E402
import thresholds as th  # noqa: E402

P = mg.P
INPUTS = ms.INPUTS + ("ttend2",)
# 0, the cardinal dates, the two dates in use, the last values below 1, and every 12th of the year
TYEARS = tuple(sorted(set((0.0, th.EQUINOX_MAR, th.SOLSTICE_JUN, 265.5 / 365.0, th.SOLSTICE_DEC) + radiation.DATES +
                          (1.0 - 1.0 / (365.0 * 36.0), 1.0 - 2.0 ** -30, float(np.nextafter(1.0, 0.0))) +
                          tuple(k / 12.0 for k in range(1, 12)))))


def reference_call(lib, c, sw, held, il, ix, kx):
    """the reference's chain on the columns c; held: tt_rsw and ssrd of the shortwave call (filled by it, read without it)"""
    G = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, il, ix).squeeze(0) if np.ndim(a) == 1
                                       else np.asarray(a, np.float64).reshape(-1, il, ix))
    a = {n: G(c[n]).copy() for n in ("tg", "qg", "phig", "pslg", "ttend", "qtend", "utend", "vtend")}
    m = {n: np.zeros((il, ix)) for n in ("precnv", "precls", "cbmf")}
    m.update({n: np.zeros((il, ix), np.int32) for n in ("iptop", "icnv")})
    m.update({n: np.zeros((kx, il, ix)) for n in ("qsat", "rh", "se")})
    lib.moist_run(*[P(a[n]) for n in ("tg", "qg", "phig", "pslg", "ttend", "qtend")],
                  *[P(m[n]) for n in ("precnv", "precls", "cbmf", "iptop", "icnv", "qsat", "rh", "se")])
    o = {n: np.zeros((il, ix)) for n in ("cloudc", "clstr", "ssr", "tsr", "slrd", "slr", "olr")}
    o["ssrd"], o["tt_rsw"] = held["ssrd"], held["tt_rsw"]
    icl = np.zeros((2, il, ix), np.int32)
    o["tt_rlw"] = np.zeros((kx, il, ix))
    lib.rad_down(ctypes.c_int(1 if sw else 0), P(a["tg"]), P(a["qg"]), P(a["phig"]), P(a["pslg"]), P(m["se"]), P(m["rh"]),
                 P(m["precnv"]), P(m["precls"]), P(m["iptop"]), P(G(c["fmask"])), P(G(c["albsfc"])), P(icl), P(o["cloudc"]),
                 P(o["clstr"]), P(o["ssrd"]), P(o["ssr"]), P(o["tsr"]), P(o["tt_rsw"]), P(o["slrd"]), P(o["tt_rlw"]))
    s = {n: np.zeros((3, il, ix)) for n in surface.SFC_3}
    s["hfluxn"] = np.zeros((2, il, ix))
    s.update({n: np.zeros((il, ix)) for n in surface.SFC_2D})
    lib.sfc_run(P(G(c["ug"])), P(G(c["vg"])), P(a["tg"]), P(a["qg"]), P(m["rh"]), P(a["phig"]), P(a["pslg"]), P(G(c["phis0"])),
                *[P(G(c[n])) for n in surface.BOUNDARY], P(o["ssrd"]), P(o["slrd"]),
                *[P(s[n]) for n in surface.SFC_3 + ("hfluxn",) + surface.SFC_2D])
    lib.rad_up(P(a["tg"]), P(a["pslg"]), P(s["ts"]), P(o["slrd"]), P(s["slru"]), P(o["slr"]), P(o["olr"]), P(o["tt_rsw"]),
               P(o["tt_rlw"]), P(a["ttend"]))
    b = {n: np.zeros((kx, il, ix)) for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")}
    lib.pbl_run(P(a["qg"]), P(a["phig"]), P(a["pslg"]), P(m["se"]), P(m["rh"]), P(m["qsat"]), P(m["icnv"]),
                *[P(s[n]) for n in surface.FLUX3], *[P(a[n]) for n in ("utend", "vtend", "ttend", "qtend")],
                *[P(b[n]) for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")])
    assert not b["ut_pbl"][:-1].any() and not b["vt_pbl"][:-1].any()       # zero above level kx
    out = {"moist." + n: m[n] for n in m}
    out.update({"rad." + n: o[n] for n in ("slrd", "slr", "olr", "tt_rlw")})
    if sw:
        out.update({"rad." + n: o[n].copy() for n in ("cloudc", "clstr", "ssrd", "ssr", "tsr", "tt_rsw")})
        out["rad.icltop"] = icl[0]
    out.update({"sfc." + n: s[n] for n in surface.SFC_3 + ("hfluxn", "tskin", "u0", "v0", "t0")})
    out.update({"pbl.ut_pbl": b["ut_pbl"][-1], "pbl.vt_pbl": b["vt_pbl"][-1], "pbl.tt_pbl": b["tt_pbl"], "pbl.qt_pbl": b["qt_pbl"]})
    out.update(ts=s["ts"], fsfcu=s["slru"][2])
    out.update({n: a[n] for n in th.TEND})
    return {n: np.asarray(v).reshape(-1, il * ix).squeeze() for n, v in out.items()}


def init(tag, lib):
    ix, il, kx, tab = mg.init_levels(tag, lib)
    lib.rad_tables(P(np.zeros((4, 301))))
    t = [np.zeros(6)] + [np.zeros(kx) for _ in ms.TABLES[1:]]
    lib.sfc_tables(*[P(x) for x in t])
    return tab


def date(lib, tyear, il, ix):
    z = {n: np.zeros((il, ix)) for n in mr.ZON}
    lib.rad_date(ctypes.c_double(tyear), *[P(z[n]) for n in mr.ZON])
    for n in mr.ZON:
        assert np.all(z[n] == z[n][:, :1])
    return {n: z[n][:, 0].copy() for n in mr.ZON}


def run(tag, lib, seed=None):
    """seed: the thresholds.build seed of a variant outside thresholds.TAGS whose constructed columns are wanted all the same
    (make_golden_physlevels.py)"""
    ix, il, kx, _, _ = physlevels.variant(tag)
    ncol = il * ix
    tab = init(tag, lib)
    d = {tag + "_tyear": np.array(TYEARS)}
    zs = [date(lib, ty, il, ix) for ty in TYEARS]
    year = np.stack([np.stack([z[n] for z in zs]) for n in mr.ZON])            # [5, dates, il]
    d[tag + "_year_digest"] = np.array(synth.digest(year))
    if tag in ("t30", "t63k16"):
        d[tag + "_year"] = year
    if tag not in th.TAGS and seed is None:
        return d
    seed = th.SEED[tag] if seed is None else seed
    coa = np.zeros(il)
    lib.sfc_coa(P(coa))
    sqcoa = np.repeat(np.sqrt(coa), ix)
    zon = radiation.zonal_columns(date(lib, radiation.DATES[0], il, ix), 1, il, ix)
    c, sub, r1, r2 = th.build(tab, ncol, seed, zon, sqcoa)
    H = th.hits(tab, c, r1, zon)
    for row in th.CLASS_I:
        for side in row["sides"]:
            assert H[row["id"], side][sub].any(), "%s: no stored column on side %d of %s" % (tag, side, row["id"])
    forog = np.zeros((il, ix))
    lib.sfc_orog(P(np.ascontiguousarray(c["phis0"].reshape(il, ix))), P(forog))
    held = {"ssrd": np.zeros((il, ix)), "tt_rsw": np.zeros((kx, il, ix))}
    worst = 0.0
    for step, cc, r, sw in ((1, c, r1, True), (2, th.second(c), r2, False)):
        ref = reference_call(lib, cc, sw, held, il, ix, kx)
        mine = th.flat(r, kx)
        for n, v in ref.items():
            w = np.asarray(mine[n]).reshape(v.shape)
            if v.dtype.kind == "i":
                assert np.array_equal(v, w), "%s call %d %s: restatement differs" % (tag, step, n)
            else:
                worst = max(worst, synth.relerr(w, v))
            if step == 2 and n.startswith("moist."):
                continue
            d["%s_c%d_%s" % (tag, step, n)] = v[kx - 1, sub] if n in ("utend", "vtend") else v[..., sub]
    print("%s: %d stored columns, restatement against the reference worst %.1e" % (tag, sub.size, worst))
    d[tag + "_seed"] = np.int64(seed)
    d[tag + "_sub"] = sub
    d[tag + "_forog"] = forog.reshape(-1)[sub]
    d[tag + "_in_names"] = np.array(INPUTS)
    d[tag + "_in_digest"] = np.array([synth.digest(np.asarray(c[n], np.float64)) for n in INPUTS])
    return d


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_thresholds: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    tmp = tempfile.mkdtemp(prefix="spdy_thr_")
    d, done = {}, []

    def work():
        for tag in mg.BUILDS:
            d.update(run(tag, ms.build(tag, tmp)))
            done.append(tag)
    # the reference's (ix, il, kx) work arrays are automatic arrays: several MB of stack at T63 L16
    import threading
    threading.stack_size(256 << 20)
    t = threading.Thread(target=work)
    try:
        t.start()
        t.join()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if len(done) < len(mg.BUILDS):
        sys.exit("make_golden_thresholds: a variant failed")
    for tag in ("t30k5", "t30k7"):
        assert str(d[tag + "_year_digest"]) == str(d["t30_year_digest"]), tag
    out = os.path.join(HERE, "ref_thresholds.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%.2f MB)" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
