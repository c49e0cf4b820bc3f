"""Surface fluxes and vertical diffusion of the column: get_surface_fluxes with lfluxland = .true. (surface_fluxes.f90:97-295),
set_orog_land_sfc_drag (:300-309), get_vertical_diffusion_tend (vertical_diffusion.f90:30-143) and the boundary-layer sums of
get_physical_tendencies (physics.f90:193-205) restated in NumPy, their level tables, and seeded columns to run them on.  Pinned to
the flang-built reference by tests/golden/ref_surface.npz (tests/golden/make_golden_surface.py); the device kernels
(csrc/spdy_surface.hip) are checked against both.

Arrays as in tests/moist.py and tests/radiation.py: [kx, ncol] columns (level k of the reference at row k - 1), vectorised over
columns.  Default-real literals are float32 values widened to double: f32(x).  What the reference does oddly is restated as it
is: fhum0 = 0 (q1 = qa(kx), rh unused), hfluxn(:,:,2) with + shf + alhc*evap, t0 computed twice, ftemp0*t1 + gtemp0*t2 kept,
x**2.0 = x*x, x**3.0 = x*(x*x), x**4.0 a pow call."""
import numpy as np

import moist
import radiation
import support
import synth
from moist import ALHC, CP, GRAV, P0, f32, get_qsat
from radiation import EMISFC, SBC

# surface_fluxes.f90:12-34, vertical_diffusion.f90:19-26, physical_constants.f90:23-25
FWIND0, FTEMP0, FHUM0, CDL, CDS, CHL, CHS = f32(0.95), f32(1.0), f32(0.0), f32(2.4e-3), f32(1.0e-3), f32(1.2e-3), f32(0.9e-3)
VGUST, CTDAY, DTHETA, FSTAB, HDRAG, CLAMBDA, CLAMBSN = f32(5.0), f32(1.0e-2), f32(3.0), f32(0.67), f32(2000.0), f32(7.0), f32(7.0)
TRSHC, TRVDI, TRVDS, REDSHC, RHGRAD, SEGRAD = f32(6.0), f32(24.0), f32(6.0), f32(0.5), f32(0.5), f32(0.1)
RGAS = f32(np.float32(2.0) / np.float32(7.0)) * CP

SFC_3 = ("ustr", "vstr", "shf", "evap", "slru")               # (ix,il,3): land, sea, weighted
SFC_2D = ("ts", "tskin", "u0", "v0", "t0")                    # (ix,il)
FLUX3 = ("ustr", "vstr", "shf", "evap")                       # plane 3 of these is what the boundary layer reads
BOUNDARY = ("fmask", "sst", "stl", "soilw", "snowc", "alb_l", "alb_s")
SFC_BRANCHES = ("lapse", "inversion", "land_clamp_hi", "land_mid_unstable", "land_mid_stable", "land_clamp_lo", "sea_clamp_hi",
                "sea_mid_unstable", "sea_mid_stable", "sea_clamp_lo", "evap_pos", "evap_zero")
PBL_BRANCHES = ("shc_cnv_drh", "shc_cnv_nodrh", "shc_nocnv_drh", "shc_nocnv_nodrh", "stable_diff", "stable_none", "qdiff_some",
                "qdiff_none", "damp_some", "damp_none")


def _margin(a, b, exact=False):
    return moist._margin(np.asarray(a, np.float64), np.broadcast_to(np.asarray(b, np.float64), np.shape(a)), exact)


def forog(phis0):
    """set_orog_land_sfc_drag (surface_fluxes.f90:300-309)"""
    rhdrag = 1.0 / (GRAV * HDRAG)
    return 1.0 + rhdrag * (1.0 - np.exp(-np.maximum(phis0, 0.0) * rhdrag))


def vdiff_tables(tab):
    """vertical_diffusion.f90:57-77 and the per-level drh0 / fvdiq2 of :80-81, :114-115: scalars [cshc cvdi fshcq fshcse fvdiq fvdise],
    rsig [kx], rsig1 [kx] (entry kx unused = 0), drh0 [kx], fvdiq2 [kx] (entry k - 1 for the pair of levels k, k + 1; last 0)."""
    kx, dhs, fsg, sigh = tab["kx"], tab["dhs"], tab["fsg"], tab["sigh"]
    nl1 = kx - 1
    cshc = dhs[kx - 1] / 3600.0
    cvdi = (sigh[nl1] - sigh[1]) / float(np.float32(nl1 - 1) * np.float32(3600.0))
    fshcq, fshcse = cshc / TRSHC, cshc / (TRSHC * CP)
    fvdiq, fvdise = cvdi / TRVDI, cvdi / (TRVDS * CP)
    rsig = 1.0 / dhs
    rsig1 = np.zeros(kx)
    rsig1[:nl1] = 1.0 / (1.0 - sigh[1:kx])
    drh0, fvdiq2 = np.zeros(kx), np.zeros(kx)
    drh0[:nl1] = RHGRAD * (fsg[1:] - fsg[:-1])
    fvdiq2[:nl1] = fvdiq * sigh[1:kx]
    return {"vd_scalars": np.array([cshc, cvdi, fshcq, fshcse, fvdiq, fvdise]), "vd_rsig": rsig, "vd_rsig1": rsig1,
            "vd_drh0": drh0, "vd_fvdiq2": fvdiq2}


def fluxes(tab, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd, phis0, fo, sqcoa):
    """get_surface_fluxes(..., lfluxland = .true.) on [kx, ncol] columns.  bnd: dict of BOUNDARY fields [ncol]; phis0, fo (forog),
    sqcoa (sqrt(coa(j)) of the column's latitude) [ncol].  Returns SFC_3 as [3, ncol], hfluxn [2, ncol], SFC_2D [ncol], `margin`
    and `branch_cols`."""
    kx = tab["kx"]
    wvi2, sigl = tab["wvi"][1][kx - 1], tab["sigl"][kx - 1]
    fmask, tsea, stl, soilw, snowc, alb_l, alb_s = [bnd[n] for n in BOUNDARY]
    psa = np.exp(pslg)
    ua, va, ta, tb, phi = ug[kx - 1], vg[kx - 1], tg[kx - 1], tg[kx - 2], phig[kx - 1]
    qa = np.maximum(qg[kx - 1], 0.0)                           # physics.f90:113, before the call
    esbc = EMISFC * SBC
    u0, v0 = FWIND0 * ua, FWIND0 * va
    gtemp0, rcp = 1.0 - FTEMP0, 1.0 / CP
    dt1 = wvi2 * (ta - tb)
    t11 = ta + dt1
    t12 = t11 - phis0 * dt1 / (RGAS * 288.0 * sigl)
    t22 = ta + rcp * phi
    t21 = t22 - rcp * phis0
    lapse = ta > tb
    margin = _margin(ta, tb, exact=True)
    t11 = np.where(lapse, FTEMP0 * t11 + gtemp0 * t21, ta)
    t12 = np.where(lapse, FTEMP0 * t12 + gtemp0 * t22, ta)
    t0 = t12 + fmask * (t11 - t12)
    den0 = (P0 * psa / (RGAS * t0)) * np.sqrt(u0 * u0 + v0 * v0 + VGUST * VGUST)
    tskin = stl + CTDAY * sqcoa * ssrd * (1.0 - alb_l) * psa
    rdth, astab = FSTAB / DTHETA, 0.5

    def stability(ts_, t2):
        d = ts_ - t2
        un = ts_ > t2
        hi, lo = un & (d > DTHETA), ~un & (astab * d < -DTHETA)
        m = np.minimum(_margin(ts_, t2), np.where(un, _margin(d, DTHETA), _margin(astab * d, -DTHETA)))
        dth = np.where(un, np.minimum(DTHETA, d), np.maximum(-DTHETA, astab * d))
        return dth, m, (hi, un & ~hi, ~un & ~lo, lo)
    dthl, m, land_br = stability(tskin, t21)
    margin = np.minimum(margin, m)
    den1 = den0 * (1.0 + dthl * rdth)
    cdldv = CDL * den0 * fo
    ustr1, vstr1 = -cdldv * ua, -cdldv * va
    chlcp = CHL * CP
    shf1 = chlcp * den1 * (tskin - t11)
    q1 = qa
    qs1 = get_qsat(tskin, psa, 1.0)
    margin = np.minimum(margin, _margin(tskin, moist.T0))
    dq = soilw * qs1 - q1
    margin = np.minimum(margin, _margin(soilw * qs1, q1))
    evap1 = CHL * den1 * np.maximum(0.0, dq)
    tsk3 = tskin * (tskin * tskin)
    dslr = 4.0 * esbc * tsk3
    slru1 = esbc * tsk3 * tskin
    hf1 = ssrd * (1.0 - alb_l) + slrd - (slru1 + shf1 + ALHC * evap1)
    clamb = CLAMBDA + snowc * (CLAMBSN - CLAMBDA)
    hf1 = hf1 - clamb * (tskin - stl)
    dtskin = tskin + 1.0
    qs2 = get_qsat(dtskin, psa, 1.0)
    margin = np.minimum(margin, _margin(dtskin, moist.T0))
    wet = evap1 > 0.0
    qs2 = np.where(wet, soilw * (qs2 - qs1), 0.0)
    dtskin = hf1 / (clamb + dslr + CHL * den1 * (CP + ALHC * qs2))
    tskin = tskin + dtskin
    shf1 = shf1 + chlcp * den1 * dtskin
    evap1 = evap1 + CHL * den1 * qs2 * dtskin
    slru1 = slru1 + dslr * dtskin
    hf1 = clamb * (tskin - stl)
    dths, m, sea_br = stability(tsea, t22)
    margin = np.minimum(margin, m)
    den2 = den0 * (1.0 + dths * rdth)
    cdsdv = CDS * den2
    ustr2, vstr2 = -cdsdv * ua, -cdsdv * va
    shf2 = CHS * CP * den2 * (tsea - t12)
    qs2 = get_qsat(tsea, psa, 1.0)
    margin = np.minimum(margin, _margin(tsea, moist.T0, exact=True))
    evap2 = CHS * den2 * (qs2 - q1)
    slru2 = esbc * np.power(tsea, 4.0)
    hf2 = ssrd * (1.0 - alb_s) + slrd - slru2 + shf2 + ALHC * evap2
    w = lambda a, b: np.stack([a, b, b + fmask * (a - b)])
    out = {"ustr": w(ustr1, ustr2), "vstr": w(vstr1, vstr2), "shf": w(shf1, shf2), "evap": w(evap1, evap2), "slru": w(slru1, slru2),
           "hfluxn": np.stack([hf1, hf2]), "ts": tsea + fmask * (stl - tsea), "tskin": tsea + fmask * (tskin - tsea), "u0": u0,
           "v0": v0, "t0": t12 + fmask * (t11 - t12), "margin": margin, "den0": den0, "dq": dq}
    br = {"lapse": lapse, "inversion": ~lapse, "evap_pos": wet, "evap_zero": ~wet}
    for side, b in (("land", land_br), ("sea", sea_br)):
        for n, v in zip(("clamp_hi", "mid_unstable", "mid_stable", "clamp_lo"), b):
            br["%s_%s" % (side, n)] = v
    out["branch_cols"] = br
    return out


def pbl(tab, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend):
    """get_vertical_diffusion_tend and physics.f90:197-205 on [kx, ncol] columns; flux3 [4, ncol] = ustr3 vstr3 shf3 evap3.  Returns
    ut_pbl, vt_pbl [ncol] (level kx; zero above), tt_pbl, qt_pbl [kx, ncol], the updated utend .. qtend, `margin`, `branch_cols`."""
    kx = tab["kx"]
    nl1 = kx - 1
    v = vdiff_tables(tab)
    cshc, cvdi, fshcq, fshcse, fvdiq, fvdise = v["vd_scalars"]
    rsig, rsig1, sigh = v["vd_rsig"], v["vd_rsig1"], tab["sigh"]
    n = se.shape[1]
    qa = np.maximum(qg, 0.0)
    tt, qt = np.zeros((kx, n)), np.zeros((kx, n))
    # 2. shallow convection
    drh0, fvdiq2 = v["vd_drh0"][nl1 - 1], v["vd_fvdiq2"][nl1 - 1]
    dmse = se[kx - 1] - se[nl1 - 1] + ALHC * (qa[kx - 1] - qsat[nl1 - 1])
    drh = rh[kx - 1] - rh[nl1 - 1]
    margin = np.minimum(_margin(se[kx - 1] - se[nl1 - 1], -(ALHC * (qa[kx - 1] - qsat[nl1 - 1]))), _margin(rh[kx - 1], rh[nl1 - 1]))
    margin = np.minimum(margin, _margin(drh, drh0))
    un = dmse >= 0.0
    fcnv = np.where(icnv > 0, REDSHC, 1.0)
    fluxse = fcnv * fshcse * dmse
    tt[nl1 - 1] = np.where(un, fluxse * rsig[nl1 - 1], 0.0)
    tt[kx - 1] = np.where(un, -fluxse * rsig[kx - 1], 0.0)
    a = un & (drh >= 0.0)
    b = ~un & (drh > drh0)
    fluxq = np.where(a, fcnv * fshcq * qsat[kx - 1] * drh, fvdiq2 * qsat[nl1 - 1] * drh)
    qt[nl1 - 1] = np.where(a | b, fluxq * rsig[nl1 - 1], 0.0)
    qt[kx - 1] = np.where(a | b, -fluxq * rsig[kx - 1], 0.0)
    br = {"shc_cnv_drh": a & (icnv > 0), "shc_cnv_nodrh": un & ~a & (icnv > 0), "shc_nocnv_drh": a & ~(icnv > 0),
          "shc_nocnv_nodrh": un & ~a & ~(icnv > 0), "stable_diff": b, "stable_none": ~un & ~b}
    # 3. vertical diffusion of moisture above the PBL
    some = np.zeros(n, bool)
    for k in range(3, kx - 1):
        if sigh[k] > 0.5:
            d0, f2 = v["vd_drh0"][k - 1], v["vd_fvdiq2"][k - 1]
            drh = rh[k] - rh[k - 1]
            c = drh >= d0
            margin = np.minimum(margin, _margin(drh, d0))
            fluxq = f2 * qsat[k - 1] * drh
            qt[k - 1] = np.where(c, qt[k - 1] + fluxq * rsig[k - 1], qt[k - 1])
            qt[k] = np.where(c, qt[k] - fluxq * rsig[k], qt[k])
            some |= c
    br["qdiff_some"], br["qdiff_none"] = some, ~some
    # 4. damping of super-adiabatic lapse rate
    some = np.zeros(n, bool)
    for k in range(1, nl1 + 1):
        se0 = se[k] + SEGRAD * (phig[k - 1] - phig[k])
        c = se[k - 1] < se0
        margin = np.minimum(margin, _margin(se[k - 1], se0))
        fluxse = fvdise * (se0 - se[k - 1])
        tt[k - 1] = np.where(c, tt[k - 1] + fluxse * rsig[k - 1], tt[k - 1])
        for k1 in range(k + 1, kx + 1):
            tt[k1 - 1] = np.where(c, tt[k1 - 1] - fluxse * rsig1[k - 1], tt[k1 - 1])
        some |= c
    br["damp_some"], br["damp_none"] = some, ~some
    # physics.f90:197-205
    rps = 1.0 / np.exp(pslg)
    gs, gc = tab["grdsig"][kx - 1], tab["grdscp"][kx - 1]
    ut = 0.0 + flux3[0] * rps * gs
    vt = 0.0 + flux3[1] * rps * gs
    tt[kx - 1] = tt[kx - 1] + flux3[2] * rps * gc
    qt[kx - 1] = qt[kx - 1] + flux3[3] * rps * gs
    un, vn = np.array(utend, np.float64), np.array(vtend, np.float64)
    un[kx - 1] = un[kx - 1] + ut
    vn[kx - 1] = vn[kx - 1] + vt
    return {"ut_pbl": ut, "vt_pbl": vt, "tt_pbl": tt, "qt_pbl": qt, "utend": un, "vtend": vn, "ttend": ttend + tt,
            "qtend": qtend + qt, "margin": margin, "branch_cols": br}


# ---------------------------------------------------------------------------------------------------- seeded inputs
MIN_MARGIN = 1e-9


def _draw(tab, ncol, seed):
    """radiation.py's draw, shaped so that the surface and boundary-layer branches all occur (inversions and super-adiabatic pairs in
    the lowest levels, humid layers aloft), plus the winds, the boundary fields and the incoming utend / vtend."""
    kx = tab["kx"]
    d = radiation._draw(tab, ncol, seed)
    u = synth.splitmix64(seed + 0x5FC, ncol * (3 * kx + 16)).reshape(3 * kx + 16, ncol)
    tg, qg = d["tg"], d["qg"]
    tg_drawn = tg.copy()
    # a third of the columns: an inversion in the lowest two levels; a tenth: a super-adiabatic lowest layer
    tg[-1] = np.where(u[0] < 1 / 3, tg[-2] - 4.0 * u[1], tg[-1])
    tg[-1] = np.where(u[0] > 0.9, tg[-2] + 12.0 + 6.0 * u[1], tg[-1])
    # a super-adiabatic layer aloft in a tenth of the columns
    for k in range(1, kx - 2):
        tg[k] = np.where((u[2] < 0.1) & (np.floor(u[3] * (kx - 3)) == k - 1), tg[k + 1] - 2.0 * u[4], tg[k])
    d["tg2"] = d["tg2"] + (tg - tg_drawn)
    # humid layers aloft in a fifth of the columns: the humidity of the level below a dry one raised
    for k in range(2, kx - 1):
        wet = (u[5] < 0.2) & (np.floor(u[6] * (kx - 3)) == k - 2)
        qg[k] = np.where(wet, np.maximum(qg[k], 0.0) + 0.6 * get_qsat(tg[k], np.exp(d["pslg"]), tab["fsg"][k]), qg[k])
    d["ug"] = (3.0 + 37.0 * u[16:16 + kx]) * np.where(u[16 + kx:16 + 2 * kx] < 0.5, -1.0, 1.0)
    d["vg"] = (3.0 + 37.0 * u[16 + kx:16 + 2 * kx]) * np.where(u[16:16 + kx] < 0.5, -1.0, 1.0)
    d["utend"] = 1e-4 * (2.0 * u[16 + 2 * kx:16 + 3 * kx] - 1.0)
    d["vtend"] = d["utend"][::-1].copy()
    fmask = d["fmask"]
    d["sst"] = tg[-1] + 24.0 * u[7] - 8.0
    d["stl"] = tg[-1] + 16.0 * u[8] - 8.0
    d["soilw"] = np.where(u[9] < 0.25, 0.0, u[10])
    d["snowc"] = np.where(u[11] < 0.5, 0.0, u[12])
    d["alb_l"] = 0.1 + 0.5 * u[13]
    d["alb_s"] = 0.07 + 0.5 * u[14]
    d["phis0"] = np.where(fmask > 0.0, GRAV * 3000.0 * u[15] ** 2, 0.0)
    return d


def chain(tab, c, zon, sqcoa, compute_sw=True, state=None):
    """The whole column physics (physics.f90:110-205) on columns c: moist block, radiation down, surface fluxes, radiation up,
    boundary layer.  Returns (outputs of every block by name, the radiation state)."""
    st = {} if state is None else state
    m = moist.column_block(tab, c["tg"], c["qg"], c["phig"], c["pslg"], c["ttend"], c["qtend"])
    r = radiation.down(tab, c["tg"], c["qg"], c["phig"], c["pslg"], m["rh"], m["precnv"], m["precls"], m["iptop"], c["fmask"],
                       c["albsfc"], zon, compute_sw, st)
    ssrd = r["ssrd"] if compute_sw else st["ssrd_held"]
    st["ssrd_held"] = ssrd
    s = fluxes(tab, c["ug"], c["vg"], c["tg"], c["qg"], c["phig"], c["pslg"], ssrd, r["slrd"], c, c["phis0"], forog(c["phis0"]), sqcoa)
    up = radiation.up(tab, c["tg"], c["pslg"], s["ts"], s["slru"][2], st, m["ttend"])
    f3 = np.stack([s[n][2] for n in FLUX3])
    p = pbl(tab, c["qg"], c["phig"], c["pslg"], m["se"], m["rh"], m["qsat"], m["icnv"], f3, c["utend"], c["vtend"], up["ttend"],
            m["qtend"])
    margin = np.minimum(np.minimum(m["margin"], r["margin"]), np.minimum(s["margin"], p["margin"]))
    # ts = tsea + fmask*(stl - tsea) is a rounding sum, except at fmask = 0 where it is the input sst itself (class (i))
    up_margin = np.where(c["fmask"] == 0.0, np.inf, up["margin"]) if moist.EXACT_TIES else up["margin"]
    margin = np.minimum(margin, np.minimum(up_margin, np.min(radiation._tie(c["tg"], exact=True), axis=0)))
    return {"moist": m, "down": r, "sfc": s, "up": up, "pbl": p, "flux3": f3, "ssrd": ssrd, "margin": margin}, st


def sqcoa_columns(coa_half, nb, il, ix):
    """sqrt(coa(j)) per column of nb (il, ix) states (coa symmetric about the equator, geometry.f90:68-73)"""
    coa = np.concatenate([coa_half[:il // 2], coa_half[:il // 2][::-1]])
    return np.tile(np.repeat(np.sqrt(coa), ix), nb)


def columns(tab, ncol, seed, zon, sqcoa):
    """ncol columns with every input of the chain (dict of [kx, ncol] / [ncol]).  A column with any decision of any block within
    MIN_MARGIN of its threshold is drawn again from the next stream."""
    d = _draw(tab, ncol, seed)
    for attempt in range(1, 50):
        r, _ = chain(tab, d, zon, sqcoa)
        bad = np.nonzero(r["margin"] < MIN_MARGIN)[0]
        if bad.size == 0:
            return d
        new = _draw(tab, ncol, seed + 7919 * attempt)
        for k in d:
            d[k][..., bad] = new[k][..., bad]
    raise RuntimeError("could not draw columns clear of ties")


def branch_cols(r):
    b = dict(r["sfc"]["branch_cols"])
    b.update(r["pbl"]["branch_cols"])
    return b


# ------------------------------------------------------------------------------------------------ what the GPU tests share
ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")
SFC_OUT = SFC_3 + ("hfluxn",) + SFC_2D
PBL_OUT = ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl", "utend", "vtend", "ttend", "qtend")


def case(tag, seed, nb=1, date=0, plan=None):
    """(plan with date and no orography yet, tables, columns, zonal and sqrt(coa) per column).  plan: (sp, its half levels) of a
    count outside support.PHYSICS_TAGS (tests/levels.py), used in place of the plan of tag"""
    if plan is None:
        ix, il, kx = support.grid(tag)
        sp, hsg = support.plan(tag, 64), moist.HSG[kx]
    else:
        sp, hsg = plan
        ix, il = sp.ix, sp.il
    sp.radiation_set_date(radiation.DATES[date])
    tab = moist.tables(hsg)
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, nb, il, ix)
    sqcoa = sqcoa_columns(sp.table("coa_half"), nb, il, ix)
    c = columns(tab, nb * il * ix, seed, zon, sqcoa)
    return sp, tab, c, zon, sqcoa
