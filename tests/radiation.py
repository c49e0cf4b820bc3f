"""Radiation of the column: the radiation schemes of get_physical_tendencies (physics.f90:146-166, :180-186) restated in NumPy --
clouds and the shortwave fluxes (shortwave_radiation.f90:74-234, :332-410), the longwave fluxes (longwave_radiation.f90:16-194),
their tables (radset, :197-220) and the zonal forcing of a date (get_zonal_average_fields + solar, shortwave_radiation.f90:238-329)
-- plus seeded columns to run them on.  Pinned to the flang-built reference by tests/golden/ref_radiation.npz
(tests/golden/make_golden_radiation.py); the device kernels (csrc/spdy_radiation.hip) are checked against both.

Arrays as in tests/moist.py: the restatement works on [kx, ncol] columns (level k of the reference at row k - 1), vectorised over
columns and looping over k (and bands) as the reference does.  The module state of the reference (tau2, stratc, flux) and the
held shortwave heating are a dict `state`.  Default-real literals are float32 values widened to double: f32(x)."""
import math

import numpy as np

import moist
import synth
from moist import CP, f32

SBC, EPSLW, EMISFC = f32(5.67e-8), f32(0.05), f32(0.98)
SOLC, RHCL1, RHCL2, QACL, WPCL, PMAXCL = f32(342.0), f32(0.30), f32(1.00), f32(0.20), f32(0.2), f32(10.0)
CLSMAX, CLSMINL, GSE_S0, GSE_S1 = f32(0.60), f32(0.15), f32(0.25), f32(0.40)
ALBCL, ALBCLS, EPSSW = f32(0.43), f32(0.50), f32(0.020)
ABSDRY, ABSAER, ABSWV1, ABSWV2, ABSCL1, ABSCL2 = f32(0.033), f32(0.033), f32(0.022), f32(15.000), f32(0.015), f32(0.15)
ABLWIN, ABLCO2, ABLWV1, ABLWV2, ABLCL1, ABLCL2 = f32(0.3), f32(6.0), f32(0.7), f32(50.0), f32(12.0), f32(0.6)
# two dates, so that each hemisphere has polar night (stratz > 0) in one of them
DATES = (0.0411, 0.5411)


def fband_table():
    """radset (longwave_radiation.f90:197-220): fband(100:400, 4) as [4, 301] -- flattened, the column-major Fortran array.
    (0.148 - 3.0e-6*(jtemp - 247)**2) is default real: float32 product and difference, widened, times eps1 in double."""
    eps1 = 1.0 - EPSLW
    fb = np.zeros((4, 301))
    jt = np.arange(200, 321)
    sq = lambda c: ((jt - c) ** 2).astype(np.float32)
    fb[1, 100:221] = (np.float32(0.148) - np.float32(3.0e-6) * sq(247)).astype(np.float64) * eps1
    fb[2, 100:221] = (np.float32(0.356) - np.float32(5.2e-6) * sq(282)).astype(np.float64) * eps1
    fb[3, 100:221] = (np.float32(0.314) + np.float32(1.0e-5) * sq(315)).astype(np.float64) * eps1
    fb[0, 100:221] = eps1 - (fb[1, 100:221] + fb[2, 100:221] + fb[3, 100:221])
    fb[:, :100] = fb[:, 100:101]
    fb[:, 221:] = fb[:, 220:221]
    return fb


FBAND = fband_table()


def nint(x):
    """Fortran nint: round half away from zero"""
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def fb(t, jb, clamp=True):
    """fband(nint(t), jb) (jb 1-based); the device clamps the index to [100, 400]"""
    n = nint(np.clip(t, 100.0, 400.0)) if clamp else nint(t)
    return FBAND[jb - 1, n - 100]


def zonal(sia_half, coa_half, tyear):
    """get_zonal_average_fields(tyear) + solar (shortwave_radiation.f90:238-329): fsol, ozone, ozupp, zenit, stratz per latitude
    [il], j = 0 southernmost (sia(j) = -sia_half(j), sia(il+1-j) = sia_half(j), coa symmetric)."""
    iy = len(sia_half)
    sia = np.concatenate([-np.asarray(sia_half), np.asarray(sia_half)[::-1]])
    coa = np.concatenate([np.asarray(coa_half[:iy]), np.asarray(coa_half[:iy])[::-1]])
    asin1 = f32(np.arcsin(np.float32(1.0)))
    alpha = f32(np.float32(4.0) * np.float32(np.arcsin(np.float32(1.0)))) * (tyear + f32(np.float32(10.0) / np.float32(365.0)))
    coz1 = 1.0 * max(0.0, math.cos(alpha - 0.0))
    coz2, azen, fs0 = f32(1.8), 1.0, 6.0
    rzen = -(math.cos(alpha) * f32(23.45) * asin1 / 90.0)
    # solar(tyear, 4.0*solc, topsr)
    csol = 4.0 * SOLC
    pigr = 2.0 * asin1
    a = 2.0 * pigr * tyear
    ca1, sa1 = math.cos(a), math.sin(a)
    ca2 = ca1 * ca1 - sa1 * sa1
    sa2 = 2. * sa1 * ca1
    ca3 = ca1 * ca2 - sa1 * sa2
    sa3 = sa1 * ca2 + sa2 * ca1
    decl = (f32(0.006918) - f32(0.399912) * ca1 + f32(0.070257) * sa1 - f32(0.006758) * ca2 + f32(0.000907) * sa2
            - f32(0.002697) * ca3 + f32(0.001480) * sa3)
    fdis = f32(1.000110) + f32(0.034221) * ca1 + f32(0.001280) * sa1 + f32(0.000719) * ca2 + f32(0.000077) * sa2
    cdecl, sdecl = math.cos(decl), math.sin(decl)
    tdecl = sdecl / cdecl
    csolp = csol / pigr
    out = {n: np.zeros(len(sia)) for n in ("fsol", "ozone", "ozupp", "zenit", "stratz")}
    for j in range(len(sia)):
        s, c = float(sia[j]), float(coa[j])
        ch0 = min(1.0, max(-1.0, -(tdecl * s / c)))
        h0 = math.acos(ch0)
        sh0 = math.sin(h0)
        topsr = csolp * fdis * (h0 * s * sdecl + sh0 * c * cdecl)
        flat2 = 1.5 * (s * s) - 0.5
        fsol = topsr
        ozupp = 0.5 * EPSSW
        ozone = f32(0.4) * EPSSW * (1.0 + coz1 * s + coz2 * flat2)
        zb = 1.0 - (c * math.cos(rzen) + s * math.sin(rzen))
        zenit = 1.0 + azen * (zb * zb)                          # **nzen with nzen = 2.0: zb*zb in the reference's build
        out["fsol"][j] = fsol
        out["ozupp"][j] = fsol * ozupp * zenit
        out["ozone"][j] = fsol * ozone * zenit
        out["zenit"][j] = zenit
        out["stratz"][j] = max(fs0 - fsol, 0.0)
    return out


def _margin(a, b, exact=False):
    return moist._margin(a, b, exact)


def _tie(t, exact=False):
    """relative distance of t from the nearest half-integer (a tie of nint); exact=True marks an input temperature (class (i) of
    tests/thresholds.py: nint's rounding half away from zero decides), clear inside moist.exact_ties()"""
    if exact and moist.EXACT_TIES:
        return np.full(np.shape(t), np.inf)
    return np.abs(t - (np.floor(t) + 0.5)) / np.maximum(np.abs(t), 1.0)


def down(tab, tg, qg, phig, pslg, rh, precnv, precls, iptop, fmask, albsfc, zon, compute_sw, state):
    """physics.f90:146-166 on [kx, ncol] columns.  zon: dict of the zonal fields per column [ncol].  state: dict (updated in place;
    a fresh one is {}): tau2 [4, kx, ncol], stratc [2, ncol], tt_rsw [kx, ncol], flux [4, ncol], dfabs [kx, ncol].  Returns the
    outputs (slrd; with compute_sw cloudc, clstr, icltop, ssrd, ssr, tsr, tt_rsw), `margin` and, with compute_sw, `branch_cols`."""
    kx = tab["kx"]
    nl1, nlp = kx - 1, kx + 1
    dhs, fsg, grdscp, wvi2 = tab["dhs"], tab["fsg"], tab["grdscp"], tab["wvi"][1]
    tg = np.asarray(tg, np.float64)
    n = tg.shape[1]
    psg = np.exp(pslg)
    rps = 1.0 / psg
    qa = np.maximum(qg, 0.0)
    out = {}
    margin = np.min(_tie(tg, exact=True), axis=0)
    if compute_sw:
        se = CP * tg + phig
        gse = (se[kx - 2] - se[kx - 1]) / (phig[kx - 2] - phig[kx - 1])
        # clouds
        rrcl = 1. / (RHCL2 - RHCL1)
        c = rh[nl1 - 1] > RHCL1
        margin = np.minimum(margin, _margin(rh[nl1 - 1], np.full(n, RHCL1)))
        cloudc = np.where(c, rh[nl1 - 1] - RHCL1, 0.0)
        icltop = np.where(c, nl1, nlp)
        qacl_open = np.zeros(n, bool)        # qa within one ulp of qacl at a level where the other half of the test holds
        for k in range(3, kx - 1):
            drh = rh[k - 1] - RHCL1
            margin = np.minimum(margin, np.minimum(_margin(drh, cloudc), _margin(qa[k - 1], np.full(n, QACL), exact=True)))
            up = (drh > cloudc) & (qa[k - 1] > QACL)
            qacl_open |= (drh > cloudc) & (np.abs(qa[k - 1] - QACL) <= np.spacing(QACL))
            cloudc = np.where(up, drh, cloudc)
            icltop = np.where(up, k, icltop)
        pr1 = np.minimum(PMAXCL, f32(86.4) * (precnv + precls))
        m = np.minimum(1.0, cloudc * rrcl)
        cloudc = np.minimum(1.0, WPCL * np.sqrt(pr1) + m * m)
        icl_rh = icltop
        icltop = np.minimum(iptop, icltop)
        qcloud = qa[nl1 - 1]
        clfact, rgse = f32(1.2), 1.0 / (GSE_S1 - GSE_S0)
        fstab = np.maximum(0.0, np.minimum(1.0, rgse * (gse - GSE_S0)))
        clstr = fstab * np.maximum(CLSMAX - clfact * cloudc, 0.0)
        clsea = clstr
        clstrl = np.maximum(clstr, CLSMINL) * rh[kx - 1]
        clstr = clstr + fmask * (clstrl - clstr)

        # get_shortwave_rad_fluxes
        fband2 = f32(0.05)
        fband1 = 1.0 - fband2
        tau2 = np.zeros((4, kx, n))
        flux = np.zeros((4, n))
        dfabs = np.zeros((kx, n))
        for k in range(1, kx + 1):
            tau2[2, k - 1] = np.where(icltop == k, ALBCL * cloudc, 0.0)
        tau2[2, kx - 1] = ALBCLS * clstr
        psaz = psg * zon["zenit"]
        acloud = cloudc * np.minimum(ABSCL1 * qcloud, ABSCL2)
        tau2[0, 0] = np.exp(-psaz * dhs[0] * ABSDRY)
        for k in range(2, nl1 + 1):
            abs1 = ABSDRY + ABSAER * fsg[k - 1] ** 2
            tau2[0, k - 1] = np.where(k >= icltop, np.exp(-psaz * dhs[k - 1] * (abs1 + ABSWV1 * qa[k - 1] + acloud)),
                                      np.exp(-psaz * dhs[k - 1] * (abs1 + ABSWV1 * qa[k - 1])))
        abs1 = ABSDRY + ABSAER * fsg[kx - 1] ** 2
        tau2[0, kx - 1] = np.exp(-psaz * dhs[kx - 1] * (abs1 + ABSWV1 * qa[kx - 1]))
        for k in range(2, kx + 1):
            tau2[1, k - 1] = np.exp(-psaz * dhs[k - 1] * ABSWV2 * qa[k - 1])
        fsol = zon["fsol"]
        ftop = fsol
        flux[0] = fsol * fband1
        flux[1] = fsol * fband2
        for k, oz in ((1, zon["ozupp"]), (2, zon["ozone"])):
            dfabs[k - 1] = flux[0]
            flux[0] = tau2[0, k - 1] * (flux[0] - oz * psg)
            dfabs[k - 1] = dfabs[k - 1] - flux[0]
        for k in range(3, kx + 1):
            tau2[2, k - 1] = flux[0] * tau2[2, k - 1]
            flux[0] = flux[0] - tau2[2, k - 1]
            dfabs[k - 1] = flux[0]
            flux[0] = tau2[0, k - 1] * flux[0]
            dfabs[k - 1] = dfabs[k - 1] - flux[0]
        for k in range(2, kx + 1):
            dfabs[k - 1] = dfabs[k - 1] + flux[1]
            flux[1] = tau2[1, k - 1] * flux[1]
            dfabs[k - 1] = dfabs[k - 1] - flux[1]
        fsfcd = flux[0] + flux[1]
        flux[0] = flux[0] * albsfc
        fsfc = fsfcd - flux[0]
        for k in range(kx, 0, -1):
            dfabs[k - 1] = dfabs[k - 1] + flux[0]
            flux[0] = tau2[0, k - 1] * flux[0]
            dfabs[k - 1] = dfabs[k - 1] - flux[0]
            flux[0] = flux[0] + tau2[2, k - 1]
        ftop = ftop - flux[0]
        # 5. longwave transmissivities
        for k in (1,):
            tau2[0, k - 1] = np.exp(-psg * dhs[k - 1] * ABLWIN)
            tau2[1, k - 1] = np.exp(-psg * dhs[k - 1] * ABLCO2)
            tau2[2, k - 1] = 1.0
            tau2[3, k - 1] = 1.0
        for k in range(2, kx + 1, kx - 2):                        # do k = 2, kx, kx - 2: levels 2 and kx
            tau2[0, k - 1] = np.exp(-psg * dhs[k - 1] * ABLWIN)
            tau2[1, k - 1] = np.exp(-psg * dhs[k - 1] * ABLCO2)
            tau2[2, k - 1] = np.exp(-psg * dhs[k - 1] * ABLWV1 * qa[k - 1])
            tau2[3, k - 1] = np.exp(-psg * dhs[k - 1] * ABLWV2 * qa[k - 1])
        acloud = cloudc * ABLCL2
        for k in range(3, nl1 + 1):
            deltap = psg * dhs[k - 1]
            acloud1 = np.where(k < icltop, acloud, ABLCL1 * cloudc)
            tau2[0, k - 1] = np.exp(-deltap * (ABLWIN + acloud1))
            tau2[1, k - 1] = np.exp(-deltap * ABLCO2)
            tau2[2, k - 1] = np.exp(-deltap * np.maximum(ABLWV1 * qa[k - 1], acloud))
            tau2[3, k - 1] = np.exp(-deltap * np.maximum(ABLWV2 * qa[k - 1], acloud))
        eps1 = EPSLW / (dhs[0] + dhs[1])
        state["tau2"] = tau2
        state["stratc"] = np.stack([zon["stratz"] * psg, eps1 * psg])
        tt_rsw = np.stack([dfabs[k] * rps * grdscp[k] for k in range(kx)])
        state["tt_rsw"] = tt_rsw
        out.update(cloudc=cloudc, clstr=clstr, icltop=icltop.astype(np.int32), ssrd=fsfcd, ssr=fsfc, tsr=ftop, tt_rsw=tt_rsw)
        out["branch_cols"] = {"cltop_nl1": icltop == nl1, "cltop_mid": (icltop >= 3) & (icltop <= kx - 2),
                              "cltop_iptop": iptop < icl_rh, "cltop_2": icltop == 2, "cltop_none": icltop == nlp,
                              "strat_land": (fmask > 0) & (clstr > 0), "strat_sea": (fmask < 1) & (clsea > 0),
                              "polar_night": zon["stratz"] > 0, "fband_low": np.any(nint(tg) < 200, axis=0)}
        out["ties"] = {"qacl_open": qacl_open, "icl_rh": icl_rh, "cloudc_rh": m, "pr1": pr1}

    # get_downward_longwave_rad_fluxes
    tau2 = state["tau2"]
    st4a = blackbody(tab, tg)
    flux = np.zeros((4, n))
    dfabs = np.zeros((kx, n))
    fsfcd = np.zeros(n)
    k = 1
    for jb in (1, 2):
        emis = 1.0 - tau2[jb - 1, k - 1]
        brad = fb(tg[k - 1], jb) * (st4a[0, k - 1] + emis * st4a[1, k - 1])
        flux[jb - 1] = emis * brad
        dfabs[k - 1] = dfabs[k - 1] - flux[jb - 1]
    flux[2:] = 0.0
    for jb in range(1, 5):
        for k in range(2, kx + 1):
            emis = 1.0 - tau2[jb - 1, k - 1]
            brad = fb(tg[k - 1], jb) * (st4a[0, k - 1] + emis * st4a[1, k - 1])
            dfabs[k - 1] = dfabs[k - 1] + flux[jb - 1]
            flux[jb - 1] = tau2[jb - 1, k - 1] * flux[jb - 1] + emis * brad
            dfabs[k - 1] = dfabs[k - 1] - flux[jb - 1]
    for jb in range(1, 5):
        fsfcd = fsfcd + EMISFC * flux[jb - 1]
    corlw = EPSLW * EMISFC * st4a[0, kx - 1]
    dfabs[kx - 1] = dfabs[kx - 1] - corlw
    fsfcd = fsfcd + corlw
    state["flux"] = flux
    state["dfabs"] = dfabs
    state["slrd"] = fsfcd
    out["slrd"] = fsfcd
    out["margin"] = margin
    return out


def blackbody(tab, ta):
    """longwave_radiation.f90:38-66: st4a [2, kx, ncol]; ta**4.0 is a pow call in the reference's build, ta**3.0 ta*(ta*ta)"""
    kx = tab["kx"]
    wvi2 = tab["wvi"][1]
    st4a = np.zeros((2,) + ta.shape)
    for k in range(1, kx):
        st4a[0, k - 1] = ta[k - 1] + wvi2[k - 1] * (ta[k] - ta[k - 1])
    st4a[1, 0] = 0.75 * ta[0] + 0.25 * st4a[0, 0]
    st4a[1, 1] = 0.50 * ta[1] + 0.25 * (st4a[0, 0] + st4a[0, 1])
    anis = 1.0
    for k in range(3, kx):
        st4a[1, k - 1] = 0.5 * anis * np.maximum(st4a[0, k - 1] - st4a[0, k - 2], 0.0)
    st4a[1, kx - 1] = anis * np.maximum(ta[kx - 1] - st4a[0, kx - 2], 0.0)
    for k in (1, 2):
        st4a[0, k - 1] = SBC * np.power(st4a[1, k - 1], 4.0)
        st4a[1, k - 1] = 0.0
    for k in range(3, kx + 1):
        st3a = SBC * (ta[k - 1] * (ta[k - 1] * ta[k - 1]))
        st4a[0, k - 1] = st3a * ta[k - 1]
        st4a[1, k - 1] = 4.0 * st3a * st4a[1, k - 1]
    return st4a


def up(tab, tg, pslg, ts, fsfcu, state, ttend):
    """physics.f90:180-186: get_upward_longwave_rad_fluxes and the tendency.  Returns slr, olr, tt_rlw and the new ttend."""
    kx = tab["kx"]
    dhs, grdscp = tab["dhs"], tab["grdscp"]
    tau2, stratc = state["tau2"], state["stratc"]
    st4a = blackbody(tab, tg)
    flux = state["flux"].copy()
    dfabs = state["dfabs"].copy()
    refsfc = 1.0 - EMISFC
    fsfc = fsfcu - state["slrd"]
    for jb in range(1, 5):
        flux[jb - 1] = fb(ts, jb) * fsfcu + refsfc * flux[jb - 1]
    dfabs[kx - 1] = dfabs[kx - 1] + EPSLW * fsfcu
    for jb in range(1, 5):
        for k in range(kx, 1, -1):
            emis = 1.0 - tau2[jb - 1, k - 1]
            brad = fb(tg[k - 1], jb) * (st4a[0, k - 1] - emis * st4a[1, k - 1])
            dfabs[k - 1] = dfabs[k - 1] + flux[jb - 1]
            flux[jb - 1] = tau2[jb - 1, k - 1] * flux[jb - 1] + emis * brad
            dfabs[k - 1] = dfabs[k - 1] - flux[jb - 1]
    k = 1
    for jb in (1, 2):
        emis = 1.0 - tau2[jb - 1, k - 1]
        brad = fb(tg[k - 1], jb) * (st4a[0, k - 1] - emis * st4a[1, k - 1])
        dfabs[k - 1] = dfabs[k - 1] + flux[jb - 1]
        flux[jb - 1] = tau2[jb - 1, k - 1] * flux[jb - 1] + emis * brad
        dfabs[k - 1] = dfabs[k - 1] - flux[jb - 1]
    corlw1 = dhs[0] * stratc[1] * st4a[0, 0] + stratc[0]
    corlw2 = dhs[1] * stratc[1] * st4a[0, 1]
    dfabs[0] = dfabs[0] - corlw1
    dfabs[1] = dfabs[1] - corlw2
    ftop = corlw1 + corlw2
    for jb in range(1, 5):
        ftop = ftop + flux[jb - 1]
    psg = np.exp(pslg)
    rps = 1.0 / psg
    tt_rlw = np.stack([dfabs[k] * rps * grdscp[k] for k in range(kx)])
    return {"slr": fsfc, "olr": ftop, "tt_rlw": tt_rlw, "ttend": ttend + state["tt_rsw"] + tt_rlw, "margin": _tie(ts)}


# ---------------------------------------------------------------------------------------------------- seeded inputs
def _draw(tab, ncol, seed):
    """One draw: moist.py's columns, 8 % of them dried (no cloud, no precipitation), the surface fields and the second step's
    inputs.  Everything [kx, ncol] or [ncol]."""
    kx = tab["kx"]
    tg, qg, phig, pslg, ttend, qtend = moist._draw(kx, tab["fsg"], ncol, seed)
    u = synth.splitmix64(seed + 0x5A17, ncol * (kx + 8)).reshape(kx + 8, ncol)
    qg = np.where(u[0] < 0.08, 0.05 * qg, qg)
    fmask = np.where(u[1] < 1 / 3, 0.0, np.where(u[1] < 2 / 3, 1.0, u[2]))
    albsfc = 0.07 + 0.6 * u[3]
    ts = tg[-1] + 6.0 * u[4] - 3.0
    fsfcu = EMISFC * SBC * (tg[-1] + 6.0 * u[5] - 3.0) ** 4
    # the step without shortwave: the same columns 0.5 K warmer or colder per level, a new surface and a new ttend
    tg2 = tg + (u[8:8 + kx] - 0.5)
    ts2 = ts + (2.0 * u[6] - 1.0)
    fsfcu2 = fsfcu * (1.0 + 0.02 * (2.0 * u[7] - 1.0))
    return {"tg": tg, "qg": qg, "phig": phig, "pslg": pslg, "ttend": ttend, "qtend": qtend, "fmask": fmask, "albsfc": albsfc,
            "ts": ts, "fsfcu": fsfcu, "tg2": tg2, "ts2": ts2, "fsfcu2": fsfcu2, "ttend2": ttend[::-1].copy()}


MIN_MARGIN = 1e-9


def _with_moist(tab, d, zon):
    m = moist.column_block(tab, d["tg"], d["qg"], d["phig"], d["pslg"], d["ttend"], d["qtend"])
    d = dict(d, rh=m["rh"], precnv=m["precnv"], precls=m["precls"], iptop=m["iptop"], ttend_m=m["ttend"])
    r = down(tab, d["tg"], d["qg"], d["phig"], d["pslg"], d["rh"], d["precnv"], d["precls"], d["iptop"], d["fmask"], d["albsfc"],
             zon, True, {})
    margin = np.minimum(np.minimum(m["margin"], r["margin"]), np.minimum(_tie(d["ts"]), _tie(d["ts2"])))
    margin = np.minimum(margin, np.min(_tie(d["tg2"]), axis=0))
    return d, margin


def columns(tab, ncol, seed, zon):
    """ncol columns with every input of both steps (dict of [kx, ncol] / [ncol]; rh, precnv, precls, iptop and the moist ttend_m
    from moist.column_block).  A column with any decision (moist or radiation, nint ties included) within MIN_MARGIN of its
    threshold is drawn again from the next stream.  zon: the zonal fields per column (zonal_columns)."""
    d = _draw(tab, ncol, seed)
    for attempt in range(1, 50):
        full, margin = _with_moist(tab, d, zon)
        bad = np.nonzero(margin < MIN_MARGIN)[0]
        if bad.size == 0:
            return full
        new = _draw(tab, ncol, seed + 7919 * attempt)
        for k in d:
            d[k][..., bad] = new[k][..., bad]
    raise RuntimeError("could not draw columns clear of ties")


def zonal_columns(z, nb, il, ix):
    """the zonal fields of one date ([il] each) per column of nb (il, ix) states"""
    return {k: np.tile(np.repeat(np.asarray(v), ix), nb) for k, v in z.items()}


def grids(a, nb, il, ix):
    """[kx, ncol] -> [nb, kx, il, ix]; [ncol] -> [nb, il, ix]"""
    a = np.asarray(a)
    if a.ndim == 1:
        return np.ascontiguousarray(a.reshape(nb, il, ix))
    return np.ascontiguousarray(np.moveaxis(a.reshape(a.shape[0], nb, il, ix), 0, 1))


def cols(a):
    """[nb, kx, il, ix] -> [kx, ncol]; [nb, il, ix] -> [ncol]"""
    a = np.asarray(a)
    if a.ndim == 3:
        return a.reshape(-1)
    return np.moveaxis(a, 1, 0).reshape(a.shape[1], -1)


def two_steps(tab, c, zon):
    """The recorded sequence on columns c (columns()): a shortwave step (down with compute_sw, up) on the first inputs, then a
    step without shortwave on the second (tg2, ts2, fsfcu2, ttend2) with the state held.  Returns (step1, step2) output dicts."""
    st = {}
    r1 = down(tab, c["tg"], c["qg"], c["phig"], c["pslg"], c["rh"], c["precnv"], c["precls"], c["iptop"], c["fmask"], c["albsfc"],
              zon, True, st)
    r1.update(up(tab, c["tg"], c["pslg"], c["ts"], c["fsfcu"], st, c["ttend_m"]))
    r2 = down(tab, c["tg2"], c["qg"], c["phig"], c["pslg"], None, None, None, None, None, None, zon, False, st)
    r2.update(up(tab, c["tg2"], c["pslg"], c["ts2"], c["fsfcu2"], st, c["ttend2"]))
    return r1, r2


SW_OUT = ("cloudc", "clstr", "ssrd", "ssr", "tsr", "slrd", "slr", "olr", "tt_rsw", "tt_rlw", "ttend")
NOSW_OUT = ("slrd", "slr", "olr", "tt_rlw", "ttend")
