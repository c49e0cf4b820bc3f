"""The slab land, sea and ice models and the daily forcing: the reference side of tests/test_gpu_surfmodel.py.

NumPy restatements, per column, of date.f90:109-157 (newdate and imont1, tmonth, tyear), interpolation.f90:16-69 (forint,
forin5), the constant fields of land_model_init (land_model.f90:75-87, :141-180) and sea_model_init (sea_model.f90:137-150,
:204-250), couple_land_atm with run_land_model (land_model.f90:184-239), couple_sea_atm with run_sea_model and obs_ssta
(sea_model.f90:253-444) and set_forcing parts 2 and 4 (forcing.f90:55-62, :84-97), with the reference's float32 literals
(SURVEY.md App. A); pinned to the flang-built reference by tests/golden/ref_surfmodel.npz.

The stock run reads its climatologies from files.  climatology() makes seeded ones over an orography from longrun.boundary's
formulas: a seasonal cycle on the land and sea temperatures, an ice fraction where the sea is cold, snow where the land is, alb0
on both sides of 0.4, the land fraction on both sides of thrsh and flandmin.  sstan_month(k) is month k of the "file" of SST
anomalies.  Driver: run() follows the main loop's cadence (speedy.f90:27-54): set_forcing(1) on the first step of a day, the step
(here: seeded flux fields), newdate, couple_sea_land(1 + model_step/nsteps)."""
import numpy as np

import longrun
import moist
import synth

f32 = moist.f32
NSTEPS = 36                                           # params.f90:30
DELT = float(np.float32(86400.0) / np.float32(NSTEPS))  # params.f90:31
ISSTY0 = 1979                                         # params.f90:43
NCAL365 = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
SSTFR = float(np.float32(273.2) - np.float32(1.8))   # sea_model.f90:285, :400: a float32 difference
ALBSEA, ALBICE, ALBSN, EMISFC = f32(0.07), f32(0.60), f32(0.60), f32(0.98)   # mod_radcon.f90:22-27
SBC, ALHC, SD2SC, REFRH1, GAMMA = f32(5.67e-8), f32(2501.0), f32(60.0), f32(0.7), f32(6.0)
THRSH, THIRD = f32(0.1), float(np.float32(1.0) / np.float32(3.0))
LAND, ICE, SSTAN, DEFAULT = 1, 2, 4, 7                # the flags of include/spdy.h
TABLES = ("fmask_l", "fmask_s", "rhcapl", "cdland", "rhcaps", "rhcapi", "cdsea", "cdice")
FIELDS = ("stlcl_ob", "snowdcl_ob", "soilwcl_ob", "stl_lm", "stl_am", "snowd_am", "soilw_am", "sstcl_ob", "sicecl_ob", "ticecl_ob",
          "sstan_ob", "sst_om", "tice_om", "sice_om", "sst_am", "sstan_am", "sice_am", "tice_am", "ssti_om")
FORCING = ("snowc", "alb_l", "alb_s", "albsfc", "corh")
CLIM12 = ("stl12", "snowd12", "soilw12", "sst12", "sice12")
# the three date windows of about three days (108 steps): tmonth crossing 0.5, a month change with obs_ssta, the turn of the year
WINDOWS = {"midmonth": (1982, 1, 15), "month": (1982, 1, 30), "year": (1982, 12, 30)}
WINDOW_STEPS = 3 * NSTEPS


# ------------------------------------------------------------------------------------------------ date.f90
class Date:
    """model_datetime with imont1, tmonth, tyear (date.f90:96-105, :109-157; iseasc = 1, the 365-day calendar)"""

    def __init__(self, year, month, day, hour=0, minute=0):
        self.start_year = year
        self.year, self.month, self.day, self.hour, self.minute = year, month, day, hour, minute
        self._derive()

    def _derive(self):
        before = sum(NCAL365[:self.month - 1])
        self.imont1 = self.month
        # (day - 0.5)/float(ndaycal): default reals
        self.tmonth = float(np.float32(self.day - 0.5) / np.float32(NCAL365[self.month - 1]))
        self.tyear = float(np.float32(before + self.day - 0.5) / np.float32(365))

    def newdate(self):
        self.minute += 24 * 60 // NSTEPS
        if self.minute >= 60:
            self.minute %= 60
            self.hour += 1
        if self.hour >= 24:
            self.hour %= 24
            self.day += 1
        if self.year % 4 == 0 and self.month == 2:
            if self.day > 29:
                self.day, self.month = 1, self.month + 1
        elif self.day > NCAL365[self.month - 1]:
            self.day, self.month = 1, self.month + 1
        if self.month > 12:
            self.month, self.year = 1, self.year + 1
        self._derive()

    def key(self):
        return (self.year, self.month, self.day)


def weights(imont1, tmonth):
    """forin5's 0-based months m5 and weights w5 (wm2 wm1 w0 wp1 wp2), forint's months m2 and weight wmon, and s2, the second
    slot of forint(2, sstan3) (interpolation.f90:16-69; c0 = 1.0/12.0 is a float32 quotient)"""
    imon = imont1 - 1
    c0 = float(np.float32(1.0) / np.float32(12.0))
    t0, t1, t2 = c0 * tmonth, c0 * (1.0 - tmonth), 0.25 * tmonth * (1 - tmonth)
    w5 = (-t1 + t2, -c0 + 8 * t1 - 6 * t2, 7 * c0 + 10 * t2, -c0 + 8 * t0 - 6 * t2, -t0 + t2)
    m5 = tuple((imon + k - 2) % 12 for k in range(5))
    if tmonth <= 0.5:
        return {"w5": w5, "m5": m5, "m2": (imon, (imon - 1) % 12), "s2": 0, "wmon": 0.5 - tmonth}
    return {"w5": w5, "m5": m5, "m2": (imon, (imon + 1) % 12), "s2": 2, "wmon": tmonth - 0.5}


def forin5(w, a):
    m, c = w["m5"], w["w5"]
    return c[0] * a[m[0]] + c[1] * a[m[1]] + c[2] * a[m[2]] + c[3] * a[m[3]] + c[4] * a[m[4]]


def forint(w, a, m0=None, m1=None):
    m0, m1 = (w["m2"] if m0 is None else (m0, m1))
    return a[m0] + w["wmon"] * (a[m1] - a[m0])


# ------------------------------------------------------------------------------------------------ the constant fields
def tables(fmask, alb0, sia_half, ix, delt=DELT):
    """land_model.f90:75-87, :141-180 and sea_model.f90:137-150, :204-250 for fmask, alb0 [il * ix] (j = 0 southernmost)"""
    il = 2 * len(sia_half)
    fl = np.where(fmask >= THRSH, np.where(fmask > 1.0 - THRSH, 1.0, fmask), 0.0)
    fs0 = 1.0 - fmask
    fs = np.where(fs0 >= THRSH, np.where(fs0 > 1.0 - THRSH, 1.0, fs0), 0.0)
    hcapl, hcapli, tdland = 1.0 * f32(2.50e+6), f32(5.0) * f32(1.93e+6), f32(40.0)
    dmask = np.where(fl < THIRD, 0.0, 1.0)
    t = {"fmask_l": fl, "fmask_s": fs, "rhcapl": np.where(alb0 < f32(0.4), delt / hcapl, delt / hcapli),
         "cdland": dmask * tdland / (1. + dmask * tdland)}
    s = np.asarray(sia_half, np.float64)
    radang = np.concatenate([-np.arcsin(s), np.arcsin(s)[::-1]])                           # geometry.f90:74-75
    asin1 = np.arcsin(np.float32(1.0))
    deglat = radang * 90.0 / float(asin1)
    coslat = np.cos(float(asin1 / np.float32(90.0)) * deglat)
    hcaps = f32(4.18e+6) * (f32(60.0) + (f32(40.0) - f32(60.0)) * (coslat * coslat * coslat))
    hcapi = f32(1.93e+6) * (f32(2.5) + (f32(1.5) - f32(2.5)) * (coslat * coslat))
    dm = np.ones((il, ix))                                                                 # l_globe
    dm[1:-1] = 0.25 * (dm[:-2] + 2 * dm[1:-1] + dm[2:])
    dm = np.where(fs < THIRD, 0.0, dm.reshape(-1))
    tdsst, tdice = f32(90.0), f32(30.0)
    t.update(rhcaps=np.repeat(delt / hcaps, ix), rhcapi=np.repeat(delt / hcapi, ix), cdsea=dm * tdsst / (1. + dm * tdsst),
             cdice=dm * tdice / (1. + dm * tdice))
    return t


# ------------------------------------------------------------------------------------------------ the models
class Model:
    """The module state of land_model and sea_model (fields [ncol]) and mod_radcon's surface fields.  clim: fmask, alb0 [ncol],
    stl12 .. sice12 [12, ncol], sstan3 [3, ncol]; tab: tables(); ssta(k): month k of the anomaly file [ncol] (obs_ssta)."""

    def __init__(self, clim, tab, flags=DEFAULT, ssta=None, start_year=1982):
        self.c, self.t, self.flags, self.ssta, self.start_year = clim, tab, flags, ssta, start_year
        n = clim["fmask"].size
        self.sstan3 = np.array(clim["sstan3"], copy=True) if flags & SSTAN else np.zeros((3, n))
        self.f = {k: np.zeros(n) for k in FIELDS + FORCING}
        self.margin = np.inf                # the smallest |sstcl_ob - sstfr| before the adjustment, over all calls
        self.branch = {k: np.zeros(n, bool) for k in ("warm", "cold", "warm_ice", "warm_noice", "snow_clamped", "snow_free")}

    def couple(self, day, date, flux=None):
        """couple_sea_land(day) at the date `date` (a Date; obs_ssta runs where the reference runs it).  flux: hfluxn [2, ncol],
        shf, evap [3, ncol], ssrd [ncol] of the step before.  Returns True where obs_ssta has replaced the anomaly window."""
        f, c, t, w = self.f, self.c, self.t, weights(date.imont1, date.tmonth)
        # couple_land_atm
        f["stlcl_ob"], f["snowdcl_ob"], f["soilwcl_ob"] = forin5(w, c["stl12"]), forint(w, c["snowd12"]), forint(w, c["soilw12"])
        if day == 0:
            f["stl_lm"] = f["stlcl_ob"].copy()
            f["stl_am"] = f["stlcl_ob"].copy()
        elif self.flags & LAND:
            tanom = f["stl_lm"] - f["stlcl_ob"]
            tanom = t["cdland"] * (tanom + t["rhcapl"] * flux["hfluxn"][0])
            f["stl_lm"] = tanom + f["stlcl_ob"]
            f["stl_am"] = f["stl_lm"].copy()
        else:
            f["stl_am"] = f["stlcl_ob"].copy()
        f["snowd_am"], f["soilw_am"] = f["snowdcl_ob"].copy(), f["soilwcl_ob"].copy()
        # couple_sea_atm
        sstcl, sicecl = forin5(w, c["sst12"]), forint(w, c["sice12"])
        shifted = False
        if self.flags & SSTAN:
            if date.day == 1 and day > 0:                            # obs_ssta: on EVERY call of the month's first day
                next_month = (self.start_year - ISSTY0) * 12 + date.month
                self.sstan3 = np.stack([self.sstan3[1], self.sstan3[2], self.ssta(next_month)])
                shifted = True
            f["sstan_ob"] = forint(w, self.sstan3, 1, w["s2"])
        self.margin = min(self.margin, float(np.abs(sstcl - SSTFR).min()))
        warm = sstcl > SSTFR
        self.branch["warm"] |= warm
        self.branch["cold"] |= ~warm
        sw = np.minimum(0.5, sicecl)
        self.branch["warm_ice"] |= warm & (sw > 0.0)
        self.branch["warm_noice"] |= warm & ~(sw > 0.0)
        sc = np.maximum(0.5, sicecl)
        with np.errstate(divide="ignore", invalid="ignore"):
            f["sstcl_ob"] = np.where(warm, np.where(sw > 0.0, SSTFR + (sstcl - SSTFR) / (1.0 - sw), sstcl), SSTFR)
            f["ticecl_ob"] = np.where(warm, SSTFR, SSTFR + (sstcl - SSTFR) / sc)
        f["sicecl_ob"] = np.where(warm, sw, sc)
        if day == 0:
            f["sst_om"] = np.zeros_like(sstcl)                        # sea_coupling_flag <= 0
            f["tice_om"], f["sice_om"] = f["ticecl_ob"].copy(), f["sicecl_ob"].copy()
        elif self.flags & ICE:
            self._run_sea_model(flux)
        f["sstan_am"] = f["sstan_ob"].copy() if self.flags & SSTAN else np.zeros_like(sstcl)
        sst_am = f["sstcl_ob"] + f["sstan_am"]
        ice = bool(self.flags & ICE)
        f["sice_am"] = (f["sice_om"] if ice else f["sicecl_ob"]).copy()
        f["tice_am"] = (f["tice_om"] if ice else f["ticecl_ob"]).copy()
        f["sst_am"] = sst_am + f["sice_am"] * (f["tice_am"] - sst_am)
        f["ssti_om"] = f["sst_om"] + f["sice_am"] * (f["tice_am"] - f["sst_om"])
        return shifted

    def _run_sea_model(self, flux):
        f, t = self.f, self.t
        hfl2 = flux["hfluxn"][1]
        difice = ((ALBSEA - ALBICE) * flux["ssrd"] + EMISFC * SBC * (SSTFR ** 4.0 - f["tice_am"] ** 4.0) + flux["shf"][1] +
                  flux["evap"][1] * ALHC)
        hflux_i = hfl2 + difice * (1.0 - f["sice_am"])
        hflux = hfl2 - 0.0 - f["sicecl_ob"] * (hflux_i + 1.0 * (SSTFR - f["tice_om"]))
        tanom = f["sst_om"] - f["sstcl_ob"]
        tanom = t["cdsea"] * (tanom + t["rhcaps"] * hflux)
        f["sst_om"] = tanom + f["sstcl_ob"]
        hflux = hflux_i + 1.0 * (SSTFR - f["tice_om"])
        tanom = f["tice_om"] - f["ticecl_ob"]
        anom0 = f32(20.0)
        cdis = t["cdice"] * (anom0 / (anom0 + np.abs(tanom)))
        tanom = cdis * (tanom + t["rhcapi"] * hflux)
        f["tice_om"] = tanom + f["ticecl_ob"]
        f["sice_om"] = f["sicecl_ob"].copy()

    def forcing(self, phis0):
        """set_forcing parts 2 and 4 over the surface geopotential phis0 [ncol]; corh is what grid_to_spec turns into qcorh"""
        f, c, t = self.f, self.c, self.t
        sc = f["snowd_am"] / SD2SC
        self.branch["snow_clamped"] |= sc > 1.0
        self.branch["snow_free"] |= ~(sc > 1.0)
        f["snowc"] = np.minimum(1.0, sc)
        f["alb_l"] = c["alb0"] + f["snowc"] * (ALBSN - c["alb0"])
        f["alb_s"] = ALBSEA + f["sice_am"] * (ALBICE - ALBSEA)
        f["albsfc"] = f["alb_s"] + t["fmask_l"] * (f["alb_l"] - f["alb_s"])
        gamlat = GAMMA / (f32(1000.0) * moist.GRAV)
        pexp = 1. / (longrun_rgas() * gamlat)
        tsfc = t["fmask_l"] * f["stl_am"] + t["fmask_s"] * f["sst_am"]
        tref = tsfc + gamlat * phis0
        psfc = (tsfc / tref) ** pexp
        # get_qsat's sig <= 0 form divides by ps(1,1) - 0.378 qsat with ps = psfc/psfc: the sig > 0 form at sig = ps = 1
        qref = moist.get_qsat(tref, psfc / psfc, 1.0)
        qsfc = moist.get_qsat(tsfc, psfc, 1.0)
        f["corh"] = REFRH1 * (qref - qsfc)

    def boundary(self):
        """the fields spdy_surface_model_boundary hands out, under spdy_sfc_boundary's names, and albsfc"""
        f = self.f
        return {"fmask": self.t["fmask_l"], "sst": f["sst_am"], "stl": f["stl_am"], "soilw": f["soilw_am"], "snowc": f["snowc"],
                "alb_l": f["alb_l"], "alb_s": f["alb_s"], "albsfc": f["albsfc"]}


def longrun_rgas():
    """rgas = akap*cp (physical_constants.f90:23-24): akap = 2.0/7.0 is a float32 quotient"""
    return float(np.float32(2.0) / np.float32(7.0)) * moist.CP


# ------------------------------------------------------------------------------------------------ seeded inputs
CLIM_SEED = 5301


def orography(ex, seed=4242, height=2000.0):
    """longrun.rest_state's seeded orography [il, ix] with the transforms of ex (the oracle, or a plan)"""
    nx, mx, trunc = ex.nx, ex.mx, ex.trunc
    l = np.arange(mx)[None, :] + np.arange(nx)[:, None]
    oro = synth.spectra(1, trunc, first=seed)[0] * (1.0 / (1.0 + l)) ** 0.5
    oro[0, 0] = 0.0
    g = ex.spec_to_grid(oro, 1)
    return np.maximum(g, 0.0) * (longrun.GRAV * height / g.max())


def sstan_month(k, ncol, seed=CLIM_SEED):
    """month k (1-based, from January of ISSTY0) of the seeded file of SST anomalies: within +-1.5 K"""
    return 3.0 * (synth.splitmix64(seed + 1000 + k, ncol) - 0.5)


def climatology(phis0, lat, seed=CLIM_SEED, start=(1982, 1)):
    """Monthly climatologies over the orography phis0 [il, ix] at the latitudes lat [il], from longrun.boundary's annual fields:
    the temperatures get a seasonal cycle (warm in the northern July) and per-month noise, the polar sea is cooled below the
    freezing point, the sea ice follows the sea temperature (zero above 273.5 K), the snow depth the land temperature (above
    60 mm, where the cover is clamped, below about 260 K), alb0 rises with latitude past 0.4.  sstan3: the months around
    `start` as sea_model_init reads them."""
    il, ix = phis0.shape
    n = il * ix
    b = longrun.boundary(phis0, lat, seed)
    sl, s2 = np.repeat(np.sin(lat), ix), np.repeat(np.sin(lat) ** 2, ix)
    u = synth.splitmix64(seed + 1, 12 * 3 * n).reshape(12, 3, n)
    ua = synth.splitmix64(seed + 2, n)
    season = -np.cos(2.0 * np.pi * (np.arange(12) + 0.5) / 12.0)           # -1 in January, +1 in July
    stl12 = np.stack([b["stl"] + 9.0 * season[m] * sl + 0.4 * (u[m, 0] - 0.5) for m in range(12)])
    sst12 = np.stack([b["sst"] - 5.0 * s2 ** 4 + 2.5 * season[m] * sl + 0.4 * (u[m, 1] - 0.5) for m in range(12)])
    swl1 = np.stack([b["soilw"] * (0.8 + 0.2 * u[m, 2]) * 0.5 for m in range(12)])
    raw = {"stl12": stl12, "sst12": sst12, "snowd12": np.clip(268.0 - stl12, 0.0, None) * 8.0, "swl1": swl1,
           "sice12": np.clip((273.5 - sst12) / 4.0, 0.0, 1.0)}
    isst0 = (start[0] - ISSTY0) * 12 + start[1]
    raw["sstan3"] = np.stack([sstan_month(isst0 - 2 + m, n, seed) for m in (1, 2, 3)])
    c = after_init(b["fmask"], raw)
    c.update(fmask=b["fmask"], alb0=0.12 + 0.5 * s2 * (0.4 + 0.6 * ua))
    return c


RSW = 1.0 / (f32(0.30) + 3 * (f32(0.30) - f32(0.17)))      # land_model.f90:58-61, :115-119: swcap, swwil, idep2 = 3


def after_init(fmask, raw):
    """What land_model_init and sea_model_init make of the fields they read (the caller's part of spdy_surface_model_create):
    the soil water availability from the top layer's water content swl1 (land_model.f90:121-133 with no vegetation and a dry
    second layer: min(1, rsw*swl1)), max(icec, 0), and forchk's replacement wherever the binary mask of the model is 0
    (boundaries.f90:47-72: 273 K for the temperatures, 0 for the others).  fillsf changes nothing: no value is below 0.  Applying
    it twice changes nothing either, so the reference can be given these fields."""
    bl, bs = fmask >= THRSH, (1.0 - fmask) >= THRSH              # bmask_l, bmask_s
    c = {"stl12": np.where(bl, raw["stl12"], 273.0), "snowd12": np.where(bl, raw["snowd12"], 0.0),
         "sst12": np.where(bs, raw["sst12"], 273.0), "sice12": np.where(bs, np.maximum(raw["sice12"], 0.0), 0.0),
         "sstan3": np.where(bs, raw["sstan3"], 0.0), "swl1": raw["swl1"]}
    if "soilw12" in raw:
        c["soilw12"] = np.where(bl, raw["soilw12"], 0.0)
    else:
        c["soilw12"] = np.where(bl, np.minimum(1.0, RSW * (raw["swl1"] + 0.0 * np.maximum(0.0, 3 * 0.0 - 3 * f32(0.17)))), 0.0)
    return c


def ssta_reader(fmask, seed=CLIM_SEED):
    """obs_ssta's read of month k of the anomaly file, with its forchk"""
    bs = (1.0 - fmask) >= THRSH
    return lambda k: np.where(bs, sstan_month(k, fmask.size, seed), 0.0)


def fluxes(step, ncol, seed=CLIM_SEED):
    """the flux fields a step leaves for the surface models, seeded per step: hfluxn [2, ncol] (W/m2), shf, evap [3, ncol]
    (W/m2, g/(m2 s)), ssrd [ncol] (W/m2)"""
    u = synth.splitmix64(seed + 50000 + step, 9 * ncol).reshape(9, ncol)
    return {"hfluxn": 240.0 * (u[0:2] - 0.5), "shf": 80.0 * (u[2:5] - 0.4), "evap": 0.08 * u[5:8], "ssrd": 420.0 * u[8]}


# ------------------------------------------------------------------------------------------------ the main loop's cadence
def run(model, start, nsteps, phis0, flux_of, on_forcing=None, on_step=None):
    """initialize_coupler and set_forcing(0) at the date start = (year, month, day), then nsteps steps of speedy.f90:27-54:
    set_forcing(1) on the first step of a day, the step (flux_of(model_step) -> the fluxes it leaves), newdate,
    couple_sea_land(1 + model_step/nsteps).  on_forcing(model_step, date) after every forcing (model_step 0: set_forcing(0)),
    on_step(model_step, day, date, flux, shifted) after every couple (model_step 0: initialize_coupler)."""
    date = Date(*start)
    model.start_year = start[0]
    model.couple(0, date)
    if on_step:
        on_step(0, 0, date, None, False)
    model.forcing(phis0)
    if on_forcing:
        on_forcing(0, date)
    model_step = 1
    for _ in range(nsteps):
        if (model_step - 1) % NSTEPS == 0:
            model.forcing(phis0)
            if on_forcing:
                on_forcing(model_step, date)
        flux = flux_of(model_step)
        model_step += 1
        date.newdate()
        day = 1 + model_step // NSTEPS
        shifted = model.couple(day, date, flux)
        if on_step:
            on_step(model_step - 1, day, date, flux, shifted)
    return date
