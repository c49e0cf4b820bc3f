"""Decisions of the column physics ON their thresholds, and the regimes outside the ordinary draw.

INVENTORY lists every comparison, compared clamp, nint and integer decision of the five blocks of get_physical_tendencies
(physics.f90:110-205) with the reference's file:line, its operator and its class:
  "i"    exactly reachable: both sides are inputs, literals or results of clamps, bit-identical on the device and in the reference
         whatever the rounding of the arithmetic before them.  At an exact tie the answer is fixed by the reference's operator
         (> or >=, nint's half away from zero), so a column can be built ON the threshold and next to it (np.nextafter);
  "ii"   not exactly reachable: one side comes out of exp, log, sqrt, ** or a rounding sum.  The margin rule of moist.columns /
         radiation.columns / surface.columns stays (no column within MIN_MARGIN of the threshold);
  "host" decided once per plan or per date on the host (level tables, the zonal forcing), pinned bit for bit by table tests.
Class-(i) rows name the sides that can be built: 0 the tie, -1 / +1 its one-ulp neighbours; a side that no input reaches (the
result of a max(., 0) cannot be below 0) is left out and the row's `how` says why.

build() lays the constructions (jobs) over an ordinary drawn state, a few columns each, removes NEAR ties (0 < margin <
MIN_MARGIN, moist.exact_ties) by drawing the column underneath again, and never the constructed exact ones.  hits() finds, from
the inputs and the restatement's outputs alone, which columns sit on which side of which row.  tests/golden/ref_thresholds.npz
(tests/golden/make_golden_thresholds.py) holds the flang-built reference's results on these columns.

regime() draws whole states outside the ordinary distribution (cold, hot and saturated, dry, high orography, calm, all sea, all
land); REGIME_SEEDS are those for which the restatement alone leaves at most 1 % of the columns near a tie
(tests/test_thresholds_cpu.py checks it)."""
import numpy as np

import guards
import moist
import physstep
import radiation
import support
import surface
import synth
from conftest import TOL
from moist import T0
from radiation import QACL

MIN_MARGIN = surface.MIN_MARGIN
TAGS = ("t30", "t30k5")                       # T30 L8 and one other level count
SEED = {"t30": 8301, "t30k5": 8302}
REPS, NUNIFORM = 1, 16                        # columns per (row, instance, side); evenly spread plain columns kept with them


# Class-(i) rows whose tie changes an output if the operator is the other one (>= for >, rint for nint): the constructed columns
# PIN the operator there.  Established by making that change in the NumPy restatement and running it against the flang-built
# fixture (tests/test_thresholds_cpu.py::test_restatement_matches_reference_on_thresholds fails for these four and for no other
# row); the device is held to the same fixture.  sfc.evap0 was already pinned by the drawn columns of tests/surface.py, where
# evap == 0 over a moist soil is common; the three radiation rows were pinned by nothing before.  On every other class-(i) row
# both operators give the same result at the tie: the two branches meet there (qsat at t0; the lapse branch at ta == tb, where
# dt1 = 0 and ftemp0 = 1 leave t1 = ta either way), a zero is a zero, the table is flat.  Those columns are robustness cases --
# signed zeros, denormals, ends of tables and ranges, exact 0 and 1 after clamps -- that a kernel must get through unharmed, and
# say nothing about its operator.
OBSERVABLE = ("sw.qacl", "lw.nint_tg", "lw.nint_ts", "sfc.evap0")


def row(id, block, ref, op, cls, how="", sides=()):
    return {"id": id, "block": block, "ref": ref, "op": op, "cls": cls, "how": how, "sides": tuple(sides),
            "observable": id in OBSERVABLE}


ALL = (-1, 0, 1)
INVENTORY = [
    # ---- thermodynamic fields and humidity
    row("moist.qclamp", "moist", "physics.f90:113", "max(qg, 0.0)", "i", "qg = +0.0 at levels kx, kx-1, 2; neighbours the denormals next to 0", ALL),
    row("moist.qclamp_negzero", "moist", "physics.f90:113", "max(qg, 0.0)", "i", "qg = -0.0 (a zero has no other neighbours)", (0,)),
    row("moist.t0", "moist", "humidity.f90:65", "ta >= t0", "i", "tg = t0 at level kx and at a middle level", ALL),
    row("moist.psmin", "moist", "convection.f90:199", "psa > psmin", "ii", "psa = exp(pslg)"),
    # ---- convection
    row("cnv.mse1", "moist", "convection.f90:203", "min(mse0, mse1)", "ii"),
    row("cnv.mss0", "moist", "convection.f90:206", "max(mse0, mss(kx))", "ii"),
    row("cnv.ktop1", "moist", "convection.f90:216", "mss0 > mss2", "ii"),
    row("cnv.ktop2", "moist", "convection.f90:222", "mse1 > mss2", "ii"),
    row("cnv.ktop1_kx", "moist", "convection.f90:228", "ktop1 < kx", "i", "integer; ktop1 is kx or at most kx-3: every column is off the tie by 3 levels"),
    row("cnv.lqthr", "moist", "convection.f90:232", "qa(kx) > qthr0 .and. qa(nl1) > qthr1", "ii", "qthr = rhbl*qsat"),
    row("cnv.ktop2_kx", "moist", "convection.f90:234", "ktop2 < kx", "i", "integer, as ktop1 < kx"),
    row("cnv.qdif", "moist", "convection.f90:236", "max(qa(kx) - qthr0, (mse0 - msthr)*rlhc)", "ii"),
    row("cnv.itop_nlp", "moist", "convection.f90:78", "itop == nlp", "i", "integer; columns without convection (dried, below psmin)", (0,)),
    row("cnv.qmax", "moist", "convection.f90:85", "max(1.01*qa, qsat)", "ii"),
    row("cnv.qb", "moist", "convection.f90:90", "min(qb, qa)", "ii"),
    row("cnv.fpsa", "moist", "convection.f90:94", "min(1.0, (psa - psmin)*rdps)", "ii"),
    row("cnv.fqmax", "moist", "convection.f90:95", "min(fqmax, qdif/(qmax - qb))", "ii"),
    row("cnv.delq", "moist", "convection.f90:138", "delq > 0.0", "ii", "delq = rhil*qsat - qa"),
    row("cnv.precnv", "moist", "convection.f90:151", "max(fuq - fmass*qsatb, 0.0)", "ii"),
    # ---- large-scale condensation
    row("lsc.rhref", "moist", "large_scale_condensation.f90:70", "max(rhref, rhblsc)", "host"),
    row("lsc.dqa", "moist", "large_scale_condensation.f90:76", "dqa < 0.0", "ii", "dqa = rhref*qsat - qa"),
    row("lsc.itop_2", "moist", "large_scale_condensation.f90:77", "min(k, itop)", "i", "integer; level 2 saturated: iptop = 2", (0,)),
    row("lsc.itop_nl1", "moist", "large_scale_condensation.f90:77", "min(k, itop)", "i",
        "integer; a dried column with only level kx-1 saturated: iptop = kx-1", (0,)),
    row("lsc.itop_nlp", "moist", "large_scale_condensation.f90:77", "min(k, itop)", "i",
        "integer; dried columns: no level condenses or convects, iptop = kx+1", (0,)),
    row("lsc.dtlsc", "moist", "large_scale_condensation.f90:79", "min(-dqlsc, dqmax*psa2)", "ii"),
    # ---- clouds and shortwave
    row("sw.rhcl1", "radiation", "shortwave_radiation.f90:362", "rh(nl1) > rhcl1", "ii", "rh = qa/qsat"),
    row("sw.drh", "radiation", "shortwave_radiation.f90:376", "drh > cloudc", "ii"),
    row("sw.qacl", "radiation", "shortwave_radiation.f90:376", "qa > qacl", "i",
        "qg = qacl at levels 3 .. kx-2, cold and under no lower cloud (counted where drh > cloudc holds, so that the test decides)", ALL),
    row("sw.pmaxcl", "radiation", "shortwave_radiation.f90:386", "min(pmaxcl, 86.4*(precnv + precls))", "ii"),
    row("sw.pr0", "radiation", "shortwave_radiation.f90:386-387", "sqrt(pr1) at precnv == 0 and precls == 0", "i",
        "dried columns: both are exactly 0 after the reference's max / where (nothing below 0 exists)", (0,)),
    row("sw.cloudc1", "radiation", "shortwave_radiation.f90:387", "min(1.0, ...) twice, then max(clsmax - clfact*cloudc, 0.0) :403", "i",
        "level kx-1 super-saturated: cloudc clamped to exactly 1 (nothing above 1 exists; below 1 is the ordinary draw)", (0,)),
    row("sw.icltop_min", "radiation", "shortwave_radiation.f90:388", "min(iptop, icltop)", "i", "integer; iptop == icltop at kx-1", (0,)),
    row("sw.fstab", "radiation", "shortwave_radiation.f90:402", "max(0.0, min(1.0, rgse*(gse - gse_s0)))", "ii"),
    row("sw.clstr", "radiation", "shortwave_radiation.f90:403", "max(clsmax - clfact*cloudc, 0.0)", "ii", "but see sw.cloudc1"),
    row("sw.clstrl", "radiation", "shortwave_radiation.f90:406", "max(clstr, clsminl)", "ii"),
    row("sw.icltop_le", "radiation", "shortwave_radiation.f90:106", "icltop <= kx", "i", "integer; icltop = kx+1 in dried columns (sw.pr0), kx-1 in sw.icltop_min", (0,)),
    row("sw.acloud", "radiation", "shortwave_radiation.f90:117", "min(abscl1*qcloud, abscl2)", "ii"),
    row("sw.k_icltop", "radiation", "shortwave_radiation.f90:125,216", "k >= icltop, k < icltop", "i",
        "integer; k runs through icltop in every cloudy column"),
    row("sw.ablwv", "radiation", "shortwave_radiation.f90:224-225", "max(ablwv*qa, acloud)", "ii"),
    row("sw.coz1", "radiation", "shortwave_radiation.f90:251", "max(0.0, cos(alpha - dalpha))", "host"),
    row("sw.fsol0", "radiation", "shortwave_radiation.f90:282,323", "max(fs0 - fsol, 0.0); ch0 = min(1.0, max(-1.0, .))", "host",
        "polar night: fsol == 0 exactly in the date table; the columns of those latitudes must give exactly 0 shortwave", (0,)),
    # ---- longwave
    row("lw.st4a0", "radiation", "longwave_radiation.f90:50,53", "max(st4a(k,1) - st4a(k-1,1), 0.0)", "i",
        "the lowest three levels at one temperature: the difference is exactly 0 (its neighbours pass through a rounding sum)", (0,)),
    row("lw.nint_tg", "radiation", "longwave_radiation.f90:83,98,160,175", "nint(ta)", "i",
        "tg = n + 0.5 for n = 206, 247, 282, 300, 318 at the level nearest to it (even n: where rint differs); 199.5, 200.5, 320.5 "
        "at level 1 (the table is flat below 200 and above 320: only 200.5 decides there)", ALL),
    row("lw.fband_range", "radiation", "longwave_radiation.f90:83 (mod_radcon fband(100:400,4))", "index within the table", "i",
        "tg = 99.5, 100, 400 and the double below 400.5 at level 1: the ends of the range the reference can index", ALL),
    row("lw.nint_ts", "radiation", "longwave_radiation.f90:145", "nint(ts)", "i",
        "sst = n + 0.5 (n = 271, 288, 300) with fmask = 0, where ts = sst exactly", ALL),
    # ---- surface fluxes
    row("sfc.lapse", "surface", "surface_fluxes.f90:126", "ta(kx) > ta(nl1)", "i", "equal temperatures in the lowest two levels (dt1 = 0 and ftemp0 = 1: both branches give t1 = ta, a robustness case)", ALL),
    row("sfc.land_stab", "surface", "surface_fluxes.f90:158-161", "tskin > t2(1); min(dtheta, .); max(-dtheta, .)", "ii"),
    row("sfc.qsat_tskin", "surface", "humidity.f90:65", "tskin >= t0, tskin + 1 >= t0", "ii", "tskin is a rounding sum"),
    row("sfc.evap_clamp", "surface", "surface_fluxes.f90:190", "max(0.0, soilw*qsat0 - q1)", "i",
        "soilw = 0 and q(kx) = 0: the difference is exactly 0 (0*x - 0)", (0,)),
    row("sfc.evap0", "surface", "surface_fluxes.f90:214", "evap(1) > 0.0", "i",
        "evap is exactly 0 after the clamp of :190 where the air is moister than the wet soil (soilw > 0, so that the branch "
        "taken changes qsat0(2)); nothing below 0 exists, above 0 is the ordinary draw", (0,)),
    row("sfc.sea_stab", "surface", "surface_fluxes.f90:239-242", "tsea > t2(2); min(dtheta, .); max(-dtheta, .)", "ii"),
    row("sfc.tsea_t0", "surface", "humidity.f90:65", "tsea >= t0", "i", "sst = t0", ALL),
    row("sfc.forog", "surface", "surface_fluxes.f90:308", "max(phi0, 0.0)", "i", "phis0 = 0 on land; neighbours the denormals", ALL),
    row("sfc.wind0", "surface", "surface_fluxes.f90:139-140", "sqrt(u0**2 + v0**2 + vgust**2), no comparison", "i",
        "wind exactly 0 at every level, and the denormal above it", (0, 1)),
    # ---- boundary fields at the ends of their range (no comparison in the reference; a shortcut in a kernel would be one)
    row("bnd.fmask", "surface", "surface_fluxes.f90:285-293; shortwave_radiation.f90:407", "weighting by fmask", "i", "0 and 1 and the doubles inside", ALL),
    row("bnd.snowc", "surface", "surface_fluxes.f90:205", "clamb = clambda + snowc*(clambsn - clambda)", "i", "0 and 1 and the doubles inside", ALL),
    row("bnd.soilw", "surface", "surface_fluxes.f90:190", "soilw*qsat0", "i", "0 and 1 and the doubles inside", ALL),
    row("bnd.albsfc", "radiation", "shortwave_radiation.f90:170", "flux*albsfc", "i", "0 and 1 and the doubles inside", ALL),
    row("bnd.alb_l", "surface", "surface_fluxes.f90:149", "ssrd*(1.0 - alb_l)", "i", "0 and 1 and the doubles inside", ALL),
    row("bnd.alb_s", "surface", "surface_fluxes.f90:268", "ssrd*(1.0 - alb_s)", "i", "0 and 1 and the doubles inside", ALL),
    # ---- vertical diffusion
    row("pbl.dmse", "pbl", "vertical_diffusion.f90:88", "dmse >= 0.0", "ii"),
    row("pbl.icnv", "pbl", "vertical_diffusion.f90:89", "icnv > 0", "i", "integer; icnv is -1 or at least 3: no column on the tie"),
    row("pbl.drh_shc", "pbl", "vertical_diffusion.f90:95", "drh >= 0.0", "ii", "rh = qa/qsat; exactly 0 - 0 in dry columns (regime `dry`)"),
    row("pbl.drh0", "pbl", "vertical_diffusion.f90:100", "drh > drh0", "ii"),
    row("pbl.sigh", "pbl", "vertical_diffusion.f90:110", "sigh(k) > 0.5", "host"),
    row("pbl.drh_diff", "pbl", "vertical_diffusion.f90:117", "drh >= drh0", "ii"),
    row("pbl.se0", "pbl", "vertical_diffusion.f90:133", "se(k) < se0", "ii"),
]
CLASS_I = [r for r in INVENTORY if r["sides"]]


def nx(x, side):
    return x if side == 0 else np.nextafter(x, side * np.inf)


def _qsat(tab, c, j, lev):
    return moist.get_qsat(c["tg"][lev - 1, j], np.exp(c["pslg"][j]), tab["fsg"][lev - 1])


def jobs(tab):
    """[(row id, side, reps, fn(c, j))]: fn puts the columns j of the dict c on that side of that row's threshold"""
    kx = tab["kx"]
    J = []

    def add(id, side, fn, reps=REPS):
        J.append((id, side, reps, fn))

    def put(name, lev, value):
        def fn(c, j, side=None):
            c[name][lev - 1, j] = value
        return fn

    for side in ALL:
        for lev in (kx, kx - 1, 2):
            add("moist.qclamp", side, put("qg", lev, nx(0.0, side)))
        for lev in (kx, max(3, kx // 2)):
            add("moist.t0", side, put("tg", lev, nx(T0, side)))
        for n in (206, 247, 282, 300, 318):
            def fn(c, j, v=nx(n + 0.5, side)):
                k = np.argmin(np.abs(c["tg"][2:, j] - v), axis=0) + 2
                c["tg"][k, j] = v
            add("lw.nint_tg", side, fn)
        for v in (199.5, 200.5, 320.5):
            add("lw.nint_tg", side, put("tg", 1, nx(v, side)))
        for n in (271, 288, 300):
            def fn(c, j, v=nx(n + 0.5, side)):
                c["fmask"][j] = 0.0
                c["sst"][j] = v
            add("lw.nint_ts", side, fn)

        def fn(c, j, v=nx(QACL, side)):      # cold enough aloft for rh > rhcl1 at qacl, and no cloud from level kx-1: drh > cloudc
            c["tg"][2:kx - 2, j] = 235.25
            c["qg"][kx - 2, j] = 0.0
            c["qg"][2:kx - 2, j] = v
        add("sw.qacl", side, fn, 4)

        def fn(c, j, side=side):
            c["tg"][kx - 1, j] = nx(c["tg"][kx - 2, j], side)
        add("sfc.lapse", side, fn)

        def fn(c, j, v=nx(T0, side)):
            c["sst"][j] = v
        add("sfc.tsea_t0", side, fn)

        def fn(c, j, v=nx(0.0, side)):
            c["fmask"][j] = 1.0
            c["phis0"][j] = v
        add("sfc.forog", side, fn)
        for name in ("fmask", "snowc", "soilw", "albsfc", "alb_l", "alb_s"):
            for end in ((0.0,) if side == 1 else (1.0,) if side == -1 else (0.0, 1.0)):
                def fn(c, j, name=name, v=nx(end, side)):
                    c[name][j] = v
                add("bnd." + name, side, fn)
    # the ends of the range of fband(100:400,4) that the reference can index (nint(99.5) = 100, nint(400.5-) = 400)
    for v, side in ((99.5, 0), (nx(99.5, 1), 1), (100.0, 0), (nx(100.0, 1), 1), (nx(400.0, -1), -1), (400.0, 0), (nx(400.5, -1), -1)):
        add("lw.fband_range", side, put("tg", 1, v))
    add("moist.qclamp_negzero", 0, put("qg", kx, -0.0))
    add("moist.qclamp_negzero", 0, put("qg", 2, -0.0))

    def dried(c, j):
        c["qg"][:, j] = 0.01 * np.maximum(c["qg"][:, j], 0.0)
    add("sw.pr0", 0, dried, 2)

    def fn(c, j):
        c["qg"][kx - 2, j] = 1.3 * _qsat(tab, c, j, kx - 1)
    add("sw.cloudc1", 0, fn, 3)

    def fn(c, j):
        c["qg"][1, j] = 1.3 * _qsat(tab, c, j, 2)
    add("lsc.itop_2", 0, fn, 3)

    def fn(c, j):
        dried(c, j)
        c["qg"][kx - 2, j] = 1.05 * _qsat(tab, c, j, kx - 1)
    add("sw.icltop_min", 0, fn, 4)

    def fn(c, j):
        c["tg"][kx - 3:, j] = c["tg"][kx - 2, j]
    add("lw.st4a0", 0, fn)

    def fn(c, j):
        c["soilw"][j] = 0.0
        c["qg"][kx - 1, j] = 0.0
    add("sfc.evap_clamp", 0, fn)
    for side in (0, 1):
        def fn(c, j, v=nx(0.0, side)):
            c["ug"][:, j] = v
            c["vg"][:, j] = v
        add("sfc.wind0", side, fn)
    return J


def assignment(tab, ncol, seed):
    """[(row id, side, columns)] of jobs(tab), and the sorted set of all their columns plus NUNIFORM evenly spread ones"""
    perm = np.argsort(synth.splitmix64(seed + 0x71E5, ncol), kind="stable")
    out, at = [], 0
    for id, side, reps, fn in jobs(tab):
        out.append((id, side, perm[at:at + reps], fn))
        at += reps
    assert at <= ncol // 4
    sub = np.unique(np.concatenate([a[2] for a in out] + [np.linspace(0, ncol - 1, NUNIFORM).astype(np.int64)]))
    return out, sub


def second(c):
    """the inputs of the call without shortwave: the same temperatures (so that the nint ties hold again on the held state),
    winds and their tendencies swapped, a colder soil and radiation.py's second ttend"""
    return dict(c, ug=c["vg"], vg=c["ug"], utend=c["vtend"], vtend=c["utend"], stl=c["stl"] - 0.5, ttend=c["ttend2"])


def two_calls(tab, c, zon, sqcoa):
    """surface.chain on a shortwave call and a call without shortwave on the held state, exact ties counted as clear"""
    with moist.exact_ties():
        r1, st = surface.chain(tab, c, zon, sqcoa, True)
        r2, _ = surface.chain(tab, second(c), zon, sqcoa, False, st)
    return r1, r2


def build(tab, ncol, seed, zon, sqcoa):
    """The threshold state: (columns dict, stored column set, r1, r2).  Every job is applied to its columns of an ordinary draw;
    a column with a NEAR tie in either call gets the next stream's draw underneath and its job again."""
    assign, sub = assignment(tab, ncol, seed)
    base = surface._draw(tab, ncol, seed)
    for attempt in range(1, 50):
        c = {k: v.copy() for k, v in base.items()}
        for _, _, j, fn in assign:
            fn(c, j)
        r1, r2 = two_calls(tab, c, zon, sqcoa)
        bad = np.nonzero(np.minimum(r1["margin"], r2["margin"]) < MIN_MARGIN)[0]
        if bad.size == 0:
            return c, sub, r1, r2
        new = surface._draw(tab, ncol, seed + 7919 * attempt)
        for k in base:
            base[k][..., bad] = new[k][..., bad]
    raise RuntimeError("could not draw columns clear of near ties")


def hits(tab, c, r, zon):
    """{(row id, side): columns [ncol] bool} from the inputs c and the restatement's outputs r of the shortwave call alone"""
    kx = tab["kx"]
    tg, qg = c["tg"], c["qg"]
    H = {}
    any0 = lambda m: np.any(m, axis=0)
    for side in ALL:
        z = nx(0.0, side)
        H["moist.qclamp", side] = any0((qg == z) & (np.signbit(qg) == (side < 0)))
        H["moist.t0", side] = any0(tg == nx(T0, side))
        half = tg - np.floor(tg)
        at = {0: half == 0.5, -1: np.nextafter(tg, np.inf) - np.floor(tg) == 0.5, 1: np.nextafter(tg, -np.inf) - np.floor(tg) == 0.5}[side]
        H["lw.nint_tg", side] = any0(at)
        ts = r["sfc"]["ts"]
        at = {0: ts, -1: np.nextafter(ts, np.inf), 1: np.nextafter(ts, -np.inf)}[side]
        H["lw.nint_ts", side] = (at - np.floor(ts) == 0.5) & (c["fmask"] == 0.0)
        H["sw.qacl", side] = r["down"]["ties"]["qacl_open"] & any0(qg[2:kx - 2] == nx(QACL, side))
        H["sfc.lapse", side] = tg[kx - 1] == nx(tg[kx - 2], side)
        H["sfc.tsea_t0", side] = c["sst"] == nx(T0, side)
        H["sfc.forog", side] = (c["phis0"] == z) & (np.signbit(c["phis0"]) == (side < 0)) & (c["fmask"] > 0.0)
        for name in ("fmask", "snowc", "soilw", "albsfc", "alb_l", "alb_s"):
            ends = [nx(e, side) for e in ((0.0,) if side == 1 else (1.0,) if side == -1 else (0.0, 1.0))]
            H["bnd." + name, side] = np.isin(c[name], ends)
    H["lw.fband_range", 0] = np.isin(tg[0], (99.5, 100.0, 400.0))
    H["lw.fband_range", 1] = np.isin(tg[0], (nx(99.5, 1), nx(100.0, 1)))
    H["lw.fband_range", -1] = np.isin(tg[0], (nx(400.0, -1), nx(400.5, -1)))
    H["moist.qclamp_negzero", 0] = any0((qg == 0.0) & np.signbit(qg))
    m, d, s = r["moist"], r["down"], r["sfc"]
    H["cnv.itop_nlp", 0] = m["icnv"] == -1
    H["lsc.itop_2", 0] = m["iptop"] == 2
    H["lsc.itop_nl1", 0] = m["iptop"] == kx - 1
    H["lsc.itop_nlp", 0] = m["iptop"] == kx + 1
    H["sw.pr0", 0] = (m["precnv"] == 0.0) & (m["precls"] == 0.0) & (d["ties"]["pr1"] == 0.0)
    H["sw.cloudc1", 0] = (d["cloudc"] == 1.0) & (d["ties"]["cloudc_rh"] == 1.0)
    H["sw.icltop_min", 0] = (m["iptop"] == kx - 1) & (d["ties"]["icl_rh"] == kx - 1)
    H["sw.icltop_le", 0] = d["icltop"] == kx + 1
    H["sw.fsol0", 0] = zon["fsol"] == 0.0
    H["lw.st4a0", 0] = (tg[kx - 1] == tg[kx - 2]) & (tg[kx - 2] == tg[kx - 3])
    H["sfc.evap_clamp", 0] = (s["dq"] == 0.0) & (c["soilw"] == 0.0)
    H["sfc.evap0", 0] = (s["evap"][0] == 0.0) & (c["soilw"] > 0.0) & (s["dq"] < 0.0)
    for side in (0, 1):
        v = nx(0.0, side)
        H["sfc.wind0", side] = np.all((c["ug"] == v) & (c["vg"] == v), axis=0)
    return H


# ------------------------------------------------------------------------------------------------------------- outputs
TEND = ("utend", "vtend", "ttend", "qtend")
SW_ONLY = ("rad.cloudc", "rad.clstr", "rad.icltop", "rad.ssrd", "rad.ssr", "rad.tsr", "rad.tt_rsw")


def flat(r, kx):
    """surface.chain's outputs under the names of the device's optional outputs (physstep.expected) as columns [.., ncol], plus
    the four tendencies"""
    m, d, s, up, p = r["moist"], r["down"], r["sfc"], r["up"], r["pbl"]
    out = {"moist." + n: m[n] for n in ("precnv", "precls", "cbmf", "iptop", "icnv", "qsat", "rh", "se")}
    out.update({"rad." + n: d[n] for n in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "slrd", "tt_rsw") if n in d})
    out.update({"rad.slr": up["slr"], "rad.olr": up["olr"], "rad.tt_rlw": up["tt_rlw"]})
    out.update({"sfc." + n: s[n] for n in surface.SFC_3 + ("hfluxn", "tskin", "u0", "v0", "t0")})
    out.update({"pbl." + n: p[n] for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")})
    out.update(ts=s["ts"], fsfcu=s["slru"][2])
    out.update({n: p[n] for n in TEND})
    return out


def scales(tab, c, r):
    """Scales of the outputs that are differences of large terms, from their OPERANDS: [ncol], or [kx, ncol] where the operand
    differs from level to level (everything else is scaled by its own size in the column, guards.column_err).
      shf, evap       the bulk coefficient times the larger of the two temperatures / humidities that are subtracted;
      hfluxn, slr     the radiative and turbulent fluxes that are summed;
      ssr, tt_rsw     the downward shortwave flux at the surface, at each level times that level's rps*grdscp;
      tt_rlw          sigma*T**4 of the column's warmest level, at each level times that level's rps*grdscp;
      tt_pbl, ttend   per level the largest term added: the incoming tendency, the moist block's, the two heating rates, the
                      sensible heat flux at level kx, and -- only in columns where shallow convection or the damping of a
                      super-adiabatic lapse rate fires -- the dry static energies whose difference drives them;
      qt_pbl, qtend   likewise with the evaporation at level kx and the saturation humidities that the moisture diffusion mixes.
    For shf, hfluxn, tt_rlw, tt_pbl and ttend these operand scales are, in most columns, larger than the array's own max|ref|: for
    them the per-column norm adds only the exact zeros and the array norm beside it is the binding one."""
    kx = tab["kx"]
    s, m, br = r["sfc"], r["moist"], r["pbl"]["branch_cols"]
    psa = np.exp(c["pslg"])
    tmax = np.maximum(np.maximum(np.abs(s["tskin"]), np.abs(c["sst"])), np.abs(c["tg"][kx - 1]))
    shf = surface.CHS * moist.CP * s["den0"] * tmax
    qmax = np.maximum(moist.get_qsat(tmax, psa, 1.0), np.maximum(c["qg"][kx - 1], 0.0))
    evap = surface.CHS * s["den0"] * qmax
    lw = radiation.EMISFC * radiation.SBC * np.max(np.abs(c["tg"]), axis=0) ** 4
    sw = np.abs(r["ssrd"])
    gc, gs = tab["grdscp"][:, None] / psa, tab["grdsig"][:, None] / psa                 # [kx, ncol]
    out = {"sfc.shf": shf, "sfc.evap": evap, "sfc.hfluxn": np.maximum(lw, sw) + shf + moist.ALHC * evap, "rad.slr": lw,
           "rad.ssr": sw, "rad.tt_rlw": lw * gc, "rad.tt_rsw": sw * gc}
    vd = surface.vdiff_tables(tab)
    fires = br["damp_some"] | br["shc_cnv_drh"] | br["shc_cnv_nodrh"] | br["shc_nocnv_drh"] | br["shc_nocnv_nodrh"]
    mixes = fires | br["stable_diff"] | br["qdiff_some"]
    tt = np.maximum(np.maximum(np.abs(c["ttend"]), np.abs(m["ttend"])), np.maximum(lw, sw) * gc)
    tt[kx - 1] = np.maximum(tt[kx - 1], shf * gc[kx - 1])
    tt = np.maximum(tt, np.where(fires, np.max(np.abs(m["se"]), axis=0) * vd["vd_scalars"][5], 0.0) * vd["vd_rsig"][:, None])
    qq = np.maximum(np.abs(c["qtend"]), np.abs(m["qtend"]))
    qq[kx - 1] = np.maximum(qq[kx - 1], evap * gs[kx - 1])
    qq = np.maximum(qq, np.where(mixes, np.max(np.abs(m["qsat"][1:]), axis=0) * vd["vd_scalars"][2], 0.0) * vd["vd_rsig"][:, None])
    out.update({"pbl.tt_pbl": tt, "ttend": tt, "pbl.qt_pbl": qq, "qtend": qq})
    return out


# ------------------------------------------------------------------------------------------------------------- regimes
SOLSTICE_JUN, SOLSTICE_DEC, EQUINOX_MAR = 171.5 / 365.0, 355.5 / 365.0, 79.5 / 365.0
# name -> (seed, tyear); the seeds are those checked on the CPU against the 1 % cap (tests/test_thresholds_cpu.py)
REGIMES = {"cold": (8401, radiation.DATES[0]), "hot_saturated": (8402, radiation.DATES[1]), "dry": (8403, radiation.DATES[0]),
           "high_orography": (8404, radiation.DATES[1]), "calm": (8405, radiation.DATES[0]), "all_sea": (8406, radiation.DATES[1]),
           "all_land": (8407, radiation.DATES[0]), "solstice_jun": (8408, SOLSTICE_JUN), "solstice_dec": (8409, SOLSTICE_DEC),
           "equinox_mar": (8410, EQUINOX_MAR)}
REGIME_CAP = 0.01


def regime(name, tab, ncol):
    """One whole state (ncol columns) of the regime `name`: surface._draw reshaped.  Nothing is drawn again."""
    kx, fsg = tab["kx"], tab["fsg"]
    seed = REGIMES[name][0]
    c = surface._draw(tab, ncol, seed)
    u = synth.splitmix64(seed + 0x4E6, ncol * (2 * kx + 4)).reshape(2 * kx + 4, ncol)
    psa = np.exp(c["pslg"])
    rh = np.maximum(c["qg"], 0.0) / moist.get_qsat(c["tg"], psa, fsg[:, None])

    def rehumidify(rh):
        c["qg"] = rh * moist.get_qsat(c["tg"], np.exp(c["pslg"]), fsg[:, None])
    if name == "cold":                                   # 180 .. 230 K at every level, the surface with it
        c["tg"] = 180.0 + 50.0 * u[:kx]
        rehumidify(rh)
        c["sst"] = c["tg"][-1] + 24.0 * u[kx] - 8.0
        c["stl"] = c["tg"][-1] + 16.0 * u[kx + 1] - 8.0
    elif name == "hot_saturated":                        # 15 K warmer, rh 1.0 .. 1.1 at every level
        c["tg"] = c["tg"] + 15.0
        rehumidify(1.0 + 0.1 * u[:kx])
        c["sst"], c["stl"] = c["sst"] + 15.0, c["stl"] + 15.0
    elif name == "dry":                                  # q = 0 exactly, everywhere
        c["qg"] = np.zeros_like(c["qg"])
    elif name == "high_orography":                       # ps/p0 0.45 .. 0.8: every column below psmin
        c["pslg"] = np.log(0.45 + 0.35 * u[0])
        rehumidify(rh)
        c["phis0"] = np.where(c["fmask"] > 0.0, moist.GRAV * (2000.0 + 3500.0 * u[1]), 0.0)
    elif name == "calm":                                 # |u|, |v| < 0.1 m/s, a quarter of the values exactly 0
        c["ug"] = np.where(u[:kx] < 0.25, 0.0, 0.2 * u[:kx] - 0.1)
        c["vg"] = np.where(u[kx:2 * kx] < 0.25, 0.0, 0.2 * u[kx:2 * kx] - 0.1)
    elif name == "all_sea":                              # ice-free sea everywhere
        c["fmask"] = np.zeros(ncol)
        c["phis0"] = np.zeros(ncol)
        c["sst"] = np.maximum(c["sst"], 271.4 + u[0])
    elif name == "all_land":                             # snow-covered land everywhere, the soil dry or saturated
        c["fmask"] = np.ones(ncol)
        c["snowc"] = np.ones(ncol)
        c["soilw"] = np.where(u[0] < 0.5, 0.0, 1.0)
        c["phis0"] = moist.GRAV * 3000.0 * u[1] ** 2
    return c


def regime_run(tab, c, zon, sqcoa):
    """the restated chain on a regime's columns and the columns kept: those with no NEAR tie (exact ties stay)"""
    with moist.exact_ties():
        r, _ = surface.chain(tab, c, zon, sqcoa)
    return r, r["margin"] >= MIN_MARGIN


def check_regime(name, r, keep):
    """the cap on the exclusion, and that no branch any column takes loses all its columns to it; returns the excluded share"""
    share = 1.0 - float(np.mean(keep))
    assert share <= REGIME_CAP, (name, share)
    br = dict(r["moist"]["branch_cols"])
    br.update(surface.branch_cols(r))
    br.update(r["down"]["branch_cols"])
    for k, mask in br.items():
        assert not mask.any() or (mask & keep).any(), (name, k)
    return share


# ------------------------------------------------------------------------------------------------ device side (torch)
ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")
INT_OUT = ("moist.iptop", "moist.icnv", "rad.icltop")
NAMES = ("ug", "vg", "tg", "qg", "phig", "pslg", "albsfc") + TEND + surface.BOUNDARY


def dev(c, il, ix):
    return {n: support.dev(radiation.grids(c[n], 1, il, ix)) for n in NAMES}


def device_columns(t, kx):
    """a device output of one state as columns [.., ncol]"""
    a = t.cpu().numpy()[0]
    return a.reshape(-1, a.shape[-2] * a.shape[-1]).squeeze() if a.ndim == 3 else a.reshape(-1)


def chain(sp, kx, il, ix, calls, fused):
    """column_physics_dev on the calls [(inputs, compute_sw)] with one radiation state; {"<call>.<name>": tensor}"""
    import torch
    sp.set_option("physics_fused", fused)
    S = torch.full((sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    res, ssrd = {}, None
    for i, (d, sw) in enumerate(calls, 1):
        T = [d[n].clone() for n in TEND]
        out = sp.column_outputs(1)
        if sw:
            ssrd = out["rad"]["ssrd"]
        else:                              # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = ssrd
        sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], S, *T, out)
        torch.cuda.synchronize()
        res.update({"%d.%s" % (i, n): t for n, t in zip(TEND, T)})
        res.update({"%d.%s" % (i, n): (t.clone() if n in SW_ONLY else t) for n, t in physstep.flat_outs(out).items()
                    if sw or n not in SW_ONLY})
        res["%d.state" % i] = S.clone()
    return res


def single_calls(sp, kx, il, ix, calls):
    """the same through the five single entry points"""
    import torch
    S = torch.full((sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    res, ssrd = {}, None
    for i, (d, sw) in enumerate(calls, 1):
        U, V, T, Q = [d[n].clone() for n in TEND]
        o = sp.column_outputs(1)
        if sw:
            ssrd = o["rad"]["ssrd"]
        else:
            o["rad"]["ssrd"] = ssrd
        mo, ro = o["moist"], o["rad"]
        flux3 = torch.zeros((1, 4, il, ix), dtype=torch.float64, device="cuda")
        sp.moist_columns_dev(d["tg"], d["qg"], d["phig"], d["pslg"], T, Q, mo)
        sp.radiation_down_dev(sw, d["tg"], d["qg"], d["phig"], d["pslg"], mo["rh"], mo["precnv"], mo["precls"], mo["iptop"],
                              d["fmask"], d["albsfc"], S, ro)
        sp.surface_fluxes_dev(d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], ssrd, ro["slrd"], d, o["ts"], o["fsfcu"],
                              flux3, o["sfc"])
        sp.radiation_up_dev(d["tg"], d["pslg"], o["ts"], o["fsfcu"], S, T, ro)
        sp.pbl_dev(d["qg"], d["phig"], d["pslg"], mo["se"], mo["rh"], mo["qsat"], mo["icnv"], flux3, U, V, T, Q, o["pbl"])
        torch.cuda.synchronize()
        res.update({"%d.%s" % (i, n): t for n, t in zip(TEND, (U, V, T, Q))})
        res.update({"%d.%s" % (i, n): (t.clone() if n in SW_ONLY else t) for n, t in physstep.flat_outs(o).items()
                    if sw or n not in SW_ONLY})
        res["%d.state" % i] = S.clone()
    return res


def against(got, want, kx, scales, cols, stored, label, worst):
    """got {name: tensor} of one call on the columns `cols` (an index array or a mask) against want {name: array}: [.., ncol]
    arrays, or with stored=True the fixture's arrays, which hold the columns `cols` only and level kx only of utend and vtend.
    Integers identical, floats within TOL in the array norm and per column; the worst per-column error per block into `worst`."""
    for n, w in want.items():
        g, w = device_columns(got[n], kx), np.asarray(w)
        if n in ("utend", "vtend") and stored:         # the fixture keeps level kx; the restatement has every level
            g = g[kx - 1]
        g = g[..., cols]
        w = w if stored else w[..., cols]
        assert g.shape == w.shape, (label, n, g.shape, w.shape)
        if n in ("utend", "vtend") and not stored:     # untouched above level kx: the restatement keeps the input there
            assert np.array_equal(g[:kx - 1], w[:kx - 1]), (label, n, "above level kx")
        if n in INT_OUT:
            assert np.array_equal(g, w), (label, n, int(np.sum(g != w)))
            continue
        e = synth.relerr(g, w)
        ec = guards.column_err(g, w, scales[n][..., cols] if n in scales else None)
        blk = n.split(".")[0] if "." in n else "tend" if n in TEND else "sfc"
        if float(ec.max()) >= worst.get(blk, (-1.0, ""))[0]:
            worst[blk] = (float(ec.max()), n)
        assert e <= TOL, (label, n, "array norm", e)
        assert float(ec.max()) <= TOL, (label, n, "per column", float(ec.max()), int(np.argmax(ec)))


def check_threshold_columns(tag, sp, tab, seed, ref_sub, stored):
    """the body of test_threshold_columns_on_device on a plan sp with the tables tab of its levels: thresholds.build(seed), whose
    stored columns are ref_sub; stored(step) gives the fixture's outputs of call 1 / 2 by name"""
    import torch
    ix, il, kx = sp.ix, sp.il, sp.kx
    sp.radiation_set_date(radiation.DATES[0])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    c, sub, r1, r2 = build(tab, il * ix, seed, zon, sqcoa)
    assert np.array_equal(sub, ref_sub), "%s: the constructed columns build() chose are not the fixture's stored ones" % tag
    sp.surface_set_orography(c["phis0"].reshape(il, ix))
    c2 = second(c)
    calls = [(dev(c, il, ix), True), (dev(c2, il, ix), False)]
    sp.column_physics_workspace()
    one = chain(sp, kx, il, ix, calls, 1)
    five = chain(sp, kx, il, ix, calls, 0)
    single = single_calls(sp, kx, il, ix, calls)
    assert len(one) > 70 and set(one) == set(five) == set(single), (
        "%s: the three routes wrote different sets of outputs" % tag, len(one), len(five), len(single))
    for n, v in one.items():
        assert torch.equal(v, five[n]), ("one launch against five kernels", n)
        assert torch.equal(v, single[n]), ("one launch against the single entry points", n)
    assert not torch.isnan(one["2.state"]).any(), "%s: NaN left in the radiation state after call 2" % tag
    worst_ref, worst_all = {}, {}
    everything = np.arange(il * ix)
    for step, cc, r in ((1, c, r1), (2, c2, r2)):
        got = {n[2:]: v for n, v in one.items() if n.startswith("%d." % step) and not n.endswith("state")}
        sc = scales(tab, cc, r)
        against(got, stored(step), kx, sc, sub, True, "call %d vs reference" % step, worst_ref)
        mine = flat(r, kx)
        if step == 2:
            mine = {n: v for n, v in mine.items() if n not in SW_ONLY}
        against(got, mine, kx, sc, everything, False, "call %d vs restatement" % step, worst_all)
    sp.close()
    fmt = lambda w: ", ".join("%s %.1e (%s)" % (b, e, n) for b, (e, n) in sorted(w.items()))
    print("\n[threshold columns %s on the device, worst per-column error per block] vs reference: %s; vs restatement, every column: %s"
          % (tag, fmt(worst_ref), fmt(worst_all)))
