"""The whole column physics inside a time step: the reference side of tests/test_gpu_physics_step.py.

get_physical_tendencies (physics.f90:94-205) on the spectra of time level 1: the oracle supplies uvspec + spec_to_grid(., 2) of
(vor, div), spec_to_grid(., 1) of t, q, phi, ps and the geopotential; the blocks are the NumPy restatements (surface.chain, pinned to
the flang-built reference by tests/golden/ref_surface.npz).  The state is moist.state(o, dynstep.state(sp, seed), seed2); the
boundary fields are drawn per column around the lowest-level grid temperature of that state, as surface._draw draws them.

Columns of a transformed state cannot be redrawn one by one, so the committed SEEDS are those for which every decision margin the
chain reports is >= MIN_MARGIN in every column on every step of the tests (found by running this module's reference side on the
CPU: tests/test_physics_step_cpu.py repeats that for the first step).  Boundary values are per-column inputs: a column whose
SURFACE decisions are too close gets new ones from the next stream."""
import numpy as np

import longrun
import moist
import radiation
import support
import surface
import synth
from conftest import TOL, VARIANTS
from dynstep import PROG, ROB, oracle_dynamics_step, wave_relerr
from dynstep import state as dyn_state

MIN_MARGIN = surface.MIN_MARGIN
ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")
# tag -> (dynstep.state seed, moist.state seed, boundary seed)
SEEDS = {"t30": (8000, 5150, 31000), "t63k16": (8000, 5150, 31000)}
# The seeded state is not a balanced atmosphere: with the whole physics in it, three consecutive steps stay finite only with
# a short step (T30 L8: 2400 s and 900 s overflow on the third step, T63 L16: 300 s and 120 s; found on the CPU with this module's
# reference side).  That is a property of the seeded state, not of the physics: from the reference's rest state (longrun.rest_state)
# the step with the whole physics runs the start-up sequence and 72 leapfrog steps at the model's own delt = 2400 s (reference_run
# below, tests/test_physics_run_cpu.py, tests/test_gpu_physics_run.py).
DT = {"t30": 300.0, "t63k16": 50.0}

# ---- the two-day run with the whole physics (T30 L8, longrun.CASES)
RUN_SEED = 778            # boundary noise (longrun.boundary): the smallest margin of the 74 steps is 6.3e-10 ("wind"), 3.3e-10 ("rest")
RUN_MARGIN = 1e-11        # no decision of any column on any step closer to its threshold: > 100 x the device's single-step error level
NSTRAD = 3                # speedy.f90:35
RESYNC = (10, 37, 38, 72)  # leapfrog steps before which the whole state is recorded: two shortwave steps, two without


def shortwave_step(n):
    """compute_shortwave of leapfrog step n (1-based; n <= 0: the two start-up steps): .true. initially
    (shortwave_radiation.f90:67), then mod(model_step, nstrad) == 1 (speedy.f90:21,35)"""
    return n <= 0 or n % NSTRAD == 1


def grids_of(o, st):
    """physics.f90:94-104 with the oracle: ug, vg, tg, qg, phig [kx, il, ix] and pslg [il, ix] of time level 1"""
    kx = o.kx
    phi = o.geopotential(st["t"][0], st["phis"])
    uv = [o.uvspec(st["vor"][0, k], st["div"][0, k]) for k in range(kx)]
    ug = np.stack([o.spec_to_grid(u, 2) for u, _ in uv])
    vg = np.stack([o.spec_to_grid(v, 2) for _, v in uv])
    tg, qg, phig = (np.stack([o.spec_to_grid(a[k], 1) for k in range(kx)]) for a in (st["t"][0], st["tr"][0], phi))
    return {"ug": ug, "vg": vg, "tg": tg, "qg": qg, "phig": phig, "pslg": o.spec_to_grid(st["ps"][0], 1)}


def draw_boundary(tlow, seed):
    """fmask, albsfc (radiation._draw's recipe) and the surface boundary fields (surface._draw's) around tlow [ncol]"""
    n = tlow.size
    u = synth.splitmix64(seed, n * 11).reshape(11, n)
    return {"fmask": np.where(u[0] < 1 / 3, 0.0, np.where(u[0] < 2 / 3, 1.0, u[1])), "albsfc": 0.07 + 0.6 * u[2],
            "sst": tlow + 24.0 * u[3] - 8.0, "stl": tlow + 16.0 * u[4] - 8.0, "soilw": np.where(u[5] < 0.25, 0.0, u[6]),
            "snowc": np.where(u[7] < 0.5, 0.0, u[8]), "alb_l": 0.1 + 0.5 * u[9], "alb_s": 0.07 + 0.5 * u[10]}


def columns_of(g, bnd, phis0, ut, vt, tt, qt):
    """surface.chain's column dict from grids [kx, il, ix] / [il, ix] and per-column boundary fields"""
    kx = g["tg"].shape[0]
    c = {n: np.ascontiguousarray(g[n]).reshape(kx, -1) for n in ("ug", "vg", "tg", "qg", "phig")}
    c["pslg"] = g["pslg"].reshape(-1)
    c.update(utend=ut.reshape(kx, -1), vtend=vt.reshape(kx, -1), ttend=tt.reshape(kx, -1), qtend=qt.reshape(kx, -1))
    c.update(bnd)
    c["phis0"] = phis0.reshape(-1)
    return c


class Case:
    """One resolution's plan-independent reference data: tables, state, orography, zonal forcing, boundary fields."""

    def __init__(self, tag, sp, o, date=0, st=None, bnd=None, hsg=None, seeds=None):
        """st, bnd: a given state (the orography is its phis on the grid) and the boundary fields to use with it as they are;
        without them both are drawn from seeds (default SEEDS[tag]).  hsg: the half levels of sp and o where they are not
        moist.HSG's (a plan of tests/levels.py)"""
        self.tag, self.o = tag, o
        self.kx, self.il, self.ix = o.kx, o.il, o.ix
        self.tab = moist.tables(moist.HSG[self.kx] if hsg is None else hsg)
        seeds = SEEDS[tag] if seeds is None else seeds
        self.st = moist.state(o, dyn_state(sp, seeds[0]), seeds[1]) if st is None else st
        self.phis0 = o.spec_to_grid(self.st["phis"], 1)
        self.sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, self.il, self.ix)
        self.set_date(sp, date)
        if bnd is not None:
            self.bnd = bnd
            return
        sb = seeds[2]
        g = grids_of(o, self.st)
        zero = np.zeros((self.kx, self.il, self.ix))
        self.bnd = draw_boundary(g["tg"][-1].reshape(-1), sb)
        for attempt in range(1, 50):          # boundary values only: the surface scheme's own decisions
            r, _ = surface.chain(self.tab, columns_of(g, self.bnd, self.phis0, zero, zero, zero, zero), self.zon, self.sqcoa)
            bad = np.nonzero(r["sfc"]["margin"] < MIN_MARGIN)[0]
            if bad.size == 0:
                break
            new = draw_boundary(g["tg"][-1].reshape(-1), sb + 7919 * attempt)
            for k in self.bnd:
                self.bnd[k][bad] = new[k][bad]
        else:
            raise RuntimeError("could not draw boundary values clear of ties")

    def set_date(self, sp, date):
        """the zonal forcing of radiation.DATES[date] from the plan's tables (spdy_radiation_set_date on sp)"""
        sp.radiation_set_date(radiation.DATES[date])
        self.zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, self.il, self.ix)

    def physics(self, st, compute_sw, rad_state, ut, vt, tt, qt, bnd=None):
        """get_physical_tendencies on st: ut .. qt [kx, il, ix] updated in place; returns surface.chain's outputs (+ "grids")"""
        g = grids_of(self.o, st)
        c = columns_of(g, bnd or self.bnd, self.phis0, ut, vt, tt, qt)
        r, _ = surface.chain(self.tab, c, self.zon, self.sqcoa, compute_sw, rad_state)
        shp = ut.shape
        for a, n in ((ut, "utend"), (vt, "vtend"), (tt, "ttend"), (qt, "qtend")):
            a[...] = r["pbl"][n].reshape(shp)
        r["grids"] = g
        return r

    def hook(self, compute_sw, rad_state, record, bnd=None):
        """physics= hook of dynstep.oracle_dynamics_step"""
        def hook(o, st, ut, vt, tt, qt):
            record.clear()
            record.update(self.physics(st, compute_sw, rad_state, ut, vt, tt, qt, bnd))
        return hook


def run_case(sp, o, name, seed=RUN_SEED):
    """the Case of the two-day run `name` of longrun.CASES: the reference's rest state over the seeded orography, longrun.boundary's
    fields over that orography"""
    st = longrun.rest_state(o, wind=longrun.CASES[name])
    bnd = longrun.boundary(o.spec_to_grid(st["phis"], 1), longrun.latitudes(sp.table("sia_half")), seed)
    return Case("t30", sp, o, st=st, bnd=bnd)


def reference_run(case, resync=()):
    """The reference side of the run with the whole physics: longrun.run (start-up steps + 72 leapfrog steps at delt = 2400 s)
    with oracle_dynamics_step and case.hook, the reference's shortwave cadence, ONE radiation state, RAW filter off in the
    start-up steps.  Returns
      cps  {n: prognostics after leapfrog step n, + "rad" (rad_state_array) and "ssrd" (the held ssrd)} for n in longrun.CHECKPOINTS,
      log  one entry per step (74): n, sw, margin (the smallest of all columns), convecting columns, branch counts,
      pre  {n: what leapfrog step n starts from and gives} for n in resync: "st" (both time levels), "rs" (the radiation state
           dict, held ssrd included), "new" / "out" (oracle_dynamics_step's results), "rec" (the chain's outputs of that step)."""
    o, kx = case.o, case.kx
    rs, rec, log, pre, extra, count = {}, {}, [], {}, {}, [0]
    copy = lambda d: {k: np.array(v, copy=True) for k, v in d.items()}

    def step(j1, j2, dt, st):
        count[0] += 1
        n = count[0] - 2
        sw = shortwave_step(n)
        if n in resync:
            pre[n] = {"st": copy(st), "rs": copy(rs)}
        new, out = oracle_dynamics_step(o, st, j1, dt, 0.0 if j1 == 1 else ROB, j2=j2, physics=case.hook(sw, rs, rec))
        mb = rec["moist"]["branch"]
        br = {k: int(v.sum()) for k, v in surface.branch_cols(rec).items()}
        log.append({"n": n, "sw": sw, "margin": float(rec["margin"].min()), "convecting": mb["columns"] - mb["no_conv"],
                    "moist": dict(mb), "branches": br})
        if n in resync:
            pre[n].update(new=copy(new), out=out, rec=dict(rec))
        if n in longrun.CHECKPOINTS:
            extra[n] = {"rad": rad_state_array(rs, kx), "ssrd": rs["ssrd_held"].copy()}
        return new
    cps = longrun.run(step, o.tail_init, case.st)
    for n in cps:
        cps[n].update(extra[n])
    return cps, log, pre


# ---- tests/golden/ref_physrun.npz: the restatements on columns of the "wind" run, pinned to the flang-built reference
PHYSRUN_STEPS = (70, 72)          # the grids before leapfrog step 70 (70 mod 3 = 1: shortwave) and 72 (none, on the held state)
PHYSRUN_INPUTS = ("ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend", "qtend", "albsfc", "phis0") + surface.BOUNDARY
RAD_STATE = ("tau2", "stratc", "tt_rsw", "flux", "dfabs", "slrd", "ssrd_held")


def chain_outputs(r, c):
    """what ref_physrun.npz stores of surface.chain's outputs r on columns c ([.., ncol] each): everything ref_surface.npz stores,
    and the moist block's and the longwave scheme's results that feed it"""
    m, s, p = r["moist"], r["sfc"], r["pbl"]
    out = {n: s[n] for n in surface.SFC_3 + ("hfluxn",) + surface.SFC_2D}
    out.update(forog=surface.forog(c["phis0"]), ssrd=r["ssrd"], slrd=r["down"]["slrd"], ut_pbl=p["ut_pbl"], vt_pbl=p["vt_pbl"],
               tt_pbl=p["tt_pbl"], qt_pbl=p["qt_pbl"], utend=p["utend"][-1], vtend=p["vtend"][-1], ttend=p["ttend"], qtend=p["qtend"],
               icnv=m["icnv"], iptop=m["iptop"], precnv=m["precnv"], precls=m["precls"], cbmf=m["cbmf"], slr=r["up"]["slr"],
               olr=r["up"]["olr"])
    return out


def check_coverage(r, label=""):
    """The margins first, then that the state exercises the physics; prints the branch counts."""
    assert float(r["margin"].min()) >= MIN_MARGIN, (label, float(r["margin"].min()), int(np.argmin(r["margin"])))
    mb = r["moist"]["branch"]
    sb = {k: int(v.sum()) for k, v in r["sfc"]["branch_cols"].items()}
    print("[physics branches %s] moist %s; surface %s" % (label, mb, sb))
    assert 0 < mb["no_conv"] < mb["columns"]                                   # some but not all columns convect
    assert mb["lsc_interior"] + mb["lsc_kx"] > 0                               # large-scale condensation occurs
    unstable = sb["land_clamp_hi"] + sb["land_mid_unstable"] + sb["sea_clamp_hi"] + sb["sea_mid_unstable"]
    stable = sb["land_clamp_lo"] + sb["land_mid_stable"] + sb["sea_clamp_lo"] + sb["sea_mid_stable"]
    assert unstable > 0 and stable > 0                                         # both stability branches of the surface scheme


def expected(r, kx, il, ix):
    """the chain's outputs under the names of spdy_column_physics_out, shaped as the device writes one state"""
    g3, g2 = (kx, il, ix), (il, ix)
    m, d, s, up, p = r["moist"], r["down"], r["sfc"], r["up"], r["pbl"]
    out = {"moist": {n: m[n].reshape(g3 if m[n].ndim == 2 else g2) for n in ("precnv", "precls", "cbmf", "iptop", "icnv", "qsat", "rh", "se")},
           "rad": {n: d[n].reshape(g3 if d[n].ndim == 2 else g2) for n in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "slrd", "tt_rsw")
                   if n in d},
           "sfc": {n: s[n].reshape((-1,) + g2) for n in surface.SFC_3 + ("hfluxn",)}, "pbl": {}}
    out["rad"].update(slr=up["slr"].reshape(g2), olr=up["olr"].reshape(g2), tt_rlw=up["tt_rlw"].reshape(g3))
    out["sfc"].update({n: s[n].reshape(g2) for n in ("tskin", "u0", "v0", "t0")})
    out["pbl"].update(ut_pbl=p["ut_pbl"].reshape(g2), vt_pbl=p["vt_pbl"].reshape(g2), tt_pbl=p["tt_pbl"].reshape(g3),
                      qt_pbl=p["qt_pbl"].reshape(g3))
    out["ts"], out["fsfcu"] = s["ts"].reshape(g2), s["slru"][2].reshape(g2)
    return out


def rad_state_array(state, kx):
    """the restatement's radiation state in the device's layout: [6 kx + 7, ncol] (csrc/spdy_radiation_column.hpp)"""
    n = state["slrd"].size
    return np.concatenate([state["tau2"].reshape(4 * kx, n), state["stratc"], state["tt_rsw"], state["flux"], state["dfabs"],
                           state["slrd"].reshape(1, n)])


def rad_state_rows(kx):
    """name -> rows of rad_state_array"""
    rows, at = {}, 0
    for n, size in (("tau2", 4 * kx), ("stratc", 2), ("tt_rsw", kx), ("flux", 4), ("dfabs", kx), ("slrd", 1)):
        rows[n] = slice(at, at + size)
        at += size
    return rows


# ------------------------------------------------------------------------------------------------ device side (torch)
def flat_outs(out):
    f = {}
    for k, v in out.items():
        if isinstance(v, dict):
            f.update({"%s.%s" % (k, n): t for n, t in v.items()})
        else:
            f[k] = v
    return f


def device_boundary(bnd, il, ix):
    return {n: support.dev(np.ascontiguousarray(v).reshape(1, il, ix)) for n, v in bnd.items()}


TEND = ("utend", "vtend", "ttend", "qtend")
KX = 8                    # the level count of the two-day and three-day runs (T30 L8)


def plan_case(tag, oracle_factory, levels_case=None):
    """(plan, oracle, Case, kx) of the tests that run the physics from spectra.  levels_case: (sp, o, half levels, Case seeds) of a
    count outside conftest.VARIANTS (tests/levels.py)"""
    if levels_case is None:
        kx = VARIANTS[tag][3]
        sp, o = support.plan(tag, 4 * kx + 4), oracle_factory(tag)
        case = Case(tag, sp, o)
    else:
        sp, o, hsg, seeds = levels_case
        kx, case = sp.kx, Case(tag, sp, o, hsg=hsg, seeds=seeds)
    sp.surface_set_orography(case.phis0)
    return sp, o, case, kx


def errors(out, exp, errs, label):
    """every optional output against the reference: integers identical; the floats' relative errors into errs"""
    got, want = flat_outs(out), flat_outs(exp)
    for n, w in want.items():
        g = got[n].cpu().numpy()[0]
        if g.dtype == np.int32:
            assert np.array_equal(g, w.astype(np.int32)), "%s: the device's %s is not the reference's (integers)" % (label, n)
        else:
            errs["%s %s" % (label, n)] = synth.relerr(g, w)


def check_physics_from_spectra(tag, sp, o, case, kx):
    """spdy_physics_dev on a shortwave call and a call without shortwave on the held state, on a plan, its oracle and their Case: the
    four tendencies, every optional output of every block and the radiation state against the reference within TOL, integers
    identical; returns the worst (array, error)"""
    import torch
    il, ix = sp.il, sp.ix
    st = case.st
    phi = o.geopotential(st["t"][0], st["phis"])
    spec = [support.dev(a) for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])]
    bnd = device_boundary(case.bnd, il, ix)
    S = torch.full((sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    rs, errs = {}, {}
    for step, sw in ((1, True), (2, False)):
        t0 = [synth.splitmix64(70 + 4 * step + i, kx * il * ix).reshape(kx, il, ix) * s for i, s in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
        ref_t = [a.copy() for a in t0]
        r = case.physics(st, sw, rs, *ref_t)
        if step == 1:
            check_coverage(r, tag)
        margin = float(r["margin"].min())
        assert margin >= MIN_MARGIN, "%s step %d: smallest decision margin %.3e below MIN_MARGIN %.1e" % (tag, step, margin, MIN_MARGIN)
        T, out = [support.dev(a) for a in t0], sp.column_outputs(1)
        if sw:
            ssrd = out["rad"]["ssrd"]
        else:                          # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = ssrd
        sp.physics_dev(sw, *spec, bnd, bnd["albsfc"], S, *T, out)
        torch.cuda.synchronize()
        for n, a, b in zip(TEND, T, ref_t):
            errs["step %d %s" % (step, n)] = synth.relerr(a.cpu().numpy(), b)
        exp = expected(r, kx, il, ix)
        if not sw:                     # written by shortwave calls only: the device leaves them as they were
            for n in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "tt_rsw"):
                exp["rad"].pop(n, None)
        errors(out, exp, errs, "step %d" % step)
        errs["step %d radiation state" % step] = synth.relerr(S.cpu().numpy().reshape(6 * kx + 7, il * ix), rad_state_array(rs, kx))
    top = sorted(errs.items(), key=lambda kv: -kv[1])
    print("\n[physics from spectra %s] %d arrays, worst %.1e; largest: %s" % (tag, len(errs), top[0][1],
                                                                             ", ".join("%s %.1e" % kv for kv in top[:8])))
    assert top[0][1] <= TOL, "%s: %s differs from the reference by %.3e, above TOL %.1e" % (tag, top[0][0], top[0][1], TOL)
    sp.close()
    return top[0]


def gridded(tag, nb, seed, plan=None, keep=None):
    """nb gridded states of surface.columns with the plan that holds their date and orography.  plan: (sp, its half levels) of a
    count outside support.PHYSICS_TAGS (tests/levels.py), used in place of the plan of tag.  keep: a dict that receives the reference
    side of the states (tab, zon, sqcoa, and the columns c1, c2 of the two calls)"""
    if plan is None:
        ix, il, kx = support.grid(tag)
        sp, hsg = support.plan(tag, 64), moist.HSG[kx]
    else:
        sp, hsg = plan
        ix, il, kx = sp.ix, sp.il, sp.kx
    sp.radiation_set_date(radiation.DATES[0])
    tab = moist.tables(hsg)
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, nb, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), nb, il, ix)
    c = surface.columns(tab, nb * il * ix, seed, zon, sqcoa)
    ph = c["phis0"].reshape(nb, il * ix)
    ph[:] = ph[0]
    sp.surface_set_orography(ph[0].reshape(il, ix))
    G = lambda a: support.dev(radiation.grids(a, nb, il, ix))
    c2 = dict(c, tg=c["tg2"], ug=c["vg"], vg=c["ug"], sst=c["sst"] + 0.5, stl=c["stl"] - 0.5, ttend=c["ttend2"])
    names = ("ug", "vg", "tg", "qg", "phig", "pslg", "albsfc") + TEND + surface.BOUNDARY
    if keep is not None:
        keep.update(tab=tab, zon=zon, sqcoa=sqcoa, c1=c, c2=c2)
    return sp, kx, il, ix, {n: G(c[n]) for n in names}, {n: G(c2[n]) for n in names}


def run_gridded(sp, nb, kx, il, ix, d1, d2, with_out):
    """a shortwave call, then a call without shortwave on the held state; returns everything written, by name"""
    import torch
    S = torch.full((nb * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    res = {"state": S}
    for i, d, sw in ((1, d1, True), (2, d2, False)):
        T = [d[n].clone() for n in TEND]
        out = sp.column_outputs(nb) if with_out else None
        if with_out and i == 2:        # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = res["out1.rad.ssrd"]
        sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], S, *T, out)
        res.update({"%s%d" % (n, i): t for n, t in zip(TEND, T)})
        if with_out:
            res.update({"out%d.%s" % (i, n): t for n, t in flat_outs(out).items()})
        if i == 1:
            torch.cuda.synchronize()
            res["state1"] = S.clone()
    torch.cuda.synchronize()
    return res


def rad_errors(got, ref):
    """got, ref [6 KX + 7, ncol]: the relative error of each part of the radiation state (tt_rsw is 1e-7 of the fluxes' size: one
    norm over the whole array would not see it)"""
    assert np.all(np.isfinite(got)), "radiation state not finite"
    return {n: synth.relerr(got[r], ref[r]) for n, r in rad_state_rows(KX).items()}


def checkpoint_errors(got, ref, ncol):
    """got: device tensors, ref: arrays, of one checkpoint -> {name: relative error, the larger of the plain and the mean-free norm}"""
    e = {}
    for k in PROG:
        g = got[k].cpu().numpy()
        assert np.all(np.isfinite(g.real)) and np.all(np.isfinite(g.imag)), "%s of the checkpoint is not finite" % k
        e[k] = max(synth.relerr(g, ref[k]), wave_relerr(g, ref[k]))
    rad = rad_errors(got["rad"].cpu().numpy().reshape(-1, ncol), ref["rad"])
    e["rad"] = max(rad.values())
    assert all(v == v for v in list(e.values()) + list(rad.values())), (          # max() drops a NaN
        "a relative error of the checkpoint is NaN", e, rad)
    return e
