"""The run with the whole physics AND the surface coupled: the reference side of tests/test_gpu_coupled_run.py.

physstep.reference_run's two cases (longrun.CASES: "rest", "wind") extended by surfmodel's driver in the main loop's order
(speedy.f90:27-54): initialize_coupler and set_forcing(0) at the start date, the two start-up steps, then for every leapfrog step
set_forcing(1) on the first step of a day (albedos, the real qcorh = grid_to_spec(corh), the zonal radiation forcing of the
date), the step with the surface model's own boundary fields, newdate, couple_sea_land on that step's hfluxn, shf, evap and the
held ssrd.  Three days (108 steps) from 30 January: over the month boundary, where obs_ssta runs."""
import numpy as np

import longrun
import modelstep
import physstep
import radiation
import support
import surface
import surfmodel as sm
import synth
from dynstep import PROG, ROB, oracle_dynamics_step

START = sm.WINDOWS["month"]
NSTEPS = 3 * sm.NSTEPS
CHECKPOINTS = (36, 72, 108)                       # each day's end
SKIP_AT, LATE_AT = 5, 37          # the faults: no couple_dev after step 5; the forcing of day 2 after step 37 instead of before it
# late_forcing moves forcing_dev behind the WHOLE of step 37 (its graph and its couple), not merely behind its physics_dev: step 37
# alone then runs with the albedos, snowc and qcorh of day 1, one day stale, and every later step has the right ones.  The test
# relies on that single step being noticed at the end of day 2 (step 72), 35 steps later.


def zonal(sp, case, tyear):
    """the zonal radiation forcing of the date from the plan's host tables (spdy_radiation_set_date on sp)"""
    sp.radiation_set_date(tyear)
    return radiation.zonal_columns({n: sp.table(n) for n in physstep.ZON}, 1, case.il, case.ix)


def setup(sp, o, name):
    """(case, climatology, restated surface model) of the run `name`"""
    case = physstep.run_case(sp, o, name)
    c = sm.climatology(case.phis0, longrun.latitudes(sp.table("sia_half")), start=START[:2])
    tab = sm.tables(c["fmask"], c["alb0"], sp.table("sia_half"), case.ix)
    return case, c, sm.Model(c, tab, ssta=sm.ssta_reader(c["fmask"]), start_year=START[0])


def reference_run(sp, o, name):
    """Returns (cps, log, events): cps {n: prognostics, "rad", "surf" (every field of the model), "qcorh"} at CHECKPOINTS; log one
    entry per step (n, sw, margin of the physics' decisions, the model's freezing-point margin so far); events {n: (date after the
    step's newdate, day changed, obs_ssta ran with this window)} for the device side's host calls."""
    case, c, model = setup(sp, o, name)
    kx, shape = case.kx, (case.il, case.ix)
    phis0 = case.phis0.reshape(-1)
    date = sm.Date(*START)
    model.couple(0, date)
    model.forcing(phis0)
    st = dict(case.st, qcorh=o.grid_to_spec(model.f["corh"].reshape(shape)))
    case.zon = zonal(sp, case, date.tyear)
    rs, rec, log, extra, events, count = {}, {}, [], {}, {}, [0]

    def step(j1, j2, dt, st):
        count[0] += 1
        n = count[0] - 2
        sw = physstep.shortwave_step(n)
        if n >= 1 and (n - 1) % sm.NSTEPS == 0:                       # set_forcing(1)
            model.forcing(phis0)
            st = dict(st, qcorh=o.grid_to_spec(model.f["corh"].reshape(shape)))
            case.zon = zonal(sp, case, date.tyear)
        bnd = {k: v.copy() for k, v in model.boundary().items()}
        new, _ = oracle_dynamics_step(o, st, j1, dt, 0.0 if j1 == 1 else ROB, j2=j2, physics=case.hook(sw, rs, rec, bnd))
        if n >= 1:
            key = date.key()
            date.newdate()
            s = rec["sfc"]
            shifted = model.couple(1 + (n + 1) // sm.NSTEPS, date, {"hfluxn": s["hfluxn"], "shf": s["shf"], "evap": s["evap"],
                                                                    "ssrd": rs["ssrd_held"]})
            events[n] = ((date.imont1, date.tmonth, date.tyear), date.key() != key, model.sstan3.copy() if shifted else None)
        log.append({"n": n, "sw": sw, "margin": float(rec["margin"].min()), "freeze": model.margin})
        if n in CHECKPOINTS:
            extra[n] = {"rad": physstep.rad_state_array(rs, kx), "surf": {k: v.copy() for k, v in model.f.items()},
                        "qcorh": np.array(st["qcorh"], copy=True)}
        return new
    cps = longrun.run(step, o.tail_init, st, nsteps=NSTEPS, checkpoints=CHECKPOINTS)
    for n in cps:
        cps[n].update(extra[n])
    return cps, log, events


# ------------------------------------------------------------------------------------------------ device side (torch)
def device_run(sp, case, c, events, fault=None):
    """The run on the device in the order of calls of DESIGN s14, as graph replays.  fault: None, "skip_couple" or "late_forcing" (SKIP_AT,
    LATE_AT).  Returns ({n: prognostics, rad, qcorh, surf
    at CHECKPOINTS}, node counts of the step graph without / with couple_dev)."""
    import torch
    s = support.package()
    il, ix, dt = sp.il, sp.ix, longrun.DELT
    shaped = {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + (il, ix)) for k, v in c.items()}
    M = s.SurfaceModel(sp, shaped, sm.DELT)
    D, W = modelstep.device_state(case.st), modelstep.Workspace(sp)
    out = sp.column_outputs(1, ("sfc", "rad"), names=("hfluxn", "shf", "evap", "ssrd"))
    F = dict(out["sfc"], **out["rad"])
    bnd, albsfc = M.boundary()
    P = {"bnd": dict(bnd, albsfc=albsfc), "rad": modelstep.radiation_state(sp)}
    phys = lambda sw: modelstep.whole_physics(P, sw, out)
    torch.cuda.synchronize()
    date = sm.Date(*START)
    M.set_date(date.imont1, date.tmonth, date.tyear)
    M.couple_dev(0)                                           # initialize_coupler
    M.forcing_dev(D["qcorh"])                                 # set_forcing(0)
    modelstep.startup(sp, dt, lambda j1, j2, dt_, n: modelstep.step(sp, D, W, dt_, j1, j2, 0.0, phys(physstep.shortwave_step(n))))
    couple = lambda: M.couple_dev(1, F["hfluxn"], F["shf"], F["evap"], F["ssrd"])     # day only tells 0 from > 0
    graphs = {}
    for sw in (True, False):
        for last in (False, True):
            with sp.graph_capture() as g:
                modelstep.step(sp, D, W, 2.0 * dt, physics=phys(sw))
                if last:
                    couple()
            graphs[sw, last] = g
    nodes = {k: g.num_nodes() for k, g in graphs.items()}
    res = {}
    for n in range(1, NSTEPS + 1):
        sw = physstep.shortwave_step(n)
        first = (n - 1) % sm.NSTEPS == 0
        if first and not (fault == "late_forcing" and n == LATE_AT):
            M.forcing_dev(D["qcorh"])
        (imont1, tmonth, tyear), new_day, sstan3 = events[n]
        if sstan3 is not None:                                # obs_ssta ran: the window the couple of this step reads
            M.set_sst_anomaly(sstan3.reshape(3, il, ix))
        if fault == "skip_couple" and n == SKIP_AT:
            graphs[sw, False].launch()
        elif new_day:                                         # the date changes between the step and its couple
            graphs[sw, False].launch()
            M.set_date(imont1, tmonth, tyear)
            couple()
        else:
            graphs[sw, True].launch()
        if fault == "late_forcing" and n == LATE_AT:
            M.forcing_dev(D["qcorh"])
        if n in CHECKPOINTS:
            sp.synchronize()
            res[n] = dict({k: D[k].clone() for k in PROG}, rad=P["rad"].clone(), qcorh=D["qcorh"].clone(),
                          surf={k: M.field(k).numpy().reshape(-1) for k in sm.FIELDS + sm.FORCING})
            torch.cuda.synchronize()
    for g in graphs.values():
        g.close()
    M.close()
    return res, nodes


def errors(got, ref, ncol):
    """physstep.checkpoint_errors plus qcorh and every field of the surface model (an all-zero reference field: the absolute error)"""
    e = physstep.checkpoint_errors(got, ref, ncol)
    e["qcorh"] = synth.relerr(got["qcorh"].cpu().numpy(), ref["qcorh"])
    for k, v in ref["surf"].items():
        x = got["surf"][k]
        assert np.all(np.isfinite(x)), "%s of the surface model is not finite at the checkpoint" % k
        s = np.abs(v).max()
        e[k] = float(np.abs(x - v).max() / s) if s > 0 else float(np.abs(x).max())
    return e
