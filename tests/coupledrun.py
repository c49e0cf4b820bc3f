"""The run with the whole physics AND the surface coupled: the reference side of tests/test_gpu_coupled_run.py.

physstep.reference_run's two cases (longrun.CASES: "rest", "wind") extended by surfmodel's driver in the main loop's order
(speedy.f90:27-54): initialize_coupler and set_forcing(0) at the start date, the two start-up steps, then for every leapfrog step
set_forcing(1) on the first step of a day (albedos, the real qcorh = grid_to_spec(corh), the zonal radiation forcing of the
date), the step with the surface model's own boundary fields, newdate, couple_sea_land on that step's hfluxn, shf, evap and the
held ssrd.  Three days (108 steps) from 30 January: over the month boundary, where obs_ssta runs."""
import numpy as np

import longrun
import physstep
import radiation
import surface
import surfmodel as sm
from dynstep import ROB, oracle_dynamics_step

START = sm.WINDOWS["month"]
NSTEPS = 3 * sm.NSTEPS
CHECKPOINTS = (36, 72, 108)                       # each day's end


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
