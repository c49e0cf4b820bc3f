"""GPU: longrun's "rest" and "wind" cases with the whole physics AND the surface coupled, in the order of calls of DESIGN s14: the
start-up steps, then three days (108 leapfrog steps) from 30 January, over the month boundary, as graph replays.  The step reads
the surface model's own arrays (spdy_surface_model_boundary) and writes out.sfc.hfluxn / shf / evap and out.rad.ssrd, which
couple_dev reads as the LAST NODE of the step's graph on steps within a day; on a day's last step the graph without it is
replayed, the host sets the new date and couple_dev is issued eagerly; forcing_dev (albedos and the real qcorh, written into the
array the step reads) precedes the first step of a day.  The reference side is tests/coupledrun.py (its conditions are asserted on
the CPU by tests/test_coupled_run_cpu.py and again here).  At each day's end the prognostics, the radiation state, qcorh and every
field of the surface model agree within TOL.  The test notices what it is for: with couple_dev skipped for one step, or
forcing_dev issued after a day's first step instead of before it, the first checkpoint after the fault fails."""
import numpy as np
import pytest

import coupledrun
import longrun
import modelstep
import moist
import physstep
import surfmodel as sm
import synth
from conftest import TOL
from modelstep import PROG
from test_gpu_physics_run import KX, _checkpoint_errors

pytestmark = pytest.mark.gpu

SKIP_AT, LATE_AT = 5, 37          # the faults: no couple_dev after step 5; the forcing of day 2 after step 37 instead of before it
# late_forcing moves forcing_dev behind the WHOLE of step 37 (its graph and its couple), not merely behind its physics_dev: step 37
# alone then runs with the albedos, snowc and qcorh of day 1, one day stale, and every later step has the right ones.  The test
# relies on that single step being noticed at the end of day 2 (step 72), 35 steps later.


def _device_run(sp, case, c, events, fault=None):
    """Returns ({n: prognostics, rad, qcorh, surf at CHECKPOINTS}, node counts of the step graph without / with couple_dev)."""
    import torch
    s = moist.package()
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
    date = sm.Date(*coupledrun.START)
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
    for n in range(1, coupledrun.NSTEPS + 1):
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
        if n in coupledrun.CHECKPOINTS:
            sp.synchronize()
            res[n] = dict({k: D[k].clone() for k in PROG}, rad=P["rad"].clone(), qcorh=D["qcorh"].clone(),
                          surf={k: M.field(k).numpy().reshape(-1) for k in sm.FIELDS + sm.FORCING})
            torch.cuda.synchronize()
    for g in graphs.values():
        g.close()
    M.close()
    return res, nodes


def _errors(got, ref, ncol):
    e = _checkpoint_errors(got, ref, ncol)
    e["qcorh"] = synth.relerr(got["qcorh"].cpu().numpy(), ref["qcorh"])
    for k, v in ref["surf"].items():
        x = got["surf"][k]
        assert np.all(np.isfinite(x)), k
        s = np.abs(v).max()
        e[k] = float(np.abs(x - v).max() / s) if s > 0 else float(np.abs(x).max())
    return e


@pytest.mark.parametrize("name", list(longrun.CASES))
def test_three_day_coupled_run(name, oracle_factory):
    o = oracle_factory("t30")
    sp = moist.plan("t30", 4 * KX + 4)
    cps, log, events = coupledrun.reference_run(sp, o, name)
    case, c, _ = coupledrun.setup(sp, o, name)
    assert min(e["margin"] for e in log) >= physstep.RUN_MARGIN and log[-1]["freeze"] >= physstep.RUN_MARGIN
    sp.surface_set_orography(case.phis0)
    sp.physics_workspace()
    sp.use_own_stream()
    ncol = sp.il * sp.ix
    got, nodes = _device_run(sp, case, c, events)
    lines, worst = [], ("", 0.0)
    for n in coupledrun.CHECKPOINTS:
        e = _errors(got[n], cps[n], ncol)
        top = sorted(e.items(), key=lambda kv: -kv[1])[:6]
        lines.append("step %3d: " % n + " ".join("%s %.1e" % kv for kv in top))
        worst = max([worst] + [("step %d %s" % (n, k), v) for k, v in e.items()], key=lambda x: x[1])
    print("\n[3-day coupled run '%s' vs the reference side, largest relative errors; decision margin %.1e, freezing-point margin %.1e]\n  "
          % (name, min(e["margin"] for e in log), log[-1]["freeze"]) + "\n  ".join(lines))
    print("[graph nodes] step %d, step + couple_dev %d (shortwave %d, %d)" % (nodes[False, False], nodes[False, True], nodes[True, False],
                                                                            nodes[True, True]))
    assert worst[1] <= TOL, (name, worst)
    assert nodes[False, True] == nodes[False, False] + 1 and nodes[True, True] == nodes[True, False] + 1, nodes
    # the test notices what it is for: the first checkpoint after each fault fails
    for fault, cp in (("skip_couple", 36), ("late_forcing", 72)):
        bad, _ = _device_run(sp, case, c, events, fault)
        e = _errors(bad[cp], cps[cp], ncol)
        print("[fault %s] largest relative error at step %d: %.1e" % (fault, cp, max(e.values())))
        assert max(e.values()) > TOL, (fault, cp)
    sp.close()
