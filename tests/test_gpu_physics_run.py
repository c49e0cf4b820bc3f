"""GPU: the time step with the whole physics over a two-day run at the model's own time step -- the reference's start-up sequence
(time_stepping.f90:12-24) and 72 leapfrog steps at delt = 2400 s from its rest state (tests/longrun.py), the shortwave radiation
in the reference's cadence (speedy.f90:35, nstrad = 3) on ONE radiation state, as replays of two captured graphs; and the step
resynchronised with the reference at four points of that run, where every column's every output is compared.  The reference side
is tests/physstep.py: reference_run (oracle_dynamics_step + the NumPy restatements of the physics); its conditions are asserted
on the CPU by tests/test_physics_run_cpu.py and again here."""
import numpy as np
import pytest

import longrun
import modelstep
import physstep
import support
import synth
from conftest import TOL
from dynstep import wave_relerr
from modelstep import PROG
from physstep import KX, TEND

pytestmark = pytest.mark.gpu


def _setup(name, oracle_factory):
    o = oracle_factory("t30")
    sp = support.plan("t30", 4 * KX + 4)
    case = physstep.run_case(sp, o, name)
    sp.surface_set_orography(case.phis0)
    sp.physics_workspace()
    sp.use_own_stream()
    return sp, o, case


def _device_run(sp, case, adiabatic_nodes=False):
    """Start-up steps as eager calls with the three initialize_implicit calls, then one graph with and one without shortwave,
    captured once each and replayed in the reference's cadence; nothing but replays between checkpoints.  The radiation state
    starts as NaN.  Returns ({n: clones of the prognostics and the radiation state after leapfrog step n}, node counts)."""
    import torch
    dt = longrun.DELT
    D, W, P = modelstep.device_state(case.st), modelstep.Workspace(sp), modelstep.physics_buffers(sp, case.bnd)
    torch.cuda.synchronize()
    phys = lambda sw: modelstep.whole_physics(P, sw)
    modelstep.startup(sp, dt, lambda j1, j2, dt_, n: modelstep.step(sp, D, W, dt_, j1, j2, 0.0, phys(physstep.shortwave_step(n))))
    graphs = {}
    torch.cuda.synchronize()
    for sw in (True, False):
        with sp.graph_capture() as g:
            modelstep.step(sp, D, W, 2.0 * dt, physics=phys(sw))
        graphs[sw] = g
    nodes = {sw: g.num_nodes() for sw, g in graphs.items()}
    out = {}
    for n in range(1, longrun.NSTEPS + 1):
        graphs[physstep.shortwave_step(n)].launch()
        if n in longrun.CHECKPOINTS:
            sp.synchronize()
            out[n] = dict({k: D[k].clone() for k in PROG}, rad=P["rad"].clone())
            torch.cuda.synchronize()                      # the clones are torch's stream's, the next replay the plan's
    if adiabatic_nodes:
        with sp.graph_capture() as g0:
            modelstep.step(sp, D, W, 2.0 * dt)
        nodes["adiabatic"] = g0.num_nodes()
        g0.close()
    for g in graphs.values():
        g.close()
    return out, nodes


@pytest.mark.parametrize("name", ["rest", "wind"])
def test_two_day_run_with_physics(name, oracle_factory):
    """BASELINE config 1's stand-in WITH its physics on the device: start-up steps eager, then 72 replays of two captured graphs
    (shortwave / none) in the reference's cadence, from the reference's rest state at delt = 2400 s, the radiation state NaN
    before the first step.  At every checkpoint vor, div, t, tr, ps (plain and mean-free norm) and every part of the radiation
    state within TOL = 1e-12 of the reference side (oracle_dynamics_step + the restatements of the physics), whose every decision
    of every column on every step is >= RUN_MARGIN from its threshold: no column is excluded.  A second run from the same
    inputs and a run with the plan option "physics_fused" 0 are bit-equal at every checkpoint; each graph has exactly 3 nodes
    more than the adiabatic step's.
    Measured on MI355X (profiles/r07_two_day_physics_run_error.txt): prognostics worst 2.3e-14 ("rest", div at step 36), 2.4e-15
    ("wind"); radiation state worst 6.9e-14 / 1.3e-13 at step 72; nodes 4 -> 7.  With the cadence shifted by one step, the radiation
    state zeroed between replays or the physics reading level j2 in the start-up steps the test fails at the first checkpoint
    after the change."""
    import torch
    sp, o, case = _setup(name, oracle_factory)
    ncol = sp.il * sp.ix
    cps, log, _ = physstep.reference_run(case)
    margin = min(e["margin"] for e in log)
    assert margin >= physstep.RUN_MARGIN, margin
    got, nodes = _device_run(sp, case, adiabatic_nodes=True)
    lines, worst = [], ("", 0.0)
    for n in longrun.CHECKPOINTS:
        e = physstep.checkpoint_errors(got[n], cps[n], ncol)
        lines.append("step %2d: " % n + " ".join("%s %.1e" % kv for kv in e.items()))
        worst = max([worst] + [("step %d %s" % (n, k), v) for k, v in e.items()], key=lambda x: x[1])
    print("\n[2-day run with the whole physics '%s' vs the reference side, relative error (max of plain and mean-free norm); "
          "smallest decision margin %.1e]\n  " % (name, margin) + "\n  ".join(lines))
    print("[graph nodes] adiabatic %(adiabatic)d, with the whole physics %(False)d (shortwave %(True)d)" % {str(k): v for k, v in nodes.items()})
    assert worst[1] <= TOL, (name, worst)
    assert nodes[True] - nodes["adiabatic"] == 3 and nodes[False] - nodes["adiabatic"] == 3, nodes

    again, _ = _device_run(sp, case)
    sp.set_option("physics_fused", 0)
    five, nodes5 = _device_run(sp, case)
    sp.set_option("physics_fused", 1)
    assert nodes5[True] > nodes[True]                     # the option took effect: five launches, not one
    for n in longrun.CHECKPOINTS:
        for k in got[n]:
            assert torch.equal(again[n][k], got[n][k]), ("second run", n, k)
            assert torch.equal(five[n][k], got[n][k]), ("five calls", n, k)
    sp.close()


@pytest.mark.parametrize("name", ["wind"])
def test_resynchronised_steps(name, oracle_factory):
    """test_physics_from_spectra on columns the model made: before leapfrog steps 10 and 37 (shortwave) and 38 and 72 (none) of
    "wind" the device takes the reference's state (both time levels, its radiation state and held ssrd) and (i) physics_dev with
    every optional output gives the four tendencies, all outputs and the radiation state within TOL and the integers identical
    on every column; (ii) one whole step gives the prognostics, the PL operands and the radiation state of
    oracle_dynamics_step within TOL.  Measured on MI355X: 204 arrays, worst 1.0e-13 (tt_pbl before step 37)."""
    import torch
    sp, o, case = _setup(name, oracle_factory)
    il, ix, dt = sp.il, sp.ix, 2.0 * longrun.DELT
    ncol = il * ix
    _, log, pre = physstep.reference_run(case, physstep.RESYNC)        # leaves o.tail_init(2 delt) in place
    assert sorted(pre) == sorted(physstep.RESYNC)
    sp.initialize_implicit(dt)
    bnd = physstep.device_boundary(case.bnd, il, ix)
    W = modelstep.Workspace(sp)
    errs = {}
    for n in physstep.RESYNC:
        sw, st = physstep.shortwave_step(n), pre[n]["st"]
        assert log[n + 1]["n"] == n and log[n + 1]["margin"] >= physstep.RUN_MARGIN
        # (i) the physics alone, from zero tendencies
        rs = {k: v.copy() for k, v in pre[n]["rs"].items()}
        ref_t = [np.zeros((KX, il, ix)) for _ in TEND]
        r = case.physics(st, sw, rs, *ref_t)
        assert float(r["margin"].min()) >= physstep.RUN_MARGIN
        held = support.dev(pre[n]["rs"]["ssrd_held"].reshape(1, il, ix))
        S = support.dev(physstep.rad_state_array(pre[n]["rs"], KX).reshape(-1))
        phi = o.geopotential(st["t"][0], st["phis"])
        spec = [support.dev(a) for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])]
        T, out = [support.dev(a * 0.0) for a in ref_t], sp.column_outputs(1)
        if not sw:                      # ssrd stays where the last shortwave call put it (include/spdy.h): the reference's
            out["rad"]["ssrd"] = held.clone()
        torch.cuda.synchronize()        # the uploads are torch's stream's, the calls the plan's
        sp.physics_dev(sw, *spec, bnd, bnd["albsfc"], S, *T, out)
        torch.cuda.synchronize()
        label = "step %d physics" % n
        for name, a, b in zip(TEND, T, ref_t):
            errs["%s %s" % (label, name)] = synth.relerr(a.cpu().numpy(), b)
        exp = physstep.expected(r, KX, il, ix)
        if not sw:
            for name in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "tt_rsw"):
                exp["rad"].pop(name, None)
            assert torch.equal(out["rad"]["ssrd"], held)
        physstep.errors(out, exp, errs, label)
        after = physstep.rad_state_array(rs, KX)
        for name, e in physstep.rad_errors(S.cpu().numpy().reshape(-1, ncol), after).items():
            errs["%s state %s" % (label, name)] = e
        # (ii) the whole step
        D = modelstep.device_state(st)
        P = {"bnd": bnd, "rad": support.dev(physstep.rad_state_array(pre[n]["rs"], KX).reshape(-1))}
        torch.cuda.synchronize()
        modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, sw, out={"rad": {"ssrd": held}}))
        sp.synchronize()
        label = "step %d whole" % n
        for k in PROG:
            g = D[k].cpu().numpy()
            errs["%s %s" % (label, k)] = max(synth.relerr(g, pre[n]["new"][k]), wave_relerr(g, pre[n]["new"][k]))
        errs["%s PL" % label] = synth.relerr(W.PL.cpu().numpy(), pre[n]["out"]["PL"])
        for name, e in physstep.rad_errors(P["rad"].cpu().numpy().reshape(-1, ncol), after).items():
            errs["%s state %s" % (label, name)] = e
    assert all(v == v for v in errs.values()), [k for k, v in errs.items() if v != v]
    top = sorted(errs.items(), key=lambda kv: -kv[1])
    print("\n[resynchronised steps] %d arrays, worst %.1e; largest: %s" % (len(errs), top[0][1],
                                                                          ", ".join("%s %.1e" % kv for kv in top[:10])))
    assert top[0][1] <= TOL, top[0]
    sp.close()
