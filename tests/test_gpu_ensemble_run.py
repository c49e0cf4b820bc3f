"""GPU: the coupled ensemble run (include/spdy.h "ensemble time step", "surface models", "diagnostics"): ONE surface
model and ONE guard for the E members of an ensemble, one launch per call each, and a humidity correction qcorh per member in the
spectral step.  Members have DIFFERENT states and boundary fields (tests/test_gpu_ensemble.py's construction); every member must
come out, bit for bit, as the single-state step with a single SurfaceModel and a single Diagnostics leaves that member's state, and
a coupled three-day run of two members is held to the reference side of tests/test_gpu_coupled_run.py."""
import ctypes

import numpy as np
import pytest

import coupledrun
import diagnostics as dg
import ensemblerun as er
import ensemblestep as es
import longrun
import modelstep
import physstep
import support
import surfmodel as sm
from conftest import TOL
from dynstep import ROB

pytestmark = pytest.mark.gpu

ARG = -1
STEP_ENTRIES = [n for n, (what, _) in enumerate(er.SEQUENCE) if what == "step"]
FORCING_ENTRIES = [n for n, (what, _) in enumerate(er.SEQUENCE) if what == "forcing"]


def _coupled_members(sp, o, E):
    """E physically shaped states with per-member boundary fields over member 0's orography, and the climatology over it"""
    sts, bnds = es.physics_members(sp, o, E)
    phis0 = o.spec_to_grid(sts[0]["phis"], 1)
    clim = er.shaped(sm.climatology(phis0, longrun.latitudes(sp.table("sia_half"))), sp.grid_shape)
    return sts, bnds, clim


@pytest.mark.parametrize("E", [3, 1])
def test_member_equals_its_single_objects(E, oracle_factory):
    """T30 L8.  couple_dev(0) and forcing_dev; two steps with the physics, shortwave on the first, each followed by check_dev and
    couple_dev(1); forcing_dev again and a third step (ensemblerun.SEQUENCE).  Every member's prognostics, phi, operands, radiation
    state, surface-model fields, qcorh and guard rows are bit-equal to the single-state run of that member.  E = 1: the new creates
    and the option set against the existing entry points.  The test notices what it is for: after the second forcing the members'
    qcorh differ, and with member 0's qcorh in every slot the other members' third-step tr comes out differently."""
    s = support.package()
    dt = physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds, clim = _coupled_members(sp, o, E)
    sp.initialize_implicit(dt)
    snaps, rows, _ = er.run_ensemble(sp, s, es, sts, bnds, clim, dt, ROB)
    size = sp.radiation_state_size()
    last = snaps[-1]
    assert np.isfinite(last["vor"][:, 0].cpu().numpy()).all() and np.isfinite(rows[0]).all()
    assert all(np.isfinite(last["surf"][k]).all() for k in er.SURF)
    for e in range(E):
        ref_snaps, ref_rows, _ = er.run_single(sp, s, es, modelstep, sts[e], bnds[e], clim, dt, ROB)
        assert er.member_differences(es, snaps, rows, e, ref_snaps, ref_rows, size) == [], (E, e)
    if E > 1:
        q = snaps[FORCING_ENTRIES[1]]["qcorh"]
        for e in range(1, E):
            assert not support.same_bits(q[e], q[0]), e
            assert not np.array_equal(last["surf"]["sst_am"][e], last["surf"]["sst_am"][0]), e
        assert not np.array_equal(rows[0], rows[1])
        shared, _, _ = er.run_ensemble(sp, s, es, sts, bnds, clim, dt, ROB, same_qcorh=True)
        assert support.same_bits(shared[-1]["tr"][:, 0], last["tr"][:, 0])               # member 0 has its own either way
        for e in range(1, E):
            assert not support.same_bits(shared[-1]["tr"][:, e], last["tr"][:, e]), e
    sp.close()


def _guard_inputs(sp, E):
    """three checked steps of E members [step][name] -> (E, kx, nx, mx) host arrays: step 0 in range; step 1 member 1 too warm at
    level 3 and with reke > 500 at level 5; step 2 member 1 back in range and member 2 too cold at level 0"""
    base = [dg.state(sp, 5100 + 100 * e) for e in range(E)]
    elm2 = sp.table("elm2")
    steps = [{n: np.stack([b[n] for b in base]) for n in ("vor", "div", "t")} for _ in range(3)]
    x = steps[1]
    x["t"][1, 3, 0, 0] = complex(400.0 / dg.SQRT_HALF, x["t"][1, 3, 0, 0].imag)
    reke5 = dg.diag(base[1]["vor"], base[1]["div"], base[1]["t"], elm2)[0, 5]
    x["vor"][1, 5] *= np.sqrt(1000.0 / reke5)
    steps[2]["t"][2, 0, 0, 0] = complex(100.0 / dg.SQRT_HALF, steps[2]["t"][2, 0, 0, 0].imag)
    return steps


def test_guard_isolation_stickiness_and_ring():
    """E = 3, capacity 2, three check_dev calls on constructed spectra (finite values only)."""
    s = support.package()
    E = 3
    sp = support.ensemble_plan("t30", E)
    kx, elm2 = sp.kx, sp.table("elm2")
    steps = _guard_inputs(sp, E)
    want = np.array([[dg.diag(x["vor"][e], x["div"][e], x["t"][e], elm2) for x in steps] for e in range(E)])     # [E, 3, 3, kx]
    masks = [[dg.masks(want[e, n]) for n in range(3)] for e in range(E)]
    assert all(not m.any() for m in masks[0]) and not masks[1][0].any() and not masks[1][2].any() and not masks[2][1].any()
    assert masks[1][1][3] == dg.TEMP_HIGH and masks[1][1][5] == dg.REKE and np.count_nonzero(masks[1][1]) == 2
    assert masks[2][2][0] == dg.TEMP_LOW and np.count_nonzero(masks[2][2]) == 1
    G = s.Diagnostics(sp, capacity=2, first_step=0, nmem=E)
    got = np.zeros_like(want)
    for n, x in enumerate(steps):
        G.check_dev(*[support.dev(x[k]) for k in ("vor", "div", "t")])
        for e in range(E):
            got[e, n] = G.read(n, 1, member=e)[0]
    bad = (ctypes.c_longlong * E)()
    assert sp.lib.spdy_ens_diagnostics_stopped(G.h, bad) == 2 and list(bad) == [-1, 1, 2] == G.stopped()
    st = [G.status(e) for e in range(E)]
    assert st[1]["bad_step"] == 1 and st[1]["bad_level"] == 3 and st[1]["bad_mask"] == dg.TEMP_HIGH | dg.REKE
    assert np.array_equal(st[1]["bad_row"], got[1, 1])
    assert st[0]["bad_step"] == -1 and st[0]["bad_row"] is None and st[0]["bad_mask"] == 0
    assert st[2]["bad_step"] == 2 and st[2]["bad_level"] == 0 and st[2]["bad_mask"] == dg.TEMP_LOW
    assert np.array_equal(st[2]["bad_row"], got[2, 2])         # member 1's offence at step 1 did not freeze member 2's saved row
    assert [x["next_step"] for x in st] == [3, 3, 3]
    rows = np.zeros((2, 3, kx))
    for e in range(E):
        assert sp.lib.spdy_ens_diagnostics_read(G.h, e, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)) == ARG      # overwritten
        assert np.array_equal(G.read(1, 2, member=e), got[e, 1:])                  # every member's ring went on following the step
    with pytest.raises(s.SpdyError) as err:
        G.read(1, 1, member=E)
    assert err.value.code == ARG
    with pytest.raises(s.DiagnosticsStop) as stop:
        G.raise_if_stopped()
    assert stop.value.status["member"] == 1 and " member 1\n" + dg.lines(1, got[1, 1]) + dg.STOP == str(stop.value)
    # a single object on each member's slice: the same bits; the restatement: within the bound of DESIGN s16
    bound = 2.0 * (sp.mx * sp.nx - 1) * 2.0 ** -53
    for e in range(E):
        d = s.Diagnostics(sp, capacity=2, first_step=0)
        for n, x in enumerate(steps):
            d.check_dev(*[support.dev(np.ascontiguousarray(x[k][e])) for k in ("vor", "div", "t")])
            assert np.array_equal(d.read(n, 1)[0], got[e, n]), (e, n)
        assert d.status()["bad_step"] == st[e]["bad_step"] and d.status()["bad_mask"] == st[e]["bad_mask"]
        d.close()
        rel = float(np.abs(got[e] / want[e] - 1.0).max())
        print("[guard, member %d] rows vs the restatement %.1e (bound %.1e)" % (e, rel, bound))
        assert rel <= bound, (e, rel)
    G.close()
    sp.close()


def _surface_setup(sp, E, s):
    import torch
    phis0 = sm.orography(sp)
    sp.surface_set_orography(phis0)
    clim = er.shaped(sm.climatology(phis0, longrun.latitudes(sp.table("sia_half"))), sp.grid_shape)
    ncol = phis0.size
    flux = [sm.fluxes(1 + e, ncol) for e in range(E)]
    shape = {"hfluxn": (2,), "shf": (3,), "evap": (3,), "ssrd": ()}
    F = {k: torch.from_numpy(np.stack([np.ascontiguousarray(f[k]).reshape(shape[k] + sp.grid_shape) for f in flux])).cuda()
         for k in er.FLUXES}
    return clim, F


def _surface_run(sp, s, clim, F, nmem):
    """couple(0), couple(1) on F, forcing: every field and qcorh"""
    import torch
    M = s.SurfaceModel(sp, clim, sm.DELT, nmem=nmem)
    date = sm.Date(*er.DATE)
    M.set_date(date.imont1, date.tmonth, date.tyear)
    M.couple_dev(0)
    before = {k: M.field(k).numpy() for k in er.SHARED_FIELDS}
    M.couple_dev(1, *[F[k] for k in er.FLUXES])
    q = torch.zeros((nmem,) + sp.spec_shape, dtype=torch.complex128, device="cuda")
    M.forcing_dev(q)
    sp.synchronize()
    res = {k: M.field(k).numpy().reshape((nmem,) + sp.grid_shape) for k in er.SURF + ("fmask_l",)}
    after = {k: M.field(k).numpy() for k in er.SHARED_FIELDS}
    M.close()
    return res, q, before, after


def test_coupler_isolation():
    """E = 3, member 1's flux inputs all NaN: members 0 and 2 come out as in the clean run, the shared fields are untouched"""
    s = support.package()
    E = 3
    sp = support.plan("t30", max_batch=4)
    clim, F = _surface_setup(sp, E, s)
    clean, q0, _, _ = _surface_run(sp, s, clim, F, E)
    bad = {k: v.clone() for k, v in F.items()}
    for v in bad.values():
        v[1] = float("nan")
    got, q1, before, after = _surface_run(sp, s, clim, bad, E)
    for e in (0, 2):
        for k in er.SURF + ("fmask_l",):
            assert np.array_equal(got[k][e], clean[k][e], equal_nan=True), (e, k)
        assert support.same_bits(q1[e], q0[e]), e
    assert np.isnan(got["stl_lm"][1]).any() and np.isfinite(clean["stl_lm"]).all()
    assert not np.array_equal(clean["stl_lm"][0], clean["stl_lm"][2])             # the members' fluxes differ
    for k in er.SHARED_FIELDS:
        assert np.array_equal(before[k], after[k]) and np.isfinite(after[k]).all(), k
    for e in range(E):
        assert np.array_equal(got["fmask_l"][e], got["fmask_l"][0])
    sp.close()


def test_graph(oracle_factory):
    """{the coupled ensemble step, check_dev, couple_dev(1)} captured as one graph per shortwave setting: exactly the nodes of the
    single-state step captured by the same sequence with its two single objects; the replays (the graph without shortwave runs
    twice) give the eager calls' bits; the guard's counter advances by one per replay for every member."""
    s = support.package()
    E, dt = 3, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds, clim = _coupled_members(sp, o, E)
    sp.initialize_implicit(dt)
    sp.use_own_stream()
    eager, rows, _ = er.run_ensemble(sp, s, es, sts, bnds, clim, dt, ROB)
    snaps, grows, nodes = er.run_ensemble(sp, s, es, sts, bnds, clim, dt, ROB, graph=True)
    _, _, nodes1 = er.run_single(sp, s, es, modelstep, sts[0], bnds[0], clim, dt, ROB, graph=True)
    print("[graph nodes of step + check_dev + couple_dev, shortwave / not] ensemble of %d: %s, single state: %s" % (E, nodes, nodes1))
    assert nodes == nodes1 and len(nodes) == 2
    for n, (a, b) in enumerate(zip(snaps, eager)):
        bad = [k for k in es.COMPARED + ("rad", "qcorh") if not support.same_bits(a[k], b[k])]
        bad += [k for k in er.SURF if not np.array_equal(a["surf"][k], b["surf"][k], equal_nan=True)]
        assert bad == [], (n, bad)
    assert np.array_equal(grows, rows, equal_nan=True)
    done = 0
    for n, snap in enumerate(snaps):
        done += n in STEP_ENTRIES
        assert snap["next_step"] == [done] * E, (n, snap["next_step"])
    sp.close()


def _ensemble_days(sp, cases, c, events):
    """test_gpu_coupled_run._device_run for the members of an ensemble, in the order of calls of DESIGN s17: ONE surface model and
    ONE guard.  Returns ({n: [per member: prognostics, rad, qcorh, surf]}, node counts, the guard's state at the end)."""
    import torch
    s = support.package()
    E, dt = len(cases), longrun.DELT
    M = s.SurfaceModel(sp, er.shaped(c, sp.grid_shape), sm.DELT, nmem=E)
    G = s.Diagnostics(sp, capacity=8, first_step=1, nmem=E)
    ens = s.Ensemble(sp, E, member_qcorh=True)
    ens.set_shared(cases[0].st)
    for e, case in enumerate(cases):
        ens.set_member(e, case.st)
    out = sp.column_outputs(E, ("sfc", "rad"), names=er.FLUXES)
    F = dict(out["sfc"], **out["rad"])
    bnd, albsfc = M.boundary()
    size = sp.radiation_state_size()
    P = {"bnd": bnd, "albsfc": albsfc, "out": out, "rad": torch.full((E * size,), float("nan"), dtype=torch.float64, device="cuda")}
    ens.physics_workspace()
    torch.cuda.synchronize()
    date = sm.Date(*coupledrun.START)
    M.set_date(date.imont1, date.tmonth, date.tyear)
    M.couple_dev(0)
    M.forcing_dev(ens.qcorh)
    ens.startup(dt, lambda n: dict(P, sw=physstep.shortwave_step(n)))
    couple = lambda: M.couple_dev(1, *[F[k] for k in er.FLUXES])
    graphs, nodes = {}, {}
    for sw in (True, False):
        with sp.graph_capture() as g:
            ens.step(2, 2, 2.0 * dt, dict(P, sw=sw))
        nodes[sw, "step"] = g.num_nodes()
        g.close()
        for last in (False, True):
            with sp.graph_capture() as g:
                ens.step(2, 2, 2.0 * dt, dict(P, sw=sw))
                G.check_dev(ens.vor[1], ens.div[1], ens.t[1])
                if last:
                    couple()
            graphs[sw, last] = g
            nodes[sw, last] = g.num_nodes()
    res = {}
    for n in range(1, coupledrun.NSTEPS + 1):
        sw = physstep.shortwave_step(n)
        if (n - 1) % sm.NSTEPS == 0:
            M.forcing_dev(ens.qcorh)
        (imont1, tmonth, tyear), new_day, sstan3 = events[n]
        if sstan3 is not None:
            M.set_sst_anomaly(sstan3.reshape((3,) + sp.grid_shape))
        if new_day:
            graphs[sw, False].launch()
            M.set_date(imont1, tmonth, tyear)
            couple()
        else:
            graphs[sw, True].launch()
        if n in coupledrun.CHECKPOINTS:
            sp.synchronize()
            surf = {k: M.field(k).numpy() for k in er.SURF}
            res[n] = [dict({k: getattr(ens, k)[:, e].clone() for k in es.PROG}, rad=P["rad"][e * size:(e + 1) * size].clone(),
                           qcorh=ens.qcorh[e].clone(), surf={k: v[e].reshape(-1) for k, v in surf.items()}) for e in range(E)]
            torch.cuda.synchronize()
    guard = {"stopped": G.stopped(), "next_step": [G.status(e)["next_step"] for e in range(E)]}
    for g in graphs.values():
        g.close()
    M.close(); G.close()
    return res, nodes, guard


def test_coupled_days_against_the_reference(oracle_factory):
    """E = 2: member 0 is longrun's "rest" case, member 1 its "wind" case, over the same seeded orography and climatology.  Driven as
    tests/test_gpu_coupled_run.py drives one state: the start-up steps, then the three days of coupledrun (108 steps, the whole
    run) as graph replays, forcing_dev before a day's first step, set_date / set_sst_anomaly from the reference run's events.  At
    every checkpoint each member is within conftest.TOL of coupledrun.reference_run of its case and bit-equal to coupledrun.device_run of its
    case.  The run uses the batched objects: the guard and the coupler add two nodes to the step's graph, whatever E."""
    names = ("rest", "wind")
    E = len(names)
    o = oracle_factory("t30")
    sp = support.ensemble_plan("t30", E)
    refs = [coupledrun.reference_run(sp, o, name) for name in names]
    setups = [coupledrun.setup(sp, o, name) for name in names]
    cases, c = [x[0] for x in setups], setups[0][1]
    # what the layout shares is shared by the two cases
    for k in ("phis", "tcorh"):
        assert np.array_equal(cases[0].st[k], cases[1].st[k]), k
    assert np.array_equal(cases[0].phis0, cases[1].phis0) and all(np.array_equal(c[k], setups[1][1][k]) for k in c)
    events = refs[0][2]
    for n in events:
        assert events[n][:2] == refs[1][2][n][:2] and (events[n][2] is None) == (refs[1][2][n][2] is None)
        assert events[n][2] is None or np.array_equal(events[n][2], refs[1][2][n][2])
    for cps, log, _ in refs:
        assert min(x["margin"] for x in log) >= physstep.RUN_MARGIN and log[-1]["freeze"] >= physstep.RUN_MARGIN
    sp.surface_set_orography(cases[0].phis0)
    sp.physics_workspace()
    sp.use_own_stream()
    ncol = sp.il * sp.ix
    got, nodes, guard = _ensemble_days(sp, cases, c, events)
    singles = [coupledrun.device_run(sp, cases[e], c, refs[e][2]) for e in range(E)]
    worst = ("", 0.0)
    for e, name in enumerate(names):
        for n in coupledrun.CHECKPOINTS:
            err = coupledrun.errors(got[n][e], refs[e][0][n], ncol)
            worst = max([worst] + [("%s step %d %s" % (name, n, k), v) for k, v in err.items()], key=lambda x: x[1])
            one = singles[e][0][n]
            bad = [k for k in es.PROG + ("rad", "qcorh") if not support.same_bits(got[n][e][k], one[k])]
            bad += [k for k in er.SURF if not np.array_equal(got[n][e]["surf"][k], one["surf"][k], equal_nan=True)]
            assert bad == [], (name, n, bad)
    print("\n[coupled ensemble days vs the reference side] largest relative error %.1e (%s)" % (worst[1], worst[0]))
    print("[graph nodes] ensemble step %d, + check_dev %d, + couple_dev %d (shortwave %d, %d, %d); single-state step %d"
          % (nodes[False, "step"], nodes[False, False], nodes[False, True], nodes[True, "step"], nodes[True, False], nodes[True, True],
             singles[0][1][False, False]))
    assert worst[1] <= TOL, worst
    for sw in (True, False):
        assert nodes[sw, False] == nodes[sw, "step"] + 1 and nodes[sw, True] == nodes[sw, "step"] + 2, nodes
        assert nodes[sw, "step"] <= singles[0][1][sw, False], (nodes, singles[0][1])
    assert not support.same_bits(got[108][0]["qcorh"], got[108][1]["qcorh"])           # the members' corrections have parted
    assert guard["stopped"] == [-1] * E and guard["next_step"] == [coupledrun.NSTEPS + 1] * E, guard
    sp.close()


def test_t63_members_equal_single_objects():
    """T63 L16, E = 2.  couple_dev, the forcing's column kernel and check_dev have no transform in front of them: bit-equal to the
    single objects on the same inputs.  The members' qcorh is held to the single call's within 1e-13 of the field's maximum where
    the transform of two fields takes another launch form than that of one (the bound tests/test_gpu_fused_ops.py holds the T63
    forms to); which case occurred is printed."""
    s = support.package()
    E = 2
    sp = support.plan("t63k16", max_batch=4)
    clim, F = _surface_setup(sp, E, s)
    got, q, _, _ = _surface_run(sp, s, clim, F, E)
    assert not np.array_equal(got["sst_om"][0], got["sst_om"][1]) and np.isfinite(q.cpu().numpy()).all()
    for e in range(E):
        one, q1, _, _ = _surface_run(sp, s, clim, {k: v[e:e + 1].contiguous() for k, v in F.items()}, 1)
        for k in er.SURF + ("fmask_l",):
            assert np.array_equal(got[k][e], one[k][0], equal_nan=True), (e, k)
        if support.same_bits(q[e], q1[0]):
            print("[t63 forcing] member %d: qcorh bit-equal to the single call's" % e)
        else:
            err = es.relerr(q[e], q1[0])
            print("[t63 forcing] member %d: qcorh differs from the single call's by %.2e of its maximum" % (e, err))
            assert err <= 1e-13, (e, err)
    x = [dg.state(sp, 5400 + 100 * e) for e in range(E)]
    G = s.Diagnostics(sp, capacity=2, nmem=E)
    G.check_dev(*[support.dev(np.stack([m[k] for m in x])) for k in ("vor", "div", "t")])
    for e in range(E):
        d = s.Diagnostics(sp, capacity=2)
        d.check_dev(*[support.dev(x[e][k]) for k in ("vor", "div", "t")])
        assert np.array_equal(d.read(0, 1), G.read(0, 1, member=e)), e
        d.close()
    assert not np.array_equal(G.read(0, 1, member=0), G.read(0, 1, member=1))
    G.close()
    sp.close()
