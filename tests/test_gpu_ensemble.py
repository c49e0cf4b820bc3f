"""GPU: the ensemble time step (include/spdy.h "ensemble time step", speedy.f90_amd/ensemble.py).  E members with
DIFFERENT states go through one step's launches; every member must come out as the existing single-state step leaves that member's
state -- bit for bit at T30, where a field's bits do not depend on the batch it travels in -- and one member is anchored to the
oracle so that both sides of those equalities cannot be wrong together."""
import numpy as np
import pytest

import ensemblestep as es
import modelstep
import physstep
import support
import synth
from conftest import TOL
from dynstep import ROB, oracle_dynamics_step, wave_relerr

pytestmark = pytest.mark.gpu

DELT = 2400.0


@pytest.mark.parametrize("E,kx", [(3, 8), (2, 5), (2, 7), (17, 8), (2, 1), (3, 4), (2, 6), (2, 9), (3, 12), (2, 15)])
@pytest.mark.parametrize("seq", ["leapfrog", "startup"])
def test_member_equals_single_adiabatic(E, kx, seq):
    """T30: two consecutive leapfrog steps / the start-up pair; every member's prognostics, phi and its slices of U, V, PL bit-equal
    to the single-state step on that member's state.  kx = 5, 7: the FULL = false kernels; E = 17 pushes the transform launches
    out of the model-sized form.  kx = 1, 4, 6: the small blocks of the 8-bound kernels; 9, 12, 15: the 16-bound kernels' FULL =
    false forms, which nothing else runs with members (tests/levels.py)."""
    sp = es.plan_of_levels(kx, E)
    steps = es.LEAPFROG if seq == "leapfrog" else es.STARTUP
    sts = es.member_states(sp, E)
    snaps = es.run_ensemble(sp, es.build(sp, sts), steps, DELT)
    for e in range(E):
        assert es.differing(sp, snaps, e, sts[e], steps, DELT) == [], (E, kx, seq, e)
    sp.close()


# T63: (step, array) pairs that no transform lies in front of -- bit equality is required whatever form the launches take.  phi of
# the first step is the hydrostatic integration of the given t (time level 1) in the spectral step itself.  Every other compared
# array is downstream of the step's inverse and direct launches, whose form at T63 depends on the batch.
T63_NO_TRANSFORM_IN_FRONT = {(0, "phi")}


def test_t63_member_equals_single():
    """T63 L16, E = 2, two leapfrog steps.  Bit equality is asserted where the route to the array is the same by construction
    (T63_NO_TRANSFORM_IN_FRONT).  Elsewhere the route to the spectra may differ: E = 2 doubles every launch's batch, which moves the
    inverse launch across the derive-on-load threshold and the direct launch to another form, and at T63 a field's bits depend on
    the launch form (pairs are formed inside a segment, vds is applied in another place) while its value does not, to rounding.
    Those arrays are held to 1e-13 of the array's maximum, the bound tests/test_gpu_fused_ops.py holds the T63 launch forms to
    against each other; each one that is bit-equal all the same, and each difference, is printed."""
    E = 2
    sp = support.ensemble_plan("t63k16", E)
    sts = es.member_states(sp, E)
    snaps = es.run_ensemble(sp, es.build(sp, sts), es.LEAPFROG, 1200.0)
    worst, equal, must = 0.0, [], []
    for e in range(E):
        ref = es.run_single(sp, sts[e], es.LEAPFROG, 1200.0)
        for n, (got, want) in enumerate(zip(snaps, ref)):
            m = es.member_of(got, e)
            for k in es.COMPARED:
                if support.same_bits(m[k], want[k]):
                    equal.append((e, n, k))
                    continue
                err = es.relerr(m[k], want[k])
                print("[t63 ensemble] member %d step %d %s: relative difference %.2e" % (e, n + 1, k, err))
                worst = max(worst, err)
                if (n, k) in T63_NO_TRANSFORM_IN_FRONT:
                    must.append((e, n, k))
    print("[t63 ensemble] bit-equal (member, step, array): %s; worst difference of the others %.2e" % (sorted(equal), worst))
    assert must == [], must
    assert worst <= 1e-13, worst
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_one_member_equals_existing_entry_points(tag):
    """E = 1 through the new entry points: the existing entry points' bits (also the regression check on nmem = 1)"""
    sp = support.ensemble_plan(tag, 1)
    sts = es.member_states(sp, 1)
    for steps in (es.LEAPFROG, es.STARTUP):
        snaps = es.run_ensemble(sp, es.build(sp, sts), steps, 1200.0)
        assert es.differing(sp, snaps, 0, sts[0], steps, 1200.0) == [], tag
    sp.close()


def test_isolation():
    """Member 1 of 3 all NaN: members 0 and 2 come out as on their own, and the shared inputs are untouched"""
    import torch
    E = 3
    sp = support.ensemble_plan("t30", E)
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    for n in es.PROG:
        getattr(ens, n)[:, 1] = complex(float("nan"), float("nan"))
    shared = {n: getattr(ens, n).clone() for n in ("phis", "tcorh", "qcorh")}
    snaps = es.run_ensemble(sp, ens, es.LEAPFROG, DELT)
    for e in (0, 2):
        assert es.differing(sp, snaps, e, sts[e], es.LEAPFROG, DELT) == [], e
    assert torch.isnan(torch.view_as_real(snaps[-1]["vor"][:, 1])).all()
    for n, v in shared.items():
        assert support.same_bits(getattr(ens, n), v), n
    sp.close()


def test_member_zero_against_oracle(oracle_factory):
    """The absolute anchor: member 0 of the (3, 8) case against the oracle's call-by-call step, at the tolerance and in the norms of
    tests/test_gpu_step.py::test_dynamical_core_step_graph"""
    E = 3
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts = es.member_states(sp, E)
    o.tail_init(DELT)
    snaps = es.run_ensemble(sp, es.build(sp, sts), es.LEAPFROG[:1], DELT)
    new, out = oracle_dynamics_step(o, sts[0], 2, DELT, ROB)
    m = es.member_of(snaps[0], 0)
    for k in ("U", "V", "PL"):
        assert synth.relerr(m[k].cpu().numpy(), out[k]) <= TOL, k
    assert max(synth.relerr(m["phi"].cpu().numpy(), out["phi"]), wave_relerr(m["phi"].cpu().numpy(), out["phi"])) <= TOL
    for k in es.PROG:
        g = m[k].cpu().numpy()
        assert synth.relerr(g, new[k]) <= TOL and wave_relerr(g, new[k]) <= TOL, k
    sp.close()


# ---------------------------------------------------------------------------------------------- with the whole physics
def _single_physics_run(sp, st, bnd, dt, nsteps=3):
    """three single-state steps with spdy_physics_dev, shortwave on the first; the snapshots and the radiation state after each"""
    D, W = modelstep.device_state(st), modelstep.Workspace(sp)
    P = modelstep.physics_buffers(sp, bnd)
    out = []
    for n in range(nsteps):
        modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, n == 0))
        sp.synchronize()
        out.append(dict(es.single_snapshot(D, W), rad=P["rad"].clone()))
    return out


def test_full_physics(oracle_factory):
    """T30 L8, E = 3, three steps, shortwave on the first, per-member boundary fields and radiation states: every member bit-equal
    to spdy_physics_dev plus the single step on that member, radiation state included"""
    E, dt = 3, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds = es.physics_members(sp, o, E)
    sp.initialize_implicit(dt)
    ens, P = es.build(sp, sts), es.ens_physics(sp, bnds)
    snaps = []
    for n in range(3):
        ens.step(2, 2, dt, dict(P, sw=n == 0), eps=ROB)
        sp.synchronize()
        snaps.append(dict(es.snapshot(ens), rad=P["rad"].clone()))
    size = sp.radiation_state_size()
    assert np.isfinite(snaps[-1]["vor"][:, 0].cpu().numpy()).all()
    for e in range(E):
        ref = _single_physics_run(sp, sts[e], bnds[e], dt)
        for n in range(3):
            m = es.member_of(snaps[n], e)
            bad = [k for k in es.COMPARED if not support.same_bits(m[k], ref[n][k])]
            assert bad == [], (e, n, bad)
            assert support.same_bits(snaps[n]["rad"][e * size:(e + 1) * size], ref[n]["rad"]), (e, n, "radiation state")
    sp.close()


def test_graph(oracle_factory):
    """The ensemble step, adiabatic and with the physics, captured into one graph each: the replays give the eager calls' bits, and
    neither graph has more nodes than the single-state step captured by the same sequence"""
    import torch
    E, dt = 3, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds = es.physics_members(sp, o, E)
    sp.initialize_implicit(dt)
    sp.use_own_stream()
    for with_physics in (False, True):
        P = es.ens_physics(sp, bnds)
        phys = (lambda sw: dict(P, sw=sw)) if with_physics else (lambda sw: None)
        ens = es.build(sp, sts)
        eager = []
        for n in range(2):
            ens.step(2, 2, dt, phys(n == 0), eps=ROB)
            sp.synchronize()
            eager.append(dict(es.snapshot(ens), rad=P["rad"].clone()))
        # the same two steps as graph replays, from the same start
        ens2 = es.build(sp, sts)
        P["rad"].fill_(float("nan"))
        if with_physics:
            ens2.physics_workspace()
        torch.cuda.synchronize()
        graphs = {}
        for sw in ((True, False) if with_physics else (False,)):
            with sp.graph_capture() as g:
                ens2.step(2, 2, dt, phys(sw), eps=ROB)
            graphs[sw] = g
        for n in range(2):
            graphs[with_physics and n == 0].launch()
            sp.synchronize()
            got = dict(es.snapshot(ens2), rad=P["rad"])
            bad = [k for k in got if not support.same_bits(got[k], eager[n][k])]
            assert bad == [], (with_physics, n, bad)
        # the single-state step, captured by the same sequence of calls
        D, W, P1 = modelstep.device_state(sts[0]), modelstep.Workspace(sp), modelstep.physics_buffers(sp, bnds[0])
        sp.physics_workspace()
        torch.cuda.synchronize()
        with sp.graph_capture() as g1:
            modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P1, False) if with_physics else None)
        n_ens, n_one = graphs[False].num_nodes(), g1.num_nodes()
        print("[graph nodes, physics=%s] ensemble of %d: %d, single state: %d" % (with_physics, E, n_ens, n_one))
        assert n_ens <= n_one, (with_physics, n_ens, n_one)
        for g in list(graphs.values()) + [g1]:
            g.close()
    sp.close()


def test_per_member_guard_and_coupling(oracle_factory):
    """One Diagnostics object and one surface model per member, called on views of an E = 2 ensemble after each of two steps with
    the physics: check_dev on member(e)'s time level 1, couple_dev on member e's slices of the physics' optional outputs (hfluxn,
    shf, evap, ssrd, E states back to back).  They give, bit for bit, the rows and the fields that a second object of each kind
    gives on the single-state run of that member.  Both calls read contiguous slices of one member: no batched form is needed."""
    import longrun
    import surfmodel as sm
    import speedy_f90_amd as s
    E, dt = 2, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds = es.physics_members(sp, o, E)
    sp.initialize_implicit(dt)
    phis0 = o.spec_to_grid(sts[0]["phis"], 1)
    c = sm.climatology(phis0, longrun.latitudes(sp.table("sia_half")))
    clim = {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + sp.grid_shape) for k, v in c.items()}
    date = sm.Date(1982, 1, 15)
    flux_names = ("hfluxn", "shf", "evap", "ssrd")

    def objects():
        d, m = s.Diagnostics(sp, capacity=4, first_step=0), s.SurfaceModel(sp, clim, sm.DELT)
        m.set_date(date.imont1, date.tmonth, date.tyear)
        m.couple_dev(0)
        return d, m

    def flat(out):
        return dict(out["sfc"], **out["rad"])

    # the ensemble: one pair of objects per member, on the member's views
    ens, P = es.build(sp, sts), es.ens_physics(sp, bnds)
    P["out"] = sp.column_outputs(E, ("sfc", "rad"), names=flux_names)
    F = flat(P["out"])
    assert F["hfluxn"].shape == (E, 2) + sp.grid_shape and F["ssrd"].shape == (E,) + sp.grid_shape
    objs = [objects() for _ in range(E)]
    for n in range(2):
        ens.step(2, 2, dt, dict(P, sw=n == 0), eps=ROB)
        for e, (d, m) in enumerate(objs):
            D = ens.member(e)
            assert D["vor"][0].is_contiguous() and D["vor"].shape == (2, sp.kx, sp.nx, sp.mx)
            d.check_dev(D["vor"][0], D["div"][0], D["t"][0])
            m.couple_dev(1, *[F[k][e] for k in flux_names])
        sp.synchronize()
    got = [(np.array(d.read(0, 2)), {k: m.field(k).numpy().copy() for k in sm.FIELDS}) for d, m in objs]
    for d, m in objs:
        d.close(); m.close()
    # the single runs
    for e in range(E):
        d, m = objects()
        D, W, P1 = modelstep.device_state(sts[e]), modelstep.Workspace(sp), modelstep.physics_buffers(sp, bnds[e])
        out = sp.column_outputs(1, ("sfc", "rad"), names=flux_names)
        F1 = flat(out)
        for n in range(2):
            modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P1, n == 0, out))
            d.check_dev(D["vor"][0], D["div"][0], D["t"][0])
            m.couple_dev(1, *[F1[k][0] for k in flux_names])
            sp.synchronize()
        rows, fields = np.array(d.read(0, 2)), {k: m.field(k).numpy().copy() for k in sm.FIELDS}
        assert np.array_equal(got[e][0], rows, equal_nan=True), e
        for k in sm.FIELDS:
            assert np.array_equal(got[e][1][k], fields[k], equal_nan=True), (e, k)
        if e == 0:
            assert np.isfinite(rows).all() and all(np.isfinite(v).all() for v in fields.values())
        d.close(); m.close()
    # the test notices what it is for: the members' rows differ, and coupling changed the models
    assert not np.array_equal(got[0][0], got[1][0])
    assert any(not np.array_equal(got[0][1][k], got[1][1][k]) for k in sm.FIELDS)
    sp.close()


def test_single_state_and_ensemble_interleaved_on_one_plan(oracle_factory):
    """T30 L8: a single state (modelstep.step with spdy_physics_dev) and an ensemble of E = 2 (Ensemble.step, physics on) take turns on
    ONE plan for three steps, shortwave on the first only, no ssrd supplied through `out` on either side: step n of the single state,
    step n of the ensemble, step n + 1 of the single state, ...  The single state's prognostics and PL after every step, and every
    member after every step, are bit-equal to the same steps run alone on a fresh plan.  The physics from spectra of the two forms
    is one body, but each form keeps a workspace of its own, and the held ssrd lives there between shortwave steps: a shared
    workspace would hand the one run the other's ssrd on steps 2 and 3.  All three states differ."""
    import radiation
    E, dt = 2, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds = es.physics_members(sp, o, E + 1)               # members 0, 1; the single state is the third
    phis0 = o.spec_to_grid(sts[0]["phis"], 1)

    def run(sp, single, ensemble):
        sp.initialize_implicit(dt)
        D, W, P1 = modelstep.device_state(sts[E]), modelstep.Workspace(sp), modelstep.physics_buffers(sp, bnds[E])
        ens, P = es.build(sp, sts[:E]), es.ens_physics(sp, bnds[:E])
        one, many = [], []
        for n in range(3):
            if single:
                modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P1, n == 0))
                sp.synchronize()
                one.append(modelstep.snapshot(D, W, P1))
            if ensemble:
                ens.step(2, 2, dt, dict(P, sw=n == 0), eps=ROB)
                sp.synchronize()
                many.append(dict(es.snapshot(ens), rad=P["rad"].clone()))
        return one, many

    one, many = run(sp, True, True)
    sp.close()
    alone = {}
    for which in ("single", "ensemble"):
        sp = support.ensemble_plan("t30", E)
        sp.radiation_set_date(radiation.DATES[0])
        sp.surface_set_orography(phis0)
        alone[which] = run(sp, which == "single", which == "ensemble")[which == "ensemble"]
        sp.close()
    assert np.isfinite(one[-1]["vor"].cpu().numpy()).all() and np.isfinite(many[-1]["vor"].cpu().numpy()).all()
    for n in range(3):
        bad = [k for k in one[n] if not support.same_bits(one[n][k], alone["single"][n][k])]
        assert bad == [], ("single state", n, bad)
        for e in range(E):
            got, want = es.member_of(many[n], e), es.member_of(alone["ensemble"][n], e)
            bad = [k for k in es.COMPARED if not support.same_bits(got[k], want[k])]
            assert bad == [], ("member", e, n, bad)
        assert support.same_bits(many[n]["rad"], alone["ensemble"][n]["rad"]), ("radiation states", n)
