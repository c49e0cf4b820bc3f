"""What the coupled-ensemble tests share (tests/test_ensemble_run_cpu.py, tests/test_gpu_ensemble_run.py): the layout rule of a
surface model of nmem members restated, the climatology of a plan, and the two sides of "a member equals its single objects" --
the coupled ensemble sequence with ONE surface model and ONE guard of nmem members, and the same sequence on one member's state
through the single-state step (modelstep.step), a single SurfaceModel and a single Diagnostics."""
import numpy as np

import longrun
import support
import surfmodel as sm

FLUXES = ("hfluxn", "shf", "evap", "ssrd")
SHARED_FIELDS = ("fmask_s", "alb0", "rhcapl", "cdland", "rhcaps", "rhcapi", "cdsea", "cdice")
FIELD_ORDER = ("fmask_l",) + SHARED_FIELDS + sm.FIELDS + sm.FORCING        # the names of spdy_surface_model_field, in array order
PER_MEMBER = ("fmask_l",) + sm.FIELDS + sm.FORCING
SURF = sm.FIELDS + sm.FORCING
NCLIM = 5 * 12 + 3


def surf_slot(name, nmem, e):
    """The place of (field, member) in a surface model's array in units of one grid, as include/spdy.h words it: fmask_l of the nmem
    members; the eight fields held once; every field a kernel writes as a stack of nmem grids; the climatologies ("clim<i>")."""
    n1 = len(SHARED_FIELDS)
    if name == "fmask_l":
        return e
    if name in SHARED_FIELDS:
        return nmem + SHARED_FIELDS.index(name)
    if name in SURF:
        return nmem + n1 + SURF.index(name) * nmem + e
    return nmem + n1 + len(SURF) * nmem + int(name[4:])


def shaped(c, shape):
    return {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + tuple(shape)) for k, v in c.items()}


def host_climatology(sp, ex=None):
    """surfmodel's seeded climatology over its seeded orography, as SurfaceModel takes it.  ex: who transforms the orography (the
    oracle where sp is a host-only plan, which does not transform)"""
    return shaped(sm.climatology(sm.orography(ex or sp), longrun.latitudes(sp.table("sia_half"))), sp.grid_shape)


# ---------------------------------------------------------------------------------------------- the two sides on the device
DATE = (1982, 1, 15)
SEQUENCE = (("forcing", None), ("step", True), ("step", False), ("forcing", None), ("step", False))   # after couple(0); (what, shortwave)
OVERRIDES = (("sst", "sst_am"), ("stl", "stl_am"), ("stl", "stl_lm"), ("soilw", "soilw_am"))   # drawn boundary field -> model field


def _flat(out):
    return dict(out["sfc"], **out["rad"])


def _start(M, bnds, nmem):
    """the date, couple(0), then each member's own drawn sea and land temperatures and soil water in place of the climatology's:
    members that differ from the first forcing on"""
    date = sm.Date(*DATE)
    M.set_date(date.imont1, date.tmonth, date.tyear)
    M.couple_dev(0)
    for src, dst in OVERRIDES:
        a = np.stack([np.asarray(b[src], np.float64).reshape(M.sp.grid_shape) for b in bnds])
        M.field(dst).upload(a if nmem > 1 else a[0])


def run_ensemble(sp, s, es, sts, bnds, clim, dt, rob, capacity=4, same_qcorh=False, graph=False):
    """The coupled sequence on an ensemble of len(sts) members with a humidity correction per member: one SurfaceModel and one
    Diagnostics of nmem members.  same_qcorh: after every forcing member 0's qcorh is copied into every member's slot (what a
    shared qcorh would be).  graph: {step, check_dev, couple_dev} is captured once per shortwave setting and launched instead of
    issued eagerly.
    Returns the list of snapshots after each entry of SEQUENCE, the guard's rows [E, steps, 3, kx] and the graphs' node counts."""
    import torch
    E = len(sts)
    ens = s.Ensemble(sp, E, member_qcorh=True)
    ens.set_shared(sts[0])
    for e, st in enumerate(sts):
        ens.set_member(e, st)
    M, G = s.SurfaceModel(sp, clim, sm.DELT, nmem=E), s.Diagnostics(sp, capacity=capacity, first_step=0, nmem=E)
    bnd, albsfc = M.boundary()
    out = sp.column_outputs(E, ("sfc", "rad"), names=FLUXES)
    F = _flat(out)
    P = {"bnd": bnd, "albsfc": albsfc, "out": out,
         "rad": torch.full((E * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")}
    _start(M, bnds, E)
    ens.physics_workspace()
    torch.cuda.synchronize()

    def one(sw):
        ens.step(2, 2, dt, dict(P, sw=sw), eps=rob)
        G.check_dev(ens.vor[1], ens.div[1], ens.t[1])
        M.couple_dev(1, *[F[k] for k in FLUXES])
    snaps, nodes, graphs = [], [], {}
    for what, sw in SEQUENCE:
        if what == "forcing":
            M.forcing_dev(ens.qcorh)
            if same_qcorh:
                ens.qcorh.copy_(ens.qcorh[0].clone().expand_as(ens.qcorh))
        elif graph:                                       # one graph per shortwave setting, replayed where it comes again
            if sw not in graphs:
                with sp.graph_capture() as g:
                    one(sw)
                graphs[sw] = g
                nodes.append(g.num_nodes())
            graphs[sw].launch()
        else:
            one(sw)
        sp.synchronize()
        snap = es.snapshot(ens)
        snap.update(rad=P["rad"].clone(), qcorh=ens.qcorh.clone(), surf={k: M.field(k).numpy() for k in SURF},
                    shared={k: M.field(k).numpy() for k in SHARED_FIELDS}, next_step=[G.status(e)["next_step"] for e in range(E)])
        snaps.append(snap)
    nsteps = sum(1 for what, _ in SEQUENCE if what == "step")
    rows = np.stack([G.read(0, nsteps, member=e) for e in range(E)])
    for g in graphs.values():
        g.close()
    M.close(); G.close()
    return snaps, rows, nodes


def run_single(sp, s, es, modelstep, st, bnd1, clim, dt, rob, capacity=4, graph=False):
    """the same sequence on one state: modelstep.step, a single SurfaceModel, a single Diagnostics"""
    import torch
    D, W = modelstep.device_state(st), modelstep.Workspace(sp)
    M, G = s.SurfaceModel(sp, clim, sm.DELT), s.Diagnostics(sp, capacity=capacity, first_step=0)
    bnd, albsfc = M.boundary()
    out = sp.column_outputs(1, ("sfc", "rad"), names=FLUXES)
    F = _flat(out)
    P = {"bnd": dict(bnd, albsfc=albsfc), "rad": modelstep.radiation_state(sp)}
    _start(M, [bnd1], 1)
    sp.physics_workspace()
    torch.cuda.synchronize()

    def one(sw):
        modelstep.step(sp, D, W, dt, 2, 2, rob, physics=modelstep.whole_physics(P, sw, out))
        G.check_dev(D["vor"][1], D["div"][1], D["t"][1])
        M.couple_dev(1, *[F[k] for k in FLUXES])
    snaps, nodes, graphs = [], [], {}
    for what, sw in SEQUENCE:
        if what == "forcing":
            M.forcing_dev(D["qcorh"])
        elif graph:                                       # one graph per shortwave setting, replayed where it comes again
            if sw not in graphs:
                with sp.graph_capture() as g:
                    one(sw)
                graphs[sw] = g
                nodes.append(g.num_nodes())
            graphs[sw].launch()
        else:
            one(sw)
        sp.synchronize()
        snap = es.single_snapshot(D, W)
        snap.update(rad=P["rad"].clone(), qcorh=D["qcorh"].clone(), surf={k: M.field(k).numpy() for k in SURF})
        snaps.append(snap)
    nsteps = sum(1 for what, _ in SEQUENCE if what == "step")
    rows = G.read(0, nsteps)
    for g in graphs.values():
        g.close()
    M.close(); G.close()
    return snaps, rows, nodes


def member_differences(es, snaps, rows, e, ref_snaps, ref_rows, size):
    """[(entry of SEQUENCE, what)] where member e of the ensemble run is not bit-equal to the single run"""
    bad = []
    for n, (got, want) in enumerate(zip(snaps, ref_snaps)):
        m = es.member_of(got, e)
        bad += [(n, k) for k in es.COMPARED if not support.same_bits(m[k], want[k])]
        if not support.same_bits(got["rad"][e * size:(e + 1) * size], want["rad"]):
            bad.append((n, "rad"))
        if not support.same_bits(got["qcorh"][e], want["qcorh"]):
            bad.append((n, "qcorh"))
        E = got["qcorh"].shape[0]
        for k in SURF:
            x = got["surf"][k][e] if E > 1 else got["surf"][k]
            if not np.array_equal(x, want["surf"][k], equal_nan=True):
                bad.append((n, k))
    if not np.array_equal(rows[e], ref_rows, equal_nan=True):
        bad.append(("rows", "guard"))
    return bad
