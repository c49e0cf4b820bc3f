#!/usr/bin/env python3
"""What an ensemble member costs: graph replays of the E-member step (speedy.f90_amd/ensemble.py) against the single-state
captured step of tests/modelstep.py, adiabatic and with the whole physics, T30 L8 and T63 L16.

Per size and E it prints one JSON row: microseconds per step (median of --repeats timings of --reps replays, with the range),
microseconds per member-step, the speed-up per member over E single-state steps measured in the same process, and the launches'
byte model (below) as a fraction of 8 TB/s.  Timing as tools/physics_step_rate.py: HIP events around the replays, 10 warm-up
replays, the forms interleaved repeat by repeat; every repeat starts from the same state.

The comparison with an earlier build: --single-only times the single-state step alone and works with a library that has no
ensemble entry points; select it with $SPDY_LIB.  Run that and this build's --single-only alternately, twice each: the difference
between two runs of the same build is the run-to-run spread a difference between the builds has to exceed.

--coupled measures a RUN's step instead: graph replays of {the step with the physics, check_dev on time level 2, couple_dev(1)}.
The batched form is one SurfaceModel and one Diagnostics of E members (two launches behind the step, whatever E, and a humidity
correction per member); the per-member form is E single objects on the members' views, 2 E launches, which is all a library from
before the batched objects can do.  --earlier-library binds such a library ($SPDY_LIB): what it lacks is left out, the member
forms of one member are its unsuffixed calls, and only the per-member form (and, without --coupled, what it has) is measured.

--output measures the ensemble OUTPUT instead (include/spdy.h, "ensemble output"): graph replays of Ensemble.output with members and
statistics -- one inverse batch of all members and one epilogue kernel, whatever E -- against E replays' worth of the single-state
spdy_output_batch_dev on the members' views in one graph (3 E launches: the only way to the same member fields without the call,
and it gives no statistics), and the call's inverse batch captured alone.  The epilogue's time is taken as the difference of the
first and the last -- a difference of two graph replays, not a kernel trace -- and its byte model ((5 kx + 1) E FP64 grids read
once, (E + 2) (5 kx + 1) float32 grids written) is given as a fraction of 8 TB/s, as is the whole call's.

--sppt measures SPPT for an ensemble instead (include/spdy.h, "SPPT"; at T30 L8, E = 1, 4 and 16 and 100 replays per timing unless
told otherwise), both sides of each comparison in the same run: (a) the captured advance of one pattern object of E members --
three launches whatever E -- against E captured advances of single objects replayed back to back; (b) the captured ensemble step
with the whole physics and SPPT (Ensemble.step with physics["sppt"]) against the same step without SPPT and against E single-state
captured steps with SPPT (tests/modelstep.py's sppt_physics), each on a state, a workspace and a pattern object of its own.

--letkf measures the ensemble ANALYSIS instead (include/spdy.h, "ensemble analysis"; T30 L8, E = 4, 16 and 32, 100 replays per timing
unless told otherwise): graph replays of Ensemble.analyse -- five launches, six where the direct batch streams (here from E = 16 on) -- with a network of 416 columns (26 x 16) that
observes u, v, t, q at every level and ps, 13 728 observations, sigma_h = 500 km, sigma_v = 0.1, rho = 1.1; each observation has the
members' spread at its place as error and a value one such error around their mean.  Next to it the captured ensemble step with
the whole physics, whose 36 replays are the model side of one six-hour cycle.  Every repeat starts from the same state; inside a
repeat the replays analyse the state the replay before left.  --stride SI SJ sets the analysis' weight stride (one launch more:
the local problems on the coarse columns, then the kernel that interpolates their transforms to every column); the row then has
the number of coarse columns and the byte count of that kernel's reads -- per grid column and level one E x E transform per
stencil entry of non-zero weight, and the members' values -- to set against its time from a kernel trace.  --at-pressure adds the
analysis of the same stations with u, v, t and q given at the pressures p0 fsg[k] instead of on the levels k (include/spdy.h,
"observations at a pressure"): the observation kernel that interpolates per member in the plain one's place, the
same launch count; the row has the number of observations that are in column on the starting state.  --mask K [K ...] adds, for
every K, the analysis under a member mask that drops the last K members (K = half: E / 2; K = 0: the masked call with every member
in use, the price of the indirection alone; include/spdy.h, "member mask"): one launch more, and the local problems
of E - K members in the launch shape of E.  Set them against the plain analysis of E - K members: --members 31 15 3 16 8 2.
--relax RTPP RTPS adds the analysis of the same network by an object with relaxation on (include/spdy.h, "relaxation"; DESIGN.md
s24), next to the one with relaxation off in the same run: one launch more; the row has the difference of the two medians, the
relaxation kernel's bytes -- the ensemble and the raw increments read, the relaxed increments and the factors written -- and
their time at 8 TB/s.  Replays of Ensemble.analyse analyse the state the replay before left, which a relaxed ensemble changes, so
that pair of rows compares two different workloads; the pair "grid analysis" / "grid analysis relaxed" replays Letkf.analyse_grid
of both objects on one gridded ensemble, the start state's, and its difference is the relaxation's own cost.
--slots S divides the network into S equal time slots (include/spdy.h, "observations in time slots") and adds the
captured Ensemble.observe of the middle slot -- the inverse batch and the slot's one launch -- and the captured slot analysis,
Ensemble.analyse(slots=True), next to the plain analysis of the same object.  Replays of Ensemble.analyse analyse the state the
replay before left while the slots keep the start state's hx, so that pair compares two different workloads; the pair "grid analysis
plain" / "grid analysis slots" replays Letkf.analyse_grid of the object on one gridded ensemble, the start state's, with every slot
observed on it -- the same bits and so the same work -- and its difference is the finish kernel against the observation kernel it
replaces.  With --at-pressure the same rows for the at-pressure object.

--qc [GROSS] adds the analysis of the same network by an object with the background check on (include/spdy.h, "background check and
observation statistics"; default threshold 5): one launch more.  As with --relax, the pair "grid analysis" / "grid
analysis checked" replays Letkf.analyse_grid of both objects on one gridded ensemble and its difference is the check's cost less the
work the rejected observations take out of the transform; "checked none rejected" is the same launch at a threshold nothing
exceeds, its difference the check's launch alone.

--adaptive adds the analysis of the same network by an object with adaptive inflation on (include/spdy.h, "adaptive inflation";
DESIGN.md s28): two launches more, last.  As with --relax, the pair "grid analysis" / "grid analysis adaptive" on one gridded ensemble
is the one whose difference is the feature's own cost.
--osse measures what a twin experiment adds to that cycle (include/spdy.h, "nature run"), in the --letkf set-up and next
to its two graphs: (a) the captured {Nature.set_state, Nature.observe} -- the truth to the grid and the 13 728 values drawn from it,
three launches; (b) the captured Ensemble.verify -- the inverse batch of all members and the two score launches; (c) the host route
to the same values that a build without the nature run offers, wall-clock with its synchronisations: the single-state output call,
the download of its float32 grids, the operator and the noise in vectorised NumPy on the stencils the Letkf already holds, and
Letkf.set_obs (median of --repeats calls after one warm-up).  The rows of (a) and (b) give their share of the cycle {36 steps,
analysis}; the row of (c) its ratio to (a).

--pressure measures the pressure-level output instead (include/spdy.h, "pressure-level output"; T30 L8, the reference
script's eight levels, E = 4, 16 and 32, 100 replays per timing unless told otherwise): graph replays of Ensemble.output_pressure with
members, statistics and `below`, in both coordinates, next to (a) Ensemble.output on the same build, and (b) the route a build without
the call offers to the same fields -- Ensemble.output, the download of its float32 members, np.interp's rule vectorised over the
columns in NumPy, and mean and spread on the host -- wall-clock with its synchronisation (median of --repeats calls after one
warm-up).  The kernel's byte model: per level (5 * 2 + 1) E FP64 grids read in the first pass and again in the second, (E + 2) 5 + 1
float32 grids written; and the surface-pressure row.

    python tools/ensemble_rate.py [--sizes t30 t63k16] [--members 1 2 4 8 16 32] [--reps 200] [--repeats 5] [--json out.json]
    SPDY_LIB=/path/to/earlier/libspdy.so python tools/ensemble_rate.py --single-only --label parent
    python tools/ensemble_rate.py --coupled --members 1 2 4 8 16
    python tools/ensemble_rate.py --output --json profiles/ensemble_output_rate.json
    python tools/ensemble_rate.py --sppt --json profiles/ensemble_sppt_rate.json
    python tools/ensemble_rate.py --letkf --json profiles/ensemble_letkf_rate.json
    python tools/ensemble_rate.py --letkf --stride 2 2
    python tools/ensemble_rate.py --letkf --at-pressure --members 4 32 --json profiles/ensemble_letkf_pobs_rate.json
    python tools/ensemble_rate.py --letkf --mask 0 1 half
    python tools/ensemble_rate.py --letkf --slots 6 --at-pressure --json profiles/ensemble_letkf_slots_rate.json
    python tools/ensemble_rate.py --letkf --relax 0 0.9 --json profiles/ensemble_letkf_relax_rate.json
    python tools/ensemble_rate.py --letkf --qc --json profiles/ensemble_letkf_qc_rate.json
    python tools/ensemble_rate.py --letkf --adaptive --json profiles/ensemble_letkf_infl_rate.json
    SPDY_LIB=/path/to/earlier/libspdy.so python tools/ensemble_rate.py --letkf --earlier-library --label parent
    python tools/ensemble_rate.py --osse --json profiles/ensemble_osse_rate.json
    python tools/ensemble_rate.py --pressure --json profiles/ensemble_pressure_rate.json
    SPDY_LIB=/path/to/earlier/libspdy.so python tools/ensemble_rate.py --coupled --earlier-library --label parent"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import modelstep  # noqa: E402
import physstep  # noqa: E402
import support  # noqa: E402
import synth  # noqa: E402
import speedy_f90_amd as s  # noqa: E402
from conftest import VARIANTS  # noqa: E402

HBM = 8.0e12


def byte_model(sp, physics):
    """bytes one member's step moves through HBM if every launch reads its inputs and writes its outputs once: the inverse batch
    (6 kx + 1 spectra in, 6 kx + 2 grids out), the grid tendencies (6 kx + 2 grids in, 9 kx + 1 out), the direct batch (9 kx + 1
    grids in, as many spectra out), the spectral step (those spectra and both time levels of the prognostics in; the prognostics,
    the tendencies and phi out); with physics the geopotential, its inverse launch (5 kx + 1 fields) and the chain (those grids,
    the four tendencies in and out, 9 boundary fields, the radiation state of 6 kx + 7 fields in and out)"""
    kx, spec, grid = sp.kx, sp.nx * sp.mx * 16, sp.il * sp.ix * 8
    prog = 2 * (4 * kx + 1)
    b = (6 * kx + 1) * spec + 2 * (6 * kx + 2) * grid + 2 * (9 * kx + 1) * grid + 2 * (9 * kx + 1) * spec
    b += (prog + 3) * spec + (prog + 4 * kx + 1 + kx) * spec
    if physics:
        b += 2 * kx * spec + (5 * kx + 1) * (spec + 2 * grid) + (8 * kx + 9 + 2 * (6 * kx + 7)) * grid
    return b


def time_interleaved(fns, rearm, reps, repeats):
    for fn in fns.values():
        for _ in range(10):
            fn()
    us = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            rearm()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[n].append(a.elapsed_time(b) * 1e3 / reps)
    return {n: (float(np.median(v)), min(v), max(v)) for n, v in us.items()}


def run(tag, members, reps, repeats, label, rows):
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    emax = max(members) if members else 1
    sp = support.plan(tag, emax * (4 * kx + 4))
    case = physstep.Case(tag, sp, o)
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    sp.physics_workspace()
    # the single-state step
    W, P, D0 = modelstep.Workspace(sp), modelstep.physics_buffers(sp, case.bnd, 0.0), modelstep.device_state(case.st)
    D = {n: D0[n].clone() for n in D0}
    modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, True))     # a shortwave step first: the radiation state is whole
    sp.synchronize()
    rad0 = P["rad"].clone()
    graphs, rearms = {}, []
    for name, phys in (("single adiabatic", False), ("single physics", True)):
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, False) if phys else None)
        graphs[name] = g

    def rearm_single():
        for n in D:
            D[n].copy_(D0[n])
        P["rad"].copy_(rad0)
    rearms.append(rearm_single)
    ens = {}
    for E in members:
        en = s.Ensemble(sp, E)
        en.set_shared(case.st)
        for e in range(E):
            en.set_member(e, case.st)
        dev = physstep.device_boundary(case.bnd, sp.il, sp.ix)
        bnd = {n: v.expand((E,) + tuple(v.shape[1:])).contiguous() for n, v in dev.items()}
        PE = {"bnd": bnd, "albsfc": bnd["albsfc"], "rad": rad0.repeat(E), "sw": False}
        en.physics_workspace()
        start = {n: getattr(en, n).clone() for n in ("vor", "div", "t", "tr", "ps")}
        for name, phys in (("E=%d adiabatic" % E, None), ("E=%d physics" % E, PE)):
            torch.cuda.synchronize()
            with sp.graph_capture() as g:
                en.step(2, 2, dt, phys, eps=modelstep.ROB)
            graphs[name] = g

        def rearm(en=en, start=start, PE=PE, E=E):
            for n, v in start.items():
                getattr(en, n).copy_(v)
            PE["rad"].copy_(rad0.repeat(E))
        rearms.append(rearm)
        ens[E] = en
    nodes = {n: g.num_nodes() for n, g in graphs.items()}
    t = time_interleaved({n: g.launch for n, g in graphs.items()}, lambda: [r() for r in rearms], reps, repeats)
    for name, (med, lo, hi) in t.items():
        phys = name.endswith("physics")
        E = 1 if name.startswith("single") else int(name.split()[0][2:])
        one = t["single physics" if phys else "single adiabatic"][0]
        row = {"label": label, "size": tag, "form": name, "members": E, "nodes": nodes[name], "us_per_step": round(med, 2),
               "us_min": round(lo, 2), "us_max": round(hi, 2), "us_per_member_step": round(med / E, 2),
               "speedup_per_member_vs_single": round(one / (med / E), 2),
               "byte_model_fraction_of_8TBps": round(E * byte_model(sp, phys) / (med * 1e-6) / HBM, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for g in graphs.values():
        g.close()
    sp.close()


def earlier_library():
    """Bind a library from before this build's newest entry points: drop what it lacks from the table; one member's member forms
    are its unsuffixed calls; the option it does not know describes the layout it always has."""
    from speedy_f90_amd import _lib
    from speedy_f90_amd import spectral
    raw = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in _lib.SIGNATURES if not hasattr(raw, n)]
    for n in missing:
        del _lib.SIGNATURES[n]
    lib = _lib.load()
    shims = {"spdy_ens_surface_model_create": lambda h, nmem, *a: lib.spdy_surface_model_create(h, *a),
             "spdy_ens_diagnostics_create": lambda h, nmem, *a: lib.spdy_diagnostics_create(h, *a),
             "spdy_ens_diagnostics_status": lambda d, member, *a: lib.spdy_diagnostics_status(d, *a),
             "spdy_ens_diagnostics_read": lambda d, member, *a: lib.spdy_diagnostics_read(d, *a),
             "spdy_surface_model_members": lambda m, name: 1}
    for n in missing:
        if n in shims:
            setattr(lib, n, shims[n])
    if "spdy_ens_surface_model_create" in missing:
        plain = spectral.Spectral.set_option
        spectral.Spectral.set_option = lambda self, name, value: None if name == "ens_member_qcorh" and not value else plain(self, name, value)
    return missing


def run_coupled(tag, members, reps, repeats, label, rows, batched):
    """graph replays of {step with physics, check_dev, couple_dev(1)}: per-member objects, and (batched) one object for all"""
    import longrun
    import surfmodel as sm
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    sp = support.plan(tag, max(members) * (4 * kx + 4))
    case = physstep.Case(tag, sp, o)
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    c = sm.climatology(case.phis0, longrun.latitudes(sp.table("sia_half")))
    clim = {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + sp.grid_shape) for k, v in c.items()}
    date = sm.Date(1982, 1, 15)
    names = ("hfluxn", "shf", "evap", "ssrd")
    P1 = modelstep.physics_buffers(sp, case.bnd, 0.0)
    D1 = modelstep.device_state(case.st)
    sp.physics_workspace()
    modelstep.step(sp, D1, modelstep.Workspace(sp), dt, physics=modelstep.whole_physics(P1, True))   # a whole radiation state
    sp.synchronize()
    rad0 = P1["rad"].clone()
    dev = physstep.device_boundary(case.bnd, sp.il, sp.ix)

    def model(nmem):
        M = s.SurfaceModel(sp, clim, sm.DELT, nmem=nmem) if nmem > 1 else s.SurfaceModel(sp, clim, sm.DELT)
        M.set_date(date.imont1, date.tmonth, date.tyear)
        M.couple_dev(0)
        return M
    graphs, rearms, keep = {}, [], []
    for E in members:
        for form in ("per-member",) + (("batched",) if batched else ()):
            en = s.Ensemble(sp, E, member_qcorh=True) if form == "batched" else s.Ensemble(sp, E)
            en.set_shared(case.st)
            for e in range(E):
                en.set_member(e, case.st)
            out = sp.column_outputs(E, ("sfc", "rad"), names=names)
            F = dict(out["sfc"], **out["rad"])
            if form == "batched":
                M, G = model(E), (s.Diagnostics(sp, 64, 0, E) if E > 1 else s.Diagnostics(sp, 64, 0))
                M.forcing_dev(en.qcorh)
                bnd, albsfc = M.boundary()
                keep.append((M, G))
            else:
                Ms, Gs = [model(1) for _ in range(E)], [s.Diagnostics(sp, 64, 0) for _ in range(E)]
                b = {n: v.expand((E,) + tuple(v.shape[1:])).contiguous() for n, v in dev.items()}
                bnd, albsfc = b, b["albsfc"]
                keep.append((Ms, Gs))
            PE = {"bnd": bnd, "albsfc": albsfc, "rad": rad0.repeat(E), "sw": False, "out": out}
            en.physics_workspace()
            start = {n: getattr(en, n).clone() for n in ("vor", "div", "t", "tr", "ps")}
            torch.cuda.synchronize()
            with sp.graph_capture() as g:
                en.step(2, 2, dt, PE, eps=modelstep.ROB)
                if form == "batched":
                    G.check_dev(en.vor[1], en.div[1], en.t[1])
                    M.couple_dev(1, *[F[k] for k in names])
                else:
                    for e in range(E):
                        Gs[e].check_dev(en.vor[1, e], en.div[1, e], en.t[1, e])
                    for e in range(E):
                        Ms[e].couple_dev(1, *[F[k][e] for k in names])
            graphs["coupled %s E=%d" % (form, E)] = g
            keep.append((en, PE, out))

            def rearm(en=en, start=start, PE=PE, E=E):
                for n, v in start.items():
                    getattr(en, n).copy_(v)
                PE["rad"].copy_(rad0.repeat(E))
            rearms.append(rearm)
    nodes = {n: g.num_nodes() for n, g in graphs.items()}
    t = time_interleaved({n: g.launch for n, g in graphs.items()}, lambda: [r() for r in rearms], reps, repeats)
    for name, (med, lo, hi) in t.items():
        E = int(name.split("=")[1])
        row = {"label": label, "size": tag, "form": name, "members": E, "nodes": nodes[name], "us_per_step": round(med, 2),
               "us_min": round(lo, 2), "us_max": round(hi, 2), "us_per_member_step": round(med / E, 2)}
        per = t.get("coupled per-member E=%d" % E)
        if "batched" in name and per:
            row["us_saved_vs_per_member"] = round(per[0] - med, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for g in graphs.values():
        g.close()
    sp.close()


def run_output(tag, members, reps, repeats, label, rows):
    """graph replays of the ensemble output call, of E single-state output calls, and of the call's inverse batch alone"""
    import ensemblestep
    kx = VARIANTS[tag][3]
    sp = support.plan(tag, max(members) * (4 * kx + 4))
    spec, grid = sp.nx * sp.mx * 16, sp.il * sp.ix
    graphs, keep = {}, []
    for E in members:
        en = ensemblestep.build(sp, ensemblestep.member_states(sp, E))
        sp.ens_geopotential_dev(E, en.t[0], en.phis, en.phi)                 # phi of time level 1: an input of the snapshot
        zeros = lambda shapes: {n: torch.zeros(sh, dtype=torch.float32, device="cuda") for n, sh in shapes.items()}
        out = {g: zeros(sh) for g, sh in en.output_shapes().items()}
        per = zeros(en.output_shapes()["members"])
        flat = lambda a: a.view((-1,) + tuple(a.shape[-2:]))
        ug, vg = (torch.zeros((E * kx, sp.il, sp.ix), dtype=torch.float64, device="cuda") for _ in range(2))
        plain = torch.zeros((3 * E * kx + E, sp.il, sp.ix), dtype=torch.float64, device="cuda")
        en.output_workspace()
        single = lambda e: sp.output_batch_dev(en.vor[0, e], en.div[0, e], en.t[0, e], en.tr[0, e], en.phi[e], en.ps[0, e],
                                               *[per[n][e] for n in ("u", "v", "t", "q", "phi", "ps")])
        single(0)                                                           # its workspace, before the capture
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            en.output(out=out)
        graphs["output E=%d ensemble call" % E] = g
        with sp.graph_capture() as g:
            for e in range(E):
                single(e)
        graphs["output E=%d single calls" % E] = g
        with sp.graph_capture() as g:
            sp.inverse_batch_segs_dev(flat(en.vor[0]), flat(en.div[0]), ug, vg, [flat(en.t[0]), flat(en.tr[0]), flat(en.phi), en.ps[0]],
                                      plain, kcos_pairs=2, kcos=1)
        graphs["output E=%d inverse batch alone" % E] = g
        keep.append((en, out, per, ug, vg, plain))
    nodes = {n: g.num_nodes() for n, g in graphs.items()}
    t = time_interleaved({n: g.launch for n, g in graphs.items()}, lambda: None, reps, repeats)
    for name, (med, lo, hi) in t.items():
        E = int(name.split("=")[1].split()[0])
        row = {"label": label, "size": tag, "form": name, "members": E, "nodes": nodes[name], "us_per_call": round(med, 2),
               "us_min": round(lo, 2), "us_max": round(hi, 2)}
        if name.endswith("ensemble call"):
            singles, inv = t["output E=%d single calls" % E][0], t["output E=%d inverse batch alone" % E][0]
            epi_bytes = (5 * kx + 1) * grid * (8 * E + 4 * (E + 2))
            call_bytes = epi_bytes + E * (5 * kx + 1) * (spec + 8 * grid)
            row.update(speedup_vs_single_calls=round(singles / med, 2), us_epilogue_by_difference=round(med - inv, 2),
                       epilogue_bytes=epi_bytes, call_byte_model_fraction_of_8TBps=round(call_bytes / (med * 1e-6) / HBM, 4),
                       epilogue_byte_model_fraction_of_8TBps=round(epi_bytes / ((med - inv) * 1e-6) / HBM, 4) if med > inv else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for g in graphs.values():
        g.close()
    sp.close()


def host_pressure_levels(en, sigma, plev, repeats):
    """the host route to the pressure-level members, mean and spread, microseconds wall-clock (median, min, max): Ensemble.output,
    the download of its float32 members, np.interp's rule on (ps / 100) * sigma vectorised over the columns, the statistics in NumPy"""
    import time
    names = ("u", "v", "t", "q", "phi")
    p_hpa = np.asarray(plev, np.float64) / 100.0
    us = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = {n: a.cpu().numpy() for n, a in en.output(stats=False)["members"].items()}
        X = (m["ps"][:, None] / np.float32(100.0)) * sigma[None, :, None, None]             # (E, kx, il, ix)
        res = {}
        for x in p_hpa:
            kb = np.clip(np.sum(X <= x, axis=1) - 1, 0, X.shape[1] - 2)[:, None]
            x0, x1 = np.take_along_axis(X, kb, 1)[:, 0], np.take_along_axis(X, kb + 1, 1)[:, 0]
            w = np.clip((x - x0) / (x1 - x0), 0.0, 1.0).astype(np.float64)
            for n in names:
                f0, f1 = np.take_along_axis(m[n], kb, 1)[:, 0], np.take_along_axis(m[n], kb + 1, 1)[:, 0]
                y = f0 + w * (f1 - f0)
                res.setdefault(n, []).append((y.astype(np.float32), y.mean(axis=0).astype(np.float32), y.std(axis=0, ddof=1).astype(np.float32)))
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us[1:])), min(us[1:]), max(us[1:])


def run_pressure(tag, members, reps, repeats, label, rows):
    """graph replays of the pressure-level output in both coordinates and of the sigma-level output, and the host route"""
    import ensemblestep
    import pressurelevels
    kx = VARIANTS[tag][3]
    sp = support.plan(tag, max(members) * (4 * kx + 4))
    plev = list(pressurelevels.SCRIPT_LEVELS)
    nlev, grid = len(plev), sp.il * sp.ix
    sigma = sp.table("fsg").astype(np.float32)
    graphs, keep, host = {}, [], {}
    for E in members:
        en = ensemblestep.build(sp, ensemblestep.member_states(sp, E))
        sp.ens_geopotential_dev(E, en.t[0], en.phis, en.phi)                 # phi of time level 1: an input of the snapshot
        zeros = lambda sh: torch.zeros(sh, dtype=torch.float32, device="cuda")
        group = lambda shapes: {g: ({n: zeros(x) for n, x in sh.items()} if isinstance(sh, dict) else zeros(sh)) for g, sh in shapes.items()}
        out_s, out_p = group(en.output_shapes()), {c: group(en.output_pressure_shapes(nlev)) for c in ("p", "logp")}
        en.output_workspace()
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            en.output(out=out_s)
        graphs["pressure E=%d sigma-level output" % E] = g
        for c in ("p", "logp"):
            with sp.graph_capture() as g:
                en.output_pressure(plev, c, below=True, out=out_p[c])
            graphs["pressure E=%d output_pressure %s" % (E, c)] = g
        host[E] = host_pressure_levels(en, sigma, plev, repeats)
        keep.append((en, out_s, out_p))
    nodes = {n: g.num_nodes() for n, g in graphs.items()}
    t = time_interleaved({n: g.launch for n, g in graphs.items()}, lambda: None, reps, repeats)
    for name, (med, lo, hi) in t.items():
        E = int(name.split("=")[1].split()[0])
        row = {"label": label, "size": tag, "form": name, "members": E, "levels": nlev, "nodes": nodes[name], "us_per_call": round(med, 2),
               "us_min": round(lo, 2), "us_max": round(hi, 2)}
        if "output_pressure" in name:
            sig = t["pressure E=%d sigma-level output" % E][0]
            kernel_bytes = grid * (nlev * (2 * 11 * E * 8 + ((E + 2) * 5 + 1) * 4) + 2 * E * 8 + (E + 2) * 4)
            row.update(ratio_to_sigma_level_output=round(med / sig, 3), host_route_us_wall=round(host[E][0], 1),
                       host_route_us_min=round(host[E][1], 1), host_route_us_max=round(host[E][2], 1),
                       host_route_times_this=round(host[E][0] / med, 1), kernel_bytes=kernel_bytes)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for g in graphs.values():
        g.close()
    sp.close()


def run_sppt(tag, members, reps, repeats, label, rows):
    """graph replays of (a) the ensemble advance and E single advances, (b) the ensemble step with the physics without and with SPPT
    and E single-state steps with SPPT"""
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    emax = max(members)
    sp = support.plan(tag, emax * (4 * kx + 4))
    case = physstep.Case(tag, sp, o)
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    sp.physics_sppt_workspace()
    # the single-state steps: a state, a workspace, a radiation state and a pattern object per member
    D0 = modelstep.device_state(case.st)
    P0 = modelstep.physics_buffers(sp, case.bnd, 0.0)
    modelstep.step(sp, {n: v.clone() for n, v in D0.items()}, modelstep.Workspace(sp), dt, physics=modelstep.whole_physics(P0, True))
    sp.synchronize()
    rad0 = P0["rad"].clone()                                   # after a shortwave step: the radiation state is whole
    seed = lambda e: 1000 + e
    singles = []
    for e in range(emax):
        D, W = {n: v.clone() for n, v in D0.items()}, modelstep.Workspace(sp)
        P = {"bnd": P0["bnd"], "rad": rad0.clone()}
        pat = s.Sppt(sp, 36, seed=seed(e))
        torch.cuda.synchronize()
        with sp.graph_capture() as ga:
            pat.advance_dev()
        with sp.graph_capture() as gs:
            modelstep.step(sp, D, W, dt, physics=modelstep.sppt_physics(P, False, pat))
        singles.append((D, W, P, pat, ga, gs))
    fns, nodes, rearms, keep = {}, {}, [], []

    def rearm_singles():
        for D, _, P, pat, _, _ in singles:
            for n in modelstep.PROG:
                D[n].copy_(D0[n])
            P["rad"].copy_(rad0)
    rearms.append(rearm_singles)
    for E in members:
        en = s.Ensemble(sp, E)
        en.set_shared(case.st)
        for e in range(E):
            en.set_member(e, case.st)
        dev = physstep.device_boundary(case.bnd, sp.il, sp.ix)
        bnd = {n: v.expand((E,) + tuple(v.shape[1:])).contiguous() for n, v in dev.items()}
        PE = {"bnd": bnd, "albsfc": bnd["albsfc"], "rad": rad0.repeat(E), "sw": False}
        pat = s.Sppt(sp, 36, seeds=[seed(e) for e in range(E)])
        en.physics_workspace(sppt=True)
        start = {n: getattr(en, n).clone() for n in modelstep.PROG}
        torch.cuda.synchronize()
        graphs = {}
        with sp.graph_capture() as g:
            pat.advance_dev()
        graphs["advance E=%d ensemble" % E] = g
        with sp.graph_capture() as g:
            en.step(2, 2, dt, PE, eps=modelstep.ROB)
        graphs["step E=%d ensemble physics" % E] = g
        with sp.graph_capture() as g:
            en.step(2, 2, dt, dict(PE, sppt=pat), eps=modelstep.ROB)
        graphs["step E=%d ensemble physics + SPPT" % E] = g
        for n, g in graphs.items():
            fns[n], nodes[n] = g.launch, g.num_nodes()

        def all_of(which, E=E):
            def fn():
                for x in singles[:E]:
                    x[which].launch()
            return fn
        fns["advance E=%d single objects" % E], nodes["advance E=%d single objects" % E] = all_of(4), E * singles[0][4].num_nodes()
        fns["step E=%d single states physics + SPPT" % E] = all_of(5)
        nodes["step E=%d single states physics + SPPT" % E] = E * singles[0][5].num_nodes()

        def rearm(en=en, start=start, PE=PE, E=E):
            for n, v in start.items():
                getattr(en, n).copy_(v)
            PE["rad"].copy_(rad0.repeat(E))
        rearms.append(rearm)
        keep.append((en, PE, pat, graphs))
    t = time_interleaved(fns, lambda: [r() for r in rearms], reps, repeats)
    for name, (med, lo, hi) in t.items():
        E = int(name.split("=")[1].split()[0])
        row = {"label": label, "size": tag, "form": name, "members": E, "nodes": nodes[name], "us": round(med, 2), "us_min": round(lo, 2),
               "us_max": round(hi, 2), "us_per_member": round(med / E, 2)}
        if name.endswith("ensemble"):
            row["speedup_vs_single_objects"] = round(t["advance E=%d single objects" % E][0] / med, 2)
        if name.endswith("ensemble physics + SPPT"):
            row["us_over_step_without_sppt"] = round(med - t["step E=%d ensemble physics" % E][0], 2)
            row["speedup_vs_single_states"] = round(t["step E=%d single states physics + SPPT" % E][0] / med, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for _, _, _, graphs in keep:
        for g in graphs.values():
            g.close()
    for x in singles:
        x[4].close(); x[5].close()
    sp.close()


def host_observations(sp, lt, tr, cols, err, repeats):
    """the host route to a nature run's observation values, microseconds wall-clock (median, min, max): the single-state output of
    the truth's spectra `tr`, its download, H and the noise in NumPy, Letkf.set_obs"""
    import time
    kx = sp.kx
    s.check(sp.lib.spdy_output_workspace(sp.h))
    out = [torch.empty((kx, sp.il, sp.ix), dtype=torch.float32, device="cuda") for _ in range(5)]
    out.append(torch.empty((sp.il, sp.ix), dtype=torch.float32, device="cuda"))
    phi = torch.zeros_like(tr[0])
    idx, w = lt.table("stencil_index"), lt.table("stencil_weight")
    row = np.where(cols[0] == 4, 4 * kx, cols[0] * kx + cols[1])[:, None]
    rng = np.random.default_rng(1)
    us = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp.output_batch_dev(tr[0], tr[1], tr[2], tr[3], phi, tr[4], *out)
        u, v, t, q, _, ps = [a.cpu().numpy().astype(np.float64) for a in out]
        f = np.concatenate([u, v, t, q, ps[None]]).reshape(4 * kx + 1, -1)[row, idx]
        h = ((w[:, 0] * f[:, 0] + w[:, 1] * f[:, 1]) + w[:, 2] * f[:, 2]) + w[:, 3] * f[:, 3]
        lt.set_obs(*cols, h + err * rng.standard_normal(h.size), err)
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us[1:])), min(us[1:]), max(us[1:])


def run_letkf(tag, members, reps, repeats, label, rows, stride=(1, 1), osse=False, at_pressure=False, masks=(), relax=None, slots=0,
              qc=None, adaptive=False):
    """graph replays of the ensemble analysis and of the ensemble step with the physics (36 of them: one six-hour cycle); osse: and
    of the nature run's observe and verify, and the host route to the same observation values; at_pressure: and of the analysis of
    the same stations with u, v, t, q given at the pressures p0 fsg[k] (Letkf.set_obs(p=...)), values and errors unchanged; relax
    = (rtpp, rtps): and of the analysis of the same network by an object with that relaxation on; slots = S: and, with the network
    divided into S equal time slots, of one slot's Ensemble.observe and of the slot analysis, next to the plain analysis of the same
    object (with at_pressure also for that object); qc = gross: and of the analysis of the same network by an object with the
    background check on at that threshold; adaptive: and of the analysis of the same network by an object with adaptive inflation
    on (Letkf.set_adaptive_inflation's defaults): two launches more"""
    import ensemblestep
    from oracle.pyoracle import Oracle, build
    build()
    kx = VARIANTS[tag][3]
    o = Oracle(*VARIANTS[tag])
    if tag in synth.SIGMA_SETS:
        o.set_sigma(synth.SIGMA_SETS[tag])
    sp = support.plan(tag, max(members) * (4 * kx + 4))
    case = physstep.Case(tag, sp, o)
    sp.surface_set_orography(case.phis0)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt)
    sp.physics_workspace()
    P = modelstep.physics_buffers(sp, case.bnd, 0.0)
    modelstep.step(sp, modelstep.device_state(case.st), modelstep.Workspace(sp), dt, physics=modelstep.whole_physics(P, True))
    sp.synchronize()
    rad0 = P["rad"].clone()                                   # after a shortwave step: the radiation state is whole
    # the network: 26 x 16 columns, u, v, t, q at every level and ps
    lon, lat = np.meshgrid((np.arange(26) + 0.5) * (360.0 / 26), -75.0 + 10.0 * np.arange(16))
    var = np.concatenate([np.repeat(np.arange(4), kx), [4]])
    lev = np.concatenate([np.tile(np.arange(kx), 4), [0]])
    nloc, per = lon.size, var.size
    cols = [np.tile(var, nloc), np.tile(lev, nloc), np.repeat(lon.ravel(), per), np.repeat(lat.ravel(), per)]
    nobs = nloc * per
    rng = np.random.default_rng(0)
    fns, nodes, rearms, keep, interp, host, used, pressure_objects, mask_objects = {}, {}, [], [], {}, {}, {}, [], []
    rejected = {}
    for E in members:
        # the members: the case's state plus a hundredth of the differences between seeded states (0.3 K in t)
        ms = ensemblestep.member_states(sp, E + 1)
        en = s.Ensemble(sp, E)
        en.set_shared(case.st)
        for e in range(E):
            en.set_member(e, {n: case.st[n] + 0.01 * (ms[e + 1][n] - ms[0][n]) for n in modelstep.PROG})
        start = {n: getattr(en, n).clone() for n in modelstep.PROG}
        lt = s.Letkf(sp, E, nobs, 5.0e5, 0.1, 1.1, **({} if stride == (1, 1) else {"weight_stride": stride}))
        lt.set_obs(*cols, np.zeros(nobs), np.ones(nobs))
        en.analyse(lt)                                        # a first call gives H x of every member: the values come from it
        torch.cuda.synchronize()
        f = lt.fields()
        spread = f["hx"].std(dim=1).cpu().numpy() + 1e-300
        lt.set_obs(*cols, f["hxmean"].cpu().numpy() + spread * rng.standard_normal(nobs), spread)
        dev = physstep.device_boundary(case.bnd, sp.il, sp.ix)
        bnd = {n: v.expand((E,) + tuple(v.shape[1:])).contiguous() for n, v in dev.items()}
        PE = {"bnd": bnd, "albsfc": bnd["albsfc"], "rad": rad0.repeat(E), "sw": False}
        en.physics_workspace()
        for n, v in start.items():
            getattr(en, n).copy_(v)
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            en.analyse(lt)
        fns["analysis E=%d" % E], nodes["analysis E=%d" % E] = g.launch, g.num_nodes()
        for K in sorted({E // 2 if m == "half" else int(m) for m in masks}):
            use = torch.ones(E, dtype=torch.int32, device="cuda")
            use[E - K:] = 0                                   # the last K members are not in use
            with sp.graph_capture() as gm:
                en.analyse(lt, use=use)
            name = "analysis E=%d mask K=%d" % (E, K)
            fns[name], nodes[name] = gm.launch, gm.num_nodes()
            mask_objects.append((use, gm))
        ltp = None
        if at_pressure:
            ltp = s.Letkf(sp, E, nobs, 5.0e5, 0.1, 1.1, **({} if stride == (1, 1) else {"weight_stride": stride}))
            ltp.set_obs(cols[0], np.where(cols[0] == 4, 0, s.OBS_AT_P), cols[2], cols[3], lt.field("value").numpy(), spread,
                        p=1.0e5 * sp.table("fsg")[cols[1]])
            en.analyse(ltp)                                   # once eagerly: how many of them are in column on this state
            torch.cuda.synchronize()
            used[E] = int(ltp.field("obs_used").numpy().sum())
            for n, v in start.items():
                getattr(en, n).copy_(v)
            torch.cuda.synchronize()
            with sp.graph_capture() as gp:
                en.analyse(ltp)
            fns["analysis at p E=%d" % E], nodes["analysis at p E=%d" % E] = gp.launch, gp.num_nodes()
            pressure_objects.append((ltp, gp))
        for kind, obj in ((("", lt),) + ((" at p", ltp),) * at_pressure) * (slots > 0):
            obj.set_slots([nobs * k // slots for k in range(slots + 1)])
            for k in range(slots):                            # every slot once, on the start state: the analysis asks for it
                en.observe(obj, k)
            torch.cuda.synchronize()
            with sp.graph_capture() as go:
                en.observe(obj, slots // 2)
            with sp.graph_capture() as gf:
                en.analyse(obj, slots=True)
            for name, gr in (("slot observe%s E=%d" % (kind, E), go), ("analysis slots%s E=%d" % (kind, E), gf)):
                fns[name], nodes[name] = gr.launch, gr.num_nodes()
                mask_objects.append((obj, gr))
            # Replays of Ensemble.analyse analyse the state the replay before left, while the slots keep the start state's hx: the
            # two graphs above solve different eigenproblems.  The finish kernel's own cost against the observation kernel's is the
            # difference of Letkf.analyse_grid, plain and by slots, on ONE gridded ensemble -- the start state's, which the last
            # observe left in the grid workspace -- with every slot observed on it: the same bits, so the same work after it
            grid = torch.from_numpy(obj.field("grid").numpy()).cuda()
            L = E * kx
            xs = [grid[v * L:(v + 1) * L].reshape((E, kx) + sp.grid_shape) for v in range(4)] + [grid[4 * L:]]
            out = [torch.empty_like(a) for a in xs]
            for k in range(slots):
                obj.observe_grid(k, *xs)
            for name, how in (("grid analysis plain%s E=%d" % (kind, E), False), ("grid analysis slots%s E=%d" % (kind, E), True)):
                with sp.graph_capture() as gg:
                    obj.analyse_grid(*xs, out=out, slots=how)
                fns[name], nodes[name] = gg.launch, gg.num_nodes()
                mask_objects.append(((xs, out), gg))
        if relax is not None:
            ltr = s.Letkf(sp, E, nobs, 5.0e5, 0.1, 1.1, rtpp=relax[0], rtps=relax[1],
                          **({} if stride == (1, 1) else {"weight_stride": stride}))
            ltr.set_obs(*cols, lt.field("value").numpy(), spread)
            with sp.graph_capture() as gr:
                en.analyse(ltr)
            fns["analysis relaxed E=%d" % E], nodes["analysis relaxed E=%d" % E] = gr.launch, gr.num_nodes()
            pressure_objects.append((ltr, gr))
            # Replays of Ensemble.analyse analyse the state the replay before left, and a relaxed ensemble keeps another spread
            # than an unrelaxed one: the two graphs above do different work in the Jacobi sweeps.  The relaxation's own cost is the
            # difference of Letkf.analyse_grid on ONE gridded ensemble, the start state's, which every replay reads again
            nat = s.Nature(sp, capacity=1)
            en.verify(ltr, nat, 0)
            torch.cuda.synchronize()
            grid = torch.from_numpy(ltr.field("grid").numpy()).cuda()
            L = E * kx
            xs = [grid[v * L:(v + 1) * L].reshape((E, kx) + sp.grid_shape) for v in range(4)] + [grid[4 * L:]]
            out = [torch.empty_like(a) for a in xs]
            nat.close()
            for name, obj in (("grid analysis E=%d" % E, lt), ("grid analysis relaxed E=%d" % E, ltr)):
                with sp.graph_capture() as gg:
                    obj.analyse_grid(*xs, out=out)
                fns[name], nodes[name] = gg.launch, gg.num_nodes()
                mask_objects.append(((xs, out), gg))
        if qc is not None:
            ltq = s.Letkf(sp, E, nobs, 5.0e5, 0.1, 1.1, **({} if stride == (1, 1) else {"weight_stride": stride}))
            ltq.set_obs(*cols, lt.field("value").numpy(), spread)
            ltq.set_background_check(qc)
            with sp.graph_capture() as gq:
                en.analyse(ltq)
            fns["analysis checked E=%d" % E], nodes["analysis checked E=%d" % E] = gq.launch, gq.num_nodes()
            pressure_objects.append((ltq, gq))
            # The check's own cost is the difference of Letkf.analyse_grid on ONE gridded ensemble, the start state's, which every
            # replay reads again: a rejected observation takes work out of the transform, so the pair is taken once more with the
            # threshold so high that nothing is rejected ("statistics only" has the same launch)
            nat = s.Nature(sp, capacity=1)
            en.verify(ltq, nat, 0)
            torch.cuda.synchronize()
            grid = torch.from_numpy(ltq.field("grid").numpy()).cuda()
            L = E * kx
            xs = [grid[v * L:(v + 1) * L].reshape((E, kx) + sp.grid_shape) for v in range(4)] + [grid[4 * L:]]
            out = [torch.empty_like(a) for a in xs]
            nat.close()
            for name, obj, gross in (("grid analysis E=%d" % E, lt, None), ("grid analysis checked E=%d" % E, ltq, qc),
                                     ("grid analysis checked none rejected E=%d" % E, ltq, 1.0e6)):
                if name in fns:
                    continue
                if gross is not None:
                    obj.set_background_check(gross)
                with sp.graph_capture() as gg:
                    obj.analyse_grid(*xs, out=out)
                fns[name], nodes[name] = gg.launch, gg.num_nodes()
                mask_objects.append(((xs, out), gg))
                if gross is not None:
                    gg.launch()
                    torch.cuda.synchronize()
                    rejected["%s" % name] = int(obj.obs_stats()["n_rej"].sum())
        if adaptive:
            lta = s.Letkf(sp, E, nobs, 5.0e5, 0.1, 1.1, adaptive=True, **({} if stride == (1, 1) else {"weight_stride": stride}))
            lta.set_obs(*cols, lt.field("value").numpy(), spread)
            with sp.graph_capture() as ga:
                en.analyse(lta)
            fns["analysis adaptive E=%d" % E], nodes["analysis adaptive E=%d" % E] = ga.launch, ga.num_nodes()
            pressure_objects.append((lta, ga))
            # Replays of Ensemble.analyse analyse the state the replay before left, and the field moves from replay to replay: the
            # two graphs above solve different eigenproblems.  What the two launches and the per-item diagonal add is the
            # difference of Letkf.analyse_grid on ONE gridded ensemble, the start state's, which every replay reads again
            nat = s.Nature(sp, capacity=1)
            en.verify(lta, nat, 0)
            torch.cuda.synchronize()
            grid = torch.from_numpy(lta.field("grid").numpy()).cuda()
            L = E * kx
            xs = [grid[v * L:(v + 1) * L].reshape((E, kx) + sp.grid_shape) for v in range(4)] + [grid[4 * L:]]
            out = [torch.empty_like(a) for a in xs]
            nat.close()
            for name, obj in (("grid analysis E=%d" % E, lt), ("grid analysis adaptive E=%d" % E, lta)):
                if name in fns:
                    continue
                with sp.graph_capture() as gg:
                    obj.analyse_grid(*xs, out=out)
                fns[name], nodes[name] = gg.launch, gg.num_nodes()
                mask_objects.append(((xs, out), gg))
        if stride != (1, 1):
            terms = int(np.count_nonzero(lt.table("interp_weight")))
            interp[E] = {"coarse_columns": int(lt.table("coarse_columns").size),
                         "apply_read_bytes": 8 * (terms * kx * E * E + (4 * kx + 1) * E * sp.il * sp.ix)}
        with sp.graph_capture() as gs:
            en.step(2, 2, dt, PE, eps=modelstep.ROB)
        fns["step E=%d physics" % E], nodes["step E=%d physics" % E] = gs.launch, gs.num_nodes()
        if osse:                                              # the truth: member 0's state at the start
            nat = s.Nature(sp, seed=E, capacity=2)
            tr = [start[n][0, 0].clone() for n in modelstep.PROG]
            with sp.graph_capture() as ga:
                nat.set_state(*tr)
                nat.observe(lt, 1.0)
            with sp.graph_capture() as gb:
                en.verify(lt, nat, 0)
            fns["observe E=%d" % E], nodes["observe E=%d" % E] = ga.launch, ga.num_nodes()
            fns["verify E=%d" % E], nodes["verify E=%d" % E] = gb.launch, gb.num_nodes()
            host[E] = host_observations(sp, lt, tr, cols, spread, repeats)
            keep.append((en, nat, PE, ga, gb))

        def rearm(en=en, start=start, PE=PE, E=E):
            for n, v in start.items():
                getattr(en, n).copy_(v)
            PE["rad"].copy_(rad0.repeat(E))
        rearms.append(rearm)
        keep.append((en, lt, PE, g, gs))
    t = time_interleaved(fns, lambda: [r() for r in rearms], reps, repeats)
    for name, (med, lo, hi) in t.items():
        E = int(name.split("=")[1].split()[0])
        row = {"label": label, "size": tag, "form": name, "members": E, "observations": nobs, "nodes": nodes[name], "us": round(med, 2),
               "us_min": round(lo, 2), "us_max": round(hi, 2)}
        if name.startswith("analysis"):
            row.update(stride=list(stride), **interp.get(E, {}))
            if name.startswith("analysis at p"):
                row.update(observations_in_column=used[E])
            if name.startswith("analysis slots"):
                plain = t[name.replace("analysis slots", "analysis")][0]
                row.update(slots=slots, us_over_plain=round(med - plain, 2))
            if " mask K=" in name:
                row.update(members_used=E - int(name.split("K=")[1]))
            cycle = 36 * t["step E=%d physics" % E][0]
            row.update(us_36_steps=round(cycle, 1), analysis_share_of_cycle=round(med / (med + cycle), 4))
        if "relaxed" in name:
            # next to the unrelaxed form of the same call: the difference of two graph replays; the relaxation kernel's bytes:
            # the ensemble and the raw increments read, the relaxed increments and the factors written
            extra = med - t[name.replace(" relaxed", "")][0]
            moved = 8 * (3 * E + 1) * (4 * kx + 1) * sp.il * sp.ix
            row.update(rtpp=relax[0], rtps=relax[1], us_over_unrelaxed=round(extra, 2), relax_bytes=moved,
                       relax_us_at_hbm_peak=round(moved / HBM * 1e6, 2))
        if "checked" in name:
            # next to the unchecked form of the same call: the difference of two graph replays; what the check's launch reads
            plain = name.replace(" checked none rejected", "").replace(" checked", "")
            row.update(gross=qc, us_over_unchecked=round(med - t[plain][0], 2), check_read_bytes=8 * nobs * (E + 3) + 4 * nobs)
            if name in rejected:
                row.update(rejected=rejected[name])
        if "adaptive" in name:
            # next to the same call with the scalar rho: the difference of two graph replays
            row.update(us_over_scalar_rho=round(med - t[name.replace(" adaptive", "")][0], 2))
        if name.startswith("grid analysis slots"):
            row.update(slots=slots, us_over_plain=round(med - t[name.replace("grid analysis slots", "grid analysis plain")][0], 2))
        if name.startswith("slot observe"):
            row.update(slots=slots, observations_in_slot=nobs * (slots // 2 + 1) // slots - nobs * (slots // 2) // slots)
        if name.startswith(("observe", "verify")):
            cycle = 36 * t["step E=%d physics" % E][0] + t["analysis E=%d" % E][0]
            row.update(us_cycle=round(cycle, 1), share_of_cycle=round(med / cycle, 5))
        rows.append(row)
        print(json.dumps(row), flush=True)
    for E, (med, lo, hi) in host.items():
        row = {"label": label, "size": tag, "form": "host route E=%d" % E, "members": E, "observations": nobs, "us": round(med, 1),
               "us_min": round(lo, 1), "us_max": round(hi, 1), "clock": "wall", "times_observe": round(med / t["observe E=%d" % E][0], 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for _, gm in mask_objects:
        gm.close()
    for _, lt, _, g, gs in keep:
        g.close(); gs.close(); lt.close()
    for ltp, gp in pressure_objects:
        gp.close(); ltp.close()
    sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+")
    ap.add_argument("--members", nargs="+", type=int)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--coupled", action="store_true")
    ap.add_argument("--output", action="store_true")
    ap.add_argument("--sppt", action="store_true")
    ap.add_argument("--letkf", action="store_true")
    ap.add_argument("--osse", action="store_true")
    ap.add_argument("--at-pressure", action="store_true")
    ap.add_argument("--slots", type=int, default=0, metavar="S")
    ap.add_argument("--mask", nargs="+", default=[], metavar="K")
    ap.add_argument("--pressure", action="store_true")
    ap.add_argument("--relax", nargs=2, type=float, metavar=("RTPP", "RTPS"))
    ap.add_argument("--qc", nargs="?", type=float, const=5.0, metavar="GROSS")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--stride", nargs=2, type=int, default=[1, 1], metavar=("SI", "SJ"))
    ap.add_argument("--earlier-library", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--reps", type=int)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    a.letkf = a.letkf or a.osse
    a.sizes = a.sizes or (["t30"] if a.sppt or a.letkf or a.pressure else ["t30", "t63k16"])
    a.members = a.members or ([4, 16, 32] if a.letkf or a.pressure else [1, 4, 16] if a.sppt else [1, 2, 4, 8, 16, 32])
    a.reps = a.reps or (100 if a.sppt or a.letkf or a.pressure else 200)
    if a.single_only:          # a library from before the ensemble entry points: bind (on first use) without them
        from speedy_f90_amd import _lib
        for n in [n for n in _lib.SIGNATURES if n.startswith("spdy_ens_") or n == "spdy_sppt_members"]:
            del _lib.SIGNATURES[n]
    batched = True
    if a.earlier_library:
        batched = "spdy_ens_surface_model_create" not in earlier_library()
    rows = []
    with torch.cuda.stream(torch.cuda.Stream()):      # the plan follows torch's stream: captures are legal, the events sit on it
        for tag in a.sizes:
            if a.letkf:
                run_letkf(tag, a.members, a.reps, a.repeats, a.label, rows, tuple(a.stride), a.osse, a.at_pressure, a.mask,
                          tuple(a.relax) if a.relax else None, a.slots, a.qc, a.adaptive)
            elif a.pressure:
                run_pressure(tag, a.members, a.reps, a.repeats, a.label, rows)
            elif a.sppt:
                run_sppt(tag, a.members, a.reps, a.repeats, a.label, rows)
            elif a.output:
                run_output(tag, a.members, a.reps, a.repeats, a.label, rows)
            elif a.coupled:
                run_coupled(tag, a.members, a.reps, a.repeats, a.label, rows, batched)
            else:
                run(tag, [] if a.single_only else a.members, a.reps, a.repeats, a.label, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
