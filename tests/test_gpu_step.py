"""GPU: the device-resident spectral side of a time step and the captured model-step graph
(BASELINE.json config 5: T63 L16 with horizontal diffusion + implicit solve, hipGraph-captured).

Checker: the C oracle.  implicit_terms, do_horizontal_diffusion, get_geopotential and all transforms/operators in it
are pinned to flang builds of the reference (also at 16 levels), and since round 3 so is step_field_2d/3d
(time_stepping.f90:126-167: the two functions compile on their own, oracle/build_ref.sh; test_step_fields_vs_golden).
Since the end of round 3 the WHOLE adiabatic step of the oracle (tests/dynstep.py::oracle_dynamics_step: grid-space tendencies,
get_spectral_tendencies, the diffusion block of step() included) is pinned bit for bit to the reference's own
time_stepping.f90 / tendencies.f90 compiled by flang (oracle/build_ref.sh: tendencies.f90 minus its three physics lines;
tests/test_oracle_golden.py::test_dynamics_step_pinned)."""
import os

import numpy as np
import pytest

import dynstep
import modelstep
import synth
from conftest import TOL, VARIANTS
from dynstep import ROB, WIL, SDRAG, state, wave_relerr

pytestmark = pytest.mark.gpu



def ok(x, ref, tol=TOL):
    assert x.shape == ref.shape
    err = synth.relerr(x, ref)
    assert err <= tol, err


def make_plan(tag, max_batch):
    import speedy_f90_amd as s
    trunc, ix, iy, kx = VARIANTS[tag]
    sp = s.Spectral((trunc, ix, iy), kx=kx, max_batch=max_batch, device=0)
    if tag in synth.SIGMA_SETS:
        sp.set_sigma(synth.SIGMA_SETS[tag])
    return sp


@pytest.mark.parametrize("tag", ["t30", "t63", "t30k5", "t63k16", "t30k20"])
def test_step_entry_points_vs_oracle(tag, oracle_factory):
    import torch
    sp, o = make_plan(tag, 64), oracle_factory(tag)
    kx, nx, mx = sp.kx, sp.nx, sp.mx
    sp.initialize_implicit(4800.0); o.tail_init(4800.0)
    st = state(sp, 3000)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vdt, ddt, tdt, qdt = (synth.cfield((kx, nx, mx), 60 + i, s) for i, s in enumerate((1e-9, 1e-10, 1e-4, 1e-7)))
    psdt = synth.cfield((nx, mx), 70, 1e-7)
    # --- get_spectral_tendencies (tendencies.f90:242-293), j2 = 2
    d_div, d_t, d_ps, d_phis = dev(st["div"][1]), dev(st["t"][1]), dev(st["ps"][1]), dev(st["phis"])
    g_ddt, g_tdt, g_psdt, g_phi = dev(ddt), dev(tdt), dev(psdt), torch.zeros((kx, nx, mx), dtype=torch.complex128, device="cuda")
    sp.spectral_tendencies_dev(d_div, d_t, d_ps, d_phis, g_ddt, g_tdt, g_psdt, g_phi)
    r_ddt, r_tdt, r_psdt, r_phi = o.spectral_tendencies(st["div"][1], st["t"][1], st["ps"][1], st["phis"], ddt, tdt, psdt)
    torch.cuda.synchronize()
    ok(g_ddt.cpu().numpy(), r_ddt); ok(g_tdt.cpu().numpy(), r_tdt); ok(g_psdt.cpu().numpy(), r_psdt); ok(g_phi.cpu().numpy(), r_phi)
    assert g_psdt[0, 0].item() == 0
    # --- get_geopotential on device
    g_phi2 = torch.zeros_like(g_phi)
    sp.geopotential_dev(d_t, d_phis, g_phi2)
    torch.cuda.synchronize()
    ok(g_phi2.cpu().numpy(), o.geopotential(st["t"][1], st["phis"]))
    # --- the diffusion block of step() (time_stepping.f90:62-96), with and without the tracer
    ins = [dev(st[n][0]) for n in ("vor", "div", "t", "tr")] + [dev(st["tcorh"]), dev(st["qcorh"])]
    outs = [dev(x) for x in (vdt, ddt, tdt, qdt)]
    sp.hdiff_step_dev(*ins, SDRAG, *outs)
    ref = o.hdiff_step(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], st["tcorh"], st["qcorh"], SDRAG, vdt, ddt, tdt, qdt)
    torch.cuda.synchronize()
    for a, b in zip(outs, ref):
        ok(a.cpu().numpy(), b)
    outs2 = [dev(x) for x in (vdt, ddt, tdt)]
    sp.hdiff_step_dev(ins[0], ins[1], ins[2], None, ins[4], None, SDRAG, *outs2, None)
    torch.cuda.synchronize()
    for a, b in zip(outs2, ref[:3]):
        ok(a.cpu().numpy(), b)
    # --- step_field_2d/3d (time_stepping.f90:121-167): forward step (j1 = 1, eps = 0) and filtered leapfrog (j1 = 2)
    for j1, eps, dt in ((1, 0.0, 1200.0), (2, ROB, 4800.0)):
        f3, f2 = dev(st["t"]), dev(st["ps"])
        d3, d2 = dev(tdt), dev(psdt)
        sp.step_fields_dev([(f2, d2), (f3, d3)], j1, dt, eps, WIL)
        torch.cuda.synchronize()
        r3, rd3 = o.step_field(j1, dt, eps, WIL, st["t"], tdt)
        r2, rd2 = o.step_field(j1, dt, eps, WIL, st["ps"], psdt)
        ok(f3.cpu().numpy(), r3); ok(f2.cpu().numpy(), r2); ok(d3.cpu().numpy(), rd3); ok(d2.cpu().numpy(), rd2)
        # host-pointer form
        h3, hd3 = sp.step_field(j1, dt, eps, WIL, st["t"], tdt)
        ok(h3, r3); ok(hd3, rd3)
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_step_fields_vs_golden(tag):
    """spdy_step_fields_dev / spdy_step_field against the reference's OWN step_field_3d / step_field_2d
    (time_stepping.f90:126-167, flang build of the two functions cut from the reference file; tests/golden/ref_step.npz):
    j1 = 1 (forward step) and j1 = 2 (leapfrog + Robert-Asselin-Williams filter) -- pinned, not restated."""
    import torch
    z, sp = dynstep.step_golden(), make_plan(tag, 64)
    wil, rob = z[tag + "_wil_rob"]
    F3, D3, F2, D2 = dynstep.step_inputs(sp.kx, sp.nx, sp.mx)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for j1, dt, eps in ((1, 2400.0, 0.0), (2, 4800.0, rob)):
        key = "%s_j%d_" % (tag, j1)
        sub = dynstep.STEP_CASES[tag] if dynstep.STEP_CASES[tag] else (dynstep.STEP_J1_SUB if j1 == 1 else None)
        cut = (lambda a: a[(Ellipsis,) + sub]) if sub else (lambda a: a)
        f3, d3, f2, d2 = dev(F3), dev(D3), dev(F2), dev(D2)
        sp.step_fields_dev([(f2, d2), (f3, d3)], j1, dt, eps, wil)
        torch.cuda.synchronize()
        ok(cut(f3.cpu().numpy()), z[key + "f3"]); ok(f2.cpu().numpy(), z[key + "f2"])
        assert np.array_equal(cut(d3.cpu().numpy()), z[key + "d3"]) and np.array_equal(d2.cpu().numpy(), z[key + "d2"])
        h3, hd3 = sp.step_field(j1, dt, eps, wil, F3, D3)                       # host-pointer form
        ok(cut(h3), z[key + "f3"]); assert np.array_equal(cut(hd3), z[key + "d3"])
    sp.close()


def oracle_step(o, st, G, j1, dt, eps):
    """One spectral-side step on the host, call by call (the reference's own sequence; the grid-space dynamics and
    physics between the two transform batches are replaced by the given grid fields G)."""
    kx = o.kx
    j2 = 1                                                # leapfrog: dynamical tendencies from time level 2 (0-based 1)
    out = {}
    # inverse batch (tendencies.f90:89-101): uvspec + spec_to_grid(.,2) per level, spec_to_grid(.,1) of vor, div, t, tr
    ug, vg = [], []
    for k in range(kx):
        u, v = o.uvspec(st["vor"][j2, k], st["div"][j2, k])
        ug.append(o.spec_to_grid(u, 2)); vg.append(o.spec_to_grid(v, 2))
    out["ug"], out["vg"] = np.stack(ug), np.stack(vg)
    out["plain"] = np.stack([o.spec_to_grid(st[n][j2, k], 1) for n in ("vor", "div", "t", "tr") for k in range(kx)])
    # direct batch (tendencies.f90:212-234 shape): 3 kx vdspec pairs + 3 kx + 1 plain fields
    P = 3 * kx
    vd = [o.vdspec(G["ug"][i], G["vg"][i], 2) for i in range(P)]
    out["pvor"], out["pdiv"] = np.stack([x[0] for x in vd]), np.stack([x[1] for x in vd])
    out["pspec"] = np.stack([o.grid_to_spec(G["plain"][i]) for i in range(P + 1)])
    vordt, divdt = out["pvor"][:kx].copy(), out["pdiv"][:kx].copy()
    tdt, trdt = out["pdiv"][kx:2 * kx].copy(), out["pdiv"][2 * kx:3 * kx].copy()
    psdt = out["pspec"][P].copy()
    # spectral tendencies + implicit correction (tendencies.f90:34-38)
    divdt, tdt, psdt, phi = o.spectral_tendencies(st["div"][0], st["t"][0], st["ps"][0], st["phis"], divdt, tdt, psdt)
    divdt, tdt, psdt = o.implicit_terms(divdt, tdt, psdt)
    # diffusion + time integration (time_stepping.f90:62-118)
    vordt, divdt, tdt, trdt = o.hdiff_step(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], st["tcorh"], st["qcorh"], SDRAG,
                                           vordt, divdt, tdt, trdt)
    new = dict(st)
    new["ps"], _ = o.step_field(j1, dt, eps, WIL, st["ps"], psdt)
    for n, d in (("vor", vordt), ("div", divdt), ("t", tdt), ("tr", trdt)):
        new[n], _ = o.step_field(j1, dt, eps, WIL, st[n], d)
    out["phi"] = phi
    return new, out


@pytest.mark.parametrize("tag", ["t30", "t63", "t63k16"])
def test_model_step_graph(tag, oracle_factory):
    """The whole spectral side of a time step -- both transform batches (spdy_inverse_batch_dev, spdy_direct_batch_dev),
    get_spectral_tendencies, implicit_terms, the diffusion block and the leapfrog/RAW update of all five prognostics --
    captured into ONE graph on device-resident state, replayed for two consecutive steps and compared with the oracle
    call by call.  t63k16 is BASELINE.json config 5 (T63 L16)."""
    import torch
    kx = VARIANTS[tag][3]
    sp, o = make_plan(tag, 4 * kx + 4), oracle_factory(tag)
    nx, mx, il, ix = sp.nx, sp.mx, sp.il, sp.ix
    dt = 4800.0
    sp.initialize_implicit(dt); o.tail_init(dt)
    st = state(sp, 5000)
    P = 3 * kx
    G = {"ug": synth.grids(P, ix, il, first=9000) * 1e-3, "vg": synth.grids(P, ix, il, first=9500) * 1e-3,
         "plain": synth.grids(P + 1, ix, il, first=9900) * 1e-4}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    D = {n: dev(st[n]) for n in st}
    DG = {n: dev(G[n]) for n in G}
    c128 = lambda *shape: torch.zeros(shape, dtype=torch.complex128, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    ug, vg, plain_g = f64(kx, il, ix), f64(kx, il, ix), f64(4 * kx, il, ix)
    pvor, pdiv, pspec = c128(P, nx, mx), c128(P, nx, mx), c128(P + 1, nx, mx)
    phi = c128(kx, nx, mx)
    torch.cuda.synchronize()
    sp.use_own_stream()

    # inverse batch from time level 2: kx (vor, div) pairs -> (u, v) grids; the vor, div, t, tr levels -> grids, read straight
    # from the four prognostic arrays (spdy_inverse_batch_segs_dev: nothing runs outside the graph between replays)
    plain_src = [D[n][1] for n in ("vor", "div", "t", "tr")]
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        sp.inverse_batch_segs_dev(D["vor"][1], D["div"][1], ug, vg, plain_src, plain_g, kcos_pairs=2, kcos=1)
        sp.direct_batch_dev(DG["ug"], DG["vg"], pvor, pdiv, DG["plain"], pspec, kcos=2)
        # tendencies are views into the direct batch's outputs: vordt/divdt = pair block 0, tdt = div of block 1, trdt = div of block 2
        vordt, divdt, tdt, trdt, psdt = pvor[:kx], pdiv[:kx], pdiv[kx:2 * kx], pdiv[2 * kx:3 * kx], pspec[P]
        sp.spectral_tendencies_dev(D["div"][0], D["t"][0], D["ps"][0], D["phis"], divdt, tdt, psdt, phi)
        sp.implicit_terms_dev(divdt, tdt, psdt)
        sp.hdiff_step_dev(D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], D["tcorh"], D["qcorh"], SDRAG, vordt, divdt, tdt, trdt)
        sp.step_fields_dev([(D["ps"], psdt), (D["vor"], vordt), (D["div"], divdt), (D["t"], tdt), (D["tr"], trdt)], 2, dt, ROB, WIL)
    assert float(ug.abs().max()) == 0.0                                           # nothing ran during the capture
    ref = st
    for step in range(2):
        g.launch()
        sp.synchronize()
        ref, out = oracle_step(o, ref, G, 2, dt, ROB)
        ok(ug.cpu().numpy(), out["ug"]); ok(vg.cpu().numpy(), out["vg"]); ok(plain_g.cpu().numpy(), out["plain"])
        ok(phi.cpu().numpy(), out["phi"])
        for n in ("ps", "vor", "div", "t", "tr"):
            ok(D[n].cpu().numpy(), ref[n])
    g.close()
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_output_path_vs_reference(tag, oracle_factory):
    """SURVEY s8 f4 against the REFERENCE, no oracle in between: spdy_output_batch_dev on the seeded state vs the golden float32
    fields of the reference's own lines (input_output.f90:183-205 cut out of the file as they are and compiled by flang,
    tests/golden/ref_output.npz) at 8, 5 and 16 levels.  Every value within one float32 ulp; the five linear fields differ in
    at most a handful of values (an FP64 difference of 1e-15 only shows next to a float32 rounding boundary)."""
    import torch
    from golden.make_golden import OUT_SUB, OUT_SEED
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_output.npz"))
    sp, o = make_plan(tag, 4 * VARIANTS[tag][3] + 4), oracle_factory(tag)
    kx, il, ix = sp.kx, sp.il, sp.ix
    st = state(sp, OUT_SEED)
    phi = o.geopotential(st["t"][0], st["phis"])            # an INPUT of the snapshot (pinned: test_other_level_counts_and_geopotential)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ins = [dev(st[n][0]) for n in ("vor", "div", "t", "tr")] + [dev(phi), dev(st["ps"][0])]
    outs = [torch.zeros((kx, il, ix), dtype=torch.float32, device="cuda") for _ in range(5)] + [torch.zeros((il, ix), dtype=torch.float32, device="cuda")]
    sp.output_batch_dev(*ins, *outs)
    torch.cuda.synchronize()
    flips = total = 0
    for name, a in zip(("u", "v", "t", "q", "phi", "ps"), outs):
        a = a.cpu().numpy()
        a = a if name == "ps" else a[OUT_SUB[tag]]
        b = z["%s_%s" % (tag, name)]
        ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (name, ulp.max())
        if name != "ps":
            flips += int((ulp != 0).sum()); total += b.size
    print("output path vs reference %s: %d of %d linear float32 values differ by one ulp" % (tag, flips, total))
    assert flips <= 8, flips
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63"])
def test_output_path(tag, oracle_factory):
    """the snapshot path of input_output.f90:184-206 as one device call.  float32 results must be
    BIT-EXACT where the epilogue is linear (u, v, t, q*1e-3, phi/grav: an inverse-transform difference of 1e-15 only
    shows when a value sits within that distance of a float32 rounding boundary -- counted, at most a handful); ps_out
    goes through exp(), so it is held to one float32 ulp."""
    import torch
    sp, o = make_plan(tag, 4 * 8 + 4), oracle_factory(tag)
    kx, nx, mx, il, ix = sp.kx, sp.nx, sp.mx, sp.il, sp.ix
    st = state(sp, 7000)
    phi = o.geopotential(st["t"][0], st["phis"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ins = [dev(st[n][0]) for n in ("vor", "div", "t", "tr")] + [dev(phi), dev(st["ps"][0])]
    outs = [torch.zeros((kx, il, ix), dtype=torch.float32, device="cuda") for _ in range(5)] + [torch.zeros((il, ix), dtype=torch.float32, device="cuda")]
    sp.output_batch_dev(*ins, *outs)
    torch.cuda.synchronize()
    ref = o.output(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])
    flips = 0
    for name, a, b in zip(("u", "v", "t", "q", "phi", "ps"), outs, ref):
        a = a.cpu().numpy()
        ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (name, ulp.max())
        flips += int((ulp != 0).sum())
        assert synth.relerr(a.astype(np.float64), b.astype(np.float64)) <= 2e-7
    assert flips <= 8, flips          # of ~190k (T30) / ~750k (T63) float32 values
    # captured into a graph it gives the same bits
    sp.use_own_stream()
    outs2 = [torch.zeros_like(x) for x in outs]
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        sp.output_batch_dev(*ins, *outs2)
    g.launch(); sp.synchronize()
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    g.close(); sp.close()


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_dynamical_core_step_vs_reference_step(tag):
    """The device step against the REFERENCE'S OWN step(): golden vectors of one call of time_stepping.f90 step(j1, j2, dt) --
    the file compiled by flang unchanged, on tendencies.f90 minus its three physics lines (tests/golden/ref_dynstep.npz,
    tests/golden/make_golden.py) -- for the forward half step (j1 = j2 = 1, T30 L8) and the filtered leapfrog step
    (j1 = j2 = 2) at 8, 5 and 16 levels.  No oracle in between: HIP kernels vs flang-compiled Fortran, 1e-12 of each array's
    maximum, with and without the global mean."""
    import os
    import torch
    from conftest import ROOT
    from golden.make_golden import DYNSTEP_CASES, DYN63_SUB, STEP_SUB
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_dynstep.npz"))
    kx = VARIANTS[tag][3]
    sp = make_plan(tag, 4 * kx + 4)
    sub = DYN63_SUB if tag == "t63k16" else STEP_SUB
    st = state(sp, 8000)
    for j1, j2, dt in (DYNSTEP_CASES if tag == "t30" else DYNSTEP_CASES[1:]):
        sp.initialize_implicit(dt)
        D, W = modelstep.device_state(st), modelstep.Workspace(sp)
        modelstep.step(sp, D, W, dt, j1, j2, 0.0 if j1 == 1 else ROB)
        sp.synchronize()
        key = "%s_j%d%d_" % (tag, j1, j2)
        worst = 0.0
        for n in ("vor", "div", "t", "tr"):
            got, ref = D[n].cpu().numpy()[(Ellipsis,) + sub[1:]], z[key + n]
            worst = max(worst, synth.relerr(got, ref), wave_relerr(got, ref))
        worst = max(worst, synth.relerr(D["ps"].cpu().numpy(), z[key + "ps"]), wave_relerr(W.phi.cpu().numpy()[sub], z[key + "phi"]))
        print("\n[device step vs reference step() %s j1=%d j2=%d dt=%g] worst relative error %.1e" % (tag, j1, j2, dt, worst))
        assert worst <= TOL, (tag, j1, j2, worst)
    sp.close()


FORMS = {False: "separate", True: "one_launch", "composite": "composite"}


@pytest.mark.parametrize("one_launch_tail", [False, True, "composite"])
@pytest.mark.parametrize("tag", ["t30", "t63k16", "t30k20"])
def test_dynamical_core_step_graph(tag, one_launch_tail, oracle_factory):
    """SURVEY s8 f3 + f2: a COMPLETE adiabatic time step of the dynamical core on device-resident state, captured into one
    graph -- inverse batch (+ grad -> grid), grid-space dynamical tendencies (tendencies.f90:105-197), direct batch,
    tendency combination, spectral tendencies, implicit correction, diffusion block, leapfrog/RAW -- replayed for two
    steps against the oracle's call-by-call sequence.  Only get_physical_tendencies (column physics, out of scope) is
    missing from the reference's step().

    Bars (measured values: tools/step_error_budget.py, profiles/r03_step_error_budget.json):
      * every TENDENCY -- grid (U, V, PL) and spectral (vordt .. psdt after the implicit correction and the diffusion) -- and
        the geopotential: 1e-12 of the array's maximum, the north star's bar, in both norms;
      * prognostics after each of the two chained steps: 1e-12 in the wave norm (global mean removed) as well as in the plain
        norm -- the leapfrog adds dt * tendency (relative error <= 1e-12) to a filtered state that is exact to rounding."""
    kx = VARIANTS[tag][3]
    sp, o = make_plan(tag, 4 * kx + 4), oracle_factory(tag)
    errs = modelstep.run_dynamical_core_steps(sp, o, FORMS[one_launch_tail])
    sp.close()
    print("\n[step errors %s one_launch=%s] " % (tag, one_launch_tail) + "; ".join(
        "%s: " % st + " ".join("%s %.1e/%.1e" % (n, e[0], e[1]) for n, e in d.items()) for st, d in errs.items()))
    for st, d in errs.items():
        for n, (e_all, e_wave) in d.items():
            assert e_all <= TOL and e_wave <= TOL, (tag, st, n, e_all, e_wave)


@pytest.mark.parametrize("case", ["rest", "wind"])
def test_two_day_run_vs_reference(case, oracle_factory):
    """BASELINE config 1's stand-in on the device: the reference's start-up sequence (time_stepping.f90:12-24: forward half step,
    first leapfrog step, three initialize_implicit calls) as eager calls, then `step(2, 2, 2*delt)` captured ONCE and replayed 72
    times = 2 model days at T30 L8, from the reference's own rest state over a seeded orography (tests/longrun.py), with nothing
    but graph replays between the checkpoints.  Checked against golden vectors of the FLANG-BUILT REFERENCE running the same 74
    steps (tests/golden/ref_run72.npz; no oracle in the comparison -- the oracle only builds the initial state).
    Bar: the north star's 1e-12 of each array's maximum, with and without the global mean, at EVERY checkpoint up to step 72
    (measured: <= 1.8e-14 after two days, profiles/r04_two_day_run_error.txt -- rounding differences are not amplified
    measurably by two days of this flow)."""
    import torch
    import longrun
    from conftest import ROOT
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_run72.npz"))
    o = oracle_factory("t30")
    sp = make_plan("t30", 36)
    st = longrun.rest_state(o, wind=longrun.CASES[case])
    D, W = modelstep.device_state(st), modelstep.Workspace(sp)
    sp.use_own_stream()
    torch.cuda.synchronize()
    modelstep.startup(sp, longrun.DELT, lambda j1, j2, dt, n: modelstep.step(sp, D, W, dt, j1, j2, 0.0))
    with sp.graph_capture() as g:
        modelstep.step(sp, D, W, 2.0 * longrun.DELT)
    lines, worst = [], 0.0
    for n in range(1, longrun.NSTEPS + 1):
        g.launch()
        if n in longrun.CHECKPOINTS:
            sp.synchronize()
            e = {}
            for k in ("vor", "div", "t", "tr", "ps"):
                got, ref = longrun.cut(k, D[k].cpu().numpy()), z["%s_%d_%s" % (case, n, k)]
                assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), (case, n, k)
                e[k] = max(synth.relerr(got, ref), wave_relerr(got, ref))
            worst = max(worst, max(e.values()))
            lines.append("step %2d: " % n + " ".join("%s %.1e" % kv for kv in e.items()))
    g.close(); sp.close()
    print("\n[2-day run '%s' vs the flang-built reference, relative error (max of plain and mean-free norm)]\n  " % case + "\n  ".join(lines))
    assert worst <= TOL, (case, worst)
