"""One model step on the device, for the GPU tests and the rate tools: the only place under tests/ and tools/ that knows the
step's call sequence and the layout of its scratch buffers (tests/test_modelstep_cpu.py pins both without a GPU).

A step is step(j1, j2, dt) of time_stepping.f90:35-121: the inverse batch with grad ps, the grid tendencies
(tendencies.f90:89-197), optionally the geopotential and the physics (tendencies.f90:203-206), the direct batch with the spectral
step.  bench.py keeps its own two copies of this sequence on purpose: the benchmark is the yardstick and depends on no test helper,
so it is not a call site of this module."""
import physstep
import support
from dynstep import PROG, ROB, SDRAG, WIL, oracle_dynamics_step, wave_relerr
from dynstep import state as dyn_state

FORMS = ("composite", "one_launch", "separate")


class Workspace:
    """The 13 scratch buffers of a step by name, and the views into them that the calls take."""

    def __init__(self, sp, device="cuda"):
        import torch
        kx, nx, mx, il, ix = sp.kx, sp.nx, sp.mx, sp.il, sp.ix
        P = 3 * kx
        f64 = lambda n: torch.zeros((n, il, ix), dtype=torch.float64, device=device)
        c128 = lambda n: torch.zeros((n, nx, mx), dtype=torch.complex128, device=device)
        self.ug, self.vg, self.plain_g = f64(kx), f64(kx), f64(4 * kx)           # plain_g = vorg | divg | tg | trg
        self.px, self.py = f64(1), f64(1)
        self.U, self.V, self.PL = f64(P), f64(P), f64(P + 1)                     # [utend | ..], [vtend | ..], [KE | ttend | qtend | ps]
        self.pvor, self.pdiv, self.pspec = c128(P), c128(P), c128(P + 1)
        self.phi, self.phim = c128(kx), c128(kx)                                 # the step's geopotential, the physics' (level 1)
        g = self.plain_g
        self.vorg, self.divg, self.tg, self.trg = g[:kx], g[kx:2 * kx], g[2 * kx:3 * kx], g[3 * kx:]
        self.utend, self.vtend, self.ttend, self.qtend = self.U[:kx], self.V[:kx], self.PL[kx:2 * kx], self.PL[2 * kx:3 * kx]
        # the tendencies the spectral step leaves in the direct batch's outputs: vordt / divdt = pair block 0, tdt = div of block 1,
        # trdt = div of block 2, psdt = the last plain field
        self.vordt, self.divdt, self.tdt, self.trdt, self.psdt = (self.pvor[:kx], self.pdiv[:kx], self.pdiv[kx:2 * kx],
                                                                  self.pdiv[2 * kx:], self.pspec[P])


def device_state(st):
    """the state dict on the device"""
    return {n: support.dev(st[n]) for n in st}


def radiation_state(sp, fill=float("nan")):
    import torch
    return torch.full((sp.radiation_state_size(),), fill, dtype=torch.float64, device="cuda")


def physics_buffers(sp, bnd, fill=float("nan")):
    """what the physics reads and holds besides the state: the boundary fields on the device and a radiation state of `fill`"""
    return {"bnd": physstep.device_boundary(bnd, sp.il, sp.ix), "rad": radiation_state(sp, fill)}


def step(sp, D, W, dt, j1=2, j2=2, eps=ROB, physics=None, form="composite"):
    """step(j1, j2, dt).  The dynamics read time level j2 (tendencies.f90:89-107); physics(sp, D, W) runs between the grid
    tendencies and the direct batch.  form: "composite" (direct batch + spectral step as one call), "one_launch" (the direct
    batch, then spectral_step_dev), "separate" (grad ps as its own call, the direct batch, then the five spectral kernels)."""
    assert form in FORMS, form
    lv = j2 - 1
    plain_src = [D[n][lv] for n in ("vor", "div", "t", "tr")]        # read in place from the four prognostic arrays
    if form == "separate":
        sp.inverse_batch_segs_dev(D["vor"][lv], D["div"][lv], W.ug, W.vg, plain_src, W.plain_g, kcos_pairs=2, kcos=1)
        sp.grad_to_grid_dev(D["ps"][lv:lv + 1], W.px, W.py, 2)
    else:                                                            # everything that goes to the grid as one call
        sp.inverse_batch_segs_dev(D["vor"][lv], D["div"][lv], W.ug, W.vg, plain_src, W.plain_g, D["ps"][lv:lv + 1], W.px, W.py,
                                  kcos_pairs=2, kcos=1)
    sp.grid_tendencies_dev(W.ug, W.vg, W.tg, W.vorg, W.divg, W.trg, W.px, W.py, W.U, W.V, W.PL)
    if physics:
        physics(sp, D, W)
    if form == "composite":
        sp.direct_batch_spectral_step_dev(W.U, W.V, W.PL, W.pvor, W.pdiv, W.pspec, D["vor"], D["div"], D["t"], D["tr"], D["ps"],
                                          D["phis"], D["tcorh"], D["qcorh"], SDRAG, j1, dt, eps, WIL, W.phi, kcos=2)
        return
    sp.direct_batch_dev(W.U, W.V, W.pvor, W.pdiv, W.PL, W.pspec, kcos=2)
    if form == "one_launch":
        sp.spectral_step_dev(W.pvor, W.pdiv, W.pspec, D["vor"], D["div"], D["t"], D["tr"], D["ps"], D["phis"], D["tcorh"], D["qcorh"],
                             SDRAG, j1, dt, eps, WIL, W.phi)
        return
    sp.tendency_combine_dev(W.pdiv, W.pspec)
    sp.spectral_tendencies_dev(D["div"][0], D["t"][0], D["ps"][0], D["phis"], W.divdt, W.tdt, W.psdt, W.phi)
    sp.implicit_terms_dev(W.divdt, W.tdt, W.psdt)
    sp.hdiff_step_dev(D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], D["tcorh"], D["qcorh"], SDRAG, W.vordt, W.divdt, W.tdt, W.trdt)
    sp.step_fields_dev([(D["ps"], W.psdt), (D["vor"], W.vordt), (D["div"], W.divdt), (D["t"], W.tdt), (D["tr"], W.trdt)],
                       j1, dt, eps, WIL)


# ---- the physics of a step (tendencies.f90:203-206): always on time level 1 (physics.f90:94-104), whatever j2 is

def moist_physics():
    """geopotential + the moist block alone"""
    def run(sp, D, W):
        sp.geopotential_dev(D["t"][0], D["phis"], W.phim)
        sp.moist_physics_dev(D["t"][0], D["tr"][0], W.phim, D["ps"][0], W.ttend, W.qtend)
    return run


def whole_physics(P, sw, out=None):
    """geopotential + physics_dev.  out: its optional outputs (e.g. {"rad": {"ssrd": held}} to supply the held ssrd)"""
    def run(sp, D, W):
        sp.geopotential_dev(D["t"][0], D["phis"], W.phim)
        sp.physics_dev(sw, D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], W.phim, D["ps"][0], P["bnd"], P["bnd"]["albsfc"], P["rad"],
                       W.utend, W.vtend, W.ttend, W.qtend, out)
    return run


def sppt_physics(P, sw, pat, advance=True):
    """geopotential, the pattern's advance, then physics_sppt_dev in place of physics_dev"""
    def run(sp, D, W):
        sp.geopotential_dev(D["t"][0], D["phis"], W.phim)
        if advance:
            pat.advance_dev()
        sp.physics_sppt_dev(pat, sw, D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], W.phim, D["ps"][0], P["bnd"], P["bnd"]["albsfc"],
                            P["rad"], W.utend, W.vtend, W.ttend, W.qtend)
    return run


def startup(sp, delt, step_fn):
    """first_step of time_stepping.f90:12-24: the forward half step, the first leapfrog step and the three initialize_implicit
    calls.  step_fn(j1, j2, dt, n) performs a step; n = -1, 0 numbers the two for physstep.shortwave_step."""
    sp.initialize_implicit(0.5 * delt)
    step_fn(1, 1, 0.5 * delt, -1)
    sp.synchronize()
    sp.initialize_implicit(delt)
    step_fn(1, 2, delt, 0)
    sp.synchronize()
    sp.initialize_implicit(2.0 * delt)


def snapshot(D, W, P):
    """clones of the prognostics, the PL operands and the radiation state"""
    return dict({n: D[n].clone() for n in PROG}, PL=W.PL.clone(), rad=P["rad"].clone())


def three_steps(sp, case, dt, run):
    """three consecutive steps, shortwave on the first only (nstrad = 3), one radiation state held throughout; run(D, W, P, sw)
    performs one step.  Returns the snapshots after each step, and D, W, P."""
    D, W, P = device_state(case.st), Workspace(sp), physics_buffers(sp, case.bnd)
    after = []
    for n in range(3):
        run(D, W, P, n == 0)
        sp.synchronize()
        after.append(snapshot(D, W, P))
    return after, D, W, P


def oracle_dynamical_core_steps(o, sp, nsteps=2, dt=2400.0):
    """the oracle's side of run_dynamical_core_steps: [(state after step n, its out dict)], to be computed once and shared"""
    o.tail_init(dt)
    ref, seq = dyn_state(sp, 8000), []
    for n in range(nsteps):
        ref, out = oracle_dynamics_step(o, ref, 2, dt, ROB)
        seq.append((ref, out))
    return seq


def run_dynamical_core_steps(sp, o, form, nsteps=2, ref_steps=None, keep=None):
    """Captures a COMPLETE adiabatic time step of the dynamical core on device-resident state into one graph, replays it
    `nsteps` times against the oracle's call-by-call sequence and returns, per step, {array: (relerr, wave_relerr)} for the
    grid tendencies U, V, PL, the geopotential, the spectral tendencies the step leaves in place ("one_launch" keeps them in
    registers) and the five prognostics.  ref_steps: the oracle's sequence where the caller holds it already
    (oracle_dynamical_core_steps; o is not used then).  keep: a list that receives, per step, host copies of U, V, PL, phi and
    the prognostics as the device left them."""
    import torch
    import synth
    dt = 2400.0
    sp.initialize_implicit(dt)
    if ref_steps is None:
        o.tail_init(dt)
    st = dyn_state(sp, 8000)
    D, W = device_state(st), Workspace(sp)
    sp.use_own_stream()
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        step(sp, D, W, dt, form=form)
    err = lambda a, b: (synth.relerr(a.cpu().numpy(), b), wave_relerr(a.cpu().numpy(), b))
    ref, errs = st, {}
    for n in range(nsteps):
        g.launch()                                      # the graph is the whole step: nothing else runs between replays
        sp.synchronize()
        ref, out = oracle_dynamics_step(o, ref, 2, dt, ROB) if ref_steps is None else ref_steps[n]
        if keep is not None:
            keep.append(dict({k: getattr(W, k).cpu().numpy() for k in ("U", "V", "PL", "phi")}, **{k: D[k].cpu().numpy() for k in PROG}))
        e = {k: (synth.relerr(a.cpu().numpy(), out[k]),) * 2 for k, a in (("U", W.U), ("V", W.V), ("PL", W.PL))}
        e["phi"] = err(W.phi, out["phi"])
        if form != "one_launch":
            # the tendencies the spectral side leaves behind (after implicit correction and diffusion): the quantity the
            # north star's 1e-12 names
            for k in ("vordt", "divdt", "tdt", "trdt", "psdt"):
                e[k] = err(getattr(W, k), out[k])
        for k in ("ps", "vor", "div", "t", "tr"):
            e[k] = err(D[k], ref[k])
        errs["step%d" % (n + 1)] = {k: (float(v[0]), float(v[1])) for k, v in e.items()}
    g.close()
    return errs
