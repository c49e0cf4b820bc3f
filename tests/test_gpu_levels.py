"""GPU: the level-dependent kernels of the time step (csrc/spdy_step.hip, csrc/spdy_api_step.hip) at every class of their
specialisation by level count -- tests/levels.py names the classes and the counts.  conftest.VARIANTS only has kx = 5, 7, 8, 16 and
20: the 9..15 instantiations (plain, write-through, level-sharded, ensemble), the counts below 5, the even partial block, the first
serial count and the implicit kernel above 64 KiB of LDS run here and nowhere else.

Checker: the C oracle on levels.sigma(kx), pinned bit for bit to flang builds of the reference at 5, 7, 8, 16 and -- inside the
9..15 class -- 12 levels (tests/test_oracle_golden.py::test_levels12_pinned).  Bar: conftest.TOL in synth.relerr and
dynstep.wave_relerr, per array; the error per level is printed, and held to the same bar where the operation does not couple
levels."""
import numpy as np
import pytest

import ensemblestep as es
import guards
import levels
import modelstep
import shardedstep
import support
import synth
from conftest import TOL
from dynstep import ROB, SDRAG, WIL, state, wave_relerr

pytestmark = pytest.mark.gpu

LEVELS = levels.LEVELS
FORMS = ("separate", "one_launch", "composite")
ROUNDING = 1e-13          # include/spdy.h: what the forms of a step agree to where they are not bit-equal ("to rounding")


def by_level(name, got, ref, kx, hold):
    """prints the per-level error (guards.field_err over the level axis of [.., kx, n, m] arrays, both host arrays) and names the
    worst level; hold: the operation is level-local, so every level is held to TOL on its own"""
    import torch
    g = torch.from_numpy(np.ascontiguousarray(got)).reshape((-1, kx) + got.shape[-2:]).transpose(0, 1).contiguous()
    r = torch.from_numpy(np.ascontiguousarray(ref)).reshape((-1, kx) + ref.shape[-2:]).transpose(0, 1).contiguous()
    e = guards.field_err(torch, g, r)
    k, w = guards.worst(e)
    print("[levels kx=%d] %s: worst level %d of %d, %.1e" % (kx, name, k, kx, w))
    if hold:
        assert w <= TOL, (name, "level", k, w)
    return k, w


def ok(name, x, ref, kx=None, hold=False):
    assert x.shape == ref.shape, name
    where = by_level(name, x, ref, kx, hold) if kx and x.ndim >= 3 and x.shape[-3] % kx == 0 else None
    e, ew = synth.relerr(x, ref), wave_relerr(x, ref) if np.iscomplexobj(ref) else 0.0
    assert e <= TOL and ew <= TOL, (name, e, ew, "worst level", where)      # (NaN, a field never written, fails too)


# ------------------------------------------------------------------------------------------------ a. entry points one by one
@pytest.mark.parametrize("kx", LEVELS)
def test_entry_points_vs_oracle(kx):
    """tests/test_gpu_step.py::test_step_entry_points_vs_oracle at every level count, every output a view into a guarded
    allocation that starts as NaN (in-out arguments: as their inputs), every input compared with a copy afterwards"""
    import torch
    sp, o = levels.plan("t30", kx, 64 if kx <= 15 else 4 * kx + 4), levels.oracle("t30", kx)
    nx, mx, il, ix = sp.nx, sp.mx, sp.il, sp.ix
    st = state(sp, 3000)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda a: a.cpu().numpy()
    vdt, ddt, tdt, qdt = (synth.cfield((kx, nx, mx), 60 + i, s) for i, s in enumerate((1e-9, 1e-10, 1e-4, 1e-7)))
    psdt = synth.cfield((nx, mx), 70, 1e-7)
    imp = synth.tail_inputs(kx, nx, mx)
    # the outputs, in call order: spectral tendencies (ddt, tdt, psdt, phi) | geopotential | hdiff with (4) and without (3) the
    # tracer | implicit terms at two dt (div, t, ps each) | step_fields for j1 = 1, 2 (f3, f2, d3, d2 each)
    counts = [kx, kx, 1, kx] + [kx] + [kx] * 4 + [kx] * 3 + [kx, kx, 1] * 2 + [2 * kx, 2, kx, 1] * 2
    C = guards.Guarded(torch, (nx, mx), counts, complex_=True)
    G = guards.Guarded(torch, (il, ix), [3 * kx, 3 * kx, 3 * kx + 1])
    out = iter(C.outs)

    def put(a):                                         # the next guarded output, holding a (an in-out argument)
        v = next(out)
        v.view(a.shape).copy_(dev(a))
        return v.view(a.shape)
    d_in = {n: dev(st[n]) for n in st}
    keep = {n: d_in[n].clone() for n in d_in}
    sp.initialize_implicit(4800.0); o.tail_init(4800.0)
    # --- get_spectral_tendencies (tendencies.f90:242-293), j2 = 2
    g_ddt, g_tdt, g_psdt = put(ddt), put(tdt), put(psdt).view(nx, mx)
    g_phi = next(out)
    sp.spectral_tendencies_dev(d_in["div"][1], d_in["t"][1], d_in["ps"][1], d_in["phis"], g_ddt, g_tdt, g_psdt, g_phi)
    r = o.spectral_tendencies(st["div"][1], st["t"][1], st["ps"][1], st["phis"], ddt, tdt, psdt)
    torch.cuda.synchronize()
    for name, a, b in zip(("spectend divdt", "spectend tdt", "spectend psdt", "spectend phi"), (g_ddt, g_tdt, g_psdt, g_phi), r):
        ok(name, host(a), b, kx)
    assert g_psdt[0, 0].item() == 0
    # --- get_geopotential
    g_phi2 = next(out)
    sp.geopotential_dev(d_in["t"][1], d_in["phis"], g_phi2)
    torch.cuda.synchronize()
    ok("geopotential", host(g_phi2), o.geopotential(st["t"][1], st["phis"]), kx)
    # --- the diffusion block of step() (time_stepping.f90:62-96), with and without the tracer: level-local
    ins = [d_in[n][0] for n in ("vor", "div", "t", "tr")] + [d_in["tcorh"], d_in["qcorh"]]
    outs = [put(x) for x in (vdt, ddt, tdt, qdt)]
    sp.hdiff_step_dev(*ins, SDRAG, *outs)
    ref = o.hdiff_step(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], st["tcorh"], st["qcorh"], SDRAG, vdt, ddt, tdt, qdt)
    torch.cuda.synchronize()
    for name, a, b in zip(("vordt", "divdt", "tdt", "trdt"), outs, ref):
        ok("hdiff " + name, host(a), b, kx, hold=True)
    outs2 = [put(x) for x in (vdt, ddt, tdt)]
    sp.hdiff_step_dev(ins[0], ins[1], ins[2], None, ins[4], None, SDRAG, *outs2, None)
    torch.cuda.synchronize()
    for name, a, b in zip(("vordt", "divdt", "tdt"), outs2, ref[:3]):
        ok("hdiff (no tracer) " + name, host(a), b, kx, hold=True)
    # --- implicit_terms (implicit.f90:168-217) at two time steps
    for dt in (1200.0, 4800.0):
        sp.initialize_implicit(dt); o.tail_init(dt)
        a, b, c = put(imp[0]), put(imp[1]), put(imp[2]).view(nx, mx)
        sp.implicit_terms_dev(a, b, c)
        torch.cuda.synchronize()
        for name, x, y in zip(("divdt", "tdt", "psdt"), (a, b, c), o.implicit_terms(*imp)):
            ok("implicit dt=%g %s" % (dt, name), host(x), y, kx)
    # --- step_field_2d/3d (time_stepping.f90:121-167): forward step and filtered leapfrog; level-local
    for j1, eps, dt in ((1, 0.0, 1200.0), (2, ROB, 4800.0)):
        f3, f2, d3, d2 = put(st["t"]), put(st["ps"]), put(tdt), put(psdt).view(nx, mx)
        sp.step_fields_dev([(f2, d2), (f3, d3)], j1, dt, eps, WIL)
        torch.cuda.synchronize()
        r3, rd3 = o.step_field(j1, dt, eps, WIL, st["t"], tdt)
        r2, rd2 = o.step_field(j1, dt, eps, WIL, st["ps"], psdt)
        ok("step_fields j1=%d f3" % j1, host(f3), r3, kx, hold=True); ok("step_fields j1=%d d3" % j1, host(d3), rd3, kx, hold=True)
        ok("step_fields j1=%d f2" % j1, host(f2), r2); ok("step_fields j1=%d d2" % j1, host(d2), rd2)
    assert next(out, None) is None
    # --- get_grid_point_tendencies (tendencies.f90:105-197)
    gr = lambda first, scale, n=kx: synth.grids(n, ix, il, first=first) * scale
    ug, vg, tg, vorg, divg, trg = gr(100, 40.0), gr(200, 40.0), gr(300, 60.0) + 250.0, gr(400, 1e-4), gr(500, 1e-5), gr(600, 1e-2)
    px, py = gr(700, 1e-2, 1), gr(701, 1e-2, 1)
    h_in = (ug, vg, tg, vorg, divg, trg, px, py)
    g_in = [dev(x) for x in h_in]
    U, V, PL = G.outs
    sp.grid_tendencies_dev(*g_in, U, V, PL)
    torch.cuda.synchronize()
    for name, a, b in zip("U V PL".split(), (U, V, PL), o.grid_tendencies(ug, vg, tg, vorg, divg, trg, px[0], py[0])):
        ok("grid tendencies " + name, host(a), np.asarray(b).reshape(host(a).shape))
        by_level("grid tendencies " + name, host(a)[:3 * kx], np.asarray(b).reshape(host(a).shape)[:3 * kx], kx, hold=False)
    # nothing outside the outputs was written, no input was changed
    assert C.intact(), ("spectral outputs", C.hits())
    assert G.intact(), ("grid outputs", G.hits())
    for n in d_in:
        assert support.same_bits(d_in[n], keep[n]), n
    for a, b in zip(g_in, h_in):
        assert np.array_equal(host(a), b)
    sp.close()


def test_level_counts_side_by_side():
    """Plans of 32, 22 and 12 levels alive together, made in that order: the implicit kernel of each still launches and gives
    the oracle's values (its dynamic-LDS limit above 64 KiB is a property of the kernel, not of the plan made last)."""
    import torch
    plans = [levels.plan("t30", kx, 4) for kx in (32, 22, 12)]
    for sp in plans:
        sp.initialize_implicit(2400.0)
    for sp in plans:
        o = levels.oracle("t30", sp.kx)
        o.tail_init(2400.0)
        imp = synth.tail_inputs(sp.kx, sp.nx, sp.mx)
        d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in imp]
        sp.implicit_terms_dev(*d)
        torch.cuda.synchronize()
        for name, x, y in zip(("divdt", "tdt", "psdt"), d, o.implicit_terms(*imp)):
            ok("implicit kx=%d %s" % (sp.kx, name), x.cpu().numpy(), y)
    for sp in plans:
        sp.close()


# ------------------------------------------------------------------------------------- b, c. the whole step in its three forms
_REF, _RUNS = {}, {}


def reference_steps(tag, kx, sp):
    """the oracle's two steps at (tag, kx): computed once, shared by every form, never changed"""
    if (tag, kx) not in _REF:
        _REF[tag, kx] = modelstep.oracle_dynamical_core_steps(levels.oracle(tag, kx), sp)
    return _REF[tag, kx]


def device_steps(tag, kx, form):
    """(errors vs the oracle, what the device left after each of the two replays) of modelstep.run_dynamical_core_steps"""
    if (tag, kx, form) not in _RUNS:
        sp = levels.plan(tag, kx, 4 * kx + 4)
        keep = []
        errs = modelstep.run_dynamical_core_steps(sp, None, form, ref_steps=reference_steps(tag, kx, sp), keep=keep)
        sp.close()
        print("\n[step errors %s L%d %s] " % (tag, kx, form) + "; ".join(
            "%s: " % st + " ".join("%s %.1e/%.1e" % (n, e[0], e[1]) for n, e in d.items()) for st, d in errs.items()))
        w = max(((max(e), n) for n, e in errs["step2"].items()), key=lambda x: (np.isnan(x[0]), x[0]))
        print("[worst of step 2 %s L%d %s] %s %.1e" % (tag, kx, form, w[1], w[0]))
        _RUNS[tag, kx, form] = (errs, keep)
    return _RUNS[tag, kx, form]


def hold_errors(errs, what):
    for st, d in errs.items():
        for n, (e_all, e_wave) in d.items():
            assert e_all <= TOL and e_wave <= TOL, (what, st, n, e_all, e_wave)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kx", LEVELS)
def test_dynamical_core_step_graph(kx, form):
    """tests/test_gpu_step.py::test_dynamical_core_step_graph at every level count: the complete adiabatic step captured into one
    graph, two replays against the oracle.  Above 16 levels the one-launch entry points fall back to the five kernels."""
    hold_errors(device_steps("t30", kx, form)[0], (kx, form))


@pytest.mark.parametrize("kx", LEVELS)
def test_forms_agree(kx):
    """At T30 a field's bits do not depend on the launch form of the transforms: up to 16 levels "one_launch" and "composite" run
    the same spectral-step kernel on the same spectra and must agree bit for bit on every prognostic, phi and U, V, PL; the
    five-kernel form ("separate", and every form above 16 levels) evaluates the same sums in other groupings and is held to
    1e-13 of the array's maximum."""
    runs = {f: device_steps("t30", kx, f)[1] for f in FORMS}
    names = modelstep.PROG + ("phi", "U", "V", "PL")
    for n in range(2):
        one, comp, sep = (runs[f][n] for f in ("one_launch", "composite", "separate"))
        for k in names:
            assert np.all(np.isfinite(comp[k])), (kx, n, k)
            if kx <= 16:
                assert np.array_equal(one[k], comp[k]), (kx, n, k, synth.relerr(one[k], comp[k]))
            else:
                assert synth.relerr(one[k], comp[k]) <= ROUNDING, (kx, n, k, synth.relerr(one[k], comp[k]))
            assert synth.relerr(sep[k], comp[k]) <= ROUNDING, (kx, n, k, synth.relerr(sep[k], comp[k]))


# ------------------------------------------------------------------------------------------------ d. T63, the raw-pair route
@pytest.mark.parametrize("kx", [12, 9])
def test_t63_raw_pair_route(kx):
    """T63 at 12 and 9 levels: the direct batch leaves the pairs' spectra un-vds'ed and spectral_step_kernel<8, false, false>
    applies vds where it reads them (use_raw63 accepts kx <= 16) -- composite and one_launch, two replays against the oracle."""
    for form in ("composite", "one_launch"):
        hold_errors(device_steps("t63", kx, form)[0], (kx, form))


# ------------------------------------------------------------------------------------------- e. write-through instantiations
@pytest.mark.parametrize("kx", [6, 12])
def test_write_through_policy_same_bits(kx):
    """tests/test_gpu_determinism.py::test_write_through_policy_same_bits in the <8, false> and <16, false> grid-tendencies
    kernels: the write-through instantiation (wt_min_mb = 1) against the write-back one (0), same bits"""
    import torch
    sp = levels.plan("t30", kx, 4 * kx + 4)
    sp.initialize_implicit(2400.0)
    dev = torch.device("cuda", 0)
    nb = 4 * kx + 2
    S = torch.from_numpy(synth.spectra(nb, sp.trunc, first=11, full_rows=True)).to(dev)
    rng = np.random.default_rng(99)
    px, py = (torch.from_numpy(rng.uniform(-1e-2, 1e-2, (1, sp.il, sp.ix))).to(dev) for _ in range(2))

    def run():
        f64 = lambda n: torch.full((n, sp.il, sp.ix), float("nan"), dtype=torch.float64, device=dev)
        G, U, V, PL = f64(nb), f64(3 * kx), f64(3 * kx), f64(3 * kx + 1)
        back = torch.full((3 * kx, sp.nx, sp.mx), float("nan"), dtype=torch.complex128, device=dev)
        sp.spec_to_grid_dev(S, G, kcos=1)
        g = [G[i * kx:(i + 1) * kx] for i in range(4)]
        sp.grid_tendencies_dev(g[0], g[1], g[2] + 250.0, g[3], g[0] * 1e-6, g[1].abs() * 1e-3, px, py, U, V, PL)
        sp.grid_to_spec_dev(U, back)
        sp.synchronize()
        return G, U, V, PL, back
    sp.set_option("wt_min_mb", 1)
    a = run()
    sp.set_option("wt_min_mb", 0)
    b = run()
    for i, (x, y) in enumerate(zip(a, b)):
        assert not torch.isnan(x.real if x.is_complex() else x).any(), i
        assert torch.equal(x, y), (kx, i)
    sp.close()


# ------------------------------------------------------------------------------------------------------------- f. ensemble
def test_ensemble_in_guarded_arrays():
    """(E, kx) = (3, 12), both sequences, with every array of the ensemble a view into a guarded allocation (Ensemble adopts
    caller-made tensors): each member bit-equal to the single-state step, and no store outside the arrays -- in particular none
    behind the level-free slots 3 E kx + e of PL and pspec."""
    import torch
    import speedy_f90_amd as s
    from speedy_f90_amd.ensemble import shapes
    E, kx, delt = 3, 12, 2400.0
    sp = levels.plan("t30", kx, E * (4 * kx + 4))
    sh = shapes(E, kx, sp.nx, sp.mx, sp.il, sp.ix)
    for seq in (es.LEAPFROG, es.STARTUP):
        pools, arrays = [], {}
        for cplx in (True, False):
            names = [n for n in sh if sh[n][1] == cplx]
            field = (sp.nx, sp.mx) if cplx else (sp.il, sp.ix)
            pool = guards.Guarded(torch, field, [int(np.prod(sh[n][0][:-2])) for n in names], complex_=cplx)
            for n, v in zip(names, pool.outs):
                v.zero_()
                arrays[n] = v.view(sh[n][0])
            pools.append(pool)
        ens = s.Ensemble(sp, E, arrays=arrays)
        assert ens.PL.data_ptr() == arrays["PL"].data_ptr() and ens.vor.data_ptr() == arrays["vor"].data_ptr()
        sts = es.member_states(sp, E)
        ens.set_shared(sts[0])
        for e, st in enumerate(sts):
            ens.set_member(e, st)
        snaps = es.run_ensemble(sp, ens, seq, delt)
        for pool in pools:
            assert pool.intact(), pool.hits()
        for e in range(E):
            assert es.differing(sp, snaps, e, sts[e], seq, delt) == [], (seq, e)
    sp.close()


# ------------------------------------------------------------------------------- g. level-sharded step, in-process ranks
SHARDED = [(12, 5), (9, 2), (15, 4), (6, 4)]       # (kx, world): uneven level blocks in the SH forms of the 16- and 8-bound kernels


@pytest.mark.parametrize("kx,world", SHARDED)
def test_sharded_step_in_process_ranks(kx, world, oracle_factory, monkeypatch):
    """tests/test_gpu_sharded_step.py::test_sharded_step_in_process_ranks (the all-gather form) on a (trunc, kx) pair: bit-equal
    to the unsharded step, and within TOL of the oracle"""
    shardedstep.in_process_ranks(("t30", kx), world, oracle_factory, monkeypatch)


@pytest.mark.parametrize("kx,world", SHARDED)
def test_sharded_step_transposed_in_process_ranks(kx, world, oracle_factory, monkeypatch):
    """The same for the transposed form.  That test's traffic figure -- a rank receives under 0.6 of the all-gather form's bytes
    from four ranks on -- belongs to its equal level blocks: spdy_comm_describe charges the all-gather form the average block and
    the transposed form the rank's own, so with ragged blocks the rank holding an extra level sits higher (6 levels on 4 ranks:
    0.6005 at the ranks with two levels).  Here every rank is held to receiving less than in the all-gather form."""
    shardedstep.transposed_in_process_ranks(("t30", kx), world, oracle_factory, monkeypatch, pays=1.0)
