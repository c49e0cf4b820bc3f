"""GPU: moist physics on the device (csrc/spdy_physics.hip; physics.f90:110-138) -- against the flang-built reference's
fixture, batch composition, the path from spectra, and a whole time step with the block in it, plain and captured."""
import os

import numpy as np
import pytest

import guards
import modelstep
import moist
import support
import synth
from conftest import GOLDEN, TOL, VARIANTS
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from dynstep import state as dyn_state

pytestmark = pytest.mark.gpu

FLOATS = ("ttend", "qtend", "precnv", "precls", "cbmf", "qsat", "rh", "se")
INTS = ("iptop", "icnv")


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_moist_columns_vs_reference(tag):
    """spdy_moist_columns_dev with every optional output against the reference on the stored sample, and against the restatement
    on EVERY column (array norm and, per column by its own scale, guards.column_err): integers identical, floats within TOL."""
    z = np.load(os.path.join(GOLDEN, "ref_moist.npz"))
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    ins = moist.grid_inputs(tab, (1, il, ix), int(z[tag + "_seed"]))
    sub = z[tag + "_sub"]
    sp = support.plan(tag)
    r = sp.moist_columns(*ins)
    sp.close()
    worst = 0.0
    for n in INTS:
        assert np.array_equal(r[n].reshape(-1, il * ix)[:, sub].squeeze(), z["%s_%s" % (tag, n)]), n
    for n in FLOATS:
        e = synth.relerr(r[n].reshape(-1, il * ix)[:, sub].squeeze(), z["%s_%s" % (tag, n)])
        worst = max(worst, e)
        assert e <= TOL, (n, e)
    want = moist.block(tab, *ins)
    worst_col = 0.0
    for n in INTS:
        assert np.array_equal(r[n].reshape(-1), want[n].reshape(-1)), n
    for n in FLOATS:
        g, w = r[n].reshape(-1, il * ix), want[n].reshape(-1, il * ix)
        e = synth.relerr(g, w)
        assert e <= TOL, (n, "every column", e)
        if n not in ("ttend", "qtend"):      # sums of large terms: by the array norm here, by their operands in test_gpu_thresholds.py
            ec = float(guards.column_err(g, w).max())
            worst_col = max(worst_col, ec)
            assert ec <= TOL, (n, "per column", ec)
    print("[moist columns %s vs restatement, every column] per column worst %.1e" % (tag, worst_col))
    if kx == 5:            # convection.f90:198: the loop do k = kx-3, 3, -1 is empty -- no column convects
        assert np.all(r["icnv"] == -1)
    else:
        assert r["icnv"].max() > 0
    print("\n[moist columns %s vs reference] worst %.1e" % (tag, worst))


def test_null_outputs_and_batch_composition():
    """All optional outputs NULL leaves ttend / qtend bit-equal to the full call; nb = 1, 7, 64 states in one launch are each
    bit-equal to the same state launched alone."""
    import torch
    sp = support.plan("t30", 64)
    ix, il, kx = support.grid("t30")
    tab = moist.tables(moist.HSG[kx])
    for nb in (1, 7, 64):
        tg, qg, phig, pslg, tt, qt = (support.dev(a) for a in moist.grid_inputs(tab, (nb, il, ix), 9100 + nb))
        T, Q, out = tt.clone(), qt.clone(), sp.column_outputs(nb, "moist")
        sp.moist_columns_dev(tg, qg, phig, pslg, T, Q, out)
        T0, Q0 = tt.clone(), qt.clone()
        sp.moist_columns_dev(tg, qg, phig, pslg, T0, Q0, None)
        torch.cuda.synchronize()
        assert torch.equal(T, T0) and torch.equal(Q, Q0), nb
        for b in range(nb):
            Tb, Qb, ob = tt[b:b + 1].clone(), qt[b:b + 1].clone(), sp.column_outputs(1, "moist")
            sp.moist_columns_dev(tg[b:b + 1], qg[b:b + 1], phig[b:b + 1], pslg[b:b + 1], Tb, Qb, ob)
            torch.cuda.synchronize()
            assert torch.equal(Tb[0], T[b]) and torch.equal(Qb[0], Q[b]), (nb, b)
            for n in ob:
                assert torch.equal(ob[n][0], out[n][b]), (nb, b, n)
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_moist_physics_from_spectra(tag, oracle_factory):
    """spdy_moist_physics_dev (one inverse launch + the column kernel) against the restatement on the oracle's transforms."""
    import torch
    kx = support.grid(tag)[2]
    sp, o = support.plan(tag, 4 * kx + 4), oracle_factory(tag)
    st = moist.state(o, dyn_state(sp, 8000), 4242)
    phi = o.geopotential(st["t"][0], st["phis"])
    il, ix = sp.il, sp.ix
    tt0 = synth.splitmix64(77, kx * il * ix).reshape(kx, il, ix) * 1e-4
    qt0 = synth.splitmix64(78, kx * il * ix).reshape(kx, il, ix) * 1e-7
    rec = {}
    tt, qt = tt0.copy(), qt0.copy()
    moist.make_hook(rec)(o, st, None, None, tt, qt)
    assert rec["margin"].min() >= moist.MIN_MARGIN
    T, Q, out = support.dev(tt0), support.dev(qt0), sp.column_outputs(1, "moist")
    sp.moist_physics_dev(support.dev(st["t"][0]), support.dev(st["tr"][0]), support.dev(phi), support.dev(st["ps"][0]), T, Q, out)
    torch.cuda.synchronize()
    worst = max(synth.relerr(T.cpu().numpy(), tt), synth.relerr(Q.cpu().numpy(), qt))
    for n in ("precnv", "precls", "cbmf", "qsat", "rh", "se"):
        worst = max(worst, synth.relerr(out[n].cpu().numpy()[0], rec[n]))
    for n in INTS:
        assert np.array_equal(out[n].cpu().numpy()[0], rec[n]), n
    print("\n[moist physics from spectra %s] worst %.1e, min margin %.1e" % (tag, worst, rec["margin"].min()))
    assert worst <= TOL
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_step_with_moist_physics(tag, oracle_factory):
    """A whole T30 L8 / T63 L16 step with the moist block between the grid tendencies and the direct batch against
    oracle_dynamics_step(physics=moist hook) within TOL; the same step captured and replayed is bit-equal to the plain launches,
    and its graph has exactly 3 nodes more than the adiabatic step's (geopotential, the inverse launch, the column kernel)."""
    import torch
    kx = VARIANTS[tag][3]
    sp, o = support.plan(tag, 4 * kx + 4), oracle_factory(tag)
    dt = 2400.0
    sp.initialize_implicit(dt); o.tail_init(dt)
    st = moist.state(o, dyn_state(sp, 8000), 5150)
    W = modelstep.Workspace(sp)
    fresh = lambda: modelstep.device_state(st)
    sp.moist_workspace()
    sp.use_own_stream()
    # plain launches
    D = fresh()
    modelstep.step(sp, D, W, dt, physics=modelstep.moist_physics())
    sp.synchronize()
    plain = {n: D[n].clone() for n in ("vor", "div", "t", "tr", "ps")}
    PLd = W.PL.cpu().numpy()
    rec = {}
    ref, out = oracle_dynamics_step(o, st, 2, dt, ROB, physics=moist.make_hook(rec))
    assert rec["margin"].min() >= moist.MIN_MARGIN
    assert rec["branch"]["no_conv"] < rec["branch"]["columns"] and rec["branch"]["lsc_interior"] > 0
    worst = synth.relerr(PLd, out["PL"])
    for n in ("ps", "vor", "div", "t", "tr"):
        got = plain[n].cpu().numpy()
        worst = max(worst, synth.relerr(got, ref[n]), wave_relerr(got, ref[n]))
    print("\n[step with moist physics %s vs oracle] worst %.1e; branches %s" % (tag, worst, rec["branch"]))
    assert worst <= TOL, worst
    # captured and replayed: bit-equal
    D = fresh()
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        modelstep.step(sp, D, W, dt, physics=modelstep.moist_physics())
    g.launch()
    sp.synchronize()
    for n in plain:
        assert torch.equal(D[n], plain[n]), n
    D0 = fresh()
    torch.cuda.synchronize()
    with sp.graph_capture() as g0:
        modelstep.step(sp, D0, W, dt)
    n1, n0 = g.num_nodes(), g0.num_nodes()
    print("[graph nodes %s] adiabatic %d, with moist physics %d" % (tag, n0, n1))
    assert n1 - n0 == 3, (n0, n1)
    g.close(); g0.close(); sp.close()
