"""GPU: the full-physics time step -- spdy_physics_dev (one inverse launch + the one-launch column physics,
csrc/spdy_column_chain.hip) from spectra against the oracle's transforms and the chain of restatements (tests/physstep.py); the
one-launch kernel against the five calls bit for bit; a whole time step with the whole physics for three consecutive steps
against oracle_dynamics_step, captured and replayed, and twice from the same inputs."""
import numpy as np
import pytest

import modelstep
import moist
import physstep
import radiation
import surface
import synth
from conftest import TOL, VARIANTS
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from modelstep import PROG

pytestmark = pytest.mark.gpu

TEND = ("utend", "vtend", "ttend", "qtend")


def _plan_case(tag, oracle_factory, levels_case=None):
    """levels_case: (sp, o, half levels, physstep.Case seeds) of a count outside conftest.VARIANTS (tests/levels.py)"""
    if levels_case is None:
        kx = VARIANTS[tag][3]
        sp, o = moist.plan(tag, 4 * kx + 4), oracle_factory(tag)
        case = physstep.Case(tag, sp, o)
    else:
        sp, o, hsg, seeds = levels_case
        kx, case = sp.kx, physstep.Case(tag, sp, o, hsg=hsg, seeds=seeds)
    sp.surface_set_orography(case.phis0)
    return sp, o, case, kx


def _errors(out, exp, errs, label):
    """every optional output against the reference: integers identical; the floats' relative errors into errs"""
    got, want = physstep.flat_outs(out), physstep.flat_outs(exp)
    for n, w in want.items():
        g = got[n].cpu().numpy()[0]
        if g.dtype == np.int32:
            assert np.array_equal(g, w.astype(np.int32)), (label, n)
        else:
            errs["%s %s" % (label, n)] = synth.relerr(g, w)


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_physics_from_spectra(tag, oracle_factory):
    """spdy_physics_dev on a shortwave call and a call without shortwave on the held state: the four tendencies, every optional
    output of every block and the radiation state against the reference within TOL, integers identical.
    Measured on MI355X: worst 4.3e-14 (t30), 8.8e-14 (t63k16) over 68 arrays."""
    check_physics_from_spectra(tag, *_plan_case(tag, oracle_factory))


def check_physics_from_spectra(tag, sp, o, case, kx):
    """the body of test_physics_from_spectra on a plan, its oracle and their physstep.Case; returns the worst (array, error)"""
    import torch
    il, ix = sp.il, sp.ix
    st = case.st
    phi = o.geopotential(st["t"][0], st["phis"])
    spec = [moist.dev(a) for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])]
    bnd = physstep.device_boundary(case.bnd, il, ix)
    S = torch.full((sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    rs, errs = {}, {}
    for step, sw in ((1, True), (2, False)):
        t0 = [synth.splitmix64(70 + 4 * step + i, kx * il * ix).reshape(kx, il, ix) * s for i, s in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
        ref_t = [a.copy() for a in t0]
        r = case.physics(st, sw, rs, *ref_t)
        if step == 1:
            physstep.check_coverage(r, tag)
        assert float(r["margin"].min()) >= physstep.MIN_MARGIN
        T, out = [moist.dev(a) for a in t0], sp.column_outputs(1)
        if sw:
            ssrd = out["rad"]["ssrd"]
        else:                          # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = ssrd
        sp.physics_dev(sw, *spec, bnd, bnd["albsfc"], S, *T, out)
        torch.cuda.synchronize()
        for n, a, b in zip(TEND, T, ref_t):
            errs["step %d %s" % (step, n)] = synth.relerr(a.cpu().numpy(), b)
        exp = physstep.expected(r, kx, il, ix)
        if not sw:                     # written by shortwave calls only: the device leaves them as they were
            for n in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "tt_rsw"):
                exp["rad"].pop(n, None)
        _errors(out, exp, errs, "step %d" % step)
        errs["step %d radiation state" % step] = synth.relerr(S.cpu().numpy().reshape(6 * kx + 7, il * ix),
                                                              physstep.rad_state_array(rs, kx))
    top = sorted(errs.items(), key=lambda kv: -kv[1])
    print("\n[physics from spectra %s] %d arrays, worst %.1e; largest: %s" % (tag, len(errs), top[0][1],
                                                                             ", ".join("%s %.1e" % kv for kv in top[:8])))
    assert top[0][1] <= TOL, top[0]
    sp.close()
    return top[0]


def _gridded(tag, nb, seed, plan=None, keep=None):
    """nb gridded states of surface.columns with the plan that holds their date and orography.  plan: (sp, its half levels) of a
    count outside moist.VARIANTS (tests/levels.py), used in place of the plan of tag.  keep: a dict that receives the reference
    side of the states (tab, zon, sqcoa, and the columns c1, c2 of the two calls)"""
    import torch
    if plan is None:
        ix, il, kx = moist.VARIANTS[tag]
        sp, hsg = moist.plan(tag, 64), moist.HSG[kx]
    else:
        sp, hsg = plan
        ix, il, kx = sp.ix, sp.il, sp.kx
    sp.radiation_set_date(radiation.DATES[0])
    tab = moist.tables(hsg)
    zon = radiation.zonal_columns({n: sp.table(n) for n in physstep.ZON}, nb, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), nb, il, ix)
    c = surface.columns(tab, nb * il * ix, seed, zon, sqcoa)
    ph = c["phis0"].reshape(nb, il * ix)
    ph[:] = ph[0]
    sp.surface_set_orography(ph[0].reshape(il, ix))
    G = lambda a: moist.dev(radiation.grids(a, nb, il, ix))
    c2 = dict(c, tg=c["tg2"], ug=c["vg"], vg=c["ug"], sst=c["sst"] + 0.5, stl=c["stl"] - 0.5, ttend=c["ttend2"])
    names = ("ug", "vg", "tg", "qg", "phig", "pslg", "albsfc") + TEND + surface.BOUNDARY
    if keep is not None:
        keep.update(tab=tab, zon=zon, sqcoa=sqcoa, c1=c, c2=c2)
    return sp, kx, il, ix, {n: G(c[n]) for n in names}, {n: G(c2[n]) for n in names}


def _run_gridded(sp, nb, kx, il, ix, d1, d2, with_out):
    """a shortwave call, then a call without shortwave on the held state; returns everything written, by name"""
    import torch
    S = torch.full((nb * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    res = {"state": S}
    for i, d, sw in ((1, d1, True), (2, d2, False)):
        T = [d[n].clone() for n in TEND]
        out = sp.column_outputs(nb) if with_out else None
        if with_out and i == 2:        # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = res["out1.rad.ssrd"]
        sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], S, *T, out)
        res.update({"%s%d" % (n, i): t for n, t in zip(TEND, T)})
        if with_out:
            res.update({"out%d.%s" % (i, n): t for n, t in physstep.flat_outs(out).items()})
        if i == 1:
            torch.cuda.synchronize()
            res["state1"] = S.clone()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("tag", ["t30", "t30k5", "t30k7", "t63k16"])
def test_one_launch_equals_five_calls(tag, nb):
    """spdy_column_physics_dev with "physics_fused" 1 against 0, a shortwave call followed by a call without shortwave on the
    held state: torch.equal on the tendencies, every requested output and the radiation state; with out = NULL the tendencies
    and the radiation state also equal those of the all-outputs run."""
    import torch
    sp, kx, il, ix, d1, d2 = _gridded(tag, nb, 9800 + nb)
    sp.column_physics_workspace()
    runs = {}
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        for with_out in (True, False):
            runs[fused, with_out] = _run_gridded(sp, nb, kx, il, ix, d1, d2, with_out)
    full = runs[0, True]
    assert len(full) > 60
    for n, v in full.items():
        assert torch.equal(runs[1, True][n], v), ("one launch, all outputs", n)
    for key in ((1, False), (0, False)):
        for n, v in runs[key].items():
            assert torch.equal(v, full[n]), (key, n)
    assert not torch.isnan(full["state"]).any()
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_step_with_whole_physics(tag, oracle_factory):
    """Three consecutive T30 L8 / T63 L16 steps with the whole physics against three oracle_dynamics_step(physics=hook) calls:
    after each step vor, div, t, tr, ps and the PL operands within TOL.  Two runs from the same inputs are bit-equal.  The step
    captured with compute_sw 1 and with 0 and replayed for the three steps is bit-equal to the plain launches, also after a new
    date and new boundary values; with the one-launch kernel the graph has exactly 3 nodes more than the adiabatic step's.
    Measured on MI355X: worst 2.9e-13 (t30, third step), 1.4e-14 (t63k16); nodes 4 -> 7 (t30), 5 -> 8 (t63k16), 12 / 13 as five calls."""
    import torch
    sp, o, case, kx = _plan_case(tag, oracle_factory)
    dt = physstep.DT[tag]
    sp.initialize_implicit(dt); o.tail_init(dt)
    sp.physics_workspace()
    sp.use_own_stream()
    plain_run = lambda D, W, P, sw: modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, sw))
    got, _, _, _ = modelstep.three_steps(sp, case, dt, plain_run)
    # the reference: margins and coverage first, then the comparison
    st, rs, rec, worst = case.st, {}, {}, 0.0
    refs = []
    for step in range(3):
        st, out = oracle_dynamics_step(o, st, 2, dt, ROB, physics=case.hook(step == 0, rs, rec))
        physstep.check_coverage(rec, "%s step %d" % (tag, step + 1))
        refs.append((st, out))
    for step, (st, out) in enumerate(refs):
        w = synth.relerr(got[step]["PL"].cpu().numpy(), out["PL"])
        for n in PROG:
            g = got[step][n].cpu().numpy()
            w = max(w, synth.relerr(g, st[n]), wave_relerr(g, st[n]))
        print("[step %d with the whole physics %s vs oracle] worst %.1e" % (step + 1, tag, w))
        worst = max(worst, w)
    assert worst <= TOL, worst

    # determinism: a second run from the same inputs
    again, _, _, _ = modelstep.three_steps(sp, case, dt, plain_run)
    for step in range(3):
        for n in got[step]:
            assert torch.equal(again[step][n], got[step][n]), ("second run", step, n)

    # captured: one graph with shortwave, one without, replayed for the three steps
    graphs = {}

    def captured_run(D, W, P, sw):
        if sw not in graphs:
            torch.cuda.synchronize()
            with sp.graph_capture() as g:
                plain_run(D, W, P, sw)
            graphs[sw] = g
        graphs[sw].launch()
    cap, D, W, P = modelstep.three_steps(sp, case, dt, captured_run)
    for step in range(3):
        for n in got[step]:
            assert torch.equal(cap[step][n], got[step][n]), ("captured", step, n)
    # a new date and new boundary values between replays: the same graphs against plain launches on the same values
    sp.radiation_set_date(radiation.DATES[1])
    bnd2 = dict(case.bnd, sst=case.bnd["sst"] + 1.25, soilw=case.bnd["soilw"] * 0.5, alb_l=case.bnd["alb_l"] * 0.9)
    for n, v in physstep.device_boundary(bnd2, sp.il, sp.ix).items():
        P["bnd"][n].copy_(v)
    for n in case.st:
        D[n].copy_(moist.dev(case.st[n]))
    P["rad"].fill_(float("nan"))
    torch.cuda.synchronize()
    rep = []
    for step in range(3):
        graphs[step == 0].launch()
        sp.synchronize()
        rep.append(modelstep.snapshot(D, W, P))
    case2 = type("C", (), {"st": case.st, "bnd": bnd2})
    new, _, _, _ = modelstep.three_steps(sp, case2, dt, plain_run)
    changed = 0
    for step in range(3):
        for n in new[step]:
            assert torch.equal(rep[step][n], new[step][n]), ("replayed", step, n)
            changed += int(not torch.equal(rep[step][n], got[step][n]))
    assert changed >= 12                                  # the replays followed the new date and boundary values

    # node counts against the adiabatic step
    D0 = modelstep.device_state(case.st)
    torch.cuda.synchronize()
    with sp.graph_capture() as g0:
        modelstep.step(sp, D0, W, dt)
    n0, n1, n1s = g0.num_nodes(), graphs[False].num_nodes(), graphs[True].num_nodes()
    print("[graph nodes %s] adiabatic %d, whole physics in one launch %d (shortwave %d)" % (tag, n0, n1, n1s))
    assert n1 - n0 == 3 and n1s - n0 == 3, (n0, n1, n1s)
    sp.set_option("physics_fused", 0)
    with sp.graph_capture() as g5:
        plain_run(D0, W, P, True)
    print("[graph nodes %s] whole physics as five calls, shortwave: %d" % (tag, g5.num_nodes()))
    assert g5.num_nodes() - n0 > 3
    # spdy_physics_dev under option 0 against the default, bit for bit
    sp.radiation_set_date(radiation.DATES[0])
    five, _, _, _ = modelstep.three_steps(sp, case, dt, plain_run)
    for step in range(3):
        for n in got[step]:
            assert torch.equal(five[step][n], got[step][n]), ("five calls", step, n)
    for g in (g0, g5, graphs[True], graphs[False]):
        g.close()
    sp.close()
