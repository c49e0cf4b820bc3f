"""GPU: the full-physics time step -- spdy_physics_dev (one inverse launch + the one-launch column physics,
csrc/spdy_column_chain.hip) from spectra against the oracle's transforms and the chain of restatements (tests/physstep.py); the
one-launch kernel against the five calls bit for bit; a whole time step with the whole physics for three consecutive steps
against oracle_dynamics_step, captured and replayed, and twice from the same inputs."""
import pytest

import modelstep
import physstep
import radiation
import support
import synth
from conftest import TOL
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from modelstep import PROG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_physics_from_spectra(tag, oracle_factory):
    """spdy_physics_dev on a shortwave call and a call without shortwave on the held state: the four tendencies, every optional
    output of every block and the radiation state against the reference within TOL, integers identical.
    Measured on MI355X: worst 4.3e-14 (t30), 8.8e-14 (t63k16) over 68 arrays."""
    physstep.check_physics_from_spectra(tag, *physstep.plan_case(tag, oracle_factory))


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("tag", ["t30", "t30k5", "t30k7", "t63k16"])
def test_one_launch_equals_five_calls(tag, nb):
    """spdy_column_physics_dev with "physics_fused" 1 against 0, a shortwave call followed by a call without shortwave on the
    held state: torch.equal on the tendencies, every requested output and the radiation state; with out = NULL the tendencies
    and the radiation state also equal those of the all-outputs run."""
    import torch
    sp, kx, il, ix, d1, d2 = physstep.gridded(tag, nb, 9800 + nb)
    sp.column_physics_workspace()
    runs = {}
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        for with_out in (True, False):
            runs[fused, with_out] = physstep.run_gridded(sp, nb, kx, il, ix, d1, d2, with_out)
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
    sp, o, case, kx = physstep.plan_case(tag, oracle_factory)
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
        D[n].copy_(support.dev(case.st[n]))
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
