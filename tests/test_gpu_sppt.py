"""GPU: SPPT on the device -- the pattern object (spdy_sppt_*: the counter-based noise, the AR(1) update, the plan's inverse
transform, the clip) against the restatement tests/sppt.py, its application to the tendencies (spdy_physics_sppt_dev,
spdy_column_physics_sppt_dev) bit for bit against the formula on the results without SPPT and in both forms of the chain, the
captured {advance; physics} replayed, and three consecutive time steps with SPPT against oracle_dynamics_step."""
import numpy as np
import pytest

import modelstep
import physstep
import sppt
import support
import synth
from conftest import TOL, VARIANTS
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from modelstep import PROG
from physstep import TEND

pytestmark = pytest.mark.gpu

TAGS = ["t30", "t63k16"]
SEED = 0x5EED0123456789AB
FIELDS = ("eta", "spec", "pattern")


def _shape(sp):
    return (sp.kx, sp.nx, sp.mx)


@pytest.mark.parametrize("tag", TAGS)
def test_noise(tag):
    """Two drawn advances: eta against the restated generator within TOL; a second object with the same seed gives the same bits,
    another seed does not; reset reproduces the first run; draws counts the advances."""
    import speedy_f90_amd as s
    sp = support.plan(tag, 4 * VARIANTS[tag][3] + 4)
    a, b, c = s.Sppt(sp, 36, seed=SEED), s.Sppt(sp, 36, seed=SEED), s.Sppt(sp, 36, seed=SEED + 1)
    assert a.draws() == 0
    first = []
    for d in range(2):
        for x in (a, b, c):
            x.advance_dev()
        got, want = a.numpy("eta"), sppt.noise(SEED, d, _shape(sp))
        e = synth.relerr(got, want)
        print("[sppt noise %s] draw %d: eta vs restatement %.1e, std %.4f" % (tag, d, e, got.real.std()))
        assert e <= TOL
        assert np.abs(got.real).max() <= 10.0 and np.abs(got.imag).max() <= 10.0
        first.append({n: a.numpy(n) for n in FIELDS})
        for n in FIELDS:
            assert np.array_equal(b.numpy(n), first[d][n]), (d, n)
            assert not np.array_equal(c.numpy(n), first[d][n]), (d, n)
        assert np.abs(first[d]["pattern"]).max() <= 1.0
    assert not np.array_equal(first[0]["eta"], first[1]["eta"])
    assert a.draws() == 2 and b.draws() == 2
    a.reset(SEED)
    assert a.draws() == 0
    for d in range(2):
        a.advance_dev()
        for n in FIELDS:
            assert np.array_equal(a.numpy(n), first[d][n]), ("after reset", d, n)
    c.reset(SEED)                      # another object, other history: the same stream once the seed is the same
    c.advance_dev()
    assert np.array_equal(c.numpy("pattern"), first[0]["pattern"])
    sp.close()


@pytest.mark.parametrize("tag", TAGS)
def test_ar1_transform_clip(tag, oracle_factory):
    """Three advances on injected noise, scaled so that the clip to +-1 is at work (and the clip to +-10 too): spec and pattern
    against the restatement after each; |pattern| <= 1 exactly; draws counts injected advances too."""
    import speedy_f90_amd as s
    sp, o = support.plan(tag, 4 * VARIANTS[tag][3] + 4), oracle_factory(tag)
    pat, ref = s.Sppt(sp, 36, seed=1), sppt.Pattern(o)
    worst = 0.0
    for d in range(3):
        eta = 4.0 * sppt.raw_noise(SEED + 7, d, int(np.prod(_shape(sp)))).reshape(_shape(sp))
        assert np.abs(eta.real).max() > 10.0                                    # the first clip has work to do
        want = ref.advance(eta)
        frac = float((np.abs(ref.grid) > 1.0).mean())
        assert 0.01 <= frac <= 0.99, frac
        pat.advance_dev(support.dev(eta))
        got = pat.numpy("pattern")
        es, ep = synth.relerr(pat.numpy("spec"), ref.spec), synth.relerr(got, want)
        print("[sppt AR(1) %s] advance %d: spec %.1e, pattern %.1e, clipped %.1f %%" % (tag, d, es, ep, 100 * frac))
        worst = max(worst, es, ep)
        assert np.abs(got).max() == 1.0
    assert worst <= TOL, worst
    assert pat.draws() == 3
    sp.close()


def _physics_inputs(sp, o, case, kx):
    st = case.st
    phi = o.geopotential(st["t"][0], st["phis"])
    spec = [support.dev(a) for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])]
    bnd = physstep.device_boundary(case.bnd, sp.il, sp.ix)
    t0 = [synth.splitmix64(170 + i, kx * sp.il * sp.ix).reshape(kx, sp.il, sp.ix) * f for i, f in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
    return spec, bnd, t0


def _nan_state(sp, nb=1):
    import torch
    return torch.full((nb * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("tag", TAGS)
def test_application_from_spectra(tag, oracle_factory):
    """spdy_physics_sppt_dev equals the formula of physics.f90:212-221 evaluated in NumPy on spdy_physics_dev's own result and the
    entry values, bit for bit, in both forms of the chain; every optional output and the radiation state are those of the call
    without SPPT; the pattern object is not advanced."""
    import torch
    import speedy_f90_amd as s
    sp, o, case, kx = physstep.plan_case(tag, oracle_factory)
    spec, bnd, t0 = _physics_inputs(sp, o, case, kx)
    mu = sppt.mu(kx)
    pat = s.Sppt(sp, 36, mu, seed=SEED)
    pat.advance_dev()
    P = pat.numpy("pattern")
    assert P.std() > 0.05
    T, out, S = [support.dev(a) for a in t0], sp.column_outputs(1), _nan_state(sp)
    sp.physics_dev(True, *spec, bnd, bnd["albsfc"], S, *T, out)
    torch.cuda.synchronize()
    want = [sppt.apply(t.cpu().numpy(), d, P, mu) for t, d in zip(T, t0)]
    assert all(not np.array_equal(w, t.cpu().numpy()) for w, t in zip(want[2:], T[2:]))
    plain = physstep.flat_outs(out)
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        T2, out2, S2 = [support.dev(a) for a in t0], sp.column_outputs(1), _nan_state(sp)
        sp.physics_sppt_dev(pat, True, *spec, bnd, bnd["albsfc"], S2, *T2, out2)
        torch.cuda.synchronize()
        for n, t, w in zip(TEND, T2, want):
            assert np.array_equal(t.cpu().numpy(), w), (fused, n, synth.relerr(t.cpu().numpy(), w))
        for n, t in physstep.flat_outs(out2).items():
            assert torch.equal(t, plain[n]), (fused, n)
        assert torch.equal(S2, S) and not torch.isnan(S2).any()
    assert pat.draws() == 1 and np.array_equal(pat.numpy("pattern"), P)
    sp.close()


@pytest.mark.parametrize("tag", TAGS)
def test_application_on_gridded_states(tag):
    """spdy_column_physics_sppt_dev on three states with three different patterns and out = NULL, in both forms: the formula on
    spdy_column_physics_dev's result, bit for bit; a NULL mu is all ones."""
    import torch
    import speedy_f90_amd as s
    nb = 3
    sp, kx, il, ix, d, _ = physstep.gridded(tag, nb, 9950)
    pat = s.Sppt(sp, 36, seed=SEED + 3)
    pats = []
    for _ in range(nb):
        pat.advance_dev()
        pats.append(pat.numpy("pattern"))
    P = np.stack(pats)
    assert not np.array_equal(P[0], P[1]) and not np.array_equal(P[1], P[2])
    dP = support.dev(P)
    sp.column_physics_sppt_workspace()
    args = lambda T, S: (True, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], S, *T)
    T0 = [d[n].cpu().numpy() for n in TEND]
    T, S = [d[n].clone() for n in TEND], _nan_state(sp, nb)
    sp.column_physics_dev(*args(T, S))
    torch.cuda.synchronize()
    for mu in (sppt.mu(kx), None):
        m = np.ones(kx) if mu is None else mu
        want = [np.stack([sppt.apply(t.cpu().numpy()[b], t0[b], P[b], m) for b in range(nb)]) for t, t0 in zip(T, T0)]
        for fused in (1, 0):
            sp.set_option("physics_fused", fused)
            T2, S2 = [d[n].clone() for n in TEND], _nan_state(sp, nb)
            sp.column_physics_sppt_dev(dP, mu, *args(T2, S2))
            torch.cuda.synchronize()
            for n, t, w in zip(TEND, T2, want):
                assert np.array_equal(t.cpu().numpy(), w), (fused, n, mu is None)
            assert torch.equal(S2, S)
    sp.close()


@pytest.mark.parametrize("tag", TAGS)
def test_captured_advance_and_physics(tag, oracle_factory):
    """{advance_dev(NULL); physics_sppt_dev} captured once and replayed three times equals three eager rounds on a second object
    with the same seed, bit for bit: the first-step branch and the counter are read on the device.  Node counts: the advance is
    3 nodes; the one-launch physics with SPPT adds none to spdy_physics_dev's graph, the five calls add their save and apply."""
    import torch
    import speedy_f90_amd as s
    sp, o, case, kx = physstep.plan_case(tag, oracle_factory)
    spec, bnd, t0 = _physics_inputs(sp, o, case, kx)
    mu = sppt.mu(kx)
    sp.physics_sppt_workspace()
    sp.use_own_stream()
    a, b = s.Sppt(sp, 36, mu, seed=SEED), s.Sppt(sp, 36, mu, seed=SEED)

    def rounds(step):
        T, S, after = [support.dev(x) for x in t0], _nan_state(sp), []
        torch.cuda.synchronize()
        for _ in range(3):
            step(T, S)
            sp.synchronize()
            after.append([t.clone() for t in T] + [S.clone()])
        return T, S, after

    def eager(T, S):
        b.advance_dev()
        sp.physics_sppt_dev(b, True, *spec, bnd, bnd["albsfc"], S, *T)
    _, _, want = rounds(eager)
    graphs = []

    def replay(T, S):
        if not graphs:
            with sp.graph_capture() as g:
                a.advance_dev()
                sp.physics_sppt_dev(a, True, *spec, bnd, bnd["albsfc"], S, *T)
            graphs.append(g)
        graphs[0].launch()
    T, S, got = rounds(replay)
    for r in range(3):
        for x, y in zip(got[r], want[r]):
            assert torch.equal(x, y), r
    assert not torch.equal(got[0][2], got[1][2])
    assert a.draws() == 3 and b.draws() == 3
    for n in FIELDS:
        assert np.array_equal(a.numpy(n), b.numpy(n)), n

    def nodes(body):
        with sp.graph_capture() as g:
            body()
        n = g.num_nodes()
        g.close()
        return n
    plain = lambda: sp.physics_dev(True, *spec, bnd, bnd["albsfc"], S, *T)
    with_sppt = lambda: (a.advance_dev(), sp.physics_sppt_dev(a, True, *spec, bnd, bnd["albsfc"], S, *T))
    n_adv, n1, n1s = nodes(a.advance_dev), nodes(plain), nodes(with_sppt)
    sp.set_option("physics_fused", 0)
    n5, n5s = nodes(plain), nodes(with_sppt)
    print("[sppt graph nodes %s] advance %d; physics in one launch %d, with SPPT %d; as five calls %d, with SPPT %d"
          % (tag, n_adv, n1, n1s, n5, n5s))
    assert n_adv == 3 and n1s == n1 + n_adv and n5s == n5 + n_adv + 2, (n_adv, n1, n1s, n5, n5s)
    assert graphs[0].num_nodes() == n1s
    graphs[0].close()
    sp.close()


@pytest.mark.parametrize("tag", TAGS)
def test_three_steps_with_sppt(tag, oracle_factory):
    """The three-step case of tests/test_gpu_physics_step.py with SPPT on every step (noise drawn on the device) against
    oracle_dynamics_step with a physics hook that applies the restated pattern: vor, div, t, tr, ps and the PL operands within TOL
    after each step.  With the advance left out on the second step the error is far over the bar: the test sees the pattern."""
    import speedy_f90_amd as s
    sp, o, case, kx = physstep.plan_case(tag, oracle_factory)
    dt, mu = physstep.DT[tag], sppt.mu(kx)
    sp.initialize_implicit(dt); o.tail_init(dt)
    sp.physics_sppt_workspace()
    sp.use_own_stream()
    pat = s.Sppt(sp, 36, mu, seed=SEED)
    sppt_step = lambda D, W, P, sw, advance=True: modelstep.step(sp, D, W, dt, physics=modelstep.sppt_physics(P, sw, pat, advance))
    got, _, _, _ = modelstep.three_steps(sp, case, dt, sppt_step)
    assert pat.draws() == 3
    ref = sppt.Pattern(o)
    st, rs, rec, refs = case.st, {}, {}, []
    for step in range(3):
        inner = case.hook(step == 0, rs, rec)

        def hook(o_, st_, ut, vt, tt, qt, step=step, inner=inner):
            dyn = [x.copy() for x in (ut, vt, tt, qt)]
            inner(o_, st_, ut, vt, tt, qt)
            p = ref.advance(sppt.noise(SEED, step, _shape(sp)))
            for x, d in zip((ut, vt, tt, qt), dyn):
                x[...] = sppt.apply(x, d, p, mu)
        st, out = oracle_dynamics_step(o, st, 2, dt, ROB, physics=hook)
        physstep.check_coverage(rec, "%s step %d with SPPT" % (tag, step + 1))
        refs.append((st, out))

    def worst_of(run):
        worst = 0.0
        for step, (st, out) in enumerate(refs):
            w = synth.relerr(run[step]["PL"].cpu().numpy(), out["PL"])
            for n in PROG:
                g = run[step][n].cpu().numpy()
                w = max(w, synth.relerr(g, st[n]), wave_relerr(g, st[n]))
            worst = max(worst, w)
        return worst
    worst = worst_of(got)
    print("[three steps with SPPT %s vs oracle] worst %.1e" % (tag, worst))
    assert worst <= TOL, worst
    # the same with the second step's advance left out: its pattern is the first step's
    pat.reset(SEED)
    count = [0]

    def skipping(D, W, P, sw):
        count[0] += 1
        sppt_step(D, W, P, sw, advance=count[0] != 2)
    bad = worst_of(modelstep.three_steps(sp, case, dt, skipping)[0])
    print("[three steps with SPPT %s, advance skipped on step 2] worst %.1e" % (tag, bad))
    assert bad > TOL, bad
    sp.close()
