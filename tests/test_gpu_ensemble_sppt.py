"""GPU: SPPT for an ensemble (include/spdy.h "SPPT", the ensemble form): a pattern object of E members whose ONE
advance gives every member the bits of a single object with that member's seed, whichever branch each member is in and whatever
its neighbours hold; spdy_ens_physics_sppt_dev against the single-state call per member and against the formula; the captured
Ensemble.step with physics["sppt"]; the error codes that need a device."""
import ctypes

import numpy as np
import pytest

import ensemblesppt as esp
import ensemblestep as es
import physstep
import sppt
import support
import synth
from conftest import TOL
from dynstep import ROB
from ensemblesppt import FIELDS, NSTEPS, SEED

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -5
TEND = ("utend", "vtend", "ttend", "qtend")


# ---------------------------------------------------------------------------------------------- 1. member equals single
@pytest.mark.parametrize("tag,E,nadv", [("t30", 3, 3), ("t30", 17, 1), ("t30k5", 2, 1)])
def test_member_equals_single(tag, E, nadv):
    """Drawn advances (the first branch once, then the AR(1) branch): after each, every member's eta, spec and pattern are bit-equal
    to a single object with that member's seed, and draws counts per member.  Member 0's eta is held to the restated generator, so
    both sides cannot be wrong together.  E = 17: 136 fields push the inverse launch out of the model-sized form.  Two members with
    the same seed are bit-equal to each other, wherever they sit."""
    import speedy_f90_amd as s
    sp = support.ensemble_plan(tag, E)
    sd = esp.seeds(E)
    pat, one = s.Sppt(sp, NSTEPS, seeds=sd), esp.singles(sp, sd)
    assert pat.members() == E and all(pat.draws(e) == 0 for e in range(E))
    first = None
    for d in range(nadv):
        pat.advance_dev()
        got = esp.fields(pat)
        assert got["eta"].shape == (E,) + esp.shape(sp) and got["pattern"].shape == (E, sp.kx) + sp.grid_shape
        for e in range(E):
            one[e].advance_dev()
            assert esp.differing(got, e, one[e]) == [], (tag, E, d, e)
            assert pat.draws(e) == d + 1
        err = synth.relerr(got["eta"][0], sppt.noise(sd[0], d, esp.shape(sp)))
        print("[ensemble sppt %s E=%d] draw %d: member 0's eta vs restatement %.1e" % (tag, E, d, err))
        assert err <= TOL
        assert not np.array_equal(got["eta"][0], got["eta"][1])
        assert np.abs(got["pattern"]).max() <= 1.0
        first = got if first is None else first
    if E == 3:
        twin = s.Sppt(sp, NSTEPS, seeds=[sd[1], sd[1], sd[0]])
        twin.advance_dev()
        got = esp.fields(twin)
        for n in FIELDS:
            assert support.same_bits(got[n][0], got[n][1]), n
            assert support.same_bits(got[n][0], first[n][1]) and support.same_bits(got[n][2], first[n][0]), n
    sp.close()


# ---------------------------------------------------------------------------------------------- 2. injected noise, both clips
def test_injected_noise_with_both_clips(oracle_factory):
    """E = 2, three advances on injected noise scaled as tests/test_gpu_sppt.py::test_ar1_transform_clip scales it, different per
    member: spec and pattern of each member against the restatement on the oracle; |pattern| <= 1 exactly."""
    import speedy_f90_amd as s
    E = 2
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    pat, ref = s.Sppt(sp, NSTEPS, seeds=[1, 2]), [sppt.Pattern(o) for _ in range(E)]
    worst = 0.0
    for d in range(3):
        eta = esp.injected(E, d, esp.shape(sp))
        assert np.abs(eta.real).max(axis=(1, 2, 3)).min() > 10.0                    # the first clip has work to do in every member
        pat.advance_dev(support.dev(eta))
        got = esp.fields(pat)
        for e in range(E):
            want = ref[e].advance(eta[e])
            frac = float((np.abs(ref[e].grid) > 1.0).mean())
            assert 0.01 <= frac <= 0.99, frac
            es_, ep = synth.relerr(got["spec"][e], ref[e].spec), synth.relerr(got["pattern"][e], want)
            print("[ensemble sppt AR(1)] advance %d member %d: spec %.1e, pattern %.1e, clipped %.1f %%" % (d, e, es_, ep, 100 * frac))
            worst = max(worst, es_, ep)
            assert np.abs(got["pattern"][e]).max() == 1.0
        assert not np.array_equal(got["pattern"][0], got["pattern"][1])
    assert worst <= TOL, worst
    assert [pat.draws(e) for e in range(E)] == [3, 3]
    sp.close()


# ---------------------------------------------------------------------------------------------- 3. mixed branches in one launch
def test_mixed_branches_in_one_launch():
    """E = 3: after three advances member 1 is reset to another seed and the object advanced once more.  That launch takes the
    first-draw branch for member 1 -- bit-equal to a single object's first advance with the new seed -- and the AR(1) branch for
    members 0 and 2 -- bit-equal to the fourth advance of a run without the reset.  Draws are (4, 1, 4)."""
    import speedy_f90_amd as s
    E, other = 3, SEED ^ 0xABCDEF
    sp = support.ensemble_plan("t30", E)
    sd = esp.seeds(E)
    pat, plain, one = s.Sppt(sp, NSTEPS, seeds=sd), s.Sppt(sp, NSTEPS, seeds=sd), s.Sppt(sp, NSTEPS, seed=other)
    for _ in range(3):
        pat.advance_dev(); plain.advance_dev()
    before = esp.fields(pat)
    pat.reset(other, member=1)
    assert [pat.draws(e) for e in range(E)] == [3, 0, 3]
    for n in FIELDS:                                               # the reset touches the counter and the seed, nothing else
        assert support.same_bits(esp.fields(pat)[n], before[n]), n
    pat.advance_dev(); plain.advance_dev(); one.advance_dev()
    got, want = esp.fields(pat), esp.fields(plain)
    for e in (0, 2):
        for n in FIELDS:
            assert support.same_bits(got[n][e], want[n][e]), (e, n)
    assert esp.differing(got, 1, one) == []
    assert not np.array_equal(got["spec"][1], want["spec"][1])
    assert [pat.draws(e) for e in range(E)] == [4, 1, 4] and [plain.draws(e) for e in range(E)] == [4, 4, 4]
    sp.close()


# ---------------------------------------------------------------------------------------------- 4. isolation
def test_isolation():
    """E = 3, injected eta with NaN and both infinities in member 1 only: members 0 and 2 -- eta, spec, pattern, draws -- are
    bit-equal to the same run with finite values there, on that advance and on the drawn advance that follows."""
    import speedy_f90_amd as s
    E = 3
    sp = support.ensemble_plan("t30", E)
    sd, kx = esp.seeds(E), sp.kx
    clean, bad = s.Sppt(sp, NSTEPS, seeds=sd), s.Sppt(sp, NSTEPS, seeds=sd)
    eta = esp.injected(E, 0, esp.shape(sp))
    dirty = eta.copy()
    dirty[1, :kx // 2] = complex(float("nan"), float("nan"))
    dirty[1, kx // 2:] = complex(float("inf"), -float("inf"))
    for step, (a, b) in enumerate(((eta, dirty), (None, None))):
        clean.advance_dev(None if a is None else support.dev(a))
        bad.advance_dev(None if b is None else support.dev(b))
        got, want = esp.fields(bad), esp.fields(clean)
        for e in (0, 2):
            for n in FIELDS:
                assert support.same_bits(got[n][e], want[n][e]), (step, e, n)
            assert bad.draws(e) == clean.draws(e) == step + 1
        assert np.isfinite(want["pattern"]).all()
        assert not support.same_bits(got["spec"][1], want["spec"][1]), step          # the poison was there
    assert bad.draws(1) == 2
    sp.close()


# ---------------------------------------------------------------------------------------------- 5. the application
def _spectra(o, sts):
    """time level 1 of the members as the ensemble call takes it: vor, div, t, q, phi [E, kx, nx, mx], ps [E, nx, mx]"""
    phi = [o.geopotential(st["t"][0], st["phis"]) for st in sts]
    lev = [np.stack([st[n][0] for st in sts]) for n in ("vor", "div", "t", "tr")]
    return lev + [np.stack(phi), np.stack([st["ps"][0] for st in sts])]


def _nan_state(sp, nb):
    import torch
    return torch.full((nb * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("tag,E,forms", [("t30", 3, (1, 0)), ("t30k5", 2, (1,))])
def test_application(tag, E, forms, oracle_factory):
    """Members with different states, boundary fields and patterns.  Each member's utend, vtend, ttend, qtend, its radiation state
    and every optional output from ens_physics_sppt_dev are bit-equal to physics_sppt_dev on that member's state with a single
    object of that member's seed, in both forms of the chain.  Member 0 is anchored: its tendencies equal physics.f90:212-221
    evaluated in NumPy on ens_physics_dev's own result and the entry tendencies."""
    import torch
    import speedy_f90_amd as s
    sp, o = support.ensemble_plan(tag, E), oracle_factory(tag)
    kx, size = sp.kx, sp.radiation_state_size()
    sts, bnds = es.physics_members(sp, o, E)
    spec = _spectra(o, sts)
    dspec = [support.dev(a) for a in spec]
    P = es.ens_physics(sp, bnds)
    t0 = [synth.splitmix64(170 + i, E * kx * sp.il * sp.ix).reshape((E, kx) + sp.grid_shape) * f
          for i, f in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
    sd, mu = esp.seeds(E), esp.mu(kx)
    pat, one = s.Sppt(sp, NSTEPS, mu, seeds=sd), esp.singles(sp, sd, mu)
    pat.advance_dev()
    for x in one:
        x.advance_dev()
    pattern = pat.numpy("pattern")
    assert pattern.std() > 0.05 and not np.array_equal(pattern[0], pattern[1])
    # without SPPT, for the anchor
    T, S = [support.dev(a) for a in t0], _nan_state(sp, E)
    sp.ens_physics_dev(E, True, *dspec, P["bnd"], P["albsfc"], S, *T)
    torch.cuda.synchronize()
    anchor = [sppt.apply(t.cpu().numpy()[0], d[0], pattern[0], mu) for t, d in zip(T, t0)]
    assert all(not np.array_equal(w, t.cpu().numpy()[0]) for w, t in zip(anchor[2:], T[2:]))
    for fused in forms:
        sp.set_option("physics_fused", fused)
        T2, out2, S2 = [support.dev(a) for a in t0], sp.column_outputs(E), _nan_state(sp, E)
        sp.ens_physics_sppt_dev(E, pat, True, *dspec, P["bnd"], P["albsfc"], S2, *T2, out2)
        torch.cuda.synchronize()
        for n, t, w in zip(TEND, T2, anchor):
            assert np.array_equal(t.cpu().numpy()[0], w), (fused, n, "anchor")
        assert support.same_bits(S2, S) and not torch.isnan(S2).any()
        flat2 = physstep.flat_outs(out2)
        for e in range(E):
            bnd = physstep.device_boundary(bnds[e], sp.il, sp.ix)
            T1, out1, S1 = [support.dev(a[e]) for a in t0], sp.column_outputs(1), _nan_state(sp, 1)
            sp.physics_sppt_dev(one[e], True, *[support.dev(a[e]) for a in spec], bnd, bnd["albsfc"], S1, *T1, out1)
            torch.cuda.synchronize()
            for n, t2, t1 in zip(TEND, T2, T1):
                assert support.same_bits(t2[e], t1), (fused, e, n)
            assert support.same_bits(S2[e * size:(e + 1) * size], S1), (fused, e, "radiation state")
            for n, t1 in physstep.flat_outs(out1).items():
                assert support.same_bits(flat2[n][e], t1[0]), (fused, e, n)
    assert [pat.draws(e) for e in range(E)] == [1] * E and np.array_equal(pat.numpy("pattern"), pattern)      # not advanced
    sp.close()


# ---------------------------------------------------------------------------------------------- 6. the captured step
def _nodes(sp, body):
    with sp.graph_capture() as g:
        body()
    n = g.num_nodes()
    g.close()
    return n


def test_captured_step(oracle_factory):
    """E = 2: {Ensemble.step with physics["sppt"]} captured once and replayed three times gives the bits of three eager steps from
    the same start, prognostics, operands, radiation states and patterns.  The same eager run with the advance left out of the
    second step differs: the comparison sees the pattern.  In the fused form ens_physics_sppt_dev has exactly the nodes of
    ens_physics_dev, so the captured step has the advance's three more than the step without SPPT."""
    import torch
    import speedy_f90_amd as s
    E, dt = 2, physstep.DT["t30"]
    sp, o = support.ensemble_plan("t30", E), oracle_factory("t30")
    sts, bnds = es.physics_members(sp, o, E)
    sp.initialize_implicit(dt)
    sp.use_own_stream()
    sd, mu = esp.seeds(E), esp.mu(sp.kx)

    def start():
        return es.build(sp, sts), es.ens_physics(sp, bnds), s.Sppt(sp, NSTEPS, mu, seeds=sd)

    def snap(ens, P, pat):
        sp.synchronize()
        return dict(es.snapshot(ens), rad=P["rad"].clone(), **{n: torch.from_numpy(v.copy()) for n, v in esp.fields(pat).items()})

    def eager(skip=None):
        ens, P, pat = start()
        out = []
        for n in range(3):
            ens.step(2, 2, dt, dict(P, sw=True, sppt=esp.NoAdvance(pat) if n == skip else pat), eps=ROB)
            out.append(snap(ens, P, pat))
        return out, [pat.draws(e) for e in range(E)]

    want, draws = eager()
    assert draws == [3, 3]
    ens, P, pat = start()
    ens.physics_workspace(sppt=True)
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        ens.step(2, 2, dt, dict(P, sw=True, sppt=pat), eps=ROB)
    assert [pat.draws(e) for e in range(E)] == [0, 0]                      # a capture runs nothing
    for n in range(3):
        g.launch()
        got = snap(ens, P, pat)
        bad = [k for k in got if not support.same_bits(got[k], want[n][k])]
        assert bad == [], (n, bad)
    assert [pat.draws(e) for e in range(E)] == [3, 3]
    assert np.isfinite(want[-1]["vor"][:, 0].cpu().numpy()).all()
    skipped, draws = eager(skip=1)
    assert draws == [2, 2]
    assert support.same_bits(skipped[0]["vor"], want[0]["vor"]) and not support.same_bits(skipped[1]["vor"], want[1]["vor"])
    assert not support.same_bits(skipped[2]["pattern"], want[2]["pattern"])
    # node counts
    n_step = g.num_nodes()
    n_plain = _nodes(sp, lambda: ens.step(2, 2, dt, dict(P, sw=True), eps=ROB))
    args = (True, ens.vor[0], ens.div[0], ens.t[0], ens.tr[0], ens.phim, ens.ps[0], P["bnd"], P["albsfc"], P["rad"], ens.utend, ens.vtend,
            ens.ttend, ens.qtend)
    n_phys, n_phys_sppt = _nodes(sp, lambda: sp.ens_physics_dev(E, *args)), _nodes(sp, lambda: sp.ens_physics_sppt_dev(E, pat, *args))
    n_adv = _nodes(sp, pat.advance_dev)
    print("[ensemble sppt graph nodes] step %d, with SPPT %d; physics %d, with SPPT %d; advance %d" % (n_plain, n_step, n_phys, n_phys_sppt,
                                                                                                    n_adv))
    assert n_adv == 3 and n_phys_sppt == n_phys and n_step == n_plain + n_adv, (n_adv, n_phys, n_phys_sppt, n_plain, n_step)
    g.close()
    sp.close()


def test_advance_is_three_nodes_whatever_the_members():
    """the captured advance of E = 1, 2 and 17 members: noise, ONE inverse launch, clip"""
    import speedy_f90_amd as s
    sp = support.ensemble_plan("t30", 17)
    sp.use_own_stream()
    for E in (1, 2, 17):
        pat = s.Sppt(sp, NSTEPS, nmem=E, seed=SEED)
        assert _nodes(sp, pat.advance_dev) == 3, E
        pat.close()
    sp.close()


# ---------------------------------------------------------------------------------------------- 7. T63 L16
def test_t63_member_equals_single(oracle_factory):
    """T63 L16, E = 2, two drawn advances.  Eta is bit-equal to the single objects: no transform lies in front of it.  Spec and
    pattern are held to the restatement within TOL; at T63 a field's bits may depend on the launch form
    (tests/test_gpu_ensemble.py::test_t63_member_equals_single), so their bit equality to the single objects is printed, not
    required."""
    import speedy_f90_amd as s
    E = 2
    sp, o = support.ensemble_plan("t63k16", E), oracle_factory("t63k16")
    sd = esp.seeds(E)
    pat, one, ref = s.Sppt(sp, NSTEPS, seeds=sd), esp.singles(sp, sd), [sppt.Pattern(o) for _ in range(E)]
    worst = 0.0
    for d in range(2):
        pat.advance_dev()
        got = esp.fields(pat)
        for e in range(E):
            one[e].advance_dev()
            diff = esp.differing(got, e, one[e])
            print("[t63 ensemble sppt] advance %d member %d: not bit-equal to the single object: %s" % (d, e, diff or "nothing"))
            assert "eta" not in diff, (d, e)
            want = ref[e].advance(sppt.noise(sd[e], d, esp.shape(sp)))
            es_, ep = synth.relerr(got["spec"][e], ref[e].spec), synth.relerr(got["pattern"][e], want)
            print("[t63 ensemble sppt] advance %d member %d: spec %.1e, pattern %.1e vs restatement" % (d, e, es_, ep))
            worst = max(worst, es_, ep)
            assert pat.draws(e) == d + 1
    assert worst <= TOL, worst
    sp.close()


# ---------------------------------------------------------------------------------------------- 8. error codes on a device plan
def test_error_codes_on_a_device_plan():
    """s of another member count and s of another plan in the physics call, max_batch < nmem*kx at create: SPDY_ERR_ARG, before
    anything is enqueued; create, reset and draws while a capture is open: SPDY_ERR_STATE, and the capture stays usable."""
    import torch
    import speedy_f90_amd as s
    E, kx = 2, 8
    sp, other, small = support.ensemble_plan("t30", E), support.ensemble_plan("t30", E), support.plan("t30", 20)
    lib = sp.lib
    sp.radiation_set_date(0.0)
    sp.surface_set_orography(np.zeros(sp.grid_shape))
    z = lambda *shape, c=False: torch.zeros(shape, dtype=torch.complex128 if c else torch.float64, device="cuda")
    lev, grid = (E, kx, sp.nx, sp.mx), (E,) + sp.grid_shape
    bnd = {n: z(*grid) for n in ("fmask", "sst", "stl", "soilw", "snowc", "alb_l", "alb_s")}
    args = (True, z(*lev, c=True), z(*lev, c=True), z(*lev, c=True), z(*lev, c=True), z(*lev, c=True), z(E, sp.nx, sp.mx, c=True), bnd,
            z(*grid), z(E * sp.radiation_state_size()), *[z(E, kx, *sp.grid_shape) for _ in range(4)])
    two, three, foreign = s.Sppt(sp, NSTEPS, nmem=2), s.Sppt(sp, NSTEPS, nmem=3), s.Sppt(other, NSTEPS, nmem=2)
    for pat, word in ((three, "3 patterns"), (foreign, "another plan")):
        with pytest.raises(s.SpdyError) as e:
            sp.ens_physics_sppt_dev(E, pat, *args)
        assert e.value.code == ARG and word in str(e.value), word
    with pytest.raises(s.SpdyError) as e:
        sp.physics_sppt_dev(two, *[a[0] if torch.is_tensor(a) and a.dim() > 1 else a for a in args])
    assert e.value.code == ARG
    with pytest.raises(s.SpdyError) as e:                                   # 3 * 8 fields do not fit max_batch = 20
        s.Sppt(small, NSTEPS, nmem=3)
    assert e.value.code == ARG
    s.Sppt(small, NSTEPS, nmem=2).close()
    sp.use_own_stream()
    h, n = ctypes.c_void_p(), ctypes.c_longlong()
    sd = (ctypes.c_ulonglong * 2)(1, 2)
    with sp.graph_capture() as g:
        two.advance_dev()
        rc = (lib.spdy_ens_sppt_create(sp.h, 2, NSTEPS, None, sd, ctypes.byref(h)), lib.spdy_ens_sppt_reset(two.h, 1, 5),
              lib.spdy_ens_sppt_draws(two.h, 1, ctypes.byref(n)), lib.spdy_sppt_reset(two.h, 5), lib.spdy_sppt_draws(two.h, ctypes.byref(n)))
    assert rc == (STATE,) * 5, rc
    assert [two.draws(e) for e in range(2)] == [0, 0]
    g.launch()
    sp.synchronize()
    assert [two.draws(e) for e in range(2)] == [1, 1]
    g.close()
    for p in (sp, other, small):
        p.close()
