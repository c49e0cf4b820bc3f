"""GPU: observations given at a pressure (include/spdy.h, "ensemble analysis, observations at a pressure"; Letkf.set_obs(p=...);
DESIGN.md s22) against the NumPy restatement (tests/letkfpressure.py): the observation-space quantities to the bit on crafted
ensembles that hold every class of target, the tie to the model-level path, the rejection of out-of-column observations, the
vertical localisation, the analysis of an ensemble's spectral state against the restatement fed by the oracle's transforms, the
nature run's values, the capture, and one analysis of the twin experiment.  T30; the section "on the T63 L16 grid" repeats the
observation space, the vertical localisation, the nature run's values and the analysis from spectra at 192 x 96 x 16."""
import ctypes

import numpy as np
import pytest

import letkf as lk
import letkfpressure as lp
import nature as nt
import pressurelevels as pl
import support

pytestmark = pytest.mark.gpu

FIELDS = ("hx", "hxmean", "y", "departure", "obs_lnsigma", "obs_used")
ERR_STATE = -5


TAGS = {2: "t30k2", 5: "t30k5", 8: "t30"}      # the T30 plans by their level count; "t30k2" is this file's, on pl.SIGMA_L2
T63 = "t63k16"


def _plan(tag, nmem):
    import speedy_f90_amd as s
    if tag == "t30k2":
        sp = s.Spectral("t30", kx=2, max_batch=nmem * 12, device=0)
        sp.set_sigma(pl.SIGMA_L2)
    else:
        sp = support.ensemble_plan(tag, nmem)
    return sp, lp.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


def device_fields(lt):
    return {n: lt.field(n).numpy() for n in FIELDS}


def same_but_nan_bits(a, b):
    """bit for bit the same where either is a number, NaN where the other is: which NaN an operation on a NaN returns (its sign, its
    payload) is the hardware's choice, not the definition's"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and support.same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def increments(sp, lt, x):
    got = lk.run(lt, x, names=())
    return {v: got[v] for v in lk.VARS}


# ---------------------------------------------------------------------------------------------------- 1. observation space
def observation_space(sp, g, E):
    """hx, hxmean, y, departure, obs_lnsigma and obs_used of the crafted network bit-equal to the restatement, with 0, 1, 257 (more
    than one workgroup at every E, the last one partly filled) and all observations: there is no transcendental on the device"""
    x = lp.craft(g, E, seed=7 + E)
    full = lp.network(g, x)
    for n in (0, 1, min(257, len(full["var"]) - 1), len(full["var"])):
        obs = lk.subset(full, np.arange(len(full["var"])) < n)
        lt = lp.make(sp, E, obs)
        inc = increments(sp, lt, x)
        assert all(np.isfinite(a).all() for a in inc.values())
        want = lk.obs_space(g, x, obs, stencil=lp.tables(lt))
        got = device_fields(lt) if n else want               # no observation: nothing to read, the call itself is the test
        for name in FIELDS:
            assert support.same_bits(got[name], want[name]), (g.kx, E, n, name, np.nonzero(got[name] != want[name]))
        assert np.array_equal(lt.table("lnp"), lp.lnp(obs))
        lt.close()
    assert (want["obs_used"] == 0.0).sum() >= 10


@pytest.mark.parametrize("E", [2, 3, 32])
@pytest.mark.parametrize("kx", [2, 5, 8])
def test_observation_space(kx, E, plans):
    """`observation_space` (tests/test_letkf_pressure_cpu.py asserts the network's classes)"""
    sp, g = plans(TAGS[kx])
    observation_space(sp, g, E)


# ---------------------------------------------------------------------------------------------------- 2. the tie to the existing path
@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_tie_to_model_levels(stride, plans):
    """Every variable constant in the vertical per member and point, every at-pressure observation in column, sigma_v = 0: hx and
    the increments of analyse_grid have the bits of the same stations given on model levels through spdy_letkf_set_obs"""
    import speedy_f90_amd as s
    sp, g = plans("t30")
    E = 3
    x = lk.ensemble(g, E, seed=12)
    for v in lk.VARS[:4]:
        x[v] = np.repeat(x[v][:, 3:4], g.kx, axis=1)
    x["ps"] = np.random.default_rng(13).uniform(-0.05, 0.05, x["ps"].shape)
    names = dict(lp.targets(g))
    pts = lk.edge_points(g) + [(7.3 * o, -80.0 + 2.1 * o) for o in range(70)]
    tg = [names[n] for n in names if n != "above"]
    n = len(pts) * 3
    var = np.arange(n) % 5
    plain = lk.observations(g, x, var, np.arange(n) % g.kx, [pts[o % len(pts)][0] for o in range(n)], [pts[o % len(pts)][1] for o in range(n)], 0.5)
    atp = dict(plain, lev=np.where(np.arange(n) % 3 == 2, plain["lev"], lp.AT_P),
               p=np.array([pl.P0 * np.exp(tg[o % len(tg)]) for o in range(n)]))
    assert lp.at_pressure(atp).sum() > n // 2 and (lk.obs_space(g, x, atp)["obs_used"] == 1.0).all()
    res = []
    for obs, make in ((plain, lk.make), (atp, lp.make)):
        lt = s.Letkf(sp, E, n, lk.SIGMA_H, 0.0, lk.RHO, weight_stride=stride)
        lt.set_obs(*(lk.args(obs) if make is lk.make else lp.args(obs)))
        inc = increments(sp, lt, x)
        res.append((inc, lt.field("hx").numpy(), lt.field("obs_used").numpy()))
        lt.close()
    assert support.same_bits(res[0][1], res[1][1])
    assert (res[0][2] == 1.0).all() and (res[1][2] == 1.0).all()
    for v in lk.VARS:
        assert support.same_bits(res[0][0][v], res[1][0][v]), v
    assert float(np.max(np.abs(res[1][0]["t"]))) > 0.0


# ---------------------------------------------------------------------------------------------------- 3. rejection
@pytest.mark.parametrize("E", [3, 32])
def test_rejected_observations_take_no_part(E, plans):
    """The crafted network, rejected observations interleaved with used ones (its order is a permutation), and one more rejected
    observation whose stencil no other shares and whose members hold NaN at level 0, the level its target is clamped to: the
    increments are bit-equal to those of the network with the rejected observations removed"""
    sp, g = plans("t30")
    x = lp.craft(g, E, seed=21 + E)
    obs = lp.network(g, x)
    lone = lp.make_pobs([lk.T], [lp.AT_P], [pl.P0 * np.exp(dict(lp.targets(g))["above"])], [200.3], [-47.2], [250.0], [1.0])
    idx, _ = lk.stencil(g, obs["lon"], obs["lat"])
    mine, _ = lk.stencil(g, lone["lon"], lone["lat"])
    assert not np.isin(idx, mine).any()
    x["t"].reshape(E, g.kx, -1)[:, 0, mine[0]] = np.nan
    n = len(obs["var"])
    both = {k: np.insert(obs[k], n // 2, lone[k]) for k in obs}
    want = lk.obs_space(g, x, both)
    used = want["obs_used"] == 1.0
    assert (~used).sum() >= 10 and (used[:-1] != used[1:]).sum() >= 10                               # interleaved
    assert not used[n // 2] and np.isnan(want["hx"][n // 2]).all() and np.isfinite(want["hx"][used]).all()
    lt = lp.make(sp, E, both)
    a = increments(sp, lt, x)
    got, want = device_fields(lt), lk.obs_space(g, x, both, stencil=lp.tables(lt))
    assert np.array_equal(want["obs_used"] == 1.0, used)
    for name in FIELDS:
        assert same_but_nan_bits(got[name], want[name]), name
    assert np.isnan(got["departure"][n // 2]) and np.isnan(got["hx"][n // 2]).all()
    lt.close()
    lt = lp.make(sp, E, lk.subset(both, used))
    b = increments(sp, lt, x)
    assert (lt.field("obs_used").numpy() == 1.0).all()
    lt.close()
    for v in lk.VARS:
        assert support.same_bits(a[v], b[v]), v
    nan = np.isnan(a["t"])
    assert nan.sum() == E * len(set(mine[0])) and nan.reshape(E, g.kx, -1)[:, 0, mine[0]].all()      # the grid's own NaN, nothing more
    assert all(np.isfinite(a[v]).all() for v in ("u", "v", "q", "ps"))


# ---------------------------------------------------------------------------------------------------- 4. vertical localisation
def vertical_localisation(tag, sp, g):
    """sigma_v = 0.3: the increments against the restatement, which localises with ln sigma_o = ln(p/p0) - psbar, within
    tests/letkf.py's limits (the Jacobi route sampled at the hardest columns, as tests/test_gpu_letkf.py does)"""
    E, sigma_v = 3, 0.3
    x = lp.craft(g, E, seed=31)
    obs = lp.network(g, x)
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=32, outside=8)
    C, b = lk.problems(g, obs, lk.obs_space(g, x, obs), lk.SIGMA_H, sigma_v, cols)
    lim, ref, kappa = lk.limits(g, x, C, b, lk.RHO, cols, E, lk.hardest(C, lk.RHO, 12))
    lt = lp.make(sp, E, obs, sigma_v)
    got = increments(sp, lt, x)
    lns = lt.field("obs_lnsigma").numpy()
    lt.close()
    worst = {v: float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v] for v in lk.VARS}
    print("[pobs vertical localisation%s] %d observations, %d columns, kappa %.2e, ratio to the limit: %s"
          % (tag, len(obs["var"]), len(cols), kappa, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    # the position differs from the host table's where ps is not 0: the localisation is the call's, not the upload's
    atp = lp.at_pressure(obs)
    assert (lns[atp] != lp.lnp(obs)[atp]).any() and np.array_equal(lns[~atp], lk.lnsigma(g, dict(obs, lev=np.where(atp, 0, obs["lev"])))[~atp])


def test_vertical_localisation(plans):
    """kx = 8: `vertical_localisation`"""
    sp, g = plans("t30")
    vertical_localisation("", sp, g)


def test_vertical_factor_of_zero_changes_nothing(plans):
    """sigma_v = 0.02, so c_v = 0.0365 and the support 0.073: observations in the middle of the first bracket, at least 0.6 from
    every level in ln sigma, appended to the network, are in column and used, and leave every increment's bits"""
    sp, g = plans("t30")
    E, sigma_v = 3, 0.02
    x = lp.craft(g, E, seed=41)
    x["ps"][lp.PATCH_MEMBER] = np.where(x["ps"][lp.PATCH_MEMBER] == lp.HIGH, 0.0, x["ps"][lp.PATCH_MEMBER])
    obs = lp.network(g, x)
    mid = pl.P0 * np.exp(dict(lp.targets(g))["mid0"])
    more = lp.make_pobs([lk.T, lk.U, lk.Q], [lp.AT_P] * 3, [mid] * 3, [100.0, 101.0, 250.0], [20.0, 21.0, -30.0], [260.0, 5.0, 4.0], [0.1] * 3)
    both = {k: np.concatenate([obs[k], more[k]]) for k in obs}
    s = lk.obs_space(g, x, both)
    assert (s["obs_used"][-3:] == 1.0).all()
    assert float(np.min(np.abs(g.lnfsg[:, None] - s["obs_lnsigma"][None, -3:]))) >= 2.0 * sigma_v * np.sqrt(10.0 / 3.0)
    res = []
    for o in (obs, both):
        lt = lp.make(sp, E, o, sigma_v)
        res.append(increments(sp, lt, x))
        lt.close()
    for v in lk.VARS:
        assert support.same_bits(res[0][v], res[1][v]), v
    assert float(np.max(np.abs(res[0]["t"]))) > 0.0


# ---------------------------------------------------------------------------------------------------- 5. from spectra
@pytest.mark.parametrize("E", [3, 32])
def test_from_spectra(E, plans, oracle_factory):
    """Ensemble.analyse on the standard test ensemble (tests/ensemblestep.py's member states, kx = 5) with radiosonde-like stations
    reporting u, v, t and q at 925, 850, 700, 500, 300, 200 and 100 hPa, sigma_v = 0.3, against the restatement on the oracle's
    grids through the oracle's direct transforms: every prognostic of time level 1 within 1e-12 of its scale, the limit
    tests/test_gpu_letkf.py holds its spectral route to; time level 2 keeps its bits; obs_used equals the restatement's (tests/
    test_letkf_pressure_cpu.py asserts that no target is within 1e-9 of an end level on these inputs) and holds both kinds;
    obs_lnsigma, formed from the device's own ps grids, within 1e-12; five graph nodes' worth of launches is test_capture's matter"""
    import torch
    import ensemblestep as es
    sp, g = plans("t30k5")
    o = oracle_factory("t30k5")
    sts, x, net = lp.spectral_case(sp, o, g, E)
    want, space = lp.spectral_analysis(o, g, sts, x, net)
    ens = es.build(sp, sts)
    lt = lp.make(sp, E, net, lp.SPECTRAL_SIGMA_V)
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.analyse(lt)
    torch.cuda.synchronize()
    used = lt.field("obs_used").numpy()
    assert np.array_equal(used, space["obs_used"]) and 0.2 * len(used) <= used.sum() <= 0.9 * len(used)
    assert float(np.max(np.abs(lt.field("obs_lnsigma").numpy() - space["obs_lnsigma"]))) <= 1e-12
    worst = 0.0
    for n in es.PROG:
        a = getattr(ens, n)
        assert support.same_bits(a[1], before[n][1]), n
        assert not support.same_bits(a[0], before[n][0]), n
        for e in range(E):
            ref = want[e][n]
            err = float(np.max(np.abs(a[0, e].cpu().numpy() - ref)) / np.max(np.abs(ref)))
            worst = max(worst, err)
            assert err <= 1e-12, (n, e, err)
    print("[pobs from spectra E=%d] %d of %d observations used, largest error %.3e of the scale" % (E, int(used.sum()), len(used), worst))
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. the nature run
def device_draws(sp, n, seed, draws):
    """z_o of the device for draw number `draws`, bit for bit: nature_slot_draw_kernel on a model-level network with error 1 and a truth
    of zeros stores 0 + (1 * 1) * z_o"""
    import speedy_f90_amd as s
    nat = s.Nature(sp, seed=seed, capacity=1)
    lt = s.Letkf(sp, 2, n, lk.SIGMA_H)
    lt.set_obs(np.zeros(n, int), np.zeros(n, int), np.zeros(n), np.zeros(n), np.zeros(n), np.ones(n))
    for _ in range(draws + 1):
        nat.observe(lt, 1.0)
    z = lt.field("value").numpy()
    nat.close(); lt.close()
    return z


def test_nature_values(plans):
    """observe on the crafted network with the crafted ensemble's high-terrain member as the truth: noise = 0 gives the
    restatement's bits, clamped where the truth is out of column (above the top, below the patch); noise > 0 gives h + (noise error)
    z with the device's own draws of the model-level kernel to the bit, and those draws are tests/nature.py's within the limit
    tests/test_gpu_nature.py holds them to; draws advances by one per call.  Measured on an MI355X: the device's draws differ from
    NumPy's by at most 2.2e-16 and are not bit-equal to them (the device's randn is its own logarithm and cosine), so bits are asked
    against the draws nature_slot_draw_kernel itself stores, and NumPy's are held to that limit"""
    import speedy_f90_amd as s
    sp, g = plans("t30")
    seed = 0x51DE
    x = lp.craft(g, 2, seed=51)
    truth = nt.as_truth(x, lp.PATCH_MEMBER)
    net = lp.network(g, x)
    n = len(net["var"])
    h = lp.truth_values(g, truth, net)
    alone = lk.obs_space(g, {v: np.stack([truth[v], truth[v]]) for v in lk.VARS}, net)
    out = alone["obs_used"] == 0.0
    assert out.sum() >= 10 and np.isfinite(h).all()
    nat = s.Nature(sp, seed=seed, capacity=1)
    nat.field("truth").upload(nt.rows(truth))
    lt = lp.make(sp, 2, net)
    h = lp.truth_values(g, truth, net, lp.tables(lt))
    assert nat.draws() == 0
    nat.observe(lt, 0.0)
    assert support.same_bits(lt.field("value").numpy(), h) and nat.draws() == 1
    nat.observe(lt, 0.75)
    got = lt.field("value").numpy()
    assert nat.draws() == 2
    nat.close(); lt.close()
    z = device_draws(sp, n, seed, 1)
    assert support.same_bits(got, h + (0.75 * net["error"]) * z)
    zref = nt.draw(seed, 1, n)
    tol = 1e-12 * float(np.max(np.abs(zref)))
    print("[pobs nature] device draws against tests/nature.py: %.3e, bit-equal %s" % (float(np.max(np.abs(z - zref))), support.same_bits(z, zref)))
    assert float(np.max(np.abs(z - zref))) <= tol


# ---------------------------------------------------------------------------------------------------- 7. the capture
def test_capture(plans):
    """A captured analyse_grid with out= replays to the eager bits; after the input ps has been overwritten with another ensemble's
    the replay gives that ensemble's eager result, in obs_lnsigma and obs_used too; the graph has as many nodes as the same capture
    with a model-level network; spdy_pobs_set is refused while a capture is open"""
    import torch
    import speedy_f90_amd as s
    sp, g = plans("t30")
    E = 3
    x1 = lp.craft(g, E, seed=61)
    x2 = dict(x1, ps=np.random.default_rng(62).uniform(-0.05, 0.05, x1["ps"].shape))
    obs = lp.network(g, x1)
    want = [lk.obs_space(g, x, obs) for x in (x1, x2)]
    assert not np.array_equal(want[0]["obs_used"], want[1]["obs_used"])
    lt = lp.make(sp, E, obs, 0.3)
    want = [lk.obs_space(g, x, obs, stencil=lp.tables(lt)) for x in (x1, x2)]
    eager = []
    for x in (x1, x2):
        inc = increments(sp, lt, x)
        f = device_fields(lt)
        eager.append((inc, f))
    for k in (0, 1):
        for name in FIELDS:
            assert support.same_bits(eager[k][1][name], want[k][name]), (k, name)
    xd = [support.dev(x1[v]) for v in lk.VARS]
    out = tuple(torch.empty_like(a) for a in xd)
    plain = lk.make(sp, E, lk.edge_obs(g, x1), 0.3)
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gm:
            plain.analyse_grid(*xd, out=out)
        with sp.graph_capture() as gr:
            lt.analyse_grid(*xd, out=out)
            one = (s.PObs * 1)(s.PObs(lk.T, lp.AT_P, 50000.0, 10.0, 5.0, 1.0, 1.0))
            assert sp.lib.spdy_pobs_set(lt.h, 1, ctypes.cast(one, ctypes.c_void_p)) == ERR_STATE
            assert b"capture" in sp.lib.spdy_last_error()
        assert gr.num_nodes() == gm.num_nodes() == 2, (gr.num_nodes(), gm.num_nodes())
        for k in (0, 1, 0):
            xd[4].copy_(torch.from_numpy((x1, x2)[k]["ps"]))
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for v, a in zip(lk.VARS, out):
                assert support.same_bits(a.cpu().numpy(), eager[k][0][v]), (k, v)
            f = device_fields(lt)
            for name in FIELDS:
                assert support.same_bits(f[name], eager[k][1][name]), (k, name)
        # a graph captured with a model-level network, replayed after a set with pressures (the header asks for a new capture):
        # the old observation kernel finds level 0 for an at-pressure observation, never a negative level, and stays in bounds
        n = plain.nobs
        plain.set_obs(np.full(n, lk.T), np.full(n, lp.AT_P), obs["lon"][:n], obs["lat"][:n], np.full(n, 250.0), np.ones(n),
                      p=np.full(n, 50000.0))
        xd[4].copy_(torch.from_numpy(x1["ps"]))
        torch.cuda.synchronize()
        gm.launch()
        sp.synchronize()
        level0 = lk.make_obs(np.full(n, lk.T), np.zeros(n), obs["lon"][:n], obs["lat"][:n], np.full(n, 250.0), np.ones(n))
        assert support.same_bits(plain.field("hx").numpy(), lk.observe(g, x1, level0, lp.tables(plain))[0])
        assert all(bool(torch.isfinite(a).all()) for a in out)
        gr.close(); gm.close()
    finally:
        sp.use_torch_stream()
    lt.close(); plain.close()


# ---------------------------------------------------------------------------------------------------- 8. the twin step
def test_twin_step():
    """One analysis of tests/nature.py's twin set-up with a radiosonde-like network at pressures (tests/letkfpressure.py:
    twin_inputs; tests/test_letkf_pressure_cpu.py asserts the condition on the restatement first): the values drawn by
    Nature.observe, the scores by Nature.verify_grid; the rmse of the analysis mean of u, v and t is below the background's at both
    levels, and the observations used are the restatement's"""
    import speedy_f90_amd as s
    c = nt.TWIN
    kx, E = c["kx"], c["E"]
    sp = s.Spectral("t30", kx=kx, max_batch=64, device=0)
    sp.set_sigma(nt.twin_sigma(kx))
    g = lp.Geometry(sp)
    truth, x, net = lp.twin_inputs(g)
    nat = s.Nature(sp, seed=c["noise_seed"], capacity=2)
    nat.field("truth").upload(nt.rows(truth))
    lt = lp.make(sp, E, net, c["sigma_v"], c["rho"], c["sigma_h"])
    nat.observe(lt, 1.0)
    xd = [support.dev(x[v]) for v in lk.VARS]
    nat.verify_grid(*xd, slot=0)
    inc = lt.analyse_grid(*xd)
    nat.verify_grid(*[a + b for a, b in zip(xd, inc)], slot=1)
    got = nat.field("scores").numpy()
    assert np.array_equal(lt.field("obs_used").numpy(), lk.obs_space(g, x, net, stencil=lp.tables(lt))["obs_used"])
    ratios = {v: got[1][0][n * kx:(n + 1) * kx] / got[0][0][n * kx:(n + 1) * kx] for n, v in enumerate(lk.VARS[:3])}
    print("[pobs twin, device] rmse analysis / background: %s" % " ".join("%s %s" % (v, np.round(r, 3)) for v, r in ratios.items()))
    assert all((r < 1.0).all() for r in ratios.values()), ratios
    nat.close(); lt.close(); sp.close()


# ---------------------------------------------------------------------------------------------------- 9. on the T63 L16 grid
@pytest.mark.parametrize("E", [2, 3, 32])
def test_observation_space_t63(E, plans):
    """192 x 96 x 16: `observation_space` on the crafted network of 1 114 observations -- obsop_pressure runs 16 trips of its bracket
    search over four stencil columns (tests/test_letkf_t63_cpu.py asserts the network's classes, every bracket of the 15 among them)"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    observation_space(sp, g, E)


def test_vertical_localisation_t63(plans):
    """192 x 96 x 16: `vertical_localisation`"""
    sp, g = plans(T63)
    vertical_localisation(" T63 L16", sp, g)


def test_nature_values_t63(plans):
    """192 x 96 x 16: Nature.observe with noise = 0 on the crafted network, the crafted ensemble's high-terrain member as the truth,
    gives the restatement's bits, clamped where the truth is out of column (test_nature_values' first statement)"""
    import speedy_f90_amd as s
    sp, g = plans(T63)
    x = lp.craft(g, 2, seed=51)
    truth = nt.as_truth(x, lp.PATCH_MEMBER)
    net = lp.network(g, x)
    alone = lk.obs_space(g, {v: np.stack([truth[v], truth[v]]) for v in lk.VARS}, net)
    assert (alone["obs_used"] == 0.0).sum() >= 10
    nat = s.Nature(sp, seed=0x51DE, capacity=1)
    nat.field("truth").upload(nt.rows(truth))
    lt = lp.make(sp, 2, net)
    h = lp.truth_values(g, truth, net, lp.tables(lt))
    assert np.isfinite(h).all() and nat.draws() == 0
    nat.observe(lt, 0.0)
    assert support.same_bits(lt.field("value").numpy(), h) and nat.draws() == 1
    nat.close(); lt.close()


def drifted_states(sp, sts, fraction=0.1, seed=8500):
    """the member states a fraction of the way towards another seeded ensemble's: the state of an earlier time slot"""
    import ensemblestep as es
    other = es.member_states(sp, len(sts), seed)
    return [dict(st, **{n: st[n] + fraction * (ot[n] - st[n]) for n in es.PROG}) for st, ot in zip(sts, other)]


@pytest.mark.parametrize("slots", [False, True], ids=["plain", "slots"])
def test_from_spectra_t63(slots, plans, oracle_factory):
    """192 x 96 x 16, E = 3, 40 radiosonde-like stations (1 120 observations at a pressure), sigma_v = 0.3, weight stride (2, 2),
    relaxation (0.3, 0.9): Ensemble.analyse -- and, with slots, Ensemble.observe of two slots on two ensembles' spectra, then
    analyse(slots=True) -- against the restatement (tests/letkfinterp.py's analysis, tests/letkfrelax.py's relaxation) on the
    oracle's grids through the oracle's direct transforms, under test_from_spectra's rule: every prognostic of time level 1 within
    1e-12 of its scale, time level 2 keeps its bits, obs_used equals the restatement's and holds both kinds, obs_lnsigma within
    1e-12.  The increments go back through the direct transform as E (4 kx + 1) = 195 fields"""
    import torch
    import ensemblestep as es
    import letkfinterp as li
    import letkfrelax as lr
    sp, g = plans(T63)
    o = oracle_factory(T63)
    E, stride, relax = 3, (2, 2), (0.3, 0.9)
    sts, x, net = lp.spectral_case(sp, o, g, E, stations=40)
    n = len(net["var"])
    assert n == 40 * len(lp.SOUNDING) * 4 and lp.margin(g, x, net) >= lp.MARGIN
    how, first = {}, [0, n // 2 + 1, n]
    if slots:
        earlier = drifted_states(sp, sts)
        xa = lk.oracle_grids(o, earlier)
        assert lp.margin(g, xa, net) >= lp.MARGIN
        how = dict(xs=[xa, x], first=first)
    space = lk.obs_space(g, x, net, **how)
    inc, _, _ = li.analyse(g, x, net, lk.SIGMA_H, lp.SPECTRAL_SIGMA_V, lk.RHO, *stride, **how)
    dx, f = lr.relax(lr.at_columns(x, np.arange(g.ix * g.il)), inc, *relax)
    assert max(float(a.max()) for a in f.values()) > 1.0
    want = lp.to_spectra(o, g, sts, dx)
    ens = es.build(sp, sts)
    lt = lp.make(sp, E, net, lp.SPECTRAL_SIGMA_V)
    lt.set_weight_stride(*stride)
    lt.set_relaxation(*relax)
    before = {name: getattr(ens, name).clone() for name in es.PROG}
    if slots:
        lt.set_slots(first)
        es.build(sp, earlier).observe(lt, 0)
        ens.observe(lt, 1)
        ens.analyse(lt, slots=True)
    else:
        ens.analyse(lt)
    torch.cuda.synchronize()
    used = lt.field("obs_used").numpy()
    assert np.array_equal(used, space["obs_used"]) and 0.2 * len(used) <= used.sum() <= 0.9 * len(used)
    assert float(np.max(np.abs(lt.field("obs_lnsigma").numpy() - space["obs_lnsigma"]))) <= 1e-12
    if slots:
        now = lk.observe(g, x, net)[0]
        assert np.max(np.abs(space["hx"][:first[1]] - now[:first[1]])) > 1e-3       # the earlier slot's time matters
    worst = 0.0
    for name in es.PROG:
        a = getattr(ens, name)
        assert support.same_bits(a[1], before[name][1]), name
        assert not support.same_bits(a[0], before[name][0]), name
        for e in range(E):
            ref = want[e][name]
            err = float(np.max(np.abs(a[0, e].cpu().numpy() - ref)) / np.max(np.abs(ref)))
            worst = max(worst, err)
            assert err <= 1e-12, (name, e, err)
    print("[pobs from spectra T63 L16 %s] %d of %d observations used, largest error %.3e of the scale, ratio to the limit %.3f"
          % ("slots" if slots else "plain", int(used.sum()), len(used), worst, worst / 1e-12))
    lt.close()
