"""GPU: the nature run (include/spdy.h "nature run", Nature, Ensemble.verify) against its NumPy restatement
(tests/nature.py): the truth against the oracle's transforms and, to the bit, against the grid the analysis forms; the observation
values at the operator's edges and at 0, 1 and 300 observations; the noise against the restated generator; the scores at the
register-count extremes of the member loop and on the other grid; the exact statements; the isolation of a non-finite row; the
captured cycle; and the twin condition on the device.  T30 with kx = 5 and E = 3 unless said otherwise."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import nature as nt
import support
from conftest import TOL
from dynstep import state as dyn_state

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SIGMA_H, SIGMA_V, RHO = 5.0e5, 0.1, 1.1
E0, NOBS = 3, 300
EPS = lk.EPS
LEVEL1 = ("vor", "div", "t", "tr", "ps")


def level1(D):
    """time level 1 of a single-state dict of device views (Ensemble.member), in set_state's order"""
    return [D[n][0] for n in LEVEL1]


def spectra(st):
    """time level 1 of a host state as device tensors, in set_state's order"""
    return [support.dev(np.ascontiguousarray(st[n][0], np.complex128)) for n in LEVEL1]


def gridded(lt, sp):
    """the analysis object's grid workspace as a gridded ensemble (after verify: the members on the grid)"""
    G, E, kx = lt.field("grid").numpy(), lt.nmem, sp.kx
    x = {v: G[n * E * kx:(n + 1) * E * kx].reshape((E, kx) + sp.grid_shape) for n, v in enumerate(lk.VARS[:4])}
    x["ps"] = G[4 * E * kx:]
    return x


def network(g, x, total=NOBS):
    """tests/letkf.edge_obs (the poles, the longitude seam, every variable) plus random observations, `total` in all: more than one
    workgroup of the draw kernel and not a multiple of its 256 threads"""
    edge = lk.edge_obs(g, x)
    net = lk.concat(edge, lk.sparse_obs(g, x, n=total - len(edge["var"])))
    assert len(net["var"]) == total and total > 256 and total % 256
    return net


def score_limits(g, x, truth, w, E):
    """(relative limit of rmse and spread, absolute limit of bias per row (4 kx + 1)).  rmse and spread are roots of sums of ncol
    non-negative terms, each the result of an E-term sum and a handful of operations, and the root halves the relative error: 4
    (ncol + E + 8) eps.  The bias is a sum of ncol terms that cancels, so its error scales with <|m - truth|>: 4 (ncol + E) eps of
    it."""
    ncol = g.ix * g.il
    absm = {v: np.abs(np.sum(x[v].reshape(E, -1, g.il, g.ix) - truth[v].reshape(-1, g.il, g.ix)[None], axis=0) / E) for v in lk.VARS}
    gw = nt.normalised(w)
    mean = np.concatenate([np.einsum("j,kj->k", gw, absm[v].sum(axis=-1) / g.ix) for v in lk.VARS])
    return 4 * (ncol + E + 8) * EPS, 4 * (ncol + E) * EPS * mean


def compare_scores(tag, got, want, rel, bias_abs):
    """got, want: (3, 4 kx + 1) tables rmse | bias | spread; prints the measured error-to-limit ratios and asserts them"""
    r = {"rmse": np.max(np.abs(got[0] - want[0]) / (rel * want[0])), "spread": np.max(np.abs(got[2] - want[2]) / (rel * want[2])),
         "bias": np.max(np.abs(got[1] - want[1]) / bias_abs)}
    print("[nature scores %s] error / limit: %s" % (tag, " ".join("%s %.2e" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, (tag, r)
    return r


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lk.Geometry(sp), nt.gaussian_weights(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30k5", nmem=32: get(tag, nmem)


@pytest.fixture(scope="module")
def case(plans, oracle_factory):
    """the seeded states of tests/test_gpu_letkf.py's Ensemble.analyse case, a truth state of another seed, the oracle's grids of
    the members (computed once, read only) and the 300-observation network"""
    sp, g, w = plans()
    sts = es.member_states(sp, E0)
    x = lk.oracle_grids(oracle_factory("t30k5"), sts)
    return {"sp": sp, "g": g, "w": w, "sts": sts, "x": x, "truth_state": dyn_state(sp, 7000), "net": network(g, x)}


def make(sp, E, net, capacity=2, seed=SEED):
    import speedy_f90_amd as s
    lt = s.Letkf(sp, E, max(len(net["var"]), 1), SIGMA_H, SIGMA_V, RHO)
    lt.set_obs(*lk.args(net))
    return s.Nature(sp, seed=seed, capacity=capacity), lt


def noise_limit(z_ref, h, err):
    """what tests/test_gpu_sppt.py holds the device's randn to (TOL of the largest draw) plus 4 eps |h| / error for the two
    roundings of h + (noise error) z and of the difference the test takes"""
    return TOL * np.max(np.abs(z_ref)) + 4 * EPS * np.abs(h) / err


# ---------------------------------------------------------------------------------------------------- 1. the truth
def test_truth(case, oracle_factory):
    """set_state of member 1's state: every variable within 1e-12 of its scale of the oracle's transforms.  And to the bit: with
    observe(noise = 0) the value table is H(truth), and the analysis of an ensemble whose member 1 holds that state computes hx[:,
    1] from its own inverse batch of E members -- the same bits, so the truth is the grid the analysis forms."""
    import torch
    sp, g, net = case["sp"], case["g"], case["net"]
    ens = es.build(sp, case["sts"])
    nat, lt = make(sp, E0, net)
    nat.set_state(*level1(ens.member(1)))
    truth = nat.truth()
    for v in lk.VARS:
        ref = case["x"][v][1]
        err = float(np.max(np.abs(truth[v] - ref)) / np.max(np.abs(ref)))
        print("[nature truth] %s vs the oracle: %.3e" % (v, err))
        assert truth[v].shape == ref.shape and err <= 1e-12, (v, err)
    nat.observe(lt, 0.0)
    value = lt.field("value").numpy()
    h = nt.observe(g, truth, net, net["error"], SEED, 0, 0.0)
    scale = np.array([np.max(np.abs(truth[lk.VARS[v]])) for v in net["var"]])
    assert float(np.max(np.abs(value - h) / (16 * EPS * scale))) <= 1.0        # the operator's bound of tests/test_gpu_letkf.py
    ens.analyse(lt)
    torch.cuda.synchronize()
    hx = lt.field("hx").numpy()
    assert support.same_bits(hx[:, 1], value)
    assert not support.same_bits(hx[:, 0], value)
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 2. sizes
def test_no_and_one_observation(case):
    """nobs = 0 writes nothing and still counts; nobs = 1 (a workgroup with one live thread) gives the restatement's value"""
    sp, g = case["sp"], case["g"]
    nat, lt = make(sp, E0, case["net"])
    nat.set_state(*spectra(case["truth_state"]))
    truth = nat.truth()
    nat.observe(lt, 0.0)
    before = lt.field("value").numpy()
    lt.set_obs(*lk.args(lk.make_obs([], [], [], [], [], [])))
    nat.observe(lt, 1.0)
    assert nat.draws() == 2
    one = {k: a[5:6] for k, a in case["net"].items()}
    lt.set_obs(*lk.args(one))
    nat.observe(lt, 1.0)
    assert nat.draws() == 3
    got = lt.field("value").numpy()
    h = nt.operator(g, truth, one)
    z = (got - h) / one["error"]
    assert got.shape == (1,) and abs(z[0] - nt.draw(SEED, 2, 1)[0]) <= noise_limit(nt.draw(SEED, 2, 1), h, one["error"])[0]
    assert before.shape == (NOBS,)
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 3. the noise
def test_noise(case):
    """(value(noise = 1) - value(noise = 0)) / error is the restatement's z within the limit of tests/test_gpu_sppt.py plus 4 eps
    |h| / error; two calls give draws 0 and 1; reset(seed) starts over bit-equal; another seed differs; noise scales"""
    sp, g, net = case["sp"], case["g"], case["net"]
    nat, lt = make(sp, E0, net)
    nat.set_state(*spectra(case["truth_state"]))
    assert nat.draws() == 0
    nat.observe(lt, 0.0)
    h = lt.field("value").numpy()
    assert nat.draws() == 1                       # noise = 0 counts too
    nat.reset(SEED)
    assert nat.draws() == 0
    values = []
    for d in range(2):
        nat.observe(lt, 1.0)
        values.append(lt.field("value").numpy())
        z, ref = (values[d] - h) / net["error"], nt.draw(SEED, d, NOBS)
        worst = float(np.max(np.abs(z - ref) / noise_limit(ref, h, net["error"])))
        print("[nature noise] draw %d: error / limit %.3f, mean %.3f, std %.3f" % (d, worst, z.mean(), z.std()))
        assert worst <= 1.0, (d, worst)
    assert nat.draws() == 2 and not support.same_bits(values[0], values[1])
    nat.reset(SEED)
    nat.observe(lt, 1.0)
    assert support.same_bits(lt.field("value").numpy(), values[0])
    nat.observe(lt, 0.5)                          # draw 1 at half the amplitude
    half = (lt.field("value").numpy() - h) / net["error"]
    assert float(np.max(np.abs(half - 0.5 * nt.draw(SEED, 1, NOBS)) / noise_limit(nt.draw(SEED, 1, NOBS), h, net["error"]))) <= 1.0
    nat.reset(SEED + 1)
    nat.observe(lt, 1.0)
    assert not support.same_bits(lt.field("value").numpy(), values[0])
    state = nat.field("state").numpy().view(np.uint64)
    assert int(state[0]) == SEED + 1 and int(state[1]) == 1
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 4. the scores
def test_scores_of_a_state(case):
    """Ensemble.verify on the seeded states against tests/nature.scores on the grids the call formed (downloaded), E = 3, kx = 5"""
    sp, g, w = case["sp"], case["g"], case["w"]
    ens = es.build(sp, case["sts"])
    nat, lt = make(sp, E0, case["net"])
    nat.set_state(*spectra(case["truth_state"]))
    ens.verify(lt, nat, 1)
    x, truth = gridded(lt, sp), nat.truth()
    rel, bias_abs = score_limits(g, x, truth, w, E0)
    got = nat.field("scores").numpy()
    compare_scores("t30k5 E=3", got[1], nt.flat(nt.scores(g, x, truth, w)), rel, bias_abs)
    assert not got[0].any()                       # slot 0 was never written
    sc = nat.scores(1)
    assert sc["rmse"]["t"].shape == (sp.kx,) and isinstance(sc["spread"]["ps"], float) and nat.scores()["bias"]["u"].shape == (2, sp.kx)
    assert support.same_bits(np.asarray(nt.flat(sc), np.float64), got[1])
    with pytest.raises(ValueError):               # the member count is the Letkf's
        es.build(sp, case["sts"][:2]).verify(lt, nat)
    nat.close(); lt.close()


@pytest.mark.parametrize("E", [2, 32])
def test_scores_member_extremes(E):
    """kx = 2 at E = 2 and E = 32, the register-count extremes of the member loop (its 8- and 32-member forms), on gridded
    ensembles through verify_grid"""
    import speedy_f90_amd as s
    sp = s.Spectral("t30", kx=2, max_batch=16, device=0)
    sp.set_sigma(nt.twin_sigma(2))
    g, w = lk.Geometry(sp), nt.gaussian_weights(sp)
    x, truth = lk.ensemble(g, E, seed=60 + E), nt.as_truth(lk.ensemble(g, 1, seed=59))
    nat = s.Nature(sp, capacity=1)
    nat.field("truth").upload(nt.rows(truth))
    nat.verify_grid(*[support.dev(x[v]) for v in lk.VARS], slot=0)
    rel, bias_abs = score_limits(g, x, truth, w, E)
    compare_scores("t30k2 E=%d" % E, nat.field("scores").numpy()[0], nt.flat(nt.scores(g, x, truth, w)), rel, bias_abs)
    nat.close(); sp.close()


def test_scores_t63(plans):
    """T63 L16, E = 2: 192 longitudes, two passes of a workgroup over its latitude, 96 latitudes"""
    sp, g, w = plans("t63k16", 2)
    E = 2
    ens = es.build(sp, es.member_states(sp, E))
    nat, lt = make(sp, E, lk.make_obs([], [], [], [], [], []), capacity=1)
    nat.set_state(*spectra(dyn_state(sp, 7000)))
    ens.verify(lt, nat, 0)
    x, truth = gridded(lt, sp), nat.truth()
    rel, bias_abs = score_limits(g, x, truth, w, E)
    compare_scores("t63k16 E=2", nat.field("scores").numpy()[0], nt.flat(nt.scores(g, x, truth, w)), rel, bias_abs)
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 5. exact statements
def test_exact_statements(case):
    """every member equal to the truth: rmse, bias and spread are exactly 0 in every row; two runs of verify are bit-equal; a
    verify into slot 1 leaves slot 0's bits"""
    sp = case["sp"]
    nat, lt = make(sp, E0, case["net"])
    same = es.build(sp, [case["sts"][1]] * E0)
    nat.set_state(*level1(same.member(2)))
    same.verify(lt, nat, 0)
    assert not nat.field("scores").numpy()[0].any()
    ens = es.build(sp, case["sts"])
    ens.verify(lt, nat, 0)
    first = nat.field("scores").numpy()
    assert first[0].all() and not first[1].any()
    ens.verify(lt, nat, 0)
    assert support.same_bits(nat.field("scores").numpy(), first)
    nat.set_state(*spectra(case["truth_state"]))
    ens.verify(lt, nat, 1)
    after = nat.field("scores").numpy()
    assert support.same_bits(after[0], first[0]) and after[1].all() and not support.same_bits(after[1], first[0])
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 6. isolation
def test_nonfinite_row_stays_in_its_row(case):
    """one NaN in member 1's t at level 2 (a spectral coefficient: that member's grid of that level) makes the three scores of row
    (t, 2) NaN and leaves every other row's bits.  Test data, not a fault: the kernels have fixed loop bounds."""
    sp = case["sp"]
    kx, k = sp.kx, 2
    nat, lt = make(sp, E0, case["net"])
    ens = es.build(sp, case["sts"])
    nat.set_state(*spectra(case["truth_state"]))
    ens.verify(lt, nat, 0)
    ens.t[0, 1, k, 1, 1] = float("nan")
    ens.verify(lt, nat, 1)
    clean, got = nat.field("scores").numpy()
    row = 2 * kx + k
    others = np.arange(4 * kx + 1) != row
    assert np.isnan(got[:, row]).all() and np.isfinite(clean).all()
    assert support.same_bits(got[:, others], clean[:, others])
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 7. the capture
def test_capture(case):
    """one graph of set_state, observe, verify(slot 0), Ensemble.analyse, verify(slot 1), replayed three times on unchanged input
    spectra with the ensemble restored in between: draws advances by 3, the last replay's values are the restatement's draw 2, slot
    0 is bit-equal across the replays and equal to the eager call's, and slot 1 moves with the noise"""
    import torch
    sp, g, net = case["sp"], case["g"], case["net"]
    nat, lt = make(sp, E0, net)
    ens = es.build(sp, case["sts"])
    x0 = {n: getattr(ens, n).clone() for n in es.PROG}
    tr = spectra(case["truth_state"])

    def cycle():
        nat.set_state(*tr)
        nat.observe(lt, 1.0)
        ens.verify(lt, nat, 0)
        ens.analyse(lt)
        ens.verify(lt, nat, 1)

    cycle()
    eager = nat.field("scores").numpy()
    eager_value = lt.field("value").numpy()
    nat.observe(lt, 0.0)
    h = lt.field("value").numpy()
    nat.reset(SEED)
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            cycle()
        slot1 = []
        for r in range(3):
            for n in es.PROG:
                getattr(ens, n).copy_(x0[n])
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            got = nat.field("scores").numpy()
            assert support.same_bits(got[0], eager[0]), r
            slot1.append(got[1])
            if r == 0:
                assert support.same_bits(got[1], eager[1]) and support.same_bits(lt.field("value").numpy(), eager_value)
        assert nat.draws() == 3
        z, ref = (lt.field("value").numpy() - h) / net["error"], nt.draw(SEED, 2, NOBS)
        worst = float(np.max(np.abs(z - ref) / noise_limit(ref, h, net["error"])))
        print("[nature capture] draw 2 of the third replay: error / limit %.3f" % worst)
        assert worst <= 1.0
        assert not support.same_bits(slot1[0], slot1[1]) and not support.same_bits(slot1[1], slot1[2])
        gr.close()
    finally:
        sp.use_torch_stream()
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 8. the twin condition
def test_twin_condition_on_the_device():
    """The inputs of tests/test_nature_cpu.py's twin test through observe, Letkf.analyse_grid and the device scores.  The values
    are the restatement's within the noise limit.  The background scores match the restatement's within the lk.limits of the scores.
    The analysis side: the device's increments are held to the restatement's (fed the device's own values) by tests/
    test_gpu_letkf.py's limit L_v per variable; a change of every member's error by at most L moves mbar by at most L, so rmse and
    bias by at most L (the weights sum to 1), and the deviations d_e - mbar by at most 2 L, so spread by at most 2 sqrt(E / (E -
    1)) L <= 3 L; those are added to the scores' own lk.limits.  And the analysis' rmse of t and ps is below the background's."""
    import speedy_f90_amd as s
    c = nt.TWIN
    kx, E = c["kx"], c["E"]
    sp = s.Spectral("t30", kx=kx, max_batch=64, device=0)
    sp.set_sigma(nt.twin_sigma(kx))
    g, w = lk.Geometry(sp), nt.gaussian_weights(sp)
    truth, x, net = nt.twin_inputs(g)
    nat = s.Nature(sp, seed=c["noise_seed"], capacity=2)
    nat.field("truth").upload(nt.rows(truth))
    lt = s.Letkf(sp, E, c["nobs"], c["sigma_h"], c["sigma_v"], c["rho"])
    lt.set_obs(*lk.args(net))
    nat.observe(lt, 1.0)
    value = lt.field("value").numpy()
    h, zref = nt.operator(g, truth, net), nt.draw(c["noise_seed"], 0, c["nobs"])
    assert float(np.max(np.abs((value - h) / net["error"] - zref) / noise_limit(zref, h, net["error"]))) <= 1.0
    xd = [support.dev(x[v]) for v in lk.VARS]
    nat.verify_grid(*xd, slot=0)
    inc = lt.analyse_grid(*xd)
    nat.verify_grid(*[a + b for a, b in zip(xd, inc)], slot=1)
    got = nat.field("scores").numpy()
    # the restatement, fed the device's values
    obs = dict(net)
    obs["value"] = value
    C, b = lk.problems(g, obs, lk.obs_space(g, x, obs), c["sigma_h"], c["sigma_v"])
    lim, ref_inc, kappa = lk.limits(g, x, C, b, c["rho"], np.arange(g.ix * g.il), E)
    worst = {v: float(np.max(np.abs(lk.at_columns(a.cpu().numpy(), np.arange(g.ix * g.il)) - ref_inc[v]))) / lim[v]
             for v, a in zip(lk.VARS, inc)}
    print("[nature twin, device] kappa %.1f, increments / limit: %s" % (kappa, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    rel, bias_abs = score_limits(g, x, truth, w, E)
    compare_scores("twin background", got[0], nt.flat(nt.scores(g, x, truth, w)), rel, bias_abs)
    xa = nt.analysed(x, ref_inc, g)
    want = nt.flat(nt.scores(g, xa, truth, w))
    rel_a, bias_a = score_limits(g, xa, truth, w, E)
    L = np.concatenate([np.full(kx if v != "ps" else 1, lim[v]) for v in lk.VARS])
    r = {"rmse": np.max(np.abs(got[1][0] - want[0]) / (rel_a * want[0] + L)), "bias": np.max(np.abs(got[1][1] - want[1]) / (bias_a + L)),
         "spread": np.max(np.abs(got[1][2] - want[2]) / (rel_a * want[2] + 3 * L))}
    print("[nature scores twin analysis] error / limit: %s" % " ".join("%s %.2e" % kv for kv in r.items()))
    assert max(r.values()) <= 1.0, r
    t, ps = slice(2 * kx, 3 * kx), 4 * kx
    print("[nature twin, device] rmse analysis / background: t %s, ps %.3f" % (np.round(got[1][0][t] / got[0][0][t], 3), got[1][0][ps] / got[0][0][ps]))
    assert (got[1][0][t] < got[0][0][t]).all() and got[1][0][ps] < got[0][0][ps]
    nat.close(); lt.close(); sp.close()
