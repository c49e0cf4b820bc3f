"""GPU: the background check and the observation statistics (include/spdy.h, "background check and observation statistics";
Letkf.set_background_check).  The check's kernel against the NumPy restatement of tests/letkfqc.py, fed with the
device's own y, departure and errors: decisions, fields and statistics bit for bit; the checked analysis against the unchecked one
of the network without the rejected observations; every route with its flags and one graph node more; off is off; the stats-only
call; a twin experiment with planted gross errors.  T30; the section "on the T63 L16 grid" holds the decisions, the statistics and
the checked analysis to the same statements at 192 x 96 x 16."""
import importlib.util
import json
import os

import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfmask as lm
import letkfpressure as lp
import letkfqc as qc
import letkfslots as ls
import support
import twincycle as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIGMA_V = 0.1
GROSS = 3.0


T63 = "t63k16"


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lp.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


@pytest.fixture(scope="module")
def big(plans):
    """(E, tag) -> (the ensemble, 2100 observations: the operator's edge cases, the sparse set and a cluster); made once, never changed"""
    made = {}

    def get(E, tag="t30"):
        if (E, tag) not in made:
            _, g = plans(tag)
            x = lk.ensemble(g, E, seed=60 + E)
            made[(E, tag)] = (x, lk.subset(lk.concat(lk.edge_obs(g, x), lk.sparse_obs(g, x), lk.clustered_obs(g, x, n=2100)), slice(0, 2100)))
        return made[(E, tag)]
    return get


CHECKED = ("y", "departure", "hxmean", "value", "obs_used", "obs_check", "obs_rinv")


def analyse(lt, x, out=None, **how):
    """lk.run with what the check read and wrote, and the statistics"""
    return dict(lk.run(lt, x, out=out, names=CHECKED, **how), stats=lt.obs_stats())


restated, table, same_decisions = qc.restated, qc.table, qc.same_decisions


# ---------------------------------------------------------------------------------------------------- 1. decisions and fields
@pytest.mark.parametrize("nobs", [0, 1, 255, 256, 257, 700, 1023, 1024, 1025, 2100])
@pytest.mark.parametrize("E", [2, 3, 5, 32])
def test_decisions_and_fields(E, nobs, plans, big):
    """obs_used, obs_check, obs_rinv and the statistics equal the restatement bit for bit on the device's own y and departure.  The
    values are planted at hxmean +- gross sqrt(v) (1 +- 1e-9) from a first call's hxmean and y, four per group: the ones outside
    are rejected, the ones inside pass.  One observation's value is NaN, set through the device's value array: it is not rejected
    and makes only its own group's sums NaN.  nobs: the edges of a chunk of 256, as the transform kernel scans, and of the check's
    own chunk of 1024, and a network of more than two chunks"""
    sp, g = plans()
    x, all_obs = big(E)
    obs = lk.subset(all_obs, slice(0, nobs))
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_background_check(GROSS)
    first = analyse(lt, x)
    if nobs == 0:
        assert not table(first["stats"]).view(np.int64).any() and first["t"].any()       # rho = 1.1: pure inflation, exact zero rows
        lt.close()
        return
    value, outside, inside = qc.plant(obs, first["hxmean"], qc.spread2(first["y"]), GROSS, seed=nobs + E)
    nan_at = -1
    if nobs >= 255:
        nan_at = int(np.setdiff1d(np.arange(nobs), np.concatenate([outside, inside]))[100])
        value[nan_at] = np.nan
    lt.field("value").upload(value)
    got = analyse(lt, x)
    dec, rows = restated(got, obs, GROSS)
    assert same_decisions(got, dec, obs)
    assert (got["obs_check"][outside] == qc.REJECTED).all() and (got["obs_check"][inside] == qc.PASSED).all()
    if nobs >= 255:
        assert len(outside) == len(inside) == 10 and got["obs_check"][nan_at] == qc.PASSED and np.isnan(got["departure"][nan_at])
        bad = np.isnan(table(got["stats"])).any(axis=1)
        assert bad.sum() == 1 and bad[obs["var"][nan_at]]
    assert qc.same_rows(table(got["stats"]), rows)
    assert table(got["stats"])[:, 0].sum() == nobs and table(got["stats"])[:, 2].sum() == (got["obs_check"] == qc.REJECTED).sum()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 2. takes no part
def analysis_without_the_rejected(sp, g, E, x, obs):
    """With the check on the increments on the grid equal, bit for bit, those of the unchecked call on the network with the rejected
    observations removed; the columns out of range of every rejected observation keep the unchecked call's bits, the others do not"""
    obs = dict(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_background_check(GROSS)
    first = analyse(lt, x)
    obs["value"], outside, _ = qc.plant(obs, first["hxmean"], qc.spread2(first["y"]), GROSS, seed=2)
    lt.field("value").upload(obs["value"])
    got = analyse(lt, x)
    rejected = got["obs_check"] == qc.REJECTED
    assert rejected[outside].all() and 10 <= rejected.sum() < 100
    without = lk.make(sp, E, lk.subset(obs, ~rejected), SIGMA_V)
    ref = lk.run(without, x)
    lt.set_background_check(0.0)
    plain = lk.run(lt, x)
    near = lk.in_range(g, lk.subset(obs, rejected)).any(axis=1)
    assert near.sum() >= 64 and (~near).sum() >= 64
    for v in lk.VARS:
        assert support.same_bits(got[v], ref[v]) and ref[v].any(), v
        assert support.same_bits(lk.at_columns(got[v], ~near), lk.at_columns(plain[v], ~near)), v
        assert not support.same_bits(lk.at_columns(got[v], near), lk.at_columns(plain[v], near)), v
    lt.close(); without.close()


def test_analysis_equals_the_analysis_without_the_rejected(plans, big):
    """E = 5: `analysis_without_the_rejected`"""
    sp, g = plans()
    analysis_without_the_rejected(sp, g, 5, *big(5))


# ---------------------------------------------------------------------------------------------------- 3. every route
def gross_errors(obs, every=7, size=40.0):
    """every `every`-th value moved by `size` errors: far outside any threshold used here"""
    out = dict(obs)
    out["value"] = obs["value"].copy()
    out["value"][::every] += size * obs["error"][::every]
    return out


def route(sp, lt, x, obs, in_column=None, keep=None, expect_rejections=True, **how):
    """One route: the eager checked call's flags against the restatement; the captured checked call has ONE node more than the
    captured unchecked one, and its replays leave the eager call's bits in the increments, the flags and the statistics"""
    import torch
    lt.set_background_check(GROSS)
    eager = analyse(lt, x, **how)
    dec, rows = restated(eager, obs, GROSS, in_column=in_column, keep=keep)
    assert same_decisions(eager, dec, obs), how
    assert qc.same_rows(table(eager["stats"]), rows), how
    assert bool((eager["obs_check"] == qc.REJECTED).any()) == expect_rejections
    xs = lk.grids(x)
    out = [torch.empty_like(a) for a in xs]
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        lt.set_background_check(0.0)
        with sp.graph_capture() as off:
            lt.analyse_grid(*xs, out=out, **how)
        nodes = off.num_nodes()
        off.close()
        lt.set_background_check(GROSS)
        with sp.graph_capture() as gr:
            lt.analyse_grid(*xs, out=out, **how)
        assert gr.num_nodes() == nodes + 1, (gr.num_nodes(), nodes, how)
        for _ in range(2):
            for a in out:
                a.fill_(-3.0)
            for name in ("obs_check", "obs_used", "obs_rinv"):
                f = lt.field(name)
                f.upload(np.full(f.shape, -3.0))
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for v, a in zip(lk.VARS, out):
                assert support.same_bits(a.cpu().numpy(), eager[v]), (how, v)
            for name in ("obs_check", "obs_used", "obs_rinv", "y", "departure"):
                assert support.same_bits(lt.field(name).numpy(), eager[name]), (how, name)
            assert qc.same_rows(table(lt.obs_stats()), rows), how
        gr.close()
    finally:
        sp.use_torch_stream()
    return eager, nodes


def test_route_masked(plans, big):
    """n = 3 of 5: the spread's sum and n are the mask's"""
    sp, g = plans()
    E, keep = 5, (0, 2, 3)
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    eager, _ = route(sp, lt, x, obs, keep=keep, use=support.dev(np.array(lm.flags(E, keep), np.int32)))
    full = analyse(lt, x)
    assert not support.same_bits(full["obs_rinv"], eager["obs_rinv"]) or not support.same_bits(full["y"], eager["y"])
    lt.close()


def test_route_one_member(plans, big):
    """n = 1: the test is not made, nothing is rejected, the increments are exactly zero"""
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    eager, _ = route(sp, lt, x, obs, keep=(2,), expect_rejections=False, use=support.dev(np.array(lm.flags(E, (2,)), np.int32)))
    assert (eager["obs_used"] == 1.0).all()
    for v in lk.VARS:
        assert lm.zero_bits(eager[v]), v
    lt.close()


def test_route_weight_stride(plans, big):
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_weight_stride(2, 2)
    _, nodes = route(sp, lt, x, obs)
    assert nodes == 3
    lt.close()


def test_route_relaxed(plans, big):
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_relaxation(0.3, 0.9)
    _, nodes = route(sp, lt, x, obs)
    assert nodes == 3
    lt.close()


def test_route_slots(plans, big):
    """three non-empty slots (and an empty one) observed on one ensemble: the finish kernel in the observation kernel's place, then
    the check"""
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    plain, _ = route(sp, lt, x, obs)
    ls.observe_all(lt, [x] * 4, ls.FIRST(len(obs["var"])))
    eager, nodes = route(sp, lt, x, obs, slots=True)
    assert nodes == 2
    for v in lk.VARS:
        assert support.same_bits(eager[v], plain[v]), v
    lt.close()


def test_route_at_pressure(plans):
    """a network with observations at a pressure: out of column wins over the check, and the count lands in n_out"""
    sp, g = plans()
    E = 5
    x = lp.craft(g, E, 45)
    obs = gross_errors(lp.network(g, x), every=3)
    lt = lp.make(sp, E, obs, SIGMA_V)
    in_column = lk.obs_space(g, x, obs)["obs_used"]
    eager, nodes = route(sp, lt, x, obs, in_column=in_column)
    assert nodes == 2
    out = in_column == 0.0
    assert out.sum() >= 10 and (eager["obs_check"][out] == qc.OUT).all() and (eager["obs_check"][~out] != qc.OUT).all()
    assert out[::3].any()                                  # a gross error that is out of column too: out of column wins
    assert table(eager["stats"])[:, 1].sum() == out.sum() and table(eager["stats"])[:, 2].sum() == (eager["obs_check"] == qc.REJECTED).sum() > 0
    lt.close()


# ---------------------------------------------------------------------------------------------------- 4. off is off
def test_off_is_off(plans, oracle_factory):
    """after set_background_check(0) a captured Ensemble.analyse has the five nodes tests/test_gpu_letkf.py asserts and an
    analyse_grid two, and tools/letkf_digest.py's digests of an object that had the check on and off again are the ones recorded
    for the parent commit's library (profiles/letkf_obsop_digests.json)"""
    import torch
    sp, g = plans("t30k5")
    E = 3
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    lt = lk.make(sp, E, lk.spread_obs(g, lk.oracle_grids(oracle_factory("t30k5"), sts), 20, seed=52), 0.1)
    lt.set_background_check(GROSS)
    ens.analyse(lt)
    torch.cuda.synchronize()
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as on:
            ens.analyse(lt)
        lt.set_background_check(0.0)
        with sp.graph_capture() as off:
            ens.analyse(lt)
        assert (on.num_nodes(), off.num_nodes()) == (6, 5)
        on.close(); off.close()
    finally:
        sp.use_torch_stream()
    assert (lt.field("obs_used").numpy() == 1.0).all()
    lt.close()
    spec = importlib.util.spec_from_file_location("letkf_digest", os.path.join(ROOT, "tools", "letkf_digest.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "profiles", "letkf_obsop_digests.json")) as f:
        recorded = json.load(f)["runs"][0]["digests"]
    sp8, g8 = plans()
    E = 5
    for kind, x, net, make in tool.networks(g8, E):
        lt = make(sp8, E, net, tool.SIGMA_V)
        lt.set_background_check(GROSS, np.arange(len(net["var"])) % 7)
        lk.run(lt, x)
        lt.set_background_check(0.0)
        assert tool.analysis(lt, x) == recorded["%s E=%d plain" % (kind, E)], kind
        lt.close()


# ---------------------------------------------------------------------------------------------------- 5. statistics
@pytest.mark.parametrize("ngroups", [1, 5, 64])
def test_statistics_rows(ngroups, plans, big):
    """rows for 1, 5 and 64 groups given by the caller, one group empty where there is more than one, with and without rejection:
    bit for bit the restatement's in the header's summation order"""
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    n = len(obs["var"])
    empty = ngroups // 2 if ngroups > 1 else -1
    groups = (np.arange(n) * 7 + obs["var"]) % ngroups
    groups = np.where(groups == empty, ngroups - 1, groups)
    lt = lk.make(sp, E, obs, SIGMA_V)
    for gross, slot in ((GROSS, 1), (0.0, 2)):
        lt.set_background_check(gross, groups, slot=slot)
        got = analyse(lt, x)
        dec, rows = restated(got, obs, gross, groups, ngroups)
        assert same_decisions(got, dec, obs)
        assert bool(dec["rej"].any()) == (gross > 0.0)
        assert table(got["stats"]).shape == (ngroups, 10) and qc.same_rows(table(got["stats"]), rows), (ngroups, gross)
        if empty >= 0:
            assert not table(got["stats"])[empty].view(np.int64).any()
        assert (table(got["stats"])[:, 0] > 0).sum() == ngroups - (empty >= 0)
    # the other slot's row is still there
    first = table(lt.obs_stats(1))
    assert first[:, 2].sum() > 0 and table(lt.obs_stats(2))[:, 2].sum() == 0
    lt.close()


def test_stats_only_call(plans, big):
    """Before any checked analysis the stats-only call is refused with SPDY_ERR_STATE.  After one it fills its row over the
    analysis' used set with dep the departure on the given state and dep_b the analysis' departure: on the analysed ensemble
    sum dep*dep_b is sum d_oa d_ob; obs_used and obs_check stay the analysis'; a new network needs a new analysis"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans()
    E = 5
    x, obs = big(E)
    obs = gross_errors(obs)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_background_check(GROSS)
    with pytest.raises(s.SpdyError) as err:
        lt.stats_grid(1, *lk.grids(x))
    assert err.value.code == -5 and "no analysis call with the check on" in str(err.value)
    got = analyse(lt, x)
    xa = {v: x[v] + got[v] for v in lk.VARS}
    lt.stats_grid(3, *lk.grids(xa))
    torch.cuda.synchronize()
    after = {n: lt.field(n).numpy() for n in ("y", "departure", "obs_used", "obs_check", "obs_rinv")}
    for name in ("obs_used", "obs_check", "obs_rinv"):
        assert support.same_bits(after[name], got[name]), name
    assert not support.same_bits(after["departure"], got["departure"])
    _, rows = restated(after, obs, GROSS, depb=got["departure"], code=got["obs_check"])
    oa = table(lt.obs_stats(3))
    assert qc.same_rows(oa, rows) and qc.same_rows(table(lt.obs_stats(0)), table(got["stats"]))
    used = got["obs_check"] == qc.PASSED
    prod = after["departure"][used] * got["departure"][used]
    assert abs(oa[:, 8].sum() - float(np.sum(prod))) <= used.sum() * lk.EPS * np.abs(prod).sum()
    assert (oa[:, 5] < table(got["stats"])[:, 5]).all()      # the analysis fits the used observations better than the background
    lt.set_obs(*lk.args(obs))
    with pytest.raises(s.SpdyError):
        lt.stats_grid(3, *lk.grids(xa))
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. twin experiment
def test_twin_experiment(oracle_factory):
    """tests/test_gpu_twin_cycle.py's set-up (T30 L5, E = 12, 600 stations): after the spin-up and one window's forecast
    Nature.observe draws the network, a seeded 2 % of the values are shifted on the device by 10 sqrt(v_o), and the same background
    is analysed with gross = 5 and without.  On the restatement alone (checked first): every shifted observation is rejected and no
    other.  Then the device agrees, and the checked analysis' rmse is below the unchecked one's in every observed variable"""
    import speedy_f90_amd as s
    import torch
    sp = support.ensemble_plan(tc.TAG, tc.E)
    g = lp.Geometry(sp)
    truth0, members0 = tc.initial_states(oracle_factory(tc.TAG))
    ens, tru = es.build(sp, members0), es.build(sp, [truth0])
    ens.startup(tc.DELT)
    tru.startup(tc.DELT)
    for _ in range(tc.SPINUP + tc.WINDOW):
        ens.step(2, 2, 2.0 * tc.DELT)
        tru.step(2, 2, 2.0 * tc.DELT)
    nat = s.Nature(sp, seed=tc.NOISE_SEED, capacity=3)
    nat.set_state(*[tru.member(0)[n][0] for n in es.PROG])
    blank = lk.make_obs([0] * tc.NOBS, [0] * tc.NOBS, [0.0] * tc.NOBS, [0.0] * tc.NOBS, [0.0] * tc.NOBS, [1.0] * tc.NOBS)
    lt = lk.make(sp, tc.E, blank, tc.SIGMA_V, tc.RHO, tc.SIGMA_H)
    ens.verify(lt, nat, 0)
    x = tc.gridded(lt.field("grid").numpy(), tc.E, sp.kx)
    net = tc.network(g, x)
    lt.set_obs(*lk.args(net))
    nat.observe(lt, 1.0)
    value = lt.field("value").numpy()
    # the restatement alone, on the host's own operator
    space = lk.obs_space(g, x, net)
    hxmean, Y = space["hxmean"], space["y"]
    v = qc.spread2(Y) + net["error"] * net["error"]
    shifted = np.zeros(tc.NOBS, bool)
    shifted[np.random.default_rng(27).choice(tc.NOBS, tc.NOBS // 50, replace=False)] = True
    value = np.where(shifted, value + 10.0 * np.sqrt(v), value)
    dec = qc.check(Y, value - hxmean, net["error"], 5.0)
    ratio = (value - hxmean) ** 2 / v
    print("[letkf qc twin] dep^2 / v: largest unshifted %.2f, smallest shifted %.2f (threshold 25)" % (ratio[~shifted].max(), ratio[shifted].min()))
    assert (dec["check"][shifted] == qc.REJECTED).all() and (dec["check"][~shifted] == qc.PASSED).all() and shifted.sum() == 12
    lt.field("value").upload(value)
    background = {n: getattr(ens, n).clone() for n in es.PROG}
    rmse = {}
    for tag, gross in (("checked", 5.0), ("unchecked", 0.0)):
        for n in es.PROG:
            getattr(ens, n).copy_(background[n])
        lt.set_background_check(gross)
        ens.analyse(lt)
        if gross:
            torch.cuda.synchronize()
            assert support.same_bits(lt.field("obs_check").numpy(), dec["check"])
            st = lt.obs_stats()
            assert st["n_rej"].sum() == 12 and st["n_used"].sum() == tc.NOBS - 12 and st["n_all"][lk.Q] == 0
        ens.verify(lt, nat, 1)
        rmse[tag] = nat.scores(1)["rmse"]
    for n in es.PROG:
        getattr(ens, n).copy_(background[n])
    ens.verify(lt, nat, 2)
    rmse["background"] = nat.scores(2)["rmse"]
    mean = lambda r, name: float(np.mean(np.atleast_1d(r[name])))
    for name in ("u", "v", "t", "ps"):
        c, u, b = (mean(rmse[k], name) for k in ("checked", "unchecked", "background"))
        print("[letkf qc twin] %s: rmse checked / unchecked %.3f, checked / background %.3f, unchecked / background %.3f" % (name, c / u, c / b, u / b))
        assert c < u, (name, c, u)
    lt.close(); nat.close(); sp.close()


# ---------------------------------------------------------------------------------------------------- 7. on the T63 L16 grid
@pytest.mark.parametrize("nobs", [1023, 1024, 1025, 2100])
@pytest.mark.parametrize("E", [3, 32])
def test_decisions_and_fields_t63(E, nobs, plans, big):
    """192 x 96 x 16, nobs at the edges of the check's own chunk of 1024 and above two of them, five groups given by the caller of
    which group 2 is empty: obs_used, obs_check, obs_rinv and the statistics equal the restatement bit for bit on the device's own y
    and departure, with values planted on both sides of the threshold in every non-empty group and one NaN value, as in
    test_decisions_and_fields; the empty group's row is all +0.0"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    x, all_obs = big(E, T63)
    obs = lk.subset(all_obs, slice(0, nobs))
    groups = (np.arange(nobs) * 7 + obs["var"]) % 5
    groups = np.where(groups == 2, 4, groups)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_background_check(GROSS, groups)
    first = analyse(lt, x)
    value, outside, inside = qc.plant(obs, first["hxmean"], qc.spread2(first["y"]), GROSS, seed=nobs + E, groups=groups)
    nan_at = int(np.setdiff1d(np.arange(nobs), np.concatenate([outside, inside]))[100])
    value[nan_at] = np.nan
    lt.field("value").upload(value)
    got = analyse(lt, x)
    dec, rows = restated(got, obs, GROSS, groups, 5)
    assert same_decisions(got, dec, obs)
    assert (got["obs_check"][outside] == qc.REJECTED).all() and (got["obs_check"][inside] == qc.PASSED).all()
    assert len(outside) == len(inside) == 8 and got["obs_check"][nan_at] == qc.PASSED and np.isnan(got["departure"][nan_at])
    stats = table(got["stats"])
    bad = np.isnan(stats).any(axis=1)
    assert bad.sum() == 1 and bad[groups[nan_at]]
    assert stats.shape == (5, 10) and qc.same_rows(stats, rows)
    assert not stats[2].view(np.int64).any() and (stats[:, 0] > 0).sum() == 4
    assert stats[:, 0].sum() == nobs and stats[:, 2].sum() == (got["obs_check"] == qc.REJECTED).sum()
    lt.close()


@pytest.mark.parametrize("E", [3, 32])
def test_analysis_without_the_rejected_t63(E, plans, big):
    """192 x 96 x 16, 2 100 observations: `analysis_without_the_rejected`"""
    sp, g = plans(T63)
    analysis_without_the_rejected(sp, g, E, *big(E, T63))
