"""GPU: adaptive inflation (include/spdy.h, "adaptive inflation"; Letkf.set_adaptive_inflation).  The estimate's two
kernels against the NumPy restatement of tests/letkfinfl.py, fed with the device's own y, departure, 1 / error^2 and ln sigma_o: s2
bit for bit, the sums within the restatement's absolute bound, the update bit for bit from the device's own sums.  The transform
under a field against the feature-off object with that scalar, on every route; the member mask; a captured cycle that advances the
field by itself; a twin experiment of three cycles.  T30; the section "on the T63 L16 grid" holds the sums, the update and the
transform under a field to the same statements at 192 x 96 x 16."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfinfl as li
import letkfmask as lm
import letkfpressure as lp
import letkfqc as qc
import letkfslots as ls
import levels
import support
import twincycle as tc

pytestmark = pytest.mark.gpu

SIGMA_V = 0.1
RHO0 = 1.3


T63 = "t63k16"


def _plan(tag, nmem):
    """tag: a variant's, or "t30" at a level count of its own on tests/levels.py's sigma as ("t30", kx)"""
    if isinstance(tag, tuple):
        sp = levels.plan(tag[0], tag[1], nmem * (4 * tag[1] + 4))
    else:
        sp = support.ensemble_plan(tag, nmem)
    return sp, lp.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


@pytest.fixture(scope="module")
def big(plans):
    """(E, tag) -> (the ensemble, 700 observations: the operator's edge cases, the sparse set and a cluster); made once, never changed"""
    made = {}

    def get(E, tag="t30"):
        if (E, tag) not in made:
            _, g = plans(tag)
            x = lk.ensemble(g, E, seed=80 + E)
            made[(E, tag)] = (x, lk.subset(lk.concat(lk.edge_obs(g, x), lk.sparse_obs(g, x), lk.clustered_obs(g, x, n=700)), slice(0, 700)))
        return made[(E, tag)]
    return get


STATE = ("rho", "infl_parm", "obs_s2")


def state(lt):
    """the block's three arrays, downloaded"""
    return {n: lt.field(n).numpy() for n in STATE}


def analyse(lt, x, **how):
    """lk.run with the block's three arrays, adaptive inflation on or off, and the field before the call"""
    before = lt.field("rho").numpy()
    return dict(lk.run(lt, x, names=STATE, **how), before=before)


def against_restatement(tag, g, lt, got, sigma_h, sigma_v, sigma_b, bounds=(li.RHO_MIN, li.RHO_MAX), keep=None, reff_field=False, cols=None):
    """obs_s2 to the bit, infl_parm within the bound, rho' from the device's own infl_parm and the prior field to the bit -> the
    worst ratio of a sum's error to its bound.  cols: the restatement's sums, the costly part, at these grid columns only (the
    update and obs_s2 are held everywhere)"""
    before, parm = got["before"].reshape(g.kx, -1), got["infl_parm"].reshape(3, g.kx, -1)
    if cols is not None:
        before, parm = before[:, cols], parm[:, :, cols]
    s2o, p, lim, _ = li.restate(g, lt, before, sigma_h, sigma_v, sigma_b, *bounds, keep=keep, reff_field=reff_field, cols=cols)
    assert support.same_bits(got["obs_s2"], s2o), tag
    worst = li.worst_ratio(parm, p, lim)
    print("[letkf infl] %s: worst error of a sum / bound %.3g" % (tag, worst))
    assert worst <= 1.0, (tag, worst)
    assert support.same_bits(got["rho"], li.update(got["before"], got["infl_parm"], sigma_b, *bounds)), tag
    return worst


# ---------------------------------------------------------------------------------------------------- 1. the sums
def sums(tag, sp, g, E, x, obs, cols=None):
    """sigma_v = 0 and 0.1 in turn on one object: the second call starts from the field the first one left; an empty network leaves
    exact zeros and the field's bits"""
    nobs = len(obs["var"])
    lt = lk.make(sp, E, obs, 0.0)
    lt.set_adaptive_inflation(0.5)
    assert (lt.field("rho").numpy() == lk.RHO).all()
    for sigma_v in (0.0, SIGMA_V):
        lt.set_localization(lk.SIGMA_H, sigma_v, 7.0)        # the scalar is not read, and setting it leaves the field alone
        got = analyse(lt, x)
        if nobs == 0:
            assert lm.zero_bits(got["infl_parm"]) and support.same_bits(got["rho"], got["before"])
            continue
        against_restatement("%sE=%d nobs=%d sigma_v=%g" % (tag, E, nobs, sigma_v), g, lt, got, lk.SIGMA_H, sigma_v, 0.5, cols=cols)
        assert not support.same_bits(got["rho"], got["before"]) and (got["infl_parm"][2] > 0.0).any()
    lt.close()


@pytest.mark.parametrize("nobs", [0, 1, 255, 256, 257, 700])
@pytest.mark.parametrize("E", [2, 3, 5, 32])
def test_sums(E, nobs, plans, big):
    """kx = 8: `sums`.  nobs: the edges of the scan's chunk of 256 and a network of more than two chunks"""
    sp, g = plans()
    x, all_obs = big(E)
    sums("", sp, g, E, x, lk.subset(all_obs, slice(0, nobs)))


@pytest.mark.parametrize("kx,E", [(5, 4), (7, 4), (15, 4), (20, 4), (32, 2)])
def test_sums_level_classes(kx, E, plans):
    """the level counts of tests/test_gpu_letkf.py's classes and 32, the most: lane k < kx carries level k"""
    sp, g = plans({5: "t30k5", 8: "t30"}.get(kx, ("t30", kx)), E)
    x = lk.ensemble(g, E, seed=kx)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_adaptive_inflation(0.5)
    got = analyse(lt, x)
    assert got["rho"].shape == (kx,) + sp.grid_shape and got["infl_parm"].shape == (3, kx) + sp.grid_shape
    against_restatement("kx=%d" % kx, g, lt, got, lk.SIGMA_H, SIGMA_V, 0.5)
    assert all((got["infl_parm"][2, k] > 0.0).any() for k in range(kx))
    lt.close()


@pytest.mark.parametrize("pattern", ["front256", "wave3", "hole"])
def test_sums_padded_scans(pattern, plans):
    """tests/letkf.py's padded patterns: a first chunk without a survivor, survivors in a chunk's last wave only, a whole chunk
    without one in the middle"""
    sp, g = plans("t30k5", 3)
    E = 3
    x = lk.ensemble(g, E, seed=31)
    real, pad = lk.padded_inputs(g, x)
    obs, _ = lk.interleave(real, pad, pattern)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_adaptive_inflation(0.5)
    got = analyse(lt, x)
    against_restatement(pattern, g, lt, got, lk.SIGMA_H, SIGMA_V, 0.5)
    lt.close()


def sums_edge_columns(tag, sp, g, edge_only=False):
    """the edge columns and edge observations of tests/letkf.py's edge_inputs at EDGE_SIGMA_H: polar rows, the periodic wrap, edge
    columns out of range of everything, which keep rho's bits.  edge_only: the restatement's sums are formed at the edge columns only"""
    E = 3
    x = lk.ensemble(g, E, seed=32)
    obs, cols, out = lk.edge_conditions(g, lk.edge_inputs(g, x))
    lt = lk.make(sp, E, obs, SIGMA_V, sigma_h=lk.EDGE_SIGMA_H)
    lt.set_adaptive_inflation(0.5)
    got = analyse(lt, x)
    against_restatement(tag + "edge columns", g, lt, got, lk.EDGE_SIGMA_H, SIGMA_V, 0.5, cols=cols if edge_only else None)
    rho, before = got["rho"].reshape(g.kx, -1), got["before"].reshape(g.kx, -1)
    assert support.same_bits(np.ascontiguousarray(rho[:, cols[out]]), np.ascontiguousarray(before[:, cols[out]]))
    assert (got["infl_parm"].reshape(3, g.kx, -1)[2][:, cols[~out]] > 0.0).any(axis=0).all()
    lt.close()


def test_sums_edge_columns(plans):
    """kx = 5: `sums_edge_columns`"""
    sp, g = plans("t30k5", 3)
    sums_edge_columns("", sp, g)


# ---------------------------------------------------------------------------------------------------- 2. the update
def test_update(plans, big):
    """rho' from the device's own infl_parm and the prior field, bit for bit: items with p3 == 0 keep rho's bits; bounds close
    around the prior are hit at both ends; sigma_b = 0 leaves every bit; an observation whose value is NaN (set through the value
    array) leaves rho as it is wherever it acts, and the field finite everywhere"""
    sp, g = plans()
    E = 5
    x, obs = big(E)
    lt = lk.make(sp, E, obs, SIGMA_V)
    lt.set_adaptive_inflation(10.0, 1.05, 1.2)
    got = analyse(lt, x)
    assert support.same_bits(got["rho"], li.update(got["before"], got["infl_parm"], 10.0, 1.05, 1.2))
    idle = got["infl_parm"][2] == 0.0
    assert idle.any() and (~idle).any() and support.same_bits(got["rho"][idle], got["before"][idle])
    assert (got["rho"] == 1.05).any() and (got["rho"] == 1.2).any() and (got["before"] == lk.RHO).all()
    lt.set_adaptive_inflation(0.0, 1.05, 1.2)
    frozen = analyse(lt, x)
    assert support.same_bits(frozen["rho"], frozen["before"]) and support.same_bits(frozen["infl_parm"], got["infl_parm"])
    value = obs["value"].copy()
    nan_at = 400                                                 # of the cluster
    value[nan_at] = np.nan
    lt.field("value").upload(value)
    lt.set_adaptive_inflation(10.0, 0.5, 5.0)
    nan = analyse(lt, x)
    hit = np.isnan(nan["infl_parm"][0])
    assert hit.any() and (~hit).any() and np.isnan(lt.field("departure").numpy()[nan_at])
    assert support.same_bits(nan["rho"][hit], nan["before"][hit]) and np.isfinite(nan["rho"]).all()
    assert support.same_bits(nan["rho"], li.update(nan["before"], nan["infl_parm"], 10.0, 0.5, 5.0))
    assert not support.same_bits(nan["rho"][~hit], nan["before"][~hit])
    lt.close()


# ---------------------------------------------------------------------------------------------------- 3. the transform
def gross_errors(obs, every=7, size=40.0):
    out = dict(obs)
    out["value"] = obs["value"].copy()
    out["value"][::every] += size * obs["error"][::every]
    return out


def uniform_route(tag, g, lt, x, sigma_h=lk.SIGMA_H, keep=None, reff_field=False, cols=None, **how):
    """feature off with the scalar RHO0, then on with the field uniform at RHO0: the same increments in every bit; and the
    estimate of that call against the restatement"""
    lt.set_localization(sigma_h, SIGMA_V, RHO0)
    lt.set_adaptive_inflation(on=False)
    off = analyse(lt, x, **how)
    lt.set_localization(sigma_h, SIGMA_V, 1.0)                   # not read while the feature is on
    lt.set_adaptive_inflation(0.5)
    lt.fill_inflation(RHO0)
    on = analyse(lt, x, **how)
    assert (on["before"] == RHO0).all()
    assert support.same_bits(off["rho"], off["before"]), tag      # off: nothing of the block is written
    for v in lk.VARS:
        assert support.same_bits(on[v], off[v]), (tag, v)
    assert any(off[v].any() for v in lk.VARS) or (keep is not None and len(keep) < 2), tag
    if keep is None or len(keep) >= 2:
        against_restatement(tag, g, lt, on, sigma_h, SIGMA_V, 0.5, keep=keep, reff_field=reff_field, cols=cols)
    else:
        assert support.same_bits(on["rho"], on["before"]), tag   # n < 2: rho is untouched
    return on


def uniform_routes(tag, sp, g, E, x, obs, cols=None):
    """plain, masked (3 of 5 and one member), weight stride (2, 2), relaxed, slots, background check with rejections"""
    lt = lk.make(sp, E, obs, SIGMA_V)
    plain = uniform_route(tag + "plain", g, lt, x, cols=cols)
    for keep in ((0, 2, 3), (2,)):
        uniform_route(tag + "masked %s" % (keep,), g, lt, x, keep=keep, cols=cols, use=support.dev(np.array(lm.flags(E, keep), np.int32)))
    ls.observe_all(lt, [x] * 4, ls.FIRST(len(obs["var"])))
    slots = uniform_route(tag + "slots", g, lt, x, cols=cols, slots=True)
    for v in lk.VARS:
        assert support.same_bits(slots[v], plain[v]), v
    assert support.same_bits(slots["rho"], plain["rho"])
    lt.set_slots(None)
    lt.set_relaxation(0.3, 0.9)
    uniform_route(tag + "relaxed", g, lt, x, cols=cols)
    lt.set_relaxation()
    lt.set_weight_stride(2, 2)
    strided = uniform_route(tag + "weight stride", g, lt, x, cols=cols)
    assert support.same_bits(strided["rho"], plain["rho"])       # the estimate does not depend on where transforms are solved
    lt.close()
    bad = gross_errors(obs)
    lt = lk.make(sp, E, bad, SIGMA_V)
    lt.set_background_check(3.0)
    uniform_route(tag + "background check", g, lt, x, reff_field=True, cols=cols)
    assert (lt.field("obs_check").numpy() == qc.REJECTED).any()
    lt.close()


def test_transform_uniform_routes(plans, big):
    """kx = 8, E = 5: `uniform_routes`"""
    sp, g = plans()
    uniform_routes("", sp, g, 5, *big(5))


def test_transform_uniform_at_pressure(plans):
    sp, g = plans()
    E = 5
    x = lp.craft(g, E, 45)
    obs = lp.network(g, x)
    lt = lp.make(sp, E, obs, SIGMA_V)
    uniform_route("at pressure", g, lt, x, reff_field=True)
    assert (lt.field("obs_used").numpy() == 0.0).any()
    lt.close()


def patches(sp, g, E, x, obs, stride):
    """a field of three values in patches: every (column, level) has the bits of the feature-off object with that scalar; ps those
    of level kx-1's value; at a weight stride at the coarse columns"""
    lt = lk.make(sp, E, obs, SIGMA_V)
    if stride != (1, 1):
        lt.set_weight_stride(*stride)
    values = (1.0, 1.1, 1.45)
    ncol = g.ix * g.il
    which = (np.arange(ncol)[None, :] // 700 + np.arange(g.kx)[:, None]) % 3
    field = np.array(values)[which]
    refs = []
    for rho in values:
        lt.set_localization(lk.SIGMA_H, SIGMA_V, rho)
        refs.append(lk.run(lt, x))
    lt.set_adaptive_inflation(0.0)
    lt.inflation_field().upload(field.reshape((g.kx,) + sp.grid_shape))
    got = analyse(lt, x)
    assert support.same_bits(got["rho"].reshape(g.kx, -1), field)
    cols = np.arange(ncol) if stride == (1, 1) else lt.table("coarse_columns")
    for v in lk.VARS:
        a = got[v].reshape(E, -1, ncol)
        sel = which if v != "ps" else which[g.kx - 1:]
        for n in range(3):
            r = refs[n][v].reshape(E, -1, ncol)
            at = (sel == n)[:, cols]
            assert at.any() and support.same_bits(a[:, :, cols][:, at], r[:, :, cols][:, at]), (v, n)
        assert not support.same_bits(a, refs[0][v].reshape(E, -1, ncol)), v
    lt.close()


@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_transform_patches(stride, plans, big):
    """kx = 8, E = 5: `patches`"""
    sp, g = plans()
    patches(sp, g, 5, *big(5), stride)


# ---------------------------------------------------------------------------------------------------- 4. the mask
def test_mask(plans):
    """the n members in use get the field and the increments of an n-member object on the compacted ensemble, bit for bit, over two
    calls (the second reads the field the first left); with n < 2 rho is untouched"""
    sp, g = plans()
    E, keep = 5, (0, 2, 3)
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lambda g, xc: lk.concat(lk.clustered_obs(g, xc, n=300), lk.sparse_obs(g, xc)), SIGMA_V)
    use = support.dev(np.array(lm.flags(E, keep), np.int32))
    for o in (lt, ltc):
        o.set_adaptive_inflation(0.5)
    for call in range(2):
        got, ref = analyse(lt, x, use=use), analyse(ltc, xc)
        for n in ("rho", "infl_parm", "obs_s2"):
            assert support.same_bits(got[n], ref[n]), (call, n)
        for v in lk.VARS:
            assert support.same_bits(np.ascontiguousarray(got[v][list(keep)]), ref[v]) and ref[v].any(), (call, v)
        assert not support.same_bits(got["rho"], got["before"])
    one = analyse(lt, x, use=support.dev(np.array(lm.flags(E, (2,)), np.int32)))
    for n in ("infl_parm", "obs_s2"):
        assert support.same_bits(one[n], got[n]), n
    assert support.same_bits(one["rho"], one["before"])
    lt.close(); ltc.close()


# ---------------------------------------------------------------------------------------------------- 5. capture
def test_capture(plans, oracle_factory):
    """A captured Ensemble.analyse replayed three times, each on the restored background, equals three eager calls in every bit of
    rho and of the state: the graph advances the field by itself.  It has two nodes more than the feature-off capture, which has
    the five of tests/test_gpu_letkf.py again after set_adaptive_inflation(on=False)"""
    import torch
    sp, g = plans("t30k5", 3)
    E = 3
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    lt = lk.make(sp, E, lk.spread_obs(g, lk.oracle_grids(oracle_factory("t30k5"), sts), 20, seed=52), 0.1)
    lt.set_adaptive_inflation(0.5)
    background = {n: getattr(ens, n).clone() for n in es.PROG}

    def restore():
        for n in es.PROG:
            getattr(ens, n).copy_(background[n])

    eager = []
    for _ in range(3):
        restore()
        ens.analyse(lt)
        torch.cuda.synchronize()
        eager.append(({n: getattr(ens, n).clone() for n in es.PROG}, lt.field("rho").numpy()))
    assert not support.same_bits(eager[0][1], eager[1][1]) and not support.same_bits(eager[1][1], eager[2][1])
    lt.fill_inflation(lk.RHO)
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as on:
            ens.analyse(lt)
        lt.set_adaptive_inflation(on=False)
        with sp.graph_capture() as off:
            ens.analyse(lt)
        assert (on.num_nodes(), off.num_nodes()) == (7, 5)
        off.close()
        assert (lt.field("rho").numpy() == lk.RHO).all()         # a capture runs nothing
        for want_state, want_rho in eager:
            restore()
            torch.cuda.synchronize()
            on.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), want_state[n]), n
            assert support.same_bits(lt.field("rho").numpy(), want_rho)
        on.close()
    finally:
        sp.use_torch_stream()
    lt.close()


def test_names_are_valid_on_every_object(plans):
    """tests/test_gpu_plan_objects.py's rule for the new names: asking makes the block and leaves the feature off"""
    sp, g = plans("t30k5", 3)
    x = lk.ensemble(g, 3, seed=33)
    lt = lk.make(sp, 3, lk.sparse_obs(g, x), SIGMA_V, rho=1.25)
    assert lt.field("infl_parm").shape == (3, 5) + sp.grid_shape and lt.field("obs_s2").shape == (lt.nobs,)
    assert (lt.inflation_field().numpy() == 1.25).all() and lm.zero_bits(lt.field("infl_parm").numpy())
    assert lt.adaptive is None and lt.table("adaptive_inflation")[0] == 0.0
    before = lk.run(lt, x)
    assert (lt.field("rho").numpy() == 1.25).all() and lm.zero_bits(lt.field("infl_parm").numpy())
    lt.fill_inflation(2.0)                                       # off: the field is not read
    after = lk.run(lt, x)
    for v in lk.VARS:
        assert support.same_bits(before[v], after[v]), v
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. twin experiment
TWIN_SIGMA_B = 0.2


def test_twin_experiment(oracle_factory):
    """tests/test_gpu_twin_cycle.py's set-up (T30 L5, E = 12, 600 stations of u, v, t, ps), three cycles from rho0 = 1.  With about
    15 effective observations per item vo is about 0.13, so Miyoshi's sigma_b = 0.04 (vb = 0.0016) would move the field by one
    per cent of the way to the observed value per cycle; sigma_b = 0.2 (vb = 0.04, a gain near 0.2) makes three cycles move it
    visibly.  Every cycle: the sums against the restatement fed that cycle's device arrays, rho from them to the bit, rho finite
    and inside its bounds, and exactly rho0 wherever no observation reaches"""
    import speedy_f90_amd as s
    import torch
    sp = support.ensemble_plan(tc.TAG, tc.E)
    g = lp.Geometry(sp)
    truth0, members0 = tc.initial_states(oracle_factory(tc.TAG))
    ens, tru = es.build(sp, members0), es.build(sp, [truth0])
    ens.startup(tc.DELT)
    tru.startup(tc.DELT)
    for _ in range(tc.SPINUP):
        ens.step(2, 2, 2.0 * tc.DELT)
        tru.step(2, 2, 2.0 * tc.DELT)
    nat = s.Nature(sp, seed=tc.NOISE_SEED, capacity=3)
    blank = lk.make_obs([0] * tc.NOBS, [0] * tc.NOBS, [0.0] * tc.NOBS, [0.0] * tc.NOBS, [0.0] * tc.NOBS, [1.0] * tc.NOBS)
    lt = lk.make(sp, tc.E, blank, tc.SIGMA_V, 1.0, tc.SIGMA_H)
    lt.set_adaptive_inflation(TWIN_SIGMA_B)
    reached = None
    for cycle in range(3):
        for _ in range(tc.WINDOW):
            ens.step(2, 2, 2.0 * tc.DELT)
            tru.step(2, 2, 2.0 * tc.DELT)
        nat.set_state(*[tru.member(0)[n][0] for n in es.PROG])
        if cycle == 0:
            ens.verify(lt, nat, 0)
            lt.set_obs(*lk.args(tc.network(g, tc.gridded(lt.field("grid").numpy(), tc.E, sp.kx))))
            reached = (li.horizontal(g, lt.table("unit"), tc.SIGMA_H) != 0.0).any(axis=1)
            # 600 stations at c_h = 1 826 km reach every column of T30: the last assertion below then holds over an empty set here
            # (tests 1 and 3 make it over real ones: the edge columns out of range and the items with p3 == 0)
            print("[letkf infl] twin: %d of %d columns out of every station's range" % ((~reached).sum(), reached.size))
            assert reached.any()
        nat.observe(lt, 1.0)
        before = lt.field("rho").numpy()
        ens.analyse(lt)
        torch.cuda.synchronize()
        got = dict(state(lt), before=before)
        against_restatement("twin cycle %d" % cycle, g, lt, got, tc.SIGMA_H, tc.SIGMA_V, TWIN_SIGMA_B)
        rho = got["rho"].reshape(sp.kx, -1)
        assert np.isfinite(rho).all() and rho.min() >= li.RHO_MIN and rho.max() <= li.RHO_MAX
        assert (rho[:, ~reached] == 1.0).all() and not support.same_bits(got["rho"], before)
        print("[letkf infl] twin cycle %d: mean rho over the observed items per level %s"
              % (cycle, " ".join("%.4f" % v for v in rho[:, reached].mean(axis=1))))
        ens.startup(tc.DELT)                                     # the truth is stepped on alongside, as in tests/test_gpu_twin_cycle.py
    lt.close(); nat.close(); sp.close()


# ---------------------------------------------------------------------------------------------------- 7. on the T63 L16 grid
def compared_columns(g, obs):
    """where the restatement's sums are formed on the larger grid: the columns nearest to the observations, those at the edge of
    their range and some out of range (lk.columns_for), and every eighth edge column in range of an observation"""
    edge = lk.edge_columns(g)
    edge = edge[lk.in_range(g, obs, edge).any(axis=1)]
    return np.unique(np.concatenate([lk.columns_for(g, obs, lk.SIGMA_H, most=96), edge[::8]]))


@pytest.mark.parametrize("E", [3, 32])
def test_sums_t63(E, plans, big):
    """192 x 96 x 16, 700 observations: `sums` -- letkf_infl_kernel carries level k in lane k < 16"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    x, obs = big(E, T63)
    cols = compared_columns(g, obs)
    assert len(cols) >= 150
    sums("T63 L16 ", sp, g, E, x, obs, cols)


def test_sums_edge_columns_t63(plans):
    """192 x 96 x 16: `sums_edge_columns`"""
    sp, g = plans(T63)
    sums_edge_columns("T63 L16 ", sp, g, edge_only=True)


def test_transform_uniform_routes_t63(plans, big):
    """192 x 96 x 16, E = 5: `uniform_routes`"""
    sp, g = plans(T63)
    x, obs = big(5, T63)
    uniform_routes("T63 L16 ", sp, g, 5, x, obs, compared_columns(g, obs))


@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_transform_patches_t63(stride, plans, big):
    """192 x 96 x 16, E = 5: `patches`"""
    sp, g = plans(T63)
    patches(sp, g, 5, *big(5, T63), stride)
