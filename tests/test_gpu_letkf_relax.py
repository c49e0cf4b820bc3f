"""GPU: relaxation to the prior perturbations and spread (include/spdy.h, "relaxation"; Letkf.set_relaxation).
The kernel against the NumPy restatement of tests/letkfrelax.py, fed with the raw increments the same object gives at (0, 0), which
are bit-reproducible; the three statements the header calls exact; the weight-interpolated route, aliased outputs and an empty
network; the member mask against the object of the members in use; an Ensemble's state; a captured analysis.  T30; the section "on
the T63 L16 grid" holds the kernel, the weight-interpolated route and the aliased call to the same rules at 192 x 96 x 16."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfmask as lm
import letkfrelax as lr
import support

pytestmark = pytest.mark.gpu

SIGMA_V = 0.1


T63 = "t63k16"


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lk.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


def both_sets(g, x):
    return (("clustered", lk.clustered_obs(g, x)), ("sparse", lk.sparse_obs(g, x)))


def mixed(g, x):
    return lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))


# ---------------------------------------------------------------------------------------------------- 1. against the restatement
def kernel_against_restatement(tag, sp, g, E, sets):
    """sigma_v = 0.1, (rtpp, rtps) = (0.5, 0), (0, 0.9), (0.3, 0.9): the relaxed increments at every column against `relax` of the
    object's own raw increments, within 64 E eps max|x| max(1, f) per item -- the increment bound of DESIGN.md s18 times the factor
    that multiplies the rounding of b_e -- and the inflation field against f at 64 E eps"""
    x = lk.ensemble(g, E, seed=E)
    worst, fmax = 0.0, 0.0
    for name, obs in sets(g, x):
        lt = lk.make(sp, E, obs, SIGMA_V)
        raw = lk.run(lt, x)
        for rtpp, rtps in lr.SETTINGS:
            lt.set_relaxation(rtpp, rtps)
            got = lk.run(lt, x)
            infl = got["inflation"]
            w, f = lr.compare(x, raw, got, infl, rtpp, rtps, E)
            print("[letkf relax %s %s rtpp=%.1f rtps=%.1f] ratio to the limit %.2e, largest f %.3f" % (tag, name, rtpp, rtps, w, f))
            assert any(not support.same_bits(got[v], raw[v]) for v in lk.VARS), (name, rtpp, rtps)
            worst, fmax = max(worst, w), max(fmax, f)
        lt.close()
    print("[letkf relax %s] largest ratio to the limit %.2e, largest f %.3f" % (tag, worst, fmax))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("E,kx", [(2, 8), (3, 8), (17, 8), (32, 8), (32, 5)])
def test_kernel_against_restatement(E, kx, plans):
    """the clustered and the sparse set: `kernel_against_restatement`"""
    sp, g = plans({5: "t30k5", 8: "t30"}[kx])
    kernel_against_restatement("E=%d kx=%d" % (E, kx), sp, g, E, both_sets)


# ---------------------------------------------------------------------------------------------------- 2. the exact statements
def test_untouched_columns_keep_their_bits(plans):
    """rho = 1, the clustered set: at the columns farther than 2 c_h (1 + 1e-12) from every observation the relaxed increments
    are +0.0 in every bit and inflation is exactly 1.0; in range of the cluster the ensemble has been drawn together and f > 1"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=E)
    obs = lk.clustered_obs(g, x)
    far = lk.distance(g.colunit, lk.unit(obs["lon"], obs["lat"])).min(axis=1) > 2.0 * lk.C_H * (1.0 + 1e-12)
    near = lk.in_range(g, obs).any(axis=1)
    assert far.sum() >= 4000 and near.sum() >= 64, (far.sum(), near.sum())
    lt = lk.make(sp, E, obs, SIGMA_V, rho=1.0)
    for rtpp, rtps in lr.SETTINGS + ((1.0, 1.0),):
        lt.set_relaxation(rtpp, rtps)
        got = lk.run(lt, x)
        infl = got["inflation"]
        for v in lk.VARS:
            assert lm.zero_bits(lk.at_columns(got[v], far)), (rtpp, rtps, v)
            assert lk.at_columns(got[v], near).any(), (rtpp, rtps, v)
        assert (lk.at_columns(infl, far) == 1.0).all(), (rtpp, rtps)
        assert rtps == 0.0 or rtpp == 1.0 or (lk.at_columns(infl, near) > 1.0).any(), (rtpp, rtps)
    lt.close()


@pytest.mark.parametrize("E", [3, 32])
def test_rtpp_one_moves_only_the_mean(E, plans):
    """rtpp = 1, with and without rtps: every member's increments have the bits of member 0's, and inflation is exactly 1.0"""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=E)
    lt = lk.make(sp, E, mixed(g, x), SIGMA_V)
    for rtps in (0.0, 0.9):
        lt.set_relaxation(1.0, rtps)
        got = lk.run(lt, x)
        infl = got["inflation"]
        for v in lk.VARS:
            assert lr.same_bits_everywhere(got[v]) and got[v].any(), (rtps, v)
        assert (infl == 1.0).all(), rtps
    lt.close()


def test_both_zero_is_the_analysis_it_was(plans):
    """(0, 0) after a setting that allocated the workspace and ran: the bits of an object that never had one"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=E)
    obs = mixed(g, x)
    never, lt = lk.make(sp, E, obs, SIGMA_V), lk.make(sp, E, obs, SIGMA_V)
    ref = lk.run(never, x)
    lt.set_relaxation(0.3, 0.9)
    relaxed = lk.run(lt, x)
    lt.set_relaxation(0.0, 0.0)
    got = lk.run(lt, x)
    for v in lk.VARS:
        assert support.same_bits(got[v], ref[v]) and not support.same_bits(relaxed[v], ref[v]), v
    never.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 3. routes
def weight_stride(tag, sp, g):
    """stride (2, 2), E = 17: the apply kernel's raw increments go through the same relaxation"""
    E = 17
    x = lk.ensemble(g, E, seed=E)
    lt = lk.make(sp, E, mixed(g, x), SIGMA_V)
    lt.set_weight_stride(2, 2)
    raw, got, infl = lr.raw_and_relaxed(lt, x, 0.3, 0.9)
    w, f = lr.compare(x, raw, got, infl, 0.3, 0.9, E)
    print("[letkf relax %sstride (2, 2) E=17] ratio to the limit %.2e, largest f %.3f" % (tag, w, f))
    assert w <= 1.0, w
    lt.close()


def test_weight_stride(plans):
    """kx = 8: `weight_stride`"""
    sp, g = plans()
    weight_stride("", sp, g)


def outputs_may_be_the_inputs(sp, g, stride):
    """analyse_grid with out = the input tensors: the bits of the call that does not alias"""
    import torch
    E = 17
    x = lk.ensemble(g, E, seed=E)
    lt = lk.make(sp, E, mixed(g, x), SIGMA_V)
    lt.set_weight_stride(*stride)
    lt.set_relaxation(0.3, 0.9)
    ref = lk.run(lt, x)
    finf = ref["inflation"]
    xs = [support.dev(x[v]) for v in lk.VARS]
    lt.analyse_grid(*xs, out=xs)
    torch.cuda.synchronize()
    for v, a in zip(lk.VARS, xs):
        assert support.same_bits(a.cpu().numpy(), ref[v]) and ref[v].any(), v
    assert support.same_bits(lt.field("inflation").numpy(), finf)
    lt.close()


@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_outputs_may_be_the_inputs(stride, plans):
    """kx = 8, E = 17: `outputs_may_be_the_inputs`"""
    sp, g = plans()
    outputs_may_be_the_inputs(sp, g, stride)


def test_rtps_one_takes_pure_inflation_back(plans):
    """no observation, rho = 1.21, rtps = 1: the raw increments are a tenth of the perturbations, the relaxed ones zero within
    the increments' bound"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=E)
    lt = lk.make(sp, E, lk.make_obs([], [], [], [], [], []), SIGMA_V, rho=1.21)
    raw, got, infl = lr.raw_and_relaxed(lt, x, 0.0, 1.0)
    _, f = lr.relax(x, raw, 0.0, 1.0)
    for v in lk.VARS:
        assert np.max(np.abs(raw[v])) > 0.05 * lk.perturbation_scale(x)[v], v
        ratio = float(np.max(np.abs(got[v]) / lr.limit(x, f, E, v)[None]))
        print("[letkf relax nobs=0 rho=1.21 rtps=1] %s: ratio to the limit %.2e" % (v, ratio))
        assert ratio <= 1.0, (v, ratio)
    assert np.max(np.abs(infl - 1.0 / 1.1)) <= 64 * E * lk.EPS
    lt.close()


# ---------------------------------------------------------------------------------------------------- 4. the member mask
MASKS = [(8, tuple(range(7))), (32, tuple(e for e in range(32) if e != 13)), (32, (2, 30))]


@pytest.mark.parametrize("E,keep", MASKS, ids=["E8-drop7", "E32-drop13", "E32-keep2,30"])
def test_masked_equals_compact(E, keep, plans):
    """the masked relaxed call equals, bit for bit, the relaxed call of the n-member object on the compacted ensemble, in the
    increments and in inflation; the members not in use hold exactly 0.0; NaN in them changes no bit anywhere"""
    sp, g = plans()
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, mixed, SIGMA_V)
    drop = [e for e in range(E) if e not in keep]
    for rtpp, rtps in ((0.3, 0.9), (0.0, 0.9)):
        lt.set_relaxation(rtpp, rtps)
        ltc.set_relaxation(rtpp, rtps)
        got = lk.run(lt, x, lm.flags(E, keep))
        infl = got["inflation"]
        ref = lk.run(ltc, xc)
        finf = ref["inflation"]
        for v in lk.VARS:
            assert support.same_bits(np.ascontiguousarray(got[v][list(keep)]), ref[v]) and ref[v].any(), (rtpp, rtps, v)
            assert lm.zero_bits(got[v][drop]), (rtpp, rtps, v)
        assert support.same_bits(infl, finf) and (finf != 1.0).any(), (rtpp, rtps)
    y = {v: a.copy() for v, a in x.items()}
    for v in lk.VARS:
        y[v][drop] = np.nan
    again = lk.run(lt, y, lm.flags(E, keep))
    ainf = again["inflation"]
    for v in lk.VARS:
        assert support.same_bits(again[v], got[v]), v
    assert support.same_bits(ainf, infl)
    lt.close(); ltc.close()


@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_one_member_in_use(stride, plans):
    """n = 1 with relaxation on: all-zero increments, as the masked analysis leaves them"""
    sp, g = plans()
    E = 8
    x = lk.ensemble(g, E, seed=9)
    lt = lk.make(sp, E, lk.clustered_obs(g, x, n=300), SIGMA_V)
    lt.set_weight_stride(*stride)
    lt.set_relaxation(0.3, 0.9)
    got = lk.run(lt, x, lm.flags(E, (2,)))
    infl = got["inflation"]
    for v in lk.VARS:
        assert lm.zero_bits(got[v]), v
    assert (infl == 1.0).all()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 5. an Ensemble's state
def state_of(sp, g, oracle, E, nobs=20, seed=52):
    """an Ensemble of E seeded members and an analysis object on a network of nobs observations"""
    sts = es.member_states(sp, E)
    obs = lk.spread_obs(g, lk.oracle_grids(oracle, sts), nobs, seed=seed)
    return es.build(sp, sts), lk.make(sp, E, obs, SIGMA_V)


def grids_of(sp, lt, E):
    """the analysis object's grid workspace as a gridded ensemble (or its increments)"""
    grid, kx = lt.field("grid").numpy(), sp.kx
    gx = {v: grid[i * E * kx:(i + 1) * E * kx].reshape((E, kx) + sp.grid_shape).copy() for i, v in enumerate(lk.VARS[:4])}
    gx["ps"] = grid[4 * E * kx:].copy()
    return gx


def test_ensemble_state(plans, oracle_factory):
    """T30 L5, E = 3.  The relaxed Ensemble.analyse leaves in field("grid") the bits of the relaxed analyse_grid on the gridded
    ensemble Ensemble.verify made of the same state; time level 2 keeps its bits.  With rtpp = 1 the change of every prognostic
    agrees between the members to 4 eps max|state|"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans("t30k5")
    E = 3
    ens, lt = state_of(sp, g, oracle_factory("t30k5"), E)
    nat = s.Nature(sp, capacity=1)
    nat.set_state(*[getattr(ens, n)[0, 0] for n in es.PROG])
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.verify(lt, nat, slot=0)
    torch.cuda.synchronize()
    gx = grids_of(sp, lt, E)
    lt.set_relaxation(0.3, 0.9)
    ref = lk.run(lt, gx)
    lt.set_relaxation(0.0, 0.0)
    plain = lk.run(lt, gx)
    lt.set_relaxation(0.3, 0.9)
    ens.analyse(lt)
    torch.cuda.synchronize()
    got = grids_of(sp, lt, E)
    for v in lk.VARS:
        assert support.same_bits(got[v], ref[v]) and not support.same_bits(got[v], plain[v]), v
    for n in es.PROG:
        a = getattr(ens, n)
        assert support.same_bits(a[1], before[n][1]) and not support.same_bits(a[0], before[n][0]), n
    for n in es.PROG:
        getattr(ens, n).copy_(before[n])
    lt.set_relaxation(1.0, 0.0)
    ens.analyse(lt)
    torch.cuda.synchronize()
    for n in es.PROG:
        d = (getattr(ens, n)[0] - before[n][0]).cpu().numpy()
        scale = float(np.max(np.abs(before[n][0].cpu().numpy())))
        assert np.max(np.abs(d[0])) > 0.0, n
        for e in range(1, E):
            assert np.max(np.abs(d[e] - d[0])) <= 4 * lk.EPS * scale, (n, e, float(np.max(np.abs(d[e] - d[0]))) / (lk.EPS * scale))
    lt.close(); nat.close()


# ---------------------------------------------------------------------------------------------------- 6. capture
@pytest.mark.parametrize("E", [2, 17])
def test_capture(E, plans, oracle_factory):
    """A captured relaxed Ensemble.analyse has one kernel node more than the unrelaxed capture; its replays are bit-equal to the
    eager call; it keeps the values of its capture when set_relaxation is called afterwards"""
    import torch
    sp, g = plans("t30k5")
    ens, lt = state_of(sp, g, oracle_factory("t30k5"), E)
    x0 = {n: getattr(ens, n).clone() for n in es.PROG}
    lt.set_relaxation(0.3, 0.9)
    ens.analyse(lt)
    torch.cuda.synchronize()
    eager = {n: getattr(ens, n).clone() for n in es.PROG}
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        lt.set_relaxation(0.0, 0.0)
        with sp.graph_capture() as plain:
            ens.analyse(lt)
        nodes = plain.num_nodes()
        plain.close()
        lt.set_relaxation(0.3, 0.9)
        with sp.graph_capture() as gr:
            ens.analyse(lt)
        assert gr.num_nodes() == nodes + 1, (gr.num_nodes(), nodes)
        for setting in ((0.3, 0.9), (1.0, 0.0), (0.0, 0.0)):
            lt.set_relaxation(*setting)
            for n in es.PROG:
                getattr(ens, n).copy_(x0[n])
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), eager[n]), (setting, n)
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 7. on the T63 L16 grid
@pytest.mark.parametrize("E", [3, 32])
def test_kernel_against_restatement_t63(E, plans):
    """192 x 96 x 16, a cluster of 300 and the sparse set: `kernel_against_restatement`.  letkf_relax_kernel has 4 kx + 1 = 65 items in
    blockIdx.y, and at E = 32 the raw-increment workspace is 65 x 32 grids, 307 MB"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    kernel_against_restatement("T63 L16 E=%d" % E, sp, g, E, lambda g, x: (("mixed", mixed(g, x)),))


def test_weight_stride_t63(plans):
    """192 x 96 x 16: `weight_stride`"""
    sp, g = plans(T63)
    weight_stride("T63 L16 ", sp, g)


@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_outputs_may_be_the_inputs_t63(stride, plans):
    """192 x 96 x 16, E = 17: `outputs_may_be_the_inputs`"""
    sp, g = plans(T63)
    outputs_may_be_the_inputs(sp, g, stride)
