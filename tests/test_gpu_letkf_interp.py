"""GPU: the weight interpolation of the ensemble analysis (include/spdy.h "ensemble analysis", weight interpolation;
Letkf.set_weight_stride) against its NumPy restatement (tests/letkfinterp.py on tests/letkf.py): the coarse columns
bit for bit against the same object's stride-(1, 1) call, the weight buffer and the increments at every stencil class against the
restatement, the largest LDS request with a column list, the exact statements, the analysis of an ensemble's spectral state and the
capture.  T30, kx = 5; the section "on the T63 L16 grid" holds the kernels and the host tables to the same rules at 192 x 96 x 16."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfinterp as li
import support

pytestmark = pytest.mark.gpu

STRIDES = [(2, 2), (3, 5), (4, 47)]
CENTRE, POLAR, class_columns = li.CENTRE, li.POLAR, li.class_columns


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lk.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30k5", nmem=32: get(tag, nmem)


def observations(g, x, n=600):
    """a cluster around CENTRE (more than two of the kernel's chunks), a smaller one around POLAR -- in range of the last row, of the
    short last latitude interval and of the longitude cell that wraps -- and the sparse set"""
    return lk.concat(lk.clustered_obs(g, x, n=n), lk.clustered_obs(g, x, n=200, centre=POLAR, seed=6), lk.sparse_obs(g, x))


_REFERENCE = {}


def reference(g, E, sigma_v, tag="t30k5", strides=STRIDES):
    """per (tag, E, sigma_v), once: the ensemble, the observations, per stride the chosen columns, and the restatement's transforms by
    both eigen routes at every coarse column those columns' stencils read (the union over the strides, solved in one batch)"""
    if (tag, E, sigma_v) not in _REFERENCE:
        x = lk.ensemble(g, E, seed=E)
        obs = observations(g, x)
        per = {}
        for si, sj in strides:
            idx, wgt = li.stencils(g, si, sj)
            cls = class_columns(g, si, sj)
            cols = np.unique(np.concatenate(list(cls.values())))
            per[(si, sj)] = (idx, wgt, cls, cols, li.needed(idx, wgt, cols))
        union = np.unique(np.concatenate([li.coarse_columns(g, *st)[p[4]] for st, p in per.items()]))
        T = {r: li.transforms(g, x, obs, lk.SIGMA_H, sigma_v, lk.RHO, union, r) for r in ("eigh", "jacobi")}
        _REFERENCE[(tag, E, sigma_v)] = (x, obs, per, union, T)
    return _REFERENCE[(tag, E, sigma_v)]


def run_at(sp, lt, x, si, sj):
    lt.set_weight_stride(si, sj)
    return lk.run(lt, x)


# ---------------------------------------------------------------------------------------------------- 1. the coarse columns
def coarse_columns_bit_equal(sp, g, E, strides):
    """the increments at every coarse column are bit-equal to the same object's stride-(1, 1) call on the same inputs, and the other
    columns are not all equal to it; back at (1, 1) the object gives the first result again"""
    x = lk.ensemble(g, E, seed=60 + E)
    lt = lk.make(sp, E, observations(g, x), 0.1)
    full = lk.run(lt, x)
    for si, sj in strides:
        got = run_at(sp, lt, x, si, sj)
        coarse = lt.table("coarse_columns")
        assert np.array_equal(coarse, li.coarse_columns(g, si, sj))
        for v in lk.VARS:
            a, b = (np.ascontiguousarray(lk.at_columns(r[v], coarse)) for r in (got, full))
            assert a.any() and support.same_bits(a, b), (si, sj, v)
            assert not support.same_bits(got[v], full[v]), (si, sj, v)
    again = run_at(sp, lt, x, 1, 1)
    for v in lk.VARS:
        assert support.same_bits(again[v], full[v]), v
    lt.close()


@pytest.mark.parametrize("E", [2, 3, 32])
def test_coarse_columns_bit_equal(E, plans):
    """strides (2, 2) and (3, 5): coarse_columns_bit_equal"""
    sp, g = plans()
    coarse_columns_bit_equal(sp, g, E, STRIDES[:2])


# ---------------------------------------------------------------------------------------------------- 2. against the restatement
def against_the_restatement(sp, g, E, sigma_v, tag="t30k5", strides=STRIDES):
    """rho = 1.1; grid columns of every stencil class -- interior, on a coarse row only, on a coarse longitude only, in the last
    longitude cell (i1 wraps to 0), in the short last latitude interval, j = 0, j = il-1 -- in range of a cluster and out of it.
    field("weights") at the coarse columns those stencils read: within max(16 x the difference of the restatement's two eigen routes
    in T, 64 E eps max|T|).  The increments of each variable: within max(16 x the difference of the restatement's two routes, 64 E
    eps max|x - mean|).  The library's tables against the restatement's: the indices equal, the weights within 2 eps"""
    x, obs, per, union, T = reference(g, E, sigma_v, tag, strides)
    sc = lk.perturbation_scale(x)
    lt = lk.make(sp, E, obs, sigma_v)
    d = np.minimum(*(lk.distance(g.colunit, lk.unit([p[0]], [p[1]]))[:, 0] for p in (CENTRE, POLAR)))
    for (si, sj), (idx, wgt, cls, cols, entries) in per.items():
        assert len(cls) == (7 if sj < g.il - 1 else 6) and (d[cols] < lk.C_H).sum() >= 4 and (d[cols] > 2.0 * lk.C_H).sum() >= 2
        got = run_at(sp, lt, x, si, sj)
        assert np.array_equal(lt.table("interp_index"), idx) and np.max(np.abs(lt.table("interp_weight") - wgt)) <= 2 * lk.EPS
        at = np.searchsorted(union, li.coarse_columns(g, si, sj)[entries])
        Te, Tj = T["eigh"][at], T["jacobi"][at]
        W = lt.field("weights").numpy()
        assert W.shape == (len(lt.table("coarse_columns")), g.kx, E, E)
        tlim = max(16 * float(np.max(np.abs(Te - Tj))), 64 * E * lk.EPS * float(np.max(np.abs(Te))))
        tworst = float(np.max(np.abs(W[entries] - Te))) / tlim
        ref, alt = (li.increments(g, x, li.interpolate(t, entries, idx, wgt, cols), cols) for t in (Te, Tj))
        lim = {v: max(16 * float(np.max(np.abs(ref[v] - alt[v]))), 64 * E * lk.EPS * sc[v]) for v in lk.VARS}
        worst = {v: float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v] for v in lk.VARS}
        print("[letkf interp %sE=%d sigma_v=%g stride (%d, %d)] %d columns, %d coarse; ratio to the limit: T %.3f %s"
              % ("" if tag == "t30k5" else tag + " ", E, sigma_v, si, sj, len(cols), len(entries), tworst,
                 " ".join("%s %.3f" % kv for kv in worst.items())))
        assert all(ref[v].any() for v in lk.VARS)
        assert tworst <= 1.0, (si, sj, tworst)
        assert max(worst.values()) <= 1.0, (si, sj, worst)
    lt.close()


@pytest.mark.parametrize("sigma_v", [0.0, 0.1])
@pytest.mark.parametrize("E", [2, 3, 8, 16, 17, 32])
def test_against_the_restatement(E, sigma_v, plans):
    """strides (2, 2), (3, 5) and (4, 47): against_the_restatement.  E = 2, 3 | 8 | 16 | 17, 32: an item of letkf_apply_kernel has
    2, 4 | 8 | 16 | 32 lanes."""
    sp, g = plans()
    against_the_restatement(sp, g, E, sigma_v)


def test_many_levels_with_a_column_list():
    """E = 32 at kx = 16, stride (2, 2): the largest LDS request (one level in flight) with a column list, held to the same rule at a
    column of each of the classes interior, coarse longitude only and coarse row only, all in range of the cluster"""
    import speedy_f90_amd as s
    E, kx, si, sj = 32, 16, 2, 2
    sp = s.Spectral("t30", kx=kx, max_batch=E * (2 * kx + 1), device=0)
    sp.set_sigma(np.linspace(0.0, 1.0, kx + 1) ** 1.5)
    g = lk.Geometry(sp)
    x = lk.ensemble(g, E, seed=kx)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    cols = np.unique(np.concatenate([c[:1] for c in list(class_columns(g, si, sj).values())[:3]]))      # interior, coarse longitude, coarse row
    idx, wgt = li.stencils(g, si, sj)
    ref, entries, Te = li.analyse(g, x, obs, lk.SIGMA_H, 0.1, lk.RHO, si, sj, "eigh", cols, (idx, wgt))
    alt, _, _ = li.analyse(g, x, obs, lk.SIGMA_H, 0.1, lk.RHO, si, sj, "jacobi", cols, (idx, wgt))
    lt = s.Letkf(sp, E, len(obs["var"]), lk.SIGMA_H, 0.1, lk.RHO, weight_stride=(si, sj))
    lt.set_obs(*lk.args(obs))
    got = lk.run(lt, x)
    sc = lk.perturbation_scale(x)
    lim = {v: max(16 * float(np.max(np.abs(ref[v] - alt[v]))), 64 * E * lk.EPS * sc[v]) for v in lk.VARS}
    worst = {v: float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v] for v in lk.VARS}
    print("[letkf interp kx=16 E=32] ratio to the limit: %s" % " ".join("%s %.3f" % kv for kv in worst.items()))
    lt.close()
    sp.close()
    assert all(ref[v].any() for v in lk.VARS) and max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- 3. exact statements
def test_no_observation_is_exactly_zero(plans):
    """no observations and rho = 1: every increment is +0.0, bit for bit, and so is every T"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=70)
    lt = lk.make(sp, E, lk.make_obs([], [], [], [], [], []), 0.1, 1.0)
    got = run_at(sp, lt, x, 3, 5)
    assert not lt.field("weights").numpy().any()
    for v in lk.VARS:
        assert not got[v].view(np.int64).any(), v
    lt.close()


def test_appended_observations_and_two_runs(plans):
    """rho = 1, stride (4, 47): the coarse columns are those of rows 0 and il-1.  Observations appended around a fine column near the
    equator are in its range and out of range of all four coarse columns of its stencil: its bits do not change (at stride (1, 1)
    they do).  Two runs are bit-equal."""
    sp, g = plans()
    E, si, sj = 3, 4, 47
    x = lk.ensemble(g, E, seed=71)
    base = lk.concat(lk.clustered_obs(g, x, n=200, centre=POLAR, seed=6), lk.sparse_obs(g, x))
    col = 24 * g.ix + 26
    more = lk.clustered_obs(g, x, n=300, centre=(float(g.lon[26]), float(g.lat[24])), seed=8)
    both = lk.concat(base, more)
    lt = lk.make(sp, E, both, 0.1, 1.0)
    lt.set_obs(*lk.args(base))
    first, again = run_at(sp, lt, x, si, sj), lk.run(lt, x)
    idx, wgt = lt.table("interp_index"), lt.table("interp_weight")
    four = lt.table("coarse_columns")[idx[col]]
    assert (wgt[col] != 0.0).all() and len(set(four)) == 4
    dist = lk.distance(g.colunit[np.append(four, col)], lk.unit(more["lon"], more["lat"]))
    assert float(dist[:4].min()) > 2.0 * lk.C_H * (1.0 + 1e-12) and float(dist[4].max()) < lk.C_H
    lt.set_obs(*lk.args(both))
    second = lk.run(lt, x)
    full_both = run_at(sp, lt, x, 1, 1)
    lt.set_obs(*lk.args(base))
    full_base = lk.run(lt, x)
    lt.close()
    for v in lk.VARS:
        assert support.same_bits(first[v], again[v]), v
        a, b = (np.ascontiguousarray(lk.at_columns(r[v], [col])) for r in (first, second))
        assert a.any() and support.same_bits(a, b), v
        a, b = (np.ascontiguousarray(lk.at_columns(r[v], [col])) for r in (full_base, full_both))
        assert not support.same_bits(a, b), v


@pytest.mark.parametrize("pattern", ["front255", "wave3", "hole"])
def test_padded_scans(pattern, plans):
    """E = 17, stride (2, 2), rho = 1.1, sigma_v = 0.1: the padded sets of tests/test_gpu_letkf.py::test_padded_scans (255 pad
    observations in front; 192 in front of every 64 real ones; a whole chunk between two chunks of real ones).  Every grid column
    whose stencil reads only coarse columns farther than 2 c_h (1 + 1e-12) from the pad keeps the bits of the unpadded run, in all
    five variables at every level, and so do the transforms of those coarse columns; the columns in range of the cluster are among
    them, and there are at least 4 300.  Where a stencil reads a coarse column in range of the pad the increments differ."""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=90 + E)
    real, pad = lk.padded_inputs(g, x)
    far, acted = lk.padded_conditions(g, real, pad)
    lt = lk.make(sp, E, lk.concat(real, pad), 0.1)
    lt.set_obs(*lk.args(real))
    first = run_at(sp, lt, x, 2, 2)
    W = lt.field("weights").numpy().copy()
    coarse, idx = lt.table("coarse_columns"), lt.table("interp_index")
    reads = coarse[idx]                                  # (ncol, 4) grid columns a stencil reads: an entry of weight zero repeats one that is read
    keep, changed = np.nonzero(far[reads].all(axis=1))[0], np.nonzero(acted[reads].any(axis=1))[0]
    cluster = lk.in_range(g, {k: v[:320] for k, v in real.items()}).any(axis=1)
    assert len(keep) >= 4300 and np.isin(np.nonzero(cluster)[0], keep).all() and len(changed) >= 20, (len(keep), len(changed))
    obs, at = lk.interleave(real, pad, pattern)
    lt.set_obs(*lk.args(obs))
    got = lk.run(lt, x)
    assert support.same_bits(np.ascontiguousarray(lt.field("weights").numpy()[far[coarse]]), np.ascontiguousarray(W[far[coarse]]))
    for v in lk.VARS:
        a, b = (np.ascontiguousarray(lk.at_columns(r[v], keep)) for r in (got, first))
        assert b.any() and support.same_bits(a, b), (pattern, v)
    assert any(not np.array_equal(lk.at_columns(got[v], changed), lk.at_columns(first[v], changed)) for v in lk.VARS), pattern
    print("[letkf interp padded %s] %d observations: %d columns bit-equal, %d differ" % (pattern, len(obs["var"]), len(keep), len(changed)))
    lt.close()


# ---------------------------------------------------------------------------------------------------- 4. the state
def test_state(plans, oracle_factory):
    """Ensemble.analyse at T30 L5, E = 3, stride (2, 2), against the restatement fed by the oracle's transforms: every prognostic of
    time level 1 within 1e-12 of its scale; time level 2 keeps its bits"""
    import torch
    sp, g = plans()
    E = 3
    o = oracle_factory("t30k5")
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    x = lk.oracle_grids(o, sts)
    obs = lk.spread_obs(g, x, 40, seed=50)
    inc, _, _ = li.analyse(g, x, obs, lk.SIGMA_H, 0.1, lk.RHO, 2, 2)
    grid = lambda a: a.reshape(a.shape[:-1] + (g.il, g.ix))
    lt = lk.make(sp, E, obs, 0.1)
    lt.set_weight_stride(2, 2)
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.analyse(lt)
    torch.cuda.synchronize()
    for e, st in enumerate(sts):
        vd = [o.vdspec(grid(inc["u"][e])[k], grid(inc["v"][e])[k], 2) for k in range(o.kx)]
        want = {"vor": st["vor"][0] + np.stack([a for a, _ in vd]), "div": st["div"][0] + np.stack([b for _, b in vd]),
                "t": st["t"][0] + np.stack([o.grid_to_spec(grid(inc["t"][e])[k]) for k in range(o.kx)]),
                "tr": st["tr"][0] + np.stack([o.grid_to_spec(grid(inc["q"][e])[k]) for k in range(o.kx)]),
                "ps": st["ps"][0] + o.grid_to_spec(grid(inc["ps"][e]))}
        for n in es.PROG:
            a = getattr(ens, n)
            assert support.same_bits(a[1], before[n][1]) and not support.same_bits(a[0], before[n][0]), n
            err = float(np.max(np.abs(a[0, e].cpu().numpy() - want[n])) / np.max(np.abs(want[n])))
            print("[letkf interp state] member %d %s: %.3e" % (e, n, err))
            assert err <= 1e-12, (n, e, err)
    lt.close()


# ---------------------------------------------------------------------------------------------------- 5. the capture
def test_capture(plans, oracle_factory):
    """E = 2 at stride (2, 2): the captured analysis has six kernel nodes; replays, each from the same state, equal the eager call bit
    for bit; after set_obs with the same number of observations a replay uses the new ones"""
    import torch
    sp, g = plans()
    E = 2
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    x0 = {n: getattr(ens, n).clone() for n in es.PROG}
    xg = lk.oracle_grids(oracle_factory("t30k5"), sts)
    obs, other = lk.spread_obs(g, xg, 20, seed=52), lk.spread_obs(g, xg, 20, seed=53)
    lt = lk.make(sp, E, obs, 0.1)
    lt.set_weight_stride(2, 2)

    def eager(o):
        lt.set_obs(*lk.args(o))
        for n in es.PROG:
            getattr(ens, n).copy_(x0[n])
        ens.analyse(lt)
        torch.cuda.synchronize()
        return {n: getattr(ens, n).clone() for n in es.PROG}
    want_other, want = eager(other), eager(obs)
    assert not support.same_bits(want["t"], x0["t"]) and not support.same_bits(want["t"], want_other["t"])
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            ens.analyse(lt)
        assert gr.num_nodes() == 6, gr.num_nodes()
        for w in (want, want, want_other):
            if w is want_other:
                lt.set_obs(*lk.args(other))
            for n in es.PROG:
                getattr(ens, n).copy_(x0[n])
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), w[n]), n
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. on the T63 L16 grid
T63 = "t63k16"
# (2, 2): 96 x 48 coarse columns; (3, 5): the short last interval 95; (96, 7): ni = 2, every cell wraps; (4, 95): rows 0 and il-1 only
STRIDES_T63 = [(2, 2), (3, 5), (96, 7), (4, 95)]


@pytest.mark.parametrize("E", [3, 16, 32])
def test_against_the_restatement_t63(E, plans):
    """192 x 96 x 16, sigma_v = 0.1: against_the_restatement at the strides that are only legal here -- si = 96 = ix / 2, where both
    coarse longitudes' cells wrap, sj = 95, the largest -- and at (2, 2), whose weight buffer is the largest (617 MB at E = 32), and
    (3, 5).  E = 3, 16, 32: an item of letkf_apply_kernel has 4, 16, 32 lanes and walks kx ncol = 294 912 items"""
    sp, g = plans(T63, 32)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    against_the_restatement(sp, g, E, 0.1, T63, STRIDES_T63)


@pytest.mark.parametrize("E", [3, 16, 32])
def test_coarse_columns_bit_equal_t63(E, plans):
    """192 x 96 x 16, strides (2, 2) and (3, 5): coarse_columns_bit_equal"""
    sp, g = plans(T63, 32)
    coarse_columns_bit_equal(sp, g, E, STRIDES_T63[:2])
