"""GPU: the ensemble analysis (include/spdy.h "ensemble analysis", Letkf, Ensemble.analyse) against its NumPy
restatement (tests/letkf.py): the observation operator, the analysis of gridded ensembles at every Jacobi size class (E = 2, odd,
4, 8, 16, 17, 31, 32) and every level class of the solve (all slots of a round live, idle slots, kx > 16), at the edge columns of
the grid, on hard local problems near the sweep cap, the exact statements the increment form makes -- the same bits wherever an
observation sits in the scan among them --, the closed form of one observation, the analysis of an ensemble's spectral state
against the restatement fed by the oracle's transforms, and the capture.  T30 unless said otherwise; the section "on the T63 L16
grid" holds the operator and the plain analysis to the same rules at 192 x 96 x 16 and E = 2, 3, 16, 32, and one object with
every later feature on at once (test_everything_at_once_t63) to the restatements of all of them."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfinfl as lf
import letkfinterp as li
import letkfmask as lm
import letkfpressure as lp
import letkfqc as qc
import letkfrelax as lr
import letkfslots as ls
import support

pytestmark = pytest.mark.gpu

DELT = 2400.0


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lk.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30k5", nmem=32: get(tag, nmem)


# ---------------------------------------------------------------------------------------------------- 1. the operator
def operator(tag, sp, g, E):
    """hx, hxmean and departure of about 40 observations -- on a grid point, between columns ix-1 and 0, poleward of the outermost
    rows, at lon = 360 and at negative longitude among them -- within 16 eps max|x| of the restatement: a four-term convex sum and an
    E-term sum in the same order; y is hx - hxmean in every bit"""
    x = lk.ensemble(g, E, seed=40 + E)
    obs = lk.edge_obs(g, x)
    lt = lk.make(sp, E, obs)
    lk.run(lt, x)
    got = {n: a.cpu().numpy() for n, a in lt.fields().items()}
    ref = lk.obs_space(g, x, obs)
    hx, hxmean, dep = ref["hx"], ref["hxmean"], ref["departure"]
    scale = np.array([np.max(np.abs(x[lk.VARS[v]])) for v in obs["var"]])
    for name, mine, ref, sc in (("hx", got["hx"], hx, scale[:, None]), ("hxmean", got["hxmean"], hxmean, scale),
                                ("departure", got["departure"], dep, scale)):
        worst = float(np.max(np.abs(mine - ref) / (16 * lk.EPS * sc)))
        print("[letkf operator %sE=%d] %s: %.3f of the bound" % (tag, E, name, worst))
        assert mine.shape == ref.shape and worst <= 1.0, (name, worst)
    assert support.same_bits(lt.field("y").numpy(), got["hx"] - got["hxmean"][:, None])
    lt.close()


@pytest.mark.parametrize("E", [3, 32])
def test_operator(E, plans):
    """kx = 5: `operator`"""
    sp, g = plans()
    operator("", sp, g, E)


# ---------------------------------------------------------------------------------------------------- 2. the analysis on grids
def run(tag, sp, g, x, obs, E, sigma_v, cols, rho=lk.RHO, sigma_h=lk.SIGMA_H, sample=None):
    """the device's increments, the restatement's at the columns cols, the limits (lk.limits) and kappa; the ratios are printed.
    sample: the limits' Jacobi route at so many of the columns (lk.hardest), which can only make them stricter"""
    C, b = lk.problems(g, obs, lk.obs_space(g, x, obs), sigma_h, sigma_v, cols)
    lim, ref, kappa = lk.limits(g, x, C, b, rho, cols, E, None if sample is None else lk.hardest(C, rho, sample))
    lt = lk.make(sp, E, obs, sigma_v, rho, sigma_h)
    got = lk.run(lt, x)
    lt.close()
    worst = {v: float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v] for v in lk.VARS}
    print("[letkf grid %s E=%d sigma_v=%g] %d observations, %d columns, kappa %.2e, ratio to the limit: %s"
          % (tag, E, sigma_v, len(obs["var"]), len(cols), kappa, " ".join("%s %.3f" % kv for kv in worst.items())))
    return got, ref, lim, worst, kappa


def compare(tag, sp, g, x, obs, E, sigma_v, cols, rho=lk.RHO, **how):
    _, _, _, worst, kappa = run(tag, sp, g, x, obs, E, sigma_v, cols, rho, **how)
    return worst, kappa


@pytest.mark.parametrize("sigma_v", [0.0, 0.1])
@pytest.mark.parametrize("E", [2, 3, 4, 8, 16, 17, 31, 32])
def test_analysis_on_grids(E, sigma_v, plans):
    """kx = 5, rho = 1.1: a clustered set of 1 500 observations, all in range of the columns around its centre and more than three
    times the kernel's chunk (lk.CHUNK = LETKF_CHUNK = 256 of csrc/spdy_letkf.hip), and a sparse set.  Compared at the columns
    nearest to the observations, at those at the edge of their range and at columns out of range.  The inputs reach kappa(A) >=
    1e3 and stay <= 1e6."""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=E)
    most = 48 if E < 31 else 32
    kappas = []
    for tag, obs in (("clustered", lk.clustered_obs(g, x)), ("sparse", lk.sparse_obs(g, x))):
        if tag == "clustered":
            centre = lk.distance(g.colunit, lk.unit([100.0], [20.0]))[:, 0].argmin()
            d = lk.distance(g.colunit[centre:centre + 1], lk.unit(obs["lon"], obs["lat"]))
            assert len(obs["var"]) > 3 * lk.CHUNK and float(d.max()) < 2.0 * lk.C_H        # all of them in range of one column
        cols = lk.columns_for(g, obs, lk.SIGMA_H, most=most)
        worst, kappa = compare(tag, sp, g, x, obs, E, sigma_v, cols)
        kappas.append(kappa)
        assert max(worst.values()) <= 1.0, (tag, worst)
    assert max(kappas) >= 1e3 and max(kappas) <= 1e6, kappas


def test_analysis_small_errors(plans):
    """error = 1e-4 on the sparse set, E = 17: kappa(A) near 1e9, held to the same rule"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=E)
    obs = lk.sparse_obs(g, x)
    obs["error"][:] = 1.0e-4
    worst, kappa = compare("small errors", sp, g, x, obs, E, 0.1, lk.columns_for(g, obs, lk.SIGMA_H))
    assert 1e8 <= kappa <= 1e10, kappa
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("kx", [14, 16])
def test_analysis_many_levels(kx):
    """E = 32 at kx = 14 and kx = 16, T30: the two configurations in which a workgroup's LDS holds fewer than four levels' eigen
    workspaces -- two levels in flight with 128 threads each (149 568 bytes), one with all 256 (155 712 bytes, the largest the
    object accepts).  A cluster of 300 observations (more than one chunk) and the sparse set together, held to the same rule."""
    import speedy_f90_amd as s
    E = 32
    sp = s.Spectral("t30", kx=kx, max_batch=E * (2 * kx + 1), device=0)
    sp.set_sigma(np.linspace(0.0, 1.0, kx + 1) ** 1.5)
    g = lk.Geometry(sp)
    x = lk.ensemble(g, E, seed=kx)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    worst, kappa = compare("kx=%d" % kx, sp, g, x, obs, E, 0.1, lk.columns_for(g, obs, lk.SIGMA_H, most=12, outside=4))
    sp.close()
    assert max(worst.values()) <= 1.0, worst


def levels_in_flight(E, kx):
    """nlv of DESIGN s18: the most of 4, 2, 1 levels whose eigen workspaces fit beside A and b of all levels in the 160 KB of a
    compute unit's LDS, 8 (kx E'^2 + kx E' + nlv (E'^2 + 11 E') + 16 E' + 16 kx + 424) bytes with E' = E rounded up to even"""
    ep = E + (E & 1)
    return next(n for n in (4, 2, 1) if 8 * (kx * ep * ep + kx * ep + n * (ep * ep + 11 * ep) + 16 * ep + 16 * kx + 424) <= 160 * 1024)


@pytest.mark.parametrize("kx,E", [(8, 32), (8, 4), (7, 32), (15, 32), (20, 16)])
def test_analysis_level_classes(kx, E):
    """The level classes of the solve, each on a plan of its own: kx = 8, the model's own count (four levels in flight, no idle
    slot), at E = 32 and E = 4; kx = 7 (four in flight, one slot idle in the last round); kx = 15 at E = 32 (two in flight, the
    only case in which that form has an idle slot: the level of the slot is out of range, its matrix aliased to level 0 and never
    touched); kx = 20 at E = 16 (more levels than 16, four in flight).  The cluster of 300 and the sparse set, sigma_v = 0.1, held
    to the rule of test_analysis_on_grids."""
    import speedy_f90_amd as s
    nlv = levels_in_flight(E, kx)
    assert nlv == {(8, 32): 4, (8, 4): 4, (7, 32): 4, (15, 32): 2, (20, 16): 4}[(kx, E)]
    assert (kx % nlv != 0) == ((kx, E) in ((7, 32), (15, 32)))                  # an idle slot in the last round
    sp = s.Spectral("t30", kx=kx, max_batch=E * (2 * kx + 1), device=0)
    if kx not in (5, 7, 8):
        sp.set_sigma(np.linspace(0.0, 1.0, kx + 1) ** 1.5)
    g = lk.Geometry(sp)
    x = lk.ensemble(g, E, seed=kx)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    worst, kappa = compare("kx=%d" % kx, sp, g, x, obs, E, 0.1, lk.columns_for(g, obs, lk.SIGMA_H, most=12, outside=4))
    sp.close()
    assert max(worst.values()) <= 1.0, worst


def test_analysis_t63_edges(plans):
    """T63 L16, E = 16 (18 432 columns, ix = 192, four levels in flight): edge_obs and a cluster of 300, compared
    at columns_for's columns and at every edge column (lk.edge_columns) in range of an observation; the limits' Jacobi route at 48
    of them"""
    sp, g = plans("t63k16", 16)
    E = 16
    assert (g.ix, g.il, g.kx) == (192, 96, 16) and levels_in_flight(E, g.kx) == 4
    x = lk.ensemble(g, E, seed=63)
    obs = lk.concat(lk.edge_obs(g, x), lk.clustered_obs(g, x, n=300))
    edge = lk.edge_columns(g)
    edge = edge[lk.in_range(g, obs, edge).any(axis=1)]
    cols = np.unique(np.concatenate([lk.columns_for(g, obs, lk.SIGMA_H), edge]))
    assert len(edge) >= 100
    worst, kappa = compare("T63 L16", sp, g, x, obs, E, 0.1, cols, sample=48)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- 2b. the edge columns
@pytest.mark.parametrize("E", [3, 32])
def test_edge_columns(E, plans):
    """kx = 5, sigma_v = 0.1, sigma_h = lk.EDGE_SIGMA_H (at 5e5 edge_obs alone reaches every column of longitudes 0 and ix-1, and
    the test wants some out of range): edge_obs, 200 observations around (359.5, 0) between columns ix-1 and 0, 200 around latitude
    +88 and 200 around -88 at longitudes all around the circle.  Compared at every column of rows 0, 1, il-2, il-1 and of
    longitudes 0 and ix-1 (472), the reference from lk.problems, under the rule of test_analysis_on_grids (E = 32: the
    limits' Jacobi route at 64 of the columns).  The conditions on the inputs are lk.edge_conditions'; the columns out of range of
    everything also equal pure inflation X' (sqrt(rho) - 1) within the same limits."""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=80 + E)
    obs, cols, out = lk.edge_conditions(g, lk.edge_inputs(g, x))
    got, ref, lim, worst, kappa = run("edge columns", sp, g, x, obs, E, 0.1, cols, sigma_h=lk.EDGE_SIGMA_H,
                                      sample=None if E < 32 else 64)
    assert max(worst.values()) <= 1.0, worst
    for v in lk.VARS:
        f = lk.at_columns(x[v], cols[out])
        s = np.zeros(f.shape[1:])
        for e in range(E):
            s = s + f[e]
        want = (f - (s / E)[None]) * (np.sqrt(lk.RHO) - 1.0)
        a = lk.at_columns(got[v], cols[out])
        assert a.any() and float(np.max(np.abs(a - want))) <= lim[v], v


# ---------------------------------------------------------------------------------------------------- 2c. hard local problems
@pytest.mark.parametrize("factor", [1e-3, 3e-5])
@pytest.mark.parametrize("E", [32, 31])
def test_hard_local_problems(E, factor, plans):
    """kx = 5, sigma_v = 0: 16 observations of cycling variables within a degree of one grid point with errors 1e-3 and 3e-5 of the
    spread (lk.hard_obs).  C has rank 16, the eigenvalue (E-1)/rho repeats, and kappa(A) is 4.4e6 and 4.9e9 at E = 32, 4.0e6 and
    4.4e9 at E = 31 (asserted in [1e6, 1e10]).  lk.jacobi needs up to 15 and 16 sweeps at E = 32, 14 and 14 at E = 31, the closing
    idle sweep included, where the columns of test_analysis_on_grids nearest to the cluster need 9 or 10 and those at the edge of its
    range, where C is of low rank too, up to 13: asserted above 9 and at most lk.SWEEPS = LETKF_SWEEPS, so a device result within
    the rule of test_analysis_on_grids is a converged one, not a lucky truncation.  Measured ratios to the limit: at most 0.10."""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=E)
    obs = lk.hard_obs(g, x, factor)
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=24, outside=4)
    C, _ = lk.problems(g, obs, lk.obs_space(g, x, obs), lk.SIGMA_H, 0.0, cols)
    ran = lk.jacobi(C[:, 0] + ((E - 1) / lk.RHO) * np.eye(E), counts=True)[2]          # sigma_v = 0: every level has this A
    worst, kappa = compare("hard, error %g" % factor, sp, g, x, obs, E, 0.0, cols)
    print("[letkf hard E=%d error=%g] sweeps of the restatement: up to %d" % (E, factor, ran.max()))
    assert 1e6 <= kappa <= 1e10, kappa
    assert 9 < int(ran.max()) <= lk.SWEEPS, ran.max()
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- 3. exact statements
_UNPADDED = {}


def unpadded(sp, g, E):
    """per E, once: the ensemble, the real and the pad observations, the analysis object (room for 1 600 observations) and what the
    device gives on the real ones alone: the increments, y and the departures"""
    if E not in _UNPADDED:
        x = lk.ensemble(g, E, seed=90 + E)
        real, pad = lk.padded_inputs(g, x)
        lt = lk.make(sp, E, lk.concat(real, pad), 0.1)
        lt.set_obs(*lk.args(real))
        inc = lk.run(lt, x)
        _UNPADDED[E] = (x, real, pad, lt, inc, lt.field("y").numpy().copy(), lt.fields()["departure"].cpu().numpy())
    return _UNPADDED[E]


@pytest.mark.parametrize("pattern", lk.PATTERNS)
@pytest.mark.parametrize("E", [3, 32])
def test_padded_scans(E, pattern, plans):
    """rho = 1.1, sigma_v = 0.1.  The real observations -- a cluster of 320 around (100, 20) and the 58 of the sparse set's 60 that
    are farther than 4 c_h from (280, -60) -- with observations around (280, -60) put between them (lk.interleave): one, 255 and
    256 in front, one before each, 192 in front of every 64 so that a chunk's survivors all sit in its last wave, a whole chunk of
    256 between two chunks of real ones; 379, 633, 634, 756, 1 530 and 634 observations, and with pad at the end also 512 (front1)
    and 768 (alternate).  A real observation then sits in another lane, wave, tile slot and chunk, and every column farther than
    2 c_h (1 + 1e-12) from the pad (4 465, all columns in range of the cluster among them) must keep the bits of the unpadded run
    in all five variables at every level; so must y and the departures of the real observations at their new places.  In range of
    the pad the increments differ (one u observation at the top level moves u, v, t and q there, not ps)."""
    sp, g = plans()
    x, real, pad, lt, inc, y, dep = unpadded(sp, g, E)
    far, acted = lk.padded_conditions(g, real, pad)
    far, acted, nr = np.nonzero(far)[0], np.nonzero(acted)[0], len(real["var"])
    natural = {"front1": nr + 1, "front255": nr + 255, "front256": nr + 256, "alternate": 2 * nr, "wave3": 1152 + nr, "hole": nr + 256}
    for total in (None,) + {"front1": (512,), "alternate": (768,)}.get(pattern, ()):
        obs, at = lk.interleave(real, pad, pattern, total)
        assert len(obs["var"]) == (total or natural[pattern])
        lt.set_obs(*lk.args(obs))
        got = lk.run(lt, x)
        assert support.same_bits(np.ascontiguousarray(lt.field("y").numpy()[at]), y)
        assert support.same_bits(np.ascontiguousarray(lt.fields()["departure"].cpu().numpy()[at]), dep)
        for v in lk.VARS:
            a, b = (np.ascontiguousarray(lk.at_columns(r[v], far)) for r in (got, inc))
            assert b.any() and support.same_bits(a, b), (pattern, total, v)
        assert any(not np.array_equal(lk.at_columns(got[v], acted), lk.at_columns(inc[v], acted)) for v in lk.VARS), (pattern, total)
        print("[letkf padded E=%d %s] %d observations: %d columns bit-equal, %d in range of the pad differ"
              % (E, pattern, len(obs["var"]), len(far), len(acted)))


def test_exact_zero_out_of_range(plans):
    """rho = 1, five T observations at level 2 around one point, sigma_v = 0.1: every column farther than 2 c_h from every
    observation has increments exactly 0.0 at every level, and every level farther than 2 c_v from level 2 -- all the others, and
    ps, which takes T of the lowest level -- has increments exactly 0.0 in every column"""
    sp, g = plans()
    E = 3
    x = lk.ensemble(g, E, seed=31)
    lon, lat = np.array([100.0, 101.0, 99.0, 100.5, 102.0]), np.array([20.0, 21.0, 19.5, 18.0, 22.0])
    obs = lk.observations(g, x, [lk.T] * 5, [2] * 5, lon, lat, 0.5)
    c_v = 0.1 * np.sqrt(10.0 / 3.0)
    assert all(abs(g.lnfsg[k] - g.lnfsg[2]) > 2.0 * c_v for k in range(g.kx) if k != 2)
    lt = lk.make(sp, E, obs, 0.1, 1.0)
    got = lk.run(lt, x)
    lt.close()
    far = lk.distance(g.colunit, lk.unit(lon, lat)).min(axis=1) > 2.0 * lk.C_H * (1.0 + 1e-12)
    assert far.sum() > 4000
    for v in lk.VARS:
        a = lk.at_columns(got[v], np.arange(g.ix * g.il))
        assert not a[..., far].any(), v
        if v == "ps":
            assert not a.any()
        else:
            assert not a[:, [0, 1, 3, 4]].any(), v
            assert a[:, 2].any(), v


def test_appended_observations_and_two_runs(plans):
    """rho = 1: observations appended to a set leave every column that is out of their range bit-equal; two runs are bit-equal"""
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=32)
    base = lk.clustered_obs(g, x, n=600)
    more = lk.clustered_obs(g, x, n=300, centre=(280.0, -20.0), seed=6)
    lt = lk.make(sp, E, lk.concat(base, more), 0.1, 1.0)
    lt.set_obs(*lk.args(base))
    first, again = lk.run(lt, x), lk.run(lt, x)
    lt.set_obs(*lk.args(lk.concat(base, more)))
    both = lk.run(lt, x)
    lt.close()
    untouched = lk.distance(g.colunit, lk.unit(more["lon"], more["lat"])).min(axis=1) > 2.0 * lk.C_H * (1.0 + 1e-12)
    near = lk.distance(g.colunit, lk.unit(base["lon"], base["lat"])).min(axis=1) < lk.C_H
    assert (untouched & near).sum() > 20
    for v in lk.VARS:
        assert support.same_bits(first[v], again[v]), v
        a, c = (lk.at_columns(r[v], np.nonzero(untouched)[0]) for r in (first, both))
        assert support.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(c)), v
        assert not support.same_bits(first[v], both[v]), v                  # the appended observations do act where they reach
        assert lk.at_columns(first[v], np.nonzero(near)[0]).any(), v


def test_pure_inflation(plans):
    """rho = 1.21 and no observations: T = (sqrt(rho) - 1) I, so the increment of every value is X' (sqrt(rho) - 1) with X' = x - mean,
    to 4 ulp of the increment"""
    sp, g = plans()
    for E in (2, 17):
        x = lk.ensemble(g, E, seed=33)
        lt = lk.make(sp, E, lk.make_obs([], [], [], [], [], []), 0.1, 1.21)
        got = lk.run(lt, x)
        lt.close()
        for v in lk.VARS:
            s = np.zeros(x[v].shape[1:])
            for e in range(E):
                s = s + x[v][e]
            xp = x[v] - (s / E)[None]
            want = xp * (np.sqrt(1.21) - 1.0)
            err = np.abs(got[v] - want) / np.spacing(np.abs(want))
            print("[letkf inflation E=%d] %s: %.2f ulp" % (E, v, float(err.max())))
            assert float(err.max()) <= 4.0, (E, v)


# ---------------------------------------------------------------------------------------------------- 4. the closed form
def test_closed_form(plans):
    """one T observation on a grid point at level 2: there w = 1, and with g = rho s^2 (s^2 the sample variance of T there) the mean
    increment is d g / (err^2 + g) and the analysed sample variance rho s^2 err^2 / (err^2 + g).  Bounds: the mean within the
    analysis rule 64 E eps max|x - mean|; the variance, a sum of E squares of analysed perturbations each off by at most that,
    within 4 x that x max|x - mean|."""
    sp, g = plans()
    E, i, j, k = 17, 30, 15, 2
    x = lk.ensemble(g, E, seed=34)
    col = j * g.ix + i
    tv = x["t"][:, k].reshape(E, -1)[:, col]
    err = 0.7
    obs = lk.make_obs([lk.T], [k], [g.lon[i]], [g.lat[j]], [tv.mean() + 1.3], [err])
    lt = lk.make(sp, E, obs, 0.1)
    got = lk.run(lt, x)
    lt.close()
    inc = got["t"][:, k].reshape(E, -1)[:, col]
    s2 = tv.var(ddof=1)
    gg = lk.RHO * s2
    d = obs["value"][0] - tv.mean()
    bound = 64 * E * lk.EPS * np.max(np.abs(tv - tv.mean()))
    mean_err = abs(inc.mean() - d * gg / (err * err + gg))
    var_err = abs((tv + inc).var(ddof=1) - lk.RHO * s2 * err * err / (err * err + gg))
    print("[letkf closed form] mean %.3e (bound %.3e), variance %.3e (bound %.3e)" % (mean_err, bound, var_err,
                                                                                     4 * bound * np.max(np.abs(tv - tv.mean()))))
    assert mean_err <= bound and var_err <= 4 * bound * np.max(np.abs(tv - tv.mean()))


# ---------------------------------------------------------------------------------------------------- 5. the state
def oracle_analysis(o, g, sts, obs, sigma_v, rho):
    """the analysed time level 1 of every member: the restatement's increments through the oracle's vdspec and grid_to_spec"""
    x = lk.oracle_grids(o, sts)
    inc, _ = lk.analyse(g, x, obs, lk.SIGMA_H, sigma_v, rho)
    grid = lambda a: a.reshape(a.shape[:-1] + (g.il, g.ix))
    out = []
    for e, st in enumerate(sts):
        vd = [o.vdspec(grid(inc["u"][e])[k], grid(inc["v"][e])[k], 2) for k in range(o.kx)]
        out.append({"vor": st["vor"][0] + np.stack([a for a, _ in vd]), "div": st["div"][0] + np.stack([b for _, b in vd]),
                    "t": st["t"][0] + np.stack([o.grid_to_spec(grid(inc["t"][e])[k]) for k in range(o.kx)]),
                    "tr": st["tr"][0] + np.stack([o.grid_to_spec(grid(inc["q"][e])[k]) for k in range(o.kx)]),
                    "ps": st["ps"][0] + o.grid_to_spec(grid(inc["ps"][e]))})
    return x, out


@pytest.mark.parametrize("tag,E,nobs", [("t30k5", 3, 40), ("t63k16", 2, 20)], ids=["t30k5-E3", "t63k16-E2"])
def test_state(tag, E, nobs, plans, oracle_factory):
    """Ensemble.analyse on seeded states (E = 3, kx = 5: odd stacks; T63 L16, E = 2) against the restatement fed by the oracle's
    transforms: every prognostic of time level 1 within 1e-12 of its scale; time level 2 keeps its bits"""
    import torch
    sp, g = plans(tag, 32 if tag == "t30k5" else E)
    o = oracle_factory(tag)
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    x = lk.oracle_grids(o, sts)
    obs = lk.spread_obs(g, x, nobs, seed=50)
    _, want = oracle_analysis(o, g, sts, obs, 0.1, lk.RHO)
    lt = lk.make(sp, E, obs, 0.1)
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.analyse(lt)
    torch.cuda.synchronize()
    for n in es.PROG:
        a = getattr(ens, n)
        assert support.same_bits(a[1], before[n][1]), n                  # time level 2
        assert not support.same_bits(a[0], before[n][0]), n
        for e in range(E):
            ref = want[e][n]
            err = float(np.max(np.abs(a[0, e].cpu().numpy() - ref)) / np.max(np.abs(ref)))
            print("[letkf state %s] member %d %s: %.3e" % (tag, e, n, err))
            assert err <= 1e-12, (n, e, err)
    lt.close()


def test_state_unchanged_and_restart(plans, oracle_factory):
    """no observations and rho = 1: every prognostic keeps its bits; after an analysis with observations, startup and two leapfrog
    steps stay finite"""
    import torch
    sp, g = plans()
    E = 3
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    lt = lk.make(sp, E, lk.make_obs([], [], [], [], [], []), 0.1, 1.0)
    ens.analyse(lt)
    torch.cuda.synchronize()
    for n in es.PROG:
        assert support.same_bits(getattr(ens, n), before[n]), n
    lt.close()
    lt = lk.make(sp, E, lk.spread_obs(g, lk.oracle_grids(oracle_factory("t30k5"), sts), 20, seed=51), 0.1)
    ens.analyse(lt)
    ens.startup(DELT)
    for _ in range(2):
        ens.step(2, 2, 2.0 * DELT)
    torch.cuda.synchronize()
    for n in es.PROG:
        assert not support.same_bits(getattr(ens, n)[0], before[n][0]), n
        assert bool(torch.isfinite(torch.view_as_real(getattr(ens, n))).all()), n
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. the capture
@pytest.mark.parametrize("E", [2, 17])
def test_capture(E, plans, oracle_factory):
    """analyse captured and replayed twice, each time from the same state, equals the eager call bit for bit; the graph has five
    kernel nodes"""
    import torch
    sp, g = plans()
    sts = es.member_states(sp, E)
    ens = es.build(sp, sts)
    x0 = {n: getattr(ens, n).clone() for n in es.PROG}
    lt = lk.make(sp, E, lk.spread_obs(g, lk.oracle_grids(oracle_factory("t30k5"), sts), 20, seed=52), 0.1)
    ens.analyse(lt)
    torch.cuda.synchronize()
    eager = {n: getattr(ens, n).clone() for n in es.PROG}
    assert not support.same_bits(eager["t"], x0["t"])
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            ens.analyse(lt)
        assert gr.num_nodes() == 5, gr.num_nodes()
        for _ in range(2):
            for n in es.PROG:
                getattr(ens, n).copy_(x0[n])
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), eager[n]), n
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 7. on the T63 L16 grid
T63 = "t63k16"


@pytest.mark.parametrize("E", [3, 32])
def test_operator_t63(E, plans):
    """192 x 96 x 16: `operator` -- the wrap cell between longitude 191 and 0 and the rows poleward of +-88.57 degrees"""
    sp, g = plans(T63, 32)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    operator("T63 L16 ", sp, g, E)


@pytest.mark.parametrize("E", [2, 3, 32])
def test_analysis_t63(E, plans):
    """192 x 96 x 16, sigma_v = 0.1, next to test_analysis_t63_edges' E = 16: the clustered set (1 500 observations, more than three
    chunks of 256) and the sparse set in one network, compared at columns_for's columns and at every edge column in range of an
    observation, under the rule of test_analysis_on_grids, the limits' Jacobi route at 32 of the columns.  E = 32: one level in
    flight, all 256 threads on it, the largest LDS request, 18 432 workgroups"""
    sp, g = plans(T63, 32)
    assert (g.ix, g.il, g.kx) == (192, 96, 16) and levels_in_flight(E, g.kx) == (1 if E == 32 else 4)
    x = lk.ensemble(g, E, seed=63 + E)
    obs = lk.concat(lk.clustered_obs(g, x), lk.sparse_obs(g, x))
    assert len(obs["var"]) > 3 * lk.CHUNK
    edge = lk.edge_columns(g)
    edge = edge[lk.in_range(g, obs, edge).any(axis=1)]
    cols = np.unique(np.concatenate([lk.columns_for(g, obs, lk.SIGMA_H, most=32), edge]))
    assert len(edge) >= 100
    worst, kappa = compare("T63 L16", sp, g, x, obs, E, 0.1, cols, sample=32)
    assert max(worst.values()) <= 1.0, worst


def test_everything_at_once_t63(plans):
    """192 x 96 x 16, one object with every feature on (tests/letkfslots.py's EVERYTHING): E = 8 without member 5, the crafted network
    with observations at a pressure in three slots on drifting ensembles, weight stride (2, 2), the background check with planted
    gross errors, relaxation (0.3, 0.9) and adaptive inflation from a field in patches.  Two analysis calls, the second reads the
    field the first one wrote.  Each call: hx, slot_ps, slot_out, hxmean, y, departure and obs_lnsigma have the restatement's bits on
    the library's stencils, and so have the decisions, obs_rinv and the statistics' rows; the increments of the members in use, at a
    column of every stencil class and at columns_for's, against tests/letkfinterp.py's analysis fed keep, the stencils, r_eff, xs
    and first and the field the call read, then tests/letkfrelax.py's relaxation, within the larger of the interpolation rule (16 x
    the difference of the two eigen routes, 64 n eps max|x - mean|) and letkfrelax.limit; obs_s2 to the bit, the sums within
    letkfinfl.bound, and the field from the device's own sums to the bit"""
    sp, _ = plans(T63, 32)
    g = lp.Geometry(sp)                                          # ln fsg by the C library's log, as the host code forms it
    c, case = ls.EVERYTHING, ls.everything_inputs(g)
    x, xs, obs, first, keep = (case[n] for n in ("x", "xs", "obs", "first", "keep"))
    E, n, si, sj = c["E"], len(keep), *c["stride"]
    lt = ls.everything_object(sp, case)
    xc = lk.compact(x, keep)
    sc = lk.perturbation_scale(xc)
    idx, wgt = li.stencils(g, si, sj)
    cols = np.unique(np.concatenate(list(li.class_columns(g, si, sj).values()) + [lk.columns_for(g, obs, lk.SIGMA_H, most=24, outside=4)]))
    names = lk.FIELDS + ("slot_ps", "slot_out", "obs_check", "obs_rinv")
    last = None
    for call in range(2):
        before = lt.field("rho").numpy()
        assert support.same_bits(before.reshape(g.kx, -1), case["field"]) if call == 0 else support.same_bits(before, last["rho"])
        ls.observe_all(lt, xs, first)
        got = lk.run(lt, x, lm.flags(E, keep), slots=True, names=names)
        stats = qc.table(lt.obs_stats())
        # observation space, decisions and statistics
        want = lk.obs_space(g, x, obs, keep, lp.tables(lt), xs, first)
        for name in ("hx", "slot_ps", "slot_out", "hxmean", "y", "departure", "obs_lnsigma"):
            assert support.same_bits(got[name], want[name]), (call, name)
        dec = qc.check(want["y"], want["departure"], obs["error"], c["gross"], want["obs_used"], keep)
        assert qc.same_decisions(got, dec, obs), call
        out = want["obs_used"] == 0.0
        assert out.sum() >= 10 and (got["obs_check"][out] == qc.OUT).all() and (got["obs_check"][case["outside"]] != qc.PASSED).all()
        assert (got["obs_check"][np.setdiff1d(case["outside"], np.nonzero(out)[0])] == qc.REJECTED).all()
        assert (got["obs_check"][np.setdiff1d(case["inside"], np.nonzero(out)[0])] == qc.PASSED).all()
        assert qc.same_rows(stats, qc.stats(obs["var"], 5, dec["check"], want["departure"], dec["s2"], obs["error"])), call
        assert stats[:, 1].sum() == out.sum() and stats[:, 2].sum() == (dec["check"] == qc.REJECTED).sum() >= 8
        # the increments
        how = dict(keep=keep, stencil=lp.tables(lt), r_eff=qc.reff(dec["used"], 1.0 / (obs["error"] * obs["error"])), xs=xs, first=first)
        res = {}
        for route in ("eigh", "jacobi"):
            raw, _, _ = li.analyse(g, x, obs, lk.SIGMA_H, c["sigma_v"], before, si, sj, route, cols, (idx, wgt), **how)
            res[route] = lr.relax(lr.at_columns(xc, cols), raw, *c["relaxation"])
        (ref, f), (alt, _) = res["eigh"], res["jacobi"]
        worst = {}
        for v in lk.VARS:
            lim = np.maximum(max(16 * float(np.max(np.abs(ref[v] - alt[v]))), 64 * n * lk.EPS * sc[v]), lr.limit(xc, f, n, v))
            worst[v] = float(np.max(np.abs(lk.at_columns(got[v][list(keep)], cols) - ref[v]) / lim[None]))
            assert ref[v].any() and lm.zero_bits(got[v][c["drop"]]), v
        # adaptive inflation
        s2o, p, bound, _ = lf.restate(g, lt, before.reshape(g.kx, -1)[:, cols], lk.SIGMA_H, c["sigma_v"], c["sigma_b"], keep=keep,
                                      reff_field=True, cols=cols)
        worst["sums"] = lf.worst_ratio(got["infl_parm"].reshape(3, g.kx, -1)[:, :, cols], p, bound)
        print("[letkf everything T63 L16 call %d] %d columns, %d rejected, %d out of column, largest f %.3f, ratio to the limit: %s"
              % (call, len(cols), int(stats[:, 2].sum()), int(out.sum()), max(float(a.max()) for a in f.values()),
                 " ".join("%s %.3f" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, (call, worst)
        assert support.same_bits(got["obs_s2"], s2o), call
        assert support.same_bits(got["rho"], lf.update(before, got["infl_parm"], c["sigma_b"])) and not support.same_bits(got["rho"], before)
        assert last is None or any(not support.same_bits(got[v], last[v]) for v in lk.VARS)
        last = got
    lt.close()
