"""Observations given at a pressure, restated in NumPy (include/spdy.h, "ensemble analysis, observations at a pressure") in the
header's operation order: the per-member vertical interpolation of the four stencil columns by np.interp's rule, linear in ln p
(tests/pressurelevels.py has the bracket), the bilinear sum, the vertical position the localisation uses and which observations
take part.  tests/letkf.py's `observe` calls the interpolation here for an observation at a pressure, and its `couple` forms the
position and the use; the rest of the analysis is that module's.  Also the crafted gridded ensembles and networks of the tests and
the classes they hold.

An observation set is tests/letkf.py's dict with one array more, "p" in Pa; lev == AT_P marks an observation at its p."""
import math

import numpy as np

import letkf as lk
import pressurelevels as pl
from ensembleoutput import P0

AT_P, at_pressure = lk.AT_P, lk.at_pressure
SOUNDING = (92500.0, 85000.0, 70000.0, 50000.0, 30000.0, 20000.0, 10000.0)      # Pa: a radiosonde's mandatory levels


class Geometry(lk.Geometry):
    """letkf.Geometry and ln fsg by math.log, the C library's logarithm the host code forms the level table with"""

    def __init__(self, sp):
        super().__init__(sp)
        self.fsg = np.asarray(sp.table("fsg"), np.float64)
        self.lnf = np.array([math.log(float(f)) for f in self.fsg])


def make_pobs(var, lev, p, lon, lat, value, error):
    obs = lk.make_obs(var, lev, lon, lat, value, error)
    obs["p"] = np.asarray(p, np.float64).reshape(len(obs["var"]))
    return obs


def args(obs):
    """the arguments of Letkf.set_obs with p"""
    return lk.args(obs) + [obs["p"]]


def lnp(obs):
    """x_o = ln(p_o / p0) by the C library's log; 0 for an observation that is not at a pressure"""
    return np.array([math.log(float(p) / P0) if a else 0.0 for p, a in zip(obs["p"], at_pressure(obs))])


def column_values(X, f, x):
    """np.interp's rule for one target x in the columns X (E, kx, ...) with the values f (E, kx, ...): the end level's bits outside,
    f[kb] + w (f[kb+1] - f[kb]) inside -> (z, kb, lo, hi, out): out = x < X_0 or x > X_{kx-1}"""
    kx = X.shape[1]
    kb, k1, lo, hi, below, w = pl.brackets(X, x)
    with np.errstate(all="ignore"):
        f0 = np.take_along_axis(f, kb[:, None], axis=1)[:, 0]
        f1 = np.take_along_axis(f, k1[:, None], axis=1)[:, 0]
        d = f1 - f0
        y = f0 + w * d
        return np.where(lo, f0, np.where(hi, f1, y)), kb, lo, hi, (x < X[:, 0]) | (x > X[:, kx - 1])


def stencil_columns(g, x, obs, o, idx):
    """of observation o: ps (E, 4), X (E, kx, 4), f (E, kx, 4) at its four points"""
    E = x["ps"].shape[0]
    ps4 = x["ps"].reshape(E, -1)[:, idx[o]]
    X = ps4[:, None, :] + g.lnf[None, :, None]
    f = x[lk.VARS[int(obs["var"][o])]].reshape(E, g.kx, -1)[:, :, idx[o]]
    return ps4, X, f


def tables(lt):
    """the stencils an analysis object built for its observations, for letkf.observe: the library's own bits (tests/letkf.py's
    stencil agrees with them to a few ulps, tests/test_letkf_cpu.py)"""
    return lt.table("stencil_index"), lt.table("stencil_weight")


def truth_values(g, truth, obs, stencil=None):
    """h_o of the nature run: the operator on the truth with the truth's ps, clamped where the truth is out of column"""
    return lk.observe(g, {v: truth[v][None] for v in lk.VARS}, obs, stencil)[0][:, 0]


# ---------------------------------------------------------------------------------------------------- crafted inputs
PATCH_ROWS, PATCH_COLS, PATCH_MEMBER = (20, 23), (40, 44), 1      # the high-terrain patch: rows, longitudes (half-open), member
HIGH = math.log(0.6)


def craft(g, E, seed):
    """A gridded ensemble: letkf.ensemble's fields (smooth in the vertical plus member noise), ps random in +-0.05 per member and
    point, exactly 0 in rows 0..3, and ln 0.6 for member PATCH_MEMBER in the patch"""
    x = lk.ensemble(g, E, seed)
    x["ps"] = np.random.default_rng(seed + 1000).uniform(-0.05, 0.05, x["ps"].shape)
    x["ps"][:, :4] = 0.0
    x["ps"][PATCH_MEMBER, PATCH_ROWS[0]:PATCH_ROWS[1], PATCH_COLS[0]:PATCH_COLS[1]] = HIGH
    return x


def targets(g):
    """(name, ln(p/p0)) of the crafted network's pressures: the middle of every bracket; just past every inner level (members with
    ps above 0.01 are a bracket lower); in [X_0, X_1) and (X_{kx-2}, X_{kx-1}] of every member with |ps| <= 0.05; above every top"""
    t = [("mid%d" % k, 0.5 * (g.lnf[k] + g.lnf[k + 1])) for k in range(g.kx - 1)]
    t += [("near%d" % k, g.lnf[k] + 0.01) for k in range(1, g.kx - 1)]
    return t + [("first", g.lnf[0] + 0.06), ("last", g.lnf[-1] - 0.06), ("above", g.lnf[0] - 0.2)]


def network(g, x, seed=5, nrandom=16, err_factor=0.5):
    """About 600 observations in an order that mixes the kinds: every target of `targets` as u, v, t or q at letkf.edge_points
    (date line, poles) and at random places; stations in and on the edge of the high-terrain patch at `last` (the patch member is
    below: rejected) and at a mid-column pressure (used); stations in the rows with ps = 0 at p0 fsg[k], on a model level; tests/
    letkf.py's model-level and PS observations.  Values are member 0's plus noise of the errors' size."""
    rng = np.random.default_rng(seed)
    rows = []                                            # (var, lev, p, lon, lat)
    pts = lk.edge_points(g) + [(float(rng.uniform(-400, 400)), float(rng.uniform(-85, 85))) for _ in range(nrandom)]
    n = 0
    for name, xo in targets(g):
        for lon, lat in pts:
            rows.append((n % 4, AT_P, P0 * math.exp(xo), lon, lat))
            n += 1
    j0, j1 = PATCH_ROWS
    i0, i1 = PATCH_COLS
    dlon = 360.0 / g.ix
    for lat in (float(g.lat[j0]) - 0.5, float(g.lat[j0]) + 0.5, 0.5 * float(g.lat[j0] + g.lat[j1 - 1]), float(g.lat[j1 - 1]) + 0.5):
        for lon in ((i0 - 0.5) * dlon, (i0 + 0.5) * dlon, (i1 - 1.5) * dlon, (i1 - 0.5) * dlon):
            for name, xo in (("last", g.lnf[-1] - 0.06), ("mid0", 0.5 * (g.lnf[0] + g.lnf[1]))):
                rows.append((n % 4, AT_P, P0 * math.exp(xo), lon, lat))
                n += 1
    for k in range(g.kx):
        for lon in (3.0, 121.7, 359.9):
            rows.append((n % 4, AT_P, P0 * float(g.fsg[k]), lon, 0.5 * float(g.lat[1] + g.lat[2])))
            n += 1
    model = lk.edge_obs(g, x, nrandom=60, err_factor=err_factor, seed=seed)
    var = np.concatenate([[r[0] for r in rows], model["var"]])
    order = rng.permutation(len(var))
    take = lambda a, b: np.concatenate([np.asarray(a, np.float64), np.asarray(b, np.float64)])[order]
    obs = make_pobs(var[order], take([r[1] for r in rows], model["lev"]), take([r[2] for r in rows], np.zeros(len(model["var"]))),
                    take([r[3] for r in rows], model["lon"]), take([r[4] for r in rows], model["lat"]), np.zeros(len(var)),
                    err_factor * np.array([lk.SCALE[lk.VARS[v]][1] for v in var[order]]))
    obs["value"] = lk.observe(g, x, obs)[0][:, 0] + obs["error"] * rng.standard_normal(len(var))
    return obs


def classes(g, x, obs):
    """the classes of (member, point) target a crafted pair of ensemble and network holds -> a set of names"""
    idx, _ = lk.stencil(g, obs["lon"], obs["lat"])
    atp, xo, found = at_pressure(obs), lnp(obs), set()
    found |= {"model_level"} if (~atp & (obs["var"] != lk.PS)).any() else set()
    found |= {"ps"} if (obs["var"] == lk.PS).any() else set()
    jj = idx // g.ix
    ii = idx % g.ix
    for o in np.nonzero(atp)[0]:
        ps4, X, f = stencil_columns(g, x, obs, o, idx)
        _, kb, lo, hi, out = column_values(X, f, xo[o])
        inside = ~lo & ~hi
        found |= {"bracket%d" % k for k in np.unique(kb[inside])}
        below, above = xo[o] > X[:, -1], xo[o] < X[:, 0]
        if not out.any():
            found.add("used")
            if inside.all() and kb.min() != kb.max():
                found.add("brackets_differ")
            if (inside & (kb == 0)).all():
                found.add("first_bracket")
            if (inside & (kb == g.kx - 2)).all():
                found.add("last_bracket")
            if (xo[o] == X[:, 0]).any() or (xo[o] == X[:, -1]).any():
                found.add("on_end_level")
        if above.all():
            found.add("above_all")
        if below.any() and not np.delete(below, PATCH_MEMBER, axis=0).any():
            found.add("below_one_member" if below[PATCH_MEMBER].all() else "below_one_point" if below.sum() == 1 else "below_some_points")
        if ii[o].max() - ii[o].min() == g.ix - 1:
            found.add("date_line")
        if jj[o].min() == jj[o].max():
            found.add("poleward")
    return found


def every_class(kx):
    inner = {"brackets_differ"} if kx > 2 else set()
    return ({"bracket%d" % k for k in range(kx - 1)} | inner | {"model_level", "ps", "used", "first_bracket", "last_bracket", "on_end_level",
            "above_all", "below_one_point", "below_some_points", "below_one_member", "date_line", "poleward"})


def margin(g, x, obs):
    """the smallest |x_o - X_0| and |x_o - X_{kx-1}| over the at-pressure observations, members and points"""
    idx, _ = lk.stencil(g, obs["lon"], obs["lat"])
    xo, m = lnp(obs), np.inf
    for o in np.nonzero(at_pressure(obs))[0]:
        _, X, _ = stencil_columns(g, x, obs, o, idx)
        m = min(m, float(np.min(np.abs(xo[o] - X[:, 0]))), float(np.min(np.abs(xo[o] - X[:, -1]))))
    return m


def sounding_network(g, n_stations, seed, err_factor=0.25, variables=(lk.U, lk.V, lk.T)):
    """n_stations radiosonde-like stations uniform on the sphere: SOUNDING's pressures, the given variables at each; values 0"""
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(0.0, 360.0, n_stations), np.degrees(np.arcsin(rng.uniform(-0.97, 0.97, n_stations)))
    rows = [(v, AT_P, p, lon[s], lat[s]) for s in range(n_stations) for p in SOUNDING for v in variables]
    var = np.array([r[0] for r in rows])
    return make_pobs(var, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], np.zeros(len(rows)),
                     err_factor * np.array([lk.SCALE[lk.VARS[v]][1] for v in var]))


TWIN_STATIONS, TWIN_VALUE_SEED = 130, 5


def twin_inputs(g):
    """tests/nature.py's twin experiment (T30, kx = 2, E = 6, smoothed errors) with a network of TWIN_STATIONS radiosonde-like
    stations that report u, v and t at SOUNDING's pressures.  With fsg = 0.177 and 0.677 the reports at 500, 300 and 200 hPa are in
    column, both levels bracket them; those at 925, 850, 700 hPa lie below the lowest level and that at 100 hPa above the top one:
    rejected.  -> (truth, ensemble, network with values 0)"""
    import nature as nt
    truth, x, _ = nt.twin_inputs(g)
    return truth, x, sounding_network(g, TWIN_STATIONS, nt.TWIN["network_seed"], nt.TWIN["err_factor"])


def twin_ratios(g, x, inc, truth, weights):
    """rmse of the analysis mean over the background's, {"u", "v", "t": [kx]}; inc: the increments on all columns"""
    import nature as nt
    sb, sa = nt.scores(g, x, truth, weights), nt.scores(g, nt.analysed(x, inc, g), truth, weights)
    return {v: sa["rmse"][v] / sb["rmse"][v] for v in ("u", "v", "t")}


SPECTRAL_STATIONS, SPECTRAL_SIGMA_V, MARGIN = 8, 0.3, 1e-9


def spectral_case(sp, o, g, E, stations=SPECTRAL_STATIONS):
    """The analysis from spectra: tests/ensemblestep.py's member states (the standard test ensemble), their grids by the oracle's
    transforms, and `stations` radiosonde-like stations reporting u, v, t and q at SOUNDING's pressures, each with half the
    members' spread at its place as error and a value one such error around member 0's -> (states, grids, network)"""
    import ensemblestep as es
    sts = es.member_states(sp, E)
    x = lk.oracle_grids(o, sts)
    net = sounding_network(g, stations, seed=90, variables=(lk.U, lk.V, lk.T, lk.Q))
    hx = lk.observe(g, x, net)[0]
    net["error"] = 0.5 * hx.std(axis=1, ddof=1) + 1e-300
    net["value"] = hx[:, 0] + net["error"] * np.random.default_rng(91).standard_normal(len(net["var"]))
    return sts, x, net


def to_spectra(o, g, sts, inc):
    """the analysed time level 1 of every member: the increments inc on all grid columns through the oracle's vdspec and
    grid_to_spec (tests/test_gpu_letkf.py's route) -> per member {vor, div, t, tr, ps}"""
    grid = lambda a: a.reshape(a.shape[:-1] + (g.il, g.ix))
    out = []
    for e, st in enumerate(sts):
        vd = [o.vdspec(grid(inc["u"][e])[k], grid(inc["v"][e])[k], 2) for k in range(o.kx)]
        out.append({"vor": st["vor"][0] + np.stack([a for a, _ in vd]), "div": st["div"][0] + np.stack([b_ for _, b_ in vd]),
                    "t": st["t"][0] + np.stack([o.grid_to_spec(grid(inc["t"][e])[k]) for k in range(o.kx)]),
                    "tr": st["tr"][0] + np.stack([o.grid_to_spec(grid(inc["q"][e])[k]) for k in range(o.kx)]),
                    "ps": st["ps"][0] + o.grid_to_spec(grid(inc["ps"][e]))})
    return out


def spectral_analysis(o, g, sts, x, net, rho=lk.RHO):
    """the restatement's increments on the oracle's grids, through `to_spectra` -> (per member {vor, div, t, tr, ps}, obs_space)"""
    space = lk.obs_space(g, x, net)
    C, b = lk.problems(g, net, space, lk.SIGMA_H, SPECTRAL_SIGMA_V)
    inc, _ = lk.increments(g, x, C, b, rho)
    return to_spectra(o, g, sts, inc), space


def make(sp, E, obs, sigma_v=0.0, rho=lk.RHO, sigma_h=lk.SIGMA_H):
    """the analysis object of E members with the observations obs set through spdy_pobs_set"""
    import speedy_f90_amd as s
    lt = s.Letkf(sp, E, max(len(obs["var"]), 1), sigma_h, sigma_v, rho)
    lt.set_obs(*args(obs))
    return lt
