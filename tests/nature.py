"""The nature run restated in NumPy (include/spdy.h, "nature run"): the observation values drawn from a gridded truth and the
scores of a gridded ensemble against it, exactly as the header defines them.  The operator's stencils and the layouts are those of
tests/letkf.py, the noise is tests/sppt.py's generator.

A truth is {"u", "v", "t", "q": (kx, il, ix), "ps": (il, ix)}, one member of letkf.py's gridded ensemble; scores are
{"rmse" | "bias" | "spread": {"u", "v", "t", "q": [kx], "ps": float}}, what Nature.scores(slot) returns."""
import numpy as np

import letkf as lk
import sppt

SCORES = ("rmse", "bias", "spread")


def gaussian_weights(sp):
    """the plan's Gaussian weights of the rows, south first (the table "wt" holds a hemisphere)"""
    wt = sp.table("wt")
    return np.concatenate([wt, wt[::-1]])


def normalised(weights):
    """g_j: the weights divided by their sum over j ascending"""
    s = 0.0
    for w in weights:
        s = s + float(w)
    return np.asarray(weights, np.float64) / s


def rows(truth):
    """the truth as the library holds it: (4 kx + 1, il, ix), u, v, t, q by level, then ps"""
    return np.concatenate([truth[v] for v in lk.VARS[:4]] + [truth["ps"][None]])


def as_truth(x, e=0):
    """member e of a gridded ensemble as a truth"""
    return {v: np.ascontiguousarray(x[v][e]) for v in lk.VARS}


def operator(g, truth, obs_network):
    """h_o = ((w0 x0 + w1 x1) + w2 x2) + w3 x3 on the truth"""
    idx, w = lk.stencil(g, obs_network["lon"], obs_network["lat"])
    h = np.zeros(len(obs_network["var"]))
    for o in range(len(h)):
        v = int(obs_network["var"][o])
        f = truth[lk.VARS[v]].reshape(-1, g.il * g.ix)[0 if v == lk.PS else int(obs_network["lev"][o])]
        i = idx[o]
        h[o] = ((w[o, 0] * f[i[0]] + w[o, 1] * f[i[1]]) + w[o, 2] * f[i[2]]) + w[o, 3] * f[i[3]]
    return h


def draw(seed, draws, nobs):
    """z_o of draw number `draws`: the real part of SPPT's draw of index o"""
    return sppt.raw_noise(int(seed), int(draws), int(nobs)).real if nobs else np.zeros(0)


def observe(g, truth, obs_network, errors, seed, draws, noise):
    """value_o = h_o + (noise * error_o) * z_o; with noise == 0 the product is not formed"""
    h = operator(g, truth, obs_network)
    if noise == 0.0:
        return h
    return h + (noise * np.asarray(errors, np.float64)) * draw(seed, draws, len(h))


def scores(g, x, truth, weights):
    """rmse, bias and spread of every row: d_e = x_e - truth, mbar = (sum_e d_e, e ascending) / E, s2 = (sum_e (d_e - mbar)^2, e
    ascending) / (E - 1); <a> = sum_j g_j ((sum_i a[j][i]) / ix), j ascending"""
    gw = normalised(weights)
    out = {n: {} for n in SCORES}
    for v in lk.VARS:
        E = x[v].shape[0]
        d = x[v].reshape(E, -1, g.il, g.ix) - truth[v].reshape(-1, g.il, g.ix)[None]
        s = np.zeros(d.shape[1:])
        for e in range(E):
            s = s + d[e]
        mbar = s / E
        q = np.zeros(d.shape[1:])
        for e in range(E):
            r = d[e] - mbar
            q = q + r * r
        s2 = q / (E - 1)

        def mean(a):
            zonal = a.sum(axis=-1) / g.ix
            acc = np.zeros(a.shape[0])
            for j in range(g.il):
                acc = acc + gw[j] * zonal[:, j]
            return acc
        res = {"rmse": np.sqrt(mean(mbar * mbar)), "bias": mean(mbar), "spread": np.sqrt(mean(s2))}
        for n in SCORES:
            out[n][v] = float(res[n][0]) if v == "ps" else res[n]
    return out


def flat(sc):
    """scores as the library's table of a slot: (3, 4 kx + 1)"""
    return np.stack([np.concatenate([np.atleast_1d(sc[n][v]) for v in lk.VARS]) for n in SCORES])


def analysed(x, inc, g):
    """x + the increments of letkf.analyse on all columns ((E, kx, ncol) / (E, ncol))"""
    return {v: x[v] + inc[v].reshape(x[v].shape) for v in lk.VARS}


# ---------------------------------------------------------------------------------------------------- the twin experiment
TWIN = {"kx": 2, "E": 6, "nobs": 400, "sigma_h": 1.0e6, "sigma_v": 0.0, "rho": 1.0, "base_seed": 70, "truth_seed": 71,
        "ensemble_seed": 72, "network_seed": 73, "noise_seed": 0x7717, "err_factor": 0.25, "passes": 100}


def twin_sigma(kx):
    return np.linspace(0.0, 1.0, kx + 1) ** 1.5


def smooth(a, passes):
    """`passes` 1-2-1 averages along the longitudes (periodic) and the latitudes (the outermost rows repeated)"""
    for _ in range(passes):
        a = 0.25 * np.roll(a, 1, -1) + 0.5 * a + 0.25 * np.roll(a, -1, -1)
        up = np.concatenate([a[..., :1, :], a[..., :-1, :]], axis=-2)
        down = np.concatenate([a[..., 1:, :], a[..., -1:, :]], axis=-2)
        a = 0.25 * up + 0.5 * a + 0.25 * down
    return a


def smooth_errors(g, E, seed, passes):
    """E fields per variable of spatially correlated noise with SCALE's spread: the difference of two of letkf.ensemble's draws is
    white noise (their base state cancels), smoothed and scaled back"""
    a, b = lk.ensemble(g, E, seed), lk.ensemble(g, E, seed + 500)
    out = {}
    for v in lk.VARS:
        n = smooth(a[v] - b[v], passes)
        out[v] = n * (lk.SCALE[v][1] / n.std())
    return out


def twin_inputs(g):
    """The twin experiment of the tests at T30, kx = 2, E = 6.  Truth and members are one of tests/letkf.ensemble's states plus
    errors drawn from it with different seeds; the errors are smoothed (100 passes of 1-2-1: a Gaussian of about 7 grid intervals,
    2 900 km at the equator) because white noise has as many degrees of freedom as grid points and no six members span it: with the
    draws as they come the analysis of the restatement is 20 % WORSE than the background, with these errors the local problems have
    a handful of degrees of freedom inside the localisation radius.  The network: 400 observations of t (both levels) and ps,
    uniform on the sphere, errors a quarter of the background's spread.  c_h = sigma_h sqrt(10/3) = 1 826 km and 2 c_h is the
    support, so about 400 pi (2 c_h)^2 / (4 pi rearth^2) = 33 observations reach a column; asserted: every column is in range of at
    least one (the farthest is at half the support)."""
    c = TWIN
    ref = lk.ensemble(g, 1, seed=c["base_seed"])
    et, ee = smooth_errors(g, 1, c["truth_seed"], c["passes"]), smooth_errors(g, c["E"], c["ensemble_seed"], c["passes"])
    truth = {v: np.ascontiguousarray((ref[v] + et[v])[0]) for v in lk.VARS}
    x = {v: ref[v] + ee[v] for v in lk.VARS}
    rng = np.random.default_rng(c["network_seed"])
    n = c["nobs"]
    var = np.where(np.arange(n) % 3 == 2, lk.PS, lk.T)
    lev = np.arange(n) % g.kx
    lon, lat = rng.uniform(0.0, 360.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    err = c["err_factor"] * np.array([lk.SCALE[lk.VARS[v]][1] for v in var])
    net = lk.make_obs(var, lev, lon, lat, np.zeros(n), err)
    reach = lk.distance(g.colunit, lk.unit(lon, lat)).min(axis=1)
    assert float(reach.max()) < 2.0 * c["sigma_h"] * np.sqrt(10.0 / 3.0)
    return truth, x, net
