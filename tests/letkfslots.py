"""Observations in time slots, restated in NumPy (include/spdy.h, "ensemble analysis, observations in time slots"):
observing a slot keeps what is per member -- hx, and for a network with observations at a pressure the stencil's ps and the
out-of-column flag of every member -- by tests/letkf.py's and tests/letkfpressure.py's operators on the ensemble of the slot's
time; the finish forms everything that couples members from those rows, over the members in use in ascending order; the local
problems and the increments are tests/letkf.py's, the increments on the ensemble of the analysis time.  Also the ensembles that
drift over a window and what the GPU tests share.

An observation set is tests/letkf.py's dict, with "p" (tests/letkfpressure.py) when the network may hold observations at a
pressure; `first` is the slots' ranges, S + 1 integers; `xs` is a list of S gridded ensembles, xs[s] the one slot s is observed on."""
import numpy as np

import letkf as lk
import letkfpressure as lp
import nature as nt
import support

FIELDS = ("hx", "hxmean", "y", "departure", "obs_lnsigma", "obs_used")
SLOT_FIELDS = ("hx", "slot_ps", "slot_out")
PER_OBS = ("hxmean", "departure", "obs_lnsigma", "obs_used")
FIRST = lambda nobs: [0, 1, 1, 300, nobs]      # a one-observation slot, an empty one, a boundary inside a chunk of 256, a long tail


def at_pressure(obs):
    """which observations are at a pressure; none for a set without "p" """
    return lp.at_pressure(obs) if "p" in obs else np.zeros(len(obs["var"]), bool)


def with_p(obs):
    return obs if "p" in obs else dict(obs, p=np.zeros(len(obs["var"])))


def check_first(first, nobs):
    first = [int(f) for f in first]
    assert len(first) >= 2 and first[0] == 0 and first[-1] == nobs and all(a <= b for a, b in zip(first, first[1:])), (first, nobs)
    return first


def observe_slot(g, x, obs, rows, stencil=None):
    """what observing the observations `rows` (a slice) on the ensemble x keeps -> hx (n, E), slot_ps (n, E), slot_out (n, E); the
    last two are zero for a network without an observation at a pressure"""
    sub = lp.subset(obs, rows)
    st = None if stencil is None else (stencil[0][rows], stencil[1][rows])
    E, n = x["ps"].shape[0], len(sub["var"])
    pres = at_pressure(obs).any()
    if stencil is None and not pres:
        hx = lk.obs_space(g, x, sub)[0]
    else:
        hx = lp.obs_space(g, x, with_p(sub), st)["hx"]
    ps, out = np.zeros((n, E)), np.zeros((n, E))
    if pres:
        idx, w = lk.stencil(g, sub["lon"], sub["lat"]) if st is None else st
        atp, xo = lp.at_pressure(sub), lp.lnp(sub)
        for o in range(n):
            ps4 = x["ps"].reshape(E, -1)[:, idx[o]]
            ps[o] = ((w[o, 0] * ps4[:, 0] + w[o, 1] * ps4[:, 1]) + w[o, 2] * ps4[:, 2]) + w[o, 3] * ps4[:, 3]
            if atp[o]:
                X = ps4[:, None, :] + g.lnf[None, :, None]
                with np.errstate(invalid="ignore"):
                    out[o] = ((xo[o] < X[:, 0]) | (xo[o] > X[:, g.kx - 1])).any(axis=1)
    return hx, ps, out


def finish(g, obs, hx, slot_ps, slot_out, keep=None):
    """the finish kernel's formulas on the slots' rows: the sums over the members `keep` (default: all) in ascending order"""
    E = hx.shape[1]
    keep = list(range(E)) if keep is None else sorted(keep)
    n, nobs = len(keep), hx.shape[0]
    s = np.zeros(nobs)
    for e in keep:
        s = s + hx[:, e]
    with np.errstate(all="ignore"):
        hxmean = s / n if n else np.full(nobs, np.nan)
        y = np.zeros_like(hx)
        y[:, keep] = hx[:, keep] - hxmean[:, None]
    atp = at_pressure(obs)
    lns = lk.lnsigma(g, dict(obs, lev=np.where(atp, 0, obs["lev"])))
    used = np.ones(nobs)
    if atp.any():
        xo, p = lp.lnp(obs), np.zeros(nobs)
        for e in keep:
            p = p + slot_ps[:, e]
        with np.errstate(all="ignore"):
            lns = np.where(atp, xo - p / n, lns) if n else np.where(atp, np.nan, lns)
        used = np.where((slot_out[:, keep] != 0.0).any(axis=1), 0.0, 1.0)
    return {"hx": hx, "hxmean": hxmean, "y": y, "departure": obs["value"] - hxmean, "obs_lnsigma": lns, "obs_used": used,
            "slot_ps": slot_ps, "slot_out": slot_out}


def obs_space_slots(g, xs, obs, first, keep=None, stencil=None):
    """hx row range by row range on xs[s], slot_ps and slot_out next to it, then the finish -> tests/letkfpressure.py's obs_space
    dict with "slot_ps" and "slot_out" (nobs, E) added"""
    nobs = len(obs["var"])
    first = check_first(first, nobs)
    assert len(xs) == len(first) - 1
    E = xs[0]["ps"].shape[0]
    hx, ps, out = np.zeros((nobs, E)), np.zeros((nobs, E)), np.zeros((nobs, E))
    for s, x in enumerate(xs):
        rows = slice(first[s], first[s + 1])
        if first[s + 1] > first[s]:
            hx[rows], ps[rows], out[rows] = observe_slot(g, x, obs, rows, stencil)
    return finish(g, obs, hx, ps, out, keep)


def problems_from(g, obs, s, sigma_h, sigma_v, cols=None, keep=None):
    """C (ncols, kx, n, n) and b (ncols, kx, n) from an obs_space dict s: Y of the members `keep`, d, ln sigma_o and the use of that
    dict, by tests/letkf.py's weights and ascending sums (tests/letkfpressure.py's `problems`, fed from the slots)"""
    cols = np.arange(g.ix * g.il) if cols is None else np.asarray(cols)
    E = s["hx"].shape[1]
    keep = list(range(E)) if keep is None else sorted(keep)
    n, kx, nc, nobs = len(keep), g.kx, len(cols), len(obs["var"])
    C, b = np.zeros((nc, kx, n, n)), np.zeros((nc, kx, n))
    if nobs:
        Y, d = s["y"][:, keep], s["departure"]
        wh = lk.gc(lk.distance(g.colunit[cols], lk.unit(obs["lon"], obs["lat"])) / (sigma_h * np.sqrt(10.0 / 3.0)))
        if sigma_v > 0.0:
            wv = lk.gc(np.abs(g.lnfsg[:, None] - s["obs_lnsigma"][None, :]) / (sigma_v * np.sqrt(10.0 / 3.0)))
            wt = wh[:, None, :] * wv[None, :, :]
        else:
            wt = np.repeat(wh[:, None, :], kx, axis=1)
        r = wt * (s["obs_used"] * (1.0 / (obs["error"] * obs["error"])))[None, None, :]
        with np.errstate(invalid="ignore"):
            for o in np.nonzero((r != 0.0).any(axis=(0, 1)))[0]:      # ascending; elsewhere r == 0 adds an exact zero
                at = (r[:, :, o] != 0.0).any(axis=1)
                C[at] += r[at, :, o, None, None] * (Y[o][:, None] * Y[o][None, :])
                b[at] += r[at, :, o, None] * (Y[o] * d[o])
    return C, b


def problems_slots(g, xs, obs, first, sigma_h, sigma_v, cols=None, keep=None, stencil=None):
    """-> (C, b, the obs_space dict): the local problems of the slot analysis at the grid columns `cols` (default: all)"""
    s = obs_space_slots(g, xs, obs, first, keep, stencil)
    C, b = problems_from(g, obs, s, sigma_h, sigma_v, cols, keep)
    return C, b, s


def compact(x, keep):
    return x if keep is None else {v: np.ascontiguousarray(x[v][sorted(keep)]) for v in lk.VARS}


def analyse_slots(g, x, xs, obs, first, sigma_h, sigma_v, rho, route="eigh", cols=None, keep=None, stencil=None):
    """The increments of the members in use of the analysis-time ensemble x at the grid columns `cols`, and the largest condition
    number: Y and d from the slots' times, dx_e = sum_f (x_f - xmean) T[f][e] on x"""
    C, b, _ = problems_slots(g, xs, obs, first, sigma_h, sigma_v, cols, keep, stencil)
    return lk.increments(g, compact(x, keep), C, b, rho, route, cols)


DRIFT, DRIFT_PASSES = 0.25, 8


def drifting(g, x, S, seed, fraction=DRIFT):
    """S ensembles for a window that ends at x: xs[s] = x + (S - 1 - s) fraction (member spread) (a smooth seeded field of unit
    standard deviation per member and variable), so the difference grows with the distance from the last slot; the last one is x"""
    rng = np.random.default_rng(seed)
    xs = []
    for s in range(S - 1):
        y = {}
        for v in lk.VARS:
            f = nt.smooth(rng.standard_normal(x[v].shape), DRIFT_PASSES)
            y[v] = x[v] + ((S - 1 - s) * fraction * lk.SCALE[v][1] / f.std()) * f
        xs.append(y)
    return xs + [x]


def push_out(g, xs, obs, first, slot, member):
    """Lowers xs[slot]'s ps of `member` at the four points of one at-pressure observation of the slot, so far in column for every
    member at every time, until the observation lies below that member's lowest level at the slot's time only -> (the ensembles
    with xs[slot] replaced, the observation).  The one with the largest target is taken: the smallest push"""
    first = check_first(first, len(obs["var"]))
    idx, _ = lk.stencil(g, obs["lon"], obs["lat"])
    inside = np.ones(len(obs["var"]), bool)
    for x in xs:
        inside &= lp.obs_space(g, x, obs)["obs_used"] == 1.0
    xo = lp.lnp(obs)
    rows = np.arange(first[slot], first[slot + 1])
    rows = rows[lp.at_pressure(obs)[rows] & inside[rows]]
    assert len(rows), "no at-pressure observation of slot %d is in every member's column" % slot
    o = int(rows[np.argmax(xo[rows])])
    y = {v: a.copy() for v, a in xs[slot].items()}
    y["ps"].reshape(y["ps"].shape[0], -1)[member, idx[o]] = xo[o] - g.lnf[-1] - 0.02      # X_{kx-1} = x_o - 0.02 < x_o
    return xs[:slot] + [y] + xs[slot + 1:], o


# ------------------------------------------------------------------------------------------------ what the GPU tests share
def grids(x):
    return [support.dev(x[v]) for v in lk.VARS]


def observe_all(lt, xs, first):
    """set_slots(first), then every slot observed on its ensemble (NumPy, or a list of five device tensors)"""
    lt.set_slots(first)
    for s, x in enumerate(xs):
        lt.observe_grid(s, *(grids(x) if isinstance(x, dict) else x))


def analyse(lt, x, use=None, slots=False, names=FIELDS):
    """Letkf.analyse_grid on the NumPy ensemble x -> the increments, the observation-space fields, members_used, and inflation and
    weights where the object has them, as NumPy arrays"""
    import torch
    out = lt.analyse_grid(*grids(x), use=use, slots=slots)
    torch.cuda.synchronize()
    got = {v: a.cpu().numpy() for v, a in zip(lk.VARS, out)}
    if lt.nobs:
        got.update({n: lt.field(n).numpy().copy() for n in names})
    got["members_used"] = lt.field("members_used").numpy().copy()
    if lt.relaxation != (0.0, 0.0):
        got["inflation"] = lt.field("inflation").numpy().copy()
    if lt.weight_stride != (1, 1):
        got["weights"] = lt.field("weights").numpy().copy()
    return got
