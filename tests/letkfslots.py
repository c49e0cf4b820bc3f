"""Observations in time slots (include/spdy.h, "ensemble analysis, observations in time slots").  The restatement is
tests/letkf.py's with xs and first given: `observe` on the ensemble of each slot's time keeps what is per member, `couple` forms
everything that couples members from those rows, the increments are formed on the ensemble of the analysis time.  Here: the row
ranges the tests use, the ensembles that drift over a window, and what the GPU tests share.

An observation set is tests/letkf.py's dict, with "p" (tests/letkfpressure.py) when the network may hold observations at a
pressure; `first` is the slots' ranges, S + 1 integers; `xs` is a list of S gridded ensembles, xs[s] the one slot s is observed on."""
import numpy as np

import letkf as lk
import letkfpressure as lp
import nature as nt

SLOT_FIELDS = ("hx", "slot_ps", "slot_out")
PER_OBS = ("hxmean", "departure", "obs_lnsigma", "obs_used")
FIRST = lambda nobs: [0, 1, 1, 300, nobs]      # a one-observation slot, an empty one, a boundary inside a chunk of 256, a long tail


DRIFT, DRIFT_PASSES = 0.25, 8


def drifting(g, x, S, seed, fraction=DRIFT, passes=DRIFT_PASSES):
    """S ensembles for a window that ends at x: xs[s] = x + (S - 1 - s) fraction (member spread) (a smooth seeded field of unit
    standard deviation per member and variable), so the difference grows with the distance from the last slot; the last one is x.
    passes: the smoothing of the seeded field, 1-2-1 averages (fewer where a large ensemble on a large grid makes them the cost)"""
    rng = np.random.default_rng(seed)
    xs = []
    for s in range(S - 1):
        y = {}
        for v in lk.VARS:
            f = nt.smooth(rng.standard_normal(x[v].shape), passes)
            y[v] = x[v] + ((S - 1 - s) * fraction * lk.SCALE[v][1] / f.std()) * f
        xs.append(y)
    return xs + [x]


def push_out(g, xs, obs, first, slot, member):
    """Lowers xs[slot]'s ps of `member` at the four points of one at-pressure observation of the slot, so far in column for every
    member at every time, until the observation lies below that member's lowest level at the slot's time only -> (the ensembles
    with xs[slot] replaced, the observation).  The one with the largest target is taken: the smallest push"""
    first = lk.slot_rows(first, len(obs["var"]))
    idx, _ = lk.stencil(g, obs["lon"], obs["lat"])
    inside = np.ones(len(obs["var"]), bool)
    for x in xs:
        inside &= lk.obs_space(g, x, obs)["obs_used"] == 1.0
    xo = lp.lnp(obs)
    rows = np.arange(first[slot], first[slot + 1])
    rows = rows[lp.at_pressure(obs)[rows] & inside[rows]]
    assert len(rows), "no at-pressure observation of slot %d is in every member's column" % slot
    o = int(rows[np.argmax(xo[rows])])
    y = {v: a.copy() for v, a in xs[slot].items()}
    y["ps"].reshape(y["ps"].shape[0], -1)[member, idx[o]] = xo[o] - g.lnf[-1] - 0.02      # X_{kx-1} = x_o - 0.02 < x_o
    return xs[:slot] + [y] + xs[slot + 1:], o


# ------------------------------------------------------------------------------------------------ what the GPU tests share
def observe_all(lt, xs, first):
    """set_slots(first), then every slot observed on its ensemble (NumPy, or a list of five device tensors)"""
    lt.set_slots(first)
    for s, x in enumerate(xs):
        lt.observe_grid(s, *(lk.grids(x) if isinstance(x, dict) else x))


# ------------------------------------------------------------------------------------------------ every feature at once
EVERYTHING = {"E": 8, "drop": 5, "sigma_v": 0.1, "stride": (2, 2), "relaxation": (0.3, 0.9), "gross": 3.0, "sigma_b": 0.5,
              "patches": (1.0, 1.1, 1.45)}


def everything_inputs(g, S=3, first_of=lambda n: [0, 300, 700, n], seed=71):
    """One analysis with every feature on (EVERYTHING): E = 8 without member 5; tests/letkfpressure.py's crafted ensemble and, from
    the members in use, its network with observations at a pressure, in S slots on ensembles that drift to the analysed one; values
    planted on both sides of the background check's threshold (tests/letkfqc.py's plant, from the restatement's own hxmean and
    spread); an inflation field of three values in patches -> a dict: x, xs, obs, first, keep, field (kx, ncol), outside, inside"""
    import letkfqc as qc
    c = EVERYTHING
    keep = tuple(e for e in range(c["E"]) if e != c["drop"])
    x = lp.craft(g, c["E"], seed)
    xs = drifting(g, x, S, seed + 1, passes=2)
    obs = lp.network(g, lk.compact(x, keep))
    first = first_of(len(obs["var"]))
    space = lk.obs_space(g, x, obs, keep, xs=xs, first=first)
    obs["value"], outside, inside = qc.plant(obs, space["hxmean"], qc.spread2(space["y"], keep), c["gross"], seed)
    which = (np.arange(g.ix * g.il)[None, :] // 700 + np.arange(g.kx)[:, None]) % 3
    return {"x": x, "xs": xs, "obs": obs, "first": first, "keep": keep, "field": np.array(c["patches"])[which], "outside": outside,
            "inside": inside}


def everything_object(sp, case):
    """the analysis object of `everything_inputs` with every setting made and the inflation field uploaded"""
    c = EVERYTHING
    lt = lp.make(sp, c["E"], case["obs"], c["sigma_v"])
    lt.set_weight_stride(*c["stride"])
    lt.set_relaxation(*c["relaxation"])
    lt.set_background_check(c["gross"])
    lt.set_adaptive_inflation(c["sigma_b"])
    lt.inflation_field().upload(case["field"].reshape((sp.kx,) + sp.grid_shape))
    return lt
