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
