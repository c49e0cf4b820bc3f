"""The reference side of the pressure-level output tests (include/spdy.h, "pressure-level output"): the definition restated in NumPy
in the same operation order -- the coordinate of the model levels, the bracket and the weight by np.interp's rule, y = x[k] + w *
(x[k+1] - x[k]) with every operation rounded once in FP64, and the statistics as sequential FP64 sums in ascending member order,
two passes.  The logarithms of the log-p coordinate are math.log's, the C library's the host code calls; NumPy's exp is the one
operation that may differ from the device's, by an ulp of FP64.  Also: crafted gridded ensembles that hold every class of target
(clamped above and below, every bracket, a target exactly on a level, members of one column in different brackets, every kind of
`below` count), the classes a set of inputs holds, and the reference's own route in float32 (scripts/sigma_to_pressure.py)."""
import math

import numpy as np

from ensembleoutput import GRAV, P0, QFAC

QUANTITIES = ("u", "v", "t", "q", "phi")
COORDS = ("p", "logp")
SCRIPT_LEVELS = (2500.0, 10000.0, 20000.0, 30000.0, 50000.0, 70000.0, 85000.0, 95000.0)   # the reference script's p_levels, in Pa
SIGMA_L2 = (0.0, 0.5, 1.0)                                      # half levels of a two-level set: fsg = 0.25, 0.75


def slope_factor(fsg):
    """A = max_k fsg[k+1] / (fsg[k+1] - fsg[k]): how much a relative error of the surface pressure moves a weight (1 at kx = 1)"""
    fsg = np.asarray(fsg, np.float64)
    return float(np.max(fsg[1:] / np.diff(fsg))) if len(fsg) > 1 else 1.0


def values(raw):
    """the FP64 values x_e of the model's raw grids (q in g/kg, phi in m2/s2): u, v, t as they are, q * 1.0e-3, phi / grav"""
    return {"u": raw["u"], "v": raw["v"], "t": raw["t"], "q": raw["q"] * QFAC, "phi": raw["phi"] / GRAV}


def coordinates(fsg, ps, plev, coord):
    """X (E, kx, ...) of the model levels for the raw surface pressures ps (E, ...) = log(p/p0), and the targets x (nlev)"""
    fsg, plev = [float(f) for f in fsg], [float(p) for p in plev]
    with np.errstate(all="ignore"):
        if coord == "p":
            P = P0 * np.exp(ps)
            return np.stack([P * f for f in fsg], axis=1), np.array(plev)
        return np.stack([ps + math.log(f) for f in fsg], axis=1), np.array([math.log(p / P0) for p in plev])


def brackets(X, x):
    """np.interp's rule for one target x in the columns X (E, kx, ...): kb (the bracket's first level, 0 .. kx-2), lo (x <= X_0: level
    0's value), hi (x >= X_{kx-1}: level kx-1's), below (x > X_{kx-1}) and w = (x - X_kb) / (X_{kb+1} - X_kb)"""
    kx = X.shape[1]
    with np.errstate(all="ignore"):
        kb = np.sum(X[:, 1:kx - 1] <= x, axis=1) if kx > 2 else np.zeros(X[:, 0].shape, np.int64)
        k1 = np.minimum(kb + 1, kx - 1)
        at = lambda k: np.take_along_axis(X, k[:, None], axis=1)[:, 0]
        xlo, xhi = at(kb), at(k1)
        lo = np.full(kb.shape, True) if kx == 1 else x <= X[:, 0]
        return kb, k1, lo, x >= X[:, kx - 1], x > X[:, kx - 1], (x - xlo) / (xhi - xlo)


def interpolate(fsg, xe, ps, plev, coord):
    """-> (y, cls): y[n] (E, nlev, ...) the members' values of quantity n on the levels; cls the per-level (kb, lo, hi, below, w), each
    (E, nlev, ...).  xe: {quantity: (E, kx, ...)} in FP64, ps (E, ...) raw.  A member whose ps is not finite gets NaN."""
    X, xt = coordinates(fsg, ps, plev, coord)
    per = [brackets(X, x) for x in xt]
    y = {}
    with np.errstate(all="ignore"):
        for n, f in xe.items():
            out = []
            for kb, k1, lo, hi, _, w in per:
                f0 = np.take_along_axis(f, kb[:, None], axis=1)[:, 0]
                f1 = np.take_along_axis(f, k1[:, None], axis=1)[:, 0]
                d = f1 - f0
                v = f0 + w * d
                out.append(np.where(np.isfinite(ps), np.where(lo, f0, np.where(hi, f1, v)), np.nan))
            y[n] = np.stack(out, axis=1)
    names = ("kb", "lo", "hi", "below", "w")
    cls = {m: np.stack([p[i] for p in per], axis=1) for m, i in zip(names, (0, 2, 3, 4, 5))}
    return y, cls


def statistics(y, use=None):
    """mean and spread of y (E, ...) over the members in use as the kernel forms them: sequential FP64 sums in ascending member
    order, the squared deviations from the finished mean in a second pass; n = 1: spread +0, n = 0: NaN"""
    members = [e for e in range(y.shape[0]) if use is None or use[e]]
    n = len(members)
    if n == 0:
        return np.full(y.shape[1:], np.nan), np.full(y.shape[1:], np.nan)
    with np.errstate(all="ignore"):
        s = np.zeros(y.shape[1:])
        for e in members:
            s = s + y[e]
        mean = s / float(n)
        q = np.zeros(y.shape[1:])
        for e in members:
            d = y[e] - mean
            q = q + d * d
        return mean, (np.sqrt(q / float(n - 1)) if n > 1 else np.zeros(y.shape[1:]))


def restate(fsg, xe, ps, plev, coord, use=None):
    """the whole product in FP64: {"members", "mean", "spread": {u .. phi, ps}, "below": counts, "cls": interpolate's classes}"""
    y, cls = interpolate(fsg, xe, ps, plev, coord)
    with np.errstate(all="ignore"):
        y["ps"] = P0 * np.exp(ps)
    res = {"members": y, "mean": {}, "spread": {}, "cls": cls}
    for n, a in y.items():
        res["mean"][n], res["spread"][n] = statistics(a, use)
    inc = [e for e in range(ps.shape[0]) if use is None or use[e]]
    res["below"] = cls["below"][inc].sum(axis=0).astype(np.float64) if inc else np.zeros(cls["below"].shape[1:])
    return res


def ulp_excess(dev, ref, extra=0.0):
    """|device - float32(ref)| - (one float32 ulp of the reference value + extra), its largest value in units of that bound: <= 0
    is met (NaN where the reference is NaN counts as met, anywhere else as missed).  Also returns the largest ratio error / bound."""
    r32 = np.asarray(ref).astype(np.float32)
    bound = np.spacing(np.abs(r32)).astype(np.float64) + extra
    err = np.abs(dev.astype(np.float64) - r32.astype(np.float64))
    both_nan = np.isnan(dev) & np.isnan(r32)
    ratio = np.where(both_nan, 0.0, np.where(np.isnan(err), np.inf, err / bound))
    return float(np.max(ratio))


# ------------------------------------------------------------------------------------------------ crafted gridded ensembles
def levels(fsg, nlev):
    """nlev targets in Pa, unsorted: first one exactly on a model level of a column with ps = 0, then one below the lowest level of
    some members only, one above every top, one below every bottom, then the other model levels and values in between"""
    kx = len(fsg)
    on = [P0 * float(fsg[k]) for k in ([1, 2, 3, 5, 6, 4, 0, 7] if kx == 8 else [1, 2, 3, 4, 0] if kx == 5 else list(range(kx))[::-1])]
    pool = on[:1] + [90000.0, 1000.0, 104000.0] + on[1:] + [40000.0, 20000.0, 60000.0, 52000.0, 97000.0, 8000.0, 30000.0]
    assert len(pool) >= nlev
    return pool[:nlev]


def craft(ix, il, kx, E, seed):
    """A gridded ensemble of E members in the model's raw units: {u, v, t, q, phi (E, kx, il, ix), ps (E, il, ix)}.  ps is random
    between ln 0.5 and ln 1.05, independently per member and point, and exactly 0 for every member in the first four rows; v is
    constant in the vertical."""
    r = np.random.default_rng(seed)
    shape = (E, kx, il, ix)
    raw = {"u": 10.0 * r.standard_normal(shape), "v": np.repeat(8.0 * r.standard_normal((E, 1, il, ix)), kx, axis=1),
           "t": 250.0 + 30.0 * r.standard_normal(shape), "q": 5.0 * np.abs(r.standard_normal(shape)),
           "phi": 1.0e4 * r.standard_normal(shape), "ps": r.uniform(math.log(0.5), math.log(1.05), (E, il, ix))}
    raw["ps"][:, :4] = 0.0
    return raw


def stack(raw):
    """a crafted ensemble as the device array of spdy_ens_output_pressure_grid_dev: u | v | t | q | phi | ps, flat FP64"""
    return np.concatenate([np.ascontiguousarray(raw[n], np.float64).ravel() for n in QUANTITIES + ("ps",)])


def classes(cls, n):
    """the classes of target a set of inputs holds (cls of interpolate, n members, all in use) -> a set of names"""
    kb, lo, hi, below, w = (cls[m] for m in ("kb", "lo", "hi", "below", "w"))
    inside = ~lo & ~hi
    found = {"bracket%d" % k for k in np.unique(kb[inside])}
    if (lo & ~hi).any():
        found.add("above_top")
    if below.any():
        found.add("below_bottom")
    if (inside & (w == 0.0)).any():
        found.add("on_level")
    if (inside.all(axis=0) & (kb.min(axis=0) != kb.max(axis=0))).any():
        found.add("brackets_differ")
    count = below.sum(axis=0)
    found |= {name for name, hit in (("below0", count == 0), ("below_some", (count > 0) & (count < n)), ("below_all", count == n))
              if hit.any()}
    return found


def every_class(kx, n):
    """what classes() must return for a full set of inputs: n >= 2 members, all in use.  (kx = 2 has one bracket, and a target on
    either of its levels is a clamped one: no target strictly inside lies on a level, no two members differ in their bracket)"""
    inner = {"on_level", "brackets_differ"} if kx > 2 else set()
    return {"bracket%d" % k for k in range(kx - 1)} | {"above_top", "below_bottom", "below0", "below_some", "below_all"} | inner


# ------------------------------------------------------------------------------------------------ the reference's route
def script_route(f32, ps32, sigma32, plev):
    """scripts/sigma_to_pressure.py on a float32 snapshot: per column np.interp(p_hpa, (ps32 / 100.0) * sigma32, f32), in the script's
    arithmetic -- float32 coordinates, np.interp's FP64 inside, the result stored as float32.  f32 (kx, il, ix), ps32 (il, ix)"""
    p_hpa = (np.asarray(plev, np.float64) / 100.0).astype(np.float32)
    X = (ps32 / np.float32(100.0)) * np.asarray(sigma32, np.float32)[:, None, None]
    assert X.dtype == np.float32
    out = np.empty((len(p_hpa),) + f32.shape[1:], np.float32)
    for j in range(f32.shape[1]):
        for i in range(f32.shape[2]):
            out[:, j, i] = np.interp(p_hpa, X[:, j, i], f32[:, j, i])
    return out
