"""The relaxation of the analysis restated in NumPy (include/spdy.h, "relaxation"), and what its two test files
share.  `relax` follows the header line by line; its four sums are explicit loops over the members in ascending order, because
np.sum adds pairwise and would differ from the definition by E eps |x|.

Arrays have the member axis first: a gridded ensemble and its increments are the dicts of tests/letkf.py, or those at a list of
columns ({"u" .. "q": (E, kx, ncols), "ps": (E, ncols)}, what letkf.increments gives)."""
import numpy as np

import letkf as lk
import support

EPS = lk.EPS
SETTINGS = ((0.5, 0.0), (0.0, 0.9), (0.3, 0.9))     # (rtpp, rtps) of the comparisons with the kernel


def relax_array(x, dx, rtpp, rtps, keep=None):
    """x, dx (E, ...) -> (dx' (E, ...), f (...)); keep: the members in use, default all.  Both values 0: the relaxation is not
    applied, dx comes back with its bits.  A member not in use gets 0.0 and is not read; fewer than two in use: all zero, f = 1."""
    E = x.shape[0]
    keep = list(range(E)) if keep is None else sorted(keep)
    n = len(keep)
    if rtpp == 0.0 and rtps == 0.0:
        return dx.copy(), np.ones(x.shape[1:])
    out, one = np.zeros_like(dx), np.ones(x.shape[1:])
    if n < 2:
        return out, one
    sx, sd = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for e in keep:
        sx = sx + x[e]
        sd = sd + dx[e]
    xm, dm = sx / n, sd / n
    omr = 1.0 - rtpp
    b, a = {}, {}
    sb2, sa2 = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for e in keep:
        b[e] = x[e] - xm
        a[e] = b[e] + omr * (dx[e] - dm)
        sb2 = sb2 + b[e] * b[e]
        sa2 = sa2 + a[e] * a[e]
    sb, sa = np.sqrt(sb2 / (n - 1)), np.sqrt(sa2 / (n - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(sa > 0.0, 1.0 + (rtps * (sb - sa)) / sa, 1.0)
    for e in keep:
        out[e] = dm + (f * a[e] - b[e])
    return out, f


def relax(x, dx, rtpp, rtps, keep=None):
    """the dicts' form of relax_array -> (dx', f), both dicts over letkf.VARS"""
    out, f = {}, {}
    for v in lk.VARS:
        out[v], f[v] = relax_array(x[v], dx[v], rtpp, rtps, keep)
    return out, f


def spread(x, keep=None):
    """sb of the definition, per item"""
    E = x.shape[0]
    keep = list(range(E)) if keep is None else sorted(keep)
    s = np.zeros(x.shape[1:])
    for e in keep:
        s = s + x[e]
    xm, s2 = s / len(keep), np.zeros(x.shape[1:])
    for e in keep:
        s2 = s2 + (x[e] - xm) * (x[e] - xm)
    return np.sqrt(s2 / (len(keep) - 1))


def items(f):
    """a dict of per-item fields ({"u" .. "q": (kx, ...), "ps": (...)}) in the order of the "inflation" field: (4 kx + 1, ...)"""
    return np.concatenate([f[v] for v in lk.VARS[:4]] + [f["ps"][None]])


def limit(x, f, E, v):
    """the bound on |kernel - restatement| of an item's increments: 64 E eps max|x| max(1, f), max|x| of the variable"""
    return 64 * E * EPS * float(np.max(np.abs(x[v]))) * np.maximum(1.0, f[v])


def at_columns(x, cols):
    """a gridded dict at grid columns, in the shape letkf.increments gives"""
    return {v: lk.at_columns(x[v], cols) for v in lk.VARS}


def same_bits_everywhere(a):
    """every member of a (E, ...) has the bits of member 0"""
    return all(support.same_bits(a[e], a[0]) for e in range(1, a.shape[0]))


# ------------------------------------------------------------------------------------------------ what the GPU tests share
def raw_and_relaxed(lt, x, rtpp, rtps, use=None):
    """the raw increments of the object at (0, 0) and its relaxed call at (rtpp, rtps) -> (raw, relaxed, inflation)"""
    lt.set_relaxation(0.0, 0.0)
    raw = lk.run(lt, x, use, names=())
    lt.set_relaxation(rtpp, rtps)
    got = lk.run(lt, x, use, names=())
    return raw, got, got["inflation"]


def compare(x, raw, got, infl, rtpp, rtps, E, keep=None):
    """the relaxed call against `relax` of the raw increments at every column -> the largest ratio to the limit; the inflation
    field against the restatement's f, relative, at 64 E eps (asserted)"""
    ref, f = relax(x, raw, rtpp, rtps, keep)
    worst = 0.0
    for v in lk.VARS:
        assert np.isfinite(got[v]).all() and np.isfinite(ref[v]).all(), v
        worst = max(worst, float(np.max(np.abs(got[v] - ref[v]) / limit(x, f, E, v)[None])))
    fi = items(f)
    assert infl.shape == fi.shape, (infl.shape, fi.shape)
    assert float(np.max(np.abs(infl - fi) / fi)) <= 64 * E * EPS, float(np.max(np.abs(infl - fi) / fi))
    return worst, float(fi.max())
