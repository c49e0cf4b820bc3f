"""Weight interpolation of the ensemble analysis restated in NumPy (include/spdy.h, "ensemble analysis", weight interpolation): the
coarse set of a stride, every grid column's stencil in it, the interpolated transform and the increments.  The local problems and
their two eigen routes are those of tests/letkf.py, solved at the coarse columns a comparison needs."""
import numpy as np

import letkf as lk


def coarse_rows(g, sj):
    """0, sj, 2 sj, ... together with il-1"""
    return np.unique(np.append(np.arange(0, g.il, sj), g.il - 1))


def coarse_columns(g, si, sj):
    """the grid columns j*ix+i with i and j both coarse, ascending"""
    return (coarse_rows(g, sj)[:, None] * g.ix + np.arange(0, g.ix, si)[None, :]).ravel()


def stencils(g, si, sj):
    """-> (index (ncol, 4) into coarse_columns, weight (ncol, 4)): (j0,i0) (j0,i1) (j1,i0) (j1,i1); an entry of weight zero repeats
    the first index"""
    rows = coarse_rows(g, sj)
    ni = g.ix // si
    idx, wgt = np.zeros((g.il * g.ix, 4), np.int64), np.zeros((g.il * g.ix, 4))
    for j in range(g.il):
        r0 = int(np.searchsorted(rows, j, side="right")) - 1
        r1 = r0 if j == g.il - 1 else r0 + 1
        j0, j1 = int(rows[r0]), int(rows[r1])
        b = 0.0 if j1 == j0 else (j - j0) / (j1 - j0)
        for i in range(g.ix):
            i0 = (i // si) * si
            i1 = (i0 + si) % g.ix
            a = (i - i0) / si
            e = (r0 * ni + i0 // si, r0 * ni + i1 // si, r1 * ni + i0 // si, r1 * ni + i1 // si)
            w = ((1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b)
            wgt[j * g.ix + i] = w
            idx[j * g.ix + i] = [e[n] if w[n] != 0.0 else e[0] for n in range(4)]
    return idx, wgt


def needed(idx, wgt, cols):
    """the entries of the coarse list that the stencils of the grid columns `cols` read, ascending"""
    return np.unique(idx[cols][wgt[cols] != 0.0])


def transforms(g, x, obs, sigma_h, sigma_v, rho, gridcols, route="eigh"):
    """T (n, kx, E, E) of the local problems at the grid columns `gridcols`"""
    C, b = lk.problems(g, obs, lk.obs_space(g, x, obs), sigma_h, sigma_v, gridcols)
    n, kx, E = b.shape
    return lk.transform(C.reshape(-1, E, E), b.reshape(-1, E), E, rho, route)[0].reshape(n, kx, E, E)


def interpolate(Tc, entries, idx, wgt, cols):
    """T (ncols, kx, E, E) at the grid columns `cols` from Tc, the transforms of the coarse-list entries `entries` (ascending):
    ((w0 T0 + w1 T1) + w2 T2) + w3 T3; a term of weight zero is neither read nor added, the first term present starts the sum"""
    cols = np.asarray(cols)
    out = np.zeros((len(cols),) + Tc.shape[1:])
    have = np.zeros(len(cols), bool)
    for n in range(4):
        w = wgt[cols, n]
        m = np.nonzero(w != 0.0)[0]
        at = np.searchsorted(entries, idx[cols[m], n])
        assert np.array_equal(np.asarray(entries)[at], idx[cols[m], n])
        term = w[m, None, None, None] * Tc[at]
        out[m] = np.where(have[m, None, None, None], out[m] + term, term)
        have[m] = True
    assert have.all()
    return out


def increments(g, x, Tm, cols):
    """step 4 of the analysis on given transforms Tm (ncols, kx, E, E) -> {"u" .. "q": (E, kx, ncols), "ps": (E, ncols)}"""
    cols = np.asarray(cols)
    E, kx = x["ps"].shape[0], g.kx
    out = {}
    for v in lk.VARS:
        f = x[v].reshape(E, -1, g.il * g.ix)[:, :, cols]
        s = np.zeros(f.shape[1:])
        for e in range(E):
            s = s + f[e]
        xp = f - (s / E)[None]
        out[v] = np.einsum("fkc,ckfe->ekc", xp, Tm if v != "ps" else Tm[:, kx - 1:kx])
    out["ps"] = out["ps"][:, 0]
    return out


def analyse(g, x, obs, sigma_h, sigma_v, rho, si, sj, route="eigh", cols=None, tables=None):
    """The increments of the gridded ensemble x at the grid columns `cols` (default: all) at weight stride (si, sj); also the
    coarse-list entries that were solved and their transforms"""
    cols = np.arange(g.ix * g.il) if cols is None else np.asarray(cols)
    idx, wgt = tables if tables is not None else stencils(g, si, sj)
    entries = needed(idx, wgt, cols)
    Tc = transforms(g, x, obs, sigma_h, sigma_v, rho, coarse_columns(g, si, sj)[entries], route)
    return increments(g, x, interpolate(Tc, entries, idx, wgt, cols), cols), entries, Tc
