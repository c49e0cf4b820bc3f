"""Weight interpolation of the ensemble analysis restated in NumPy (include/spdy.h, "ensemble analysis", weight interpolation): the
coarse set of a stride, every grid column's stencil in it, the interpolated transform and the increments.  The local problems and
their two eigen routes are those of tests/letkf.py, solved at the coarse columns a comparison needs.  Also the grid columns the
tests compare at, one pair per stencil class (class_columns)."""
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


CENTRE, POLAR = (100.0, 20.0), (357.0, 83.0)      # of the tests' clusters: mid-latitude; in range of the last row and of the cell that wraps


def class_columns(g, si, sj):
    """{stencil class: grid columns}: of every class the column nearest to CENTRE, of the last three the one nearest to POLAR, and of
    the first four also the one farthest from both.  At a stride whose only coarse rows are 0 and il-1 there is no column on a
    coarse row only other than those of the last two classes, and the one latitude interval is the last one"""
    rows = coarse_rows(g, sj)
    jj, ii = np.divmod(np.arange(g.ix * g.il), g.ix)
    crow, clon = np.isin(jj, rows), ii % si == 0
    inner = (jj > 0) & (jj < (rows[-2] if len(rows) > 2 else g.il - 1))
    classes = {"interior": ~crow & ~clon & inner & (ii < g.ix - si), "coarse longitude": ~crow & clon & inner,
               "coarse row": crow & ~clon & inner, "wrap": ~clon & (ii > g.ix - si) & (jj > 0) & (jj < g.il - 1),
               "last interval": (jj >= rows[-2]) & (jj < g.il - 1) & (~crow if rows[-1] - rows[-2] > 1 else crow) & ~clon,
               "j = 0": (jj == 0) & ~clon, "j = il-1": (jj == g.il - 1) & ~clon}
    dc, dp = (lk.distance(g.colunit, lk.unit([p[0]], [p[1]]))[:, 0] for p in (CENTRE, POLAR))
    out = {}
    for n, (name, mask) in enumerate(classes.items()):
        cand = np.nonzero(mask)[0]
        if name == "coarse row" and len(rows) == 2:
            continue
        assert len(cand), name
        out[name] = np.array([cand[dc[cand].argmin()], cand[dp[cand].argmin()] if n >= 4 else cand[np.minimum(dc, dp)[cand].argmax()]])
    return out


def needed(idx, wgt, cols):
    """the entries of the coarse list that the stencils of the grid columns `cols` read, ascending"""
    return np.unique(idx[cols][wgt[cols] != 0.0])


SLAB = 512           # grid columns `transforms` forms the local problems of at a time: their weights are (columns, kx, nobs)


def transforms(g, x, obs, sigma_h, sigma_v, rho, gridcols, route="eigh", **how):
    """T (n, kx, E, E) of the local problems at the grid columns `gridcols`.  rho: the scalar, or the field (kx, ncol) of adaptive
    inflation.  how: what tests/letkf.py's analyse takes for a feature -- keep (E is then the members in use), stencil, r_eff, xs and
    first"""
    gridcols = np.asarray(gridcols)
    keep, r_eff = how.get("keep"), how.get("r_eff")
    space = lk.obs_space(g, x, obs, keep, how.get("stencil"), how.get("xs"), how.get("first"))
    out = []
    for i in range(0, len(gridcols), SLAB):
        at = gridcols[i:i + SLAB]
        C, b = lk.problems(g, obs, space, sigma_h, sigma_v, at, keep, r_eff)
        n, kx, E = b.shape
        r = rho if np.ndim(rho) == 0 else np.asarray(rho, np.float64).reshape(kx, -1)[:, at].T.reshape(-1)
        out.append(lk.transform(C.reshape(-1, E, E), b.reshape(-1, E), E, r, route)[0].reshape(n, kx, E, E))
    return np.concatenate(out)


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


def analyse(g, x, obs, sigma_h, sigma_v, rho, si, sj, route="eigh", cols=None, tables=None, **how):
    """The increments of the gridded ensemble x at the grid columns `cols` (default: all) at weight stride (si, sj); also the
    coarse-list entries that were solved and their transforms.  how: `transforms`'; with keep the increments are those of the members
    in use, in their order"""
    cols = np.arange(g.ix * g.il) if cols is None else np.asarray(cols)
    idx, wgt = tables if tables is not None else stencils(g, si, sj)
    entries = needed(idx, wgt, cols)
    Tc = transforms(g, x, obs, sigma_h, sigma_v, rho, coarse_columns(g, si, sj)[entries], route, **how)
    return increments(g, lk.compact(x, how.get("keep")), interpolate(Tc, entries, idx, wgt, cols), cols), entries, Tc
