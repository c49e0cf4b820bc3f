"""The ensemble analysis restated in NumPy (include/spdy.h, "ensemble analysis" and the sections after it), exactly as the header
defines it, ONCE, as stages that feed each other and take the optional arguments the features need:

    observe    what is per member: hx, and for a network with observations at a pressure the members' ps and out-of-column flags
               (stencil: the library's own tables for bit comparisons)
    couple     what couples members, summed over the members in use in ascending order -> the obs_space dict (keep: the member mask)
    weights    the localisation weight of unit vectors and ln sigma_o at grid columns
    problems   C and b of the local problems from an obs_space dict (keep; r_eff: the background check's 1 / error^2)
    increments the transform and the increments, with two routes for the eigenproblem -- numpy.linalg.eigh and a cyclic Jacobi of
               its own -- whose difference measures what rounding alone does on given inputs

obs_space is couple(observe(...)), row range by row range on the slots' ensembles when xs and first are given; analyse is
increments(problems(obs_space(...))).  `run` is the device side of a comparison: Letkf.analyse_grid on a NumPy ensemble and what
the object holds afterwards.  The modules tests/letkf*.py next to this one keep what is a feature's own (the vertical
interpolation, the check's decisions and statistics, the relaxation, the inflation estimate, the interpolation tables).  Also the
helpers that build small observation sets and gridded ensembles for the tests.

Arrays are C-order views of the library's: a gridded ensemble is {"u", "v", "t", "q": (E, kx, il, ix), "ps": (E, il, ix)}; an
observation set is a dict of equal-length arrays var, lev, lon, lat, value, error, and "p" in Pa where the network may hold
observations at a pressure (lev == AT_P)."""
import numpy as np

import support

U, V, T, Q, PS = range(5)
AT_P = -1            # as lev: the observation sits at its pressure "p" (tests/letkfpressure.py)
FIELDS = ("hx", "hxmean", "y", "departure", "obs_lnsigma", "obs_used")      # of an obs_space dict, and the device fields of those names
VARS = ("u", "v", "t", "q", "ps")
REARTH = 6.371e6
EPS = float(np.finfo(np.float64).eps)
CHUNK = 256          # LETKF_CHUNK of csrc/spdy_letkf.hip: observations the transform kernel scans per step


class Geometry:
    """what the definition reads from a plan: the grid and the levels (a host-only plan serves)"""

    def __init__(self, sp):
        self.ix, self.il, self.kx = sp.ix, sp.il, sp.kx
        s = sp.table("sia_half")
        self.lat = np.concatenate([-np.degrees(np.arcsin(s)), np.degrees(np.arcsin(s))[::-1]])       # south first
        self.lon = np.arange(self.ix) * (360.0 / self.ix)
        self.lnfsg = np.log(sp.table("fsg"))
        lo, la = np.meshgrid(self.lon, self.lat)
        self.colunit = unit(lo.ravel(), la.ravel())                                                 # (ncol, 3), column j*ix+i


def unit(lon, lat):
    rl, rp = np.radians(np.asarray(lon, np.float64)), np.radians(np.asarray(lat, np.float64))
    return np.stack([np.cos(rp) * np.cos(rl), np.cos(rp) * np.sin(rl), np.sin(rp)], axis=-1)


def make_obs(var, lev, lon, lat, value, error):
    n = len(var)
    return {"var": np.asarray(var, np.int64).reshape(n), "lev": np.asarray(lev, np.int64).reshape(n),
            "lon": np.asarray(lon, np.float64).reshape(n), "lat": np.asarray(lat, np.float64).reshape(n),
            "value": np.asarray(value, np.float64).reshape(n), "error": np.asarray(error, np.float64).reshape(n)}


def concat(*sets):
    return {k: np.concatenate([s[k] for s in sets]) for k in sets[0]}


def args(obs):
    """the arguments of Letkf.set_obs"""
    return [obs[k] for k in ("var", "lev", "lon", "lat", "value", "error")]


def stencil(g, lon, lat):
    """-> (index (nobs, 4) of grid points j*ix+i, weight (nobs, 4)): (j0,i0) (j0,i1) (j1,i0) (j1,i1)"""
    idx, wgt = np.zeros((len(lon), 4), np.int64), np.zeros((len(lon), 4))
    for o, (lo, la) in enumerate(zip(lon, lat)):
        x = np.fmod(lo, 360.0)
        if x < 0.0:
            x += 360.0
        x = x / (360.0 / g.ix)
        i0 = int(np.floor(x))
        a = x - i0
        if i0 >= g.ix:
            i0, a = 0, 0.0
        i1 = (i0 + 1) % g.ix
        if la <= g.lat[0]:
            j0, j1, b = 0, 0, 0.0
        elif la >= g.lat[-1]:
            j0, j1, b = g.il - 1, g.il - 1, 0.0
        else:
            j0 = min(int(np.searchsorted(g.lat, la, side="right")) - 1, g.il - 2)
            j1 = j0 + 1
            b = (la - g.lat[j0]) / (g.lat[j1] - g.lat[j0])
        idx[o] = (j0 * g.ix + i0, j0 * g.ix + i1, j1 * g.ix + i0, j1 * g.ix + i1)
        wgt[o] = ((1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b)
    return idx, wgt


def dense_rows(g, idx, wgt):
    """the stencils as rows of H over the grid: equal points of a stencil add up"""
    H = np.zeros((idx.shape[0], g.ix * g.il))
    for o in range(idx.shape[0]):
        np.add.at(H[o], idx[o], wgt[o])
    return H


_grid_stencil = stencil      # `observe` takes the stencils to use under this name


def subset(obs, keep):
    """the network with the observations keep (a mask, a slice or indices) only, in their order"""
    return {k: v[keep] for k, v in obs.items()}


def members(E, keep=None):
    """the members in use, ascending (default: all)"""
    return list(range(E)) if keep is None else sorted(int(e) for e in keep)


def compact(x, keep):
    """the gridded ensemble of the members in use"""
    return x if keep is None else {v: np.ascontiguousarray(x[v][members(0, keep)]) for v in VARS}


def at_pressure(obs):
    """which observations sit at their pressure "p" (tests/letkfpressure.py); none of a set without "p" """
    return (obs["lev"] == AT_P) & (obs["var"] != PS) if "p" in obs else np.zeros(len(obs["var"]), bool)


def bilinear(w, z):
    """w (4) and z (E, 4) -> (E)"""
    return ((w[0] * z[:, 0] + w[1] * z[:, 1]) + w[2] * z[:, 2]) + w[3] * z[:, 3]


def observe(g, x, obs, stencil=None, pressure=None):
    """What is per member -> (hx (nobs, E), ps (nobs, E), out (nobs, E)).  A model-level or ps observation is the bilinear sum of its
    four points; one at a pressure that of tests/letkfpressure.py's per-column interpolation.  ps, the members' ps at the station,
    and out, 1.0 where the observation is out of the member's column at one of the points, are None unless the network has an
    observation at a pressure (pressure: whether it has, for a part of a network; default: whether obs has).  stencil: (index, weight)
    to use in the place of `stencil`'s (Letkf.table's: bit comparisons against the device)"""
    idx, w = _grid_stencil(g, obs["lon"], obs["lat"]) if stencil is None else stencil
    E, n = x["ps"].shape[0], len(obs["var"])
    atp = at_pressure(obs)
    hx, ps, out = np.zeros((n, E)), None, None
    if atp.any() if pressure is None else pressure:
        import letkfpressure as lp               # it imports this module
        xo, ps, out = lp.lnp(obs), np.zeros((n, E)), np.zeros((n, E))
    for o in range(n):
        v = int(obs["var"][o])
        if ps is not None:
            ps[o] = bilinear(w[o], x["ps"].reshape(E, -1)[:, idx[o]])
        if atp[o]:
            _, X, f = lp.stencil_columns(g, x, obs, o, idx)
            z, _, _, _, far = lp.column_values(X, f, xo[o])
            out[o] = far.any(axis=1)
        else:
            z = x[VARS[v]].reshape(E, -1, g.il * g.ix)[:, 0 if v == PS else int(obs["lev"][o])][:, idx[o]]
        hx[o] = bilinear(w[o], z)
    return hx, ps, out


def couple(g, obs, hx, ps=None, out=None, keep=None):
    """Everything that couples members, the sums over the members `keep` (default: all) in ascending order -> {"hx", "hxmean", "y"
    (0.0 for a member not in use), "departure", "obs_lnsigma" (for an observation at a pressure ln(p/p0) minus the mean of ps),
    "obs_used" (0.0 for one out of the column of a member in use)}, and ps and out as "slot_ps" and "slot_out" when given"""
    use = members(hx.shape[1], keep)
    n, nobs = len(use), hx.shape[0]
    s = np.zeros(nobs)
    for e in use:
        s = s + hx[:, e]
    with np.errstate(all="ignore"):
        hxmean = s / n if n else np.full(nobs, np.nan)
        y = np.zeros_like(hx)
        y[:, use] = hx[:, use] - hxmean[:, None]
    atp = at_pressure(obs)
    lns, used = lnsigma(g, dict(obs, lev=np.where(atp, 0, obs["lev"]))), np.ones(nobs)
    if atp.any():
        import letkfpressure as lp
        p = np.zeros(nobs)
        for e in use:
            p = p + ps[:, e]
        with np.errstate(all="ignore"):
            lns = np.where(atp, lp.lnp(obs) - p / n, lns) if n else np.where(atp, np.nan, lns)
        used = np.where((out[:, use] != 0.0).any(axis=1), 0.0, 1.0)
    s = {"hx": hx, "hxmean": hxmean, "y": y, "departure": obs["value"] - hxmean, "obs_lnsigma": lns, "obs_used": used}
    return s if ps is None else dict(s, slot_ps=ps, slot_out=out)


def slot_rows(first, nobs):
    """the slots' ranges checked: S + 1 integers from 0 to nobs that do not decrease"""
    first = [int(f) for f in first]
    assert len(first) >= 2 and first[0] == 0 and first[-1] == nobs and all(a <= b for a, b in zip(first, first[1:])), (first, nobs)
    return first


def obs_space(g, x, obs, keep=None, stencil=None, xs=None, first=None):
    """`couple` of `observe`: the observation-space quantities of one analysis call.  xs, first (tests/letkfslots.py): the rows
    first[s] <= o < first[s+1] are observed on xs[s] in x's place, and ps and out are kept for every network, zero for one without
    an observation at a pressure"""
    if xs is None:
        return couple(g, obs, *observe(g, x, obs, stencil), keep=keep)
    nobs, E = len(obs["var"]), xs[0]["ps"].shape[0]
    first = slot_rows(first, nobs)
    assert len(xs) == len(first) - 1
    pressure = bool(at_pressure(obs).any())
    hx, ps, out = np.zeros((nobs, E)), np.zeros((nobs, E)), np.zeros((nobs, E))
    for s, xsl in enumerate(xs):
        rows = slice(first[s], first[s + 1])
        if first[s + 1] > first[s]:
            got = observe(g, xsl, subset(obs, rows), None if stencil is None else (stencil[0][rows], stencil[1][rows]), pressure)
            hx[rows] = got[0]
            if pressure:
                ps[rows], out[rows] = got[1:]
    return couple(g, obs, hx, ps, out, keep)


def gc(r):
    """Gaspari and Cohn's fifth-order function as the kernel evaluates it; support r < 2.  The outer branch r^5/12 - r^4/2 + 5r^3/8
    + 5r^2/3 - 5r + 4 - 2/(3r) is taken in its factored form (2 - r)^4 (r^2 + 2r - 1/2) / (12 r), which does not cancel where the
    weight fades out"""
    r = np.asarray(r, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * (r * r) + 1.0
        s = 2.0 - r
        s2 = s * s
        outer = (s2 * s2) * ((r + 2.0) * r - 0.5) / (12.0 * r)
    return np.where(r < 2.0, np.where(r <= 1.0, inner, outer), 0.0)


def gc_powers(r):
    """the outer branch as the sum of powers of Gaspari and Cohn's eq. 4.10 (1 < r < 2)"""
    return r ** 5 / 12.0 - r ** 4 / 2.0 + 5.0 * r ** 3 / 8.0 + 5.0 * r ** 2 / 3.0 - 5.0 * r + 4.0 - 2.0 / (3.0 * r)


def distance(pc, po):
    """great-circle distance in metres of unit vectors pc (nc, 3) and po (no, 3) -> (nc, no)"""
    d = pc[:, None, :] - po[None, :, :]
    chord = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return 2.0 * REARTH * np.arcsin(np.minimum(1.0, 0.5 * chord))


def lnsigma(g, obs):
    return np.where(obs["var"] == PS, 0.0, g.lnfsg[np.where(obs["var"] == PS, 0, obs["lev"])])


def weights(g, unit, lnsigma, cols, sigma_h, sigma_v):
    """The localisation weight gc(dist / c_h) gc(|ln fsg_k - ln sigma_o| / c_v) of the observations at the unit vectors `unit`
    (nobs, 3) and vertical positions `lnsigma` (nobs) at the grid columns `cols` (None: all) -> w (ncols, kx, nobs); sigma_v <= 0:
    the horizontal factor alone at every level, and lnsigma is not read"""
    pc = g.colunit if cols is None else g.colunit[np.asarray(cols)]
    with np.errstate(invalid="ignore"):
        wh = gc(distance(pc, np.asarray(unit, np.float64).reshape(-1, 3)) / (sigma_h * np.sqrt(10.0 / 3.0)))
        if sigma_v > 0.0:
            wv = gc(np.abs(g.lnfsg[:, None] - np.asarray(lnsigma, np.float64)[None, :]) / (sigma_v * np.sqrt(10.0 / 3.0)))
            return wh[:, None, :] * wv[None, :, :]
    return np.broadcast_to(wh[:, None, :], (wh.shape[0], g.kx, wh.shape[1]))


def pair(m, r, n):
    """round-robin pair m of round r among n (even) players"""
    if m == 0:
        return n - 1, r
    return (r + m) % (n - 1), (r - m + n - 1) % (n - 1)


SLAB = 128           # matrices `jacobi` turns at a time
SWEEPS = 16          # LETKF_SWEEPS of csrc/spdy_letkf.hip: the most sweeps the kernel runs


def jacobi(A, sweeps=30, counts=False):
    """cyclic Jacobi on a batch of symmetric matrices (N, n, n) -> (lam (N, n), V (N, n, n)): round-robin pairs, an odd n padded by
    a decoupled row, a pair rotated unless |a_pq| <= eps/2 sqrt(a_pp a_qq), sweeps until no pair of any matrix rotates.  With
    counts also the sweeps each matrix ran (N,): its last sweep with a rotation and the idle one that closes it, `sweeps` at the most.
    A large batch goes slab by slab, each of a size that stays in cache and each until its own matrices are done: a sweep
    without a rotation changes no value, so a matrix's result does not depend on its neighbours"""
    N, n0 = A.shape[0], A.shape[1]
    if N > SLAB:
        parts = [jacobi(A[i:i + SLAB], sweeps, True) for i in range(0, N, SLAB)]
        lam, Vv, ran = (np.concatenate([part[n] for part in parts]) for n in range(3))
        return (lam, Vv, ran) if counts else (lam, Vv)
    ran = np.ones(N, np.int64)
    n = n0 + (n0 & 1)
    M = np.zeros((n, n, N))                                      # the batch last: a pair's rows and columns are whole slabs
    M[:n0, :n0] = np.moveaxis(A, 0, -1)
    if n != n0:
        M[n0, n0] = 1.0
    Vv = np.zeros((n, n, N))
    Vv[np.arange(n), np.arange(n)] = 1.0
    for sweep in range(sweeps):
        turned = np.zeros(N, bool)
        for r in range(n - 1):
            pq = [pair(m, r, n) for m in range(n // 2)]
            p, q = np.array([a for a, _ in pq]), np.array([b for _, b in pq])
            app, aqq, apq = M[p, p], M[q, q], M[p, q]
            with np.errstate(divide="ignore", invalid="ignore"):
                rot = ~(np.abs(apq) <= 0.5 * EPS * np.sqrt(app * aqq))
                theta = (aqq - app) / (2.0 * apq)
                t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = np.where(rot, 1.0 / np.sqrt(t * t + 1.0), 1.0)
            s = np.where(rot, t * c, 0.0)
            turned |= rot.any(axis=0)
            Mp, Mq = M[p], M[q]
            M[p], M[q] = c[:, None] * Mp - s[:, None] * Mq, s[:, None] * Mp + c[:, None] * Mq
            Mp, Mq = M[:, p], M[:, q]
            M[:, p], M[:, q] = c[None] * Mp - s[None] * Mq, s[None] * Mp + c[None] * Mq
            M[p, q] = np.where(rot, 0.0, M[p, q])
            M[q, p] = np.where(rot, 0.0, M[q, p])
            Vp, Vq = Vv[:, p], Vv[:, q]
            Vv[:, p], Vv[:, q] = c[None] * Vp - s[None] * Vq, s[None] * Vp + c[None] * Vq
        ran[turned] = min(sweep + 2, sweeps)
        if not turned.any():
            break
    lam = np.moveaxis(M[np.arange(n), np.arange(n)], -1, 0)[:, :n0]
    Vv = np.moveaxis(Vv, -1, 0)[:, :n0, :n0]      # the decoupled row keeps its place: column n0 of V stays e_n0
    return (lam, Vv, ran) if counts else (lam, Vv)


def local_problem(Y, d, r):
    """C (E, E) and b (E) of one local problem: each element summed over the observations in ascending order; an observation with
    r == 0 takes no part"""
    E = Y.shape[1]
    C, b = np.zeros((E, E)), np.zeros(E)
    for o in np.nonzero(r != 0.0)[0]:
        C = C + r[o] * (Y[o][:, None] * Y[o][None, :])
        b = b + r[o] * (Y[o] * d[o])
    return C, b


def transform(C, b, E, rho, route="eigh"):
    """batched: C (N, E, E), b (N, E) -> T (N, E, E), W, wbar, lam; rho: the scalar, or (N,), one value per problem (adaptive
    inflation: the diagonal of a problem is (E - 1) / rho of its level and column, one division)"""
    d = (E - 1) / np.asarray(rho, np.float64)
    A = C + (d[:, None, None] if d.ndim else d) * np.eye(E)
    lam, Vv = np.linalg.eigh(A) if route == "eigh" else jacobi(A)
    W = np.einsum("nfi,ni,nei->nfe", Vv, np.sqrt((E - 1) / lam), Vv)
    wbar = np.einsum("nfi,ni->nf", Vv, np.einsum("ngi,ng->ni", Vv, b) / lam)
    return W + wbar[:, :, None] - np.eye(E), W, wbar, lam


def problems(g, obs, s, sigma_h, sigma_v, cols=None, keep=None, r_eff=None):
    """C (ncols, kx, n, n) and b (ncols, kx, n) of the local problems at the grid columns `cols` (default: all) from the obs_space
    dict s: Y of the n members `keep` (default: all), d, ln sigma_o, and r = w r_eff with r_eff the 1/error^2 of this call, by
    default obs_used / error^2.  An observation is added in ascending order at the columns it reaches (r != 0 at some level) and
    nowhere else, as on the device: a non-finite Y stays within its range"""
    cols = np.arange(g.ix * g.il) if cols is None else np.asarray(cols)
    use = members(s["hx"].shape[1], keep)
    n, kx, nc = len(use), g.kx, len(cols)
    C, b = np.zeros((nc, kx, n, n)), np.zeros((nc, kx, n))
    if len(obs["var"]):
        Y, d = s["y"][:, use], s["departure"]
        r_eff = s["obs_used"] * (1.0 / (obs["error"] * obs["error"])) if r_eff is None else np.asarray(r_eff, np.float64)
        r = weights(g, unit(obs["lon"], obs["lat"]), s["obs_lnsigma"], cols, sigma_h, sigma_v) * r_eff[None, None, :]
        with np.errstate(invalid="ignore"):
            for o in np.nonzero((r != 0.0).any(axis=(0, 1)))[0]:
                at = (r[:, :, o] != 0.0).any(axis=1)
                C[at] += r[at, :, o, None, None] * (Y[o][:, None] * Y[o][None, :])
                b[at] += r[at, :, o, None] * (Y[o] * d[o])
    return C, b


def increments(g, x, C, b, rho, route="eigh", cols=None):
    """-> ({"u" .. "q": (E, kx, ncols), "ps": (E, ncols)}, the largest condition number of A)"""
    cols = np.arange(g.ix * g.il) if cols is None else np.asarray(cols)
    nc, kx, E = b.shape
    Tm, _, _, lam = transform(C.reshape(-1, E, E), b.reshape(-1, E), E, rho, route)
    Tm = Tm.reshape(nc, kx, E, E)
    out = {}
    for v in VARS:
        f = x[v].reshape(E, -1, g.il * g.ix)[:, :, cols]                     # (E, kx or 1, ncols)
        s = np.zeros(f.shape[1:])
        for e in range(E):
            s = s + f[e]
        xp = f - (s / E)[None]
        Tv = Tm if v != "ps" else Tm[:, kx - 1:kx]
        out[v] = np.einsum("fkc,ckfe->ekc", xp, Tv)
    out["ps"] = out["ps"][:, 0]
    return out, float(np.max(lam.max(axis=1) / lam.min(axis=1)))


def analyse(g, x, obs, sigma_h, sigma_v, rho, route="eigh", cols=None, keep=None, stencil=None, r_eff=None, xs=None, first=None):
    """The increments of the members in use of the gridded ensemble x at the grid columns `cols` (default: all), and the largest
    condition number.  keep: the members in use; stencil: `observe`'s; r_eff: `problems`'; xs, first: `obs_space`'s, Y and d are
    then from the slots' times and the increments are formed on x"""
    C, b = problems(g, obs, obs_space(g, x, obs, keep, stencil, xs, first), sigma_h, sigma_v, cols, keep, r_eff)
    return increments(g, compact(x, keep), C, b, rho, route, cols)


def at_columns(a, cols):
    """a device result (E, kx, il, ix) / (E, il, ix) at grid columns, in the shape `increments` gives"""
    return a.reshape(a.shape[:-2] + (-1,))[..., cols]


def perturbation_scale(x):
    """max |x_e - mean| per variable"""
    return {v: float(np.max(np.abs(x[v] - x[v].mean(axis=0)))) for v in VARS}


# ---------------------------------------------------------------------------------------------------- inputs of the tests
SCALE = {"u": (5.0, 3.0), "v": (0.0, 3.0), "t": (260.0, 2.0), "q": (4.0, 0.8), "ps": (0.0, 0.01)}      # (base, member spread)


def ensemble(g, E, seed=0):
    """a gridded ensemble of E different members: a smooth base state plus white member noise of SCALE's spread"""
    rng = np.random.default_rng(seed)
    lo, la = np.meshgrid(np.radians(g.lon), np.radians(g.lat))
    x = {}
    for v in VARS:
        base, s = SCALE[v]
        shape = (E, g.kx, g.il, g.ix) if v != "ps" else (E, g.il, g.ix)
        lev = np.arange(g.kx)[:, None, None] if v != "ps" else 0.0
        x[v] = base + 3.0 * s * np.cos(la) * np.sin(2.0 * lo + 0.3 * lev) + s * rng.standard_normal(shape)
    return x


def observations(g, x, var, lev, lon, lat, err_factor, seed=1):
    """observations of member 0 with errors err_factor * SCALE's spread: value = H x_0 + error * noise"""
    rng = np.random.default_rng(seed)
    err = err_factor * np.array([SCALE[VARS[v]][1] for v in var])
    obs = make_obs(var, lev, lon, lat, np.zeros(len(var)), err)
    obs["value"] = observe(g, x, obs)[0][:, 0] + err * rng.standard_normal(len(var))
    return obs


def edge_points(g):
    """(lon, lat) of the operator's edge cases: on a grid point, between columns ix-1 and 0, poleward of the outermost row at both
    poles, at lon = 360, at negative longitude, on the outermost rows themselves"""
    return [(float(g.lon[5]), float(g.lat[7])), (359.0, 12.3), (float(g.lon[-1]) + 1.7, -33.0), (10.0, 89.9), (200.0, -89.5),
            (77.0, 90.0), (300.0, -90.0), (360.0, 45.0), (-12.5, -5.0), (-360.0, 0.0), (725.0, 60.0), (40.0, float(g.lat[0])),
            (41.0, float(g.lat[-1])), (0.0, 0.0)]


def edge_obs(g, x, nrandom=26, err_factor=0.5, seed=3):
    """about 40 observations: every edge point with a cycling variable and level, then random ones"""
    rng = np.random.default_rng(seed)
    pts = edge_points(g) + [(float(rng.uniform(-400, 400)), float(rng.uniform(-90, 90))) for _ in range(nrandom)]
    var = [o % 5 for o in range(len(pts))]
    lev = [(3 * o) % g.kx for o in range(len(pts))]
    return observations(g, x, var, lev, [p[0] for p in pts], [p[1] for p in pts], err_factor, seed)


def clustered_obs(g, x, n=1500, centre=(100.0, 20.0), half_width=3.0, err_factor=0.125, seed=5):
    """n observations of every variable and level within half_width degrees of centre: all in range of the columns around it"""
    rng = np.random.default_rng(seed)
    var = rng.integers(0, 5, n)
    lev = rng.integers(0, g.kx, n)
    lon = centre[0] + rng.uniform(-half_width, half_width, n)
    lat = centre[1] + rng.uniform(-half_width, half_width, n)
    return observations(g, x, var, lev, lon, lat, err_factor, seed)


def sparse_obs(g, x, n=60, err_factor=0.125, seed=7):
    """n observations spread over the globe"""
    rng = np.random.default_rng(seed)
    return observations(g, x, rng.integers(0, 5, n), rng.integers(0, g.kx, n), rng.uniform(0, 360, n),
                   np.degrees(np.arcsin(rng.uniform(-1, 1, n))), err_factor, seed)


def columns_for(g, obs, sigma_h, most=48, outside=16, seed=11):
    """columns to compare at: up to `most` in range of an observation (the nearest ones and the farthest ones among them) and
    `outside` that are out of range of all"""
    rng = np.random.default_rng(seed)
    dmin = distance(g.colunit, unit(obs["lon"], obs["lat"])).min(axis=1)
    inside = np.nonzero(dmin < 2.0 * sigma_h * np.sqrt(10.0 / 3.0))[0]
    inside = inside[np.argsort(dmin[inside])]
    if len(inside) > most:
        inside = np.concatenate([inside[:most // 2], inside[-(most // 4):], rng.choice(inside[most // 2:-(most // 4)], most // 4, False)])
    out = np.nonzero(dmin >= 2.0 * sigma_h * np.sqrt(10.0 / 3.0))[0]
    return np.concatenate([inside, rng.choice(out, min(outside, len(out)), False)]).astype(np.int64)


def edge_columns(g):
    """every column of rows 0, 1, il-2, il-1 and of longitudes 0 and ix-1, ascending: where the column unit vectors, the latitude
    table and the periodic wrap meet"""
    jj, ii = np.divmod(np.arange(g.ix * g.il), g.ix)
    return np.nonzero(np.isin(jj, (0, 1, g.il - 2, g.il - 1)) | np.isin(ii, (0, g.ix - 1)))[0]


def pad_obs(g, x, n, centre, err_factor=0.125, seed=13):
    """n observations within 1 degree (great circle) of centre, variables and levels cycling, values and errors as `observe` gives"""
    rng = np.random.default_rng(seed)
    lat = centre[1] + rng.uniform(-0.7, 0.7, n)
    lon = centre[0] + rng.uniform(-0.7, 0.7, n) / np.cos(np.radians(centre[1]))
    return observations(g, x, [o % 5 for o in range(n)], [(3 * o) % g.kx for o in range(n)], lon, lat, err_factor, seed)


PATTERNS = ("front1", "front255", "front256", "alternate", "wave3", "hole")


def interleave(real, pad, pattern, total=None):
    """-> (the set, the places of real's observations in it): `real` in its order with observations of `pad`, taken in theirs,
    inserted -- front1, front255, front256: so many in front (256: the kernel's first chunk has no survivor); alternate: one
    before every real one; wave3: in every chunk of 256, 192 of pad and then 64 real ones (survivors in the chunk's last wave
    only); hole: 256 real ones, a whole chunk of pad, the other real ones.  `total`: pad appended at the end up to that size"""
    nr = len(real["var"])
    if pattern in ("front1", "front255", "front256"):
        places = int(pattern[5:]) + np.arange(nr)
    elif pattern == "alternate":
        places = 2 * np.arange(nr) + 1
    elif pattern == "wave3":
        places = (np.arange(nr) // 64) * CHUNK + 192 + np.arange(nr) % 64
    elif pattern == "hole":
        places = np.arange(nr) + np.where(np.arange(nr) < CHUNK, 0, CHUNK)
    else:
        raise ValueError(pattern)
    n = max(int(places[-1]) + 1, total or 0)
    assert total is None or n == total, (pattern, n, total)
    isreal = np.zeros(n, bool)
    isreal[places] = True
    assert n - nr <= len(pad["var"]), (pattern, n - nr)
    out = {}
    for k in real:
        out[k] = np.zeros(n, real[k].dtype)
        out[k][places] = real[k]
        out[k][~isreal] = pad[k][:n - nr]
    return out, places


# ------------------------------------------------------------------------------------------------ what the GPU tests share
SIGMA_H, RHO = 5.0e5, 1.1
C_H = SIGMA_H * np.sqrt(10.0 / 3.0)
WRAP, CLUSTER, PAD_CENTRE, HARD_CENTRE = (359.5, 0.0), (100.0, 20.0), (280.0, -60.0), (30, 15)


EDGE_SIGMA_H = 3.0e5      # of the edge-column tests: at 5e5 edge_obs alone leaves no column of longitudes 0 and ix-1 out of range


def in_range(g, obs, cols=None, sigma_h=SIGMA_H):
    """(ncols, nobs): the observation has a non-zero horizontal weight at the column"""
    return weights(g, unit(obs["lon"], obs["lat"]), None, cols, sigma_h, 0.0)[:, 0] != 0.0


def edge_inputs(g, x):
    """the observations of the edge-column tests as (name, set): edge_obs; 200 within 2 degrees of WRAP, between columns ix-1 and
    0 on the equator; 200 within 1.5 degrees of latitude +88 at longitudes all around the circle; the same at -88"""
    sets = [("edge", edge_obs(g, x)), ("wrap", clustered_obs(g, x, n=200, centre=WRAP, half_width=2.0 / np.sqrt(2.0), seed=21))]
    for name, lat, seed in (("north", 88.0, 22), ("south", -88.0, 23)):
        rng = np.random.default_rng(seed)
        sets.append((name, observations(g, x, rng.integers(0, 5, 200), rng.integers(0, g.kx, 200), rng.uniform(0.0, 360.0, 200),
                                   lat + rng.uniform(-1.5, 1.5, 200), 0.125, seed)))
    return sets


def edge_conditions(g, sets):
    """what the edge-column tests need of their inputs at sigma_h = EDGE_SIGMA_H, asserted: at least 90 % of the columns of rows 0
    and il-1 in range of 50 observations or more, columns of i = 0 and of i = ix-1 in range of the wrap cluster, edge columns out
    of range of everything; -> (the observations, edge_columns, which of those are out of range of everything)"""
    obs, cols = concat(*[s for _, s in sets]), edge_columns(g)
    jj, ii = np.divmod(cols, g.ix)
    near = in_range(g, obs, cols, EDGE_SIGMA_H)
    polar = np.isin(jj, (0, g.il - 1))
    assert polar.sum() == 2 * g.ix and (near[polar].sum(axis=1) >= 50).sum() >= 0.9 * polar.sum()
    wrap = in_range(g, dict(sets)["wrap"], cols, EDGE_SIGMA_H).any(axis=1)
    assert (wrap & (ii == 0)).any() and (wrap & (ii == g.ix - 1)).any()
    out = ~near.any(axis=1)
    assert out.sum() >= 8, out.sum()
    return obs, cols, out


def padded_inputs(g, x):
    """the padded-scan tests' sets -> (real, pad): real is a cluster of 320 around CLUSTER and the sparse set's observations farther
    than 4 c_h from PAD_CENTRE (at least 40 of its 60), pad is 1 200 observations within a degree of PAD_CENTRE"""
    sparse = sparse_obs(g, x)
    keep = distance(unit([PAD_CENTRE[0]], [PAD_CENTRE[1]]), unit(sparse["lon"], sparse["lat"]))[0] > 4.0 * C_H
    assert keep.sum() >= 40, keep.sum()
    real = concat(clustered_obs(g, x, n=320, centre=CLUSTER), {k: v[keep] for k, v in sparse.items()})
    return real, pad_obs(g, x, 1200, PAD_CENTRE)


def padded_conditions(g, real, pad, least=4300):
    """-> (far, acted): the columns farther than 2 c_h (1 + 1e-12) from every pad observation -- at least `least`, every column in
    range of real's cluster among them -- and the columns in range of a pad observation"""
    far = distance(g.colunit, unit(pad["lon"], pad["lat"])).min(axis=1) > 2.0 * C_H * (1.0 + 1e-12)
    cluster = in_range(g, {k: v[:320] for k, v in real.items()}).any(axis=1)
    assert far.sum() >= least and cluster.sum() >= 64 and far[cluster].all(), (far.sum(), cluster.sum())
    return far, in_range(g, pad).any(axis=1)


def hard_obs(g, x, err_factor):
    """16 observations of cycling variables within a degree of the grid point HARD_CENTRE, errors err_factor x SCALE's spread: C of
    rank 16 among E = 31 or 32 members, far above the diagonal (E-1)/rho"""
    i, j = HARD_CENTRE
    return pad_obs(g, x, 16, (float(g.lon[i]), float(g.lat[j])), err_factor, seed=17)


def make(sp, E, obs, sigma_v=0.0, rho=RHO, sigma_h=SIGMA_H):
    """the analysis object of E members with the observations obs set"""
    import speedy_f90_amd as s
    lt = s.Letkf(sp, E, max(len(obs["var"]), 1), sigma_h, sigma_v, rho)
    lt.set_obs(*args(obs))
    return lt


def grids(x):
    """the gridded ensemble x (NumPy) as the five device tensors of Letkf.analyse_grid"""
    return [support.dev(x[v]) for v in VARS]


def run(lt, x, use=None, slots=False, out=None, names=FIELDS):
    """Letkf.analyse_grid on the gridded ensemble x (NumPy) -> the increments under VARS, the fields `names` (those with an item:
    none per observation of an empty network), members_used, and what the object's settings add -- inflation with relaxation on,
    weights at a weight stride, rho, infl_parm and obs_s2 with adaptive inflation on -- as NumPy arrays"""
    import torch
    got = lt.analyse_grid(*grids(x), out=out, use=use, slots=slots)
    torch.cuda.synchronize()
    got = {v: a.cpu().numpy() for v, a in zip(VARS, got)}
    names = tuple(names) + ("members_used",) + (("inflation",) if lt.relaxation != (0.0, 0.0) else ())
    names += (("weights",) if lt.weight_stride != (1, 1) else ()) + (("rho", "infl_parm", "obs_s2") if lt.adaptive is not None else ())
    for n in dict.fromkeys(names):
        f = lt.field(n)
        if 0 not in f.shape:
            got[n] = f.numpy().copy()
    return got


def limits(g, x, C, b, rho, cols, E, sample=None):
    """per variable max(16 x the difference of the restatement's two routes on these inputs, 64 E eps max|x - mean|), the eigh
    route's increments and the largest condition number.  `sample` (places in cols): the Jacobi route, the costly one, runs at
    those columns only; a largest difference over fewer columns is no larger, so the limit is the same or stricter"""
    cols = np.asarray(cols)
    a, kappa = increments(g, x, C, b, rho, "eigh", cols)
    at = np.arange(len(cols)) if sample is None else np.asarray(sample)
    j, _ = increments(g, x, C[at], b[at], rho, "jacobi", cols[at])
    sc = perturbation_scale(x)
    return {v: max(16 * float(np.max(np.abs(a[v][..., at] - j[v]))), 64 * E * EPS * sc[v]) for v in VARS}, a, kappa


def hardest(C, rho, n):
    """places of n columns for `limits`' sample: the n/2 whose A = (E-1)/rho I + C has the largest condition number at some level,
    and as many spread evenly over the rest"""
    E = C.shape[-1]
    lam = np.linalg.eigvalsh(C + ((E - 1) / rho) * np.eye(E))
    order = np.argsort((lam[..., -1] / lam[..., 0]).max(axis=1))
    rest = order[:len(order) - n // 2]
    return np.unique(np.concatenate([order[len(order) - n // 2:], rest[::max(1, len(rest) // (n - n // 2))]]))


def oracle_grids(o, sts):
    """time level 1 of the member states on the grid by the oracle's transforms: true wind, t, q, ps"""
    x = {v: [] for v in VARS}
    for st in sts:
        uv = [o.uvspec(st["vor"][0, k], st["div"][0, k]) for k in range(o.kx)]
        x["u"].append(np.stack([o.spec_to_grid(a, 2) for a, _ in uv]))
        x["v"].append(np.stack([o.spec_to_grid(b, 2) for _, b in uv]))
        x["t"].append(np.stack([o.spec_to_grid(st["t"][0, k], 1) for k in range(o.kx)]))
        x["q"].append(np.stack([o.spec_to_grid(st["tr"][0, k], 1) for k in range(o.kx)]))
        x["ps"].append(o.spec_to_grid(st["ps"][0], 1))
    return {v: np.stack(a) for v, a in x.items()}


def spread_obs(g, x, n, seed):
    """n observations over the globe (the operator's edge points first), each with half the members' spread at its place as error"""
    rng = np.random.default_rng(seed)
    pts = (edge_points(g) + [(float(rng.uniform(0, 360)), float(rng.uniform(-85, 85))) for _ in range(n)])[:n]
    obs = make_obs([o % 5 for o in range(n)], [(3 * o) % g.kx for o in range(n)], [p[0] for p in pts], [p[1] for p in pts],
                   np.zeros(n), np.ones(n))
    hx = observe(g, x, obs)[0]
    obs["error"] = 0.5 * hx.std(axis=1, ddof=1) + 1e-300
    obs["value"] = hx[:, 0] + obs["error"] * rng.standard_normal(n)
    return obs
