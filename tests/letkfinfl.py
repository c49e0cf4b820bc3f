"""Adaptive inflation restated in NumPy (include/spdy.h, "adaptive inflation"): s2 of every observation, the sums
p1, p2, p3 of every (level, column) over the observations in ascending order, and the update of the field rho.  Every operation is
one IEEE operation in the header's order, so what is +, -, *, / only -- s2 and the update -- has the device's bits; the sums go
through asin and the column's unit vector and agree within `bound`."""
import numpy as np

import letkf as lk
import letkfqc as qc

SIGMA_B, RHO_MIN, RHO_MAX = 0.04, 0.9, 3.0       # Letkf.set_adaptive_inflation's defaults


def s2(y, keep=None):
    """s2_o = (sum_U y_e^2) / (n - 1): the background check's, with its bits"""
    return qc.spread2(y, keep)


def horizontal(g, ounit, sigma_h, cols=None):
    """wh (ncols, nobs): letkf.weights without a vertical scale"""
    return lk.weights(g, ounit, None, cols, sigma_h, 0.0)[:, 0]


def sums(g, ounit, olns, reff, dep, s2o, sigma_h, sigma_v, cols=None):
    """p (3, kx, ncols): p1 = sum r dep^2, p2 = sum r s2, p3 = sum w over the observations ascending, with wh = gc(dist / c_h)
    (skipped if 0), w = c_v > 0 ? wh gc(|ln fsg_k - ln sigma_o| / c_v) : wh, r = w reff_o, and an observation with r == 0 taking no
    part.  ounit (nobs, 3), olns, reff, dep, s2o (nobs): what the analysis call read -- the object's unit table, obs_lnsigma, the
    per-call 1 / error^2, departure, obs_s2"""
    ounit, dep, s2o, reff, olns = (np.asarray(a, np.float64) for a in (ounit, dep, s2o, reff, olns))
    ounit = ounit.reshape(-1, 3)
    wh = horizontal(g, ounit, sigma_h, cols)
    p = np.zeros((3, g.kx, wh.shape[0]))
    d2 = dep * dep
    with np.errstate(invalid="ignore", over="ignore"):
        for o in np.nonzero((wh != 0.0).any(axis=0))[0]:
            near = wh[:, o] != 0.0
            w = lk.weights(g, ounit[o:o + 1], olns[o:o + 1], cols, sigma_h, sigma_v)[:, :, 0].T
            r = w * reff[o]
            take = near[None, :] & (r != 0.0)
            p[0] = np.where(take, p[0] + r * d2[o], p[0])
            p[1] = np.where(take, p[1] + r * s2o[o], p[1])
            p[2] = np.where(take, p[2] + w, p[2])
    return p


def bound(g, ounit, reff, dep, s2o, sigma_h, cols=None):
    """(3, ncols): 64 eps n_loc max_o(term) for p1, p2, p3, with n_loc the observations in horizontal range of the column, the
    largest term over them, and term rinv_o dep_o^2, rinv_o s2_o and 1.  From unit weights: the device's asin and the column's
    unit vector differ from NumPy's by ulps, gc's slope is bounded, so a weight is wrong by a few eps in absolute terms (its
    relative error is unbounded where it fades out), and a sum of n_loc terms by n_loc times that times the largest term; the
    sum's own rounding is of the same form.  A non-finite term leaves its columns out (the sums are NaN on both sides there)"""
    near = horizontal(g, ounit, sigma_h, cols) != 0.0
    dep, s2o, reff = (np.asarray(a, np.float64) for a in (dep, s2o, reff))
    out = np.zeros((3, near.shape[0]))
    nloc = near.sum(axis=1)
    for i, term in enumerate((reff * (dep * dep), reff * s2o, np.ones(near.shape[1]))):
        big = np.where(near, np.abs(term)[None, :], 0.0).max(axis=1) if near.shape[1] else np.zeros(near.shape[0])
        out[i] = 64.0 * lk.EPS * nloc * big
    return out


def update(rho, p, sigma_b, rho_min=RHO_MIN, rho_max=RHO_MAX):
    """rho' of every item from the sums p (3, ...) and the prior field.  Where p3 > 0 and p2 > 0:
        ro = (p1 - p3) / p2;  t = (rho p2 + p3) / p2;  vo = (2 / p3) (t t);  g = vb / (vo + vb);  est = rho + g (ro - rho)
        rho' = fmin(fmax(est, rho_min), rho_max) if est is finite, else rho
    everywhere else rho' = rho, with rho's bits"""
    rho = np.asarray(rho, np.float64)
    p1, p2, p3 = (np.asarray(a, np.float64).reshape(rho.shape) for a in p)
    vb = np.float64(sigma_b) * np.float64(sigma_b)
    with np.errstate(all="ignore"):
        ro = (p1 - p3) / p2
        t = (rho * p2 + p3) / p2
        vo = (2.0 / p3) * (t * t)
        gain = vb / (vo + vb)
        est = rho + gain * (ro - rho)
        new = np.fmin(np.fmax(est, rho_min), rho_max)
    return np.where((p3 > 0.0) & (p2 > 0.0) & np.isfinite(est), new, rho)


def observed(p):
    """ro = (p1 - p3) / p2 where the update is made, NaN elsewhere"""
    with np.errstate(all="ignore"):
        return np.where((p[2] > 0.0) & (p[1] > 0.0), (p[0] - p[2]) / p[1], np.nan)


def call_inputs(lt, reff_field=False):
    """what an analysis call of the object lt read, downloaded: the unit table, obs_lnsigma, the per-call 1 / error^2 (obs_rinv where
    the call wrote it -- a network with observations at a pressure or the background check on -- the table rinv otherwise),
    departure and y"""
    return {"unit": lt.table("unit"), "olns": lt.field("obs_lnsigma").numpy(),
            "reff": lt.field("obs_rinv").numpy() if reff_field else lt.table("rinv"),
            "dep": lt.field("departure").numpy(), "y": lt.field("y").numpy()}


def restate(g, lt, rho, sigma_h, sigma_v, sigma_b, rho_min=RHO_MIN, rho_max=RHO_MAX, keep=None, reff_field=False, cols=None):
    """the restatement fed the device's own observation-space arrays of the latest call -> (s2, p, the bound, rho' from p)"""
    a = call_inputs(lt, reff_field)
    s2o = s2(a["y"], keep)
    p = sums(g, a["unit"], a["olns"], a["reff"], a["dep"], s2o, sigma_h, sigma_v, cols)
    lim = bound(g, a["unit"], a["reff"], a["dep"], s2o, sigma_h, cols)
    return s2o, p, lim, update(rho, p.reshape((3,) + np.shape(rho)), sigma_b, rho_min, rho_max)


def worst_ratio(got, want, lim):
    """the largest |got - want| / bound over the items (3, kx, ncols) vs (3, ncols); an item whose bound is 0 has to be met exactly;
    items that are NaN on both sides are left out"""
    got, want = got.reshape(want.shape), want
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        err = np.where(both, 0.0, np.abs(got - want))
    err = np.where(np.isnan(err), np.inf, err)              # a NaN on one side only is a miss
    lim =np.broadcast_to(lim[:, None, :], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / lim)
    return float(np.nanmax(ratio)) if ratio.size else 0.0
