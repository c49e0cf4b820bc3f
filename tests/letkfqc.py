"""The background check and the observation statistics restated in NumPy (include/spdy.h, "background check and observation
statistics"): the decision per observation from y, the departure and the error, the per-call 1/error^2 the local
analyses read, and the statistics of every group in the header's summation order -- partial t of 1024 takes the group's used
observations with o mod 1024 == t, o ascending, then a halving tree -- so the device's sums can be held to the bit.  Every operation
is one IEEE operation, as NumPy's element-wise arithmetic is.  The checked analysis is tests/letkf.py's with r_eff = reff(used,
1 / error^2).  Also the helpers the tests of the check share."""
import numpy as np

import letkf as lk
import support

PARTS = 1024         # QC_BLOCK of csrc/spdy_letkf.hip: the partial sums of a group
COLUMNS = ("n_all", "n_out", "n_rej", "n_used", "sum_dep", "sum_dep2", "sum_s2", "sum_err2", "sum_dep_depb", "sum_depb")
PASSED, REJECTED, OUT = 0.0, 1.0, 2.0


def spread2(y, keep=None):
    """s2_o = (sum_U y_e^2) / (n - 1): each square rounded, summed over U ascending, one division; n < 2 divides by 0 or -1, as
    the device does (the test is not made then)"""
    y = np.asarray(y, np.float64)
    U = lk.members(y.shape[1], keep)
    s = np.zeros(y.shape[0])
    for e in U:
        s = s + y[:, e] * y[:, e]
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / np.float64(len(U) - 1)


def check(y, dep, err, gross, in_column=None, keep=None):
    """-> {"s2", "v", "rej", "used" (bool), "check" (0.0 passed, 1.0 rejected, 2.0 out of column: out of column wins)}.  A NaN
    makes the comparison false; n < 2 or gross == 0: the test is not made"""
    y, dep, err = np.asarray(y, np.float64), np.asarray(dep, np.float64), np.asarray(err, np.float64)
    n = len(lk.members(y.shape[1], keep))
    s2 = spread2(y, keep)
    g2 = np.float64(gross) * np.float64(gross)
    v = s2 + err * err
    with np.errstate(invalid="ignore"):
        rej = (dep * dep > g2 * v) if (g2 > 0.0 and n >= 2) else np.zeros(len(dep), bool)
    incol = np.ones(len(dep), bool) if in_column is None else np.asarray(in_column) != 0
    code = np.where(~incol, OUT, np.where(rej, REJECTED, PASSED))
    return {"s2": s2, "v": v, "rej": rej, "used": code == PASSED, "check": code}


def reff(used, rinv):
    """the 1/error^2 the local analyses read: exactly 0 for an observation that is not used"""
    return np.where(used, rinv, 0.0)


def tree(terms, take):
    """the sum of terms[o] over the observations with take[o], in the header's order: partial t starts at +0.0 and adds the terms
    with o mod 1024 == t, o ascending; then partial t = partial t + partial (t + h), t < h, for h = 512 .. 1; partial 0 is the sum"""
    n = len(terms)
    part = np.zeros(PARTS)
    with np.errstate(invalid="ignore", over="ignore"):
        for base in range(0, n, PARTS):
            t = np.arange(min(PARTS, n - base))
            sel = take[base + t]
            part[t[sel]] = part[t[sel]] + terms[base + t[sel]]
        h = PARTS // 2
        while h >= 1:
            part[:h] = part[:h] + part[h:2 * h]
            h //= 2
    return part[0]


def stats(group, ngroups, code, dep, s2, err, depb=None):
    """-> [ngroups, 10], COLUMNS: the counts of every group and the sums over its used observations (code == 0); depb: the
    departure of the analysis call (a stats-only call), default dep itself"""
    group, code = np.asarray(group), np.asarray(code, np.float64)
    dep, s2, err = np.asarray(dep, np.float64), np.asarray(s2, np.float64), np.asarray(err, np.float64)
    depb = dep if depb is None else np.asarray(depb, np.float64)
    one = np.ones(len(dep))
    out = np.zeros((ngroups, len(COLUMNS)))
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (dep, dep * dep, s2, err * err, dep * depb, depb)
    for g in range(ngroups):
        mine = group == g
        used = mine & (code == PASSED)
        out[g, 0] = tree(one, mine)
        out[g, 1] = tree(one, mine & (code == OUT))
        out[g, 2] = tree(one, mine & (code == REJECTED))
        out[g, 3] = tree(one, used)
        for i, t in enumerate(terms):
            out[g, 4 + i] = tree(t, used)
    return out


def plant(obs, hxmean, s2, gross, seed, groups=None, ngroups=5):
    """values on both sides of the threshold in every group: for four observations of every non-empty group the value becomes
    hxmean +- gross sqrt(v) (1 +- 1e-9) -- outside (rejected) and inside (passed), above and below the mean.  -> (the new values,
    the places planted outside, the places planted inside)"""
    rng = np.random.default_rng(seed)
    groups = obs["var"] if groups is None else np.asarray(groups)
    value = obs["value"].copy()
    edge = gross * np.sqrt(s2 + obs["error"] * obs["error"])
    outside, inside = [], []
    for gid in range(ngroups):
        mine = np.nonzero(groups == gid)[0]
        pick = rng.permutation(mine)[:4]
        for o, (sign, side) in zip(pick, ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))):
            value[o] = hxmean[o] + sign * edge[o] * (1.0 + side * 1e-9)
            (outside if side > 0 else inside).append(int(o))
    return value, np.array(sorted(outside), np.int64), np.array(sorted(inside), np.int64)


def same_rows(got, want):
    """the statistics' rows bit for bit; where one holds a NaN the other must too (a NaN's sign and payload are the hardware's)"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and support.same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want))


# ------------------------------------------------------------------------------------------------ what the GPU tests share
def restated(got, obs, gross, groups=None, ngroups=5, in_column=None, keep=None, depb=None, code=None):
    """the restatement on the device's own y, departure and errors -> (decisions, the statistics' rows)"""
    dec = check(got["y"], got["departure"], obs["error"], gross, in_column, keep)
    code = dec["check"] if code is None else code
    rows = stats(obs["var"] if groups is None else groups, ngroups, code, got["departure"], dec["s2"], obs["error"], depb)
    return dec, rows


def table(stats):
    return np.stack([stats[n] for n in COLUMNS], axis=1)


def same_decisions(got, dec, obs):
    rinv = 1.0 / (obs["error"] * obs["error"])
    return (support.same_bits(got["obs_used"], dec["used"].astype(np.float64)) and support.same_bits(got["obs_check"], dec["check"])
            and support.same_bits(got["obs_rinv"], reff(dec["used"], rinv)))
