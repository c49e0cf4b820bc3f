"""CPU: observations given at a pressure without a device (include/spdy.h, "ensemble analysis, observations at a pressure") -- the
NumPy restatement the GPU tests compare against is held to np.interp; the crafted inputs hold every class they claim; spdy_pobs_set
exists in the library, the header, the loader and the Fortran binding; a host-only plan answers its argument checks in the header's
order with the text of spdy_last_error, a rejected call changes no table, and the lifetime rule holds.  (An open capture needs a
device: tests/test_gpu_letkf_pressure.py has that rejection.)"""
import ctypes
import math

import numpy as np
import pytest

import letkf as lk
import letkfpressure as lp
import nature as nt
import pressurelevels as pl
import support
from ensembleoutput import P0

ERR_ARG, ERR_NO_DEVICE, ERR_STATE = -1, -3, -5
TABLES = ("stencil_index", "stencil_weight", "unit", "lnsigma", "rinv", "lnp")


def _plan(kx, nmem=32):
    s = support.package()
    if kx == 2:
        sp = s.Spectral("t30", kx=2, max_batch=nmem * 5, device=-1)
        sp.set_sigma(pl.SIGMA_L2)
        return sp
    return support.plan({5: "t30k5", 8: "t30"}[kx], nmem * (2 * kx + 1), device=-1)


@pytest.fixture(scope="module")
def hosts():
    s = support.package()
    with support.plan_cache(_plan) as get:
        yield s, lambda kx: (get(kx), lp.Geometry(get(kx)))


def code(s, fn, *a):
    with pytest.raises(s.SpdyError) as err:
        fn(*a)
    return err.value.code


@pytest.mark.parametrize("kx", [2, 5, 8])
def test_restatement_against_np_interp(kx, hosts):
    """The per-column value against np.interp(x_o, X, f) on X_k = ps + ln fsg[k]: bit-equal where the target is clamped to an end
    level; inside within 8 eps (max|f| + A max|df|), the rule tests/test_pressure_levels_cpu.py holds the linear coordinate to,
    with A = max_k max|X_{k+1}| / (ln fsg[k+1] - ln fsg[k]) for this coordinate: X_k is a rounded sum of size |X|, so the weight (x
    - X_k) / (X_{k+1} - X_k) carries a relative error of that many eps, and np.interp's own slope form a few more roundings, each
    amplified by at most 1"""
    _, get = hosts
    _, g = get(kx)
    r = np.random.default_rng(11 + kx)
    ncol = 4000
    f = 250.0 + 30.0 * r.standard_normal((1, kx, ncol))
    ps = r.uniform(math.log(0.5), math.log(1.05), (1, ncol))
    X = ps[:, None, :] + g.lnf[None, :, None]
    A = float(np.max(np.abs(X[0, 1:]).max(axis=1) / np.diff(g.lnf)))
    bound = 8 * lk.EPS * (float(np.max(np.abs(f))) + A * float(np.max(np.abs(np.diff(f, axis=1)))))
    worst, seen = 0.0, set()
    for xo in list(r.uniform(math.log(0.005), math.log(1.08), 12)) + [float(g.lnf[0]), float(g.lnf[-1])]:
        z, kb, lo, hi, out = lp.column_values(X, f, xo)
        ref = np.array([np.interp(xo, X[0, :, c], f[0, :, c]) for c in range(ncol)])
        clamped = (lo | hi)[0]
        assert np.array_equal(z[0][clamped], ref[clamped])
        assert np.array_equal(z[0][lo[0]], f[0, 0][lo[0]]) and np.array_equal(z[0][(hi & ~lo)[0]], f[0, -1][(hi & ~lo)[0]])
        assert not out[0][~clamped].any()                    # out of column implies clamped; on an end level: clamped and in column
        assert np.array_equal(out[0], (xo < X[0, 0]) | (xo > X[0, -1]))
        worst = max(worst, float(np.max(np.abs(z[0] - ref))))
        seen |= {"clamped"} if clamped.any() else set()
        seen |= {"inside"} if (~clamped).any() else set()
        seen |= {"out"} if out.any() else set()
    print("[pobs restatement kx=%d] max error %.3e, bound %.3e, ratio %.3f" % (kx, worst, bound, worst / bound))
    assert seen == {"clamped", "inside", "out"} and worst <= bound


@pytest.mark.parametrize("kx", [2, 5, 8])
def test_crafted_inputs_hold_every_class(kx, hosts):
    """the crafted ensemble and network of the GPU tests: every bracket, the first and the last, members in different brackets, a
    target on an end level (in column), above every top, below for one member at one point, at some points and at all four, stencils
    across the date line and poleward of the last row, model-level and PS observations; about 600 observations"""
    _, get = hosts
    _, g = get(kx)
    for E in (2, 3):
        x = lp.craft(g, E, seed=7 + E)
        obs = lp.network(g, x)
        assert lp.classes(g, x, obs) == lp.every_class(kx), (kx, E, lp.classes(g, x, obs) ^ lp.every_class(kx))
        s = lk.obs_space(g, x, obs)
        atp = lp.at_pressure(obs)
        assert (550 <= len(obs["var"]) <= 650 if kx == 8 else len(obs["var"]) > 200) and atp.sum() >= 150 and (~atp).sum() >= 50
        assert (s["obs_used"][~atp] == 1.0).all() and 10 <= (s["obs_used"] == 0.0).sum() < atp.sum() / 2
        assert np.isfinite(s["hx"]).all()


def test_entry_point_is_bound(hosts):
    s, _ = hosts
    from speedy_f90_amd import _lib
    lib = ctypes.CDLL(s.LIB_PATH)
    assert hasattr(lib, "spdy_pobs_set") and "spdy_pobs_set" in _lib.SIGNATURES and "spdy_pobs_set" in support.fortran_bound()
    assert support.declaration("spdy_pobs_set") == "spdy_letkf *l, int nobs, const spdy_pobs *host"
    assert "SPDY_OBS_AT_P = -1" in support.header() and "SPDY_OBS_AT_P = -1_c_int" in support.fortran_binding()
    assert s.OBS_AT_P == -1 and ctypes.sizeof(s.PObs) == 48 and s.PObs.p.offset == 8 and s.PObs.lon.offset == 16
    assert "type, bind(C) :: spdy_pobs" in support.fortran_binding()


def one(**kw):
    keys = (("var", lk.T), ("lev", lp.AT_P), ("lon", 10.0), ("lat", 5.0), ("value", 1.0), ("error", 1.0), ("p", 50000.0))
    return [[kw.get(k, dflt)] for k, dflt in keys]


def tables(lt):
    return {n: lt.table(n).copy() for n in TABLES}


def test_rejections_in_order(hosts):
    """spdy_pobs_set on a host-only plan: a NULL object, nobs outside [0, max_obs], NULL observations, then the first invalid field
    in the order var, lev, p, lon, lat, value, error, each with its text; lev == -1 of a PS observation and p of a model-level one
    are ignored; kx == 1 refuses an at-pressure observation; a rejected call changes no table"""
    s, get = hosts
    sp, g = get(5)
    lib = sp.lib
    lt = s.Letkf(sp, 3, 4, 5e5)
    good = ([lk.T, lk.PS, lk.U], [lp.AT_P, lp.AT_P, 2], [10.0, 20.0, 30.0], [5.0, -5.0, 0.0], [1.0, 2.0, 3.0], [1.0, 0.5, 2.0],
            [50000.0, float("nan"), -1.0])                   # PS: lev and p ignored; model level: p ignored
    lt.set_obs(*good)
    kept = tables(lt)
    assert np.array_equal(kept["lnp"], [math.log(50000.0 / P0), 0.0, 0.0])
    assert np.array_equal(kept["lnsigma"], [math.log(50000.0 / P0), 0.0, math.log(float(sp.table("fsg")[2]))])
    assert np.array_equal(kept["rinv"], 1.0 / np.square([1.0, 0.5, 2.0]))
    last = lambda: lib.spdy_last_error()
    assert lib.spdy_pobs_set(None, 0, None) == ERR_ARG and b"null analysis object" in last()
    obs = (s.PObs * 5)()
    assert lib.spdy_pobs_set(lt.h, 5, ctypes.cast(obs, ctypes.c_void_p)) == ERR_ARG and b"pobs_set: nobs=5 outside [0, max_obs=4]" in last()
    assert lib.spdy_pobs_set(lt.h, -1, None) == ERR_ARG and b"nobs=-1" in last()
    assert lib.spdy_pobs_set(lt.h, 2, None) == ERR_ARG and b"null observations" in last()
    nan, inf = float("nan"), float("inf")
    # each case is invalid in its field and in every later one it names: the first one must answer
    for bad, text in ((dict(var=5, lev=9, p=-1.0), b"var=5"), (dict(var=-1, p=nan), b"var=-1"),
                      (dict(lev=5, p=-1.0, lon=inf), b"lev=5 outside [0, 5)"), (dict(lev=-2, p=nan), b"lev=-2"),
                      (dict(p=0.0, lon=inf), b"p must be finite and > 0"), (dict(p=-3.0, lat=91.0), b"p must be"),
                      (dict(p=nan, value=nan), b"p must be"), (dict(p=inf, error=0.0), b"p must be"),
                      (dict(lon=inf, lat=nan), b"lon is not finite"), (dict(lat=90.5, value=nan), b"lat outside"),
                      (dict(value=nan, error=0.0), b"value is not finite"), (dict(error=0.0), b"error must be"),
                      (dict(error=inf), b"error must be"), (dict(var=lk.PS, lev=lp.AT_P, p=nan, error=-1.0), b"error must be")):
        assert code(s, lt.set_obs, *one(**bad)) == ERR_ARG, bad
        assert b"pobs_set: observation 0: " in last() and text in last(), (bad, last())
    # the first invalid observation answers, not a later one
    two = [a + b for a, b in zip(one(), one(p=-1.0))]
    assert code(s, lt.set_obs, *two) == ERR_ARG and b"observation 1: p must be" in last()
    with pytest.raises(ValueError):
        lt.set_obs(*[a * 5 for a in one()])
    with pytest.raises(ValueError):
        lt.set_obs([lk.T], [0], [0.0], [0.0], [0.0], [1.0], p=[1.0, 2.0])
    now = tables(lt)
    assert lt.nobs == 3 and all(np.array_equal(now[n], kept[n]) for n in TABLES)
    lt.close()
    # one level: no bracket exists
    flat = s.Spectral("t30", kx=1, max_batch=8, device=-1)
    flat.set_sigma([0.0, 1.0])
    l1 = s.Letkf(flat, 2, 2, 5e5)
    assert code(s, l1.set_obs, *one()) == ERR_ARG and b"needs kx >= 2" in flat.lib.spdy_last_error()
    l1.set_obs(*one(lev=0))
    assert np.array_equal(l1.table("lnp"), [0.0])
    l1.close()
    flat.close()


def test_a_set_without_pressures_is_set_obs(hosts):
    """the tables of spdy_pobs_set without an at-pressure entry equal spdy_letkf_set_obs'; "lnp" is zeros there and empty after
    set_obs; a mixed set has ln(p/p0) in "lnsigma" and "lnp" and the stencils of the same places"""
    s, get = hosts
    sp, g = get(8)
    x = lk.ensemble(g, 2, seed=3)
    plain = lk.edge_obs(g, x)
    n = len(plain["var"])
    a, b = s.Letkf(sp, 2, n, 5e5), s.Letkf(sp, 2, n, 5e5)
    a.set_obs(*lk.args(plain))
    b.set_obs(*lk.args(plain), p=np.full(n, np.nan))
    for name in TABLES[:-1]:
        assert support.same_bits(a.table(name), b.table(name)), name
    assert a.table("lnp").shape == (0,) and np.array_equal(b.table("lnp"), np.zeros(n))
    mixed = dict(plain, p=np.linspace(20000.0, 90000.0, n), lev=np.where(np.arange(n) % 2 == 0, lp.AT_P, plain["lev"]))
    b.set_obs(*lp.args(mixed))
    atp = lp.at_pressure(mixed)
    assert atp.any() and (~atp).any() and (mixed["var"][np.arange(n) % 2 == 0] == lk.PS).any()
    assert np.array_equal(b.table("lnp"), lp.lnp(mixed)) and (b.table("lnp")[atp] != 0.0).all()
    assert np.array_equal(b.table("lnsigma"), np.where(atp, lp.lnp(mixed), a.table("lnsigma")))
    for name in ("stencil_index", "stencil_weight", "unit", "rinv"):
        assert support.same_bits(a.table(name), b.table(name)), name
    b.set_obs(*lk.args(plain))
    assert b.table("lnp").shape == (0,) and support.same_bits(a.table("lnsigma"), b.table("lnsigma"))
    # the device-side names exist and need a device
    for name in ("obs_lnsigma", "obs_used"):
        assert code(s, b.field, name) == ERR_NO_DEVICE
    a.close()
    b.close()


def test_lifetime_rule(hosts):
    """spdy_pobs_set on an analysis object whose plan has been destroyed: SPDY_ERR_STATE, and the text names the plan"""
    s, _ = hosts
    sp = _plan(5, 2)
    lt = s.Letkf(sp, 2, 2, 5e5)
    lt.set_obs(*one())
    obs = (s.PObs * 1)(s.PObs(lk.T, lp.AT_P, 50000.0, 10.0, 5.0, 1.0, 1.0))
    h = lt.h
    sp.close()
    assert sp.lib.spdy_pobs_set(h, 1, ctypes.cast(obs, ctypes.c_void_p)) == ERR_STATE
    assert b"has been destroyed" in sp.lib.spdy_last_error() and b"analysis object" in sp.lib.spdy_last_error()
    assert sp.lib.spdy_pobs_set(h, 0, None) == ERR_STATE
    lt.close()


@pytest.mark.parametrize("E", [3, 32])
def test_spectral_inputs_keep_clear_of_the_end_levels(E, hosts, oracle_factory):
    """the inputs of tests/test_gpu_letkf_pressure.py's analysis from spectra: no target of an at-pressure observation lies within
    1e-9 of the first or the last level of any member at any of its four points, so a device whose grids differ from the oracle's
    by 1e-12 decides in column or out exactly as the restatement does; both kinds occur"""
    _, get = hosts
    sp, g = get(5)
    sts, x, net = lp.spectral_case(sp, oracle_factory("t30k5"), g, E)
    m = lp.margin(g, x, net)
    used = lk.obs_space(g, x, net)["obs_used"]
    print("[pobs spectral inputs E=%d] margin %.3e, %d of %d used" % (E, m, int(used.sum()), len(used)))
    assert m >= lp.MARGIN and lp.at_pressure(net).all() and 0.2 * len(used) <= used.sum() <= 0.9 * len(used)


def test_twin_condition_on_the_restatement():
    """One analysis of the twin set-up with a radiosonde-like network at pressures, on the restatement: the rmse of the analysis
    mean of u, v and t is below the background's at both levels, which bracket the pressures in column.  Three of a station's seven
    pressures are in column at kx = 2, the others are rejected.  tests/test_gpu_letkf_pressure.py asserts the same on the device."""
    s = support.package()
    c = nt.TWIN
    sp = s.Spectral("t30", kx=c["kx"], max_batch=64, device=-1)
    sp.set_sigma(nt.twin_sigma(c["kx"]))
    g, w = lp.Geometry(sp), nt.gaussian_weights(sp)
    truth, x, net = lp.twin_inputs(g)
    h = lp.truth_values(g, truth, net)
    net["value"] = h + net["error"] * np.random.default_rng(lp.TWIN_VALUE_SEED).standard_normal(len(h))
    used = lk.obs_space(g, x, net)["obs_used"]
    assert used.sum() == 3 * 3 * lp.TWIN_STATIONS and len(h) == 7 * 3 * lp.TWIN_STATIONS
    C, b = lk.problems(g, net, lk.obs_space(g, x, net), c["sigma_h"], c["sigma_v"])
    inc, _ = lk.increments(g, x, C, b, c["rho"])
    ratios = lp.twin_ratios(g, x, inc, truth, w)
    print("[pobs twin, restatement] rmse analysis / background: %s" % " ".join("%s %s" % (v, np.round(r, 3)) for v, r in ratios.items()))
    assert all((r < 1.0).all() for r in ratios.values()), ratios
    sp.close()
