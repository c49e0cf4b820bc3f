"""CPU: adaptive inflation without a device (include/spdy.h, "adaptive inflation").  The library on a host-only
plan: the checks of spdy_infl_set and spdy_infl_fill in the documented order, a rejected call changing nothing, the stored values,
the binding surface.  Then the NumPy restatement (tests/letkfinfl.py) against closed forms: one observation on a grid point, the
update's branches, and synthetic departures of a known inflation."""
import ctypes
import math

import numpy as np
import pytest

import letkf as lk
import letkfinfl as li
import support

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5


@pytest.fixture(scope="module")
def host():
    """T30 L8 without a device and an analysis object of three members with four observations on it"""
    s = support.package()
    sp = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    lt = s.Letkf(sp, 3, 4, 1.0e6)
    lt.set_obs([0, 1, 2, 4], [0, 1, 2, 0], [10.0, 20.0, 30.0, 40.0], [0.0, 10.0, 20.0, 30.0], [1.0] * 4, [1.0] * 4)
    yield s, sp, lt, lk.Geometry(sp)
    lt.close()
    sp.close()


# ---------------------------------------------------------------------------------------------------- the library, host-only
def test_infl_set_checks_in_order_and_stores(host):
    """a NULL object, a destroyed plan, sigma_b, rho_min, rho_max -- each call is given everything that is wrong after the check
    under test as well and reports the first; a rejected call changes nothing; a good setting is stored, on and off"""
    s, sp, lt, _ = host
    lib = s.load()
    call = lib.spdy_infl_set
    stored = lambda: tuple(lt.table("adaptive_inflation"))
    assert stored() == (0.0, 0.0, 0.0, 0.0) and lt.adaptive is None                   # off is the state after create
    assert call(None, 1, -1.0, -1.0, -1.0) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    lt.set_adaptive_inflation(0.05, 0.8, 2.5)
    assert stored() == (1.0, 0.05, 0.8, 2.5) and lt.adaptive == (0.05, 0.8, 2.5)
    for bad in (math.nan, -0.1, math.inf):
        assert call(lt.h, 1, bad, -1.0, -1.0) == ERR_ARG and b"sigma_b must be finite and >= 0" in lib.spdy_last_error(), bad
    for bad in (math.nan, 0.0, -1.0, math.inf):
        assert call(lt.h, 1, 0.04, bad, -1.0) == ERR_ARG and b"rho_min must be finite and > 0" in lib.spdy_last_error(), bad
    for bad in (math.nan, 0.5, math.inf):
        assert call(lt.h, 1, 0.04, 0.9, bad) == ERR_ARG and b"rho_max must be finite and >= rho_min" in lib.spdy_last_error(), bad
    with pytest.raises(s.SpdyError):
        lt.set_adaptive_inflation(rho_min=2.0, rho_max=1.0)
    assert stored() == (1.0, 0.05, 0.8, 2.5) and lt.adaptive == (0.05, 0.8, 2.5)
    lt.set_adaptive_inflation(0.0, 1.0, 1.0)                                           # sigma_b = 0 and rho_min == rho_max are legal
    assert stored() == (1.0, 0.0, 1.0, 1.0)
    lt.set_adaptive_inflation(on=False)
    assert stored() == (0.0, li.SIGMA_B, li.RHO_MIN, li.RHO_MAX) and lt.adaptive is None
    gone = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    dead = s.Letkf(gone, 3, 4, 1.0e6, adaptive={"sigma_b": 0.1})
    assert dead.adaptive == (0.1, li.RHO_MIN, li.RHO_MAX) and tuple(dead.table("adaptive_inflation"))[:2] == (1.0, 0.1)
    gone.close()
    assert call(dead.h, 1, -1.0, -1.0, -1.0) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    assert lib.spdy_infl_fill(dead.h, -1.0) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    dead.close()


def test_infl_fill_checks_in_order(host):
    s, sp, lt, _ = host
    lib = s.load()
    assert lib.spdy_infl_fill(None, -1.0) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    for bad in (math.nan, 0.0, -1.0, math.inf):
        assert lib.spdy_infl_fill(lt.h, bad) == ERR_ARG and b"rho0 must be finite and > 0" in lib.spdy_last_error(), bad
    assert lib.spdy_infl_fill(lt.h, 1.0) == ERR_NO_DEVICE and b"host-only plan" in lib.spdy_last_error()
    with pytest.raises(s.SpdyError):
        lt.fill_inflation(1.0)


def test_names_and_binding_surface(host):
    s, sp, lt, _ = host
    lib = s.load()
    p = ctypes.c_void_p()
    for name in (b"rho", b"infl_parm", b"obs_s2"):
        assert name.decode() in s.letkf.LETKF_FIELDS
        assert lib.spdy_letkf_field(lt.h, name, ctypes.byref(p)) == ERR_NO_DEVICE and b"host-only plan" in lib.spdy_last_error()
        assert not p.value
    assert "adaptive_inflation" in s.letkf.LETKF_TABLES
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name, sig, decl in (("spdy_infl_set", [P, I, D, D, D], "spdy_letkf *l, int on, double sigma_b, double rho_min, double rho_max"),
                            ("spdy_infl_fill", [P, D], "spdy_letkf *l, double rho0")):
        assert hasattr(lib, name) and name in support.declared() and name in support.fortran_bound(), name
        assert s._lib.SIGNATURES[name] == sig and support.declaration(name) == decl
    assert "real(c_double), value :: sigma_b, rho_min, rho_max" in support.fortran_binding()
    assert "adaptive inflation" in support.header(comments=True)
    assert s.Letkf.set_adaptive_inflation.__doc__ and s.Letkf.fill_inflation.__doc__ and s.Letkf.inflation_field.__doc__


# ---------------------------------------------------------------------------------------------------- the restatement
def test_one_observation_on_a_grid_point(host):
    """wh = gc(0) = 1, sigma_v = 0: p1 = dep^2 / err^2, p2 = s2 / err^2, p3 = 1 at every level of the observation's column, and the
    update's closed form there; a column out of range keeps zeros and rho's bits"""
    _, _, _, g = host
    i, j = 7, 11
    col = j * g.ix + i
    y = np.array([[2.0, -2.0, 0.0]])                         # s2 = 8 / 2 = 4
    dep, err = np.array([6.0]), np.array([2.0])
    s2o = li.s2(y)
    assert s2o[0] == 4.0
    far = ((j + 12) % g.il) * g.ix + (i + 48) % g.ix
    p = li.sums(g, lk.unit([g.lon[i]], [g.lat[j]]), [0.0], 1.0 / (err * err), dep, s2o, lk.SIGMA_H, 0.0, [col, far])
    assert (p[0, :, 0] == 9.0).all() and (p[1, :, 0] == 1.0).all() and (p[2, :, 0] == 1.0).all()
    assert not p[:, :, 1].view(np.int64).any()
    # ro = (9 - 1) / 1 = 8; t = (1 * 1 + 1) / 1 = 2; vo = (2 / 1) * 4 = 8; vb = 1: g = 1 / 9; rho' = 1 + (8 - 1) / 9
    rho = np.ones((g.kx, 2))
    new = li.update(rho, p, 1.0, 0.5, 5.0)
    assert (new[:, 0] == 1.0 + (1.0 / 9.0) * 7.0).all() and support.same_bits(new[:, 1], rho[:, 1])
    assert (li.observed(p)[:, 0] == 8.0).all() and np.isnan(li.observed(p)[:, 1]).all()
    # with sigma_v > 0 the observation (ln sigma_o = ln fsg of level 2) weighs 1 at its level and less elsewhere
    pv = li.sums(g, lk.unit([g.lon[i]], [g.lat[j]]), [g.lnfsg[2]], 1.0 / (err * err), dep, s2o, lk.SIGMA_H, 0.1, [col])
    assert pv[2, 2, 0] == 1.0 and (np.delete(pv[2, :, 0], 2) < 1.0).all() and pv[0, 2, 0] == 9.0


def test_update_branches():
    """both clamps, sigma_b = 0, p3 == 0, p2 == 0, and non-finite sums: everything but a finite estimate keeps rho's bits"""
    rho = np.array([1.0, 1.0, 1.25, 1.1, 1.1, 1.1, 1.1, 1.1])
    p1 = np.array([900.0, 0.0, 30.0, 5.0, 5.0, np.nan, np.inf, 5.0])
    p2 = np.array([1.0, 10.0, 10.0, 2.0, 0.0, 2.0, 2.0, np.nan])
    p3 = np.array([1.0, 10.0, 10.0, 0.0, 3.0, 3.0, 3.0, 3.0])
    new = li.update(rho, (p1, p2, p3), 10.0, 0.9, 3.0)
    assert new[0] == 3.0 and new[1] == 0.9 and 0.9 < new[2] < 3.0 and new[2] != rho[2]
    assert support.same_bits(new[3:], rho[3:])
    frozen = li.update(rho, (p1, p2, p3), 0.0, 0.9, 3.0)
    assert support.same_bits(frozen, rho)


N, SEED, ALPHA = 4000, 20251, 1.3


def test_synthetic_departures_recover_the_inflation(host):
    """N observations on one grid point (wh = 1), E = 8 members drawn with unit variance, err = 0.5; the departures are drawn with
    variance alpha s2_o + err^2, s2_o the members' own sample variance.  Then E[p1 - p3] = alpha p2 and ro estimates alpha; dep^2
    has the variance 2 v^2, so ro's sampling error is sqrt(2 / N) (alpha + err^2 / s2), s2 the mean of s2_o.  The assertion
    allows four of these (a margin for the spread of s2_o among the observations, which the formula leaves out)"""
    _, _, _, g = host
    rng = np.random.default_rng(SEED)
    E, err = 8, 0.5
    y = rng.standard_normal((N, E))
    y = y - y.mean(axis=1, keepdims=True)
    s2o = li.s2(y)
    dep = np.sqrt(ALPHA * s2o + err * err) * rng.standard_normal(N)
    i, j = 20, 30
    p = li.sums(g, np.repeat(lk.unit([g.lon[i]], [g.lat[j]]), N, axis=0), np.zeros(N), np.full(N, 1.0 / (err * err)), dep, s2o,
                lk.SIGMA_H, 0.0, [j * g.ix + i])
    assert p[2, 0, 0] == N
    ro = float(li.observed(p)[0, 0])
    sampling = math.sqrt(2.0 / N) * (ALPHA + err * err / float(s2o.mean()))
    print("[letkf infl] ro = %.4f for alpha = %.2f, sampling error %.4f" % (ro, ALPHA, sampling))
    assert abs(ro - ALPHA) <= 4.0 * sampling
    # and the update moves rho towards it, the farther the larger sigma_b
    steps = [float(li.update(np.ones((g.kx, 1)), p, sb, 0.5, 5.0)[0, 0]) for sb in (0.0, 0.01, 0.04, 1.0)]
    assert steps[0] == 1.0 and steps[0] < steps[1] < steps[2] < steps[3] < ro
