"""CPU: the relaxation of the analysis without a device (include/spdy.h, "relaxation").  The NumPy restatement
(tests/letkfrelax.py) on the analysis tests' inputs: the three statements the header calls exact, that rtps = 1 restores the
background spread and takes pure inflation back, and f = 1 where the relaxed spread is zero.  Then the library on a host-only
plan: spdy_relax_set's rejections, an accepted setting, the field name, and the binding surface."""
import ctypes
import math

import numpy as np
import pytest

import letkf as lk
import letkfrelax as lr
import support

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
SIZES = [3, 8, 32]
SIGMA_V = 0.1


@pytest.fixture(scope="module")
def host():
    """T30 L8 without a device and an analysis object of three members on it"""
    s = support.package()
    sp = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    lt = s.Letkf(sp, 3, 4, 1.0e6)
    yield s, sp, lt
    lt.close()
    sp.close()


@pytest.fixture(scope="module")
def geometry(host):
    return lk.Geometry(host[1])


@pytest.fixture(scope="module")
def inputs(geometry):
    """(E, set) -> (x and the NumPy analysis' raw increments at letkf.columns_for(most=32), which of those columns are out of range
    of every observation); computed once, never changed"""
    made = {}

    def get(E, name):
        if (E, name) not in made:
            g = geometry
            x = lk.ensemble(g, E, seed=E)
            obs = {"clustered": lk.clustered_obs, "sparse": lk.sparse_obs}[name](g, x)
            cols = lk.columns_for(g, obs, lk.SIGMA_H, most=32)
            dx, _ = lk.analyse(g, x, obs, lk.SIGMA_H, SIGMA_V, lk.RHO, cols=cols)
            out = ~lk.in_range(g, obs, cols).any(axis=1)
            assert out.sum() >= 8 and (~out).sum() >= 8, (out.sum(), (~out).sum())
            made[(E, name)] = (lr.at_columns(x, cols), dx, out)
        return made[(E, name)]
    return get


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["clustered", "sparse"])
@pytest.mark.parametrize("E", SIZES)
def test_untouched_items_stay_untouched(E, name, inputs):
    """raw increments that are all +0.0, what a column out of every observation's range has with rho = 1: every relaxed increment
    is +0.0 in every bit and f is exactly 1.0, whatever the setting; next to them the columns in range are relaxed"""
    x, dx, out = inputs(E, name)
    raw = {v: np.where(out, 0.0, dx[v]) for v in lk.VARS}
    for rtpp, rtps in lr.SETTINGS + ((1.0, 1.0), (0.0, 1.0)):
        got, f = lr.relax(x, raw, rtpp, rtps)
        for v in lk.VARS:
            assert not np.ascontiguousarray(got[v][..., out]).view(np.int64).any(), (rtpp, rtps, v)
            assert (f[v][..., out] == 1.0).all(), (rtpp, rtps, v)
            assert (got[v][..., ~out] != raw[v][..., ~out]).any(), (rtpp, rtps, v)


@pytest.mark.parametrize("name", ["clustered", "sparse"])
@pytest.mark.parametrize("E", SIZES)
def test_rtpp_one_moves_only_the_mean(E, name, inputs):
    """rtpp = 1: every member gets the same bits, the mean increment dm, and f is exactly 1.0"""
    x, dx, _ = inputs(E, name)
    for rtps in (0.0, 0.9, 1.0):
        got, f = lr.relax(x, dx, 1.0, rtps)
        for v in lk.VARS:
            assert lr.same_bits_everywhere(got[v]) and got[v].any(), (rtps, v)
            s = np.zeros(dx[v].shape[1:])
            for e in range(E):
                s = s + dx[v][e]
            assert support.same_bits(got[v][0], s / E + 0.0), (rtps, v)
            assert (f[v] == 1.0).all(), (rtps, v)


@pytest.mark.parametrize("E", SIZES)
def test_both_zero_is_the_analysis(E, inputs):
    """(0, 0): the increments come back with their bits"""
    x, dx, _ = inputs(E, "clustered")
    got, f = lr.relax(x, dx, 0.0, 0.0)
    for v in lk.VARS:
        assert support.same_bits(got[v], dx[v]) and (f[v] == 1.0).all(), v


@pytest.mark.parametrize("name", ["clustered", "sparse"])
@pytest.mark.parametrize("E", SIZES)
def test_rtps_one_restores_the_spread(E, name, inputs):
    """rtps = 1, with and without rtpp: the sample standard deviation of x + dx' is the background's sb.  The analysis
    perturbations are f a_e, and a_e carries the rounding of b_e, eps max|x|, times f: the bound is the increments' own, 64 E eps
    max|x| max(1, f), relative to sb"""
    x, dx, out = inputs(E, name)
    for rtpp in (0.0, 0.3):
        got, f = lr.relax(x, dx, rtpp, 1.0)
        plain, _ = lr.relax(x, dx, rtpp, 0.0)
        for v in lk.VARS:
            sb = lr.spread(x[v])
            s = np.std(x[v] + got[v], axis=0, ddof=1)
            assert (np.abs(s - sb) <= lr.limit(x, f, E, v)).all(), (rtpp, v, float(np.max(np.abs(s - sb) / lr.limit(x, f, E, v))))
            # and without rtps it is not: the analysis has drawn the ensemble together in range of the observations
            shrunk = np.std(x[v] + plain[v], axis=0, ddof=1)[..., ~out]
            assert (shrunk < 0.999 * sb[..., ~out]).any(), (rtpp, v)


@pytest.mark.parametrize("E", SIZES)
def test_rtps_one_takes_pure_inflation_back(E, geometry):
    """rho = 1.21 and no observation: the raw increments are 0.1 b_e; with rtps = 1 the relaxed ones are zero to the increments'
    bound (f = 1 / 1.1 < 1)"""
    g = geometry
    x = lk.ensemble(g, E, seed=E)
    cols = np.arange(0, g.ix * g.il, 97)
    none = lk.make_obs([], [], [], [], [], [])
    dx, _ = lk.analyse(g, x, none, lk.SIGMA_H, SIGMA_V, 1.21, cols=cols)
    xc = lr.at_columns(x, cols)
    got, f = lr.relax(xc, dx, 0.0, 1.0)
    for v in lk.VARS:
        assert np.max(np.abs(dx[v])) > 0.05 * np.max(np.abs(xc[v] - xc[v].mean(axis=0))), v
        assert np.max(np.abs(f[v] - 1.0 / 1.1)) <= 64 * E * lk.EPS, v
        assert (np.abs(got[v]) <= lr.limit(xc, f, E, v)[None]).all(), (v, float(np.max(np.abs(got[v]))))


def test_zero_relaxed_spread_gives_factor_one():
    """sa == 0 -- members that are equal and get equal increments, or increments that cancel the perturbations exactly -- gives f
    = 1, not a division by zero: dx' = dm in the first case, dm - b_e in the second"""
    x = np.full((4, 3), 250.0)
    dx = np.full((4, 3), 0.5)
    for rtpp, rtps in lr.SETTINGS + ((0.0, 1.0),):
        got, f = lr.relax_array(x, dx, rtpp, rtps)
        assert (f == 1.0).all() and support.same_bits(got, dx), (rtpp, rtps)
    x = np.array([1.0, 2.0, 3.0])[:, None]
    dx = np.array([1.5, 0.5, -0.5])[:, None]
    got, f = lr.relax_array(x, dx, 0.0, 0.9)
    assert (f == 1.0).all() and (x + got == 2.5).all()


def test_members_not_in_use():
    """a member not in use gets 0.0 and is not read: NaN there changes no bit; the others get what the compacted ensemble gets;
    fewer than two in use: all zero and f = 1"""
    rng = np.random.default_rng(4)
    x, dx = 250.0 + rng.standard_normal((5, 7)), rng.standard_normal((5, 7))
    keep = (0, 2, 3)
    got, f = lr.relax_array(x, dx, 0.3, 0.9, keep)
    ref, fr = lr.relax_array(x[list(keep)], dx[list(keep)], 0.3, 0.9)
    assert support.same_bits(np.ascontiguousarray(got[list(keep)]), ref) and support.same_bits(f, fr)
    assert not got[[1, 4]].view(np.int64).any()
    y, dy = x.copy(), dx.copy()
    y[[1, 4]] = dy[[1, 4]] = np.nan
    again, fa = lr.relax_array(y, dy, 0.3, 0.9, keep)
    assert support.same_bits(again, got) and support.same_bits(fa, f)
    for few in ((2,), ()):
        got, f = lr.relax_array(x, dx, 0.3, 0.9, few)
        assert not got.view(np.int64).any() and (f == 1.0).all()


# ---------------------------------------------------------------------------------------------------- the library, host-only
def test_set_relaxation_rejects_and_accepts(host):
    """NaN, -0.1 and 1.5 (and an infinity) in either argument alone: SPDY_ERR_ARG, and the setting does not change; a good
    setting is stored on a host-only plan, where nothing is allocated"""
    s, sp, lt = host
    lib = s.load()
    call = lib.spdy_relax_set
    assert call(None, 0.5, 0.5) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    lt.set_relaxation(0.25, 0.75)
    assert lt.relaxation == (0.25, 0.75)
    for bad in (math.nan, -0.1, 1.5, math.inf):
        assert call(lt.h, bad, 0.5) == ERR_ARG and b"rtpp must lie in [0, 1]" in lib.spdy_last_error(), bad
        assert call(lt.h, 0.5, bad) == ERR_ARG and b"rtps must lie in [0, 1]" in lib.spdy_last_error(), bad
        with pytest.raises(s.SpdyError):
            lt.set_relaxation(rtps=bad)
        assert lt.relaxation == (0.25, 0.75)
    for good in ((0.0, 0.0), (1.0, 1.0), (0.0, 0.9), (0.5, 0.0)):
        lt.set_relaxation(*good)
        assert lt.relaxation == good
    lt.set_relaxation()
    assert lt.relaxation == (0.0, 0.0)
    gone = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    dead = s.Letkf(gone, 3, 4, 1.0e6, rtpp=0.5, rtps=0.5)
    assert dead.relaxation == (0.5, 0.5)
    gone.close()
    assert call(dead.h, 0.5, 0.5) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    dead.close()


def test_inflation_is_a_field_name(host):
    s, sp, lt = host
    lib = s.load()
    assert "inflation" in s.letkf.LETKF_FIELDS
    p = ctypes.c_void_p()
    assert lib.spdy_letkf_field(lt.h, b"inflation", ctypes.byref(p)) == ERR_NO_DEVICE and b"host-only plan" in lib.spdy_last_error()
    assert not p.value


def test_entry_point_exists_and_is_bound(host):
    s, sp, lt = host
    name = "spdy_relax_set"
    assert hasattr(s.load(), name) and name in support.declared() and name in support.fortran_bound()
    assert s._lib.SIGNATURES[name] == [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    assert support.declaration(name) == "spdy_letkf *l, double rtpp, double rtps"
    assert "real(c_double), value :: rtpp, rtps" in support.fortran_binding()
    assert s.Letkf.set_relaxation.__doc__ and "relaxation" in support.header(comments=True)
