"""CPU: the weight interpolation of the ensemble analysis without a device (include/spdy.h "ensemble analysis", weight
interpolation).  The library's tables on a host-only plan against the NumPy restatement (tests/letkfinterp.py), the argument checks
of spdy_letkf_set_weight_stride and their order, and what the restatement itself states: stride (1, 1) is the analysis, a coarse
column gets the full analysis, no observation and rho = 1 give exact zeros."""
import ctypes

import numpy as np
import pytest

import letkf as lk
import letkfinterp as li
import support

ERR_ARG, ERR_NO_DEVICE, ERR_STATE = -1, -3, -5
STRIDES = [(2, 2), (3, 5), (4, 47), (1, 3), (48, 1)]
TABLES = ("coarse_columns", "interp_index", "interp_weight")


@pytest.fixture(scope="module")
def host():
    s = support.package()
    sp = support.plan("t30k5", 3 * 11, device=-1)
    yield s, sp, lk.Geometry(sp)
    sp.close()


def code(s, fn, *a):
    with pytest.raises(s.SpdyError) as err:
        fn(*a)
    return err.value.code


# ---------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("si,sj", STRIDES)
def test_tables_against_the_restatement(si, sj, host):
    """T30 (ix = 96, il = 48): (2, 2) has rows 46 and 47 both coarse, (3, 5) the short last interval 45..47, (4, 47) the rows 0 and
    47 only, (48, 1) the largest si.  The coarse list and the stencil indices are equal; the weights are the same expressions of
    small integers, held to 2 eps; they are non-negative, sum to 1 within 2 eps, and are exactly (1, 0, 0, 0) at a coarse column"""
    s, sp, g = host
    lt = s.Letkf(sp, 3, 0, 5e5, weight_stride=(si, sj))
    assert lt.weight_stride == (si, sj)
    coarse, idx, wgt = (lt.table(n) for n in TABLES)
    rows = li.coarse_rows(g, sj)
    assert rows[0] == 0 and rows[-1] == g.il - 1 and np.all(np.diff(rows)[:-1] == sj) and 1 <= np.diff(rows)[-1] <= sj
    want = li.coarse_columns(g, si, sj)
    assert len(want) == len(rows) * (g.ix // si) and np.all(np.diff(want) > 0)
    assert coarse.dtype == np.int64 and np.array_equal(coarse, want)
    ridx, rwgt = li.stencils(g, si, sj)
    assert idx.shape == (g.ix * g.il, 4) and wgt.shape == (g.ix * g.il, 4)
    assert np.array_equal(idx, ridx) and idx.min() >= 0 and idx.max() < len(coarse)
    assert np.max(np.abs(wgt - rwgt)) <= 2 * lk.EPS
    assert wgt.min() >= 0.0 and np.max(np.abs(wgt.sum(axis=1) - 1.0)) <= 2 * lk.EPS
    assert np.array_equal(wgt[coarse], np.tile([1.0, 0.0, 0.0, 0.0], (len(coarse), 1)))
    assert np.array_equal(coarse[idx[coarse, 0]], coarse)                       # a coarse column's first entry is itself
    assert np.array_equal(idx[wgt == 0.0], np.broadcast_to(idx[:, :1], idx.shape)[wgt == 0.0])
    # the stencil of every column encloses it: the points' indices interpolate to the column's own (the wrap taken out)
    jj, ii = np.divmod(np.arange(g.ix * g.il), g.ix)
    pj, pi = np.divmod(coarse[idx], g.ix)
    pi = np.where(pi < ii[:, None], pi + g.ix * (pi + si <= ii[:, None]), pi)
    assert np.max(np.abs((wgt * pj).sum(axis=1) - jj)) <= 1e-12 and np.max(np.abs((wgt * pi).sum(axis=1) - ii)) <= 1e-12
    lt.close()


def test_stride_one_has_no_tables(host):
    """the default and an explicit (1, 1): all three tables have count 0, also after another stride"""
    s, sp, g = host
    lt = s.Letkf(sp, 3, 0, 5e5)
    assert lt.weight_stride == (1, 1)
    for n in TABLES:
        assert lt.table(n).size == 0
    lt.set_weight_stride(3, 5)
    assert lt.table("interp_weight").shape == (g.ix * g.il, 4)
    lt.set_weight_stride(1, 1)
    for n in TABLES:
        assert sp.lib.spdy_letkf_table(lt.h, n.encode(), None, 0) == 0
    lt.close()


# ---------------------------------------------------------------------------------------------------- the checks
def test_stride_checks(host):
    """a NULL object, then an invalid stride (si not dividing ix, si > ix/2, si < 1, sj = 0, sj = il) SPDY_ERR_ARG; a rejected stride
    changes nothing; "weights" is SPDY_ERR_STATE at stride (1, 1), after the name check and before the device check"""
    s, sp, g = host
    lib = sp.lib
    assert lib.spdy_letkf_set_weight_stride(None, 0, 0) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    lt = s.Letkf(sp, 3, 0, 5e5)
    for bad in ((5, 1), (7, 2), (96, 1), (g.ix // 2 + 1, 1), (0, 1), (-2, 1)):
        assert code(s, lt.set_weight_stride, *bad) == ERR_ARG and b"si=" in lib.spdy_last_error(), bad
    for bad in ((2, 0), (2, g.il), (2, -1), (1, 0)):
        assert code(s, lt.set_weight_stride, *bad) == ERR_ARG and b"sj=" in lib.spdy_last_error(), bad
    assert code(s, lt.set_weight_stride, 5, 0) == ERR_ARG and b"si=" in lib.spdy_last_error()       # si is looked at first
    assert lt.weight_stride == (1, 1)
    lt.set_weight_stride(1, 1)
    for n in TABLES:
        assert lt.table(n).size == 0
    lt.set_weight_stride(2, 2)
    kept = [lt.table(n).copy() for n in TABLES]
    assert code(s, lt.set_weight_stride, 5, 2) == ERR_ARG and code(s, lt.set_weight_stride, 2, g.il) == ERR_ARG
    assert lt.weight_stride == (2, 2) and all(np.array_equal(lt.table(n), k) for n, k in zip(TABLES, kept))
    d = ctypes.c_void_p()
    assert lib.spdy_letkf_field(lt.h, b"nothing", ctypes.byref(d)) == ERR_ARG
    assert lib.spdy_letkf_field(lt.h, b"weights", None) == ERR_ARG
    assert lib.spdy_letkf_field(lt.h, b"weights", ctypes.byref(d)) == ERR_NO_DEVICE
    lt.set_weight_stride(1, 1)
    assert lib.spdy_letkf_field(lt.h, b"weights", ctypes.byref(d)) == ERR_STATE
    assert lib.spdy_letkf_field(lt.h, b"hx", ctypes.byref(d)) == ERR_NO_DEVICE
    buf = np.zeros(3)
    lt.set_weight_stride(48, 1)
    assert lib.spdy_letkf_table(lt.h, b"coarse_columns", buf.ctypes.data_as(ctypes.c_void_p), 3) == ERR_ARG
    assert lib.spdy_letkf_table(lt.h, b"coarse_columns", None, 0) == 2 * g.il
    lt.close()
    with pytest.raises(s.SpdyError):
        s.Letkf(sp, 3, 0, 5e5, weight_stride=(5, 1))


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def case(host):
    _, _, g = host
    x = lk.ensemble(g, 3, seed=3)
    return g, x, lk.sparse_obs(g, x)


def same(a, b):
    return all(a[v].shape == b[v].shape and np.array_equal(a[v], b[v]) for v in lk.VARS)


def test_stride_one_is_the_analysis(case):
    """at stride (1, 1) every column is coarse, its stencil is (1, 0, 0, 0) on itself, and the increments are lk.analyse's"""
    g, x, obs = case
    cols = lk.columns_for(g, obs, 5e5, most=12, outside=4)
    idx, wgt = li.stencils(g, 1, 1)
    assert np.array_equal(li.coarse_columns(g, 1, 1), np.arange(g.ix * g.il))
    assert np.array_equal(idx, np.repeat(np.arange(g.ix * g.il)[:, None], 4, axis=1)) and np.array_equal(wgt[:, 0], np.ones(g.ix * g.il))
    got, entries, _ = li.analyse(g, x, obs, 5e5, 0.1, 1.1, 1, 1, cols=np.sort(cols), tables=(idx, wgt))
    assert np.array_equal(entries, np.sort(cols))
    assert same(got, lk.analyse(g, x, obs, 5e5, 0.1, 1.1, cols=np.sort(cols))[0])


@pytest.mark.parametrize("si,sj", [(2, 2), (3, 5), (4, 47)])
def test_coarse_columns_get_the_full_analysis(si, sj, case):
    """at any stride the increments at coarse columns equal the full analysis there; at the other columns they differ from it"""
    g, x, obs = case
    near = np.nonzero(lk.distance(g.colunit, lk.unit(obs["lon"], obs["lat"])).min(axis=1) < 1.5e6)[0]    # inside the range, 1.83e6 m
    coarse = li.coarse_columns(g, si, sj)
    cols = np.intersect1d(near, coarse)[:16]
    assert len(cols) >= 2
    got, _, _ = li.analyse(g, x, obs, 5e5, 0.1, 1.1, si, sj, cols=cols)
    full = lk.analyse(g, x, obs, 5e5, 0.1, 1.1, cols=cols)[0]
    assert same(got, full) and any(full[v].any() for v in lk.VARS)
    fine = np.setdiff1d(near, coarse)[:16]
    got, _, _ = li.analyse(g, x, obs, 5e5, 0.1, 1.1, si, sj, cols=fine)
    assert not same(got, lk.analyse(g, x, obs, 5e5, 0.1, 1.1, cols=fine)[0])


def test_no_observation_is_exactly_zero(case):
    """no observation and rho = 1: every T is exactly zero and so is every increment, at every stencil class"""
    g, x, _ = case
    none = lk.make_obs([], [], [], [], [], [])
    cols = np.array([0, 1, g.ix, g.ix + 1, 7 * g.ix + 95, 46 * g.ix + 50, 47 * g.ix + 95])
    for route in ("eigh", "jacobi"):
        got, _, Tc = li.analyse(g, x, none, 5e5, 0.1, 1.0, 3, 5, route=route, cols=cols)
        assert not Tc.any() and not any(got[v].any() for v in lk.VARS)
