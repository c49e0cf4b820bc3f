"""CPU: the ensemble analysis without a device (include/spdy.h "ensemble analysis").  The NumPy restatement (tests/letkf.py) against
the closed forms of one observation, its own properties and its two eigen routes; then the library on a host-only plan: argument
checks and their order, the observation ingestion against the restatement, SPDY_ERR_NO_DEVICE from the device calls, and the
shape errors of Letkf and Ensemble.analyse."""
import ctypes

import numpy as np
import pytest

import letkf as lk
import support

SIZES = [2, 3, 17, 32]
ERR_ARG, ERR_NO_DEVICE, ERR_STATE = -1, -3, -5


def one_observation(E, w, err, rho, seed):
    rng = np.random.default_rng(seed)
    x = 250.0 + 3.0 * rng.standard_normal(E)            # the observed variable at the observation's place
    s = 0.0
    for v in x:
        s = s + v
    Y = x - s / E
    d = 1.7
    r = np.array([w / (err * err)])
    C, b = lk.local_problem(Y[None, :], np.array([d]), r)
    return x, Y, d, C, b


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("route", ["eigh", "jacobi"])
@pytest.mark.parametrize("E", SIZES)
def test_closed_forms(E, route):
    """one observation of weight w on the observed variable: the mean increment is d g / (err^2 + g) with g = rho w s^2 and the
    analysed sample variance rho s^2 err^2 / (err^2 + g); to 2e-15 of the field scale max|x| (for the variance: times max|x - mean|)"""
    for w, err, rho in ((1.0, 0.8, 1.0), (0.37, 2.0, 1.1), (1e-3, 0.5, 1.21)):
        x, Y, d, C, b = one_observation(E, w, err, rho, seed=E)
        T = lk.transform(C[None], b[None], E, rho, route)[0][0]
        inc = Y @ T
        s2 = float(Y @ Y) / (E - 1)
        g = rho * w * s2
        scale = float(np.max(np.abs(x)))
        assert abs(inc.mean() - d * g / (err * err + g)) <= 2e-15 * scale, (w, err, rho)
        assert abs((Y + inc).var(ddof=1) - rho * s2 * err * err / (err * err + g)) <= 2e-15 * scale * np.max(np.abs(Y)), (w, err, rho)


@pytest.mark.parametrize("route", ["eigh", "jacobi"])
@pytest.mark.parametrize("E", SIZES)
def test_properties(E, route):
    """W is symmetric and W 1 = sqrt(rho) 1 (rho = 1: W 1 = 1); the perturbation increments sum to zero; w = 0 with rho = 1 gives
    increments exactly 0.0"""
    rng = np.random.default_rng(100 + E)
    Y = rng.standard_normal((3 * E, E))
    Y -= Y.mean(axis=1, keepdims=True)
    d, r = rng.standard_normal(3 * E), rng.uniform(0.1, 2.0, 3 * E)
    C, b = lk.local_problem(Y, d, r)
    for rho in (1.0, 1.1):
        T, W, wbar, _ = (a[0] for a in lk.transform(C[None], b[None], E, rho, route))
        assert np.max(np.abs(W - W.T)) <= 8 * E * lk.EPS
        assert np.max(np.abs(W @ np.ones(E) - np.sqrt(rho))) <= 8 * E * lk.EPS
    xp = rng.standard_normal(E)
    xp -= xp.mean()
    assert abs(float((xp @ (W - np.eye(E))).sum())) <= 8 * E * lk.EPS * np.max(np.abs(xp))
    C0, b0 = lk.local_problem(Y, d, np.zeros(3 * E))
    T0 = lk.transform(C0[None], b0[None], E, 1.0, route)[0][0]
    assert not T0.any() and not (xp @ T0).any()


@pytest.mark.parametrize("E", SIZES)
def test_routes_agree(E):
    """eigh and the cyclic Jacobi on the same problems, kappa(A) from 1e2 to 1e10: increments within 1.3e-14 of the field scale"""
    rng = np.random.default_rng(200 + E)
    m, rho = 3 * E, 1.1
    for target in (1e2, 1e6, 1e10):
        Y = rng.standard_normal((m, E))
        Y -= Y.mean(axis=1, keepdims=True)
        d = rng.standard_normal(m)
        C1, _ = lk.local_problem(Y, d, np.ones(m))
        r = np.full(m, (target - 1.0) * ((E - 1) / rho) / np.linalg.eigvalsh(C1)[-1])
        C, b = lk.local_problem(Y, d, r)
        Te, _, _, lam = lk.transform(C[None], b[None], E, rho, "eigh")
        Tj = lk.transform(C[None], b[None], E, rho, "jacobi")[0]
        kappa = float(lam.max() / lam.min())
        assert 0.5 * target <= kappa <= 2.0 * target
        xp = rng.standard_normal((4, E))
        xp -= xp.mean(axis=1, keepdims=True)
        diff = float(np.max(np.abs(xp @ Te[0] - xp @ Tj[0])))
        print("[letkf routes E=%d kappa=%.1e] %.2e of the field scale" % (E, kappa, diff / np.max(np.abs(xp))))
        assert diff <= 1.3e-14 * np.max(np.abs(xp)), (target, diff)


def test_jacobi_is_an_eigensolver():
    rng = np.random.default_rng(7)
    for n in (2, 3, 17, 32):
        B = rng.standard_normal((5, n, n))
        A = B @ np.swapaxes(B, 1, 2) + n * np.eye(n)
        lam, V = lk.jacobi(A)
        assert np.max(np.abs(np.einsum("nfi,ni,nei->nfe", V, lam, V) - A)) <= 64 * n * lk.EPS * np.max(np.abs(A))
        assert np.max(np.abs(np.sort(lam, axis=1) - np.linalg.eigvalsh(A))) <= 64 * n * lk.EPS * np.max(np.abs(A))


def test_gaspari_cohn():
    assert lk.gc(0.0) == 1.0 and lk.gc(2.0) == 0.0 and lk.gc(3.0) == 0.0
    r = np.linspace(0.0, 2.0, 4001)
    v = lk.gc(r)
    assert (v >= 0.0).all() and (np.diff(v) <= 1e-15).all()
    assert abs(lk.gc(1.0) - 5.0 / 24.0) <= 4 * lk.EPS and abs(lk.gc(np.nextafter(1.0, 2.0)) - 5.0 / 24.0) <= 1e-14
    outer = np.linspace(1.0, 2.0, 1001)[1:-1]
    assert np.max(np.abs(lk.gc(outer) - lk.gc_powers(outer))) <= 64 * lk.EPS       # the factored outer branch is eq. 4.10


# ---------------------------------------------------------------------------------------------------- a host-only plan
@pytest.fixture(scope="module")
def host():
    s = support.package()
    sp = support.plan("t30k5", 32 * 11, device=-1)
    yield s, sp, lk.Geometry(sp)
    sp.close()


def code(s, fn, *a):
    with pytest.raises(s.SpdyError) as err:
        fn(*a)
    return err.value.code


def test_create_checks(host):
    """create: a NULL plan, nmem outside [2, 32], max_obs < 0, a NULL result pointer, max_batch, the LDS size SPDY_ERR_ARG, in this order; a plan
    without sigma levels SPDY_ERR_STATE"""
    s, sp, _ = host
    lib, h = sp.lib, ctypes.c_void_p()
    assert lib.spdy_letkf_create(None, 1, -1, None) == ERR_ARG and b"null plan" in lib.spdy_last_error()
    for nmem in (1, 33, 0, -4):
        assert lib.spdy_letkf_create(sp.h, nmem, -1, None) == ERR_ARG and b"nmem" in lib.spdy_last_error()
    assert lib.spdy_letkf_create(sp.h, 2, -1, None) == ERR_ARG and b"max_obs" in lib.spdy_last_error()
    assert lib.spdy_letkf_create(sp.h, 2, 0, None) == ERR_ARG and b"null result" in lib.spdy_last_error()
    small = support.plan("t30k5", 2 * 11 - 1, device=-1)
    assert lib.spdy_letkf_create(small.h, 2, 0, ctypes.byref(h)) == ERR_ARG and b"max_batch" in lib.spdy_last_error()
    small.close()
    tall = s.Spectral("t30", kx=17, max_batch=32 * 35, device=-1)      # E = 32 at kx = 17: more LDS than a compute unit has
    tall.set_sigma(np.linspace(0.0, 1.0, 18))
    assert lib.spdy_letkf_create(tall.h, 32, 0, ctypes.byref(h)) == ERR_ARG and b"LDS" in lib.spdy_last_error()
    assert lib.spdy_letkf_create(tall.h, 30, 0, ctypes.byref(h)) == 0 and lib.spdy_letkf_destroy(h) == 0
    tall.close()
    bare = s.Spectral("t30", kx=16, max_batch=256, device=-1)          # kx = 16 has no sigma levels until set_sigma
    assert lib.spdy_letkf_create(bare.h, 2, 0, ctypes.byref(h)) == ERR_STATE
    bare.close()
    lt = s.Letkf(sp, 32, 0, 5e5)                                       # both ends of the range, no observations at all
    lt.set_obs([], [], [], [], [], [])
    assert lt.table("rinv").shape == (0,)
    lt.close()
    s.Letkf(sp, 2, 3, 5e5).close()
    assert lib.spdy_letkf_destroy(None) == 0


def test_localization_checks(host):
    s, sp, _ = host
    lt = s.Letkf(sp, 3, 4, 5e5)
    assert sp.lib.spdy_letkf_set_localization(None, 1.0, 1.0, 1.0) == ERR_ARG
    for bad in ((0.0, 0.1, 1.0), (-1.0, 0.1, 1.0), (float("nan"), 0.1, 1.0), (5e5, float("inf"), 1.0), (5e5, 0.1, 0.0),
                (5e5, 0.1, -2.0), (5e5, 0.1, float("nan"))):
        assert code(s, lt.set_localization, *bad) == ERR_ARG, bad
    lt.set_localization(5e5, -1.0, 1.3)                                # sigma_v <= 0: no vertical factor
    lt.close()


def test_set_obs_rejections(host):
    """var or lev out of range, a non-finite or non-positive error, |lat| > 90, non-finite lon or value, nobs > max_obs: SPDY_ERR_ARG,
    and the earlier observations stay"""
    s, sp, _ = host
    lt = s.Letkf(sp, 3, 4, 5e5)
    good = ([lk.T, lk.PS], [1, 99], [10.0, 20.0], [5.0, -5.0], [1.0, 2.0], [1.0, 0.5])      # lev is ignored for PS
    lt.set_obs(*good)
    kept = lt.table("stencil_weight").copy()
    one = lambda **kw: [[kw.get(k, dflt)] for k, dflt in (("var", lk.T), ("lev", 1), ("lon", 10.0), ("lat", 5.0), ("value", 1.0), ("error", 1.0))]
    for bad in (dict(var=5), dict(var=-1), dict(lev=5), dict(lev=-1), dict(error=0.0), dict(error=-1.0), dict(error=float("nan")),
                dict(error=float("inf")), dict(lat=90.5), dict(lat=-91.0), dict(lat=float("nan")), dict(lon=float("inf")),
                dict(value=float("nan"))):
        assert code(s, lt.set_obs, *one(**bad)) == ERR_ARG, bad
    obs = (s.letkf.Obs * 5)()
    assert sp.lib.spdy_letkf_set_obs(lt.h, 5, ctypes.cast(obs, ctypes.c_void_p)) == ERR_ARG and b"max_obs" in sp.lib.spdy_last_error()
    assert sp.lib.spdy_letkf_set_obs(lt.h, -1, None) == ERR_ARG
    assert sp.lib.spdy_letkf_set_obs(lt.h, 2, None) == ERR_ARG and b"null" in sp.lib.spdy_last_error()
    assert sp.lib.spdy_letkf_set_obs(None, 0, None) == ERR_ARG
    with pytest.raises(ValueError):
        lt.set_obs([lk.T] * 5, [0] * 5, [0.0] * 5, [0.0] * 5, [0.0] * 5, [1.0] * 5)
    with pytest.raises(ValueError):
        lt.set_obs([lk.T, lk.T], [0], [0.0], [0.0], [0.0], [1.0])
    assert lt.nobs == 2 and np.array_equal(lt.table("stencil_weight"), kept)
    lt.close()


def test_tables_against_the_restatement(host):
    """the stencils of observations on a grid point, between columns ix-1 and 0, poleward of the outermost row at both poles, at lon =
    360 and at negative longitude, as rows of H over the grid; unit vectors, ln sigma_o and 1/error^2"""
    s, sp, g = host
    pts = lk.edge_points(g)
    n = len(pts)
    obs = lk.make_obs([o % 5 for o in range(n)], [(3 * o) % g.kx for o in range(n)], [p[0] for p in pts], [p[1] for p in pts],
                      np.arange(n) * 1.0, 0.5 + np.arange(n))
    lt = s.Letkf(sp, 3, n, 5e5)
    lt.set_obs(*lk.args(obs))
    idx, wgt = lt.table("stencil_index"), lt.table("stencil_weight")
    assert idx.shape == (n, 4) and idx.min() >= 0 and idx.max() < g.ix * g.il
    assert np.max(np.abs(wgt.sum(axis=1) - 1.0)) <= 4 * lk.EPS and wgt.min() >= 0.0
    ridx, rwgt = lk.stencil(g, obs["lon"], obs["lat"])
    assert np.max(np.abs(lk.dense_rows(g, idx, wgt) - lk.dense_rows(g, ridx, rwgt))) <= 1e-13
    H = lk.dense_rows(g, idx, wgt)
    on_point = H[0]
    assert abs(on_point[7 * g.ix + 5] - 1.0) <= 1e-13                                   # on a grid point
    assert H[1][12 * g.ix:].reshape(-1, g.ix)[:, [0, g.ix - 1]].sum() > 1.0 - 1e-13      # lon 359: columns ix-1 and 0 only
    for o, row in ((3, g.il - 1), (5, g.il - 1), (4, 0), (6, 0), (11, 0), (12, g.il - 1)):
        assert abs(H[o][row * g.ix:(row + 1) * g.ix].sum() - 1.0) <= 4 * lk.EPS, o        # the outermost row, weight 1
    assert np.max(np.abs(H[7] - lk.dense_rows(g, *lk.stencil(g, np.array([0.0]), np.array([45.0])))[0])) <= 1e-13   # lon = 360 is lon = 0
    assert H[7].reshape(g.il, g.ix)[:, 1:].sum() == 0.0
    assert np.max(np.abs(H[8] - lk.dense_rows(g, *lk.stencil(g, np.array([347.5]), np.array([-5.0])))[0])) <= 1e-13
    assert np.max(np.abs(lt.table("unit") - lk.unit(obs["lon"], obs["lat"]))) <= 4 * lk.EPS
    assert np.max(np.abs(lt.table("lnsigma") - lk.lnsigma(g, obs))) <= 4 * lk.EPS
    assert np.max(np.abs(lt.table("rinv") * obs["error"] ** 2 - 1.0)) <= 4 * lk.EPS
    assert sp.lib.spdy_letkf_table(lt.h, b"nothing", None, 0) == ERR_ARG
    assert sp.lib.spdy_letkf_table(lt.h, None, None, 0) == ERR_ARG
    buf = np.zeros(3)
    assert sp.lib.spdy_letkf_table(lt.h, b"rinv", buf.ctypes.data_as(ctypes.c_void_p), 3) == ERR_ARG
    lt.close()


def test_device_calls_need_a_device(host):
    """the *_dev calls on a host-only plan: a NULL object, then no localisation, then a NULL pointer, SPDY_ERR_NO_DEVICE last"""
    import torch
    s, sp, g = host
    lib, h = sp.lib, ctypes.c_void_p()
    assert lib.spdy_letkf_create(sp.h, 3, 4, ctypes.byref(h)) == 0
    p = [ctypes.c_void_p(8)] * 10
    assert lib.spdy_letkf_analyse_grid_dev(None, *p) == ERR_ARG
    assert lib.spdy_letkf_analyse_grid_dev(h, *p) == ERR_STATE and lib.spdy_ens_letkf_dev(h, *p[:5]) == ERR_STATE
    assert lib.spdy_letkf_set_localization(h, 5e5, 0.0, 1.0) == 0
    assert lib.spdy_letkf_analyse_grid_dev(h, *(p[:9] + [None])) == ERR_ARG
    assert lib.spdy_ens_letkf_dev(h, *(p[:4] + [None])) == ERR_ARG
    assert lib.spdy_letkf_analyse_grid_dev(h, *p) == ERR_NO_DEVICE and lib.spdy_ens_letkf_dev(h, *p[:5]) == ERR_NO_DEVICE
    d = ctypes.c_void_p()
    assert lib.spdy_letkf_field(h, b"nothing", ctypes.byref(d)) == ERR_ARG
    assert lib.spdy_letkf_field(h, b"hx", None) == ERR_ARG
    assert lib.spdy_letkf_field(h, b"hx", ctypes.byref(d)) == ERR_NO_DEVICE
    assert lib.spdy_letkf_destroy(h) == 0
    lt = s.Letkf(sp, 3, 4, 5e5)
    x = [torch.zeros((3, g.kx, g.il, g.ix), dtype=torch.float64) for _ in range(4)] + [torch.zeros((3, g.il, g.ix), dtype=torch.float64)]
    assert code(s, lt.analyse_grid, *x) == ERR_NO_DEVICE
    lt.close()


def test_shape_errors(host):
    """Letkf.analyse_grid and Ensemble.analyse refuse what does not fit before anything is called"""
    import torch
    s, sp, g = host
    lt = s.Letkf(sp, 3, 4, 5e5)
    x = [torch.zeros((3, g.kx, g.il, g.ix), dtype=torch.float64) for _ in range(4)] + [torch.zeros((3, g.il, g.ix), dtype=torch.float64)]
    for i, bad in ((0, torch.zeros((2, g.kx, g.il, g.ix), dtype=torch.float64)), (4, torch.zeros((3, 1, g.il, g.ix), dtype=torch.float64)),
                   (2, torch.zeros((3, g.kx, g.il, g.ix), dtype=torch.float32)), (1, x[1].transpose(2, 3))):
        with pytest.raises(ValueError):
            lt.analyse_grid(*(x[:i] + [bad] + x[i + 1:]))
    with pytest.raises(ValueError):
        lt.analyse_grid(*x, out=x[:4])
    ens = s.Ensemble(sp, 2, device="cpu")
    with pytest.raises(ValueError):
        ens.analyse(lt)                                              # three members against two
    other = support.plan("t30k5", 3 * 20, device=-1)
    with pytest.raises(ValueError):
        s.Ensemble(other, 3, device="cpu").analyse(lt)               # another plan
    other.close()
    assert code(s, s.Ensemble(sp, 3, device="cpu").analyse, lt) == ERR_NO_DEVICE
    lt.close()
