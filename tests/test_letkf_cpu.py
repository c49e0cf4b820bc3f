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


@pytest.mark.parametrize("E", [16, 31, 32])
def test_hard_problems_and_the_sweep_cap(E):
    """Local problems built directly, C = sum_o r_o Y_o Y_o^T of n = E/2 - 4, E/2, E/2 + 4, E - 1 observations (rank below E: the
    eigenvalue (E-1)/rho repeats) with r scaled to kappa(A) = 2e6, 1e8 and 5e9, 16 seeded matrices of each.  They need more
    sweeps than a problem of full rank (n = E - 1: 9 or 10 at E = 31 and 32): the largest count, the closing idle sweep included,
    is 12 at E = 16, 14 at E = 31 and 15 at E = 32, reached at n <= E/2 + 4, whatever kappa is.  Asserted: the largest count is at
    least 12 and at most lk.SWEEPS = LETKF_SWEEPS, and jacobi(A, sweeps=16) returns the bits of jacobi(A, sweeps=30) -- on these
    inputs the kernel's cap is not what ends the solve."""
    rho, N, A, case = 1.1, 16, [], []
    for n in (E // 2 - 4, E // 2, E // 2 + 4, E - 1):
        for target in (2e6, 1e8, 5e9):
            rng = np.random.default_rng(1000 * E + n)
            for _ in range(N):
                Y = rng.standard_normal((n, E))
                Y -= Y.mean(axis=1, keepdims=True)
                r = rng.uniform(0.5, 1.5, n)
                C1, _ = lk.local_problem(Y, np.zeros(n), r)
                C, _ = lk.local_problem(Y, np.zeros(n), r * ((target - 1.0) * ((E - 1) / rho) / np.linalg.eigvalsh(C1)[-1]))
                A.append(C + ((E - 1) / rho) * np.eye(E))
            case.append((n, target))
    A = np.stack(A)
    lam, V, ran = lk.jacobi(A, sweeps=30, counts=True)
    kappa = lam.max(axis=1) / lam.min(axis=1)
    for c, (n, target) in enumerate(case):
        print("[letkf hard E=%d n=%d kappa=%.0e] sweeps %d to %d" % (E, n, target, ran[c * N:(c + 1) * N].min(), ran[c * N:(c + 1) * N].max()))
    assert 1e6 <= float(kappa.min()) and float(kappa.max()) <= 1e10, (kappa.min(), kappa.max())
    capped = lk.jacobi(A, sweeps=lk.SWEEPS)
    assert support.same_bits(capped[0], lam) and support.same_bits(capped[1], V)
    assert 12 <= int(ran.max()) <= lk.SWEEPS, ran.max()


def test_jacobi_counts_its_sweeps():
    """a diagonal matrix: one idle sweep; a matrix of one off-diagonal pair: the rotation and the idle sweep; the count stops at
    `sweeps`; the results with and without the counts are the same"""
    rng = np.random.default_rng(8)
    B = rng.standard_normal((3, 5, 5))
    A = B @ np.swapaxes(B, 1, 2) + 5.0 * np.eye(5)
    A[0] = np.diag(np.arange(1.0, 6.0))
    A[1] = np.diag(np.arange(1.0, 6.0))
    A[1, 0, 3] = A[1, 3, 0] = 0.25
    lam, V, ran = lk.jacobi(A, counts=True)
    assert ran[0] == 1 and ran[1] == 2 and 3 <= ran[2] <= 10
    assert all(support.same_bits(a, b) for a, b in zip(lk.jacobi(A), (lam, V)))
    assert lk.jacobi(A, sweeps=2, counts=True)[2].tolist() == [1, 2, 2]
    many = np.concatenate([A] * (lk.SLAB // 3 + 2))          # more than one slab
    lam2, V2, ran2 = lk.jacobi(many, counts=True)
    assert support.same_bits(lam2[-3:], lam) and support.same_bits(V2[-3:], V) and ran2[-3:].tolist() == ran.tolist()


def test_interleave():
    """every pattern keeps the real observations in their order at the places it reports, takes the pad in its order, and puts the
    real ones in the lanes, waves and chunks it says"""
    n = 375
    real = lk.make_obs(np.arange(n) % 5, np.arange(n) % 3, np.arange(n) * 0.5, np.zeros(n), np.arange(n) + 0.25, np.ones(n))
    pad = lk.make_obs(np.zeros(1200), np.zeros(1200), np.zeros(1200), np.ones(1200), -1.0 - np.arange(1200), 2.0 * np.ones(1200))
    sizes = {}
    for pattern in lk.PATTERNS:
        obs, at = lk.interleave(real, pad, pattern)
        sizes[pattern] = len(obs["var"])
        assert (np.diff(at) > 0).all() and all(np.array_equal(obs[k][at], real[k]) for k in real), pattern
        rest = np.setdiff1d(np.arange(sizes[pattern]), at)
        assert all(np.array_equal(obs[k][rest], pad[k][:len(rest)]) for k in pad), pattern
    assert sizes == {"front1": n + 1, "front255": n + 255, "front256": n + 256, "alternate": 2 * n, "wave3": 5 * 256 + 192 + n - 320,
                     "hole": n + 256}
    assert lk.interleave(real, pad, "front256")[1][0] == lk.CHUNK                         # the first chunk: pad only
    assert (lk.interleave(real, pad, "alternate")[1] % 2 == 1).all()
    assert (lk.interleave(real, pad, "wave3")[1] % lk.CHUNK >= 192).all()                 # the last wave of every chunk
    at = lk.interleave(real, pad, "hole")[1]
    assert not np.isin(at // lk.CHUNK, [1]).any() and (at // lk.CHUNK == 0).sum() == lk.CHUNK and (at // lk.CHUNK == 2).any()
    for pattern, total in (("front1", 512), ("alternate", 768)):
        obs, at2 = lk.interleave(real, pad, pattern, total)
        assert len(obs["var"]) == total and np.array_equal(at2, lk.interleave(real, pad, pattern)[1])
        assert (obs["error"][at2[-1] + 1:] == 2.0).all()


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


def test_local_problems_are_problems(host):
    """an observation is added at the columns it reaches and nowhere else, so a column's C and b do not depend on which other columns
    are asked for: `problems` at a subset of columns is `problems` at all columns restricted to that subset, bit for bit -- at columns
    in range of a cluster, at the edge of its range and out of range, with and without the vertical factor; an empty network gives
    zero"""
    _, _, g = host
    x = lk.ensemble(g, 4, seed=44)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=24, outside=6)
    s = lk.obs_space(g, x, obs)
    for sigma_v in (0.0, 0.1):
        C, b = lk.problems(g, obs, s, lk.SIGMA_H, sigma_v)
        Cl, bl = lk.problems(g, obs, s, lk.SIGMA_H, sigma_v, cols)
        assert Cl.any() and not Cl[-1].any() and support.same_bits(C[cols], Cl) and support.same_bits(b[cols], bl), sigma_v
    none = lk.make_obs([], [], [], [], [], [])
    assert not lk.problems(g, none, lk.obs_space(g, x, none), lk.SIGMA_H, 0.1, cols)[0].any()


def test_edge_inputs(host):
    """the conditions the edge-column test on the device puts on its inputs (lk.edge_conditions), and the edge columns themselves"""
    _, _, g = host
    cols = lk.edge_columns(g)
    jj, ii = np.divmod(cols, g.ix)
    assert len(cols) == 4 * g.ix + 2 * (g.il - 4) and (np.diff(cols) > 0).all()
    assert all(((jj == j).sum() == g.ix) for j in (0, 1, g.il - 2, g.il - 1)) and all((ii == i).sum() == g.il for i in (0, g.ix - 1))
    for E in (3, 32):
        sets = lk.edge_inputs(g, lk.ensemble(g, E, seed=80 + E))
        obs, _, out = lk.edge_conditions(g, sets)
        assert [len(s["var"]) for _, s in sets] == [40, 200, 200, 200]
        print("[letkf edge inputs E=%d] %d observations, %d edge columns, %d of them out of range" % (E, len(obs["var"]), len(cols), out.sum()))


def test_padded_inputs_and_the_order_of_the_sums(host):
    """the conditions of the padded-scan test on the device (lk.padded_inputs, lk.padded_conditions), its set sizes, and on the
    restatement what that test asks of the kernel: C and b of the columns out of the pad's range keep their bits under every
    pattern -- and lose them when two real observations change places, so a scan that reorders its survivors is noticed"""
    _, _, g = host
    x = lk.ensemble(g, 3, seed=90)
    real, pad = lk.padded_inputs(g, x)
    far, acted = lk.padded_conditions(g, real, pad)
    nr = len(real["var"])
    print("[letkf padded inputs] %d real observations (%d of the sparse set), %d columns compared, %d in range of the pad"
          % (nr, nr - 320, far.sum(), acted.sum()))
    assert acted.sum() >= 20 and not (acted & far).any()
    cluster = lk.in_range(g, {k: v[:320] for k, v in real.items()}).any(axis=1)
    cols = np.concatenate([np.nonzero(cluster)[0][::4], np.nonzero(far & ~cluster)[0][::300]])
    C, b = lk.problems(g, real, lk.obs_space(g, x, real), lk.SIGMA_H, 0.1, cols)
    for pattern in lk.PATTERNS:
        obs, at = lk.interleave(real, pad, pattern)
        Cp, bp = lk.problems(g, obs, lk.obs_space(g, x, obs), lk.SIGMA_H, 0.1, cols)
        assert support.same_bits(C, Cp) and support.same_bits(b, bp), pattern
    moved = {k: v.copy() for k, v in real.items()}
    for k in moved:
        moved[k][[0, 200]] = moved[k][[200, 0]]
    Cm, _ = lk.problems(g, moved, lk.obs_space(g, x, moved), lk.SIGMA_H, 0.1, cols)
    assert not support.same_bits(C, Cm) and np.max(np.abs(C - Cm)) <= 1e-12 * np.max(np.abs(C))


@pytest.mark.parametrize("E", [32, 31])
def test_hard_inputs_on_the_grid(E, host):
    """the hard problems of the device test (lk.hard_obs: 16 observations within a degree of one grid point, errors 1e-3 and 3e-5 of
    the spread, sigma_v = 0): kappa(A) in [1e6, 1e10], and lk.jacobi needs more than 9 sweeps and no more than lk.SWEEPS at the
    compared columns.  Measured: kappa 4.4e6 and 4.9e9 at E = 32 with up to 15 and 16 sweeps, 4.0e6 and 4.4e9 at E = 31 with up
    to 14 and 14."""
    _, _, g = host
    x = lk.ensemble(g, E, seed=E)
    for factor in (1e-3, 3e-5):
        obs = lk.hard_obs(g, x, factor)
        cols = lk.columns_for(g, obs, lk.SIGMA_H, most=16, outside=2)
        C, _ = lk.problems(g, obs, lk.obs_space(g, x, obs), lk.SIGMA_H, 0.0, cols)
        A = C[:, 0] + ((E - 1) / lk.RHO) * np.eye(E)                          # no vertical factor: every level has the same A
        assert support.same_bits(C[:, 0], C[:, g.kx - 1])
        lam, _, ran = lk.jacobi(A, counts=True)
        kappa = float(np.max(lam.max(axis=1) / lam.min(axis=1)))
        print("[letkf hard grid E=%d error=%g] kappa %.2e, sweeps %s" % (E, factor, kappa, ran.tolist()))
        assert 1e6 <= kappa <= 1e10 and 9 < int(ran.max()) <= lk.SWEEPS, (kappa, ran.max())


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
