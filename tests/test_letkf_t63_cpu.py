"""CPU: what the GPU tests of the ensemble analysis "on the T63 L16 grid" (tests/test_gpu_letkf*.py) rely on,
checked on a host-only plan of 192 x 96 columns and 16 levels with the library's own tables: the crafted at-pressure network holds
every class, the edge-column and padded-scan conditions hold, every weight stride of the interpolation tests gives the stencil
classes it claims, in range of a cluster and out of it, and the host tables the kernels read -- the interpolation tables and the
observation stencils -- equal the NumPy restatement's."""
import numpy as np
import pytest

import letkf as lk
import letkfinterp as li
import letkfpressure as lp
import support

TAG = "t63k16"
STRIDES = [(2, 2), (3, 5), (96, 7), (4, 95)]       # tests/test_gpu_letkf_interp.py: STRIDES_T63


@pytest.fixture(scope="module")
def host():
    s = support.package()
    sp = support.plan(TAG, 32 * (2 * 16 + 1), device=-1)
    g = lp.Geometry(sp)
    assert (g.ix, g.il, g.kx) == (192, 96, 16) == support.grid(TAG)
    yield s, sp, g
    sp.close()


@pytest.mark.parametrize("E", [2, 3, 32])
def test_crafted_pressure_network_holds_every_class(E, host):
    """tests/letkfpressure.py's crafted ensemble and network at 16 levels: every bracket and every other class of every_class(16);
    observations out of some member's column and in it"""
    _, _, g = host
    x = lp.craft(g, E, seed=7 + E)
    obs = lp.network(g, x)
    found = lp.classes(g, x, obs)
    assert found == lp.every_class(16), found ^ lp.every_class(16)
    used = lk.obs_space(g, x, obs)["obs_used"]
    atp = lp.at_pressure(obs)
    print("[letkf t63 inputs E=%d] crafted network: %d observations, %d at a pressure, %d out of column"
          % (E, len(obs["var"]), atp.sum(), (used == 0.0).sum()))
    assert len(obs["var"]) > 3 * lk.CHUNK and (used[~atp] == 1.0).all() and 10 <= (used == 0.0).sum() < atp.sum() / 2


def test_edge_and_padded_conditions(host):
    """lk.edge_conditions at EDGE_SIGMA_H and lk.padded_conditions on the ensembles the GPU tests make"""
    _, _, g = host
    for seed in (80 + 3, 80 + 32, 32):                # test_gpu_letkf.py's E = 3 and 32, test_gpu_letkf_infl.py's
        obs, cols, out = lk.edge_conditions(g, lk.edge_inputs(g, lk.ensemble(g, 3, seed=seed)))
        print("[letkf t63 inputs] edge columns: %d observations, %d columns, %d out of range" % (len(obs["var"]), len(cols), out.sum()))
        assert len(cols) == 4 * g.ix + 2 * (g.il - 4)
    real, pad = lk.padded_inputs(g, lk.ensemble(g, 3, seed=93))
    far, acted = lk.padded_conditions(g, real, pad)
    assert acted.sum() >= 20 and not (acted & far).any()


@pytest.mark.parametrize("si,sj", STRIDES)
def test_stencil_classes_of_every_stride(si, sj, host):
    """li.class_columns gives all seven stencil classes, six at (4, 95) where only rows 0 and il-1 are coarse; at least 4 of the
    compared columns lie within C_H of a cluster centre and at least 2 beyond 2 C_H; and every chosen column is of its class by the
    restatement's own stencil: the number of distinct coarse columns it reads and whether its cell wraps"""
    _, _, g = host
    cls = li.class_columns(g, si, sj)
    names = ["interior", "coarse longitude", "coarse row", "wrap", "last interval", "j = 0", "j = il-1"]
    assert list(cls) == ([n for n in names if n != "coarse row"] if sj == g.il - 1 else names)
    cols = np.unique(np.concatenate(list(cls.values())))
    d = np.minimum(*(lk.distance(g.colunit, lk.unit([p[0]], [p[1]]))[:, 0] for p in (li.CENTRE, li.POLAR)))
    assert (d[cols] < lk.C_H).sum() >= 4 and (d[cols] > 2.0 * lk.C_H).sum() >= 2, ((d[cols] < lk.C_H).sum(), (d[cols] > 2.0 * lk.C_H).sum())
    idx, wgt = li.stencils(g, si, sj)
    coarse = li.coarse_columns(g, si, sj)
    read = lambda c: np.unique(coarse[idx[c][wgt[c] != 0.0]])
    for c in cls["interior"]:
        assert len(read(c)) == 4
    for c in np.concatenate([cls["coarse longitude"], cls.get("coarse row", cls["coarse longitude"]), cls["j = 0"], cls["j = il-1"]]):
        assert len(read(c)) == 2, c
    for c in cls["wrap"]:
        assert (read(c) % g.ix == 0).any() and (read(c) % g.ix == g.ix - si).any()
    assert (read(cls["j = il-1"][0]) // g.ix == g.il - 1).all() and (read(cls["j = 0"][0]) // g.ix == 0).all()
    rows = li.coarse_rows(g, sj)                      # a last interval of one row (rows il-2 and il-1 both coarse) has no row inside
    last = g.il - 1 if rows[-1] - rows[-2] > 1 else rows[-2]
    assert all((read(c) // g.ix).max() == last and c // g.ix >= rows[-2] for c in cls["last interval"])


@pytest.mark.parametrize("si,sj", STRIDES)
def test_interpolation_tables(si, sj, host):
    """a host-only object's coarse_columns and interp_index equal the restatement's, interp_weight within 2 eps"""
    s, sp, g = host
    lt = s.Letkf(sp, 3, 0, lk.SIGMA_H, weight_stride=(si, sj))
    coarse, idx, wgt = (lt.table(n) for n in ("coarse_columns", "interp_index", "interp_weight"))
    ridx, rwgt = li.stencils(g, si, sj)
    assert np.array_equal(coarse, li.coarse_columns(g, si, sj)) and len(coarse) == (g.ix // si) * len(li.coarse_rows(g, sj))
    assert idx.shape == (g.ix * g.il, 4) and np.array_equal(idx, ridx) and idx.min() >= 0 and idx.max() < len(coarse)
    assert np.max(np.abs(wgt - rwgt)) <= 2 * lk.EPS and wgt.min() >= 0.0
    lt.close()


def test_observation_stencils(host):
    """the stencil tables of set_obs for lk.edge_obs -- the wrap cell between longitude 191 and 0, the rows poleward of the outermost
    latitude, lon = 360 and negative longitudes -- against lk.stencil, as rows of H over the grid (tests/test_letkf_cpu.py's rule);
    where the four indices are distinct they are equal one by one"""
    s, sp, g = host
    x = lk.ensemble(g, 3, seed=43)
    obs = lk.edge_obs(g, x)
    lt = s.Letkf(sp, 3, len(obs["var"]), lk.SIGMA_H)
    lt.set_obs(*lk.args(obs))
    idx, wgt = lt.table("stencil_index"), lt.table("stencil_weight")
    ridx, rwgt = lk.stencil(g, obs["lon"], obs["lat"])
    assert idx.shape == ridx.shape and idx.min() >= 0 and idx.max() < g.ix * g.il
    assert np.max(np.abs(lk.dense_rows(g, idx, wgt) - lk.dense_rows(g, ridx, rwgt))) <= 1e-13
    plain = np.array([len(set(r)) == 4 and (w > 1e-9).all() for r, w in zip(ridx, rwgt)])
    assert plain.sum() >= 20 and np.array_equal(idx[plain], ridx[plain]) and np.max(np.abs(wgt[plain] - rwgt[plain])) <= 1e-13
    assert (ridx[1] % g.ix).tolist() == [g.ix - 1, 0, g.ix - 1, 0]                  # (359, 12.3): between longitude 191 and 0
    assert np.max(np.abs(lt.table("unit") - lk.unit(obs["lon"], obs["lat"]))) <= 4 * lk.EPS
    assert np.max(np.abs(lt.table("lnsigma") - lk.lnsigma(g, obs))) <= 4 * lk.EPS
    lt.close()
