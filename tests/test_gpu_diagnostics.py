"""GPU: check_diagnostics on the device (spdy_diagnostics_*): the kernel's sums and temp against the restatement
(tests/diagnostics.py, pinned to the flang-built reference by tests/golden/ref_diagnostics.npz), the edges of the sum, the device
counter and the ring under a replayed capture, the sticky first offence on the exact thresholds, non-finite values, and the call
as the last node of a captured model step.  Expected values always come from the restatement on the downloaded inputs.

The bar of the two sums is 1e-12 relative: every term is >= 0, so two summation orders of N terms differ by at most about
2 (N - 1) 2**-53 plus a few roundings per term -- 2.2e-13 for the 992 coefficients of T30, 9.3e-13 for the 4160 of T63.  temp is
one load and one multiply and must be bit-equal."""
import ctypes

import numpy as np
import pytest

import diagnostics as dg
import dynstep
import modelstep
import support
from conftest import TOL

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -5


@pytest.fixture(scope="module")
def plans():
    """one plan per variant for the whole module"""
    with support.plan_cache(lambda tag: support.ensemble_plan(tag, 1)) as get:
        yield get


def _restated(sp, x):
    return dg.diag(x["vor"], x["div"], x["t"], sp.table("elm2"))


def _check(d, x):
    """one eager check_dev on host arrays; returns the step's row [3, kx]"""
    step = d.status()["next_step"]
    d.check_dev(*[support.dev(x[n]) for n in ("vor", "div", "t")])
    return d.read(step, 1)[0]


def _close(got, want, what=""):
    """the two sums within TOL relative per level (exact where the restatement is 0), temp bit-equal; returns the worst error"""
    assert np.array_equal(got[2], want[2]), (what, "temp", got[2], want[2])
    assert np.array_equal(got[:2][want[:2] == 0.0], want[:2][want[:2] == 0.0]), (what, "zero sums")
    nz = want[:2] != 0.0
    e = float(np.abs(got[:2][nz] / want[:2][nz] - 1.0).max()) if nz.any() else 0.0
    assert e <= TOL, (what, e)
    return e


def _diag(sp, **kw):
    import speedy_f90_amd as s
    return s.Diagnostics(sp, **kw)


@pytest.mark.parametrize("tag", ["golden", "t30k5", "t63k16"])
def test_parity(tag, plans, golden):
    """the golden levels placed in a T30 L8 state, a T30 state of 5 levels, a T63 L16 state"""
    sp = plans("t30" if tag == "golden" else tag)
    x = dg.state(sp, 5100)
    if tag == "golden":
        g = golden("diagnostics")
        for n in x:
            x[n][g["levels"]] = g[n]
    d = _diag(sp, capacity=2)
    got, want = _check(d, x), _restated(sp, x)
    e = _close(got, want, tag)
    print("\n[diagnostics parity %s] sums vs restatement %.1e; reke %.3g .. %.3g" % (tag, e, want[0].min(), want[0].max()))
    assert want[0].min() > 0.0 and want[1].min() > 0.0 and d.status()["bad_step"] == -1
    if tag == "golden":                                    # and against the reference's own numbers
        _close(got[:, g["levels"]], g["diag"], "reference")
    d.close()


def test_edges_of_the_sum(plans):
    sp = plans("t30k5")
    kx, nx, mx = sp.kx, sp.nx, sp.mx
    elm2 = sp.table("elm2").reshape(nx, mx)
    d = _diag(sp, capacity=2)
    base = dg.state(sp, 5200)
    # energy in the zonal column m = 1 only: both sums are 0.0 exactly
    zonal = {n: np.zeros_like(a) for n, a in base.items()}
    for n in ("vor", "div"):
        zonal[n][:, :, 0] = base[n][:, :, 0]
    zonal["t"] = base["t"]
    row = _check(d, zonal)
    assert np.abs(zonal["vor"]).max() > 0 and (row[:2] == 0.0).all() and np.array_equal(row[2], _restated(sp, base)[2])
    # 1e30 on every m = 1 coefficient changes no bit of either sum
    want = _check(d, base)
    big = {n: a.copy() for n, a in base.items()}
    for n in ("vor", "div"):
        big[n][:, :, 0] += 1e30
    assert np.array_equal(_check(d, big)[:2], want[:2])
    # one coefficient: the first and the last of the range and the corner outside the triangle, on one level only
    lev, v = 3, 3.0e-5 - 4.0e-5j
    for m, n in ((1, 0), (mx - 1, nx - 1), (mx - 1, 0)):
        one = {k: np.zeros_like(a) for k, a in base.items()}
        one["vor"][lev, n, m] = v
        one["div"][lev, n, m] = 2.0 * v
        row, want = _check(d, one), _restated(sp, one)
        assert want[0, lev] > 0 and abs(want[0, lev] / (elm2[n, m] * abs(v) ** 2) - 1.0) <= 1e-14
        _close(row, want, (m, n))
        others = np.arange(kx) != lev
        assert (row[:, others] == 0.0).all()               # one level nonzero touches that level's row only
    d.close()


def test_counter_and_ring(plans):
    import torch
    sp = plans("t30k5")
    x = dg.state(sp, 5300)
    D = {n: support.dev(a) for n, a in x.items()}
    d = _diag(sp, capacity=4, first_step=1)
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as g:
            d.check_dev(D["vor"], D["div"], D["t"])
            n, lev = ctypes.c_longlong(), ctypes.c_int()
            rows = np.zeros((1, 3, sp.kx))
            assert sp.lib.spdy_diagnostics_status(d.h, ctypes.byref(n), ctypes.byref(n), ctypes.byref(lev), ctypes.byref(lev), None) == STATE
            assert sp.lib.spdy_diagnostics_read(d.h, 1, 1, rows.ctypes.data_as(ctypes.c_void_p)) == STATE
            assert sp.lib.spdy_diagnostics_reset(d.h, 5) == STATE
        assert g.num_nodes() == 1                          # ONE launch
        assert d.status()["next_step"] == 1                # a capture runs nothing
        want = {}
        for step in range(1, 8):
            want[step] = dg.diag(D["vor"].cpu().numpy(), x["div"], x["t"], sp.table("elm2"))
            g.launch()
            sp.synchronize()
            D["vor"].mul_(1.25)                            # in place: the replay reads the pointers it was captured with
            torch.cuda.synchronize()
        st = d.status()
        assert st["next_step"] == 8 and st["bad_step"] == -1 and st["bad_row"] is None
        got = d.read(4, 4)
        for i, step in enumerate(range(4, 8)):
            _close(got[i], want[step], step)
        assert not np.array_equal(got[0][0], got[1][0])
        lib, P = sp.lib, rows.ctypes.data_as(ctypes.c_void_p)
        assert lib.spdy_diagnostics_read(d.h, 3, 1, P) == ARG         # overwritten
        assert lib.spdy_diagnostics_read(d.h, 8, 1, P) == ARG         # not yet written
        assert lib.spdy_diagnostics_read(d.h, 7, 1, P) == 0
        big = np.zeros((5, 3, sp.kx))
        assert lib.spdy_diagnostics_read(d.h, 7, 2, big.ctypes.data_as(ctypes.c_void_p)) == ARG
        assert lib.spdy_diagnostics_read(d.h, 3, 5, big.ctypes.data_as(ctypes.c_void_p)) == ARG
        d.reset(100)
        assert d.status()["next_step"] == 100 and (d.field("history").numpy() == 0.0).all()
        for step in (99, 100, 7):
            assert lib.spdy_diagnostics_read(d.h, step, 1, P) == ARG  # nothing of the earlier run, nothing written yet
        now = dg.diag(D["vor"].cpu().numpy(), x["div"], x["t"], sp.table("elm2"))
        g.launch()
        sp.synchronize()
        _close(d.read(100, 1)[0], now, "after reset")
        assert d.status()["next_step"] == 101 and lib.spdy_diagnostics_read(d.h, 99, 1, P) == ARG
        g.close()
    finally:
        sp.use_torch_stream()
    d.close()


def _temp_inputs(limit, above):
    """Re t(1,1,k) whose restated temp is exactly `limit`, and the nearest one whose temp lies beyond it (above or below)"""
    x = limit / dg.SQRT_HALF
    while dg.SQRT_HALF * x > limit:
        x = np.nextafter(x, -np.inf)
    while dg.SQRT_HALF * x < limit:
        x = np.nextafter(x, np.inf)
    assert dg.SQRT_HALF * x == limit, "no input gives the limit exactly"
    y = x
    while dg.SQRT_HALF * y == limit:
        y = np.nextafter(y, np.inf if above else -np.inf)
    assert dg.SQRT_HALF * y == np.nextafter(limit, np.inf if above else -np.inf)      # one ulp beyond
    return x, y


@pytest.mark.parametrize("bit", [dg.TEMP_HIGH, dg.TEMP_LOW])
def test_sticky_stop_on_the_temperature_limits(bit, plans):
    import speedy_f90_amd as s
    sp = plans("t30")
    lev, other = 5, 2
    eq, beyond = _temp_inputs(dg.LIMITS[3 if bit == dg.TEMP_HIGH else 2], bit == dg.TEMP_HIGH)
    x = dg.state(sp, 5400)
    d = _diag(sp, capacity=3, first_step=10)
    x["t"][lev, 0, 0] = eq
    row = _check(d, x)                                      # step 10: on the limit, no trip
    assert row[2, lev] == dg.LIMITS[3 if bit == dg.TEMP_HIGH else 2] and d.status()["bad_step"] == -1
    assert d.raise_if_stopped()["next_step"] == 11
    x["t"][lev, 0, 0] = beyond
    bad = _check(d, x)                                      # step 11: one ulp beyond
    want = _restated(sp, x)
    _close(bad, want, "bad row")
    assert list(dg.masks(want)) == [bit if k == lev else 0 for k in range(sp.kx)]
    first = d.status()
    assert (first["bad_step"], first["bad_level"], first["bad_mask"]) == (11, lev, bit) and np.array_equal(first["bad_row"], bad)
    x["t"][lev, 0, 0] = eq
    for step in range(12, 16):                              # in range again, and the ring (3 rows) wraps over step 11
        _check(d, x)
    x["t"][other, 0, 0] = beyond                            # a later offence of another level does not replace the first
    _check(d, x)
    st = d.status()
    assert st["next_step"] == 17
    assert (st["bad_step"], st["bad_level"], st["bad_mask"]) == (11, lev, bit) and np.array_equal(st["bad_row"], bad)
    rows = np.zeros((1, 3, sp.kx))
    assert sp.lib.spdy_diagnostics_read(d.h, 11, 1, rows.ctypes.data_as(ctypes.c_void_p)) == ARG
    with pytest.raises(s.DiagnosticsStop) as e:
        d.raise_if_stopped()
    assert str(e.value) == dg.lines(11, bad) + dg.STOP and e.value.status["bad_level"] == lev
    d.close()


def test_energy_limits_and_the_order_of_offences(plans):
    sp = plans("t30")
    x = dg.state(sp, 5500)
    want = _restated(sp, x)
    d = _diag(sp, capacity=2)
    for i, bit in ((0, dg.REKE), (1, dg.DEKE)):
        top = int(np.argmax(want[i]))
        assert np.sort(want[i])[-2] < want[i, top] * (1 - 1e-6)
        lim = list(dg.LIMITS)
        lim[i] = want[i, top] * (1 + 1e-9)                  # the sums are not bit-pinned: a clear margin on either side
        d.set_limits(lim)
        d.reset(0)
        _check(d, x)
        assert d.status()["bad_step"] == -1
        lim[i] = want[i, top] * (1 - 1e-9)
        d.set_limits(lim)
        _check(d, x)
        st = d.status()
        assert (st["bad_step"], st["bad_level"], st["bad_mask"]) == (1, top, bit)
    d.set_limits(None)                                      # the reference's again
    d.reset(0)
    assert d.field("limits").numpy().tolist() == list(dg.LIMITS)
    # two levels at different steps: the earlier step is reported
    hot, cold = 330.0 / dg.SQRT_HALF, 170.0 / dg.SQRT_HALF
    y = {n: a.copy() for n, a in x.items()}
    _check(d, y)
    y["t"][6, 0, 0] = hot
    _check(d, y)
    y["t"][1, 0, 0] = cold
    _check(d, y)
    st = d.status()
    assert (st["next_step"], st["bad_step"], st["bad_level"], st["bad_mask"]) == (3, 1, 6, dg.TEMP_HIGH)
    # two levels at the same step: the lower level, both masks
    d.reset(7)
    _check(d, y)
    st = d.status()
    assert (st["bad_step"], st["bad_level"], st["bad_mask"]) == (7, 1, dg.TEMP_LOW | dg.TEMP_HIGH)
    _close(st["bad_row"], _restated(sp, y), "two levels")
    d.close()


def test_non_finite(plans):
    sp = plans("t30")
    x = dg.state(sp, 5600)
    d = _diag(sp, capacity=4)
    base = _check(d, x)
    lev = 4
    y = {n: a.copy() for n, a in x.items()}
    y["div"][:, 3, 0] = np.nan                              # in the zonal column the reference never reads it
    assert np.array_equal(_check(d, y), base) and d.status()["bad_step"] == -1
    y["div"][lev, 3, 2] = np.nan
    row = _check(d, y)
    st = d.status()
    assert (st["bad_step"], st["bad_level"], st["bad_mask"]) == (2, lev, dg.NONFINITE)
    assert np.isnan(row[1, lev]) and list(dg.masks(row)) == [dg.NONFINITE if k == lev else 0 for k in range(sp.kx)]
    others = np.arange(sp.kx) != lev
    assert np.array_equal(row[:, others], base[:, others]) and np.array_equal(row[[0, 2], lev], base[[0, 2], lev])
    assert d.raise_if_stopped()["bad_mask"] == dg.NONFINITE            # the reference would run on
    d.close()


def _step_with_the_guard():
    """The T30 L8 adiabatic step captured without and with check_dev on time level 2 as its last node, three replays each ->
    (prognostics equal bit for bit, nodes without, nodes with, history [3, 3, kx], restated rows of the downloaded states)"""
    import torch
    sp = support.plan("t30", 4 * 8 + 4)
    dt = 2400.0
    sp.initialize_implicit(dt)
    st = dynstep.state(sp, 8000)
    d = _diag(sp, capacity=8, first_step=1)
    sp.use_own_stream()
    runs, nodes, want = [], [], []
    for guard in (False, True):
        D, W = modelstep.device_state(st), modelstep.Workspace(sp)
        torch.cuda.synchronize()
        with sp.graph_capture() as g:
            modelstep.step(sp, D, W, dt, form="composite")
            if guard:
                d.check_dev(D["vor"][1], D["div"][1], D["t"][1])
        nodes.append(g.num_nodes())
        for _ in range(3):
            g.launch()
            sp.synchronize()
            if guard:
                want.append(dg.diag(*[D[n][1].cpu().numpy() for n in ("vor", "div", "t")], sp.table("elm2")))
        runs.append({n: D[n].clone() for n in modelstep.PROG})
        g.close()
    same = all(torch.equal(runs[0][n], runs[1][n]) for n in modelstep.PROG)
    hist, status = d.read(1, 3), d.status()
    d.close()
    sp.close()
    return same, nodes, hist, np.stack(want), status


@pytest.fixture(scope="module")
def guarded_steps():
    return [_step_with_the_guard() for _ in range(2)]


def test_inside_the_step(guarded_steps):
    same, nodes, hist, want, status = guarded_steps[0]
    assert same, "the node changed the prognostics"
    assert nodes[1] == nodes[0] + 1, nodes
    assert np.isfinite(want).all() and status["next_step"] == 4
    tripped = [i + 1 for i in range(3) if dg.masks(want[i]).any()]       # the seeded state is not a balanced one: what the restatement says
    assert status["bad_step"] == (tripped[0] if tripped else -1)
    worst = max(_close(hist[i], want[i], "step %d" % (i + 1)) for i in range(3))
    print("\n[diagnostics inside the step] %d nodes with the guard; history vs restatement %.1e; reke %s" % (nodes[1], worst, hist[2][0]))
    assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[1], hist[2])


def test_determinism(guarded_steps):
    assert np.array_equal(guarded_steps[0][2], guarded_steps[1][2])
