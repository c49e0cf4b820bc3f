"""CPU: the nature run (include/spdy.h, "nature run") without a device -- its NumPy restatement (tests/nature.py)
against closed forms, the library's argument checks and their order on a host-only plan, the lifetime rule of the new object
(modelled on tests/test_plan_objects_cpu.py), and the twin condition on the restatement alone: the analysis of observations drawn
from a truth brings the ensemble mean closer to that truth."""
from support import package
import ctypes

import numpy as np
import pytest

import letkf as lk
import nature as nt
import sppt

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
KX, NMEM = 5, 3
MAX_BATCH = NMEM * (2 * KX + 1)
SEED = 0x5EED0123456789AB
EPS = lk.EPS


def host_plan(kx=KX, max_batch=MAX_BATCH):
    sp = package().Spectral("t30", kx=kx, max_batch=max_batch, device=-1)
    if kx not in (5, 8):
        sp.set_sigma(nt.twin_sigma(kx))
    return sp


@pytest.fixture(scope="module")
def geo():
    sp = host_plan()
    g, w = lk.Geometry(sp), nt.gaussian_weights(sp)
    sp.close()
    return g, w


# ---------------------------------------------------------------------------------------------------- the restatement
def test_weights_sum_to_one(geo):
    """the normalised Gaussian weights sum to 1 within 2 eps, summed exactly (math.fsum) and in the order the scores use"""
    import math
    for tag in ("t30", "t63"):
        sp = package().Spectral(tag, kx=8, max_batch=8, device=-1)
        gw = nt.normalised(nt.gaussian_weights(sp))
        sp.close()
        s = 0.0
        for w in gw:
            s = s + w
        print("[nature weights %s] exact sum - 1 = %.2e, ascending sum - 1 = %.2e" % (tag, math.fsum(gw) - 1.0, s - 1.0))
        assert gw.shape == (sp.il,) and (gw > 0).all() and np.array_equal(gw, gw[::-1])
        assert abs(math.fsum(gw) - 1.0) <= 2 * EPS and abs(s - 1.0) <= 2 * EPS


def test_scores_closed_form(geo):
    """x_e = truth + c_e with a constant c_e per member and row: bias = mean(c), rmse = |mean(c)|, spread = std(c, ddof=1), each
    within 8 eps max|c|.  Truth and constants are multiples of 2^-10 below 2^10, so truth + c_e is exact and the bound is about
    the scores' own arithmetic: the sum over E members, the division, the weighted mean over the grid (the weights sum to 1 within
    2 eps) and the root."""
    g, w = geo
    E = 5
    rng = np.random.default_rng(5)
    grid = lambda *shape: rng.integers(-2 ** 19, 2 ** 19, shape) / 1024.0
    truth = {v: grid(g.kx, g.il, g.ix) if v != "ps" else grid(g.il, g.ix) for v in lk.VARS}
    c = {v: rng.integers(-4096, 4096, (E, g.kx if v != "ps" else 1)) / 1024.0 for v in lk.VARS}
    x = {v: truth[v][None] + (c[v][:, :, None, None] if v != "ps" else c[v][:, 0, None, None]) for v in lk.VARS}
    got = nt.scores(g, x, truth, w)
    worst = 0.0
    for v in lk.VARS:
        cm = np.max(np.abs(c[v]))
        want = {"bias": c[v].mean(axis=0), "rmse": np.abs(c[v].mean(axis=0)), "spread": c[v].std(axis=0, ddof=1)}
        for n in nt.SCORES:
            err = float(np.max(np.abs(np.atleast_1d(got[n][v]) - want[n]))) / (8 * EPS * cm)
            worst = max(worst, err)
            assert err <= 1.0, (v, n, err)
    print("[nature closed form] worst error / (8 eps max|c|): %.3f" % worst)
    # every member equal to the truth: exactly zero, the reason the mean is formed on the errors
    zero = nt.scores(g, {v: np.repeat(truth[v][None], 3, axis=0) for v in lk.VARS}, truth, w)
    assert not nt.flat(zero).any()


def test_observe_noise_free_and_noise(geo):
    """noise = 0 gives H(truth) to the bit; the noise of draw d is raw_noise(seed, d, nobs).real, times noise * error; it does not
    depend on nobs: the first n of a longer draw are the shorter draw"""
    g, _ = geo
    x = lk.ensemble(g, 1, seed=3)
    truth = nt.as_truth(x)
    obs = lk.edge_obs(g, x)
    n = len(obs["var"])
    h = lk.observe(g, x, obs)[0]
    clean = nt.observe(g, truth, obs, obs["error"], SEED, 0, 0.0)
    assert np.array_equal(clean, h[:, 0]) and np.array_equal(clean, nt.operator(g, truth, obs))
    for d in (0, 1, 2 ** 32 + 5):
        z = sppt.raw_noise(SEED, d, n).real
        for noise in (1.0, 0.37):
            assert np.array_equal(nt.observe(g, truth, obs, obs["error"], SEED, d, noise), clean + (noise * obs["error"]) * z)
        assert np.array_equal(nt.draw(SEED, d, n), z) and np.array_equal(nt.draw(SEED, d, 7), z[:7])
        assert np.array_equal(sppt.raw_noise(SEED, d, 3 * n).real[:n], z)
    assert not np.array_equal(nt.draw(SEED, 0, n), nt.draw(SEED, 1, n)) and not np.array_equal(nt.draw(SEED, 0, n), nt.draw(SEED + 1, 0, n))
    z = nt.draw(SEED, 0, 20000)
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03
    assert nt.observe(g, truth, lk.make_obs([], [], [], [], [], []), np.zeros(0), SEED, 0, 1.0).shape == (0,)


# ---------------------------------------------------------------------------------------------------- the library, host-only
class Handles:
    """a nature run and analysis objects of its plan, of another plan and of a destroyed plan"""

    def __init__(self):
        s = package()
        self.lib = s.load()
        self.sp, self.other, gone = host_plan(), host_plan(), host_plan()
        self.nat = s.Nature(self.sp, seed=SEED, capacity=2)
        self.lt, self.lt_other, self.lt_gone = (s.Letkf(p, NMEM, 8, 1.0e6) for p in (self.sp, self.other, gone))
        gone.close()
        self.buf = np.zeros(16)
        self.q = self.buf.ctypes.data_as(ctypes.c_void_p)      # a non-null "device pointer": no check dereferences one
        self.ll, self.ptr = ctypes.c_longlong(-1), ctypes.c_void_p()

    def close(self):
        for o in (self.nat, self.lt, self.lt_other, self.lt_gone, self.sp, self.other):
            o.close()


@pytest.fixture()
def hs():
    h = Handles()
    yield h
    h.close()


def refused(lib, rc, code, text):
    assert rc == code and text in lib.spdy_last_error(), (rc, lib.spdy_last_error())


def test_create_checks():
    s = package()
    lib = s.load()
    sp, small = host_plan(), host_plan(max_batch=2 * KX)
    h = ctypes.c_void_p()
    refused(lib, lib.spdy_nature_create(None, 1, 2, ctypes.byref(h)), ERR_ARG, b"null plan")
    refused(lib, lib.spdy_nature_create(sp.h, 1, 0, None), ERR_ARG, b"capacity=0 < 1")
    refused(lib, lib.spdy_nature_create(sp.h, 1, -1, ctypes.byref(h)), ERR_ARG, b"capacity=-1 < 1")
    refused(lib, lib.spdy_nature_create(sp.h, 1, 2, None), ERR_ARG, b"null result pointer")
    refused(lib, lib.spdy_nature_create(small.h, 1, 2, ctypes.byref(h)), ERR_ARG, b"max_batch=10 must be >= 2*kx+1=11")
    assert not h.value
    with pytest.raises(s.SpdyError) as e:
        s.Nature(sp, capacity=0)
    assert e.value.code == ERR_ARG
    nat = s.Nature(sp, seed=-1)                   # any 64-bit pattern is a seed
    assert nat.capacity == 2 and nat.PREFIX == "spdy_nature" and issubclass(s.Nature, s.columns.PlanObject)
    nat.close(); nat.close()
    sp.close(); small.close()


def test_every_rejection_and_its_order(hs):
    """the object, then the analysis object (null, dead, of another plan), then the arguments, the device last: each call is given
    everything that is wrong after the check under test as well, and reports the first"""
    lib, n, q, l = hs.lib, hs.nat.h, hs.q, hs.lt.h
    ref = ctypes.byref
    # a null nature run, whatever else is wrong
    for rc in (lib.spdy_nature_reset(None, 1), lib.spdy_nature_draws(None, None), lib.spdy_nature_field(None, None, None),
               lib.spdy_nature_set_state_dev(None, None, q, q, q, q), lib.spdy_nature_observe_dev(None, None, -1.0),
               lib.spdy_nature_verify_dev(None, None, q, q, q, q, q, 9), lib.spdy_nature_verify_grid_dev(None, 0, q, q, q, q, q, 9)):
        assert rc == ERR_ARG and lib.spdy_last_error() == b"null nature run"
    # the analysis object
    refused(lib, lib.spdy_nature_observe_dev(n, None, -1.0), ERR_ARG, b"null analysis object")
    refused(lib, lib.spdy_nature_verify_dev(n, None, None, q, q, q, q, 9), ERR_ARG, b"null analysis object")
    refused(lib, lib.spdy_nature_observe_dev(n, hs.lt_gone.h, -1.0), ERR_STATE, b"has been destroyed")
    refused(lib, lib.spdy_nature_verify_dev(n, hs.lt_gone.h, None, q, q, q, q, 9), ERR_STATE, b"has been destroyed")
    refused(lib, lib.spdy_nature_observe_dev(n, hs.lt_other.h, -1.0), ERR_ARG, b"the analysis object belongs to another plan")
    refused(lib, lib.spdy_nature_verify_dev(n, hs.lt_other.h, None, q, q, q, q, 9), ERR_ARG, b"the analysis object belongs to another plan")
    # the arguments
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        refused(lib, lib.spdy_nature_observe_dev(n, l, bad), ERR_ARG, b"nature_observe: noise must be finite and >= 0")
    for slot in (-1, 2, 1 << 20):
        refused(lib, lib.spdy_nature_verify_dev(n, l, None, q, q, q, q, slot), ERR_ARG,
                b"nature_verify: slot=%d outside [0, capacity=2)" % slot)
    for at in range(5):
        a = [q] * 5
        a[at] = None
        refused(lib, lib.spdy_nature_verify_dev(n, l, *a, 1), ERR_ARG, b"null device pointer")
        refused(lib, lib.spdy_nature_set_state_dev(n, *a), ERR_ARG, b"null device pointer")
        refused(lib, lib.spdy_nature_verify_grid_dev(n, NMEM, *a, 0), ERR_ARG, b"null device pointer")
    for nmem in (1, 0, 33):
        refused(lib, lib.spdy_nature_verify_grid_dev(n, nmem, None, q, q, q, q, 9), ERR_ARG,
                b"nature_verify_grid: nmem=%d outside [2, 32]" % nmem)
    refused(lib, lib.spdy_nature_verify_grid_dev(n, 2, None, q, q, q, q, 2), ERR_ARG, b"nature_verify_grid: slot=2 outside [0, capacity=2)")
    refused(lib, lib.spdy_nature_draws(n, None), ERR_ARG, b"null result pointer")
    refused(lib, lib.spdy_nature_field(n, None, ref(hs.ptr)), ERR_ARG, b"null name or result pointer")
    refused(lib, lib.spdy_nature_field(n, b"truth", None), ERR_ARG, b"null name or result pointer")
    refused(lib, lib.spdy_nature_field(n, b"hx", ref(hs.ptr)), ERR_ARG, b"unknown nature field 'hx'")
    # the device last: every argument check has passed
    for rc in (lib.spdy_nature_reset(n, 1), lib.spdy_nature_draws(n, ref(hs.ll)), lib.spdy_nature_field(n, b"truth", ref(hs.ptr)),
               lib.spdy_nature_field(n, b"scores", ref(hs.ptr)), lib.spdy_nature_field(n, b"state", ref(hs.ptr)),
               lib.spdy_nature_set_state_dev(n, q, q, q, q, q), lib.spdy_nature_observe_dev(n, l, 0.0),
               lib.spdy_nature_observe_dev(n, l, 2.5), lib.spdy_nature_verify_dev(n, l, q, q, q, q, q, 0),
               lib.spdy_nature_verify_dev(n, l, q, q, q, q, q, 1), lib.spdy_nature_verify_grid_dev(n, 32, q, q, q, q, q, 1)):
        assert rc == ERR_NO_DEVICE and lib.spdy_last_error().startswith(b"host-only plan"), (rc, lib.spdy_last_error())
    assert hs.ll.value == -1 and not hs.ptr.value


def test_python_side_checks(hs):
    """the wrapper's own checks need no device: a Letkf of another plan, a member count that is not the ensemble's"""
    s = package()
    with pytest.raises(ValueError):
        hs.nat.observe(hs.lt_other)
    with pytest.raises(ValueError):
        hs.nat.verify(hs.lt_other, None, None, None, None, None)
    with pytest.raises(ValueError):
        hs.nat.scores(slot=2)
    assert s.Ensemble.verify.__doc__ and s.nature.NATURE_FIELDS == ("truth", "scores", "state")


# ---------------------------------------------------------------------------------------------------- the lifetime rule
def entry_points():
    """every spdy_nature_* call the binding declares, but _create and _destroy"""
    names = [n for n in package()._lib.SIGNATURES if n.startswith("spdy_nature_")]
    return sorted(n for n in names if not n.endswith(("_create", "_destroy")))


def arguments(hs):
    """the arguments after the handle of every entry point: valid on a live plan"""
    q, ref = hs.q, ctypes.byref
    return {"spdy_nature_reset": (7,), "spdy_nature_draws": (ref(hs.ll),), "spdy_nature_field": (b"scores", ref(hs.ptr)),
            "spdy_nature_set_state_dev": (q,) * 5, "spdy_nature_observe_dev": (hs.lt.h, 1.0),
            "spdy_nature_verify_dev": (hs.lt.h, q, q, q, q, q, 1), "spdy_nature_verify_grid_dev": (NMEM, q, q, q, q, q, 1)}


def test_every_entry_point_of_a_dead_nature_run_is_refused(hs):
    lib, of, names = hs.lib, arguments(hs), entry_points()
    assert len(names) >= 6 and not [n for n in names if n not in of], "entry points without arguments in this test"
    for n in names:      # valid while the plan lives: the call reaches the check of the device, which comes last
        rc = getattr(lib, n)(hs.nat.h, *of[n])
        assert rc == ERR_NO_DEVICE, (n, rc, lib.spdy_last_error())
    assert lib.spdy_plan_destroy(hs.sp.h) == OK
    hs.sp.h = None
    for n in names:
        rc = getattr(lib, n)(hs.nat.h, *of[n])
        assert rc == ERR_STATE, (n, rc, lib.spdy_last_error())
        assert b"has been destroyed" in lib.spdy_last_error() and b"plan this nature run" in lib.spdy_last_error(), n
    assert lib.spdy_nature_destroy(hs.nat.h) == OK and lib.spdy_nature_destroy(None) == OK
    hs.nat.h = None


def test_live_nature_run_with_a_dead_analysis_object(hs):
    lib, q = hs.lib, hs.q
    for rc in (lib.spdy_nature_observe_dev(hs.nat.h, hs.lt_gone.h, 1.0), lib.spdy_nature_verify_dev(hs.nat.h, hs.lt_gone.h, q, q, q, q, q, 0)):
        assert rc == ERR_STATE and b"plan this analysis object was made on has been destroyed" in lib.spdy_last_error()
    # and the other way round: the analysis object lives, the nature run's plan is gone
    gone = host_plan()
    nat = package().Nature(gone)
    gone.close()
    refused(lib, lib.spdy_nature_observe_dev(nat.h, hs.lt.h, 1.0), ERR_STATE, b"plan this nature run was made on has been destroyed")
    nat.close()


def test_destroy_in_either_order():
    s = package()
    lib = s.load()
    for plan_first in (False, True):
        sp = host_plan()
        objs = [s.Nature(sp, seed=e, capacity=1 + e) for e in range(3)] + [s.Letkf(sp, NMEM, 4, 1.0e6)]
        if plan_first:
            assert lib.spdy_plan_destroy(sp.h) == OK
            sp.h = None
        for o in objs:
            o.close()
        sp.close()
    sp = host_plan()
    for _ in range(50):                           # an object that stayed on the plan's list would be written to at its end
        s.Nature(sp).close()
    keep = s.Nature(sp)
    assert lib.spdy_plan_destroy(sp.h) == OK
    sp.h = None
    keep.close()


# ---------------------------------------------------------------------------------------------------- the twin condition
@pytest.fixture(scope="module")
def twin():
    """the twin experiment of tests/nature.py on the restatement, computed once: background and analysis scores"""
    c = nt.TWIN
    sp = host_plan(c["kx"], 64)
    g, w = lk.Geometry(sp), nt.gaussian_weights(sp)
    sp.close()
    truth, x, net = nt.twin_inputs(g)
    obs = dict(net)
    obs["value"] = nt.observe(g, truth, net, net["error"], c["noise_seed"], 0, 1.0)
    inc, kappa = lk.analyse(g, x, obs, c["sigma_h"], c["sigma_v"], c["rho"])
    return {"background": nt.scores(g, x, truth, w), "analysis": nt.scores(g, nt.analysed(x, inc, g), truth, w), "kappa": kappa}


def test_twin_condition_on_the_restatement(twin):
    """T30, kx = 2, E = 6, 400 observations of t and ps with noise = 1 (tests/nature.py, twin_inputs): the analysis' rmse of t at
    both levels and of ps is below the background's.  Measured ratios analysis / background: t 0.608 and 0.428, ps 0.395.  The spread of t and
    ps shrinks with it."""
    b, a = twin["background"], twin["analysis"]
    ratio = {"t": a["rmse"]["t"] / b["rmse"]["t"], "ps": a["rmse"]["ps"] / b["rmse"]["ps"]}
    print("[nature twin, restatement] kappa %.1f, rmse analysis / background: t %s, ps %.3f; spread / rmse of the analysis: t %s"
          % (twin["kappa"], np.round(ratio["t"], 3), ratio["ps"], np.round(a["spread"]["t"] / a["rmse"]["t"], 3)))
    assert (a["rmse"]["t"] < b["rmse"]["t"]).all() and a["rmse"]["ps"] < b["rmse"]["ps"]
    assert (a["spread"]["t"] < b["spread"]["t"]).all() and a["spread"]["ps"] < b["spread"]["ps"]
