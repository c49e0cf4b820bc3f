"""CPU: the conditions the twin cycle of tests/twincycle.py meets on the host reference alone -- what tests/test_nature_cpu.py does
for the one-shot twin.  They are what lets tests/test_gpu_twin_cycle.py tell a right cycle from one with a dating error: the slot
analysis of real forecasts beats its background, the same values dated at the analysis time do worse than no analysis, the cycle
survives its restart, and a member's H x moves by far more than rounding from one step to the next."""
import numpy as np
import pytest

import dynstep
import letkf as lk
import nature as nt
import support
import twincycle as tc
from conftest import TOL


@pytest.fixture(scope="module")
def cycle(oracle_factory):
    """the two windows on the host, computed once (about 7 s), read only"""
    support.package()
    sp = support.plan(tc.TAG, max_batch=4, device=-1)
    g, w = lk.Geometry(sp), nt.gaussian_weights(sp)
    sp.close()
    return g, tc.cycle(oracle_factory(tc.TAG), g, w)


def test_everything_is_finite(cycle):
    """the spectra and the gridded ensembles at every step of both windows, the values, the increments and every score"""
    _, c = cycle
    for n, win in enumerate(c["windows"]):
        for sts in win["members"] + [win["truth"], win["analysed"]]:
            for st in sts:
                assert all(np.isfinite(st[k].real).all() and np.isfinite(st[k].imag).all() for k in dynstep.PROG), n
        for x in win["x"] + win["xt"] + [win["xa"], win["inc"]]:
            assert all(np.isfinite(x[v]).all() for v in lk.VARS), n
        assert np.isfinite(win["obs"]["value"]).all() and np.isfinite(win["kappa"])
        assert all(np.isfinite(a).all() for a in win["obs_space"].values()), n
        assert np.isfinite(nt.flat(win["scores"]["background"])).all() and np.isfinite(nt.flat(win["scores"]["analysis"])).all(), n
    assert np.isfinite(nt.flat(c["windows"][0]["misdated"]["scores"])).all() and np.isfinite(nt.flat(c["free"])).all()


def test_slots_beat_the_background_and_misdating_does_not(cycle):
    """First window, rmse of the analysis over rmse of the background, the mean over the levels.  Measured at E = 12: slots at their
    own times u 0.706, t 0.561, ps 0.672; the same values with every H x taken at the analysis time u 3.415, t 2.231, ps 3.425.
    Each is asserted at the midpoint between the measured value and 1 (tests/twincycle.py, THRESHOLD): the device differs from this
    reference by rounding, a dating error lands on the other side of 1"""
    _, c = cycle
    win = c["windows"][0]
    good = tc.ratios(win["scores"]["analysis"], win["scores"]["background"])
    bad = tc.ratios(win["misdated"]["scores"], win["scores"]["background"])
    print("[twin cycle, host] window 0, kappa %.1f, rmse analysis / background: 4D %s; misdated %s"
          % (win["kappa"], " ".join("%s %.3f" % kv for kv in good.items()), " ".join("%s %.3f" % kv for kv in bad.items())))
    for v in tc.SCORED:
        assert good[v] <= tc.THRESHOLD["4d"][v] < 1.0, (v, good[v])
        assert bad[v] >= tc.THRESHOLD["misdated"][v] > 1.0, (v, bad[v])


def test_the_cycle_survives_its_restart(cycle):
    """Second window, after the members started up again from the analysed time level 1: the background's rmse of t and ps over that
    of the members that were never analysed.  Measured: t 0.834, ps 0.912 (u 0.768); asserted at the midpoint to 1.  The second
    analysis' own ratios are printed, not asserted: t 0.803, ps 0.815, u 1.301 -- twelve members without drag or inflation"""
    _, c = cycle
    win = c["windows"][1]
    r = tc.ratios(win["scores"]["background"], c["free"])
    print("[twin cycle, host] window 1, kappa %.1f, rmse background / free run: %s; analysis / background: %s"
          % (win["kappa"], " ".join("%s %.3f" % kv for kv in r.items()),
             " ".join("%s %.3f" % kv for kv in tc.ratios(win["scores"]["analysis"], win["scores"]["background"]).items())))
    for v in ("t", "ps"):
        assert r[v] <= tc.THRESHOLD["restart"][v] < 1.0, (v, r[v])


def test_a_step_moves_hx_far_beyond_rounding(cycle):
    """For every slot of both windows and every observed variable: max |hx(step n) - hx(step n +- 1)| over the slot's rows is at
    least 1e6 TOL of the variable's scale -- the condition that lets the GPU test tell the dates apart.  Measured: 3.6e-3 (t) at the
    least, 0.13 to 0.30 for the wind, against the 1e-6 asked"""
    g, c = cycle
    for n, win in enumerate(c["windows"]):
        sep = tc.separation(g, win, c["net"])
        print("[twin cycle, host] window %d, step-to-step separation of hx / scale: %s"
              % (n, " ".join("%d:%s %.1e" % (k + (r,)) for k, r in sep.items())))
        assert len(sep) == 12 and min(sep.values()) >= 1e6 * TOL, (n, sep)


def test_the_network_and_the_draws(cycle):
    """three slots of 200, every observed variable in each; the second window's values are other draws on another truth"""
    _, c = cycle
    net = c["net"]
    for s in range(3):
        assert sorted(set(net["var"][tc.rows(s)].tolist())) == sorted(tc.OBSERVED)
    assert (net["lev"][net["var"] == lk.PS] == 0).all() and set(net["lev"].tolist()) == set(range(5))
    assert not np.array_equal(c["windows"][0]["obs"]["value"], c["windows"][1]["obs"]["value"])
