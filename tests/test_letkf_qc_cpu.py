"""CPU: the background check and the observation statistics without a device (include/spdy.h, "background check and observation
statistics").  The NumPy restatement (tests/letkfqc.py) against closed forms: one observation with E = 2 on either
side of dep^2 == g2 v, a rejected observation's local problems against those of the network without it, the statistics of a
hand-made set.  Then the library on a host-only plan: the checks of the four calls and their order, a rejected call changing
nothing, and the binding surface."""
import ctypes
import math

import numpy as np
import pytest

import letkf as lk
import letkfqc as qc
import support

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
SIGMA_V = 0.1
QC_CALLS = ("spdy_qc_set", "spdy_qc_set_slot", "spdy_qc_stats_grid_dev", "spdy_qc_stats_dev")


@pytest.fixture(scope="module")
def host():
    """T30 L8 without a device and an analysis object of three members with four observations on it"""
    s = support.package()
    sp = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    lt = s.Letkf(sp, 3, 4, 1.0e6)
    lt.set_obs([0, 1, 2, 4], [0, 1, 2, 0], [10.0, 20.0, 30.0, 40.0], [0.0, 10.0, 20.0, 30.0], [1.0] * 4, [1.0] * 4)
    yield s, sp, lt
    lt.close()
    sp.close()


# ---------------------------------------------------------------------------------------------------- the restatement
def test_one_observation_on_either_side_of_the_threshold():
    """E = 2, y = (2, -2): s2 = 8; err = 1: v = 9; gross = 2: g2 v = 36.  dep = +-6 has dep^2 == g2 v and passes (the test is a
    strict one), the next double outside is rejected, the next inside passes; a NaN departure is not rejected; out of column wins"""
    y, err = np.array([[2.0, -2.0]]), np.array([1.0])
    for sign in (1.0, -1.0):
        on = qc.check(y, [sign * 6.0], err, 2.0)
        assert on["s2"][0] == 8.0 and on["v"][0] == 9.0 and not on["rej"][0] and on["used"][0] and on["check"][0] == qc.PASSED
        out = qc.check(y, [sign * math.nextafter(6.0, math.inf)], err, 2.0)
        assert out["rej"][0] and not out["used"][0] and out["check"][0] == qc.REJECTED
        assert qc.check(y, [sign * math.nextafter(6.0, 0.0)], err, 2.0)["used"][0]
    nan = qc.check(y, [math.nan], err, 2.0)
    assert not nan["rej"][0] and nan["used"][0]
    far = qc.check(y, [100.0], err, 2.0, in_column=[0.0])
    assert far["rej"][0] and far["check"][0] == qc.OUT and not far["used"][0]
    assert qc.check(y, [1.0], err, 2.0, in_column=[0.0])["check"][0] == qc.OUT
    assert (qc.reff(np.array([True, False]), np.array([4.0, 4.0])) == [4.0, 0.0]).all()


def test_no_test_without_two_members_or_with_gross_zero():
    """n < 2 (a mask that leaves one member, or none) and gross == 0: nothing is rejected, whatever the departure"""
    y = np.array([[2.0, -2.0, 0.5]])
    for keep in ((1,), ()):
        assert qc.check(y, [1e9], [1.0], 2.0, keep=keep)["used"][0]
    assert qc.check(y, [1e9], [1.0], 0.0)["used"][0]
    assert not qc.check(y, [1e9], [1.0], 2.0)["used"][0]
    # the members in use only: y of member 2 enters nothing
    a, b = qc.check(y, [5.0], [1.0], 2.0, keep=(0, 1)), qc.check(y[:, :2], [5.0], [1.0], 2.0)
    assert a["s2"][0] == b["s2"][0] == 8.0 and a["check"][0] == b["check"][0]


def test_rejected_observation_takes_no_part():
    """the local problems of the checked network are, bit for bit, those of the network without the rejected observations: a
    rejected observation has r exactly 0 and enters no sum"""
    s = support.package()
    sp = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    g = lk.Geometry(sp)
    sp.close()
    E = 5
    x = lk.ensemble(g, E, seed=3)
    obs = lk.clustered_obs(g, x, n=120)
    sp0 = lk.obs_space(g, x, obs)
    obs["value"], outside, inside = qc.plant(obs, sp0["hxmean"], qc.spread2(sp0["y"]), 3.0, seed=1)
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=12, outside=2)
    sp1 = lk.obs_space(g, x, obs)
    dec = qc.check(sp1["y"], sp1["departure"], obs["error"], 3.0)
    assert not dec["used"][outside].any() and dec["used"][inside].all() and len(outside) == len(inside) == 10
    r_eff = qc.reff(dec["used"], 1.0 / (obs["error"] * obs["error"]))
    C, b = lk.problems(g, obs, sp1, lk.SIGMA_H, SIGMA_V, cols, r_eff=r_eff)
    used = lk.subset(obs, dec["used"])
    Cs, bs = lk.problems(g, used, lk.obs_space(g, x, used), lk.SIGMA_H, SIGMA_V, cols)
    Ca, _ = lk.problems(g, obs, sp1, lk.SIGMA_H, SIGMA_V, cols)
    assert support.same_bits(C, Cs) and support.same_bits(b, bs) and not support.same_bits(C, Ca)
    sp2 = lk.obs_space(g, x, obs)                  # the checked analysis: the decisions on the restatement's own y and departure
    dec2 = qc.check(sp2["y"], sp2["departure"], obs["error"], 3.0)
    dx, _ = lk.analyse(g, x, obs, lk.SIGMA_H, SIGMA_V, lk.RHO, cols=cols, r_eff=qc.reff(dec2["used"], 1.0 / (obs["error"] * obs["error"])))
    ref, _ = lk.analyse(g, x, used, lk.SIGMA_H, SIGMA_V, lk.RHO, cols=cols)
    assert (dec2["check"] == dec["check"]).all()
    for v in lk.VARS:
        assert support.same_bits(dx[v], ref[v]) and dx[v].any(), v


def test_statistics_of_a_hand_made_set():
    """seven observations in groups 0, 2, 3 of four (group 1 is empty): small integers, so every sum is exact in any order"""
    group = np.array([0, 2, 2, 3, 0, 2, 3])
    code = np.array([0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    dep = np.array([1.0, 2.0, 50.0, 3.0, -3.0, 4.0, 5.0])
    s2 = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    err = np.array([1.0, 2.0, 1.0, 1.0, 3.0, 1.0, 2.0])
    depb = np.array([2.0, 1.0, 9.0, 9.0, 1.0, -1.0, 3.0])
    got = qc.stats(group, 4, code, dep, s2, err)
    want = np.array([[2, 0, 0, 2, -2, 10, 6, 10, 10, -2],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [3, 0, 1, 2, 6, 20, 8, 5, 20, 6],
                     [2, 1, 0, 1, 5, 25, 7, 4, 25, 5]], np.float64)
    assert support.same_bits(got, want)
    assert not got[1].view(np.int64).any()                 # exact zeros, +0.0
    oa = qc.stats(group, 4, code, dep, s2, err, depb)
    assert (oa[:, :8] == want[:, :8]).all()
    assert (oa[:, 8] == [2.0 - 3.0, 0.0, 2.0 - 4.0, 15.0]).all() and (oa[:, 9] == [3.0, 0.0, 0.0, 3.0]).all()
    # a non-finite value stays in its group's row
    dep[1] = np.nan
    bad = qc.stats(group, 4, code, dep, s2, err)
    assert np.isnan(bad[2, [4, 5, 8, 9]]).all() and support.same_bits(bad[[0, 1, 3]], want[[0, 1, 3]]) and (bad[2, :4] == want[2, :4]).all()


def test_summation_order_is_the_headers():
    """2600 observations in one group: the tree's sum is the one of 1024 strided partials and a halving tree, written out here
    with plain Python floats, and is within N eps sum|terms| of the exact sum"""
    rng = np.random.default_rng(8)
    t = rng.standard_normal(2600) * 10.0 ** rng.uniform(-3, 3, 2600)
    part = [0.0] * 1024
    for o in range(2600):
        part[o % 1024] = part[o % 1024] + t[o]
    h = 512
    while h:
        for i in range(h):
            part[i] = part[i] + part[i + h]
        h //= 2
    got = qc.tree(t, np.ones(2600, bool))
    assert got == part[0] and abs(got - math.fsum(t)) <= 2600 * lk.EPS * np.abs(t).sum()
    assert qc.tree(t, np.zeros(2600, bool)) == 0.0


# ---------------------------------------------------------------------------------------------------- the library, host-only
def _state(lib, lt):
    """"off", or "on": which refusal the stats-only call gives on a host-only plan (it can never have analysed)"""
    d = ctypes.c_void_p(8)
    assert lib.spdy_qc_stats_grid_dev(lt.h, d, d, d, d, d, None, 0) == ERR_STATE
    msg = lib.spdy_last_error()
    assert b"spdy_qc_set first" in msg or b"no analysis call with the check on" in msg, msg
    return "off" if b"spdy_qc_set first" in msg else "on"


def test_set_rejects_and_accepts_in_order(host):
    """a NULL object, a destroyed plan, gross, ngroups, the first entry out of range -- in this order; a rejected call changes
    nothing; an accepted one is stored on a host-only plan, where nothing is allocated"""
    s, sp, lt = host
    lib = s.load()
    call = lib.spdy_qc_set
    grp = (ctypes.c_int * 4)(0, 1, 2, 1)
    bad = (ctypes.c_int * 4)(0, 3, -1, 1)
    assert call(None, -1.0, 0, None) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    assert _state(lib, lt) == "off"
    for g in (math.nan, -0.5, math.inf, -math.inf):
        assert call(lt.h, g, 0, bad) == ERR_ARG and b"gross must be finite and >= 0" in lib.spdy_last_error(), g
    for n in (0, -1, 65):
        assert call(lt.h, 1.0, n, bad) == ERR_ARG and b"ngroups=" in lib.spdy_last_error(), n
    assert call(lt.h, 1.0, 3, bad) == ERR_ARG and b"observation 1: group=3 outside [0, 3)" in lib.spdy_last_error()
    assert call(lt.h, 1.0, 4, bad) == ERR_ARG and b"observation 2: group=-1" in lib.spdy_last_error()
    assert _state(lib, lt) == "off"                        # nothing has been accepted yet
    assert call(lt.h, 0.0, 99, None) == OK and _state(lib, lt) == "off"      # the default grouping: ngroups is ignored
    assert call(lt.h, 0.0, 3, grp) == OK and _state(lib, lt) == "on"         # statistics without rejection
    assert call(lt.h, 0.0, 0, None) == OK and _state(lib, lt) == "off"
    assert call(lt.h, 4.0, 0, None) == OK and _state(lib, lt) == "on"
    assert call(lt.h, math.nan, 3, grp) == ERR_ARG and _state(lib, lt) == "on"
    # the Python object follows
    lt.set_background_check(0.0)
    assert (lt.gross, lt.ngroups, lt.stats_slot) == (0.0, 5, 0) and _state(lib, lt) == "off"
    lt.set_background_check(5.0, [0, 6, 6, 2], slot=3)
    assert (lt.gross, lt.ngroups, lt.stats_slot) == (5.0, 7, 3) and _state(lib, lt) == "on"
    with pytest.raises(s.SpdyError):
        lt.set_background_check(-1.0)
    with pytest.raises(s.SpdyError):
        lt.set_background_check(1.0, [0, 64, 0, 0])
    with pytest.raises(ValueError):
        lt.set_background_check(1.0, [0, 1, 2])
    assert (lt.gross, lt.ngroups) == (5.0, 7) and _state(lib, lt) == "on"
    # set_obs returns the grouping to the default and keeps gross
    lt.set_background_check(0.0, [0, 1, 1, 0])
    lt.set_obs([0, 1, 2, 4], [0, 1, 2, 0], [10.0, 20.0, 30.0, 40.0], [0.0, 10.0, 20.0, 30.0], [1.0] * 4, [1.0] * 4)
    assert lt.ngroups == 5 and _state(lib, lt) == "off"
    lt.set_background_check(0.0)


def test_slot_and_stats_calls_check_in_order(host):
    s, sp, lt = host
    lib = s.load()
    d = ctypes.c_void_p(8)
    assert lib.spdy_qc_set_slot(None, 0) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
    for slot in (-1, 4):
        assert lib.spdy_qc_set_slot(lt.h, slot) == ERR_ARG and b"outside [0, 4)" in lib.spdy_last_error()
    for slot in (3, 0):
        assert lib.spdy_qc_set_slot(lt.h, slot) == OK
    for call in (lib.spdy_qc_stats_grid_dev, lib.spdy_qc_stats_dev):
        assert call(None, d, d, d, d, d, None, 0) == ERR_ARG and b"null analysis object" in lib.spdy_last_error()
        lt.set_background_check(0.0)
        assert call(lt.h, None, d, d, d, d, None, 9) == ERR_STATE and b"spdy_qc_set first" in lib.spdy_last_error()
        lt.set_background_check(3.0)
        # no checked analysis yet: the state is refused before the arguments are looked at
        assert call(lt.h, None, d, d, d, d, None, 9) == ERR_STATE and b"no analysis call with the check on" in lib.spdy_last_error()
    lt.set_background_check(0.0)
    p = ctypes.c_void_p()
    for name in (b"obs_check", b"obs_stats"):
        assert lib.spdy_letkf_field(lt.h, name, ctypes.byref(p)) == ERR_NO_DEVICE and not p.value
    gone = s.Spectral("t30", kx=8, max_batch=3 * 32, device=-1)
    dead = s.Letkf(gone, 3, 4, 1.0e6, gross=5.0)
    assert dead.gross == 5.0
    gone.close()
    assert lib.spdy_qc_set(dead.h, 1.0, 0, None) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    assert lib.spdy_qc_set_slot(dead.h, 0) == ERR_STATE
    assert lib.spdy_qc_stats_dev(dead.h, d, d, d, d, d, None, 0) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    dead.close()


def test_entry_points_exist_and_are_bound(host):
    """each new name is declared, exported, bound in Fortran and in SIGNATURES; nothing else carries the prefix"""
    s, sp, lt = host
    lib, sig = s.load(), s._lib.SIGNATURES
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for where in (support.declared(), support.fortran_bound(), set(sig)):
        assert {n for n in where if n.startswith("spdy_qc_")} == set(QC_CALLS)
    assert all(hasattr(lib, n) for n in QC_CALLS)
    assert sig["spdy_qc_set"] == [P, D, I, P] and sig["spdy_qc_set_slot"] == [P, I]
    assert sig["spdy_qc_stats_grid_dev"] == sig["spdy_qc_stats_dev"] == [P] * 7 + [I]
    assert support.declaration("spdy_qc_set") == "spdy_letkf *l, double gross, int ngroups, const int *group"
    assert "enum { SPDY_QC_MAX_GROUPS = 64, SPDY_QC_SLOTS = 4 };" in support.header()
    assert "SPDY_QC_MAX_GROUPS = 64_c_int, SPDY_QC_SLOTS = 4_c_int" in support.fortran_binding()
    assert (s.letkf.QC_MAX_GROUPS, s.letkf.QC_SLOTS) == (64, 4) and s.letkf.QC_COLUMNS == qc.COLUMNS
    assert "obs_check" in s.letkf.LETKF_FIELDS and "obs_stats" in s.letkf.LETKF_FIELDS
    assert "background check and observation statistics" in support.header(comments=True)
    assert s.Letkf.set_background_check.__doc__ and s.Letkf.obs_stats.__doc__ and s.Ensemble.obs_stats.__doc__
