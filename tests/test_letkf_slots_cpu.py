"""CPU: observations in time slots (include/spdy.h, "ensemble analysis, observations in time slots") -- the
identities of the NumPy restatement (tests/letkfslots.py) against tests/letkf.py and tests/letkfpressure.py, every check of every new
call on a host-only plan in the documented order, the wrappers' own checks, and the binding surface."""
import ctypes

import numpy as np
import pytest

import letkf as lk
import letkfpressure as lp
import letkfslots as ls
import support
from support import package

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
KX, NMEM, MAX_OBS = 8, 3, 40
SIGMA_V = 0.1


@pytest.fixture(scope="module")
def plan():
    sp = package().Spectral("t30", kx=KX, max_batch=NMEM * (2 * KX + 1), device=-1)
    yield sp, lp.Geometry(sp)
    sp.close()


# ---------------------------------------------------------------------------------------------------- the restatement
def same_dict(a, b, names):
    for n in names:
        assert support.same_bits(a[n], b[n]), n


def test_same_state_is_the_plain_analysis(plan):
    """statements 1 and 4, model-level: every slot on the analysed ensemble gives lk.obs_space's fields, lk.problems' C and b and
    lk.analyse's increments bit for bit, with the ranges of the GPU test, with one slot, and with no observation at all"""
    _, g = plan
    E = 4
    x = lk.ensemble(g, E, seed=2)
    obs = lk.concat(lk.clustered_obs(g, x, n=320), lk.sparse_obs(g, x))
    n = len(obs["var"])
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=12, outside=4)
    plain = lk.obs_space(g, x, obs)
    Cp, bp = lk.problems(g, obs, plain, lk.SIGMA_H, SIGMA_V, cols)
    want, _ = lk.analyse(g, x, obs, lk.SIGMA_H, SIGMA_V, lk.RHO, cols=cols)
    for first in (ls.FIRST(n), [0, n], [0, 0, n, n]):
        xs = [x] * (len(first) - 1)
        s = lk.obs_space(g, x, obs, xs=xs, first=first)
        C, b = lk.problems(g, obs, s, lk.SIGMA_H, SIGMA_V, cols)
        same_dict(s, dict(plain, obs_lnsigma=lk.lnsigma(g, obs), obs_used=np.ones(n)), lk.FIELDS)
        assert support.same_bits(C, Cp) and support.same_bits(b, bp) and not s["slot_ps"].any() and not s["slot_out"].any()
        got, _ = lk.analyse(g, x, obs, lk.SIGMA_H, SIGMA_V, lk.RHO, cols=cols, xs=xs, first=first)
        same_dict(got, want, lk.VARS)
    none = lk.make_obs([], [], [], [], [], [])
    got, _ = lk.analyse(g, x, none, lk.SIGMA_H, SIGMA_V, 1.0, cols=cols, xs=[x], first=[0, 0])
    want, _ = lk.analyse(g, x, none, lk.SIGMA_H, SIGMA_V, 1.0, cols=cols)
    same_dict(got, want, lk.VARS)
    assert all(np.max(np.abs(a)) <= 64 * E * lk.EPS * lk.perturbation_scale(x)[v] for v, a in got.items())


def test_same_state_is_the_plain_analysis_at_pressure(plan):
    """statement 1 for tests/letkfpressure.py's crafted network: the plain call's fields and its C and b bit for bit; the
    per-member rows say what the shared fields say -- obs_used == 0 exactly where a member's flag is set, and ln sigma_o from the
    mean of slot_ps"""
    _, g = plan
    E = 4
    x = lp.craft(g, E, seed=21)
    obs = lp.network(g, x)
    n = len(obs["var"])
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=12, outside=4)
    want = lk.obs_space(g, x, obs)
    Cp, bp = lk.problems(g, obs, want, lk.SIGMA_H, SIGMA_V, cols)
    assert (want["obs_used"] == 0.0).sum() >= 10
    for first in (ls.FIRST(n), [0, n]):
        s = lk.obs_space(g, x, obs, xs=[x] * (len(first) - 1), first=first)
        C, b = lk.problems(g, obs, s, lk.SIGMA_H, SIGMA_V, cols)
        same_dict(s, want, lk.FIELDS)
        assert support.same_bits(C, Cp) and support.same_bits(b, bp)
        assert np.array_equal(s["slot_out"].any(axis=1), want["obs_used"] == 0.0) and set(np.unique(s["slot_out"])) == {0.0, 1.0}
        assert not s["slot_out"][~lp.at_pressure(obs)].any() and s["slot_ps"].any()


@pytest.mark.parametrize("kind", ["model", "pressure"])
def test_splitting_a_slot_changes_nothing(kind, plan):
    """one slot split in two at any place, both halves on the same ensemble: every field keeps its bits; and the halves on different
    ensembles give, row range by row range, the rows of the unsplit call on either"""
    _, g = plan
    E = 3
    if kind == "model":
        x = lk.ensemble(g, E, seed=4)
        obs = lk.edge_obs(g, x)
    else:
        x = lp.craft(g, E, seed=22)
        obs = lk.subset(lp.network(g, x), slice(0, 60))
    n = len(obs["var"])
    whole = lk.obs_space(g, x, obs, xs=[x], first=[0, n])
    for cut in (0, 1, n // 2, n - 1, n):
        same_dict(lk.obs_space(g, x, obs, xs=[x, x], first=[0, cut, n]), whole, lk.FIELDS + ("slot_ps", "slot_out"))
    y = ls.drifting(g, x, 2, seed=9)[0]
    other, cut = lk.obs_space(g, x, obs, xs=[y], first=[0, n]), n // 3
    mixed = lk.obs_space(g, x, obs, xs=[y, x], first=[0, cut, n])
    for name in ls.SLOT_FIELDS:
        assert support.same_bits(mixed[name][:cut], other[name][:cut]) and support.same_bits(mixed[name][cut:], whole[name][cut:]), name
    assert not support.same_bits(whole["hx"], other["hx"])


def test_late_mask_in_the_restatement(plan):
    """statement 3: with member 1's rows NaN from slot 1 on and the member dropped, every field and the problems are those of the
    two other members observed on the same slots"""
    _, g = plan
    E, keep = 3, (0, 2)
    x = lk.ensemble(g, E, seed=6)
    obs = lk.edge_obs(g, x)
    n = len(obs["var"])
    first = [0, 7, n]
    xs = ls.drifting(g, x, 2, seed=3)
    bad = [xs[0], {v: a.copy() for v, a in xs[1].items()}]
    for v in lk.VARS:
        bad[1][v][1] = np.nan
    s = lk.obs_space(g, x, obs, keep, xs=bad, first=first)
    C, b = lk.problems(g, obs, s, lk.SIGMA_H, SIGMA_V, keep=keep)
    sc = lk.obs_space(g, x, obs, xs=[lk.compact(a, keep) for a in xs], first=first)
    Cc, bc = lk.problems(g, obs, sc, lk.SIGMA_H, SIGMA_V)
    assert support.same_bits(C, Cc) and support.same_bits(b, bc) and np.isfinite(C).all()
    same_dict(s, sc, ls.PER_OBS)
    assert support.same_bits(np.ascontiguousarray(s["y"][:, keep]), sc["y"]) and not s["y"][:, 1].any() and np.isnan(s["hx"][7:, 1]).all()


def test_drifting(plan):
    """the last ensemble is x itself; the difference from x is a fraction of the members' spread and grows towards the first slot"""
    _, g = plan
    x = lk.ensemble(g, 3, seed=1)
    xs = ls.drifting(g, x, 3, seed=5)
    assert len(xs) == 3 and xs[2] is x
    for v in lk.VARS:
        d0, d1 = (xs[0][v] - x[v]).std(), (xs[1][v] - x[v]).std()
        assert abs(d1 / (ls.DRIFT * lk.SCALE[v][1]) - 1.0) < 1e-12 and abs(d0 / d1 - 2.0) < 1e-12, v
    again = ls.drifting(g, x, 3, seed=5)
    assert support.same_bits(xs[0]["t"], again[0]["t"]) and not support.same_bits(xs[0]["t"], ls.drifting(g, x, 3, seed=6)[0]["t"])


# ---------------------------------------------------------------------------------------------------- the library, host-only
class Handles:
    def __init__(self, sp, g):
        s = package()
        self.lib, self.sp = s.load(), sp
        gone = s.Spectral("t30", kx=KX, max_batch=NMEM * (2 * KX + 1), device=-1)
        self.other = s.Spectral("t30", kx=KX, max_batch=NMEM * (2 * KX + 1), device=-1)
        self.lt, self.lt_gone, self.lt_other = (s.Letkf(p, NMEM, MAX_OBS, lk.SIGMA_H) for p in (sp, gone, self.other))
        gone.close()
        self.nat = s.Nature(sp, capacity=1)
        x = lk.ensemble(g, NMEM, seed=1)
        self.obs = lk.subset(lk.edge_obs(g, x), slice(0, 30))
        self.buf = np.zeros(16)
        self.q = self.buf.ctypes.data_as(ctypes.c_void_p)      # a non-null "device pointer": no check dereferences one

    def close(self):
        for o in (self.nat, self.lt, self.lt_gone, self.lt_other, self.other):
            o.close()


@pytest.fixture()
def hs(plan):
    h = Handles(*plan)
    yield h
    h.close()


def refused(lib, rc, code, text):
    assert rc == code and text in lib.spdy_last_error(), (rc, lib.spdy_last_error())


def ints(*v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


def test_slot_set_checks_and_table(hs):
    """spdy_slot_set: every check in the documented order, a rejected call changes nothing, table("slot_first"), and the reset by
    set_obs and by a set with pressures"""
    lib, lt = hs.lib, hs.lt
    lt.set_obs(*lk.args(hs.obs))
    assert lt.nobs == 30 and lt.slots is None and lt.table("slot_first").shape == (0,)
    refused(lib, lib.spdy_slot_set(None, 99, None), ERR_ARG, b"null analysis object")
    refused(lib, lib.spdy_slot_set(hs.lt_gone.h, 99, None), ERR_STATE, b"has been destroyed")
    for n in (-1, 33, 1 << 20):
        refused(lib, lib.spdy_slot_set(lt.h, n, None), ERR_ARG, b"slot_set: nslots=%d outside [0, 32]" % n)
    refused(lib, lib.spdy_slot_set(lt.h, 2, None), ERR_ARG, b"slot_set: null ranges")
    refused(lib, lib.spdy_slot_set(lt.h, 2, ints(1, 0, 31)), ERR_ARG, b"slot_set: first[0]=1 must be 0")
    refused(lib, lib.spdy_slot_set(lt.h, 3, ints(0, 12, 11, 31)), ERR_ARG, b"slot_set: first[2]=11 < first[1]=12")
    refused(lib, lib.spdy_slot_set(lt.h, 2, ints(0, 12, 31)), ERR_ARG, b"slot_set: first[2]=31 must be nobs=30")
    refused(lib, lib.spdy_slot_set(lt.h, 2, ints(0, 12, 29)), ERR_ARG, b"slot_set: first[2]=29 must be nobs=30")
    assert lt.table("slot_first").shape == (0,)
    lt.set_slots([0, 12, 12, 30])
    assert lt.slots == (0, 12, 12, 30) and lt.table("slot_first").tolist() == [0, 12, 12, 30] and lt.table("slot_first").dtype == np.int64
    refused(lib, lib.spdy_slot_set(lt.h, 2, ints(0, 31, 30)), ERR_ARG, b"slot_set: first[2]=30 < first[1]=31")
    assert lt.table("slot_first").tolist() == [0, 12, 12, 30]                       # a rejected call changes nothing
    lt.set_slots(np.arange(0, 31, 1)[[0] + list(range(30)) + [30]])                 # 31 slots, the first one empty
    assert len(lt.slots) == 32 and lt.table("slot_first").shape == (32,)
    lt.set_slots([0] * 32 + [30])                                                   # SPDY_MAX_SLOTS of them
    assert lt.table("slot_first").shape == (33,)
    lt.set_slots(None)
    assert lt.slots is None and lt.table("slot_first").shape == (0,)
    assert lib.spdy_slot_set(lt.h, 0, ints(5, 4)) == OK                             # (0, anything): no slots, first is not read
    for reset in (lambda: lt.set_obs(*lk.args(hs.obs)), lambda: lt.set_obs(*lk.args(hs.obs), p=np.full(30, 5.0e4)),
                  lambda: lt.set_obs(*lk.args(lk.make_obs([], [], [], [], [], [])))):
        lt.set_slots([0, 30] if lt.nobs else [0, 0])
        assert lt.slots is not None and lt.table("slot_first").shape == (2,)
        reset()
        assert lt.slots is None and lt.table("slot_first").shape == (0,)
    lt.set_slots([0, 0, 0])                                                         # nobs == 0: every slot is empty
    assert lt.table("slot_first").tolist() == [0, 0, 0]
    with pytest.raises(package().SpdyError) as e:                                   # a set_obs that is rejected changes nothing
        lt.set_obs([7], [0], [0.0], [0.0], [0.0], [1.0])
    assert e.value.code == ERR_ARG and lt.table("slot_first").tolist() == [0, 0, 0]


def test_dev_calls_check_order(hs):
    """the two observe calls, the two analysis calls and the nature call: every check in its order, the device last"""
    lib, lt, q, nat = hs.lib, hs.lt, hs.q, hs.nat.h
    five, ten = [q] * 5, [q] * 10
    lt.set_obs(*lk.args(hs.obs))
    observe = (lib.spdy_slot_observe_grid_dev, lib.spdy_slot_observe_dev)
    # the object
    for rc in (lib.spdy_slot_observe_grid_dev(None, -1, *[None] * 5), lib.spdy_slot_observe_dev(None, -1, *[None] * 5),
               lib.spdy_slot_analyse_grid_dev(None, *[None] * 10, None), lib.spdy_slot_ens_letkf_dev(None, *[None] * 5, None)):
        assert rc == ERR_ARG and lib.spdy_last_error() == b"null analysis object"
    for rc in (lib.spdy_slot_observe_grid_dev(hs.lt_gone.h, -1, *[None] * 5), lib.spdy_slot_observe_dev(hs.lt_gone.h, -1, *[None] * 5),
               lib.spdy_slot_analyse_grid_dev(hs.lt_gone.h, *[None] * 10, None), lib.spdy_slot_ens_letkf_dev(hs.lt_gone.h, *[None] * 5, None)):
        assert rc == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    # observe: no slots, then the slot, then the pointers
    for call in observe:
        refused(lib, call(lt.h, -1, *[None] * 5), ERR_STATE, b"slot_observe: spdy_slot_set first")
    lt.set_slots([0, 12, 12, 30])
    for call in observe:
        for slot in (-1, 3, 1 << 20):
            refused(lib, call(lt.h, slot, *[None] * 5), ERR_ARG, b"slot_observe: slot=%d outside [0, nslots=3)" % slot)
        for at in range(5):
            a = list(five)
            a[at] = None
            refused(lib, call(lt.h, 1, *a), ERR_ARG, b"null device pointer")
        for slot in (0, 1, 2):
            rc = call(lt.h, slot, *five)
            assert rc == ERR_NO_DEVICE and lib.spdy_last_error().startswith(b"host-only plan"), (slot, rc)
    # the analysis calls: the plain forms' checks (the localisation is set by Letkf's constructor), the pointers, then the slots
    fresh = package().Letkf(hs.sp, NMEM, MAX_OBS, lk.SIGMA_H)
    fresh.set_obs(*lk.args(hs.obs))
    for at in range(10):
        a = list(ten)
        a[at] = None
        refused(lib, lib.spdy_slot_analyse_grid_dev(fresh.h, *a, None), ERR_ARG, b"null device pointer")
    for at in range(5):
        a = list(five)
        a[at] = None
        refused(lib, lib.spdy_slot_ens_letkf_dev(fresh.h, *a, q), ERR_ARG, b"null device pointer")
    refused(lib, lib.spdy_slot_analyse_grid_dev(fresh.h, *ten, None), ERR_STATE, b"slot analysis: spdy_slot_set first")
    refused(lib, lib.spdy_slot_ens_letkf_dev(fresh.h, *five, None), ERR_STATE, b"slot analysis: spdy_slot_set first")
    fresh.set_slots([0, 12, 12, 30])
    # a host-only plan marks nothing (the device check refuses the observe), so slot 0 is the one named; the empty slot never is
    refused(lib, lib.spdy_slot_analyse_grid_dev(fresh.h, *ten, q), ERR_STATE, b"slot analysis: slot 0 has not been observed")
    refused(lib, lib.spdy_slot_ens_letkf_dev(fresh.h, *five, q), ERR_STATE, b"slot analysis: slot 0 has not been observed")
    fresh.set_slots([0, 0, 30])
    refused(lib, lib.spdy_slot_ens_letkf_dev(fresh.h, *five, None), ERR_STATE, b"slot analysis: slot 1 has not been observed")
    fresh.set_obs(*lk.args(lk.make_obs([], [], [], [], [], [])))
    fresh.set_slots([0, 0, 0])                                                      # nothing to observe: the device is all that is missing
    for rc in (lib.spdy_slot_analyse_grid_dev(fresh.h, *ten, None), lib.spdy_slot_ens_letkf_dev(fresh.h, *five, q)):
        assert rc == ERR_NO_DEVICE and lib.spdy_last_error().startswith(b"host-only plan"), rc
    fresh.close()
    # the nature call: spdy_nature_observe_dev's checks, then the slots, then the device
    refused(lib, lib.spdy_slot_nature_observe_dev(None, None, -1, -1.0), ERR_ARG, b"null nature run")
    refused(lib, lib.spdy_slot_nature_observe_dev(nat, None, -1, -1.0), ERR_ARG, b"null analysis object")
    refused(lib, lib.spdy_slot_nature_observe_dev(nat, hs.lt_gone.h, -1, -1.0), ERR_STATE, b"has been destroyed")
    refused(lib, lib.spdy_slot_nature_observe_dev(nat, hs.lt_other.h, -1, -1.0), ERR_ARG, b"the analysis object belongs to another plan")
    for bad in (-1.0, float("nan"), float("inf")):
        refused(lib, lib.spdy_slot_nature_observe_dev(nat, lt.h, -1, bad), ERR_ARG, b"slot_nature_observe: noise must be finite and >= 0")
    lt.set_slots(None)
    refused(lib, lib.spdy_slot_nature_observe_dev(nat, lt.h, -1, 1.0), ERR_STATE, b"slot_nature_observe: spdy_slot_set first")
    lt.set_slots([0, 12, 12, 30])
    for slot in (-1, 3):
        refused(lib, lib.spdy_slot_nature_observe_dev(nat, lt.h, slot, 1.0), ERR_ARG, b"slot_nature_observe: slot=%d outside [0, nslots=3)" % slot)
    for slot in (0, 1, 2):
        rc = lib.spdy_slot_nature_observe_dev(nat, lt.h, slot, 0.0)
        assert rc == ERR_NO_DEVICE and lib.spdy_last_error().startswith(b"host-only plan"), (slot, rc)


def test_fields_are_named_on_every_object(hs):
    """"slot_ps" and "slot_out" are names of the main block: valid on an object that never heard of slots (a host-only plan answers
    with its device check, an unknown name with SPDY_ERR_ARG)"""
    lib, p = hs.lib, ctypes.c_void_p()
    for name in (b"slot_ps", b"slot_out"):
        assert lib.spdy_letkf_field(hs.lt.h, name, ctypes.byref(p)) == ERR_NO_DEVICE
    refused(lib, lib.spdy_letkf_field(hs.lt.h, b"slot_hx", ctypes.byref(p)), ERR_ARG, b"unknown analysis field 'slot_hx'")
    s = package()
    assert s.letkf.LETKF_FIELDS[-2:] == ("slot_ps", "slot_out") and s.letkf.LETKF_TABLES[-1] == "slot_first"


def test_wrappers(hs):
    """the wrappers' own checks need no device"""
    import torch
    s, lt = package(), hs.lt
    lt.set_obs(*lk.args(hs.obs))
    for bad in ([0], [[0, 30]], [0.0, 30.0], 30):
        with pytest.raises(ValueError):
            lt.set_slots(bad)
    with pytest.raises(s.SpdyError) as e:
        lt.set_slots([0, 29])
    assert e.value.code == ERR_ARG and lt.slots is None
    lt.set_slots([0, 30])
    sp = hs.sp
    good = [torch.zeros((NMEM, KX) + sp.grid_shape, dtype=torch.float64)] * 4 + [torch.zeros((NMEM,) + sp.grid_shape, dtype=torch.float64)]
    for at, bad in ((0, good[4]), (4, good[0]), (2, good[2].to(torch.float32)), (1, good[1].transpose(2, 3))):
        a = list(good)
        a[at] = bad
        with pytest.raises(ValueError):
            lt.observe_grid(0, *a)
    with pytest.raises(s.SpdyError) as e:
        lt.observe_grid(0, *good)
    assert e.value.code == ERR_NO_DEVICE
    with pytest.raises(s.SpdyError) as e:
        lt.analyse_grid(*good, out=good, slots=True)
    assert e.value.code == ERR_STATE
    with pytest.raises(ValueError):
        hs.nat.observe(hs.lt_other, slot=0)
    with pytest.raises(s.SpdyError) as e:
        hs.nat.observe(lt, slot=1)
    assert e.value.code == ERR_ARG
    ens = s.Ensemble.__new__(s.Ensemble)
    ens.sp, ens.nmem = sp, NMEM + 1
    with pytest.raises(ValueError):
        ens.observe(hs.lt_other, 0)
    with pytest.raises(ValueError):
        ens.observe(lt, 0)
    for f in (s.Letkf.set_slots, s.Letkf.observe_grid, s.Letkf.observe_dev, s.Ensemble.observe):
        assert f.__doc__
    assert "slots" in s.Ensemble.analyse.__doc__ and "slot" in s.Nature.observe.__doc__


# ---------------------------------------------------------------------------------------------------- the binding surface
SLOT_CALLS = {
    "spdy_slot_set": "spdy_letkf *l, int nslots, const int *first",
    "spdy_slot_observe_grid_dev": "spdy_letkf *l, int slot, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg",
    "spdy_slot_observe_dev": "spdy_letkf *l, int slot, const double *vor, const double *div, const double *t, const double *q, const double *ps",
    "spdy_slot_analyse_grid_dev": "spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg, "
                                  "double *du, double *dv, double *dt, double *dq, double *dps, const int *d_use",
    "spdy_slot_ens_letkf_dev": "spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use",
    "spdy_slot_nature_observe_dev": "struct spdy_nature *n, spdy_letkf *letkf, int slot, double noise",
}


def test_binding_surface():
    """each new name is declared with the expected argument list, bound in Fortran and in SIGNATURES; nothing else carries the prefix"""
    from speedy_f90_amd import _lib
    v, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"spdy_slot_set": [v, i, v], "spdy_slot_observe_grid_dev": [v, i] + [v] * 5, "spdy_slot_observe_dev": [v, i] + [v] * 5,
            "spdy_slot_analyse_grid_dev": [v] * 12, "spdy_slot_ens_letkf_dev": [v] * 7, "spdy_slot_nature_observe_dev": [v, v, i, d]}
    assert {n for n in support.declared() if n.startswith("spdy_slot_")} == set(SLOT_CALLS)
    assert {n for n in support.fortran_bound() if n.startswith("spdy_slot_")} == set(SLOT_CALLS)
    assert {n for n in _lib.SIGNATURES if n.startswith("spdy_slot_")} == set(SLOT_CALLS)
    for name, params in SLOT_CALLS.items():
        assert support.declaration(name) == params, name
        assert _lib.SIGNATURES[name] == want[name], name
    assert "enum { SPDY_MAX_SLOTS = 32 };" in support.header() and "SPDY_MAX_SLOTS = 32_c_int" in support.fortran_binding()
    assert "observations in time slots (DESIGN.md s25)" in support.header(comments=True)
