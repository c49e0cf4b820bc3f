"""The reference side of the surface-model tests, on the CPU: the host tables of spdy_surface_model_create and the date weights
against the restatement (tests/surfmodel.py), and the conditions the GPU tests rely on -- on every step of every window, at both
resolutions, no column's interpolated sstcl_ob is closer to the freezing point sstfr than physstep.RUN_MARGIN (sice jumps there;
no column is ever excluded), and every branch of the models is taken."""
import numpy as np
import pytest

import longrun
import moist
import physstep
import support
import surfmodel as sm
import synth
from conftest import TOL


def shaped(c, shape):
    return {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + shape) for k, v in c.items()}


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_host_tables_match_restatement(tag, oracle_factory):
    """land_model_init's and sea_model_init's constant fields as the library builds them on a host-only plan"""
    s = support.package()
    sp = support.plan(tag, max_batch=4, device=-1)
    phis0 = sm.orography(oracle_factory(tag))      # a host-only plan does not transform
    c = sm.climatology(phis0, longrun.latitudes(sp.table("sia_half")))
    tab = sm.tables(c["fmask"], c["alb0"], sp.table("sia_half"), sp.ix)
    m = s.SurfaceModel(sp, shaped(c, sp.grid_shape), sm.DELT)
    for n in sm.TABLES:
        got = m.table(n).reshape(-1)
        assert np.max(np.abs(got - tab[n])) <= TOL * np.max(np.abs(tab[n])), n
    # both classes of every decision of the init routines
    fl, fs = tab["fmask_l"], tab["fmask_s"]
    assert (fl == 0.0).any() and (fl == 1.0).any() and ((fl > 0.0) & (fl < sm.THIRD)).any() and ((fl >= sm.THIRD) & (fl < 1.0)).any()
    assert (fs == 0.0).any() and (fs == 1.0).any() and ((fs > 0.0) & (fs < sm.THIRD)).any()
    assert np.unique(tab["rhcapl"]).size == 2 and np.unique(tab["cdland"]).size == 2 and np.unique(tab["cdsea"]).size == 2
    assert (c["alb0"] < moist.f32(0.4)).any() and (c["alb0"] >= moist.f32(0.4)).any()
    # no device: every device call is refused, never computed on the host
    assert sp.lib.spdy_surface_model_set_date(m.h, 1, 0.5, 0.04) == -3
    assert sp.lib.spdy_surface_model_couple_dev(m.h, 0, None, None, None, None) == -3
    m.close()
    sp.close()


def test_dates_and_weights():
    """newdate over the three windows' events, and forin5's weights: they sum to one and forint's switch is at tmonth = 0.5"""
    d = sm.Date(1982, 1, 15)
    for _ in range(sm.NSTEPS):
        d.newdate()
    assert d.key() == (1982, 1, 16) and d.tmonth == 0.5 and sm.weights(d.imont1, d.tmonth)["s2"] == 0
    for _ in range(sm.NSTEPS):
        d.newdate()
    w = sm.weights(d.imont1, d.tmonth)
    assert d.tmonth > 0.5 and w["s2"] == 2 and w["m2"] == (0, 1)
    d = sm.Date(1982, 12, 31, 23, 20)
    d.newdate()
    assert (d.year, d.month, d.day, d.hour, d.minute) == (1983, 1, 1, 0, 0) and d.imont1 == 1
    w = sm.weights(d.imont1, d.tmonth)
    assert w["m5"] == (10, 11, 0, 1, 2) and w["m2"] == (0, 11)
    assert abs(sum(w["w5"]) - 12 * float(np.float32(1.0) / np.float32(12.0))) < 1e-15
    d = sm.Date(1984, 2, 28, 23, 20)
    d.newdate()
    assert d.key() == (1984, 2, 29)


@pytest.mark.parametrize("wname", list(sm.WINDOWS))
@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_windows_conditions(tag, wname, oracle_factory):
    sp = support.plan(tag, max_batch=4, device=-1)
    phis0 = sm.orography(oracle_factory(tag))      # a host-only plan does not transform
    n = phis0.size
    start = sm.WINDOWS[wname]
    c = sm.climatology(phis0, longrun.latitudes(sp.table("sia_half")), start=start[:2])
    m = sm.Model(c, sm.tables(c["fmask"], c["alb0"], sp.table("sia_half"), sp.ix), ssta=sm.ssta_reader(c["fmask"]))
    seen = {"days": set(), "shifted": 0, "s2": set()}

    def on_step(model_step, day, date, flux, shifted):
        seen["days"].add(date.key())
        seen["shifted"] += bool(shifted)
        seen["s2"].add(sm.weights(date.imont1, date.tmonth)["s2"])
        assert all(np.isfinite(v).all() for v in m.f.values())
    end = sm.run(m, start, sm.WINDOW_STEPS, phis0.reshape(-1), lambda k: sm.fluxes(k, n), None, on_step)
    print("[surfmodel %s %s] freezing-point margin %.2e, branches %s" % (tag, wname, m.margin, {k: int(v.sum()) for k, v in m.branch.items()}))
    assert m.margin >= physstep.RUN_MARGIN, m.margin
    assert all(v.any() for v in m.branch.values()), {k: int(v.sum()) for k, v in m.branch.items()}
    assert len(seen["days"]) == 4                                 # three whole days and the midnight that ends them
    # each window crosses its event
    if wname == "midmonth":
        assert seen["s2"] == {0, 2}
    elif wname == "month":
        assert end.key() == (1982, 2, 2) and seen["shifted"] == sm.NSTEPS    # obs_ssta on every step of 1 February
    else:
        assert end.key() == (1983, 1, 2) and seen["shifted"] == sm.NSTEPS
    sp.close()


@pytest.mark.parametrize("wname", list(sm.WINDOWS))
def test_restatement_matches_reference_fixture(wname, golden, oracle_factory):
    """tests/golden/ref_surfmodel.npz (the flang-built reference's coupler, land_model, sea_model, date and forcing, T30,
    tests/golden/make_golden_surfmodel.py): the restatement on the regenerated seeded inputs gives the reference's tables, its
    fields at every recorded step, its snowc / alb_l / alb_s / albsfc after every forcing and, through the oracle's grid_to_spec of
    the restated corh, its qcorh, within TOL on the stored column sample; the reference side met the conditions."""
    g = golden("surfmodel")
    o = oracle_factory("t30")
    phis0 = sm.orography(o)
    n = phis0.size
    start = sm.WINDOWS[wname]
    c = sm.climatology(phis0, longrun.latitudes(o.table("sia_half")), start=start[:2])
    sub, ins = g[wname + "_sub"], g[wname + "_insub"]
    assert int(g["seed"]) == sm.CLIM_SEED and tuple(g["field_names"]) == sm.FIELDS and tuple(g["table_names"]) == sm.TABLES
    for k in ("fmask", "alb0") + sm.CLIM12 + ("sstan3",):                  # the regenerated inputs are the generator's
        assert np.array_equal(np.asarray(c[k])[..., ins], g["%s_in_%s" % (wname, k)]), k
    assert np.array_equal(phis0.reshape(-1)[ins], g[wname + "_in_phis0"])
    tab = sm.tables(c["fmask"], c["alb0"], o.table("sia_half"), o.ix)
    for i, k in enumerate(sm.TABLES):
        assert synth.relerr(tab[k][sub], g[wname + "_tables"][i]) <= TOL, k
    m = sm.Model(c, tab, ssta=sm.ssta_reader(c["fmask"]))
    check, fsteps, qsteps = list(g[wname + "_check"]), list(g[wname + "_forcing_steps"]), list(g[wname + "_qcorh_steps"])
    seen = {"fields": 0, "forcing": 0, "qcorh": 0}
    kept = {}

    def near(x, ref, what):
        s = np.abs(ref).max()
        e = float(np.abs(x - ref).max() / s) if s > 0 else float(np.abs(x).max())
        assert e <= TOL, (wname, what, e)

    def on_forcing(step, date):
        kept[step] = ({k: m.f[k][sub].copy() for k in sm.FORCING[:4]}, m.f["corh"].copy())

    def on_step(step, day, date, flux, shifted):
        if step in check:
            want = g[wname + "_fields"][check.index(step)]
            for i, k in enumerate(sm.FIELDS):
                near(m.f[k][sub], want[i], "step %d %s" % (step, k))
            seen["fields"] += 1
        if step in fsteps:
            for i, k in enumerate(sm.FORCING[:4]):
                near(kept[step][0][k], g[wname + "_forcing"][fsteps.index(step)][i], "forcing of step %d %s" % (step, k))
            seen["forcing"] += 1
        if step in qsteps:
            near(o.grid_to_spec(kept[step][1].reshape(phis0.shape)), g[wname + "_qcorh"][qsteps.index(step)], "qcorh of step %d" % step)
            seen["qcorh"] += 1
    sm.run(m, start, sm.WINDOW_STEPS, phis0.reshape(-1), lambda k: sm.fluxes(k, n), on_forcing, on_step)
    assert seen == {"fields": len(check), "forcing": 3, "qcorh": 2} and len(check) >= 17
    # the reference side: the margin it ran with, and every class of every decision in the stored sample
    assert float(g[wname + "_min_margin"]) >= physstep.RUN_MARGIN and m.margin == float(g[wname + "_min_margin"])
    assert all(int(v) > 0 for v in g[wname + "_class_counts"])
    fl, fs = tab["fmask_l"][sub], tab["fmask_s"][sub]
    for mask in list(m.branch.values()) + [tab["fmask_l"] == 0.0, tab["fmask_l"] == 1.0, c["alb0"] < moist.f32(0.4), c["alb0"] >= moist.f32(0.4)]:
        assert mask[sub].any()
    assert ((fl > 0.0) & (fl < sm.THIRD)).any() and ((fl >= sm.THIRD) & (fl < 1.0)).any() and ((fs > 0.0) & (fs < sm.THIRD)).any()
