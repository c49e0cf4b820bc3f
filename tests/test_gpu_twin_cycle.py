"""GPU: the 4D-LETKF cycle on real forecasts (Ensemble.step between Ensemble.observe calls, Ensemble.startup after
Ensemble.analyse(slots=True), a Nature whose truth is stepped alongside) against the host chain of tests/twincycle.py: the C oracle's
steps, tests/nature.py's values and scores, tests/letkfslots.py's analysis.  T30 L5, E = 12, 600 observations in three slots after
leapfrog steps 3, 6 and 9 of a 9-step window, two windows.  The host conditions that give these comparisons their meaning are
tests/test_twin_cycle_cpu.py's: a step moves every member's H x by 1e-3 of its scale, a million times the limits used here.
The device cycle runs once per module (`run`); the tests that need a state of their own start from the spectra it recorded."""
import numpy as np
import pytest

import dynstep
import ensemblestep as es
import letkf as lk
import letkfmask as lm
import letkfpressure as lp
import letkfrelax as lr
import nature as nt
import support
import synth
import twincycle as tc
from conftest import TOL

pytestmark = pytest.mark.gpu

E, DELT, W = tc.E, tc.DELT, tc.WINDOW
FAR = 1000.0                       # a neighbouring step is farther than FAR x the limit
LEVEL1 = es.PROG                   # Nature.set_state's order


@pytest.fixture(scope="module")
def plan():
    sp = support.ensemble_plan(tc.TAG, E)
    yield sp, lp.Geometry(sp), nt.gaussian_weights(sp)
    sp.close()


def clones(ens, names=es.PROG):
    return {n: getattr(ens, n).clone() for n in names}


def restore(ens, saved):
    for n, a in saved.items():
        getattr(ens, n).copy_(a)


def host(saved, lv):
    """time level lv of cloned prognostics as NumPy, member axis first"""
    return {n: saved[n][lv].cpu().numpy() for n in es.PROG}


def truth_spectra(tru):
    return [tru.member(0)[n][0] for n in LEVEL1]


def fresh(run, sp, nmem, saved, keep=None):
    """an Ensemble of nmem members with the cycle's shared fields and the members `keep` (default all) of the cloned prognostics"""
    import speedy_f90_amd as s
    ens = s.Ensemble(sp, nmem)
    ens.set_shared(run["host"]["started"][0])
    for n in es.PROG:
        getattr(ens, n).copy_(saved[n] if keep is None else saved[n][:, list(keep)])
    return ens


def make_letkf(sp, nmem, net):
    lt = lk.make(sp, nmem, net, tc.SIGMA_V, tc.RHO, tc.SIGMA_H)
    lt.set_slots(tc.FIRST)
    return lt


def observe_group(ens, tru, nat, lt, s, noise=1.0):
    nat.set_state(*truth_spectra(tru))
    nat.observe(lt, noise, slot=s)
    ens.observe(lt, s)


def forecast(ens, tru, nat, lt, after=None, before_step=None):
    """a window's WINDOW leapfrog steps of the members and the truth, the three groups at their steps; after(s): called once slot s
    has been observed; before_step(n): called before step n"""
    for n in range(1, W + 1):
        if before_step is not None:
            before_step(n)
        ens.step(2, 2, 2.0 * DELT)
        tru.step(2, 2, 2.0 * DELT)
        if n in tc.SLOT_STEPS:
            s = tc.SLOT_STEPS.index(n)
            observe_group(ens, tru, nat, lt, s)
            if after is not None:
                after(s)


def the_scores(sp, g, w, lt, nat, slot, ratios, tag):
    """after a verify into `slot`: the device's table against tests/nature.py's scores of the grids that call formed (the analysis
    object's workspace, downloaded) and the truth, within tests/twincycle.py's score_limits -> the table"""
    x, truth = tc.gridded(lt.field("grid").numpy(), lt.nmem, sp.kx), nat.truth()
    got = nat.field("scores").numpy()[slot]
    rel, bias_abs = tc.score_limits(g, x, truth, w, lt.nmem)
    ratios[tag] = tc.score_ratios(got, nt.flat(nt.scores(g, x, truth, w)), rel, bias_abs)
    return nat.scores(slot)


@pytest.fixture(scope="module")
def run(plan, oracle_factory):
    """The device cycle, eager, and the host chain next to it.  Host: the start-up, the spin-up and window 0's forecast from the
    seeded states; window 1's start-up and forecast from the DEVICE's analysed time level 1, downloaded (members) and the host's
    own truth.  Everything recorded is read only."""
    import speedy_f90_amd as s
    import torch
    sp, g, w = plan
    o = oracle_factory(tc.TAG)
    R = {"host": {}, "dev": {}, "ratios": {}}
    truth0, members0 = tc.initial_states(o)
    shared = {n: truth0[n] for n in ("phis", "tcorh", "qcorh")}
    started, _ = tc.startup(o, [truth0] + members0)
    spun = tc.leapfrog(o, started, tc.SPINUP)[-1]
    R["host"]["started"] = started
    R["host"]["w0"] = tc.forecast(o, spun[1:], spun[0])
    net = tc.network(g, R["host"]["w0"]["x"][0])
    R["net"] = net

    ens, tru = es.build(sp, members0), es.build(sp, [truth0])
    ens.startup(DELT)
    tru.startup(DELT)
    torch.cuda.synchronize()
    R["dev"]["started"] = (clones(ens), clones(tru))
    for _ in range(tc.SPINUP):
        ens.step(2, 2, 2.0 * DELT)
        tru.step(2, 2, 2.0 * DELT)
    torch.cuda.synchronize()
    R["dev"]["w0_start"] = (clones(ens), clones(tru))

    lt, lt0 = make_letkf(sp, E, net), make_letkf(sp, E, net)
    nat, nat0 = s.Nature(sp, seed=tc.NOISE_SEED, capacity=6), s.Nature(sp, seed=1, capacity=1)
    free = s.Ensemble(sp, E)
    free.set_shared(shared)
    for c in (0, 1):
        slots = []

        def after(sl):
            rec = {"spectra": clones(ens), "truth_spectra": clones(tru), "grid": tc.gridded(lt.field("grid").numpy(), E, sp.kx),
                   "hx": lt.field("hx").numpy(), "truth": nat.truth()}
            nat0.set_state(*truth_spectra(tru))
            nat0.observe(lt0, 0.0, slot=sl)
            rec["truth0"], rec["value0"] = nat0.truth(), lt0.field("value").numpy()
            slots.append(rec)
        forecast(ens, tru, nat, lt, after)
        win = {"slots": slots, "value": lt.field("value").numpy(), "hx": lt.field("hx").numpy(), "background": clones(ens)}
        win["phi_stale"] = ens.phi.clone()
        if c == 0:
            restore(free, win["background"])
        ens.verify(lt, nat, 2 * c)
        win["scores_b"] = the_scores(sp, g, w, lt, nat, 2 * c, R["ratios"], "window %d background" % c)
        ens.analyse(lt, slots=True)
        ens.verify(lt, nat, 2 * c + 1)
        win["scores_a"] = the_scores(sp, g, w, lt, nat, 2 * c + 1, R["ratios"], "window %d analysis" % c)
        win["fields"] = {n: lt.field(n).numpy() for n in lk.FIELDS}
        win["analysed"] = clones(ens)
        win["table"] = nat.field("scores").numpy()
        ens.startup(DELT)
        torch.cuda.synchronize()
        win["restarted"], win["phi"] = clones(ens), ens.phi.clone()
        R["dev"]["w%d" % c] = win
    # the members never analysed, at the second analysis time, against the truth the second window left in nat
    for _ in range(W):
        free.step(2, 2, 2.0 * DELT)
    free.verify(lt, nat, 4)
    R["dev"]["free"] = the_scores(sp, g, w, lt, nat, 4, R["ratios"], "free run")
    # the misdated control: the first window's values, every H x taken at the analysis time -- a plain analysis of the background
    mis = s.Ensemble(sp, E)
    mis.set_shared(shared)
    restore(mis, R["dev"]["w0"]["background"])
    plain = lk.make(sp, E, dict(net, value=R["dev"]["w0"]["value"]), tc.SIGMA_V, tc.RHO, tc.SIGMA_H)
    nat.set_state(*[R["dev"]["w0"]["slots"][2]["truth_spectra"][n][0, 0] for n in LEVEL1])
    mis.analyse(plain)
    mis.verify(plain, nat, 5)
    R["dev"]["misdated"] = the_scores(sp, g, w, plain, nat, 5, R["ratios"], "misdated analysis")
    plain.close(); lt.close(); lt0.close(); nat.close(); nat0.close()

    # window 1 on the host: the members from the device's analysed level 1, the truth the host's own
    w0 = R["dev"]["w0"]
    analysed = tc.host_states(host(w0["analysed"], 0), host(w0["analysed"], 1), shared)
    restarted, phi = tc.startup(o, analysed)
    R["host"]["w1"] = tc.forecast(o, restarted, R["host"]["w0"]["truth"][W])
    w1 = R["dev"]["w1"]
    R["host"]["restarts"] = [(restarted, phi), tc.startup(o, tc.host_states(host(w1["analysed"], 0), host(w1["analysed"], 1), shared))]
    return R


def worst(errors):
    return max(errors.values())


# ---------------------------------------------------------------------------------------------------- 1. forecast states
def test_forecast_states(run):
    """After the start-up and at every slot time of both windows the device's time level 1 of every member and of the truth is
    within conftest.TOL of the oracle chain's, in relerr and wave_relerr: the bar of test_two_day_run_vs_reference.  Window 1 is the
    test of the restart and the forecast from it: its oracle chain starts from the device's own analysed spectra"""
    lines, most = [], 0.0
    dev_ens, dev_tru = run["dev"]["started"]
    for lv in (0, 1):
        e = tc.spectral_errors(host(dev_ens, lv), run["host"]["started"][1:], lv)
        e["truth"] = worst(tc.spectral_errors(host(dev_tru, lv), run["host"]["started"][:1], lv))
        lines.append("start-up, time level %d: " % (lv + 1) + " ".join("%s %.1e" % kv for kv in e.items()))
        most = max(most, worst(e))
    for c in (0, 1):
        for sl, n in enumerate(tc.SLOT_STEPS):
            rec, ref = run["dev"]["w%d" % c]["slots"][sl], run["host"]["w%d" % c]
            e = tc.spectral_errors(host(rec["spectra"], 0), ref["members"][n], 0)
            e["truth"] = worst(tc.spectral_errors(host(rec["truth_spectra"], 0), [ref["truth"][n]], 0))
            lines.append("window %d step %d: " % (c, n) + " ".join("%s %.1e" % kv for kv in e.items()))
            most = max(most, worst(e))
    print("\n[twin cycle, forecast states vs the oracle chain, relative error]\n  " + "\n  ".join(lines))
    print("[twin cycle] forecast states: largest error / limit %.3e" % (most / TOL))
    assert most <= TOL, most


# ---------------------------------------------------------------------------------------------------- 2. dating
def test_the_date_of_a_slot(run, plan):
    """After ens.observe(lt, s): hx on the slot's rows is tests/letkfslots.py's operator on the gridded ensemble the call left in
    the analysis object's workspace, bit for bit; that ensemble is within TOL x scale of the oracle's grids of ITS step and farther
    than 1000 x that from the oracle's grids one step earlier and one step later, per variable.  The same for the truth:
    Nature.set_state then observe(slot=s, noise=0) gives tests/letkfpressure.py's truth_values on the truth it holds, bit for bit,
    and tests/nature.py's operator on the oracle's truth within (TOL + 16 eps) x scale; the truth is the oracle's of its step and
    not of a neighbouring one"""
    sp, g, _ = plan
    net = run["net"]
    lt = make_letkf(sp, E, net)
    stencil = lp.tables(lt)
    near, apart = 0.0, np.inf
    for c in (0, 1):
        ref = run["host"]["w%d" % c]
        for sl, n in enumerate(tc.SLOT_STEPS):
            rec, rows = run["dev"]["w%d" % c]["slots"][sl], tc.rows(sl)
            sub, st = lk.subset(net, rows), (stencil[0][rows], stencil[1][rows])
            assert support.same_bits(rec["hx"][rows], lk.observe(g, rec["grid"], sub, st)[0]), (c, sl)
            assert support.same_bits(rec["value0"][rows], lp.truth_values(g, rec["truth0"], sub, st)), (c, sl)
            h = nt.operator(g, ref["xt"][n], net)[rows]
            scale = np.array([np.max(np.abs(ref["xt"][n][lk.VARS[v]])) for v in net["var"][rows]])
            near = max(near, float(np.max(np.abs(rec["value0"][rows] - h) / ((TOL + 16 * lk.EPS) * scale))))
            for what, x, at in (("members", rec["grid"], ref["x"]), ("truth", rec["truth"], ref["xt"]), ("truth", rec["truth0"], ref["xt"])):
                here = tc.grid_errors(x, at[n])
                near = max(near, worst(here) / TOL)
                for m in (n - 1, n + 1):
                    there = tc.grid_errors(x, at[m])
                    apart = min(apart, min(there.values()) / (FAR * TOL))
                    assert min(there.values()) > FAR * TOL, (c, sl, what, m, there)
                assert worst(here) <= TOL, (c, sl, what, here)
    lt.close()
    print("[twin cycle] dating: largest error / limit %.3e; a neighbouring step's smallest distance / (1000 x limit) %.3e" % (near, apart))
    assert near <= 1.0, near


# ---------------------------------------------------------------------------------------------------- 3. observing changes no forecast
def test_observing_changes_no_forecast(run, plan):
    """Two ensembles from the same spectra: one through {3 steps, set_state, Nature.observe, Ensemble.observe, verify} x 3, the other
    through 9 plain steps.  Every prognostic array, both time levels, and phi have the same bits: the calls that run the analysis'
    inverse batch into the analysis object's workspace between two steps leave the next step what it would have been"""
    import speedy_f90_amd as s
    import torch
    sp, g, w = plan
    start, tstart = run["dev"]["w0_start"]
    a, b, tru = fresh(run, sp, E, start), fresh(run, sp, E, start), fresh(run, sp, 1, tstart)
    lt, nat = make_letkf(sp, E, run["net"]), s.Nature(sp, seed=3, capacity=3)
    forecast(a, tru, nat, lt, after=lambda sl: a.verify(lt, nat, sl))
    for _ in range(W):
        b.step(2, 2, 2.0 * DELT)
    torch.cuda.synchronize()
    hx = lt.field("hx").numpy()
    assert np.isfinite(nat.field("scores").numpy()).all() and all(hx[tc.rows(sl)].any() for sl in range(3))
    for n in es.PROG + ("phi",):
        assert support.same_bits(getattr(a, n), getattr(b, n)), n
    assert not support.same_bits(a.vor[0], start["vor"][0])
    lt.close(); nat.close()


# ---------------------------------------------------------------------------------------------------- 4. the analysis on forecast states
def test_the_analysis_on_forecast_states(run, plan, oracle_factory):
    """A window's forecast with its three groups, then the slot analysis of the hx those Ensemble.observe calls kept, against
    tests/letkfslots.py fed the device's own gridded slot ensembles and values: hx and obs_used exactly, hxmean, y, departure and
    obs_lnsigma within 16 eps of their scale, every variable's increments within lk.limits(...) at lk.columns_for(...) -- the rules
    of tests/test_gpu_letkf_slots.py.  Once plain and once with set_relaxation(0.3, 0.9) against tests/letkfrelax.py's relaxation
    of the plain increments.  And Ensemble.analyse(lt, slots=True) on the spectra moves time level 1 by those increments taken to
    spectra with the oracle's vdspec and grid_to_spec, within TOL"""
    import torch
    sp, g, w = plan
    o, net = oracle_factory(tc.TAG), run["net"]
    start, tstart = run["dev"]["w0_start"]
    ens, tru = fresh(run, sp, E, start), fresh(run, sp, 1, tstart)
    import speedy_f90_amd as s
    lt, nat = make_letkf(sp, E, net), s.Nature(sp, seed=tc.NOISE_SEED, capacity=1)
    xs = []
    forecast(ens, tru, nat, lt, after=lambda sl: xs.append(tc.gridded(lt.field("grid").numpy(), E, sp.kx)))
    x = xs[-1]
    obs = dict(net, value=lt.field("value").numpy())
    assert support.same_bits(obs["value"], run["dev"]["w0"]["value"]) and support.same_bits(lt.field("hx").numpy(), run["dev"]["w0"]["hx"])
    cols = lk.columns_for(g, obs, tc.SIGMA_H, most=32)
    want = lk.obs_space(g, x, obs, stencil=lp.tables(lt), xs=xs, first=tc.FIRST)
    C, b = lk.problems(g, obs, want, tc.SIGMA_H, tc.SIGMA_V, cols)
    lim, ref, kappa = lk.limits(g, x, C, b, tc.RHO, cols, E)
    got = lk.run(lt, x, slots=True)
    for n in ("hx", "obs_used"):
        assert support.same_bits(got[n], want[n]), n
    scale = np.array([np.max(np.abs(x[lk.VARS[v]])) for v in obs["var"]])
    lnscale = np.maximum(np.abs(want["obs_lnsigma"]), 1.0)
    ratios = {}
    for n, sc in (("hxmean", scale), ("y", scale[:, None]), ("departure", scale), ("obs_lnsigma", lnscale)):
        ratios[n] = float(np.max(np.abs(got[n] - want[n]) / (16 * lk.EPS * sc)))
    for v in lk.VARS:
        ratios[v] = float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v]
        assert ref[v].any(), v
    print("[twin cycle] analysis on forecast states: kappa %.2e, ratio to the limit: %s" % (kappa, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, ratios
    # the route a cycle would use: relaxed
    lt.set_relaxation(0.3, 0.9)
    relaxed = lk.run(lt, x, slots=True)
    raw = {v: got[v] for v in lk.VARS}
    rel, fmax = lr.compare(x, raw, {v: relaxed[v] for v in lk.VARS}, relaxed["inflation"], 0.3, 0.9, E)
    print("[twin cycle] relaxed analysis (0.3, 0.9): ratio to the limit %.3e, largest inflation %.3f" % (rel, fmax))
    assert rel <= 1.0 and fmax > 1.0 and not support.same_bits(relaxed["t"], got["t"])
    lt.set_relaxation(0.0, 0.0)
    # from the spectra
    before = clones(ens)
    ens.analyse(lt, slots=True)
    torch.cuda.synchronize()
    for n in lk.FIELDS:
        assert support.same_bits(lt.field(n).numpy(), got[n]), n
    hosted = tc.add_increments(o, tc.host_states(host(before, 0), host(before, 1), {}), {v: got[v] for v in lk.VARS})
    e = tc.spectral_errors(host(clones(ens), 0), hosted, 0)
    print("[twin cycle] Ensemble.analyse(slots=True) vs the increments taken to spectra: error / limit %.3e" % (worst(e) / TOL))
    assert worst(e) <= TOL, e
    for n in es.PROG:
        assert support.same_bits(getattr(ens, n)[1], before[n][1]) and support.same_bits(getattr(ens, n), run["dev"]["w0"]["analysed"][n]), n
    lt.close(); nat.close()


# ---------------------------------------------------------------------------------------------------- 5. the restart
def test_the_restart(run):
    """After the analysis and ens.startup(delt), both windows: time level 1 is the analysed one bit for bit, time level 2 and phi are
    those of the oracle's start-up from the analysed time level 1 within TOL, and they differ from the stale ones of before the
    analysis by more than 1000 x TOL.  The host start-up of each window is from the device's own analysed spectra"""
    most, apart = 0.0, np.inf
    for c in (0, 1):
        win = run["dev"]["w%d" % c]
        for n in es.PROG:
            assert support.same_bits(win["restarted"][n][0], win["analysed"][n][0]), (c, n)
        ref, phi = run["host"]["restarts"][c]
        e = tc.spectral_errors(host(win["restarted"], 1), ref, 1)
        got_phi = win["phi"].cpu().numpy()
        e["phi"] = max(max(synth.relerr(got_phi[m], phi[m]), dynstep.wave_relerr(got_phi[m], phi[m])) for m in range(E))
        most = max(most, worst(e))
        stale = host(win["background"], 1)
        far = {n: min(synth.relerr(a[m], stale[n][m]) for m in range(E)) for n, a in host(win["restarted"], 1).items()}
        far["phi"] = min(dynstep.wave_relerr(got_phi[m], win["phi_stale"].cpu().numpy()[m]) for m in range(E))
        apart = min(apart, min(far.values()) / (FAR * TOL))
        print("[twin cycle] restart of window %d: %s; distance to the stale level 2 / TOL: %s"
              % (c, " ".join("%s %.1e" % kv for kv in e.items()), " ".join("%s %.1e" % (k, v / TOL) for k, v in far.items())))
        assert min(far.values()) > FAR * TOL, far
    print("[twin cycle] restart: largest error / limit %.3e; stale state's smallest distance / (1000 x limit) %.3e" % (most / TOL, apart))
    assert most <= TOL, most


# ---------------------------------------------------------------------------------------------------- 6. what slots are for
def test_what_slots_are_for(run):
    """Every verify of the cycle against tests/nature.py's scores of the grids that call formed, within the limits of
    tests/test_gpu_nature.py (tests/twincycle.py, score_limits); and tests/test_twin_cycle_cpu.py's thresholds on the device's
    numbers: the slot analysis beats its background, the same values dated at the analysis time do worse than none, the second
    window's background beats the members never analysed"""
    for tag, r in run["ratios"].items():
        print("[twin cycle scores, %s] error / limit: %s" % (tag, " ".join("%s %.2e" % kv for kv in r.items())))
    assert len(run["ratios"]) == 6 and max(max(r.values()) for r in run["ratios"].values()) <= 1.0, run["ratios"]
    w0, w1 = run["dev"]["w0"], run["dev"]["w1"]
    good, bad = tc.ratios(w0["scores_a"], w0["scores_b"]), tc.ratios(run["dev"]["misdated"], w0["scores_b"])
    again = tc.ratios(w1["scores_b"], run["dev"]["free"])
    print("[twin cycle, device] rmse analysis / background, window 0: 4D %s; misdated %s; window 1 background / free run: %s"
          % tuple(" ".join("%s %.3f" % kv for kv in r.items()) for r in (good, bad, again)))
    assert np.isfinite(w1["table"]).all()
    for v in tc.SCORED:
        assert good[v] <= tc.THRESHOLD["4d"][v], (v, good[v])
        assert bad[v] >= tc.THRESHOLD["misdated"][v], (v, bad[v])
    for v in ("t", "ps"):
        assert again[v] <= tc.THRESHOLD["restart"][v], (v, again[v])


# ---------------------------------------------------------------------------------------------------- 7. one graph
def test_the_window_in_one_graph(run, plan):
    """The first window captured as one graph -- 9 steps of the members and of the truth, the three set_state / Nature.observe /
    Ensemble.observe groups, verify, analyse(slots=True), verify -- and launched twice from restored spectra and a reset Nature:
    the spectra, hx, value, the per-observation fields and the scores have the eager run's bits"""
    import speedy_f90_amd as s
    import torch
    sp, g, w = plan
    start, tstart = run["dev"]["w0_start"]
    ens, tru = fresh(run, sp, E, start), fresh(run, sp, 1, tstart)
    lt, nat = make_letkf(sp, E, run["net"]), s.Nature(sp, seed=tc.NOISE_SEED, capacity=6)
    eager = run["dev"]["w0"]

    def cycle():
        forecast(ens, tru, nat, lt)
        ens.verify(lt, nat, 0)
        ens.analyse(lt, slots=True)
        ens.verify(lt, nat, 1)

    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            cycle()
        for r in range(2):
            restore(ens, start)
            restore(tru, tstart)
            nat.reset(tc.NOISE_SEED)
            for name in ("hx", "value"):
                f = lt.field(name)
                f.upload(np.full(f.shape, -3.0))
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), eager["analysed"][n]), (r, n)
            assert support.same_bits(lt.field("value").numpy(), eager["value"]), r
            for n in lk.FIELDS:
                assert support.same_bits(lt.field(n).numpy(), eager["fields"][n]), (r, n)
            assert support.same_bits(nat.field("scores").numpy()[:2], eager["table"][:2]), r
            assert nat.draws() == 3
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close(); nat.close()


# ---------------------------------------------------------------------------------------------------- 8. a member lost mid-window
def test_a_member_lost_mid_window(run, plan):
    """Member 3's t is made NaN (both time levels) after slot 0 has been observed; a guard of E members records it on the next
    check_dev, and analyse(lt, use=guard.use_dev(), slots=True) gives the other members, bit for bit, what an (E - 1)-member
    forecast and analysis of the compacted states gives them (tests/letkfmask.py, same_as_compact, on time level 1 of vor, div, t,
    tr, ps in place of the gridded increments); member 3 keeps every bit.  The NaN is test data in a masked member: the kernels'
    loops have fixed bounds"""
    import speedy_f90_amd as s
    import torch
    sp, g, w = plan
    drop = 3
    keep = tuple(e for e in range(E) if e != drop)
    start, tstart = run["dev"]["w0_start"]
    net = run["net"]
    results = {}
    for nmem, members in ((E, None), (E - 1, keep)):
        ens, tru = fresh(run, sp, nmem, start, members), fresh(run, sp, 1, tstart)
        lt, nat = make_letkf(sp, nmem, net), s.Nature(sp, seed=tc.NOISE_SEED, capacity=1)
        guard = s.Diagnostics(sp, capacity=4, nmem=nmem)

        def before_step(n):
            if n == tc.SLOT_STEPS[0] + 1 and nmem == E:
                ens.t[:, drop] = complex(float("nan"), float("nan"))
            if n == tc.SLOT_STEPS[0] + 2:
                guard.check_dev(ens.vor[1], ens.div[1], ens.t[1])
        forecast(ens, tru, nat, lt, before_step=before_step)
        use = guard.use_dev()
        assert use.tolist() == (lm.flags(E, keep) if nmem == E else [1] * nmem)
        before = clones(ens)
        ens.analyse(lt, use=use if nmem == E else None, slots=True)
        torch.cuda.synchronize()
        res = {v: getattr(ens, n)[0].cpu().numpy() for v, n in zip(lk.VARS, es.PROG)}
        res.update({n: lt.field(n).numpy() for n in lm.OBS_FIELDS + ("y", "hx", "members_used")})
        if nmem == E:
            for v, n in zip(lk.VARS, es.PROG):
                assert support.same_bits(getattr(ens, n)[:, drop], before[n][:, drop]), n
                assert not support.same_bits(getattr(ens, n)[0, 0], before[n][0, 0]), n
                res[v][drop] = 0.0               # same_as_compact's form for a member not in use: it got no increment
            assert np.isnan(res["hx"][tc.rows(1), drop]).all() and np.isfinite(res["hx"][tc.rows(0), drop]).all()
        results[nmem] = res
        lt.close(); nat.close(); guard.close()
    lm.same_as_compact(results[E], results[E - 1], E, keep, "lost mid-window")
    assert np.isfinite(results[E]["t"][list(keep)]).all()
