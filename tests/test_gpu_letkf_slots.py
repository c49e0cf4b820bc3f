"""GPU: observations in time slots, the 4D-LETKF (include/spdy.h, "ensemble analysis, observations in time slots"; Letkf.set_slots,
observe_grid, analyse_grid(slots=True), Ensemble.observe, Ensemble.analyse(slots=True), Nature.observe(slot=)).  Four
statements need no tolerance: slots all observed on the analysed state give the plain analysis bit for bit; an observe writes its
slot's rows and nothing else; a member dropped at the analysis may hold anything from any slot on; one slot is no slot.  With
different times the analysis is held to the NumPy restatement (tests/letkfslots.py) by tests/letkf.py's limits(...).  T30; the section
"on the T63 L16 grid" holds the analysis of different times to the restatement at 192 x 96 x 16."""
import numpy as np
import pytest

import ensemblestep as es
import letkf as lk
import letkfmask as lm
import letkfpressure as lp
import letkfslots as ls
import nature as nt
import poison
import support

pytestmark = pytest.mark.gpu

ERR_STATE = -5


T63 = "t63k16"


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lp.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


def make(sp, E, obs, sigma_v, stride=None, relax=None):
    lt = (lp.make if "p" in obs else lk.make)(sp, E, obs, sigma_v)
    if stride is not None:
        lt.set_weight_stride(*stride)
    if relax is not None:
        lt.set_relaxation(*relax)
    return lt


def same(got, ref, names, tag):
    for n in names:
        assert support.same_bits(got[n], ref[n]), (tag, n)


# ---------------------------------------------------------------------------------------------------- 1. same state, bit for bit
def pressure_case(g, E, seed=21):
    x = lp.craft(g, E, seed)
    return x, lp.network(g, x)


# (id, E, members in use or None, sigma_v's, stride, relaxation, at-pressure network)
SAME_STATE = [("E3", 3, None, (0.0, 0.1), None, None, False), ("E32", 32, None, (0.0, 0.1), None, None, False),
              ("E8-masked7", 8, tuple(range(7)), (0.1,), None, None, False),
              ("E17-stride-relax", 17, None, (0.1,), (2, 2), (0.5, 0.5), False), ("E4-pressure", 4, None, (0.1,), None, None, True)]


@pytest.mark.parametrize("case", SAME_STATE, ids=[c[0] for c in SAME_STATE])
def test_same_state_is_the_plain_call(case, plans):
    """first = [0, 1, 1, 300, nobs] -- a one-observation slot, an empty one, a boundary inside a scan chunk of 256 and inside a
    workgroup of the at-pressure kernel, a long tail -- every slot observed on the ensemble that is analysed: the increments, hx,
    hxmean, y, departure, obs_lnsigma, obs_used, members_used, inflation and weights have the plain call's bits.  The plain call
    runs on an object of its own, so nothing of it is there to be found by the slot call"""
    tag, E, keep, sigma_vs, stride, relax, pres = case
    sp, g = plans()
    if pres:
        x, obs = pressure_case(g, E)
        used = lk.obs_space(g, x, obs)["obs_used"]
        assert (used == 0.0).sum() >= 10 and (used == 1.0).sum() >= 100          # a station is out of some member's column
    else:
        x = lk.ensemble(g, E, seed=E)
        obs = lk.clustered_obs(g, x)
    n = len(obs["var"])
    use = None if keep is None else lm.flags(E, keep)
    xd = lk.grids(x)
    for sigma_v in sigma_vs:
        plain, lt = make(sp, E, obs, sigma_v, stride, relax), make(sp, E, obs, sigma_v, stride, relax)
        ref = lk.run(plain, x, use)
        ls.observe_all(lt, [xd] * 4, ls.FIRST(n))
        got = lk.run(lt, x, use, slots=True)
        assert set(got) == set(ref) and ("inflation" in ref) == (relax is not None) and ("weights" in ref) == (stride is not None)
        same(got, ref, sorted(ref), (tag, sigma_v))
        assert all(ref[v].any() for v in lk.VARS) and ref["members_used"].tolist() == [float(E if keep is None else len(keep))]
        if pres:
            assert np.array_equal(got["obs_used"], used)
        # statement 4: one slot is no slot
        lt.set_slots([0, n])
        lt.observe_grid(0, *xd)
        same(lk.run(lt, x, use, slots=True), ref, sorted(ref), (tag, sigma_v, "one slot"))
        plain.close(); lt.close()


def test_no_observation_is_the_plain_call(plans):
    """nobs == 0, every slot empty: nothing to observe, zero increments at rho = 1, as the plain call gives them"""
    sp, g = plans()
    E = 3
    x = lk.ensemble(g, E, seed=1)
    lt = lk.make(sp, E, lk.make_obs([], [], [], [], [], []), 0.1, rho=1.0)
    ref = lk.run(lt, x)
    lt.set_slots([0, 0, 0])
    got = lk.run(lt, x, slots=True)
    for v in lk.VARS:
        assert support.same_bits(got[v], ref[v]) and lm.zero_bits(got[v]), v
    lt.close()


def state_pair(sp, g, oracle, E, nobs=20, seed=52):
    """two Ensembles of the same E seeded members and two analysis objects on one network"""
    sts = es.member_states(sp, E)
    obs = lk.spread_obs(g, lk.oracle_grids(oracle, sts), nobs, seed=seed)
    return es.build(sp, sts), es.build(sp, sts), lk.make(sp, E, obs, 0.1), lk.make(sp, E, obs, 0.1), obs


def test_same_state_from_spectra(plans, oracle_factory):
    """Ensemble.observe for every slot, then Ensemble.analyse(slots=True), against Ensemble.analyse on a copy: the spectra are
    byte-equal, T30 L5, E = 3; and the observes themselves change nothing of the state"""
    import torch
    sp, g = plans("t30k5")
    E = 3
    ens, copy, lt, plain, obs = state_pair(sp, g, oracle_factory("t30k5"), E)
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    lt.set_slots([0, 1, 1, 9, len(obs["var"])])
    for s in range(4):
        ens.observe(lt, s)
    torch.cuda.synchronize()
    for n in es.PROG:
        assert support.same_bits(getattr(ens, n), before[n]), n
    ens.analyse(lt, slots=True)
    copy.analyse(plain)
    torch.cuda.synchronize()
    for n in es.PROG:
        assert support.same_bits(getattr(ens, n), getattr(copy, n)) and not support.same_bits(getattr(ens, n)[0], before[n][0]), n
    for n in lk.FIELDS:
        assert support.same_bits(lt.field(n).numpy(), plain.field(n).numpy()), n
    lt.close(); plain.close()


# ---------------------------------------------------------------------------------------------------- 2. different times
def held_to_the_restatement(sp, g, lt, x, xs, obs, first, E, sigma_v, tag, most=32):
    """The slots observed on xs, the analysis on x = xs[-1], against tests/letkf.py with the library's own stencils: hx, slot_ps,
    slot_out and obs_used exactly; hxmean, y, departure and obs_lnsigma within 16 eps of their scale; every variable's increments
    within lk.limits(...) on the restatement's C and b and the analysis-time ensemble, at the columns lk.columns_for picks
    -> the restatement's obs_space dict and the largest ratio of an error to its limit"""
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=most)
    want = lk.obs_space(g, x, obs, stencil=lp.tables(lt), xs=xs, first=first)
    C, b = lk.problems(g, obs, want, lk.SIGMA_H, sigma_v, cols)
    lim, ref, kappa = lk.limits(g, x, C, b, lk.RHO, cols, E)
    ls.observe_all(lt, xs, first)
    got = lk.run(lt, x, slots=True, names=lk.FIELDS + ("slot_ps", "slot_out"))
    for n in ("hx", "obs_used") + (("slot_ps", "slot_out") if lk.at_pressure(obs).any() else ()):
        assert support.same_bits(got[n], want[n]), (tag, n)
    scale = np.array([np.max(np.abs(x[lk.VARS[v]])) for v in obs["var"]])
    lnscale = np.maximum(np.abs(want["obs_lnsigma"]), 1.0)
    ratios = {}
    for n, sc in (("hxmean", scale), ("y", scale[:, None]), ("departure", scale), ("obs_lnsigma", lnscale)):
        ratios[n] = float(np.max(np.abs(got[n] - want[n]) / (16 * lk.EPS * sc)))
    for v in lk.VARS:
        ratios[v] = float(np.max(np.abs(lk.at_columns(got[v], cols) - ref[v]))) / lim[v]
    print("[letkf slots %s] kappa %.2e, ratio to the limit: %s" % (tag, kappa, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, (tag, ratios)
    return want, got


@pytest.mark.parametrize("E", [4, 17])
def test_different_times_against_restatement(E, plans):
    """S = 3 on ensembles that drift towards the analysed one, the clustered set (1 500) and the sparse set (60), sigma_v = 0.1.  The
    drift matters: the slots' hx differ from the analysed ensemble's by far more than the bound"""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=E)
    xs = ls.drifting(g, x, 3, seed=40 + E)
    for tag, obs, first in (("clustered", lk.clustered_obs(g, x), [0, 300, 701, 1500]), ("sparse", lk.sparse_obs(g, x), [0, 20, 41, 60])):
        lt = lk.make(sp, E, obs, 0.1)
        want, got = held_to_the_restatement(sp, g, lt, x, xs, obs, first, E, 0.1, "E=%d %s" % (E, tag))
        now = lk.observe(g, x, obs)[0]
        assert np.max(np.abs(want["hx"][:first[1]] - now[:first[1]])) > 1e-3 and support.same_bits(got["hx"][first[2]:], want["hx"][first[2]:])
        lt.close()


def different_times_at_pressure(tag, sp, g):
    """E = 4, tests/letkfpressure.py's network, S = 3.  The drift and a push move member 2's ps at one station of slot 1 so that the
    station is below that member's lowest level at its slot's time and inside every column at the analysis time -- asserted with
    the restatement: the slot analysis leaves it out (obs_used 0, from slot_out of that member alone), a plain analysis of the
    analysed ensemble uses it"""
    E, member, slot = 4, 2, 1
    x, obs = pressure_case(g, E, seed=23)
    n = len(obs["var"])
    first = [0, 200, 401, n]
    xs, o = ls.push_out(g, ls.drifting(g, x, 3, seed=44), obs, first, slot, member)
    assert first[slot] <= o < first[slot + 1] and xs[2] is x
    lt = lp.make(sp, E, obs, 0.1)
    want, got = held_to_the_restatement(sp, g, lt, x, xs, obs, first, E, 0.1, "%sE=4 at pressure" % tag)
    assert want["slot_out"][o].tolist() == [1.0 if e == member else 0.0 for e in range(E)] and want["obs_used"][o] == 0.0
    assert lk.obs_space(g, x, obs, stencil=lp.tables(lt))["obs_used"][o] == 1.0
    assert got["obs_used"][o] == 0.0 and (got["obs_used"] == 0.0).sum() >= 10 and (got["obs_used"] == 1.0).sum() >= 100
    lt.close()


def test_different_times_at_pressure(plans):
    """kx = 8: `different_times_at_pressure`"""
    sp, g = plans()
    different_times_at_pressure("", sp, g)


# ---------------------------------------------------------------------------------------------------- 3. slot isolation
@pytest.mark.parametrize("kind", ["model", "pressure"])
def test_an_observe_writes_its_rows_only(kind, plans):
    """hx, slot_ps, slot_out and every per-observation field filled with sentinels; observing slot 2 leaves every bit outside its
    rows of the first three (of hx alone for a model-level network) and all of the others; observing it again on another ensemble
    changes those rows only"""
    sp, g = plans()
    E = 5
    if kind == "pressure":
        x, obs = pressure_case(g, E, seed=25)
    else:
        x = lk.ensemble(g, E, seed=5)
        obs = lk.clustered_obs(g, x, n=700)
    n = len(obs["var"])
    first = [0, 1, 1, 300, n - 37, n]
    r0, r1 = first[2], first[3]
    lt = make(sp, E, obs, 0.1)
    lt.set_slots(first)
    rng = np.random.default_rng(8)
    names = ls.SLOT_FIELDS + ls.PER_OBS + ("y", "value")
    sent = {}
    for name in names:
        f = lt.field(name)
        sent[name] = rng.standard_normal(f.shape) + 1000.0
        f.upload(sent[name])
    written = ls.SLOT_FIELDS if kind == "pressure" else ("hx",)
    seen = {}
    for tag, y in (("first", x), ("second", ls.drifting(g, x, 2, seed=3)[0])):
        lt.observe_grid(2, *lk.grids(y))
        now = {name: lt.field(name).numpy() for name in names}
        idx, wgt = lp.tables(lt)
        want = lk.observe(g, y, lk.subset(obs, slice(r0, r1)), (idx[r0:r1], wgt[r0:r1]), kind == "pressure")
        for name in names:
            if name in written:
                assert support.same_bits(now[name][:r0], sent[name][:r0]) and support.same_bits(now[name][r1:], sent[name][r1:]), (tag, name)
                assert support.same_bits(now[name][r0:r1], want[ls.SLOT_FIELDS.index(name)]), (tag, name)
            else:
                assert support.same_bits(now[name], sent[name]), (tag, name)
        seen[tag] = now
    assert not support.same_bits(seen["first"]["hx"][r0:r1], seen["second"]["hx"][r0:r1])
    lt.close()


# ---------------------------------------------------------------------------------------------------- 4. the late mask
@pytest.mark.parametrize("kind", ["model", "pressure"])
def test_a_member_dropped_at_the_analysis_may_hold_anything(kind, plans):
    """E = 8, S = 3 on drifting ensembles; member 5's grids are NaN, infinite or 1e300 from slot 1 on, the analysed ensemble
    included, and the mask of the analysis call drops it: the members in use, y and hx at them and every per-observation field
    are bit for bit those of a 7-member object that observed the same slots on the compacted ensembles; member 5 gets exactly 0.0"""
    sp, g = plans()
    E, drop = 8, 5
    keep = tuple(e for e in range(E) if e != drop)
    if kind == "pressure":
        x = lp.craft(g, E, seed=27)
        obs = lp.network(g, lk.compact(x, keep))
    else:
        x = lk.ensemble(g, E, seed=8)
        obs = lk.concat(lk.clustered_obs(g, lk.compact(x, keep), n=600), lk.sparse_obs(g, lk.compact(x, keep)))
    n = len(obs["var"])
    first = [0, 150, 333, n]
    xs = ls.drifting(g, x, 3, seed=12)
    lt, ltc = make(sp, E, obs, 0.1), make(sp, len(keep), obs, 0.1)
    ls.observe_all(ltc, [lk.compact(a, keep) for a in xs], first)
    ref = lk.run(ltc, lk.compact(x, keep), slots=True)
    if kind == "pressure":
        assert (ref["obs_used"] == 0.0).sum() >= 5 and (ref["obs_used"] == 1.0).sum() >= 100
    for bad in ("nan", "inf", "1e300"):
        ys = [xs[0]] + [{v: a.copy() for v, a in y.items()} for y in xs[1:]]
        for y in ys[1:]:
            for v in lk.VARS:
                for f in y[v][drop].reshape((-1,) + y[v].shape[-2:]):
                    poison.poison(f, bad)
        ls.observe_all(lt, ys, first)
        got = lk.run(lt, ys[2], lm.flags(E, keep), slots=True)
        lm.same_as_compact(got, ref, E, keep, (kind, bad))
    lt.close(); ltc.close()


# ---------------------------------------------------------------------------------------------------- 5. refusals on the device
def test_refusals_enqueue_nothing(plans, oracle_factory):
    """a non-empty slot unobserved: SPDY_ERR_STATE naming it, the state and the fields keep their bits; observing it lets the call
    through; a new set_slots forgets the marks; after set_obs the slots are gone"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans("t30k5")
    E = 3
    ens, _, lt, plain, obs = state_pair(sp, g, oracle_factory("t30k5"), E)
    plain.close()
    n = len(obs["var"])
    ens.analyse(lt)                                           # fields of a plain call to be kept
    torch.cuda.synchronize()
    before = {k: getattr(ens, k).clone() for k in es.PROG}
    fields = {k: lt.field(k).numpy() for k in lk.FIELDS}
    lt.set_slots([0, 5, 5, n])
    ens.observe(lt, 0)
    ens.observe(lt, 1)                                        # the empty one
    torch.cuda.synchronize()
    fields["hx"] = lt.field("hx").numpy()
    xg = [torch.zeros((E, sp.kx) + sp.grid_shape, dtype=torch.float64, device="cuda") for _ in range(4)]
    xg.append(torch.zeros((E,) + sp.grid_shape, dtype=torch.float64, device="cuda"))
    out = [torch.full_like(a, 7.0) for a in xg]
    for call in (lambda: ens.analyse(lt, slots=True), lambda: lt.analyse_grid(*xg, out=out, slots=True)):
        with pytest.raises(s.SpdyError, match="slot 2 has not been observed") as e:
            call()
        assert e.value.code == ERR_STATE
    torch.cuda.synchronize()
    for k in es.PROG:
        assert support.same_bits(getattr(ens, k), before[k]), k
    for k in lk.FIELDS:
        assert support.same_bits(lt.field(k).numpy(), fields[k]), k
    assert all(bool((a == 7.0).all()) for a in out)
    ens.observe(lt, 2)
    ens.analyse(lt, slots=True)
    torch.cuda.synchronize()
    assert not support.same_bits(ens.t[0], before["t"][0])
    lt.set_slots([0, 5, 5, n])                                # the marks are of the latest set_slots
    with pytest.raises(s.SpdyError, match="slot 0 has not been observed"):
        ens.analyse(lt, slots=True)
    lt.set_obs(*lk.args(obs))
    assert lt.slots is None and lt.table("slot_first").shape == (0,)
    for call in (lambda: ens.analyse(lt, slots=True), lambda: ens.observe(lt, 0)):
        with pytest.raises(s.SpdyError, match="spdy_slot_set first") as e:
            call()
        assert e.value.code == ERR_STATE
    ens.analyse(lt)                                           # the plain call is what it was
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. capture
@pytest.mark.parametrize("E", [2, 17])
def test_capture(E, plans):
    """{observe slot 0 on one ensemble, observe slot 1 on a second, the slot analysis of the second with out= given} as one graph:
    the analysis contributes the plain call's node count and each observe one node; two replays equal the eager calls and each
    other bit for bit; with new contents written into the captured tensors a replay equals the eager calls on those contents"""
    import torch
    sp, g = plans()
    x = lk.ensemble(g, E, seed=30 + E)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    n = len(obs["var"])
    first = [0, 123, n]
    lt = lk.make(sp, E, obs, 0.1)
    eager = {}
    for tag, seed in (("a", 1), ("b", 2)):
        xs = ls.drifting(g, x if tag == "a" else lk.ensemble(g, E, seed=77), 2, seed=seed)
        ls.observe_all(lt, xs, first)
        eager[tag] = (xs, lk.run(lt, xs[1], slots=True))
    assert not support.same_bits(eager["a"][1]["t"], eager["b"][1]["t"])
    xa, xb = (lk.grids(y) for y in eager["a"][0])
    out = tuple(torch.empty_like(a) for a in xb)
    lt.set_slots(first)
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as plain:
            lt.analyse_grid(*xb, out=out)
        base = plain.num_nodes()
        plain.close()
        with sp.graph_capture() as one:
            lt.observe_grid(0, *xa)
        assert one.num_nodes() == 1, one.num_nodes()
        one.close()
        with sp.graph_capture() as gr:
            lt.observe_grid(0, *xa)
            lt.observe_grid(1, *xb)
            lt.analyse_grid(*xb, out=out, slots=True)
        assert base == 2 and gr.num_nodes() == base + 2, (base, gr.num_nodes())
        runs = []
        for tag in ("a", "a", "b"):
            for dst, src in zip(xa + xb, lk.grids(eager[tag][0][0]) + lk.grids(eager[tag][0][1])):
                dst.copy_(src)
            for name in ("hx", "y", "hxmean", "departure"):
                f = lt.field(name)
                f.upload(np.full(f.shape, -3.0))
            for a in out:
                a.fill_(-3.0)
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            got = {v: a.cpu().numpy() for v, a in zip(lk.VARS, out)}
            got.update({name: lt.field(name).numpy() for name in lk.FIELDS})
            same(got, eager[tag][1], lk.VARS + lk.FIELDS, (E, tag))
            runs.append(got)
        same(runs[0], runs[1], lk.VARS + lk.FIELDS, (E, "replays"))
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 7. the nature run by slots
@pytest.mark.parametrize("kind", ["model", "pressure"])
def test_nature_observes_a_slot(kind, plans):
    """Nature.observe(letkf, slot=s) writes the slot's values -- the bits the whole network's call gives them at the same draw
    count -- and leaves the others; draws advances by one, for an empty slot too; noise = 0 gives H(truth) on the range; the slots
    one after the other on a moving truth give each range its own time's values"""
    import speedy_f90_amd as s
    sp, g = plans()
    E, seed = 4, 0x51075
    if kind == "pressure":
        x, obs = pressure_case(g, E, seed=29)
    else:
        x = lk.ensemble(g, E, seed=9)
        obs = lk.clustered_obs(g, x, n=700)
    n = len(obs["var"])
    first = [0, 1, 1, 300, n]
    lt = make(sp, E, obs, 0.1)
    nat = s.Nature(sp, seed=seed, capacity=1)
    truths = [nt.as_truth(x, e) for e in range(3)]
    whole = []
    for d, noise in ((0, 0.75), (1, 0.0), (2, 0.75), (3, 0.75)):      # the whole network at draws 0 .. 3 on truth 0, 0, 1, 2
        nat.field("truth").upload(nt.rows(truths[max(d - 1, 0)]))
        nat.observe(lt, noise)
        whole.append(lt.field("value").numpy())
    assert nat.draws() == 4 and support.same_bits(whole[1], lp.truth_values(g, truths[0], obs, lp.tables(lt)))
    assert not support.same_bits(whole[2][300:], whole[3][300:])
    lt.set_slots(first)
    sent = np.random.default_rng(4).standard_normal(n) + 500.0
    nat.reset(seed)
    nat.field("truth").upload(nt.rows(truths[0]))
    lt.field("value").upload(sent)
    nat.observe(lt, 0.75, slot=2)                                      # draws 0
    got = lt.field("value").numpy()
    assert support.same_bits(got[1:300], whole[0][1:300]) and support.same_bits(got[:1], sent[:1]) and support.same_bits(got[300:], sent[300:])
    nat.observe(lt, 0.0, slot=0)                                       # draws 1
    nat.field("truth").upload(nt.rows(truths[1]))
    assert nat.draws() == 2
    nat.observe(lt, 0.75, slot=1)                                      # draws 2, the empty slot: counts, writes nothing
    nat.observe(lt, 0.75, slot=3)                                      # draws 3, on truth 1: the whole network's draw 3 was on truth 2
    got2 = lt.field("value").numpy()
    assert nat.draws() == 4
    assert support.same_bits(got2[:1], whole[1][:1]) and support.same_bits(got2[1:300], got[1:300])
    nat.reset(seed)
    for _ in range(3):
        nat.observe(lt, 0.0, slot=1)
    nat.observe(lt, 0.75)                                              # the whole network at draws 3 on truth 1
    assert support.same_bits(got2[300:], lt.field("value").numpy()[300:])
    nat.close(); lt.close()


# ---------------------------------------------------------------------------------------------------- 8. the cycle in one graph
def test_the_cycle_in_one_graph(plans, oracle_factory):
    """{forecast; Nature.set_state; Nature.observe(slot=s); Ensemble.observe(s)} for three slots, the middle one empty, then verify,
    Ensemble.analyse(slots=True), verify, T30 L5, E = 3.  The forecast between two slots is stood in for by a capturable call that
    moves every member's state and is known to keep it finite on these seeded states, a plain analysis with a second object (the
    states are synthetic: several model steps from them are not a forecast).  The rows of the first slot are those of the state one
    such call in, not of the analysed state; the rows of the last slot -- observed on the analysed state -- are the plain call's bit
    for bit; and the whole cycle captured as one graph leaves the spectra, the scores, the values and hx of the eager cycle"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans("t30k5")
    E, seed = 3, 0x4D
    ens, _, lt, mover, obs = state_pair(sp, g, oracle_factory("t30k5"), E)
    n = len(obs["var"])
    nat = s.Nature(sp, seed=seed, capacity=2)
    x0 = {k: getattr(ens, k).clone() for k in es.PROG}
    tr = [x0[k][0, 0].clone() for k in es.PROG]
    lt.set_slots([0, 7, 7, n])

    def forecast(sl):
        ens.analyse(mover)
        nat.set_state(*tr)
        nat.observe(lt, 1.0, slot=sl)
        ens.observe(lt, sl)

    def cycle():
        for sl in range(3):
            forecast(sl)
        ens.verify(lt, nat, 0)
        ens.analyse(lt, slots=True)
        ens.verify(lt, nat, 1)

    def restore():
        for k in es.PROG:
            getattr(ens, k).copy_(x0[k])
        nat.reset(seed)

    def result():
        out = {k: getattr(ens, k).clone() for k in es.PROG}
        out.update({k: torch.from_numpy(lt.field(k).numpy()) for k in ("hx", "value") + ls.PER_OBS})
        out["scores"] = torch.from_numpy(nat.field("scores").numpy())
        return out

    cycle()
    torch.cuda.synchronize()
    eager = result()
    assert nat.draws() == 3 and not support.same_bits(eager["t"][0], x0["t"][0]) and bool(torch.isfinite(eager["scores"]).all())
    restore()
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            cycle()
        for r in range(2):
            restore()
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            got = result()
            for k in eager:
                assert support.same_bits(got[k], eager[k]), (r, k)
        gr.close()
    finally:
        sp.use_torch_stream()
    # every observation dated at the analysis time: the plain call on the state the three forecasts leave, with the cycle's values
    restore()
    for _ in range(3):
        ens.analyse(mover)
    plain = lk.make(sp, E, dict(obs, value=eager["value"].numpy()), 0.1)
    ens.analyse(plain)
    torch.cuda.synchronize()
    now = plain.field("hx").numpy()
    assert support.same_bits(eager["hx"].numpy()[7:], now[7:]) and not np.array_equal(eager["hx"].numpy()[:7], now[:7])
    assert not support.same_bits(ens.t[0], eager["t"][0])
    nat.close(); lt.close(); mover.close(); plain.close()


# ---------------------------------------------------------------------------------------------------- 9. on the T63 L16 grid
@pytest.mark.parametrize("E", [4, 17])
def test_different_times_against_restatement_t63(E, plans):
    """192 x 96 x 16, sigma_v = 0.1: three times on ensembles that drift towards the analysed one, first = FIRST(nobs) -- a
    one-observation slot, an empty one (it shares the first time), a boundary inside a chunk, a long tail -- on a model-level network
    of a cluster of 600 and the sparse set: `held_to_the_restatement`"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    x = lk.ensemble(g, E, seed=E)
    a, b, _ = ls.drifting(g, x, 3, seed=40 + E, passes=2)
    xs = [a, a, b, x]
    obs = lk.concat(lk.clustered_obs(g, x, n=600), lk.sparse_obs(g, x))
    first = ls.FIRST(len(obs["var"]))
    lt = lk.make(sp, E, obs, 0.1)
    want, got = held_to_the_restatement(sp, g, lt, x, xs, obs, first, E, 0.1, "T63 L16 E=%d" % E)
    now = lk.observe(g, x, obs)[0]
    assert np.max(np.abs(want["hx"][:first[3]] - now[:first[3]])) > 1e-3 and support.same_bits(got["hx"][first[3]:], want["hx"][first[3]:])
    lt.close()


def test_different_times_at_pressure_t63(plans):
    """192 x 96 x 16: `different_times_at_pressure`"""
    sp, g = plans(T63)
    different_times_at_pressure("T63 L16 ", sp, g)


def test_capture_everything_t63(plans):
    """192 x 96 x 16, the object with every feature on (tests/letkfslots.py's EVERYTHING; tests/test_gpu_letkf.py holds it to the
    restatement), two slots: {observe slot 0 on the earlier ensemble, observe slot 1 on the analysed one, the masked slot analysis
    with out= given} as one graph.  Three replays from the restored inflation field equal three eager calls in every bit of the
    increments, the fields, the statistics and the field, which the graph advances by itself.  The nodes are the header's counts:
    each observe one; the analysis on grids two, and one more each for the weight stride, the relaxation, the member mask and the
    background check, two more for adaptive inflation"""
    import torch
    sp, g = plans(T63)
    c = ls.EVERYTHING
    case = ls.everything_inputs(g, S=2, first_of=lambda n: [0, 400, n])
    xs, first, keep = case["xs"], case["first"], case["keep"]
    lt = ls.everything_object(sp, case)
    field = case["field"].reshape((sp.kx,) + sp.grid_shape)
    use = torch.tensor(lm.flags(c["E"], keep), dtype=torch.int32, device="cuda")
    xa, xb = lk.grids(xs[0]), lk.grids(xs[1])
    out = tuple(torch.empty_like(a) for a in xb)
    names = lk.FIELDS + ("slot_ps", "slot_out", "obs_check", "obs_rinv", "obs_s2", "rho", "infl_parm", "inflation", "weights", "obs_stats")
    lt.set_slots(first)

    def cycle():
        lt.observe_grid(0, *xa)
        lt.observe_grid(1, *xb)
        lt.analyse_grid(*xb, out=out, use=use, slots=True)

    def result():
        got = {v: a.cpu().numpy() for v, a in zip(lk.VARS, out)}
        got.update({name: lt.field(name).numpy() for name in names})
        return got

    eager = []
    for _ in range(3):
        cycle()
        torch.cuda.synchronize()
        eager.append(result())
    assert all(eager[0][v].any() for v in lk.VARS) and (eager[0]["obs_check"] == 1.0).any() and (eager[0]["obs_check"] == 2.0).any()
    assert not support.same_bits(eager[0]["rho"], eager[1]["rho"]) and not support.same_bits(eager[1]["rho"], eager[2]["rho"])
    assert not support.same_bits(eager[0]["t"], eager[1]["t"])
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            cycle()
        assert gr.num_nodes() == 2 + (2 + 1 + 1 + 1 + 1 + 2), gr.num_nodes()
        lt.inflation_field().upload(field)
        for r in range(3):
            for name in ("hx", "y", "hxmean", "departure", "obs_check", "obs_rinv"):
                f = lt.field(name)
                f.upload(np.full(f.shape, -3.0))
            for a in out:
                a.fill_(-3.0)
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            got = result()
            same(got, eager[r], lk.VARS + names, ("replay", r))
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()
