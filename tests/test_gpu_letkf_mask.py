"""GPU: the member mask of the analysis and the scores (include/spdy.h, "member mask"; use= of Ensemble.analyse, Ensemble.verify,
Letkf.analyse_grid, Nature.verify_grid; Diagnostics.use_dev).  The central statement needs no tolerance: a masked
call on E members equals, for the members in use and bit for bit, the unmasked call of an object of those n members on the
compacted ensemble -- a path the existing tests hold to the NumPy restatement.  T30; the section "on the T63 L16 grid" repeats the
central statement, the restatement and the unread member at 192 x 96 x 16."""
import numpy as np
import pytest

import diagnostics as dg
import ensemblestep as es
import letkf as lk
import letkfmask as lm
import letkfpressure as lp
import nature as nt
import poison
import support

pytestmark = pytest.mark.gpu

# (E, the members in use): n = 2 of 3; n = 7, odd, the decoupled row; n = 14 of 17; n = 31 of 32; n = 2 of 32
CASES = [(3, (1, 2)), (8, tuple(range(7))), (17, tuple(e for e in range(17) if e not in (0, 5, 16))),
         (32, tuple(e for e in range(32) if e != 13)), (32, (2, 30))]
IDS = ["E3-drop0", "E8-drop7", "E17-drop0,5,16", "E32-drop13", "E32-keep2,30"]
KEEP17 = CASES[2][1]


T63 = "t63k16"


def _plan(tag, nmem):
    sp = support.ensemble_plan(tag, nmem)
    return sp, lp.Geometry(sp)


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_plan, plan_of=lambda made: made[0]) as get:
        yield lambda tag="t30", nmem=32: get(tag, nmem)


def both_sets(g, xc):
    return (("clustered", lk.clustered_obs(g, xc)), ("sparse", lk.sparse_obs(g, xc)))


# ---------------------------------------------------------------------------------------------------- 1. bit-equality on grids
@pytest.mark.parametrize("E,keep", CASES, ids=IDS)
def test_masked_equals_compact(E, keep, plans):
    """kx = 8, the clustered set (1 500 observations in range of one column: more than three scan chunks) and the sparse set, with
    and without the vertical factor: du .. dps, y and hx at the members in use, hxmean, departure and members_used have the bits
    of the n-member object; the members not in use get exactly 0.0"""
    sp, g = plans()
    x = lk.ensemble(g, E, seed=E)
    xc = lk.compact(x, keep)
    for tag, obs in both_sets(g, xc):
        for sigma_v in (0.0, 0.1):
            lt, ltc = lk.make(sp, E, obs, sigma_v), lk.make(sp, len(keep), obs, sigma_v)
            got, ref = lk.run(lt, x, lm.flags(E, keep)), lk.run(ltc, xc)
            lm.same_as_compact(got, ref, E, keep, (tag, sigma_v))
            lt.close(); ltc.close()


@pytest.mark.parametrize("kx", [16, 14])
def test_masked_equals_compact_many_levels(kx):
    """E = 32 without member 0 at kx = 16 (one level in flight) and kx = 14 (two): the launch shape, the levels in flight and the
    LDS request are those of 32 members, the problem solved is that of 31"""
    import speedy_f90_amd as s
    E, keep = 32, tuple(range(1, 32))
    sp = s.Spectral("t30", kx=kx, max_batch=E * (2 * kx + 1), device=0)
    sp.set_sigma(np.linspace(0.0, 1.0, kx + 1) ** 1.5)
    g = lk.Geometry(sp)
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lambda g, xc: lk.concat(lk.clustered_obs(g, xc, n=300), lk.sparse_obs(g, xc)), 0.1)
    lm.same_as_compact(lk.run(lt, x, lm.flags(E, keep)), lk.run(ltc, xc), E, keep, kx)
    sp.close()


# ---------------------------------------------------------------------------------------------------- 2. against the restatement
def masked_against_restatement(tag, sp, g):
    """E = 8 without member 7, the clustered set: the masked increments against tests/letkf.py's analysis of the seven members,
    within that module's limits(...), the bound of the existing analysis tests"""
    E, keep = 8, tuple(range(7))
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lk.clustered_obs, 0.1)
    ltc.close()
    cols = lk.columns_for(g, obs, lk.SIGMA_H, most=32)
    C, b = lk.problems(g, obs, lk.obs_space(g, xc, obs), lk.SIGMA_H, 0.1, cols)
    lim, ref, kappa = lk.limits(g, xc, C, b, lk.RHO, cols, len(keep))
    got = lk.run(lt, x, lm.flags(E, keep))
    lt.close()
    worst = {v: float(np.max(np.abs(lk.at_columns(got[v][list(keep)], cols) - ref[v]))) / lim[v] for v in lk.VARS}
    print("[letkf mask %sE=8 n=7] kappa %.2e, ratio to the limit: %s" % (tag, kappa, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_masked_against_restatement(plans):
    """kx = 8: `masked_against_restatement`"""
    sp, g = plans()
    masked_against_restatement("", sp, g)


# ---------------------------------------------------------------------------------------------------- 3. a member not in use is not read
def unused_member_reaches_nothing(sp, g, drop):
    """E = 8, one member not in use holding NaN, infinities of both signs and 1e300: every output for the members in use, and the
    per-observation fields, keep the bits of the call with ordinary values there; its own increments and y are 0.0"""
    E = 8
    keep = tuple(e for e in range(E) if e != drop)
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lambda g, xc: lk.concat(lk.clustered_obs(g, xc, n=300), lk.sparse_obs(g, xc)), 0.1)
    ltc.close()
    clean = lk.run(lt, x, lm.flags(E, keep))
    for kind in ("nan", "inf", "1e300"):
        y = {v: a.copy() for v, a in x.items()}
        for v in lk.VARS:
            for f in y[v][drop].reshape((-1,) + y[v].shape[-2:]):
                poison.poison(f, kind)
        got = lk.run(lt, y, lm.flags(E, keep))
        for v in lk.VARS:
            assert support.same_bits(got[v], clean[v]), (kind, v)
        for n in lm.OBS_FIELDS + ("y", "members_used"):
            assert support.same_bits(got[n], clean[n]), (kind, n)
        assert support.same_bits(np.ascontiguousarray(got["hx"][:, keep]), np.ascontiguousarray(clean["hx"][:, keep])), kind
        assert all(np.isfinite(got[v]).all() for v in lk.VARS), kind
    lt.close()


@pytest.mark.parametrize("drop", [3, 7])
def test_unused_member_reaches_nothing_on_grids(drop, plans):
    """kx = 8: `unused_member_reaches_nothing`"""
    sp, g = plans()
    unused_member_reaches_nothing(sp, g, drop)


def state_pair(sp, g, oracle, E, keep, nobs=20, seed=52):
    """an Ensemble of E seeded members, the Ensemble of the members `keep`, and their analysis objects on one network"""
    sts = es.member_states(sp, E)
    part = [sts[e] for e in keep]
    obs = lk.spread_obs(g, lk.oracle_grids(oracle, part), nobs, seed=seed)
    return es.build(sp, sts), es.build(sp, part), lk.make(sp, E, obs, 0.1), lk.make(sp, len(keep), obs, 0.1)


def test_unused_member_keeps_its_state(plans, oracle_factory):
    """Ensemble.analyse(use=...), T30 L5, E = 4 without member 2, whose time level 1 is NaN: its vor, div, t, tr, ps are byte-equal
    before and after, and the other three are bit-equal to a 3-member Ensemble analysed by a 3-member Letkf"""
    import torch
    sp, g = plans("t30k5")
    E, keep, drop = 4, (0, 1, 3), 2
    ens, ensc, lt, ltc = state_pair(sp, g, oracle_factory("t30k5"), E, keep)
    for n in es.PROG:
        getattr(ens, n)[0, drop] = complex(float("nan"), float("nan"))
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.analyse(lt, use=lm.flags(E, keep))
    ensc.analyse(ltc)
    torch.cuda.synchronize()
    for n in es.PROG:
        a, c = getattr(ens, n), getattr(ensc, n)
        assert support.same_bits(a[0, drop], before[n][0, drop]), n
        assert support.same_bits(a[1], before[n][1]), n                                  # time level 2
        assert support.same_bits(a[0, list(keep)], c[0]) and not support.same_bits(a[0, list(keep)], before[n][0, list(keep)]), n
    assert lt.field("members_used").numpy().tolist() == [3.0]
    lt.close(); ltc.close()


# ---------------------------------------------------------------------------------------------------- 4. the old paths
def test_unmasked_paths_are_what_they_were(plans):
    """use=None, a mask of all ones and the unsuffixed C call give equal bits; members_used is nmem after the unmasked calls"""
    import ctypes
    import torch
    sp, g = plans()
    E = 17
    x = lk.ensemble(g, E, seed=3)
    obs = lk.concat(lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
    lt = lk.make(sp, E, obs, 0.1)
    none = lk.run(lt, x)
    ones = lk.run(lt, x, [1] * E)
    xs = lk.grids(x)
    out = [torch.empty_like(a) for a in xs]
    sp._sync_stream()
    assert sp.lib.spdy_letkf_analyse_grid_dev(lt.h, *[ctypes.c_void_p(a.data_ptr()) for a in xs + out]) == 0
    torch.cuda.synchronize()
    for v, a in zip(lk.VARS, out):
        assert support.same_bits(none[v], ones[v]) and support.same_bits(none[v], a.cpu().numpy()), v
    for n in lm.OBS_FIELDS + ("y", "hx", "members_used"):
        assert support.same_bits(none[n], ones[n]), n
    assert none["members_used"].tolist() == [float(E)] == lt.field("members_used").numpy().tolist()
    lt.close()


@pytest.mark.parametrize("E", [4, 17])
def test_capture_follows_the_mask(E, plans, oracle_factory):
    """A captured unmasked Ensemble.analyse still has five kernel nodes, the masked one six (include/spdy.h, "member mask":
    launches).  The masked graph holds the mask's pointer: with other contents written in place, a replay from the same state
    equals the eager call with that mask bit for bit"""
    import torch
    sp, g = plans("t30k5")
    first, second = [1] * E, [0 if e == 1 else 1 for e in range(E)]
    ens, _, lt, ltc = state_pair(sp, g, oracle_factory("t30k5"), E, tuple(range(E)))
    ltc.close()
    x0 = {n: getattr(ens, n).clone() for n in es.PROG}
    eager = {}
    for name, mask in (("first", first), ("second", second)):
        ens.analyse(lt, use=mask)
        torch.cuda.synchronize()
        eager[name] = {n: getattr(ens, n).clone() for n in es.PROG}
        for n in es.PROG:
            getattr(ens, n).copy_(x0[n])
    assert not support.same_bits(eager["first"]["t"], eager["second"]["t"])
    use = torch.tensor(first, dtype=torch.int32, device="cuda")
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as plain:
            ens.analyse(lt)
        assert plain.num_nodes() == 5, plain.num_nodes()
        plain.close()
        with sp.graph_capture() as gr:
            ens.analyse(lt, use=use)
        assert gr.num_nodes() == 6, gr.num_nodes()
        for name, mask in (("first", first), ("second", second), ("first", first)):
            use.copy_(torch.tensor(mask, dtype=torch.int32))
            for n in es.PROG:
                getattr(ens, n).copy_(x0[n])
            torch.cuda.synchronize()
            gr.launch()
            sp.synchronize()
            for n in es.PROG:
                assert support.same_bits(getattr(ens, n), eager[name][n]), (name, n)
        gr.close()
    finally:
        sp.use_torch_stream()
    lt.close()


# ---------------------------------------------------------------------------------------------------- 6. observations at a pressure
def test_pressure_network(plans):
    """tests/letkfpressure.py's crafted ensemble: member 1 alone has high terrain in a patch, so the stations there at the lowest
    pressures are out of its column and of nobody else's.  With all members they are rejected; with member 1 not in use they
    have obs_used == 1, and every field -- obs_lnsigma, from the mean ps of the members in use, among them -- and every
    increment is bit-equal to the object of the other members"""
    sp, g = plans("t30")
    E, drop = 5, lp.PATCH_MEMBER
    keep = tuple(e for e in range(E) if e != drop)
    x = lp.craft(g, E, seed=21)
    xc = lk.compact(x, keep)
    obs = lp.network(g, xc)
    lt, ltc = lp.make(sp, E, obs, 0.1), lp.make(sp, len(keep), obs, 0.1)
    full = lk.run(lt, x)
    got, ref = lk.run(lt, x, lm.flags(E, keep)), lk.run(ltc, xc)
    regained = (full["obs_used"] == 0.0) & (got["obs_used"] == 1.0)
    assert regained.sum() >= 8 and (got["obs_used"] == 0.0).sum() >= 10, (regained.sum(), (got["obs_used"] == 0.0).sum())
    assert not support.same_bits(full["obs_lnsigma"], got["obs_lnsigma"])
    lm.same_as_compact(got, ref, E, keep, "pressure")
    lt.close(); ltc.close()


# ---------------------------------------------------------------------------------------------------- 7. weight interpolation
def weight_stride(sp, g):
    """stride (2, 2), E = 17 without members 0, 5 and 16: the increments are bit-equal to the 14-member object's at that stride, and
    the leading 14 x 14 block of every matrix of `weights`, in compact indices, is its `weights`"""
    E, keep = 17, KEEP17
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lambda g, xc: lk.concat(lk.clustered_obs(g, xc, n=300), lk.sparse_obs(g, xc)), 0.1,
                                  stride=(2, 2))
    got, ref = lk.run(lt, x, lm.flags(E, keep)), lk.run(ltc, xc)
    lm.same_as_compact(got, ref, E, keep, "stride")
    w, wc = lt.field("weights").numpy(), ltc.field("weights").numpy()
    assert w.shape[2:] == (E, E) and wc.shape[2:] == (14, 14) and wc.any()
    assert support.same_bits(np.ascontiguousarray(w[:, :, :14, :14]), wc)
    lt.close(); ltc.close()


def test_weight_stride(plans):
    """kx = 8: `weight_stride`"""
    sp, g = plans()
    weight_stride(sp, g)


# ---------------------------------------------------------------------------------------------------- 8. fewer than two members
@pytest.mark.parametrize("keep", [(2,), ()], ids=["one", "none"])
@pytest.mark.parametrize("stride", [(1, 1), (2, 2)])
def test_fewer_than_two_members(keep, stride, plans, oracle_factory):
    """One member in use and none: all-zero increments with the clustered observations in range, at both kinds of stride, and an
    Ensemble's state keeps its bytes.  hxmean is the member's own hx, and NaN without a member"""
    import torch
    sp, g = plans("t30k5")
    E = 4
    x = lk.ensemble(g, E, seed=9)
    lt = lk.make(sp, E, lk.clustered_obs(g, x, n=300), 0.1)
    lt.set_weight_stride(*stride)
    got = lk.run(lt, x, lm.flags(E, keep))
    for v in lk.VARS:
        assert lm.zero_bits(got[v]), v
    assert got["members_used"].tolist() == [float(len(keep))]
    assert support.same_bits(got["hxmean"], np.ascontiguousarray(got["hx"][:, keep[0]])) if keep else np.isnan(got["hxmean"]).all()
    lt.close()
    if stride != (1, 1):
        return
    ens, _, lt, ltc = state_pair(sp, g, oracle_factory("t30k5"), E, tuple(range(E)))
    ltc.close()
    before = {n: getattr(ens, n).clone() for n in es.PROG}
    ens.analyse(lt, use=lm.flags(E, keep))
    torch.cuda.synchronize()
    for n in es.PROG:
        assert support.same_bits(getattr(ens, n), before[n]), n
    lt.close()


# ---------------------------------------------------------------------------------------------------- 9. the scores
def test_scores(plans, oracle_factory):
    """E = 8 without members 2 and 5: verify_grid(use=...) equals verify_grid of the six members bit for bit, and so does
    Ensemble.verify(use=...) on the grids it made; with a NaN member masked all scores are finite; one member gives spread +0,
    none NaN"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans("t30k5")
    E, keep = 8, (0, 1, 3, 4, 6, 7)
    nat = s.Nature(sp, capacity=3)
    x = lk.ensemble(g, E, seed=77)
    nat.field("truth").upload(nt.rows(nt.as_truth(lk.ensemble(g, 1, seed=78))))
    xc = lk.compact(x, keep)
    nat.verify_grid(*lk.grids(x), slot=0, use=lm.flags(E, keep))
    nat.verify_grid(*lk.grids(xc), slot=1)
    nat.verify_grid(*lk.grids(x), slot=2)
    sc = nat.field("scores").numpy()
    assert support.same_bits(sc[0], sc[1]) and not support.same_bits(sc[0], sc[2]) and np.isfinite(sc).all() and sc[0].all()
    y = {v: a.copy() for v, a in x.items()}
    for v in lk.VARS:
        y[v][[2, 5]] = np.nan
    nat.verify_grid(*lk.grids(y), slot=2, use=lm.flags(E, keep))
    sc = nat.field("scores").numpy()
    assert support.same_bits(sc[2], sc[1])
    nat.verify_grid(*lk.grids(y), slot=0, use=lm.flags(E, (4,)))
    nat.verify_grid(*lk.grids(y), slot=2, use=[0] * E)
    sc = nat.field("scores").numpy()
    assert np.isfinite(sc[0]).all() and sc[0, :2].all() and lm.zero_bits(sc[0, 2]) and np.isnan(sc[2]).all()
    # from spectra: the masked verify against verify_grid of the grids that call left in the analysis object's workspace
    ens, _, lt, ltc = state_pair(sp, g, oracle_factory("t30k5"), E, tuple(range(E)))
    ltc.close()
    nat.set_state(*[getattr(ens, n)[0, 0] for n in es.PROG])
    for n in es.PROG:
        getattr(ens, n)[0, 5] = complex(float("nan"), float("nan"))
    ens.verify(lt, nat, slot=0, use=lm.flags(E, keep))
    torch.cuda.synchronize()
    grid = lt.field("grid").numpy()
    kx = sp.kx
    gx = {v: grid[i * E * kx:(i + 1) * E * kx].reshape((E, kx) + sp.grid_shape) for i, v in enumerate(lk.VARS[:4])}
    gx["ps"] = grid[4 * E * kx:]
    nat.verify_grid(*lk.grids(lk.compact(gx, keep)), slot=1)
    sc = nat.field("scores").numpy()
    assert support.same_bits(sc[0], sc[1]) and np.isfinite(sc[0]).all() and sc[0, 2].all()
    lt.close(); nat.close()


# ---------------------------------------------------------------------------------------------------- 10. from the guard to the mask
def test_guard_to_mask(plans):
    """Seeded states of E = 4 members, the reke limit between the largest value of the member that has the largest and everybody
    else's: that member trips.  use_dev() equals [s == -1 for s in stopped()], eagerly and as a captured node, and stays 0 for the
    member after a later in-range step, because the record is sticky"""
    import speedy_f90_amd as s
    import torch
    sp, g = plans("t30k5")
    E = 4
    sts = [dg.state(sp, 5100 + 100 * e) for e in range(E)]
    x = {n: np.stack([st[n] for st in sts]) for n in ("vor", "div", "t")}
    reke = np.array([dg.diag(st["vor"], st["div"], st["t"], sp.table("elm2"))[0].max() for st in sts])
    order = np.argsort(reke)
    chosen, top, second = int(order[-1]), float(reke[order[-1]]), float(reke[order[-2]])
    assert second < top * (1 - 1e-6) and top < dg.LIMITS[0]
    G = s.Diagnostics(sp, capacity=4, nmem=E)
    lim = list(dg.LIMITS)
    lim[0] = 0.5 * (top + second)
    G.set_limits(lim)
    dev = [support.dev(x[n]) for n in ("vor", "div", "t")]
    assert G.use_dev().tolist() == [1] * E
    G.check_dev(*dev)
    want = [1 if e != chosen else 0 for e in range(E)]
    assert [int(b == -1) for b in G.stopped()] == want == G.use_dev().tolist()
    calm = [a.clone() for a in dev]
    calm[0][chosen] *= 0.5                                              # the member back in range: a quarter of its reke
    G.check_dev(*calm)
    assert G.stopped()[chosen] == 0 and G.status(chosen)["next_step"] == 2
    out = torch.full((E,), 7, dtype=torch.int32, device="cuda")
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as gr:
            G.use_dev(out)
        assert gr.num_nodes() == 1, gr.num_nodes()
        gr.launch()
        sp.synchronize()
        gr.close()
    finally:
        sp.use_torch_stream()
    assert out.tolist() == want
    G.close()


# ---------------------------------------------------------------------------------------------------- 11. determinism
def test_two_masked_runs_are_bit_equal(plans):
    sp, g = plans()
    E, keep = 17, KEEP17
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lk.clustered_obs, 0.1)
    ltc.close()
    a, b = lk.run(lt, x, lm.flags(E, keep)), lk.run(lt, x, lm.flags(E, keep))
    for n in a:
        assert support.same_bits(a[n], b[n]), n
    lt.close()


# ---------------------------------------------------------------------------------------------------- 12. on the T63 L16 grid
def test_masked_equals_compact_t63(plans):
    """192 x 96 x 16, E = 32 without member 0: the launch shape, the one level in flight and the LDS request are those of 32 members
    on 18 432 columns, the problem solved is that of 31, bit for bit the 31-member object's"""
    sp, g = plans(T63)
    assert (g.ix, g.il, g.kx) == (192, 96, 16)
    E, keep = 32, tuple(range(1, 32))
    x, obs, lt, ltc, xc = lm.pair(sp, g, E, keep, lambda g, xc: lk.concat(lk.clustered_obs(g, xc, n=300), lk.sparse_obs(g, xc)), 0.1)
    lm.same_as_compact(lk.run(lt, x, lm.flags(E, keep)), lk.run(ltc, xc), E, keep, T63)
    lt.close(); ltc.close()


def test_weight_stride_t63(plans):
    """192 x 96 x 16: `weight_stride`"""
    sp, g = plans(T63)
    weight_stride(sp, g)


def test_masked_against_restatement_t63(plans):
    """192 x 96 x 16: `masked_against_restatement`"""
    sp, g = plans(T63)
    masked_against_restatement("T63 L16 ", sp, g)


def test_unused_member_reaches_nothing_t63(plans):
    """192 x 96 x 16, member 3 of 8 not in use: `unused_member_reaches_nothing`"""
    sp, g = plans(T63)
    unused_member_reaches_nothing(sp, g, 3)
