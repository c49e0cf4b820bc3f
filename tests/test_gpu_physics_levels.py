"""GPU: the column physics at every level-count class of its kernels (tests/physlevels.py: 6, 9, 12, 15 levels at T30).

Every column kernel is built as <8> and <16> (csrc/spdy_columns.hpp launch_columns) and unrolled over KMAX with run-time k < kx
predicates; the other physics tests run them at 5, 7, 8 and 16 levels only, so <16> never meets an unused level there and <8>
never meets 6, the first count at which the convection diagnosis' loop do k = kx-3, 3, -1 runs.  Here: each kernel alone against
the flang-built reference's sample (tests/golden/ref_physlevels.npz) and against the restatement in every column; guard bands
round every output, tendency and the radiation state of the chain call; the one-launch chain against the five calls bit for bit;
batch composition; spdy_physics_dev from spectra; three whole steps with the physics, plain and captured; SPPT; the ensemble
physics call; and the constructed threshold columns in <16>.  Every tolerance is conftest.TOL; integers are identical.

Measured on MI355X, worst error against the restatement over every column (raw lines: profiles/r12_physics_level_counts_errors.txt):
each kernel alone 1.1e-14 (radiation tt_rsw, 15 levels); from spectra 3.0e-14 (6 levels) and 1.3e-13 (12 levels, rad.cloudc); three
steps with the whole physics 2.2e-15; the chain with SPPT 2.6e-15; the threshold columns 9.4e-14 per column (moist.precls).  A library
with KMAX written where kx is meant in the <16> form of three of the kernels passes every other physics test and fails 13 of these.

Every comparison with the restatement first asserts that no decision of any column is within MIN_MARGIN of its threshold and
that the state takes the branches (physstep.check_coverage); no column is dropped or masked."""
import os

import numpy as np
import pytest

import ensemblestep as es
import guards
import modelstep
import moist
import physlevels as pl
import physstep
import radiation
import sppt
import support
import surface
import synth
import thresholds as th
from conftest import GOLDEN, TOL
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from modelstep import PROG

pytestmark = pytest.mark.gpu

ZON = physstep.ZON
MOIST_FLOATS = ("ttend", "qtend", "precnv", "precls", "cbmf", "qsat", "rh", "se")
IL, IX, NCOL = pl.IL, pl.IX, pl.IL * pl.IX


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_physlevels.npz"))


def _tag(kx):
    return "t30k%d" % kx


def _levels_plan(kx, max_batch=64):
    """(plan, its half levels): what the helpers of the other physics tests take for a count outside support.PHYSICS_TAGS"""
    return pl.plan(kx, max_batch), pl.hsg(kx)


def _err(errs, key, got, want, per_column=False):
    """array-norm error (and the worst per-column one) of a float output into errs, asserted within TOL"""
    e = synth.relerr(np.asarray(got), np.asarray(want))
    errs[key] = max(errs.get(key, 0.0), e)
    assert e <= TOL, (key, "array norm", e)
    if per_column:
        ec = float(guards.column_err(got, want).max())
        assert ec <= TOL, (key, "per column", ec)


def _report(label, errs):
    top = sorted(errs.items(), key=lambda kv: -kv[1])
    print("\n[physics levels: %s] %d arrays, worst: %s" % (label, len(errs), ", ".join("%s %.1e" % kv for kv in top[:4])))


# ------------------------------------------------------------------------------------------------------ each kernel alone
@pytest.mark.parametrize("kx", pl.COUNTS)
def test_moist_columns(kx, ref):
    """spdy_moist_columns_dev with every optional output: the stored sample against the reference, every column against the
    restatement in the array norm and per column (guards.column_err, as tests/test_gpu_moist.py); at 6 levels some column convects
    with its top at level 3, the loop's single iteration; at 9, 12, 15 every iptop in 2 .. kx+1 occurs on the device."""
    tag, tab = _tag(kx), pl.tables(kx)
    ins = moist.grid_inputs(tab, (1, IL, IX), int(ref["moist_%s_seed" % tag]))
    sub = ref["moist_%s_sub" % tag]
    want = moist.block(tab, *ins)
    assert float(want["margin"].min()) >= moist.MIN_MARGIN
    assert 0 < want["branch"]["no_conv"] < NCOL and want["branch"]["lsc_interior"] > 0 and want["branch"]["secondary_flux"] > 0
    sp = pl.plan(kx)
    r = sp.moist_columns(*ins)
    sp.close()
    errs = {}
    for n in ("iptop", "icnv"):
        assert np.array_equal(r[n].reshape(-1)[sub], ref["moist_%s_%s" % (tag, n)]), n
        assert np.array_equal(r[n].reshape(-1), want[n].reshape(-1)), n
    for n in MOIST_FLOATS:
        g, w = r[n].reshape(-1, NCOL), want[n].reshape(-1, NCOL)
        _err(errs, n + " vs reference", g[:, sub].squeeze(), ref["moist_%s_%s" % (tag, n)])
        _err(errs, n, g, w, per_column=n not in ("ttend", "qtend"))     # sums of large terms: by the array norm (test_gpu_moist.py)
    itop = kx - r["icnv"].reshape(-1)
    if kx == 6:
        assert set(np.unique(r["icnv"]).tolist()) == {-1, 3} and int(np.sum(itop == 3)) > 0.1 * NCOL
    else:
        assert set(np.unique(r["iptop"]).tolist()) == set(range(2, kx + 2))
        assert set(np.unique(itop[itop <= kx]).tolist()) == set(range(3, kx - 2))
    _report("moist_columns %d levels" % kx, errs)


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_radiation_columns(kx, ref):
    """spdy_radiation_down_dev / _up_dev with every optional output at both dates, a shortwave call and then a call without
    shortwave on the held state: the stored sample against the reference, every column of both calls against the restatement;
    icltop identical, and every value of it that the restatement produces occurs on the device."""
    tag, tab = _tag(kx), pl.tables(kx)
    zonal = lambda d: radiation.zonal_columns({n: ref["rad_%s_d%d_%s" % (tag, d, n)] for n in ZON}, 1, IL, IX)
    c = radiation.columns(tab, NCOL, int(ref["rad_%s_seed" % tag]), zonal(0))
    sub = ref["rad_%s_sub" % tag]
    G = lambda n: radiation.grids(c[n], 1, IL, IX)[0]
    sp = pl.plan(kx)
    errs = {}
    for di, ty in enumerate(radiation.DATES):
        sp.radiation_set_date(ty)
        for n in ZON:
            assert np.array_equal(sp.table(n), ref["rad_%s_d%d_%s" % (tag, di, n)]), n
        q1, q2 = radiation.two_steps(tab, c, zonal(di))
        # the columns were drawn clear of ties at the first date; the decisions of the second date's shortwave call as well
        down = radiation.down(tab, c["tg"], c["qg"], c["phig"], c["pslg"], c["rh"], c["precnv"], c["precls"], c["iptop"], c["fmask"],
                              c["albsfc"], zonal(di), True, {})
        assert float(down["margin"].min()) >= radiation.MIN_MARGIN, di
        r1 = sp.radiation_columns(G("tg"), G("qg"), G("phig"), G("pslg"), G("rh"), G("precnv"), G("precls"), G("iptop"),
                                  G("fmask"), G("albsfc"), G("ts"), G("fsfcu"), G("ttend_m"), compute_sw=True)
        r2 = sp.radiation_columns(G("tg2"), G("qg"), G("phig"), G("pslg"), None, None, None, None, None, None, G("ts2"),
                                  G("fsfcu2"), G("ttend2"), compute_sw=False, state=r1["state"])
        for step, r, q, names in (("s1", r1, q1, radiation.SW_OUT), ("s2", r2, q2, radiation.NOSW_OUT)):
            for n in names:
                got = radiation.cols(r[n][None])
                _err(errs, "%s %s vs reference" % (step, n), got[..., sub], ref["rad_%s_d%d_%s_%s" % (tag, di, step, n)])
                _err(errs, "%s %s" % (step, n), got, q[n])
        icl = radiation.cols(r1["icltop"][None])
        assert np.array_equal(icl[sub], ref["rad_%s_d%d_s1_icltop" % (tag, di)]) and np.array_equal(icl, q1["icltop"])
        tops = set(np.unique(icl).tolist())
        assert tops == set(np.unique(q1["icltop"]).tolist()) and set(range(2, kx - 1)) | {kx + 1} <= tops, tops
    sp.close()
    _report("radiation_down / _up %d levels" % kx, errs)


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_surface_and_pbl_columns(kx, ref):
    """spdy_surface_fluxes_dev and spdy_pbl_dev with every optional output: the stored sample against the reference, every
    column against the restatement; utend and vtend above level kx untouched."""
    tag = _tag(kx)
    sp, tab, c, zon, sqcoa = surface.case(tag, int(ref["sfc_%s_seed" % tag]), plan=_levels_plan(kx))
    sub = ref["sfc_%s_sub" % tag]
    sp.surface_set_orography(c["phis0"].reshape(IL, IX))
    r, _ = surface.chain(tab, c, zon, sqcoa)
    physstep.check_coverage(r, tag)
    G = lambda a: radiation.grids(a, 1, IL, IX)[0]
    bnd = {n: G(c[n]) for n in surface.BOUNDARY}
    errs = {}
    s = sp.surface_columns(G(c["ug"]), G(c["vg"]), G(c["tg"]), G(c["qg"]), G(c["phig"]), G(c["pslg"]), G(r["ssrd"]),
                           G(r["down"]["slrd"]), bnd)
    for n in surface.SFC_OUT:
        got = s[n].reshape(-1, NCOL).squeeze()
        _err(errs, n + " vs reference", got[..., sub], ref["sfc_%s_%s" % (tag, n)])
        _err(errs, n, got, r["sfc"][n])
    assert np.array_equal(s["fsfcu"].reshape(-1), s["slru"][2].reshape(-1))
    assert np.array_equal(s["flux3"], np.stack([s[n][2] for n in surface.FLUX3]))
    m, up = r["moist"], r["up"]
    p = sp.pbl_columns(G(c["qg"]), G(c["phig"]), G(c["pslg"]), G(m["se"]), G(m["rh"]), G(m["qsat"]), G(m["icnv"]),
                       np.stack([G(f) for f in r["flux3"]]), G(c["utend"]), G(c["vtend"]), G(up["ttend"]), G(m["qtend"]))
    for n in surface.PBL_OUT:
        got, want = p[n].reshape(-1, NCOL).squeeze(), r["pbl"][n]
        if n in ("utend", "vtend"):
            assert np.array_equal(got[:kx - 1], np.asarray(c[n])[:kx - 1]), n     # untouched above level kx
            got, want = got[kx - 1], want[kx - 1]
        _err(errs, n + " vs reference", got[..., sub], ref["sfc_%s_%s" % (tag, n)])
        _err(errs, n, got, want)
    sp.close()
    _report("surface_fluxes, pbl %d levels" % kx, errs)


# ----------------------------------------------------------------------------------------- nothing outside kx levels
def _guarded_like(torch, tensors, pad):
    """tensors (float64 [1, k, il, ix] / [1, il, ix] / flat multiples of a field, or int32 [1, il, ix]) re-made as views into
    one guards.Guarded allocation with `pad` sentinel fields in every gap; an int32 field is the first half of a float64 one"""
    counts = [max(1, (t.numel() * t.element_size()) // (NCOL * 8)) for t in tensors]
    g = guards.Guarded(torch, (IL, IX), counts, pad=pad)
    views = []
    for t, o in zip(tensors, g.outs):
        if t.dtype == torch.int32:
            views.append(o.view(torch.int32).reshape(-1)[:t.numel()].view(t.shape))
        else:
            assert t.numel() == o.numel(), (t.shape, o.shape)
            views.append(o.view(t.shape))
    return g, views


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_nothing_written_outside_kx_levels(kx):
    """The chain call in both forms, a shortwave call and a call without shortwave, with the four in/out tendencies, every
    optional output and the radiation state inside guard bands of 16 - kx + 1 fields: one field more than the farthest store of
    an unused level of a KMAX = 16 kernel could reach.  The bands are unchanged, every output is written (none left NaN) and
    equals the one an ordinary allocation receives."""
    import torch
    sp, _, il, ix, d1, d2 = physstep.gridded(_tag(kx), 1, pl.CHAIN_SEED[kx], plan=_levels_plan(kx))
    sp.column_physics_workspace()
    plain = physstep.run_gridded(sp, 1, kx, il, ix, d1, d2, True)
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        S0 = torch.empty((sp.radiation_state_size(),), dtype=torch.float64, device="cuda")
        outs = [sp.column_outputs(1), sp.column_outputs(1)]
        flat = [physstep.flat_outs(o) for o in outs]
        names = [("state", S0)] + [("%s%d" % (n, i), d[n]) for i, d in ((1, d1), (2, d2)) for n in physstep.TEND]
        names += [("out%d.%s" % (i + 1, n), t) for i in range(2) for n, t in flat[i].items()]
        g, views = _guarded_like(torch, [t for _, t in names], 16 - kx + 1)
        V = dict(zip([n for n, _ in names], views))
        for i, d in ((1, d1), (2, d2)):
            for n in physstep.TEND:
                V["%s%d" % (n, i)].copy_(d[n])
        assert g.intact()
        for i, d, sw in ((1, d1, True), (2, d2, False)):
            out = {b: ({n: V["out%d.%s.%s" % (i, b, n)] for n in v} if isinstance(v, dict) else V["out%d.%s" % (i, b)])
                   for b, v in outs[i - 1].items()}
            if i == 2:                     # ssrd stays where the shortwave call put it (include/spdy.h)
                out["rad"]["ssrd"] = V["out1.rad.ssrd"]
            sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], V["state"],
                                  *[V["%s%d" % (n, i)] for n in physstep.TEND], out)
        torch.cuda.synchronize()
        assert g.intact(), (fused, [(names[min(b, len(names) - 1)][0], j) for b, j in g.hits()])
        for n, v in V.items():
            if n.startswith("out2.") and n[5:] in th.SW_ONLY:
                continue                   # written by shortwave calls only
            assert torch.equal(v, plain[n]), (fused, n)
    sp.close()


# ------------------------------------------------------------------------------------------ one launch = five calls
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("kx", pl.COUNTS)
def test_one_launch_equals_five_calls(kx, nb):
    """tests/test_gpu_physics_step.py::test_one_launch_equals_five_calls at the new counts: "physics_fused" 1 against 0, a
    shortwave call and then a call without shortwave on the held state; torch.equal on the tendencies, every output and the
    radiation state; with out = NULL the tendencies and the radiation state equal those of the all-outputs run."""
    import torch
    sp, _, il, ix, d1, d2 = physstep.gridded(_tag(kx), nb, 9800 + 10 * kx + nb, plan=_levels_plan(kx))
    sp.column_physics_workspace()
    runs = {}
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        for with_out in (True, False):
            runs[fused, with_out] = physstep.run_gridded(sp, nb, kx, il, ix, d1, d2, with_out)
    full = runs[0, True]
    assert len(full) > 60
    for n, v in full.items():
        assert torch.equal(runs[1, True][n], v), ("one launch, all outputs", n)
    for key in ((1, False), (0, False)):
        for n, v in runs[key].items():
            assert torch.equal(v, full[n]), (key, n)
    assert not torch.isnan(full["state"]).any()
    sp.close()


def test_batch_composition_at_12_levels():
    """A state's bits do not depend on nb or on its position in the batch: the chain with every output on three states at once
    against each state alone, both calls, the radiation state included."""
    import torch
    kx, nb = 12, 3
    sp, _, il, ix, d1, d2 = physstep.gridded(_tag(kx), nb, 9900 + kx, plan=_levels_plan(kx))
    sp.column_physics_workspace()
    full = physstep.run_gridded(sp, nb, kx, il, ix, d1, d2, True)
    size = sp.radiation_state_size()
    assert not torch.equal(full["ttend1"][0], full["ttend1"][1])
    for b in range(nb):
        one = physstep.run_gridded(sp, 1, kx, il, ix, *[{n: v[b:b + 1].contiguous() for n, v in d.items()} for d in (d1, d2)], True)
        for n, v in one.items():
            want = full[n][b * size:(b + 1) * size] if n.startswith("state") else full[n][b:b + 1]
            assert torch.equal(v, want), (b, n)
    sp.close()


# ------------------------------------------------------------------------------------------------------ from spectra
@pytest.mark.parametrize("kx", sorted(pl.CASE_SEEDS))
def test_physics_from_spectra(kx):
    """spdy_physics_dev against tests/levels.py's oracle transforms and the chain of restatements, a shortwave call and a call
    without shortwave, after check_coverage: tests/test_gpu_physics_step.py::test_physics_from_spectra's body."""
    name, worst = physstep.check_physics_from_spectra(_tag(kx), *physstep.plan_case(_tag(kx), None, pl.levels_case(kx)))
    assert worst <= TOL, (name, worst)


def test_step_with_whole_physics_at_12_levels():
    """Three consecutive 12-level steps with the whole physics against oracle_dynamics_step with the physics hook: vor, div, t, tr,
    ps and the PL operands within TOL in synth.relerr and wave_relerr after each step.  The step captured with and without
    shortwave and replayed for the three steps is bit-equal to the plain launches."""
    import torch
    kx = 12
    tag = _tag(kx)
    sp, o, case, _ = physstep.plan_case(tag, None, pl.levels_case(kx))
    dt = pl.DT
    sp.initialize_implicit(dt); o.tail_init(dt)
    sp.physics_workspace()
    sp.use_own_stream()
    plain_run = lambda D, W, P, sw: modelstep.step(sp, D, W, dt, physics=modelstep.whole_physics(P, sw))
    got, _, _, _ = modelstep.three_steps(sp, case, dt, plain_run)
    st, rs, rec, refs = case.st, {}, {}, []
    for step in range(3):                          # the reference: margins and coverage first, then the comparison
        st, out = oracle_dynamics_step(o, st, 2, dt, ROB, physics=case.hook(step == 0, rs, rec))
        physstep.check_coverage(rec, "%s step %d" % (tag, step + 1))
        refs.append((st, out))
    worst = 0.0
    for step, (st, out) in enumerate(refs):
        w = synth.relerr(got[step]["PL"].cpu().numpy(), out["PL"])
        for n in PROG:
            g = got[step][n].cpu().numpy()
            w = max(w, synth.relerr(g, st[n]), wave_relerr(g, st[n]))
        print("[physics levels: step %d with the whole physics %s vs oracle] worst %.1e" % (step + 1, tag, w))
        worst = max(worst, w)
    assert worst <= TOL, worst
    graphs = {}

    def captured_run(D, W, P, sw):
        if sw not in graphs:
            torch.cuda.synchronize()
            with sp.graph_capture() as g:
                plain_run(D, W, P, sw)
            graphs[sw] = g
        graphs[sw].launch()
    cap, _, _, _ = modelstep.three_steps(sp, case, dt, captured_run)
    for step in range(3):
        for n in got[step]:
            assert torch.equal(cap[step][n], got[step][n]), ("captured", step, n)
    for g in graphs.values():
        g.close()
    sp.close()


# -------------------------------------------------------------------------------------------------------------- SPPT
@pytest.mark.parametrize("kx", [6, 12])
def test_sppt_on_gridded_states(kx):
    """spdy_column_physics_sppt_dev on two gridded states with a taper that holds 0, fractions and 1 and a pattern that holds -1, 1
    and everything between: within TOL of the formula of physics.f90:212-221 on the chain of restatements, bit-equal to the
    formula on spdy_column_physics_dev's own result, and "physics_fused" 1 and 0 bit-equal; the radiation state is the one of the
    call without SPPT.  At 12 levels the first run of the SPPT kernel's <16> form with unused levels."""
    import torch
    nb, keep = 2, {}
    sp, _, il, ix, d, _ = physstep.gridded(_tag(kx), nb, 9950 + kx, plan=_levels_plan(kx), keep=keep)
    r, _ = surface.chain(keep["tab"], keep["c1"], keep["zon"], keep["sqcoa"])
    physstep.check_coverage(r, "%s sppt" % _tag(kx))
    mu = sppt.mu(kx)
    P = np.clip(1.5 * (2.0 * synth.splitmix64(9960 + kx, nb * kx * il * ix) - 1.0), -1.0, 1.0).reshape(nb, kx, il, ix)
    assert (P == 1.0).any() and (P == -1.0).any() and ((P > -1.0) & (P < 1.0)).mean() > 0.5
    dP = support.dev(P)
    sp.column_physics_sppt_workspace()
    nan_state = lambda: torch.full((nb * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    args = lambda T, S: (True, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], S, *T)
    T0 = [d[n].cpu().numpy() for n in physstep.TEND]
    T, S = [d[n].clone() for n in physstep.TEND], nan_state()
    sp.column_physics_dev(*args(T, S))
    torch.cuda.synchronize()
    own = [sppt.apply(np.moveaxis(t.cpu().numpy(), 1, 0), np.moveaxis(t0, 1, 0), np.moveaxis(P, 1, 0), mu) for t, t0 in zip(T, T0)]
    want = [sppt.apply(radiation.grids(r["pbl"][n], nb, il, ix).swapaxes(0, 1), np.moveaxis(t0, 1, 0), np.moveaxis(P, 1, 0), mu)
            for n, t0 in zip(physstep.TEND, T0)]
    errs = {}
    for fused in (1, 0):
        sp.set_option("physics_fused", fused)
        T2, S2 = [d[n].clone() for n in physstep.TEND], nan_state()
        sp.column_physics_sppt_dev(dP, mu, *args(T2, S2))
        torch.cuda.synchronize()
        for n, t, a, w in zip(physstep.TEND, T2, own, want):
            g = np.moveaxis(t.cpu().numpy(), 1, 0)
            assert np.array_equal(g, a), (fused, n)
            _err(errs, n, g, w)
        assert torch.equal(S2, S) and not torch.isnan(S2).any()
    assert all(not np.array_equal(a, np.moveaxis(t.cpu().numpy(), 1, 0)) for a, t in zip(own[2:], T[2:]))
    sp.close()
    _report("column_physics_sppt %d levels" % kx, errs)


# ---------------------------------------------------------------------------------------------------------- ensemble
def test_ensemble_physics_at_12_levels():
    """spdy_ens_physics_dev with E = 2 members of different states, boundary fields and radiation states, a shortwave call and a
    call without: each member's tendencies, optional outputs and radiation state bit-equal to spdy_physics_dev on its own."""
    import torch
    kx, E = 12, 2
    sp, o, hsg, seeds = pl.levels_case(kx, E * (4 * kx + 4))
    sts, bnds = es.physics_members(sp, o, E, hsg, seeds)
    il, ix = sp.il, sp.ix
    dev = [physstep.device_boundary(b, il, ix) for b in bnds]
    spec = [[support.dev(a) for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], o.geopotential(st["t"][0], st["phis"]),
                                      st["ps"][0])] for st in sts]
    assert not torch.equal(spec[0][2], spec[1][2])
    t0 = [[support.dev(synth.splitmix64(270 + 4 * e + i, kx * il * ix).reshape(kx, il, ix) * f) for i, f in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
          for e in range(E)]
    size = sp.radiation_state_size()
    nan_state = lambda n: torch.full((n * size,), float("nan"), dtype=torch.float64, device="cuda")
    sp.physics_workspace()
    sp.ens_physics_workspace(E)
    ebnd = {n: torch.cat([b[n] for b in dev]) for n in dev[0]}
    espec = [torch.stack([spec[e][i] for e in range(E)]) for i in range(6)]
    S, Se = [nan_state(1) for _ in range(E)], nan_state(E)
    ssrd, essrd = [None] * E, None
    for sw in (True, False):
        eT, eout = [torch.stack([t0[e][i] for e in range(E)]) for i in range(4)], sp.column_outputs(E)
        if sw:
            essrd = eout["rad"]["ssrd"]
        else:                              # ssrd stays where the shortwave call put it (include/spdy.h)
            eout["rad"]["ssrd"] = essrd
        sp.ens_physics_dev(E, sw, *espec, ebnd, ebnd["albsfc"], Se, *eT, eout)
        torch.cuda.synchronize()
        flat = physstep.flat_outs(eout)
        for e in range(E):
            T, out = [t.clone() for t in t0[e]], sp.column_outputs(1)
            if sw:
                ssrd[e] = out["rad"]["ssrd"]
            else:
                out["rad"]["ssrd"] = ssrd[e]
            sp.physics_dev(sw, *spec[e], dev[e], dev[e]["albsfc"], S[e], *T, out)
            torch.cuda.synchronize()
            for n, a, b in zip(physstep.TEND, eT, T):
                assert torch.equal(a[e], b), (sw, e, n)
            for n, t in physstep.flat_outs(out).items():
                assert torch.equal(flat[n][e:e + 1], t), (sw, e, n)
            assert torch.equal(Se[e * size:(e + 1) * size], S[e]) and not torch.isnan(S[e]).any(), (sw, e)
    sp.close()


# -------------------------------------------------------------------------------------------------------- thresholds
def test_threshold_columns_at_12_levels(ref):
    """tests/thresholds.py's constructed columns at 12 levels through the one-launch chain, the five-kernel chain and the five
    single entry points (tests/test_gpu_thresholds.py::test_threshold_columns_on_device's body): every class-(i) operator is
    pinned on its tie in the <16> kernels."""
    kx = pl.THRESHOLD_COUNT
    pre = "thr_%s_" % _tag(kx)
    stored = lambda step: {k[len(pre) + 3:]: ref[k] for k in ref.files if k.startswith("%sc%d_" % (pre, step))}
    th.check_threshold_columns(_tag(kx), pl.plan(kx, 4), pl.tables(kx), int(ref[pre + "seed"]), ref[pre + "sub"], stored)
