"""CPU: the column physics ON its thresholds (tests/thresholds.py) -- the inventory of decisions and its coverage by constructed
columns, the NumPy restatements against the flang-built reference on those columns (tests/golden/ref_thresholds.npz), the
per-column error of the reference side, the near-tie shares of the regime draws, and the date table over a year.

Measured, restatement against the reference on the constructed columns, both calls: array norm worst 4.0e-15 (t30, rad.tt_rsw),
2.0e-15 (t30k5); per-column norm (guards.column_err with thresholds.scales) worst 4.3e-14 (t30, rad.tt_rsw, a column with little
sunlight; every other output at most 4.6e-15, moist.precls), 2.9e-15 (t30k5, moist.precls): every output is below TOL / 10 = 1e-13
in every column, so the per-column bound of the GPU tests is the project's TOL.  For sfc.shf, sfc.hfluxn, rad.tt_rlw, pbl.tt_pbl and
ttend the operand scale exceeds the array's own max|ref| in most columns (thresholds.scales): for them the per-column norm adds the
exact zeros only and the array norm, asserted beside it, is the binding one."""
import os

import numpy as np
import pytest

import guards
import moist
import radiation
import support
import surface
import synth
import thresholds as th
from conftest import GOLDEN, TOL
from support import pkg  # noqa: F401

ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")
INT_OUT = ("moist.iptop", "moist.icnv", "rad.icltop")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_thresholds.npz"))


def case(tag, date=radiation.DATES[0]):
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    sp = support.plan(tag, device=-1)
    sp.radiation_set_date(date)
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    return tab, zon, sqcoa, il * ix


def stored(ref, tag, step):
    pre = "%s_c%d_" % (tag, step)
    return {k[len(pre):]: ref[k] for k in ref.files if k.startswith(pre)}


def at_sub(v, n, sub, kx):
    v = np.asarray(v)
    return v[kx - 1, sub] if n in ("utend", "vtend") else v[..., sub]


def test_inventory_is_complete_and_classed():
    ids = [r["id"] for r in th.INVENTORY]
    assert len(ids) == len(set(ids)) and len(ids) >= 60
    for r in th.INVENTORY:
        assert r["cls"] in ("i", "ii", "host") and r["ref"] and r["op"], r
        assert ":" in r["ref"] and r["ref"].split(":")[0].endswith(".f90") or "fband" in r["ref"], r
        if r["sides"]:
            assert r["cls"] in ("i", "host") and r["how"] and 0 in r["sides"], r
        if r["cls"] == "ii":
            assert not r["sides"], r
    # the files the inventory was read from
    files = {r["ref"].split(":")[0] for r in th.INVENTORY}
    assert {"convection.f90", "large_scale_condensation.f90", "humidity.f90", "shortwave_radiation.f90", "longwave_radiation.f90",
            "surface_fluxes.f90", "vertical_diffusion.f90", "physics.f90"} <= files
    # every job belongs to a class-(i) row and a side that row names; every such side has a job unless it is found, not built
    built = {(id, side) for id, side, _, _ in th.jobs(moist.tables(moist.HSG[8]))}
    named = {(r["id"], s) for r in th.CLASS_I for s in r["sides"]}
    assert built <= named
    assert named - built == {("cnv.itop_nlp", 0), ("lsc.itop_nl1", 0), ("lsc.itop_nlp", 0), ("sw.icltop_le", 0), ("sw.fsol0", 0),
                             ("sfc.evap0", 0)}
    # the rows whose tie pins the kernel's operator are marked; all of them can be built on the tie
    assert {r["id"] for r in th.INVENTORY if r["observable"]} == set(th.OBSERVABLE) <= {r["id"] for r in th.CLASS_I}


@pytest.mark.parametrize("tag", th.TAGS)
def test_every_exact_threshold_is_hit(tag, pkg, ref):
    """Every class-(i) row is hit on the tie and on every neighbour it names, by a stored column; the regeneration is pinned; no
    NEAR tie is left in any column of either call, while the default margin rule would have removed the constructed ones."""
    tab, zon, sqcoa, ncol = case(tag)
    c, sub, r1, r2 = th.build(tab, ncol, int(ref[tag + "_seed"]), zon, sqcoa)
    assert np.array_equal(sub, ref[tag + "_sub"])
    for n, dg in zip(ref[tag + "_in_names"], ref[tag + "_in_digest"]):
        assert synth.digest(np.asarray(c[str(n)], np.float64)) == str(dg), n
    H = th.hits(tab, c, r1, zon)
    for row in th.CLASS_I:
        for side in row["sides"]:
            assert H[row["id"], side][sub].any(), (row["id"], side)
    assert float(min(r1["margin"].min(), r2["margin"].min())) >= th.MIN_MARGIN
    plain, _ = surface.chain(tab, c, zon, sqcoa)          # the default rule: exact ties and their neighbours count as margin 0
    assert int(np.sum(plain["margin"][sub] < th.MIN_MARGIN)) >= 40
    assert float(plain["margin"].min()) == 0.0


@pytest.mark.parametrize("tag", th.TAGS)
def test_restatement_matches_reference_on_thresholds(tag, pkg, ref):
    """The restatements on the constructed columns, both calls: integers identical, floats within TOL in the array norm the
    existing restatement tests use, and per column by the column's own scale (printed; the bound of the GPU tests comes from it)."""
    tab, zon, sqcoa, ncol = case(tag)
    kx = tab["kx"]
    c, sub, r1, r2 = th.build(tab, ncol, int(ref[tag + "_seed"]), zon, sqcoa)
    assert np.array_equal(surface.forog(c["phis0"])[sub], ref[tag + "_forog"])
    worst, worst_col = ("", 0.0), ("", 0.0)
    for step, cc, r in ((1, c, r1), (2, th.second(c), r2)):
        mine, want = th.flat(r, kx), stored(ref, tag, step)
        assert len(want) >= (39 if step == 1 else 24)
        sc = th.scales(tab, cc, r)
        for n, w in want.items():
            g = at_sub(mine[n], n, sub, kx)
            if n in INT_OUT:
                assert np.array_equal(g, w), (step, n)
                continue
            e = synth.relerr(g, w)
            assert e <= TOL, (step, n, e)
            ec = float(guards.column_err(g, w, sc[n][..., sub] if n in sc else None).max())
            worst = max(worst, (n, e), key=lambda x: x[1])
            worst_col = max(worst_col, (n, ec), key=lambda x: x[1])
            assert ec <= TOL / 10, (step, n, ec)         # the reference side alone stays a factor 10 below TOL in every column
    print("\n[threshold columns %s, restatement vs reference] array norm worst %s %.1e, per column worst %s %.1e"
          % ((tag,) + worst + worst_col))


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_regime_near_tie_shares(tag, pkg):
    """Each regime's state has at most 1 % of its columns near a tie (they are left out, not drawn again), no branch loses all
    its columns, and the regime is what its name says."""
    kx = support.grid(tag)[2]
    for name, (seed, tyear) in th.REGIMES.items():
        tab, zon, sqcoa, ncol = case(tag, tyear)
        c = th.regime(name, tab, ncol)
        r, keep = th.regime_run(tab, c, zon, sqcoa)
        share = th.check_regime(name, r, keep)
        print("[regime %s %s] %.3f %% of %d columns left out" % (tag, name, 100 * share, ncol))
        psa = np.exp(c["pslg"])
        if name == "cold":
            assert c["tg"].min() >= 180.0 and c["tg"].max() <= 230.0 and r["down"]["branch_cols"]["fband_low"].mean() > 0.9
        if name == "hot_saturated":
            assert r["moist"]["rh"].min() >= 1.0 - 1e-12 and r["moist"]["rh"].max() <= 1.1 + 1e-12
        if name == "dry":
            assert not c["qg"].any() and not r["moist"]["precls"].any() and not r["moist"]["precnv"].any()
        if name == "high_orography":
            assert psa.max() < moist.PSMIN and psa.min() >= 0.45 and r["moist"]["branch"]["psmin_cut"] == ncol
        if name == "calm":
            assert np.abs(c["ug"]).max() < 0.1 and np.abs(c["vg"]).max() < 0.1 and np.mean(c["ug"] == 0.0) > 0.2
        if name == "all_sea":
            assert not c["fmask"].any() and c["sst"].min() >= 271.4
        if name == "all_land":
            assert c["fmask"].all() and c["snowc"].all() and set(np.unique(c["soilw"])) == {0.0, 1.0}
        assert all(np.isfinite(v).all() for v in th.flat(r, kx).values()), name


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_date_table_over_a_year(tag, pkg, ref):
    """fsol, ozone, ozupp, zenit, stratz of spdy_radiation_set_date bit for bit equal to the flang-built reference at every stored
    tyear (0, the solstices and equinoxes, the values closest below 1, the two dates in use, every 12th of the year), and the
    restatement radiation.zonal likewise."""
    ty = ref[tag + "_tyear"]
    assert ty.size >= 20 and ty[0] == 0.0 and ty[-1] == np.nextafter(1.0, 0.0) and set(radiation.DATES) <= set(ty.tolist())
    assert {th.SOLSTICE_JUN, th.SOLSTICE_DEC, th.EQUINOX_MAR} <= set(ty.tolist())
    sp = support.plan(tag, device=-1)
    got, mine = [], []
    for t in ty:
        sp.radiation_set_date(float(t))
        got.append([np.array(sp.table(n)) for n in ZON])
        z = radiation.zonal(sp.table("sia_half"), sp.table("coa_half"), float(t))
        mine.append([z[n] for n in ZON])
    got, mine = np.moveaxis(np.array(got), 0, 1), np.moveaxis(np.array(mine), 0, 1)        # [5, dates, il]
    assert synth.digest(got) == str(ref[tag + "_year_digest"])
    assert synth.digest(mine) == str(ref[tag + "_year_digest"])
    whole = ref[(tag if tag == "t63k16" else "t30") + "_year"]
    for i, n in enumerate(ZON):
        assert np.array_equal(got[i], whole[i]), n
    assert (whole[0] == 0.0).any() and (whole[4] > 0.0).any()                           # polar night is in the table
