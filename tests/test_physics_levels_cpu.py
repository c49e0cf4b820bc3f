"""CPU: the column physics at the level counts of tests/physlevels.py (6, 9, 12, 15 at T30, on tests/levels.py's half levels) --
the plan's host tables bit-equal to the flang-built reference's, the NumPy restatements against the reference at the tolerances
tests/test_moist_cpu.py, test_radiation_cpu.py, test_surface_cpu.py and test_thresholds_cpu.py hold the other variants to, and the
coverage of the fixture tests/golden/ref_physlevels.npz (tests/golden/make_golden_physlevels.py): every branch the state takes is
in the stored sample, every convection top 3 .. kx-3 and every cloud top occurs, and at 12 levels every class-(i) threshold of
tests/thresholds.py is hit by a stored column on every side it names.

Measured, restatement against the reference, worst over the four counts: moist 2.1e-15, radiation 7.5e-15, surface 1.8e-15,
threshold columns at 12 levels 5.0e-15 in the array norm (moist.cbmf) and 7.2e-15 per column (moist.precnv)."""
import os

import numpy as np
import pytest

import guards
import moist
import physlevels as pl
import physstep
import radiation
import surface
import synth
import thresholds as th
from conftest import GOLDEN, TOL
from support import pkg  # noqa: F401

ZON = physstep.ZON
MOIST_TABLES = ("sigl", "sigh", "grdsig", "grdscp", "wvi", "entr")
SFC_TABLES = ("vd_scalars", "vd_rsig", "vd_rsig1", "vd_drh0", "vd_fvdiq2")
MOIST_IN = ("tg", "qg", "phig", "pslg", "ttend", "qtend")
MOIST_FLOATS = ("ttend", "qtend", "precnv", "precls", "cbmf", "qsat", "rh", "se")
RAD_IN = ("tg", "qg", "pslg", "fmask", "albsfc", "ts", "fsfcu", "tg2", "ts2", "fsfcu2")
SFC_IN = ("ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend", "qtend", "albsfc", "phis0") + surface.BOUNDARY
SFC_OUT = surface.SFC_3 + ("hfluxn",) + surface.SFC_2D
INT_OUT = ("moist.iptop", "moist.icnv", "rad.icltop")
NCOL = pl.IL * pl.IX


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_physlevels.npz"))


def host_case(kx, date=0):
    """(host plan with the date set, tables, zonal fields and sqrt(coa) per column)"""
    sp = pl.plan(kx, device=-1)
    sp.radiation_set_date(radiation.DATES[date])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, pl.IL, pl.IX)
    return sp, pl.tables(kx), zon, surface.sqcoa_columns(sp.table("coa_half"), 1, pl.IL, pl.IX)


def sample(a, sub):
    return np.asarray(a).reshape(-1, NCOL)[:, sub].squeeze()


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_tables_bit_equal(kx, pkg, ref):
    """The level tables of the moist block and the vertical diffusion and, after spdy_radiation_set_date, the zonal forcing of
    both dates: the plan's and the restatements' bit-equal to the reference's."""
    tag = "t30k%d" % kx
    sp, tab = pl.plan(kx, device=-1), pl.tables(kx)
    assert np.array_equal(sp.table("hsg"), pl.hsg(kx))
    for n in MOIST_TABLES:
        assert np.array_equal(sp.table(n), ref["moist_%s_tab_%s" % (tag, n)]), n
        assert np.array_equal(np.ravel(tab[n]), ref["moist_%s_tab_%s" % (tag, n)]), n      # wvi [2, kx] = column-major wvi(kx,2)
    for n in SFC_TABLES:
        assert np.array_equal(sp.table(n), ref["sfc_%s_tab_%s" % (tag, n)]), n
        assert np.array_equal(surface.vdiff_tables(tab)[n], ref["sfc_%s_tab_%s" % (tag, n)]), n
    for di, ty in enumerate(radiation.DATES):
        sp.radiation_set_date(ty)
        z = radiation.zonal(sp.table("sia_half"), sp.table("coa_half"), ty)
        for n in ZON:
            assert np.array_equal(sp.table(n), ref["rad_%s_d%d_%s" % (tag, di, n)]), (n, di)
            assert np.array_equal(z[n], ref["rad_%s_d%d_%s" % (tag, di, n)]), (n, di)


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_moist_restatement_matches_reference(kx, ref):
    """tests/moist.py against the reference at 1e-13 (tests/test_moist_cpu.py's bound), integers identical; every branch in the
    sample; every convection top level 3 .. kx-3 occurs -- at 6 levels the single one, 3."""
    tag = "t30k%d" % kx
    tab = pl.tables(kx)
    ins = moist.grid_inputs(tab, (1, pl.IL, pl.IX), int(ref["moist_%s_seed" % tag]))
    sub, insub = ref["moist_%s_sub" % tag], ref["moist_%s_insub" % tag]
    for n, a in zip(MOIST_IN, ins):
        assert np.array_equal(sample(a[0], insub), ref["moist_%s_in_%s" % (tag, n)]), n
    r = moist.block(tab, *ins)
    assert float(r["margin"].min()) == float(ref["moist_%s_min_margin" % tag]) >= moist.MIN_MARGIN
    counts = dict(zip([str(x) for x in ref["moist_%s_branch_names" % tag]], ref["moist_%s_branch_counts" % tag].tolist()))
    assert counts == r["branch"] and all(v >= 0.01 * NCOL for v in counts.values()), counts
    for name, mask in r["branch_cols"].items():
        assert mask[sub].any(), name
    tops = kx - r["icnv"].reshape(-1)[r["icnv"].reshape(-1) > 0]
    assert set(np.unique(tops).tolist()) == set(range(3, kx - 2)), np.unique(tops)
    assert set(np.unique(r["iptop"]).tolist()) == set(range(2, kx + 2))
    worst = 0.0
    for n in ("iptop", "icnv"):
        assert np.array_equal(sample(r[n], sub), ref["moist_%s_%s" % (tag, n)]), n
    for n in MOIST_FLOATS:
        e = synth.relerr(sample(r[n], sub), ref["moist_%s_%s" % (tag, n)])
        worst = max(worst, e)
        assert e <= 1e-13, (n, e)
    print("\n[moist restatement %s vs reference] worst %.1e" % (tag, worst))


@pytest.mark.parametrize("di", [0, 1])
@pytest.mark.parametrize("kx", pl.COUNTS)
def test_radiation_restatement_matches_reference(kx, di, ref):
    """tests/radiation.py against the reference within TOL at both dates, a shortwave step and a step without shortwave on the held
    state; icltop identical; every branch in the sample; every cloud top the state takes is in the sample too."""
    tag = "t30k%d" % kx
    tab = pl.tables(kx)
    zonal = lambda d: radiation.zonal_columns({n: ref["rad_%s_d%d_%s" % (tag, d, n)] for n in ZON}, 1, pl.IL, pl.IX)
    c = radiation.columns(tab, NCOL, int(ref["rad_%s_seed" % tag]), zonal(0))
    sub, insub = ref["rad_%s_sub" % tag], ref["rad_%s_insub" % tag]
    for n in RAD_IN:
        assert np.array_equal(sample(c[n], insub), ref["rad_%s_in_%s" % (tag, n)]), n
    r1, r2 = radiation.two_steps(tab, c, zonal(di))
    for name, mask in r1["branch_cols"].items():
        assert mask[sub].any() or not mask.any(), name
    tops = set(np.unique(r1["icltop"]).tolist())
    assert set(range(2, kx - 1)) | {kx + 1} <= tops, tops           # every interior level, and "no cloud"
    worst = 0.0
    for step, r, names in (("s1", r1, radiation.SW_OUT + ("icltop",)), ("s2", r2, radiation.NOSW_OUT)):
        for n in names:
            g, want = np.asarray(r[n])[..., sub], ref["rad_%s_d%d_%s_%s" % (tag, di, step, n)]
            if n == "icltop":
                assert np.array_equal(g, want)
                continue
            e = synth.relerr(g, want)
            worst = max(worst, e)
            assert e <= TOL, (step, n, e)
    print("\n[radiation restatement %s date %d vs reference] worst %.1e" % (tag, di, worst))


@pytest.mark.parametrize("kx", pl.COUNTS)
def test_surface_restatement_matches_reference(kx, pkg, ref):
    """tests/surface.py's chain against the reference's chain within TOL, forog bit-equal, the branch counts and the minimum
    margin as stored, every surface and boundary-layer branch in at least 1 % of the columns and in the sample."""
    tag = "t30k%d" % kx
    sp, tab, zon, sqcoa = host_case(kx)
    c = surface.columns(tab, NCOL, int(ref["sfc_%s_seed" % tag]), zon, sqcoa)
    sub, insub = ref["sfc_%s_sub" % tag], ref["sfc_%s_insub" % tag]
    for n in SFC_IN:
        assert np.array_equal(sample(c[n], insub), ref["sfc_%s_in_%s" % (tag, n)]), n
    sp.surface_set_orography(c["phis0"].reshape(pl.IL, pl.IX))
    assert np.array_equal(sp.table("forog")[sub], ref["sfc_%s_forog" % tag])
    assert np.array_equal(surface.forog(c["phis0"])[sub], ref["sfc_%s_forog" % tag])
    r, _ = surface.chain(tab, c, zon, sqcoa)
    assert float(r["margin"].min()) == float(ref["sfc_%s_min_margin" % tag]) >= surface.MIN_MARGIN
    br = surface.branch_cols(r)
    names = [str(x) for x in ref["sfc_%s_branch_names" % tag]][:-1]
    assert set(names) == set(surface.SFC_BRANCHES + surface.PBL_BRANCHES)
    assert [int(br[n].sum()) for n in names] == ref["sfc_%s_branch_counts" % tag].tolist()[:-1]
    for name, mask in br.items():
        assert mask.sum() >= 0.01 * NCOL and mask[sub].any(), name
    p = r["pbl"]
    out = {n: r["sfc"][n] for n in SFC_OUT}
    out.update(ssrd=r["ssrd"], slrd=r["down"]["slrd"], ut_pbl=p["ut_pbl"], vt_pbl=p["vt_pbl"], tt_pbl=p["tt_pbl"], qt_pbl=p["qt_pbl"],
               utend=p["utend"][kx - 1], vtend=p["vtend"][kx - 1], ttend=p["ttend"], qtend=p["qtend"])
    worst = 0.0
    for n, v in out.items():
        e = synth.relerr(np.asarray(v)[..., sub], ref["sfc_%s_%s" % (tag, n)])
        worst = max(worst, e)
        assert e <= TOL, (n, e)
    print("\n[surface restatement %s vs reference] worst %.1e" % (tag, worst))


def test_thresholds_at_12_levels(pkg, ref):
    """thresholds.build at 12 levels: the regeneration is pinned, every class-(i) row is hit on every side it names by a stored
    column, no near tie is left, and the restatement equals the reference on those columns in both calls -- integers identical,
    floats within TOL in the array norm and TOL / 10 per column (tests/test_thresholds_cpu.py's bounds)."""
    kx = pl.THRESHOLD_COUNT
    tag, pre = "t30k%d" % kx, "thr_t30k%d_" % kx
    _, tab, zon, sqcoa = host_case(kx)
    assert int(ref[pre + "seed"]) == pl.THRESHOLD_SEED
    c, sub, r1, r2 = th.build(tab, NCOL, pl.THRESHOLD_SEED, zon, sqcoa)
    assert np.array_equal(sub, ref[pre + "sub"])
    for n, dg in zip(ref[pre + "in_names"], ref[pre + "in_digest"]):
        assert synth.digest(np.asarray(c[str(n)], np.float64)) == str(dg), n
    H = th.hits(tab, c, r1, zon)
    for row in th.CLASS_I:
        for side in row["sides"]:
            assert H[row["id"], side][sub].any(), (row["id"], side)
    assert float(min(r1["margin"].min(), r2["margin"].min())) >= th.MIN_MARGIN
    assert np.array_equal(surface.forog(c["phis0"])[sub], ref[pre + "forog"])
    worst, worst_col = ("", 0.0), ("", 0.0)
    for step, cc, r in ((1, c, r1), (2, th.second(c), r2)):
        head = "%sc%d_" % (pre, step)
        want = {k[len(head):]: ref[k] for k in ref.files if k.startswith(head)}
        assert len(want) >= (39 if step == 1 else 24)
        mine, sc = th.flat(r, kx), th.scales(tab, cc, r)
        for n, w in want.items():
            v = np.asarray(mine[n])
            g = v[kx - 1, sub] if n in ("utend", "vtend") else v[..., sub]
            if n in INT_OUT:
                assert np.array_equal(g, w), (step, n)
                continue
            e = synth.relerr(g, w)
            ec = float(guards.column_err(g, w, sc[n][..., sub] if n in sc else None).max())
            worst = max(worst, (n, e), key=lambda x: x[1])
            worst_col = max(worst_col, (n, ec), key=lambda x: x[1])
            assert e <= TOL, (step, n, e)
            assert ec <= TOL / 10, (step, n, ec)
    print("\n[threshold columns %s, restatement vs reference] array norm worst %s %.1e, per column worst %s %.1e"
          % ((tag,) + worst + worst_col))
