"""CPU: surface fluxes and vertical diffusion (physics.f90:169-170, :193-205) -- the plan's host tables against the flang-built
reference, the fixture's coverage, the NumPy restatement (tests/surface.py) against the reference, and the C ABI's argument checks
on a host-only plan.

Measured, restatement against the reference: worst relative error 3.9e-15 over the four variants (1.9e-15 at T30 L8) (TOL is 1e-12)."""
import ctypes
import os

import numpy as np
import pytest

import moist
import radiation
import support
import surface
import synth
from conftest import GOLDEN, TOL
from support import pkg  # noqa: F401

ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")
TABLES = ("vd_scalars", "vd_rsig", "vd_rsig1", "vd_drh0", "vd_fvdiq2")
INPUTS = ("ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend", "qtend", "albsfc", "phis0") + surface.BOUNDARY
SFC_OUT = surface.SFC_3 + ("hfluxn",) + surface.SFC_2D


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_surface.npz"))


def reference_case(tag, ref):
    """(tables, columns regenerated from the seed, column sample, zonal fields and sqrt(coa) per column, the restated chain) -- the
    regeneration checked against the stored inputs."""
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    sp = support.plan(tag, device=-1)
    sp.radiation_set_date(radiation.DATES[0])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    c = surface.columns(tab, il * ix, int(ref[tag + "_seed"]), zon, sqcoa)
    insub = ref[tag + "_insub"]
    for n in INPUTS:
        assert np.array_equal(np.asarray(c[n]).reshape(-1, il * ix)[:, insub].squeeze(), ref["%s_in_%s" % (tag, n)]), n
    r, _ = surface.chain(tab, c, zon, sqcoa)
    return tab, c, ref[tag + "_sub"], zon, sqcoa, r


def restated(r, kx):
    """the chain's outputs under the fixture's names"""
    out = {n: r["sfc"][n] for n in SFC_OUT}
    out.update(ssrd=r["ssrd"], slrd=r["down"]["slrd"], ut_pbl=r["pbl"]["ut_pbl"], vt_pbl=r["pbl"]["vt_pbl"], tt_pbl=r["pbl"]["tt_pbl"],
               qt_pbl=r["pbl"]["qt_pbl"], utend=r["pbl"]["utend"][kx - 1], vtend=r["pbl"]["vtend"][kx - 1], ttend=r["pbl"]["ttend"],
               qtend=r["pbl"]["qtend"])
    return out


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_surface_tables_bit_equal(tag, pkg, ref):
    """The vertical-diffusion scalars and rows and, after spdy_surface_set_orography, forog: bit for bit."""
    ix, il, kx = support.grid(tag)
    sp = support.plan(tag, device=-1)
    tab = moist.tables(moist.HSG[kx])
    for n in TABLES:
        assert np.array_equal(sp.table(n), ref["%s_tab_%s" % (tag, n)]), n
        assert np.array_equal(surface.vdiff_tables(tab)[n], ref["%s_tab_%s" % (tag, n)]), n
    assert sp.table("forog").size == 0 and sp.table("phis0").size == 0          # no orography yet
    _, c, sub, _, _, _ = reference_case(tag, ref)
    sp.surface_set_orography(c["phis0"].reshape(il, ix))
    assert np.array_equal(sp.table("phis0"), c["phis0"])
    assert np.array_equal(sp.table("forog")[sub], ref[tag + "_forog"])
    assert np.array_equal(surface.forog(c["phis0"])[sub], ref[tag + "_forog"])


def test_fixture_coverage(ref):
    """At T30 L8 every branch holds in at least 1 % of the columns; no decision within MIN_MARGIN of its threshold anywhere."""
    names = [str(x) for x in ref["t30_branch_names"]]
    counts = dict(zip(names, ref["t30_branch_counts"].tolist()))
    ncol = counts.pop("columns")
    assert ncol == 96 * 48
    assert set(counts) == set(surface.SFC_BRANCHES + surface.PBL_BRANCHES)
    for n, v in counts.items():
        assert v >= 0.01 * ncol, (n, v)
    for tag in support.PHYSICS_TAGS:
        assert float(ref[tag + "_min_margin"]) >= surface.MIN_MARGIN == 1e-9, tag


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_restatement_matches_reference(tag, ref):
    tab, c, sub, zon, sqcoa, r = reference_case(tag, ref)
    assert float(r["margin"].min()) == float(ref[tag + "_min_margin"])
    br = surface.branch_cols(r)
    names = [str(x) for x in ref[tag + "_branch_names"]][:-1]
    assert [int(br[n].sum()) for n in names] == ref[tag + "_branch_counts"].tolist()[:-1]
    for name, mask in br.items():                         # the stored sample holds every branch the state takes
        assert mask[sub].any() or not mask.any(), name
    worst = 0.0
    for n, v in restated(r, tab["kx"]).items():
        e = synth.relerr(np.asarray(v)[..., sub], ref["%s_%s" % (tag, n)])
        assert e <= TOL, (n, e)
        worst = max(worst, e)
    print("\n[surface restatement %s vs reference] worst %.1e" % (tag, worst))


def test_cabi_argument_checks(pkg):
    lib = pkg.load()
    S = pkg.spectral
    d = ctypes.c_void_p(8)
    bnd = S.SfcBoundary(*[8] * 7)
    sfc = lambda sp, nb, ptrs=None, b=bnd: lib.spdy_surface_fluxes_dev(sp.h, nb, *(ptrs or [d] * 8), ctypes.byref(b), d, d, d, None)
    pbl = lambda sp, nb, ptrs=None: lib.spdy_pbl_dev(sp.h, nb, *(ptrs or [d] * 12), None)
    chain = lambda sp, nb, sw=1, ptrs=None, alb=d, b=bnd: lib.spdy_column_physics_dev(sp.h, nb, sw, *(ptrs or [d] * 6), ctypes.byref(b),
                                                                                     alb, d, d, d, d, d, None)
    assert sfc(type("N", (), {"h": None}), 1) == -1      # NULL plan
    for kx in (4, 17):                                   # kx outside [5, 16]
        sp = pkg.Spectral("t30", kx=kx, max_batch=64, device=-1)
        assert sfc(sp, 1) == -1 and pbl(sp, 1) == -1 and chain(sp, 1) == -1
        assert lib.spdy_column_physics_workspace(sp.h) == -1
    sp = pkg.Spectral("t30", kx=6, max_batch=64, device=-1)
    assert sfc(sp, 1) == -5 and pbl(sp, 1) == -5 and chain(sp, 1) == -5        # no sigma levels
    sp = support.plan("t30", 4, device=-1)
    phis0 = np.zeros((48, 96))
    assert sfc(sp, 5) == -1 and pbl(sp, 5) == -1 and chain(sp, 5) == -1        # nb > max_batch comes first
    assert sfc(sp, 1) == -5                                                    # no orography
    assert chain(sp, 1) == -5                                                  # no date
    sp.radiation_set_date(0.25)
    assert chain(sp, 1) == -5                                                  # ... then no orography
    assert pbl(sp, 1) == -3                                                    # the boundary layer needs neither
    assert lib.spdy_surface_set_orography(sp.h, None) == -1
    bad = phis0.copy()
    bad[3, 4] = np.nan
    assert lib.spdy_surface_set_orography(sp.h, bad.ctypes.data_as(ctypes.c_void_p)) == -1
    assert sfc(sp, 1) == -5                                                    # a refused orography sets nothing
    sp.surface_set_orography(phis0)
    assert np.array_equal(sp.table("forog"), np.ones(48 * 96))
    assert sfc(sp, 1, ptrs=[d] * 7 + [None]) == -1                             # NULL slrd
    assert sfc(sp, 1, b=S.SfcBoundary(8, 8, 8, None, 8, 8, 8)) == -1           # NULL soilw
    assert lib.spdy_surface_fluxes_dev(sp.h, 1, *[d] * 8, None, d, d, d, None) == -1            # NULL boundary struct
    assert lib.spdy_surface_fluxes_dev(sp.h, 1, *[d] * 8, ctypes.byref(bnd), d, None, d, None) == -1   # NULL fsfcu
    assert pbl(sp, 1, ptrs=[d] * 6 + [None] + [d] * 5) == -1                   # NULL icnv
    assert pbl(sp, 1, ptrs=[d] * 11 + [None]) == -1                            # NULL qtend
    assert chain(sp, 1, ptrs=[None] + [d] * 5) == -1                           # NULL ug
    assert chain(sp, 1, alb=None) == -1                                        # NULL albsfc with compute_sw
    assert chain(sp, 1, 0, alb=None) == -3                                     # ... but not without it: valid, no device
    assert sfc(sp, 4) == -3 and pbl(sp, 4) == -3 and chain(sp, 4) == -3        # valid: no device
    assert sfc(sp, 0, ptrs=[None] * 8) == -3 and pbl(sp, 0, ptrs=[None] * 12) == -3   # nb = 0 needs no pointers
    assert lib.spdy_column_physics_workspace(sp.h) == -3
    sp = support.plan("t63k16", device=-1)
    sp.radiation_set_date(0.5)
    sp.surface_set_orography(np.zeros((96, 192)))
    assert sfc(sp, 1) == -3 and pbl(sp, 1) == -3 and chain(sp, 1) == -3
