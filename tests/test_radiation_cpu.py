"""CPU: radiation (physics.f90:146-166, :180-186) -- the plan's radiation tables against the flang-built reference, the fixture's
coverage, the NumPy restatement (tests/radiation.py) against the reference, and the C ABI's argument checks on a host-only plan."""
import ctypes
import os

import numpy as np
import pytest

import moist
import radiation
import support
import synth
from conftest import GOLDEN, TOL
from support import pkg  # noqa: F401

ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_radiation.npz"))


def zonal_ref(ref, tag, di):
    return {n: ref["%s_d%d_%s" % (tag, di, n)] for n in ZON}


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_radiation_tables_bit_equal(tag, pkg, ref):
    """fband and, after spdy_radiation_set_date, the zonal forcing of both dates, bit for bit."""
    sp = support.plan(tag, device=-1)
    assert np.array_equal(sp.table("fband"), ref["fband"].ravel())
    assert np.array_equal(radiation.FBAND, ref["fband"])
    for n in ZON:
        assert sp.table(n).size == 0, n                     # no date yet
    for di, ty in enumerate(radiation.DATES):
        sp.radiation_set_date(ty)
        z = radiation.zonal(sp.table("sia_half"), sp.table("coa_half"), ty)
        for n in ZON:
            assert np.array_equal(sp.table(n), ref["%s_d%d_%s" % (tag, di, n)]), (n, di)
            assert np.array_equal(z[n], ref["%s_d%d_%s" % (tag, di, n)]), (n, di)


def test_fixture_coverage(ref):
    """At T30 L8 every branch holds in at least 1 % of the columns; each hemisphere has polar night at one of the dates."""
    names = [str(x) for x in ref["t30_branch_names"]]
    counts = dict(zip(names, ref["t30_branch_counts"].tolist()))
    ncol = counts.pop("columns")
    assert ncol == 96 * 48
    for n in ("cltop_nl1", "cltop_mid", "cltop_iptop", "cltop_2", "cltop_none", "strat_land", "strat_sea", "polar_night"):
        assert counts[n] >= 0.01 * ncol, (n, counts[n])
    for tag in support.PHYSICS_TAGS:
        il = support.grid(tag)[1]
        s0, s1 = ref["%s_d0_stratz" % tag], ref["%s_d1_stratz" % tag]
        assert np.any(s0[il // 2:] > 0) and np.any(s1[:il // 2] > 0), tag


def reference_case(tag, ref, di=0):
    """(tables, columns regenerated from the seed, column sample, zonal fields per column) -- the regeneration checked against
    the stored inputs."""
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    zon = radiation.zonal_columns(zonal_ref(ref, tag, di), 1, il, ix)
    c = radiation.columns(tab, il * ix, int(ref[tag + "_seed"]), radiation.zonal_columns(zonal_ref(ref, tag, 0), 1, il, ix))
    insub = ref[tag + "_insub"]
    for n in ("tg", "qg", "pslg", "fmask", "albsfc", "ts", "fsfcu", "tg2", "ts2", "fsfcu2"):
        assert np.array_equal(np.asarray(c[n]).reshape(-1, il * ix)[:, insub].squeeze(), ref["%s_in_%s" % (tag, n)]), n
    return tab, c, ref[tag + "_sub"], zon


def check(got, ref, key, sub):
    """the sample `sub` of a restated output [kx, ncol] / [ncol] against the fixture: integers identical, floats within TOL"""
    g, want = np.asarray(got)[..., sub], ref[key]
    if key.endswith("icltop"):
        assert np.array_equal(g, want), key
    else:
        assert synth.relerr(g, want) <= TOL, (key, synth.relerr(g, want))


@pytest.mark.parametrize("di", [0, 1])
@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_restatement_matches_reference(tag, di, ref):
    tab, c, sub, zon = reference_case(tag, ref, di)
    r1, r2 = radiation.two_steps(tab, c, zon)
    for name, mask in r1["branch_cols"].items():          # the stored sample holds every branch the state takes
        assert mask[sub].any() or not mask.any(), name
    for n in radiation.SW_OUT + ("icltop",):
        check(r1[n], ref, "%s_d%d_s1_%s" % (tag, di, n), sub)
    for n in radiation.NOSW_OUT:
        check(r2[n], ref, "%s_d%d_s2_%s" % (tag, di, n), sub)


def test_cabi_argument_checks(pkg):
    lib = pkg.load()
    d = ctypes.c_void_p(8)
    sfc = pkg.spectral.RadSurface(8, 8)
    down = lambda sp, nb, sw=1, ptrs=None: lib.spdy_radiation_down_dev(sp.h, nb, sw, *(ptrs or [d] * 8), ctypes.byref(sfc), d, None)
    upc = lambda sp, nb, ptrs=None: lib.spdy_radiation_up_dev(sp.h, nb, *(ptrs or [d] * 6), None)
    for kx in (4, 17):                                   # kx outside [5, 16]
        sp = pkg.Spectral("t30", kx=kx, max_batch=64, device=-1)
        assert down(sp, 1) == -1 and upc(sp, 1) == -1
        assert lib.spdy_radiation_state_size(sp.h) == -1
    sp = pkg.Spectral("t30", kx=6, max_batch=64, device=-1)
    lib.spdy_radiation_set_date(sp.h, ctypes.c_double(0.1))
    assert down(sp, 1) == -5 and upc(sp, 1) == -5        # no sigma levels
    sp = support.plan("t30", 4, device=-1)
    assert lib.spdy_radiation_state_size(sp.h) == (6 * 8 + 7) * 96 * 48
    assert down(sp, 1) == -5 and upc(sp, 1) == -5        # no date
    assert lib.spdy_radiation_set_date(sp.h, ctypes.c_double(0.25)) == 0
    assert down(sp, 5) == -1                             # nb > max_batch
    assert down(sp, 1, ptrs=[d, d, d, None] + [d] * 4) == -1          # NULL pslg
    assert down(sp, 1, ptrs=[d] * 4 + [None] + [d] * 3) == -1        # NULL rh with compute_sw
    assert down(sp, 1, 0, ptrs=[d] * 4 + [None] * 4) == -3            # ... but not without it: valid, no device
    assert upc(sp, 1, ptrs=[d] * 5 + [None]) == -1                    # NULL ttend
    assert down(sp, 4) == -3 and upc(sp, 4) == -3                     # valid: no device
    assert down(sp, 0, ptrs=[None] * 8) == -3                         # nb = 0 needs no pointers
    sp = support.plan("t63k16", device=-1)
    sp.radiation_set_date(0.5)
    assert down(sp, 1) == -3 and upc(sp, 1) == -3
