"""CPU: moist physics (physics.f90:110-138) -- the plan's physics tables against the flang-built reference, the fixture's
coverage, the NumPy restatement (tests/moist.py) against the reference, and the C ABI's argument checks on a host-only plan."""
import ctypes
import os

import numpy as np
import pytest

import moist
import support
import synth
from conftest import GOLDEN
from support import pkg  # noqa: F401

TABLES = ("sigl", "sigh", "grdsig", "grdscp", "wvi", "entr")
FLOATS = ("ttend", "qtend", "precnv", "precls", "cbmf", "qsat", "rh", "se")
INTS = ("iptop", "icnv")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_moist.npz"))


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_physics_tables_bit_equal(tag, pkg, ref):
    sp = support.plan(tag, device=-1)
    for n in TABLES:
        assert np.array_equal(sp.table(n), ref["%s_tab_%s" % (tag, n)]), n


def test_fixture_coverage(ref):
    """At T30 L8 every branch of the block holds in at least 1 % of the columns, and no decision is within 1e-9 of its tie."""
    names = [str(x) for x in ref["t30_branch_names"]]
    counts = dict(zip(names, ref["t30_branch_counts"].tolist()))
    ncol = counts.pop("columns")
    assert ncol == 96 * 48
    for n in ("psmin_cut", "conv_ktop2", "conv_lqthr", "no_conv", "secondary_flux", "lsc_kx", "lsc_interior", "qsat_warm",
              "qsat_cold", "q_clamp"):
        assert counts[n] >= 0.01 * ncol, (n, counts[n])
    for tag in support.PHYSICS_TAGS:
        assert float(ref[tag + "_min_margin"]) >= moist.MIN_MARGIN, tag


def reference_case(tag, ref):
    """(tables, inputs regenerated from the seed [1, kx, il, ix], column sample) -- the regeneration checked against the stored inputs."""
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    ins = moist.grid_inputs(tab, (1, il, ix), int(ref[tag + "_seed"]))
    sub, insub = ref[tag + "_sub"], ref[tag + "_insub"]
    for n, a in zip(("tg", "qg", "phig", "pslg", "ttend", "qtend"), ins):
        assert np.array_equal(a[0].reshape(-1, il * ix)[:, insub].squeeze(), ref["%s_in_%s" % (tag, n)]), n
    return tab, ins, sub


def pick(a, sub, ncol):
    return np.asarray(a).reshape(-1, ncol)[:, sub].squeeze()


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_restatement_matches_reference(tag, ref):
    tab, ins, sub = reference_case(tag, ref)
    ncol = ins[3].size
    r = moist.block(tab, *ins)
    for name, mask in r["branch_cols"].items():       # the stored sample holds every branch the state takes
        assert mask[sub].any() or not mask.any(), name
    for n in INTS:
        assert np.array_equal(pick(r[n], sub, ncol), ref["%s_%s" % (tag, n)]), n
    for n in FLOATS:
        assert synth.relerr(pick(r[n], sub, ncol), ref["%s_%s" % (tag, n)]) <= 1e-13, n
    if tag == "t30k5":      # convection.f90:198: do k = kx-3, 3, -1 is empty at kx = 5
        assert np.all(ref["t30k5_icnv"] == -1)


def test_cabi_argument_checks(pkg):
    lib = pkg.load()
    dummy = ctypes.c_void_p(8)
    ptrs = [dummy] * 6
    # kx outside [5, 16]
    for kx in (4, 17):
        sp = pkg.Spectral("t30", kx=kx, max_batch=64, device=-1)
        assert lib.spdy_moist_columns_dev(sp.h, 1, *ptrs, None) == -1
        assert lib.spdy_moist_physics_dev(sp.h, *ptrs, None) == -1
    sp = support.plan("t30", 4, device=-1)
    assert lib.spdy_moist_columns_dev(sp.h, 5, *ptrs, None) == -1            # nb > max_batch
    assert lib.spdy_moist_columns_dev(sp.h, 1, *ptrs[:4], None, dummy, None) == -1   # NULL ttend
    assert lib.spdy_moist_columns_dev(sp.h, 4, *ptrs, None) == -3            # valid: no device
    assert lib.spdy_moist_physics_dev(sp.h, *ptrs, None) == -1               # max_batch < 3 kx + 1
    sp = support.plan("t30", 25, device=-1)
    assert lib.spdy_moist_physics_dev(sp.h, *ptrs[:4], None, dummy, None) == -1      # NULL ttend
    assert lib.spdy_moist_physics_dev(sp.h, *ptrs, None) == -3
    assert lib.spdy_moist_workspace(sp.h) == -3
    out = pkg.spectral.MoistOut()
    assert lib.spdy_moist_columns_dev(sp.h, 1, *ptrs, ctypes.byref(out)) == -3
    sp = support.plan("t63k16", device=-1)
    assert lib.spdy_moist_columns_dev(sp.h, 1, *ptrs, None) == -3
