"""CPU: the full-physics time step -- the C ABI's argument checks of spdy_physics_dev / spdy_physics_workspace and the plan option
"physics_fused" on a host-only plan, and the reference side of tests/test_gpu_physics_step.py (tests/physstep.py): the committed
seeds give a first step whose every decision is clear of its threshold and that exercises the physics."""
import ctypes

import numpy as np
import pytest

import physstep
import support
from conftest import VARIANTS
from support import pkg  # noqa: F401


def test_cabi_argument_checks(pkg):
    """One bad argument at a time, in the order include/spdy.h states: plan / kx / sigma / date / orography / NULL pointers /
    max_batch / host-only plan last."""
    lib = pkg.load()
    S = pkg.spectral
    d = ctypes.c_void_p(8)
    bnd = S.SfcBoundary(*[8] * 7)
    phys = lambda sp, sw=1, ptrs=None, alb=d, b=bnd, st=d, tend=None: lib.spdy_physics_dev(
        sp.h, sw, *(ptrs or [d] * 6), ctypes.byref(b) if b is not None else None, alb, st, *(tend or [d] * 4), None)
    none = type("N", (), {"h": None})
    assert phys(none) == -1 and lib.spdy_physics_workspace(None) == -1           # NULL plan
    for kx in (4, 17):                                                           # kx outside [5, 16]
        sp = pkg.Spectral("t30", kx=kx, max_batch=64, device=-1)
        assert phys(sp) == -1 and lib.spdy_physics_workspace(sp.h) == -1
    sp = pkg.Spectral("t30", kx=6, max_batch=64, device=-1)
    assert phys(sp) == -5                                                        # no sigma levels
    assert lib.spdy_physics_workspace(sp.h) == -3                                # the workspace needs none: no device
    sp = support.plan("t30", 4, device=-1)                                         # max_batch 4 < 3 kx + 1: comes late
    assert phys(sp) == -5                                                        # no date
    sp.radiation_set_date(0.25)
    assert phys(sp) == -5                                                        # ... then no orography
    sp.surface_set_orography(np.zeros((48, 96)))
    for i in range(6):                                                           # NULL vor div t q phi ps
        assert phys(sp, ptrs=[d] * i + [None] + [d] * (5 - i)) == -1, i
    assert phys(sp, b=None) == -1                                                # NULL boundary struct
    assert phys(sp, b=S.SfcBoundary(8, 8, None, 8, 8, 8, 8)) == -1               # NULL stl
    assert phys(sp, alb=None) == -1                                              # NULL albsfc with compute_sw
    assert phys(sp, st=None) == -1                                               # NULL radiation state
    for i in range(4):                                                           # NULL utend vtend ttend qtend
        assert phys(sp, tend=[d] * i + [None] + [d] * (3 - i)) == -1, i
    assert phys(sp) == -1                                                        # max_batch < 3 kx + 1
    assert b"3*kx+1" in lib.spdy_last_error()
    sp = support.plan("t30", 25, device=-1)                                        # exactly 3 kx + 1
    assert phys(sp, ptrs=[None] + [d] * 5) == -5                                 # state errors before pointers
    sp.radiation_set_date(0.25)
    sp.surface_set_orography(np.zeros((48, 96)))
    assert phys(sp, ptrs=[None] + [d] * 5) == -1
    assert phys(sp) == -3 and phys(sp, 0, alb=None) == -3                        # valid: no device
    assert lib.spdy_physics_workspace(sp.h) == -3
    sp = support.plan("t63k16", 49, device=-1)
    sp.radiation_set_date(0.5)
    sp.surface_set_orography(np.zeros((96, 192)))
    assert phys(sp) == -3
    sp = support.plan("t63k16", 48, device=-1)
    sp.radiation_set_date(0.5)
    sp.surface_set_orography(np.zeros((96, 192)))
    assert phys(sp) == -1


def test_physics_fused_option(pkg):
    lib = pkg.load()
    sp = support.plan("t30", 4, device=-1)
    for v in (0, 1, 1, 0):
        assert lib.spdy_plan_set_option(sp.h, b"physics_fused", v) == 0
    for v in (-1, 2, 7):
        assert lib.spdy_plan_set_option(sp.h, b"physics_fused", v) == -1, v
    sp.set_option("physics_fused", 1)


def test_python_binding(pkg):
    """physics_workspace / physics_dev reach the library (a host-only plan answers SPDY_ERR_NO_DEVICE)."""
    sp = support.plan("t30", 4, device=-1)
    with pytest.raises(pkg.SpdyError) as e:
        sp.physics_workspace()
    assert e.value.code == -3
    assert callable(sp.physics_dev)


def test_reference_side_first_step(oracle_factory):
    """The committed seeds at T30 L8: every decision margin of the first step's physics >= MIN_MARGIN in every column, and the
    state exercises the physics (some but not all columns convect, condensation, both surface stability branches)."""
    tag = "t30"
    kx = VARIANTS[tag][3]
    o = oracle_factory(tag)
    sp = support.plan(tag, 4 * kx + 4, device=-1)
    case = physstep.Case(tag, sp, o)
    z = lambda: np.zeros((kx, o.il, o.ix))
    st = {}
    r = case.physics(case.st, True, st, z(), z(), z(), z())
    physstep.check_coverage(r, "t30 step 1")
    assert physstep.rad_state_array(st, kx).shape == (6 * kx + 7, o.il * o.ix)
    exp = physstep.expected(r, kx, o.il, o.ix)
    assert set(exp["rad"]) == {"cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "slrd", "slr", "olr", "tt_rsw", "tt_rlw"}
