"""CPU: the ensemble form of the SPPT pattern (include/spdy.h, "SPPT": spdy_ens_sppt_create, spdy_sppt_members, spdy_ens_sppt_reset,
spdy_ens_sppt_draws, spdy_ens_physics_sppt_workspace, spdy_ens_physics_sppt_dev) without a device, T30 L8 on a host-only plan: the
symbols in the library, the header, the ctypes table and the Fortran binding; the documented error codes and their order; the
tables of an object of three members against a single object's."""
import ctypes

import numpy as np
import pytest

import support
from support import host_plan  # noqa: F401

ARG, NO_DEVICE, STATE = -1, -3, -5
NEW = ("spdy_ens_sppt_create", "spdy_sppt_members", "spdy_ens_sppt_reset", "spdy_ens_sppt_draws", "spdy_ens_physics_sppt_workspace",
       "spdy_ens_physics_sppt_dev")
TABLES = ("phi", "f0", "first", "sigma", "mu")


def _seeds(*values):
    return (ctypes.c_ulonglong * len(values))(*values)


def test_every_new_symbol_everywhere(host_plan):
    import speedy_f90_amd as s
    lib = host_plan.lib
    for n in NEW:                                   # the first lookup: fails here without the feature
        assert hasattr(lib, n), n
    bound = support.fortran_bound()
    for n in NEW:
        assert n in s._lib.SIGNATURES, n
        assert support.declaration(n) is not None, n
        assert n in bound, n
    sig = s._lib.SIGNATURES
    # the ensemble physics with SPPT is spdy_ens_physics_dev with the object after nmem, and the single form with nmem after the plan
    assert sig["spdy_ens_physics_sppt_dev"] == sig["spdy_ens_physics_dev"][:2] + [ctypes.c_void_p] + sig["spdy_ens_physics_dev"][2:]
    assert sig["spdy_ens_physics_sppt_dev"] == sig["spdy_physics_sppt_dev"][:1] + [ctypes.c_int] + sig["spdy_physics_sppt_dev"][1:]
    assert sig["spdy_ens_physics_sppt_workspace"] == sig["spdy_ens_physics_workspace"]
    assert "SPPT (a pattern object holds one pattern)" not in support.header(comments=True)


def test_create_members_and_error_codes(host_plan):
    import speedy_f90_amd as s
    sp, lib, h = host_plan, host_plan.lib, ctypes.c_void_p()
    three = _seeds(11, 12, 13)
    assert lib.spdy_ens_sppt_create(None, 3, 36, None, three, ctypes.byref(h)) == ARG
    for nmem in (0, -2):
        assert lib.spdy_ens_sppt_create(sp.h, nmem, 36, None, three, ctypes.byref(h)) == ARG, nmem
    assert lib.spdy_ens_sppt_create(sp.h, 3, 36, None, None, ctypes.byref(h)) == ARG              # NULL seeds
    assert lib.spdy_ens_sppt_create(sp.h, 3, 36, None, three, None) == ARG                        # NULL result pointer
    assert lib.spdy_ens_sppt_create(sp.h, 3, 0, None, three, ctypes.byref(h)) == ARG              # nsteps
    assert lib.spdy_sppt_members(None) == ARG
    for nmem in (1, 3):
        pat = s.Sppt(sp, 36, nmem=nmem, seed=5)
        assert pat.members() == nmem == lib.spdy_sppt_members(pat.h)
        n = ctypes.c_longlong()
        for member in (nmem, -1):                                                               # outside [0, nmem): before the device
            assert lib.spdy_ens_sppt_reset(pat.h, member, 1) == ARG, (nmem, member)
            assert lib.spdy_ens_sppt_draws(pat.h, member, ctypes.byref(n)) == ARG, (nmem, member)
        assert lib.spdy_ens_sppt_draws(pat.h, 0, None) == ARG                                     # NULL result pointer
        assert lib.spdy_ens_sppt_reset(None, 0, 1) == ARG and lib.spdy_ens_sppt_draws(None, 0, ctypes.byref(n)) == ARG
        for member in range(nmem):                                                              # everything right: no device, last
            assert lib.spdy_ens_sppt_reset(pat.h, member, 1) == NO_DEVICE
            assert lib.spdy_ens_sppt_draws(pat.h, member, ctypes.byref(n)) == NO_DEVICE
        assert lib.spdy_sppt_reset(pat.h, 1) == NO_DEVICE and lib.spdy_sppt_draws(pat.h, ctypes.byref(n)) == NO_DEVICE
        assert lib.spdy_sppt_advance_dev(pat.h, None) == NO_DEVICE
        p = ctypes.c_void_p()
        assert lib.spdy_sppt_field(pat.h, b"pattern", ctypes.byref(p)) == NO_DEVICE
        pat.close()
    pat = s.Sppt(sp, 36, seeds=[7, 8])
    assert pat.members() == 2
    pat.close()
    with pytest.raises(s.SpdyError) as e:
        s.Sppt(sp, 36, nmem=0)
    assert e.value.code == ARG
    with pytest.raises(ValueError):
        s.Sppt(sp, 36, nmem=3, seeds=[1, 2])


def test_tables_do_not_depend_on_the_members(host_plan):
    import speedy_f90_amd as s
    sp = host_plan
    mu = np.linspace(0.0, 1.0, sp.kx)
    one, three = s.Sppt(sp, 36, mu, seed=1), s.Sppt(sp, 36, mu, seeds=[4, 5, 6])
    for n in TABLES:
        assert np.array_equal(np.asarray(one.table(n)), np.asarray(three.table(n))), n
    assert three.table("sigma").shape == (sp.nx, sp.mx) and np.array_equal(three.table("mu"), mu)
    one.close(); three.close()


def _physics_call(lib, h, nmem, pat, null=False):
    """rc of spdy_ens_physics_sppt_dev on dummy non-null pointers (no check dereferences one)"""
    import speedy_f90_amd as s
    x = np.zeros(4)
    Q = x.ctypes.data_as(ctypes.c_void_p)
    P = None if null else Q
    bnd = s.spectral.SfcBoundary(*[Q] * 7)
    out = s.spectral.ColumnPhysicsOut()
    return lib.spdy_ens_physics_sppt_dev(h, nmem, pat, 1, P, *[Q] * 5, ctypes.byref(bnd), Q, Q, Q, Q, Q, Q, ctypes.byref(out))


def test_physics_call_in_the_documented_order():
    """As spdy_ens_physics_dev -- NULL plan, nmem < 1, max_batch < nmem*(3*kx+1): ARG; date and orography: STATE; a NULL required
    pointer, s among them: ARG -- then s of another plan and s of another member count: ARG; the host-only plan last."""
    import speedy_f90_amd as s
    kx = 8
    sp = s.Spectral("t30", kx=kx, max_batch=2 * (3 * kx + 1), device=-1)                       # room for two members, not three
    other = s.Spectral("t30", kx=kx, max_batch=2 * (3 * kx + 1), device=-1)
    lib = sp.lib
    two, three, foreign = s.Sppt(sp, 36, nmem=2), s.Sppt(sp, 36, nmem=3), s.Sppt(other, 36, nmem=2)
    assert _physics_call(lib, None, 2, two.h) == ARG
    assert lib.spdy_ens_physics_sppt_workspace(None, 2) == ARG
    for nmem in (0, -1, 3):
        assert _physics_call(lib, sp.h, nmem, three.h) == ARG, nmem
        assert lib.spdy_ens_physics_sppt_workspace(sp.h, nmem) == ARG, nmem
    assert lib.spdy_ens_physics_sppt_workspace(sp.h, 2) == NO_DEVICE
    assert _physics_call(lib, sp.h, 2, three.h) == STATE                                      # no date yet: before s is looked at
    sp.radiation_set_date(0.0)
    assert _physics_call(lib, sp.h, 2, two.h) == STATE                                        # no orography yet
    sp.surface_set_orography(np.zeros(sp.grid_shape))
    assert _physics_call(lib, sp.h, 2, two.h, null=True) == ARG                               # a NULL spectrum
    assert _physics_call(lib, sp.h, 2, None) == ARG                                           # s is a required pointer
    assert _physics_call(lib, sp.h, 2, foreign.h) == ARG and b"another plan" in lib.spdy_last_error()
    assert _physics_call(lib, sp.h, 2, three.h) == ARG and b"3 patterns" in lib.spdy_last_error()
    one = s.Sppt(sp, 36)
    assert _physics_call(lib, sp.h, 2, one.h) == ARG
    assert _physics_call(lib, sp.h, 1, two.h) == ARG
    x = np.zeros(4)
    Q = x.ctypes.data_as(ctypes.c_void_p)
    bnd, out = s.spectral.SfcBoundary(*[Q] * 7), s.spectral.ColumnPhysicsOut()
    single = lambda pat: lib.spdy_physics_sppt_dev(sp.h, pat, 1, *[Q] * 6, ctypes.byref(bnd), Q, Q, Q, Q, Q, Q, ctypes.byref(out))
    assert single(two.h) == ARG                                                              # the single state takes one pattern
    assert single(one.h) == NO_DEVICE
    assert _physics_call(lib, sp.h, 2, two.h) == NO_DEVICE                                    # everything right: no device, last
    assert _physics_call(lib, sp.h, 1, one.h) == NO_DEVICE
    for pat in (one, two, three, foreign):
        pat.close()
    sp.close(); other.close()


def test_python_surface(host_plan):
    """Ensemble.physics_workspace takes the flag, and a pattern object of another member count is refused before any call"""
    import inspect
    import speedy_f90_amd as s
    assert "sppt" in inspect.signature(s.Ensemble.physics_workspace).parameters
    assert list(inspect.signature(s.Sppt.__init__).parameters)[1:] == ["sp", "nsteps", "mu", "seed", "nmem", "seeds"]
    assert "member" in inspect.signature(s.Sppt.reset).parameters and "member" in inspect.signature(s.Sppt.draws).parameters
    for n in ("ens_physics_sppt_workspace", "ens_physics_sppt_dev"):
        assert hasattr(s.Spectral, n), n
    with pytest.raises(s.SpdyError) as e:
        host_plan.ens_physics_sppt_workspace(0)
    assert e.value.code == ARG
