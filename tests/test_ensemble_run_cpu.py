"""CPU: the coupled ensemble run's interface (include/spdy.h: spdy_ens_surface_model_create, spdy_surface_model_members,
spdy_ens_diagnostics_*, the plan option "ens_member_qcorh") without a device -- every new symbol in the library, the header, the
ctypes table and the Fortran binding; the two creates against their single forms; the error codes on a host-only plan; the layout
rule of the surface model's array (tests/ensemblerun.py restates it); the Python shapes."""
import ctypes

import numpy as np
import pytest

import ensemblerun as er
import support
from support import host_plan  # noqa: F401

ARG, NO_DEVICE = -1, -3
NEW = ("spdy_ens_surface_model_create", "spdy_surface_model_members", "spdy_ens_diagnostics_create", "spdy_ens_diagnostics_status",
       "spdy_ens_diagnostics_read", "spdy_ens_diagnostics_stopped")


def test_every_new_symbol_everywhere(host_plan):
    import speedy_f90_amd as s
    bound = support.fortran_bound()
    for n in NEW:
        assert hasattr(host_plan.lib, n), n
        assert n in s._lib.SIGNATURES, n
        assert support.declaration(n) is not None, n
        assert n in bound, n
    assert '"ens_member_qcorh"' in support.header(comments=True)


def test_creates_are_the_single_forms_with_nmem_after_the_plan():
    import speedy_f90_amd as s
    for one, ens in (("spdy_surface_model_create", "spdy_ens_surface_model_create"),
                     ("spdy_diagnostics_create", "spdy_ens_diagnostics_create")):
        a, b = support.declaration(one), support.declaration(ens)
        assert a is not None and b is not None, (one, ens)
        assert b == a.replace("spdy_plan *plan,", "spdy_plan *plan, int nmem,", 1), (a, b)
        sa, sb = s._lib.SIGNATURES[one], s._lib.SIGNATURES[ens]
        assert sb == sa[:1] + [ctypes.c_int] + sa[1:], ens


def test_host_only_plan(host_plan, oracle_factory):
    import speedy_f90_amd as s
    sp, lib = host_plan, host_plan.lib
    clim = er.host_climatology(sp, oracle_factory("t30"))
    for bad in (0, -1):
        with pytest.raises(s.SpdyError) as e:
            s.SurfaceModel(sp, clim, er.sm.DELT, nmem=bad)
        assert e.value.code == ARG
        with pytest.raises(s.SpdyError) as e:
            s.Diagnostics(sp, capacity=4, nmem=bad)
        assert e.value.code == ARG
    for nmem in (1, 3):
        m = s.SurfaceModel(sp, clim, er.sm.DELT, nmem=nmem)
        assert m.members() == nmem == lib.spdy_surface_model_members(m.h, None)
        assert m.members("sst_am") == nmem and m.members("corh") == nmem and m.members("stlcl_ob") == nmem
        assert m.members("fmask_l") == nmem
        assert m.members("alb0") == 1 and m.members("fmask_s") == 1 and m.members("cdice") == 1
        assert lib.spdy_surface_model_members(m.h, b"sst12") == ARG             # a climatology is not a field name
        assert lib.spdy_surface_model_members(None, None) == ARG
        for name in er.sm.FIELDS + er.sm.FORCING + ("fmask_l",):
            assert m.members(name) == nmem, name
        for name in er.SHARED_FIELDS:
            assert m.members(name) == 1, name
        x = np.zeros(8)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        p = ctypes.c_void_p()
        for rc in (lib.spdy_surface_model_couple_dev(m.h, 0, None, None, None, None),
                   lib.spdy_surface_model_couple_dev(m.h, 1, P(x), P(x), P(x), P(x)), lib.spdy_surface_model_forcing_dev(m.h, P(x)),
                   lib.spdy_surface_model_field(m.h, b"sst_am", ctypes.byref(p)), lib.spdy_surface_model_set_date(m.h, 1, 0.5, 0.04),
                   lib.spdy_surface_model_set_sst_anomaly(m.h, P(x))):
            assert rc == NO_DEVICE, nmem
        # the host tables do not depend on the members
        assert m.table("cdsea").shape == sp.grid_shape
        m.close()
    d = s.Diagnostics(sp, capacity=4, first_step=1, nmem=2)
    x = np.zeros(8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n, lev = ctypes.c_longlong(), ctypes.c_int()
    bad = (ctypes.c_longlong * 2)()
    status = lambda f, *a: f(d.h, *a, ctypes.byref(n), ctypes.byref(n), ctypes.byref(lev), ctypes.byref(lev), None)
    # the unsuffixed forms on an object of two members, and a member outside [0, nmem)
    assert status(lib.spdy_diagnostics_status) == ARG
    assert b"spdy_ens_diagnostics_status" in lib.spdy_last_error()
    assert lib.spdy_diagnostics_read(d.h, 1, 1, P(x)) == ARG
    assert b"spdy_ens_diagnostics_read" in lib.spdy_last_error()
    for member in (2, -1):
        assert status(lib.spdy_ens_diagnostics_status, member) == ARG
        assert lib.spdy_ens_diagnostics_read(d.h, member, 1, 1, P(x)) == ARG
    assert lib.spdy_ens_diagnostics_stopped(d.h, None) == ARG and lib.spdy_ens_diagnostics_stopped(None, bad) == ARG
    for rc in (status(lib.spdy_ens_diagnostics_status, 0), status(lib.spdy_ens_diagnostics_status, 1),
               lib.spdy_ens_diagnostics_read(d.h, 1, 1, 1, P(x)), lib.spdy_ens_diagnostics_stopped(d.h, bad),
               lib.spdy_diagnostics_check_dev(d.h, P(x), P(x), P(x)), lib.spdy_diagnostics_reset(d.h, 0)):
        assert rc == NO_DEVICE
    d.close()
    # one member: the unsuffixed forms are the member forms of member 0
    d = s.Diagnostics(sp, capacity=4)
    assert status(lib.spdy_diagnostics_status) == NO_DEVICE and status(lib.spdy_ens_diagnostics_status, 0) == NO_DEVICE
    assert status(lib.spdy_ens_diagnostics_status, 1) == ARG
    d.close()


def test_plan_option(host_plan):
    import speedy_f90_amd as s
    sp = host_plan
    sp.set_option("ens_member_qcorh", 1)
    sp.set_option("ens_member_qcorh", 0)
    for name, value in (("ens_member_qcorh", 2), ("ens_member_qcorh", -1), ("ens_member_tcorh", 1), ("no_such_option", 0)):
        with pytest.raises(s.SpdyError) as e:
            sp.set_option(name, value)
        assert e.value.code == ARG, (name, value)


def test_surface_layout_rule():
    """The array's layout as include/spdy.h states it, restated: with one member field n is slot n; the per-member fields are
    (nmem, il, ix) stacks, member e one grid after member e - 1; nothing overlaps and nothing is left out."""
    names = er.FIELD_ORDER
    for nmem in (1, 2, 5):
        slots = [er.surf_slot(n, nmem, e) for n in names for e in range(nmem if n in er.PER_MEMBER else 1)]
        clim = [er.surf_slot("clim%d" % i, nmem, 0) for i in range(63)]
        assert sorted(slots + clim) == list(range(len(names) + 63 + (nmem - 1) * len(er.PER_MEMBER)))
        for n in er.PER_MEMBER:
            assert [er.surf_slot(n, nmem, e) - er.surf_slot(n, nmem, 0) for e in range(nmem)] == list(range(nmem))
    assert [er.surf_slot(n, 1, 0) for n in names] == list(range(len(names)))
    assert len(er.PER_MEMBER) == 25 and set(er.PER_MEMBER) == set(er.sm.FIELDS + er.sm.FORCING + ("fmask_l",))


def test_python_shapes():
    from speedy_f90_amd import ensemble
    E, kx, nx, mx, il, ix = 3, 8, 32, 31, 48, 96
    base = ensemble.shapes(E, kx, nx, mx, il, ix)
    with_q = ensemble.shapes(E, kx, nx, mx, il, ix, member_qcorh=True)
    assert with_q["qcorh"] == ((E, nx, mx), True)
    assert base["qcorh"] == ((nx, mx), True) == ensemble.shapes(E, kx, nx, mx, il, ix, member_qcorh=False)["qcorh"]
    assert {k: v for k, v in with_q.items() if k != "qcorh"} == {k: v for k, v in base.items() if k != "qcorh"}
    assert list(with_q) == list(base)
