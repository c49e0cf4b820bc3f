"""CPU: the ensemble time step's interface without a device -- the new entry points exist in the library, the loader and the
Fortran binding; a host-only plan answers their argument checks in the documented order (include/spdy.h, "ensemble time step"); and
the layout that speedy.f90_amd/ensemble.py owns is the one the kernels index, pinned as shapes, strides and offsets."""
import ctypes
import re

import numpy as np
import pytest

import speedy_f90_amd as s
import support
from speedy_f90_amd import _lib, ensemble

ARG, NO_DEVICE, STATE = -1, -3, -5
NEW = ("grid_tendencies_dev", "spectral_step_dev", "direct_batch_spectral_step_dev", "geopotential_dev", "physics_workspace",
       "physics_dev")


def test_symbols_in_library_header_loader_and_fortran():
    lib = s.load()
    bound = support.fortran_bound()
    for n in NEW:
        name = "spdy_ens_" + n
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.match(r"spdy_plan \*plan, int nmem\b", support.declaration(name)), name             # nmem right after the plan
        assert name in bound, name
        assert _lib.SIGNATURES[name][:2] == [ctypes.c_void_p, ctypes.c_int], name
    # each generalises its neighbour: the single-state signature with nmem inserted
    for n in NEW:
        assert _lib.SIGNATURES["spdy_ens_" + n] == (_lib.SIGNATURES["spdy_" + n][:1] + [ctypes.c_int] + _lib.SIGNATURES["spdy_" + n][1:]), n
    assert s.Ensemble is ensemble.Ensemble


def _calls(lib, h, nmem, j1=2, null=False):
    """rc of the four step calls and the two physics calls on dummy non-null pointers (no check dereferences one)"""
    x = np.zeros(4)
    P = None if null else x.ctypes.data_as(ctypes.c_void_p)
    Q = x.ctypes.data_as(ctypes.c_void_p)
    bnd = s.spectral.SfcBoundary(*[P] * 7)
    out = s.spectral.ColumnPhysicsOut()
    return {"grid": lib.spdy_ens_grid_tendencies_dev(h, nmem, P, *[Q] * 10),
            "spec": lib.spdy_ens_spectral_step_dev(h, nmem, P, *[Q] * 10, 0.0, j1, 1.0, 0.0, 0.5, Q),
            "comp": lib.spdy_ens_direct_batch_spectral_step_dev(h, nmem, P, Q, Q, 2, *[Q] * 11, 0.0, j1, 1.0, 0.0, 0.5, Q),
            "geop": lib.spdy_ens_geopotential_dev(h, nmem, P, Q, Q),
            "phys": lib.spdy_ens_physics_dev(h, nmem, 1, P, *[Q] * 5, ctypes.byref(bnd), Q, Q, Q, Q, Q, Q, ctypes.byref(out)),
            "work": lib.spdy_ens_physics_workspace(h, nmem)}


def test_error_codes_in_documented_order():
    """NULL plan, nmem < 1, kx > 16 with nmem > 1, max_batch < nmem*(3*kx+1): ARG; then what the single-state call needs: STATE;
    then a NULL pointer, then j1: ARG; the host-only plan last"""
    lib = s.load()
    kx = 8
    sp = s.Spectral("t30", kx=kx, max_batch=2 * (3 * kx + 1), device=-1)                      # room for two members, not three
    assert set(_calls(lib, None, 1).values()) == {ARG}
    for nmem in (0, -1, 3):                                                                  # 3: max_batch < nmem*(3*kx+1)
        assert set(_calls(lib, sp.h, nmem).values()) == {ARG}, nmem
    # (the batch check comes before the state checks: nothing is initialised yet and nmem = 3 gave ARG above.)  Now the state:
    rc = _calls(lib, sp.h, 2)
    assert (rc["grid"], rc["spec"], rc["comp"]) == (STATE,) * 3                               # no spdy_implicit_init yet
    assert rc["geop"] == NO_DEVICE                                                           # kx = 8 has sigma levels: all checks pass
    assert rc["phys"] == STATE and rc["work"] == NO_DEVICE                                    # no date yet; the workspace needs none
    assert _calls(lib, sp.h, 2, null=True)["grid"] == STATE                                  # state before the pointers
    sp.initialize_implicit(2400.0)
    sp.radiation_set_date(0.0)
    assert _calls(lib, sp.h, 2)["phys"] == STATE                                             # no orography yet
    sp.surface_set_orography(np.zeros(sp.grid_shape))
    rc = _calls(lib, sp.h, 2, null=True)
    assert {rc[k] for k in ("grid", "spec", "comp", "geop", "phys")} == {ARG}                 # a NULL required pointer
    rc = _calls(lib, sp.h, 2, j1=3)
    assert (rc["spec"], rc["comp"]) == (ARG, ARG) and rc["grid"] == NO_DEVICE                 # j1 outside {1, 2}
    assert set(_calls(lib, sp.h, 2).values()) == {NO_DEVICE}                                 # everything right: no device, last
    assert set(_calls(lib, sp.h, 1).values()) == {NO_DEVICE}
    sp.close()
    # more than one member needs the block-per-levels kernels (kx <= 16); one member is accepted at any level count
    big = s.Spectral("t30", kx=20, max_batch=2 * 61, device=-1)
    rc = _calls(lib, big.h, 2)
    assert {rc[k] for k in ("grid", "spec", "comp", "geop")} == {ARG}
    rc = _calls(lib, big.h, 1)
    assert rc["grid"] == STATE and rc["geop"] == STATE                                       # (kx = 20 has no sigma levels of its own)
    assert rc["phys"] == ARG and rc["work"] == ARG                                           # the column physics: kx in [5, 16]
    big.close()
    with pytest.raises(ValueError):
        s.Ensemble(s.Spectral("t30", kx=8, max_batch=49, device=-1), 2)


def _offset(shape, index):
    """element offset of index in a C-contiguous array of `shape`"""
    return int(np.ravel_multi_index(index, shape))


@pytest.mark.parametrize("E,kx", [(1, 8), (3, 8), (2, 5)])
def test_layout_pinned(E, kx):
    """The formulas of the layout, on arrays of the ensemble's shapes (NumPy stands in for the device tensors: the views are made
    by the same indexing): member e's level k of a group-major array is field slot g*E*kx + e*kx + k, its level-free field slot
    3*E*kx + e; the time levels of a prognostic are E*kx fields apart; E = 1 is the single state's layout."""
    nx, mx, il, ix = 32, 31, 48, 96
    sh = ensemble.shapes(E, kx, nx, mx, il, ix)
    spec, grid = nx * mx, il * ix
    assert sh["vor"] == ((2, E, kx, nx, mx), True) and sh["ps"] == ((2, E, nx, mx), True) and sh["phis"] == ((nx, mx), True)
    assert sh["phi"][0] == (E, kx, nx, mx) and sh["ug"][0] == (E, kx, il, ix) and sh["px"][0] == (E, il, ix)
    assert sh["plain_g"][0] == (4, E, kx, il, ix) and sh["U"][0] == sh["V"][0] == (3, E, kx, il, ix)
    assert sh["PL"][0] == (3 * E * kx + E, il, ix) and sh["pspec"][0] == (3 * E * kx + E, nx, mx) and sh["pvor"][0] == (3, E, kx, nx, mx)
    for n in ("vor", "div", "t", "tr"):
        for lv in range(2):
            for e in range(E):
                for k in (0, kx - 1):
                    assert _offset(sh[n][0], (lv, e, k, 0, 0)) == ((lv * E + e) * kx + k) * spec
        assert _offset(sh[n][0], (1, 0, 0, 0, 0)) == E * kx * spec                               # the stride between time levels
    for e in range(E):
        assert _offset(sh["ps"][0], (1, e, 0, 0)) == (E + e) * spec
        assert _offset(sh["px"][0], (e, 0, 0)) == e * grid
        for g in range(3):
            for k in (0, kx - 1):
                slot = g * E * kx + e * kx + k
                assert _offset(sh["U"][0], (g, e, k, 0, 0)) == slot * grid and _offset(sh["pdiv"][0], (g, e, k, 0, 0)) == slot * spec
        for g in range(4):                                                                      # vorg | divg | tg | trg
            assert _offset(sh["plain_g"][0], (g, e, 0, 0, 0)) == (g * E + e) * kx * grid
    # the views a real Ensemble makes (torch tensors on the CPU over a host-only plan): offsets and strides in elements
    sp = s.Spectral("t30", kx=kx, max_batch=E * (4 * kx + 4), device=-1)
    ens = s.Ensemble(sp, E, device="cpu")
    for n, (shape, cplx) in sh.items():
        t = getattr(ens, n)
        assert tuple(t.shape) == shape and t.is_complex() == cplx and t.is_contiguous(), n

    def at(view, base):
        """element offset of a view inside the array it is a view of"""
        assert view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
        return view.storage_offset() - base.storage_offset()
    for e in range(E):
        D = ens.member(e)
        assert set(D) == {"vor", "div", "t", "tr", "ps", "phis", "tcorh", "qcorh"}
        for n in ("vor", "div", "t", "tr"):
            v = D[n]
            assert tuple(v.shape) == (2, kx, nx, mx) and v.stride() == (E * kx * spec, spec, mx, 1), n
            assert at(v, getattr(ens, n)) == e * kx * spec and v[0].is_contiguous() and v[1].is_contiguous(), n
        assert tuple(D["ps"].shape) == (2, nx, mx) and D["ps"].stride() == (E * spec, mx, 1) and at(D["ps"], ens.ps) == e * spec
        for n in ("phis", "tcorh", "qcorh"):
            assert D[n] is getattr(ens, n)                                                      # shared, not copied
        # the level-free fields behind PL's three groups, and the physics tendencies: (E, kx) stacks inside U, V, PL
        assert at(ens.PLs[e], ens.PL) == (3 * E * kx + e) * grid and tuple(ens.PLs.shape) == (E, il, ix)
        for g in range(3):
            assert at(ens.PLg[g, e], ens.PL) == (g * E * kx + e * kx) * grid
        assert tuple(ens.PLg.shape) == (3, E, kx, il, ix) and ens.PLg.stride() == (E * kx * grid, kx * grid, grid, ix, 1)
        assert at(ens.utend[e], ens.U) == e * kx * grid and at(ens.vtend[e], ens.V) == e * kx * grid
        assert at(ens.ttend[e], ens.PL) == (E * kx + e * kx) * grid and at(ens.qtend[e], ens.PL) == (2 * E * kx + e * kx) * grid
        for g, n in enumerate(("vorg", "divg", "tg", "trg")):
            assert at(getattr(ens, n)[e], ens.plain_g) == (g * E + e) * kx * grid, n
    for n in ("utend", "vtend", "ttend", "qtend", "vorg", "divg", "tg", "trg"):
        t = getattr(ens, n)
        assert tuple(t.shape) == (E, kx, il, ix) and t.is_contiguous(), n
    # set_member / set_shared write where member() reads
    st = {n: np.full((2, kx, nx, mx), 1.0 + e, np.complex128) for n in ("vor", "div", "t", "tr")}
    st["ps"] = np.full((2, nx, mx), 7.0, np.complex128)
    ens.set_member(E - 1, st)
    assert ens.vor[1, E - 1, kx - 1, 0, 0] == 1.0 + e and ens.ps[1, E - 1, 0, 0] == 7.0 and (E == 1 or ens.vor[1, 0, 0, 0, 0] == 0.0)
    if E == 1:                                                                                  # the single state's layout
        assert ens.member(0)["vor"].is_contiguous() and ens.PL.shape[0] == 3 * kx + 1 and ens.U.view(-1, il, ix).shape[0] == 3 * kx
    sp.close()
