"""CPU: the member mask's entry points on a host-only plan (include/spdy.h, "member mask"): they exist and are bound, check their
arguments in the order of the calls they extend -- the object, its plan, the localisation, the pointers, for verify the member
count and the slot -- accept a NULL mask up to the check of the device, which comes last; "members_used" is a field name; and the
Python wrappers refuse a mask of the wrong length or type as Ensemble.output does."""
import ctypes

import numpy as np
import pytest

import support
from support import package

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
KX, NMEM = 8, 3
NEW = ("spdy_mask_letkf_analyse_grid_dev", "spdy_mask_ens_letkf_dev", "spdy_mask_nature_verify_dev", "spdy_mask_nature_verify_grid_dev",
       "spdy_mask_from_diagnostics_dev")


class Host:
    def __init__(self):
        s = package()
        self.s, self.lib = s, s.load()
        self.sp = s.Spectral("t30", kx=KX, max_batch=NMEM * 4 * KX, device=-1)
        self.lt = s.Letkf(self.sp, NMEM, 4, 1.0e6)
        self.nat = s.Nature(self.sp, capacity=2)
        self.diag = s.Diagnostics(self.sp, capacity=2, nmem=NMEM)
        self.bare = ctypes.c_void_p()                          # an analysis object whose localisation was never set
        assert self.lib.spdy_letkf_create(self.sp.h, NMEM, 4, ctypes.byref(self.bare)) == OK
        self.gone = s.Spectral("t30", kx=KX, max_batch=NMEM * 4 * KX, device=-1)
        self.dead = [s.Letkf(self.gone, NMEM, 4, 1.0e6), s.Nature(self.gone), s.Diagnostics(self.gone, capacity=2, nmem=NMEM)]
        self.gone.close()
        self.buf = np.zeros(64)
        self.q = self.buf.ctypes.data_as(ctypes.c_void_p)      # a non-null "device pointer": no check dereferences one

    def close(self):
        assert self.lib.spdy_letkf_destroy(self.bare) == OK
        for o in [self.lt, self.nat, self.diag] + self.dead:
            o.close()
        self.sp.close()


@pytest.fixture(scope="module")
def hs():
    h = Host()
    yield h
    h.close()


def refused(lib, rc, code, text):
    assert rc == code and text in lib.spdy_last_error(), (rc, lib.spdy_last_error())


def test_entry_points_exist_and_are_bound(hs):
    declared, bound = support.declared(), support.fortran_bound()
    for name in NEW:
        assert hasattr(hs.lib, name) and name in hs.s._lib.SIGNATURES and name in declared and name in bound, name
    P, I = ctypes.c_void_p, ctypes.c_int
    sig = hs.s._lib.SIGNATURES
    assert sig[NEW[0]] == sig["spdy_letkf_analyse_grid_dev"] + [P] and sig[NEW[1]] == sig["spdy_ens_letkf_dev"] + [P]
    assert sig[NEW[2]] == sig["spdy_nature_verify_dev"][:-1] + [P, I] and sig[NEW[3]] == sig["spdy_nature_verify_grid_dev"][:-1] + [P, I]
    assert "const int *d_use" in support.declaration(NEW[0]) and support.declaration(NEW[4]) == "spdy_diagnostics *d, int *d_use"
    assert "members_used" in hs.s.letkf.LETKF_FIELDS and hs.s.Diagnostics.use_dev.__doc__


@pytest.mark.parametrize("use", ["null", "pointer"])
def test_analysis_calls_check_in_order(use, hs):
    """each call is given everything that is wrong after the check under test as well, and reports the first"""
    lib, q, l = hs.lib, hs.q, hs.lt.h
    u = None if use == "null" else q
    grid, state = lib.spdy_mask_letkf_analyse_grid_dev, lib.spdy_mask_ens_letkf_dev
    refused(lib, grid(None, *[None] * 10, u), ERR_ARG, b"null analysis object")
    refused(lib, state(None, *[None] * 5, u), ERR_ARG, b"null analysis object")
    refused(lib, grid(hs.dead[0].h, *[None] * 10, u), ERR_STATE, b"has been destroyed")
    refused(lib, state(hs.dead[0].h, *[None] * 5, u), ERR_STATE, b"has been destroyed")
    refused(lib, grid(hs.bare, *[None] * 10, u), ERR_STATE, b"spdy_letkf_set_localization first")
    refused(lib, state(hs.bare, *[None] * 5, u), ERR_STATE, b"spdy_letkf_set_localization first")
    for at in range(10):
        a = [q] * 10
        a[at] = None
        refused(lib, grid(l, *a, u), ERR_ARG, b"null device pointer")
    for at in range(5):
        a = [q] * 5
        a[at] = None
        refused(lib, state(l, *a, u), ERR_ARG, b"null device pointer")
    # the device last: every argument check has passed, with a mask and without one
    refused(lib, grid(l, *[q] * 10, u), ERR_NO_DEVICE, b"host-only plan")
    refused(lib, state(l, *[q] * 5, u), ERR_NO_DEVICE, b"host-only plan")


@pytest.mark.parametrize("use", ["null", "pointer"])
def test_verify_calls_check_in_order(use, hs):
    lib, q, n, l = hs.lib, hs.q, hs.nat.h, hs.lt.h
    u = None if use == "null" else q
    spec, grid = lib.spdy_mask_nature_verify_dev, lib.spdy_mask_nature_verify_grid_dev
    refused(lib, spec(None, None, None, q, q, q, q, u, 9), ERR_ARG, b"null nature run")
    refused(lib, grid(None, 0, None, q, q, q, q, u, 9), ERR_ARG, b"null nature run")
    refused(lib, spec(hs.dead[1].h, None, None, q, q, q, q, u, 9), ERR_STATE, b"has been destroyed")
    refused(lib, grid(hs.dead[1].h, 0, None, q, q, q, q, u, 9), ERR_STATE, b"has been destroyed")
    refused(lib, spec(n, None, None, q, q, q, q, u, 9), ERR_ARG, b"null analysis object")
    refused(lib, spec(n, hs.dead[0].h, None, q, q, q, q, u, 9), ERR_STATE, b"has been destroyed")
    for nmem in (1, 0, 33):
        refused(lib, grid(n, nmem, None, q, q, q, q, u, 9), ERR_ARG, b"nmem=%d outside [2, 32]" % nmem)
    for slot in (-1, 2):
        refused(lib, spec(n, l, None, q, q, q, q, u, slot), ERR_ARG, b"slot=%d outside [0, capacity=2)" % slot)
        refused(lib, grid(n, NMEM, None, q, q, q, q, u, slot), ERR_ARG, b"slot=%d outside [0, capacity=2)" % slot)
    for at in range(5):
        a = [q] * 5
        a[at] = None
        refused(lib, spec(n, l, *a, u, 1), ERR_ARG, b"null device pointer")
        refused(lib, grid(n, NMEM, *a, u, 1), ERR_ARG, b"null device pointer")
    refused(lib, spec(n, l, *[q] * 5, u, 1), ERR_NO_DEVICE, b"host-only plan")
    refused(lib, grid(n, 32, *[q] * 5, u, 0), ERR_NO_DEVICE, b"host-only plan")


def test_guard_mask_and_field_check_in_order(hs):
    lib, q = hs.lib, hs.q
    use = lib.spdy_mask_from_diagnostics_dev
    refused(lib, use(None, None), ERR_ARG, b"null diagnostics object")
    refused(lib, use(hs.dead[2].h, None), ERR_STATE, b"has been destroyed")
    refused(lib, use(hs.diag.h, None), ERR_ARG, b"null mask")
    refused(lib, use(hs.diag.h, q), ERR_NO_DEVICE, b"host-only plan")
    p = ctypes.c_void_p()
    refused(lib, lib.spdy_letkf_field(hs.lt.h, b"members_used", ctypes.byref(p)), ERR_NO_DEVICE, b"host-only plan")
    refused(lib, lib.spdy_letkf_field(hs.lt.h, b"members_unused", ctypes.byref(p)), ERR_ARG, b"unknown analysis field")
    assert not p.value


def test_wrappers_refuse_a_wrong_mask(hs):
    """a mask that is not one int32 flag per member: ValueError before anything is enqueued, as Ensemble.output"""
    import torch
    s, sp = hs.s, hs.sp
    ens = s.Ensemble(sp, NMEM, device="cpu")
    g4 = torch.zeros((NMEM, KX) + sp.grid_shape, dtype=torch.float64)
    gp = torch.zeros((NMEM,) + sp.grid_shape, dtype=torch.float64)
    for bad in ([1, 0], [1] * (NMEM + 1), torch.ones(NMEM, dtype=torch.int64), torch.ones(NMEM + 1, dtype=torch.int32),
                torch.ones(2 * NMEM, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="use must be"):
            hs.lt.analyse_grid(g4, g4, g4, g4, gp, use=bad)
        with pytest.raises(ValueError, match="use must be"):
            hs.lt.analyse_dev(None, None, None, None, None, use=bad)
        with pytest.raises(ValueError, match="use must be"):
            ens.analyse(hs.lt, use=bad)
        with pytest.raises(ValueError, match="use must be"):
            ens.verify(hs.lt, hs.nat, use=bad)
        with pytest.raises(ValueError, match="use must be"):
            hs.nat.verify_grid(g4, g4, g4, g4, gp, use=bad)
    with pytest.raises(ValueError, match="use_dev"):
        hs.diag.use_dev(out=torch.ones(NMEM, dtype=torch.int64))
    # a good mask passes the wrapper and reaches the library, which has no device here
    with pytest.raises(s.SpdyError) as e:
        hs.lt.analyse_grid(g4, g4, g4, g4, gp, use=[1, 0, 1])
    assert e.value.code == ERR_NO_DEVICE
