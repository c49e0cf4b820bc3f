"""CPU: check_diagnostics -- the restatement (tests/diagnostics.py) against the flang-built reference (tests/golden/
ref_diagnostics.npz: the two sums, temp bit for bit, the printed lines), its predicate on the limits, spdy_diagnostics_format
against the reference's text and Fortran's format reversion, the error codes on a host-only plan, and the Fortran interfaces."""
import ctypes
import re

import numpy as np
import pytest

import diagnostics as dg
import support
from support import host_plan  # noqa: F401

ARG, NO_DEVICE = -1, -3
NEW = ("create", "destroy", "set_limits", "reset", "check_dev", "status", "read", "field", "format")


def test_restatement_against_the_reference(golden, host_plan):
    g = golden("diagnostics")
    want = g["diag"]
    got = dg.diag(g["vor"], g["div"], g["t"], host_plan.table("elm2"))
    worst = float(np.abs(got[:2] / want[:2] - 1.0).max())
    print("\n[diagnostics restatement vs reference] sums %.1e, reke %s" % (worst, want[0]))
    assert want[0].min() > 1.0 and want[1].min() > 1.0              # a state with eddies on it
    assert worst <= 1e-15
    assert np.array_equal(got[2], want[2])
    assert dg.lines(int(g["istep"]), g["diag_all"]) == str(g["text"])
    assert np.array_equal(g["diag_all"][:, g["levels"]], want)


def test_the_factor_of_temp_is_the_widened_float32(golden):
    g = golden("diagnostics")
    re_t = g["t"][:, 0, 0].real
    assert dg.SQRT_HALF == 0.707106769084930419921875 == float(np.float32(0.5) ** np.float32(0.5))
    assert np.array_equal(g["diag"][2], dg.SQRT_HALF * re_t)
    assert not np.array_equal(g["diag"][2], np.sqrt(0.5) * re_t)    # the double square root gives other bits


@pytest.mark.parametrize("row,bit,up", [(0, dg.REKE, True), (1, dg.DEKE, True), (2, dg.TEMP_LOW, False), (2, dg.TEMP_HIGH, True)])
def test_predicate_is_strict_at_each_limit(row, bit, up):
    lim = dg.LIMITS[{dg.REKE: 0, dg.DEKE: 1, dg.TEMP_LOW: 2, dg.TEMP_HIGH: 3}[bit]]
    d = np.array([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0], [250.0, 260.0, 270.0]])
    assert not dg.stops(d) and (dg.masks(d) == 0).all()
    d[row, 1] = lim                                                 # equal to the limit: no trip
    assert not dg.stops(d) and (dg.masks(d) == 0).all()
    d[row, 1] = np.nextafter(lim, np.inf if up else -np.inf)        # one ulp beyond: this bit at this level, nothing else
    assert dg.stops(d) and list(dg.masks(d)) == [0, bit, 0]
    d[row, 1] = np.nextafter(lim, -np.inf if up else np.inf)        # one ulp inside
    assert not dg.stops(d)


def test_nan_trips_none_of_the_four():
    for row in range(3):
        d = np.array([[10.0, 20.0], [1.0, 2.0], [250.0, 260.0]])
        d[row, 1] = np.nan
        assert not dg.stops(d) and list(dg.masks(d)) == [0, dg.NONFINITE]
    d = np.array([[np.inf, 20.0], [1.0, 2.0], [250.0, 260.0]])
    assert dg.stops(d) and list(dg.masks(d)) == [dg.REKE | dg.NONFINITE, 0]


# kx = 16 by the format-reversion rule: ten fields after the head, the other six as a record of their own, no head, no indent
ROW16 = np.array([np.arange(16) * 1.25, 100.0 + np.arange(16) * 0.5, 200.0 + np.arange(16) * 7.0])
TEXT16 = (" step =    42 reke =    0.00    1.25    2.50    3.75    5.00    6.25    7.50    8.75   10.00   11.25\n"
          "   12.50   13.75   15.00   16.25   17.50   18.75\n"
          "              deke =  100.00  100.50  101.00  101.50  102.00  102.50  103.00  103.50  104.00  104.50\n"
          "  105.00  105.50  106.00  106.50  107.00  107.50\n"
          "              temp =  200.00  207.00  214.00  221.00  228.00  235.00  242.00  249.00  256.00  263.00\n"
          "  270.00  277.00  284.00  291.00  298.00  305.00\n")


def test_format(golden, host_plan):
    import speedy_f90_amd as s
    g = golden("diagnostics")
    lib = host_plan.lib
    assert s.spectral.format_diagnostics(lib, int(g["istep"]), g["diag_all"]) == str(g["text"])
    assert s.spectral.format_diagnostics(lib, 42, ROW16) == TEXT16 == dg.lines(42, ROW16)
    # fields that do not fit are asterisks, as Fortran writes them; so is a step of more than six digits
    odd = np.array([[123456.0, -0.004], [np.nan, np.inf], [-12345.678, 99999.994]])
    assert s.spectral.format_diagnostics(lib, 1234567, odd) == dg.lines(1234567, odd)
    assert "********" in dg.lines(1, odd) and " step =******" in dg.lines(1234567, odd) and "     NaN     Inf" in dg.lines(1, odd)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = lib.spdy_diagnostics_format(16, 42, P(ROW16), None, 0)
    assert n == len(TEXT16)
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.spdy_diagnostics_format(16, 42, P(ROW16), buf, n) == ARG            # no room for the terminator
    assert lib.spdy_diagnostics_format(16, 42, P(ROW16), buf, n + 1) == n and buf.value.decode() == TEXT16
    assert lib.spdy_diagnostics_format(16, 42, None, buf, n + 1) == ARG
    assert lib.spdy_diagnostics_format(0, 42, P(ROW16), buf, n + 1) == ARG


def test_host_only_plan_and_error_codes(host_plan):
    import speedy_f90_amd as s
    sp, lib, h = host_plan, host_plan.lib, ctypes.c_void_p()
    assert lib.spdy_diagnostics_create(None, 4, 0, ctypes.byref(h)) == ARG
    assert lib.spdy_diagnostics_create(sp.h, 4, 0, None) == ARG
    assert lib.spdy_diagnostics_create(sp.h, 0, 0, ctypes.byref(h)) == ARG
    assert lib.spdy_diagnostics_create(sp.h, -1, 0, ctypes.byref(h)) == ARG
    assert lib.spdy_diagnostics_create(sp.h, 4, -1, ctypes.byref(h)) == ARG
    d = s.Diagnostics(sp, capacity=4, first_step=1)                                # create works without a device
    x = np.zeros(8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n, lev = ctypes.c_longlong(), ctypes.c_int()
    p = ctypes.c_void_p()
    for rc in (lib.spdy_diagnostics_check_dev(d.h, P(x), P(x), P(x)),
               lib.spdy_diagnostics_status(d.h, ctypes.byref(n), ctypes.byref(n), ctypes.byref(lev), ctypes.byref(lev), None),
               lib.spdy_diagnostics_read(d.h, 1, 1, P(x)), lib.spdy_diagnostics_reset(d.h, 0), lib.spdy_diagnostics_set_limits(d.h, None),
               lib.spdy_diagnostics_field(d.h, b"history", ctypes.byref(p))):
        assert rc == NO_DEVICE
    for rc in (lib.spdy_diagnostics_check_dev(None, P(x), P(x), P(x)), lib.spdy_diagnostics_check_dev(d.h, None, P(x), P(x)),
               lib.spdy_diagnostics_check_dev(d.h, P(x), None, P(x)), lib.spdy_diagnostics_check_dev(d.h, P(x), P(x), None),
               lib.spdy_diagnostics_status(None, None, None, None, None, None), lib.spdy_diagnostics_read(None, 1, 1, P(x)),
               lib.spdy_diagnostics_read(d.h, 1, 1, None), lib.spdy_diagnostics_read(d.h, 1, 0, P(x)), lib.spdy_diagnostics_reset(None, 0),
               lib.spdy_diagnostics_reset(d.h, -1), lib.spdy_diagnostics_set_limits(None, None),
               lib.spdy_diagnostics_field(None, b"history", ctypes.byref(p)), lib.spdy_diagnostics_field(d.h, None, ctypes.byref(p)),
               lib.spdy_diagnostics_field(d.h, b"history", None), lib.spdy_diagnostics_field(d.h, b"nothing", ctypes.byref(p))):
        assert rc == ARG
    assert lib.spdy_diagnostics_destroy(None) == 0
    with pytest.raises(s.SpdyError) as e:
        d.field("history")
    assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        d.set_limits([1.0, 2.0])
    d.close()
    assert (s.spectral.DIAG_REKE, s.spectral.DIAG_DEKE, s.spectral.DIAG_TEMP_LOW, s.spectral.DIAG_TEMP_HIGH, s.spectral.DIAG_NONFINITE,
            s.spectral.DIAG_REFERENCE) == (dg.REKE, dg.DEKE, dg.TEMP_LOW, dg.TEMP_HIGH, dg.NONFINITE, dg.REFERENCE)


def test_header_mask_bits_and_fortran_interfaces():
    hdr, declared, bound = support.header(comments=True), support.declared(), support.fortran_bound()
    for name, bit in (("REKE", dg.REKE), ("DEKE", dg.DEKE), ("TEMP_LOW", dg.TEMP_LOW), ("TEMP_HIGH", dg.TEMP_HIGH), ("NONFINITE", dg.NONFINITE)):
        assert re.search(r"SPDY_DIAG_%s = %d\b" % (name, bit), hdr), name
    for n in NEW:
        assert "spdy_diagnostics_%s" % n in bound, n
        assert "spdy_diagnostics_%s" % n in declared, n
