"""CPU: the ensemble output's interface without a device -- the entry points exist in the library, the header, the loader and the
Fortran binding, and a host-only plan answers their argument checks in the documented order (include/spdy.h, "ensemble output")."""
import ctypes
import re

import numpy as np
import pytest

import speedy_f90_amd as s
import support
from speedy_f90_amd import _lib, spectral

ARG, NO_DEVICE = -1, -3
NEW = ("spdy_ens_output_workspace", "spdy_ens_output_batch_dev")


def test_symbols_in_library_header_loader_and_fortran():
    lib = s.load()
    hdr, f90, bound = support.header(comments=True), support.fortran_binding(), support.fortran_bound()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.match(r"spdy_plan \*plan, int nmem\b", support.declaration(name)), name             # nmem right after the plan
        assert name in bound, name
        assert _lib.SIGNATURES[name][:2] == [ctypes.c_void_p, ctypes.c_int], name
    assert len(_lib.SIGNATURES["spdy_ens_output_batch_dev"]) == 12
    # the struct: six float pointers in the header's order, in the loader and in the Fortran binding
    m = re.search(r"typedef struct \{[^\n]*\n((?:(?!typedef)[^}])*)\}\s*spdy_output_fields;", hdr)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s+\*", body) == ["float", "float"]                                  # nothing but float pointers
    assert tuple(re.findall(r"\*(\w+)", body)) == spectral.OutputFields.NAMES == ("u", "v", "t", "q", "phi", "ps")
    assert ctypes.sizeof(spectral.OutputFields) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert re.search(r"type, bind\(C\) :: spdy_output_fields\s*\n\s*type\(c_ptr\) :: u = c_null_ptr, v = c_null_ptr, t = c_null_ptr, "
                     r"q = c_null_ptr, phi = c_null_ptr, ps = c_null_ptr", f90)
    assert "ensemble output" in hdr
    assert callable(s.Ensemble.output) and callable(s.Ensemble.output_workspace)
    assert callable(s.Spectral.ens_output_batch_dev) and callable(s.Spectral.ens_output_workspace)


def _call(lib, h, nmem, null_in=False, groups=(True, True, True), null_field=None):
    """rc of spdy_ens_output_batch_dev on dummy non-null pointers (no check dereferences a field)"""
    x = np.zeros(4)
    Q = x.ctypes.data_as(ctypes.c_void_p)
    ins = [Q] * 6
    if null_in:
        ins[4] = None
    structs = []
    for g, want in enumerate(groups):
        if not want:
            structs.append(None)
            continue
        f = spectral.OutputFields(*[Q.value] * 6)
        if null_field == g:
            f.phi = None
        structs.append(f)
    return lib.spdy_ens_output_batch_dev(h, nmem, *ins, None, *[None if f is None else ctypes.byref(f) for f in structs])


def test_error_codes_in_documented_order():
    """NULL plan, nmem < 1, max_batch < nmem*(3*kx+1): ARG; a NULL required pointer or no output group: ARG; the host-only plan
    last, NO_DEVICE"""
    lib = s.load()
    kx = 8
    sp = s.Spectral("t30", kx=kx, max_batch=2 * (3 * kx + 1), device=-1)                      # room for two members, not three
    assert _call(lib, None, 1) == ARG and lib.spdy_ens_output_workspace(None, 1) == ARG
    for nmem in (0, -1, 3):                                                                  # 3: max_batch < nmem*(3*kx+1)
        assert _call(lib, sp.h, nmem) == ARG, nmem
        assert lib.spdy_ens_output_workspace(sp.h, nmem) == ARG, nmem
    assert "max_batch" in lib.spdy_last_error().decode()
    assert _call(lib, sp.h, 3, null_in=True) == ARG and "max_batch" in lib.spdy_last_error().decode()   # the batch before the pointers
    assert _call(lib, sp.h, 2, null_in=True) == ARG and "null" in lib.spdy_last_error().decode()
    assert _call(lib, sp.h, 2, groups=(False, False, False)) == ARG                           # no output group
    assert "no output group" in lib.spdy_last_error().decode()
    for g in range(3):                                                                       # inside a given struct all six are required
        assert _call(lib, sp.h, 2, null_field=g) == ARG, g
    for groups in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        assert _call(lib, sp.h, 2, groups=groups) == NO_DEVICE, groups                       # everything right: no device, last
    assert _call(lib, sp.h, 1) == NO_DEVICE and lib.spdy_ens_output_workspace(sp.h, 2) == NO_DEVICE
    with pytest.raises(s.SpdyError):
        sp.ens_output_workspace(2)
    sp.close()
    # no restriction on the level count: the epilogue has a level per block, the transforms take any batch
    big = s.Spectral("t30", kx=20, max_batch=2 * 61, device=-1)
    assert _call(lib, big.h, 2) == NO_DEVICE and _call(lib, big.h, 3) == ARG
    big.close()


def test_output_shapes_and_argument_validation():
    """Ensemble.output's shapes, and its own checks, on CPU tensors over a host-only plan (nothing reaches the library)"""
    import torch
    sp = s.Spectral("t30", kx=5, max_batch=3 * 24, device=-1)
    ens = s.Ensemble(sp, 3, device="cpu")
    sh = ens.output_shapes()
    assert sh["members"]["t"] == (3, 5, 48, 96) and sh["members"]["ps"] == (3, 48, 96)
    assert sh["mean"]["phi"] == sh["spread"]["phi"] == (5, 48, 96) and sh["mean"]["ps"] == sh["spread"]["ps"] == (48, 96)
    assert all(tuple(d) == spectral.OutputFields.NAMES for d in sh.values())
    with pytest.raises(ValueError):
        ens.output(members=False, stats=False)
    with pytest.raises(ValueError):
        ens.output(use=[1, 0])                                                               # not one flag per member
    with pytest.raises(ValueError):
        ens.output(use=torch.ones(3, dtype=torch.int64))
    bad = {"mean": {n: torch.zeros(shape, dtype=torch.float64) for n, shape in sh["mean"].items()}}
    with pytest.raises(ValueError):
        ens.output(members=False, out=bad)
    sp.close()
