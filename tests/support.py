"""What the tests and tools share that belongs to no scheme: the package and its plans, the variant table, arrays on the device,
the bit-for-bit comparison, a cache of plans for a module's fixtures, the `pkg` and `host_plan` fixtures, and the readers of the
binding surface (include/spdy.h, speedy.f90_amd/fortran/spdy_c.f90).  torch is imported inside the functions that need it, so the
CPU tests import this module without a device."""
import contextlib
import os
import re

import numpy as np
import pytest

import synth
from conftest import ROOT, VARIANTS

# the variants the column-physics fixtures are made for (tests/golden/ref_moist.npz and its neighbours), in the order of the test ids
PHYSICS_TAGS = ("t30", "t30k5", "t30k7", "t63k16")


def grid(tag):
    """(ix, il, kx) of a variant of conftest.VARIANTS"""
    _, ix, iy, kx = VARIANTS[tag]
    return ix, 2 * iy, kx


def package():
    """speedy_f90_amd, with libspdy.so built if it is not there yet"""
    import speedy_f90_amd as s
    if not os.path.exists(s.LIB_PATH):
        s.build()
    return s


def plan(tag, max_batch=64, device=0):
    """the plan of the variant tag (device -1: host-only), with the sigma levels of tests/synth.py at kx = 16"""
    import speedy_f90_amd as s
    trunc, _, _, kx = VARIANTS[tag]
    sp = s.Spectral("t%d" % trunc, kx=kx, max_batch=max_batch, device=device)
    if kx == 16:
        sp.set_sigma(synth.SIGMA_L16)
    return sp


def ensemble_plan(tag, nmem):
    """the plan of the variant tag with room for an ensemble of nmem members: 4 kx + 4 fields per member in a step's largest launch"""
    return plan(tag, nmem * (4 * VARIANTS[tag][3] + 4))


def dev(a, dtype=None):
    """a NumPy array as a CUDA tensor (optionally converted to dtype)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def same_bits(a, b):
    """same shape, same dtype and bit for bit the same values, NaN payloads and signs of zero included; integers identical (two
    tensors or two NumPy arrays; nothing is converted)"""
    if _is_torch(a):
        import torch
        if a.shape != b.shape or a.dtype != b.dtype:
            return False
        if not a.dtype.is_floating_point and not a.is_complex():
            return torch.equal(a, b)
        a, b = (torch.view_as_real(x.contiguous()) if x.is_complex() else x.contiguous() for x in (a, b))
        bits = {4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.view(bits), b.view(bits))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@contextlib.contextmanager
def plan_cache(make, plan_of=lambda made: made):
    """get(*key): make(*key), made once per key; on exit every plan made is closed (plan_of picks the plan out of what make returns)"""
    made = {}

    def get(*key):
        if key not in made:
            made[key] = make(*key)
        return made[key]
    try:
        yield get
    finally:
        for v in made.values():
            plan_of(v).close()


@pytest.fixture(scope="module")
def pkg():
    return package()


@pytest.fixture(scope="module")
def host_plan():
    """T30 L8 without a device"""
    package()
    sp = plan("t30", max_batch=4, device=-1)
    yield sp
    sp.close()


# ---------------------------------------------------------------------------------------------------- the binding surface
def header(comments=False):
    """include/spdy.h, without its comments unless they are asked for"""
    with open(os.path.join(ROOT, "include", "spdy.h")) as f:
        text = f.read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared():
    """the spdy_* functions the header declares"""
    return set(re.findall(r"\b(spdy_[a-z0-9_]+)\s*\(", header()))


def declaration(name):
    """the parameter list of `int name(...)` as the header declares it, blanks squeezed; None if it declares no such function"""
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header())
    return None if m is None else re.sub(r"\s+", " ", m.group(1)).strip()


def fortran_binding():
    """speedy.f90_amd/fortran/spdy_c.f90"""
    with open(os.path.join(ROOT, "speedy.f90_amd", "fortran", "spdy_c.f90")) as f:
        return f.read()


def fortran_bound():
    """the C names spdy_c.f90 has a bind(C) interface for"""
    return set(re.findall(r'bind\(C, name="(spdy_[a-z0-9_]+)"\)', fortran_binding()))
