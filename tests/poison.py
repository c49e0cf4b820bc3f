"""Poison for the isolation tests (test_gpu_isolation.py): what goes into one field or member of a batch to show that nothing of
it reaches the fields beside it.

Kinds, each in place on ONE field (a device tensor or a NumPy array; complex spectra [nx, mx], real grids or Fourier rows [il, .]):
    "nan"    every entry a quiet NaN
    "inf"    every entry infinite with both signs present: +inf in the real part and -inf in the imaginary part of a complex field;
             a real field alternates +inf / -inf along its last axis
    "1e300"  every entry the finite value 1e300 (a neighbour's bits change if it is added to them and taken away again, where a NaN
             would have to be multiplied or added to show)
    "entry"  an ordinary field with ONE bad entry: +inf at coefficient (n, m') = (1, 1) of a spectrum, NaN at point (il / 2, 3) of a
             real field

reached(): whether the poison shows in an output the reference computes from the poisoned input.  NaN and inf give a non-finite
output.  1e300 does NOT overflow a transform: an output is a sum of fewer than 2e4 products of an input with table entries of
magnitude below 1e2 (Legendre functions, twiddles, quadrature weights; the operators' factors reach the earth's radius, 6.4e6, so
there it may), and 1e300 * 2e4 * 1e2 is below the largest double, 1.8e308.  So for that kind the poison counts as having reached an
output that is non-finite OR whose magnitude is at least 1e290 -- 280 decades above anything the ordinary inputs give.  (And
where an operator makes two outputs of it, in one of the two: the field is zonally constant, so the reference's divergence of
such a u, or vorticity of such a v, is an exact zero times it.)
"""
import numpy as np

KINDS = ("nan", "inf", "1e300", "entry")
HUGE = 1e290


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def poison(field, kind):
    """One field, in place."""
    assert kind in KINDS, kind
    cplx = field.is_complex() if _is_torch(field) else np.iscomplexobj(field)
    nan, inf = float("nan"), float("inf")
    if kind == "nan":
        field[...] = complex(nan, nan) if cplx else nan
    elif kind == "1e300":
        field[...] = complex(1e300, 1e300) if cplx else 1e300
    elif kind == "inf":
        if cplx:
            field[...] = complex(inf, -inf)
        else:
            field[..., 0::2] = inf
            field[..., 1::2] = -inf
    elif cplx:
        field[1, 1] = complex(inf, 0.0)
    else:
        field[field.shape[0] // 2, 3] = nan
    return field


def _real(x):
    if _is_torch(x):
        import torch
        return torch.view_as_real(x.contiguous()) if x.is_complex() else x
    x = np.ascontiguousarray(x)
    return x.view(np.float64) if np.iscomplexobj(x) else x


def nonfinite(x):
    """at least one NaN or infinity in x"""
    r = _real(x)
    if _is_torch(r):
        import torch
        return not bool(torch.isfinite(r).all())
    return not bool(np.isfinite(r).all())


def reached(x, kind):
    """the poison of `kind` shows in the output field(s) x (see the module's text for "1e300")"""
    if nonfinite(x):
        return True
    if kind != "1e300":
        return False
    r = _real(x)
    return float(r.abs().max() if _is_torch(r) else np.abs(r).max()) >= HUGE


def dead_mask(nx, mx, trunc):
    """[nx, mx] True where l = n + m' > trunc + 1: the entries the inverse transform never reads (legendre.f90:93)"""
    return np.add.outer(np.arange(nx), np.arange(mx)) > trunc + 1
