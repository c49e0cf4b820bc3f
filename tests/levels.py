"""Level counts outside conftest.VARIANTS, for the tests of the level-dependent step kernels (csrc/spdy_step.hip,
csrc/spdy_api_step.hip): one count per path of the kernels' specialisation by kx, a half-level set for any count, and plans and
oracles built on it.

    kx      grid_tendencies_kernel     spectral_step_kernel    implicit_kernel
    1..7    <8, false>                 <4, false>              ky = kx, one pass
    8       <8, true>                  <4, true>
    9..15   <16, false>                <8, false>
    16      <16, true>                 <8, true>               ky = 16, one pass
    17..21  serial                     five kernels            ky = 16, the level loop strides
    22..32  serial                     five kernels            as above, dynamic LDS above 64 KiB

LEVELS: 1 (kx - 1 = 0 clamps, kxp = 2, a 16-thread block), 2 (the recurrence rows are k = 0 and k = 1), 4 (every row in one wave),
6 (even, no pad column), 9 (first of the 16-bound: the hb = 8 block empty, one live element in the second register block), 12
(middle of that class, even), 15 (one short of full, pad column), 17 (first serial count; the implicit kernel's second pass has
one level), 22 (first count above 64 KiB of LDS), 32 (the maximum: two full passes, 96 KiB)."""
import numpy as np

from conftest import VARIANTS

LEVELS = (1, 2, 4, 6, 9, 12, 15, 17, 22, 32)

_oracles = {}


def sigma(kx):
    """kx + 1 half levels from 0 to 1, thin layers at the top and at the surface, written like the reference's literals
    (float32 values widened to double: synth.SIGMA_L16's convention)."""
    x = np.linspace(0.0, 1.0, kx + 1)
    h = 0.6 * 0.5 * (1.0 - np.cos(np.pi * x)) + 0.4 * x
    h[0], h[-1] = 0.0, 1.0
    return h.astype(np.float32).astype(np.float64)


def plan(trunc_tag, kx, max_batch, device=0):
    """a plan of kx levels on sigma(kx); device = -1: a host plan (tables only)"""
    import speedy_f90_amd as s
    sp = s.Spectral(VARIANTS[trunc_tag][:3], kx=kx, max_batch=max_batch, device=device)
    sp.set_sigma(sigma(kx))
    return sp


def oracle(trunc_tag, kx):
    """the C oracle at kx levels on sigma(kx); one per (resolution, kx) and session"""
    key = (trunc_tag, kx)
    if key not in _oracles:
        from oracle.pyoracle import Oracle, build
        build()
        o = Oracle(*VARIANTS[trunc_tag][:3], kx)
        o.set_sigma(sigma(kx))
        _oracles[key] = o
    return _oracles[key]
