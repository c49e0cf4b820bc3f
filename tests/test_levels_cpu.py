"""CPU: the product's level tables at every level count of tests/levels.py (host plans, device = -1) -- the sigma-derived tables,
the vertical profiles of the orographic correction and, at two time steps, the implicit and diffusion tables, bit for bit against
the oracle's; and the edges of the accepted range."""
import numpy as np
import pytest

import levels
from conftest import VARIANTS
from support import pkg  # noqa: F401


def test_sigma_sets():
    """sigma(kx): kx + 1 strictly increasing float32 values from 0 to 1"""
    for kx in levels.LEVELS:
        h = levels.sigma(kx)
        assert h.shape == (kx + 1,) and h[0] == 0.0 and h[-1] == 1.0
        assert np.all(np.diff(h) > 0) and np.array_equal(h, h.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("kx", levels.LEVELS)
def test_level_tables_match_oracle(kx, pkg):
    sp = pkg.Spectral(VARIANTS["t30"][:3], kx=kx, device=-1)
    with pytest.raises(pkg.SpdyError, match="no sigma levels"):      # the reference has no set at this count (geometry.f90:42-48)
        sp.initialize_implicit(2400.0)
    sp.set_sigma(levels.sigma(kx))
    sp.initialize_implicit(2400.0)
    o = levels.oracle("t30", kx)
    assert np.array_equal(sp.table("hsg"), levels.sigma(kx))
    for n in ("hsg", "dhs", "fsg", "dhsr", "fsgr", "tcorv", "qcorv"):
        a, b = sp.table(n), o.table(n)
        assert a.shape == b.shape == (kx + (n == "hsg"),), n
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), n
    for dt in (1200.0, 4800.0):
        sp.initialize_implicit(dt)
        o.tail_init(dt)
        for n in ("dmp1", "dmp1d", "dmp1s", "tref", "tref1", "tref2", "tref3", "xc", "xd", "xj", "dhsx", "elz"):
            a, b = sp.table(n), o.table(n)
            assert np.all(np.isfinite(a)), (dt, n)
            assert np.array_equal(a, b), (dt, n)
    sp.close()


def test_level_count_range(pkg):
    """1 <= kx <= SPDY_MAX_KX = 32: 33 and 0 are refused"""
    with pytest.raises(pkg.SpdyError) as e:
        pkg.Spectral(VARIANTS["t30"][:3], kx=33, device=-1)
    assert e.value.code == -2                        # SPDY_ERR_UNSUPPORTED
    with pytest.raises(pkg.SpdyError):
        pkg.Spectral(VARIANTS["t30"][:3], kx=0, device=-1)
    pkg.Spectral(VARIANTS["t30"][:3], kx=32, device=-1).close()
