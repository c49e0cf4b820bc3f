"""CPU: the pressure-level output without a device (include/spdy.h, "pressure-level output") -- the NumPy restatement the GPU tests
compare against is held to np.interp; the entry points exist in the library, the header, the loader and the Fortran binding; and a
host-only plan answers their argument checks in the order the header documents, with the text of spdy_last_error."""
import ctypes
import re

import numpy as np
import pytest

import pressurelevels as pl
import speedy_f90_amd as s
import support
from speedy_f90_amd import _lib, spectral

ARG, NO_DEVICE, STATE = -1, -3, -5
NEW = ("spdy_ens_output_pressure_dev", "spdy_ens_output_pressure_grid_dev", "spdy_output_pressure_dev")
FSG8 = [0.025, 0.095, 0.2, 0.34, 0.51, 0.685, 0.835, 0.95]


def test_restatement_against_np_interp():
    """Linear mode on random columns: within 8 eps (max|f| + A max|df|) of np.interp(x, X, f), A = max_k fsg[k+1] / (fsg[k+1] -
    fsg[k]) (np.interp forms slope = df / dX and f + slope * (x - X): a few roundings, each amplified by at most (x - X) / dX <= 1,
    and X itself is rounded); in the two clamped classes bit-equal"""
    r = np.random.default_rng(11)
    eps = np.finfo(np.float64).eps
    for fsg in (FSG8, [0.075, 0.25, 0.5, 0.775, 0.95], [0.25, 0.75], [0.5]):
        kx, ncol = len(fsg), 4000
        A = pl.slope_factor(fsg)
        f = 250.0 + 30.0 * r.standard_normal((1, kx, ncol))
        ps = r.uniform(np.log(0.5), np.log(1.05), (1, ncol))
        plev = list(r.uniform(500.0, 108000.0, 12)) + [1e5 * fsg[0], 1e5 * fsg[-1]]
        y, cls = pl.interpolate(fsg, {"t": f}, ps, plev, "p")
        X, xt = pl.coordinates(fsg, ps, plev, "p")
        ref = np.stack([[np.interp(x, X[0, :, c], f[0, :, c]) for c in range(ncol)] for x in xt])
        got, lo, hi = y["t"][0], cls["lo"][0], cls["hi"][0]
        clamped = lo | hi
        assert clamped.any() and (kx == 1 or (~clamped).any())
        assert np.array_equal(got[clamped], ref[clamped])                                  # the end level's bits
        assert np.array_equal(got[lo], np.broadcast_to(f[0, 0], got.shape)[lo])
        assert np.array_equal(got[hi & ~lo], np.broadcast_to(f[0, -1], got.shape)[hi & ~lo])
        df = float(np.max(np.abs(np.diff(f, axis=1)))) if kx > 1 else 0.0
        bound = 8 * eps * (float(np.max(np.abs(f))) + A * df)
        worst = float(np.max(np.abs(got - ref)))
        print("[plev restatement kx=%d] max error %.3e, bound %.3e, ratio %.3f" % (kx, worst, bound, worst / bound))
        assert worst <= bound
    # log mode is the same rule in another coordinate: exact on a level, and monotone between two
    y, _ = pl.interpolate(FSG8, {"t": np.arange(8.0).reshape(1, 8, 1)}, np.zeros((1, 1)), [1e5 * f for f in FSG8] + [30000.0], "logp")
    assert np.array_equal(y["t"][0, :8, 0], np.arange(8.0)) and 2.0 < y["t"][0, 8, 0] < 3.0


def test_restatement_statistics_and_classes():
    """the sequential two-pass statistics: n = 1 spread +0, n = 0 NaN, a member not in use is absent; a crafted ensemble holds
    every class of target at kx = 2, 5, 8"""
    y = np.array([[1.0, 2.0], [3.0, np.nan], [5.0, 8.0]])
    mean, spread = pl.statistics(y, [1, 0, 1])
    assert np.array_equal(mean, [3.0, 5.0]) and np.allclose(spread, [np.sqrt(8.0), np.sqrt(18.0)])
    mean, spread = pl.statistics(y, [0, 0, 1])
    assert np.array_equal(mean, [5.0, 8.0]) and not spread.any() and not np.signbit(spread).any()
    assert all(np.isnan(a).all() for a in pl.statistics(y, [0, 0, 0]))
    for fsg in ([0.25, 0.75], [0.075, 0.25, 0.5, 0.775, 0.95], FSG8):
        raw = pl.craft(96, 48, len(fsg), 3, 5)
        for coord in pl.COORDS:
            _, cls = pl.interpolate(fsg, pl.values(raw), raw["ps"], pl.levels(fsg, 8), coord)
            assert pl.classes(cls, 3) == pl.every_class(len(fsg), 3), (len(fsg), coord)


def test_symbols_in_library_header_loader_and_fortran():
    lib = s.load()
    hdr, bound = support.header(comments=True), support.fortran_bound()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in bound, name
    ens, grid, one = (support.declaration(n) for n in NEW)
    assert re.match(r"spdy_plan \*plan, int nmem\b", ens) and re.match(r"spdy_plan \*plan, int nmem, const double \*grid\b", grid)
    # the single state: the ensemble call without nmem, d_use and the statistics groups -- its one group as six float pointers
    inputs = "const double *vor, const double *div, const double *t, const double *q, const double *phi, const double *ps"
    levels = "int nlev, const double *plev, int coord"
    groups = "const spdy_output_fields *members, const spdy_output_fields *mean, const spdy_output_fields *spread, float *below"
    assert ens == "spdy_plan *plan, int nmem, %s, const int *d_use, %s, %s" % (inputs, levels, groups)
    assert grid == "spdy_plan *plan, int nmem, const double *grid, const int *d_use, %s, %s" % (levels, groups)
    assert one == "spdy_plan *plan, %s, %s, %s" % (inputs, levels, ", ".join("float *%s_out" % n for n in spectral.OutputFields.NAMES))
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NEW[0]] == [P, I] + [P] * 7 + [I, P, I] + [P] * 4
    assert _lib.SIGNATURES[NEW[1]] == [P, I] + [P] * 2 + [I, P, I] + [P] * 4
    assert _lib.SIGNATURES[NEW[2]] == [P] * 7 + [I, P, I] + [P] * 6
    assert re.search(r"SPDY_MAX_PLEV = 32, SPDY_PLEV_LINEAR_P = 0, SPDY_PLEV_LOG_P = 1", hdr)
    assert spectral.MAX_PLEV == 32 and spectral.PLEV_COORDS == {"p": 0, "logp": 1}
    f90 = support.fortran_binding()
    assert re.search(r"SPDY_MAX_PLEV = 32_c_int, SPDY_PLEV_LINEAR_P = 0_c_int, SPDY_PLEV_LOG_P = 1_c_int", f90)
    assert "pressure-level output" in hdr and hdr.index("pressure-level output") > hdr.index("ensemble output")
    assert callable(s.Ensemble.output_pressure) and callable(s.Ensemble.output_pressure_shapes)
    assert all(callable(getattr(s.Spectral, n[5:])) for n in NEW)


def test_header_documents_the_order_of_the_checks():
    """the order the library is held to below is the one the header states"""
    hdr = re.sub(r"\s*\n \*\s*", " ", support.header(comments=True))
    block = hdr[hdr.index("pressure-level output"):hdr.index("enum { SPDY_MAX_PLEV")]
    order = ["a NULL plan", "nmem < 1", "max_batch < nmem*(3*kx+1)", "nlev outside [1, SPDY_MAX_PLEV]", "a NULL plev",
             "not finite or not > 0", "an unknown coord", "no sigma levels SPDY_ERR_STATE", "a NULL required pointer", "no output group",
             "not 8-byte aligned", "a host-only plan SPDY_ERR_NO_DEVICE last"]
    at = [block.index(text, block.index("Checks, in this order")) for text in order]
    assert at == sorted(at)


class Call:
    """one entry point on dummy non-null pointers (no check dereferences a field); keyword arguments replace the defaults"""

    def __init__(self, lib, which):
        self.lib, self.which = lib, which
        self.x = np.zeros(8)
        self.lev = np.array([50000.0, 85000.0, 20000.0])

    def __call__(self, h, nmem=2, null_in=False, nlev=3, plev="ok", coord=0, groups=(True, True, True), null_field=None, skew=None,
                 below=None):
        base = self.x.ctypes.data
        assert base % 16 == 0
        Q = ctypes.c_void_p(base)
        plev = self.lev if isinstance(plev, str) else plev
        pp = None if plev is None else plev.ctypes.data_as(ctypes.c_void_p)
        structs = []
        for g, want in enumerate(groups):
            f = spectral.OutputFields(*[base] * 6) if want else None
            if want and null_field == g:
                f.phi = None
            if want and skew == g:
                f.t = base + 4
            structs.append(f)
        self.keep = structs
        refs = [None if f is None else ctypes.byref(f) for f in structs]
        tail = (nlev, pp, coord)
        if self.which == "ens":
            ins = [Q] * 6
            if null_in:
                ins[4] = None
            return self.lib.spdy_ens_output_pressure_dev(h, nmem, *ins, None, *tail, *refs, below)
        if self.which == "grid":
            return self.lib.spdy_ens_output_pressure_grid_dev(h, nmem, None if null_in else Q, None, *tail, *refs, below)
        ins = [Q] * 6
        if null_in:
            ins[4] = None
        outs = [base] * 6
        if null_field == 0:
            outs[4] = None
        if skew == 0:
            outs[2] = base + 4
        return self.lib.spdy_output_pressure_dev(h, *ins, *tail, *outs)


@pytest.mark.parametrize("which", ["ens", "grid", "single"])
def test_error_codes_in_documented_order(which):
    """every rejection in the header's order, each with what comes later in the order wrong as well, and the host-only plan last"""
    lib = s.load()
    call = Call(lib, which)
    kx = 8
    sp = s.Spectral("t30", kx=kx, max_batch=2 * (3 * kx + 1), device=-1)                      # room for two members, not three
    nosig = s.Spectral("t30", kx=6, max_batch=2 * 19, device=-1)                              # kx = 6: no sigma levels yet
    text = lambda: lib.spdy_last_error().decode()
    wrong_later = dict(null_in=True, nlev=0, plev=None, coord=7, groups=(False, False, False))
    assert call(None, **wrong_later) == ARG and "null plan" in text()
    if which != "single":
        for nmem in (0, -1):
            assert call(sp.h, nmem=nmem, **wrong_later) == ARG and "nmem=%d < 1" % nmem in text()
    if which == "ens":
        assert call(sp.h, nmem=3, **wrong_later) == ARG and "max_batch" in text()
    if which == "grid":                                                                      # no transform: no max_batch check
        assert call(sp.h, nmem=3) == NO_DEVICE
    later = dict(null_in=True, coord=7, groups=(False, False, False))
    for nlev in (0, -1, 33):
        assert call(sp.h, nlev=nlev, plev=None, **later) == ARG and "nlev=%d outside [1, 32]" % nlev in text()
    assert call(sp.h, plev=None, **later) == ARG and "null plev" in text()
    for l, bad in ((0, 0.0), (1, -500.0), (2, float("nan")), (1, float("inf")), (0, float("-inf"))):
        lev = np.array([50000.0, 85000.0, 20000.0])
        lev[l] = bad
        assert call(sp.h, plev=lev, **later) == ARG and "plev[%d]=" % l in text() and "must be finite and > 0" in text()
    later.pop("coord")
    for coord in (2, -1, 7):
        assert call(sp.h, coord=coord, **later) == ARG and "unknown coord=%d" % coord in text()
    assert call(nosig.h, **later) == STATE and "needs sigma levels" in text()
    assert call(nosig.h, coord=1, **later) == STATE
    assert call(sp.h, null_in=True, groups=(False, False, False)) == ARG and "null device pointer" in text()
    if which != "single":
        assert call(sp.h, groups=(False, False, False), below=call.x.ctypes.data) == ARG and "no output group" in text()
        for g in range(3):                                                                   # inside a given struct all six are required
            assert call(sp.h, null_field=g) == ARG and "null device pointer" in text(), g
            assert call(sp.h, skew=g) == ARG and "8-byte aligned" in text(), g
        assert call(sp.h, below=call.x.ctypes.data + 4) == ARG and "8-byte aligned" in text()
        for groups in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
            for coord in (0, 1):
                assert call(sp.h, groups=groups, coord=coord, below=call.x.ctypes.data) == NO_DEVICE and "host-only plan" in text()
    else:
        assert call(sp.h, null_field=0) == ARG and "null device pointer" in text()
        assert call(sp.h, skew=0) == ARG and "8-byte aligned" in text()
    for coord in (0, 1):
        assert call(sp.h, coord=coord, nlev=1) == NO_DEVICE and "host-only plan" in text()
    sp.close()
    nosig.close()


def test_grid_alignment():
    """the gridded ensemble is read as pairs of doubles: 16-byte aligned, checked with the pointers"""
    lib = s.load()
    sp = s.Spectral("t30", kx=8, max_batch=50, device=-1)
    buf = np.zeros(12)
    off = (16 - buf.ctypes.data % 16) % 16
    lev = np.array([50000.0])
    f = spectral.OutputFields(*[buf.ctypes.data + off] * 6)
    call = lambda ptr: lib.spdy_ens_output_pressure_grid_dev(sp.h, 1, ctypes.c_void_p(ptr), None, 1, lev.ctypes.data_as(ctypes.c_void_p), 0,
                                                             ctypes.byref(f), None, None, None)
    assert call(buf.ctypes.data + off + 8) == ARG and "16-byte aligned" in lib.spdy_last_error().decode()
    assert call(buf.ctypes.data + off) == NO_DEVICE
    sp.close()


def test_output_pressure_shapes_and_argument_validation():
    """Ensemble.output_pressure's shapes, and its own checks, on CPU tensors over a host-only plan (nothing reaches the library)"""
    import torch
    sp = s.Spectral("t30", kx=5, max_batch=3 * 24, device=-1)
    ens = s.Ensemble(sp, 3, device="cpu")
    sh = ens.output_pressure_shapes(4)
    assert sh["members"]["t"] == (3, 4, 48, 96) and sh["members"]["ps"] == (3, 48, 96)
    assert sh["mean"]["phi"] == sh["spread"]["phi"] == (4, 48, 96) and sh["mean"]["ps"] == sh["spread"]["ps"] == (48, 96)
    assert sh["below"] == (4, 48, 96)
    assert all(tuple(sh[g]) == spectral.OutputFields.NAMES for g in ("members", "mean", "spread"))
    lev = [50000.0, 85000.0, 20000.0, 70000.0]
    with pytest.raises(ValueError):
        ens.output_pressure(lev, members=False, stats=False)
    with pytest.raises(ValueError):
        ens.output_pressure(lev, use=[1, 0])                                                 # not one flag per member
    with pytest.raises(ValueError):
        ens.output_pressure(lev, use=torch.ones(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ens.output_pressure([])
    with pytest.raises(ValueError):
        ens.output_pressure(list(range(1, 34)))
    with pytest.raises(ValueError):
        ens.output_pressure(lev, coord="sigma")
    bad = {"mean": {n: torch.zeros(shape, dtype=torch.float64) for n, shape in sh["mean"].items()}}
    with pytest.raises(ValueError):
        ens.output_pressure(lev, members=False, out=bad)
    with pytest.raises(ValueError):
        ens.output_pressure(lev, below=True, out={"below": torch.zeros((3, 48, 96))})
    sp.close()
