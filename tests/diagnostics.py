"""check_diagnostics restated in NumPy: the reference side of tests/test_diagnostics_cpu.py and tests/test_gpu_diagnostics.py.

diagnostics.f90:16-75 as the reference writes it: per level the two sums -Re(inverse_laplacian(x) conjg(x)) over m = 2 .. mx,
n = 1 .. nx (spectral.f90:91-96: inverse_laplacian = -x elm2), accumulated in the reference's order (m outer, n inner), temp =
sqrt(0.5) Re t(1,1,k) with sqrt(0.5) a default real, the range test and the three printed lines.  Pinned to the flang-built
reference by tests/golden/ref_diagnostics.npz (tests/golden/make_golden_diagnostics.py).  Arrays are NumPy C-order views of the
reference's: a spectrum (mx,nx,kx) is [kx, nx, mx], diag(kx,3) is [3, kx]."""
import numpy as np

import dynstep

SQRT_HALF = float(np.sqrt(np.float32(0.5)))            # 0.707106769084930419921875
LIMITS = (500.0, 500.0, 180.0, 320.0)                  # reke, deke, temp low, temp high (diagnostics.f90:61-62)
REKE, DEKE, TEMP_LOW, TEMP_HIGH, NONFINITE = 1, 2, 4, 8, 16
REFERENCE = REKE | DEKE | TEMP_LOW | TEMP_HIGH
STOP = "Model variables out of accepted range"


def terms(x, elm2):
    """[kx, nx, mx - 1]: what each coefficient with m >= 2 adds to the level's sum, as the reference evaluates it"""
    x = np.asarray(x, np.complex128)[..., 1:]
    e = np.asarray(elm2, np.float64).reshape(x.shape[-2], -1)[:, 1:]
    tr, ti = -x.real * e, -x.imag * e                  # inverse_laplacian
    return -(tr * x.real + ti * x.imag)                # -Re(temp conjg(x))


def eddy_energy(x, elm2):
    """[kx]: the terms added one after the other in the reference's loop order"""
    t = terms(x, elm2)
    seq = np.swapaxes(t, -1, -2).reshape(t.shape[0], -1)       # m outer, n inner
    return np.cumsum(seq, axis=1)[:, -1]               # cumsum adds sequentially, left to right


def diag(vor, div, t, elm2):
    """[3, kx]: reke | deke | temp"""
    return np.stack([eddy_energy(vor, elm2), eddy_energy(div, elm2), SQRT_HALF * np.asarray(t)[:, 0, 0].real])


def masks(d, limits=LIMITS):
    """[kx] int: the reference's four strict comparisons per level, and NONFINITE where any of the three numbers is not finite"""
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore"):
        m = (REKE * (d[0] > limits[0]) + DEKE * (d[1] > limits[1]) + TEMP_LOW * (d[2] < limits[2]) + TEMP_HIGH * (d[2] > limits[3]))
    return m.astype(np.int64) + NONFINITE * (~np.isfinite(d).all(axis=0))


def stops(d, limits=LIMITS):
    """whether the reference stops on this row"""
    return bool((masks(d, limits) & REFERENCE).any())


def f8_2(x):
    s = "NaN".rjust(8) if np.isnan(x) else ("Inf" if x > 0 else "-Inf").rjust(8) if np.isinf(x) else "%8.2f" % x
    return s if len(s) == 8 else "*" * 8


def lines(step, d):
    """2001 format(' step =',i6,' reke =', (10f8.2)), 2002 / 2003 format(13x,' deke =', (10f8.2)): past ten values format reversion
    returns to the group (10f8.2), so further records hold up to ten fields and nothing else"""
    d = np.asarray(d, np.float64)
    out = []
    for i, name in enumerate(("reke", "deke", "temp")):
        istep = "%6d" % step
        head = (" step =" + (istep if len(istep) == 6 else "*" * 6) if i == 0 else " " * 13) + " %s =" % name
        f = [f8_2(v) for v in d[i]]
        out.append(head + "".join(f[:10]))
        out.extend("".join(f[j:j + 10]) for j in range(10, len(f), 10))
    return "".join(l + "\n" for l in out)


def state(sp, seed):
    """time level 2 of the seeded model state: vor, div, t [kx, nx, mx], the winds scaled down into the accepted range (the seeded
    state's own reke is of order 1e4)"""
    st = dynstep.state(sp, seed)
    return {n: np.ascontiguousarray(st[n][1]) * f for n, f in (("vor", 1e-2), ("div", 1e-1), ("t", 1.0))}
