"""The host-pointer entry points of the C ABI as a table of cases, for tests/test_gpu_host_calls.py and tools/host_call_digest.py:
the nineteen bodies of csrc/spdy_api.hip and csrc/spdy_api_step.hip that stage a call's host arrays (spdy_detail::HostCall), and the
two one-field forms on top of the transform batches.

A case is the call's argument list after the plan, built from seeded inputs (tests/synth.py): I(array) an input, O(array) an
output with the contents the caller hands in, anything else a number passed by value.  Every output that is not also an input is
handed in filled with FILL, so that what a call leaves untouched shows (spdy_grad, spdy_vds, spdy_uvspec upload their outputs
for that; a call of nb = 0 writes nothing).  run_host calls the entry point through the raw library, run_dev its `_dev`
counterpart on device copies of the same arrays."""
import ctypes

import numpy as np

import synth

OK, ERR_ARG, ERR_STATE = 0, -1, -5
FILL = 0.375                  # real and imaginary part of every element an output is handed in with
MAX_BATCH, KX = 16, 8
BATCHES = (0, 1, 3, 16)       # at the default 512 KB threshold 3 and 16 grids straddle it at T30 and T63, 16 spectra between them
NLEVS = (1, 8)                # spdy_hdiff, spdy_step_field (2 nlev <= max_batch)
DT = 2400.0
ROB, WIL = 0.05, 0.53


class I:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)


class O(I):
    pass


def fill(*shape, dtype=np.complex128):
    return O(np.full(shape, FILL * (1 + 1j) if dtype == np.complex128 else FILL, dtype))


class Data:
    """the seeded inputs of one resolution, made once"""

    def __init__(self, sp):
        n, t = MAX_BATCH, sp.trunc
        self.S, self.S2 = synth.spectra(n, t, first=5200, full_rows=True), synth.spectra(n, t, first=5300, full_rows=True)
        self.G, self.G2 = synth.grids(n, sp.ix, sp.il, first=5200), synth.grids(n, sp.ix, sp.il, first=5300)
        self.F = (synth.splitmix64(5400, n * sp.il * 2 * sp.mx) - 0.5).reshape((n,) + sp.four_shape)
        self.D = synth.spectra(n, t, first=5500) * 1e-5
        self.dmp, self.dmp1 = (synth.splitmix64(5600 + i, sp.nx * sp.mx).reshape(sp.spec_shape) for i in (0, 1))
        self.tail = synth.tail_inputs(sp.kx, sp.nx, sp.mx, seed=5700)
        self.spec, self.grid, self.four = sp.spec_shape, sp.grid_shape, sp.four_shape


def mixed_kcos(nb):
    return np.array([1 + (b % 3 == 1) for b in range(nb)], np.int32)


def _step_dev(sp, nlev, j1, dt, eps, wil, field, fdt):
    from speedy_f90_amd.spectral import StepOp
    op = (StepOp * 1)(StepOp(nlev, field.value, fdt.value))
    return sp.lib.spdy_step_fields_dev(sp.h, 1, ctypes.cast(op, ctypes.c_void_p), j1, dt, eps, wil)


# name -> (what nb runs over, args(d, nb), the _dev call given the same arguments with device pointers for the arrays; None: the four
# stage calls have no _dev form -- the test compares their chains with the transforms' _dev forms on the four-kernel path)
CASES = {
    "spdy_spec_to_grid_batch:flag": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), I(np.full(nb, 2, np.int32)), fill(nb, *d.grid, dtype=np.float64)],
                                     lambda sp, nb, s, k, g: sp.lib.spdy_spec_to_grid_dev(sp.h, nb, s, None, 2, g)),
    "spdy_spec_to_grid_batch:mixed": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), I(mixed_kcos(nb)), fill(nb, *d.grid, dtype=np.float64)],
                                      lambda sp, nb, s, k, g: sp.lib.spdy_spec_to_grid_dev(sp.h, nb, s, k, 1, g)),
    "spdy_grid_to_spec_batch": (BATCHES, lambda d, nb: [nb, I(d.G[:nb]), fill(nb, *d.spec)],
                                lambda sp, *a: sp.lib.spdy_grid_to_spec_dev(sp.h, *a)),
    "spdy_spec_to_grid": (None, lambda d, nb: [I(d.S[5]), 2, fill(*d.grid, dtype=np.float64)],
                          lambda sp, s, k, g: sp.lib.spdy_spec_to_grid_dev(sp.h, 1, s, None, k, g)),
    "spdy_grid_to_spec": (None, lambda d, nb: [I(d.G[5]), fill(*d.spec)], lambda sp, g, s: sp.lib.spdy_grid_to_spec_dev(sp.h, 1, g, s)),
    "spdy_legendre_inv": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), fill(nb, *d.four, dtype=np.float64)], None),
    "spdy_legendre_dir": (BATCHES, lambda d, nb: [nb, I(d.F[:nb]), fill(nb, *d.spec)], None),
    "spdy_fourier_inv": (BATCHES, lambda d, nb: [nb, I(d.F[:nb]), 2, fill(nb, *d.grid, dtype=np.float64)], None),
    "spdy_fourier_dir": (BATCHES, lambda d, nb: [nb, I(d.G[:nb]), fill(nb, *d.four, dtype=np.float64)], None),
    "spdy_laplacian": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), fill(nb, *d.spec)], lambda sp, *a: sp.lib.spdy_laplacian_dev(sp.h, *a)),
    "spdy_inverse_laplacian": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), fill(nb, *d.spec)],
                               lambda sp, *a: sp.lib.spdy_inverse_laplacian_dev(sp.h, *a)),
    "spdy_trunct": (BATCHES, lambda d, nb: [nb, O(d.S[:nb])], lambda sp, *a: sp.lib.spdy_trunct_dev(sp.h, *a)),
    "spdy_grad": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), fill(nb, *d.spec), fill(nb, *d.spec)],
                  lambda sp, *a: sp.lib.spdy_grad_dev(sp.h, *a)),
    "spdy_vds": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), I(d.S2[:nb]), fill(nb, *d.spec), fill(nb, *d.spec)],
                 lambda sp, *a: sp.lib.spdy_vds_dev(sp.h, *a)),
    "spdy_uvspec": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), I(d.S2[:nb]), fill(nb, *d.spec), fill(nb, *d.spec)],
                    lambda sp, *a: sp.lib.spdy_uvspec_dev(sp.h, *a)),
    "spdy_uvspec_to_grid": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), I(d.S2[:nb]), fill(nb, *d.grid, dtype=np.float64),
                                                    fill(nb, *d.grid, dtype=np.float64), 2],
                            lambda sp, *a: sp.lib.spdy_uvspec_to_grid_dev(sp.h, *a)),
    "spdy_grad_to_grid": (BATCHES, lambda d, nb: [nb, I(d.S[:nb]), fill(nb, *d.grid, dtype=np.float64), fill(nb, *d.grid, dtype=np.float64), 2],
                          lambda sp, *a: sp.lib.spdy_grad_to_grid_dev(sp.h, *a)),
    "spdy_vdspec": (BATCHES, lambda d, nb: [nb, I(d.G[:nb]), I(d.G2[:nb]), fill(nb, *d.spec), fill(nb, *d.spec), 2],
                    lambda sp, *a: sp.lib.spdy_vdspec_dev(sp.h, *a)),
    "spdy_hdiff": (NLEVS, lambda d, nl: [nl, I(d.S[:nl]), I(d.D[:nl]), I(d.dmp), I(d.dmp1), fill(nl, *d.spec)],
                   lambda sp, *a: sp.lib.spdy_hdiff_dev(sp.h, *a)),
    "spdy_implicit_terms": (None, lambda d, nb: [O(d.tail[0]), O(d.tail[1]), O(d.tail[2])],
                            lambda sp, *a: sp.lib.spdy_implicit_terms_dev(sp.h, *a)),
    "spdy_geopotential": (None, lambda d, nb: [I(d.S[:KX]), I(d.S2[0]), fill(KX, *d.spec)],
                          lambda sp, *a: sp.lib.spdy_geopotential_dev(sp.h, *a)),
    "spdy_step_field": (NLEVS, lambda d, nl: [nl, 2, 2 * DT, ROB, WIL, O(np.stack([d.S[:nl], d.S2[:nl]])), O(d.D[:nl])], _step_dev),
}
STAGES = ("spdy_legendre_inv", "spdy_legendre_dir", "spdy_fourier_inv", "spdy_fourier_dir")
# case -> the array arguments (counted among the arrays) that may be null
OPTIONAL = {"spdy_spec_to_grid_batch:flag": (1,), "spdy_spec_to_grid_batch:mixed": (1,)}
ROUTES = {"device": "0", "default": None}     # route -> $SPDY_HOST_STAGE_KB while the plan allocates its staging (None: unset)


def name_of(case):
    return case.split(":")[0]


def sizes(case):
    """the batch sizes (level counts) of a case; (None,) for a call without one"""
    return CASES[case][0] or (None,)


def plan(tag):
    """the plan of the tests and the digests: kx = 8, max_batch = 16, the implicit tables built, and the staging allocated by a first
    host-pointer call -- $SPDY_HOST_STAGE_KB is read there, so the plan's routes are those of the environment it is made in"""
    import speedy_f90_amd as s
    sp = s.Spectral(tag, kx=KX, max_batch=MAX_BATCH, device=0)
    sp.initialize_implicit(DT)
    sp.trunct(np.zeros(sp.spec_shape, np.complex128))
    return sp


def arguments(case, d, nb):
    """a fresh argument list: the output arrays are the caller's copies"""
    return [O(a.a.copy()) if isinstance(a, O) else a for a in CASES[case][1](d, nb)]


def run_host(sp, case, args, null=None):
    """(return code, the output arrays after the call); null: the index among the array arguments that is passed as a null pointer"""
    ptr, k = [], 0
    for a in args:
        if isinstance(a, I):
            ptr.append(None if k == null else a.a.ctypes.data_as(ctypes.c_void_p))
            k += 1
        else:
            ptr.append(a)
    rc = getattr(sp.lib, name_of(case))(sp.h, *ptr)
    return rc, [a.a for a in args if isinstance(a, O)]


def run_dev(sp, case, args):
    """(return code, the outputs of the _dev counterpart on device copies of the same arrays, as NumPy arrays)"""
    import torch
    sp._sync_stream()
    t = [torch.from_numpy(a.a.copy()).cuda() if isinstance(a, I) else a for a in args]
    rc = CASES[case][2](sp, *[ctypes.c_void_p(x.data_ptr()) if torch.is_tensor(x) else x for x in t])
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x, a in zip(t, args) if isinstance(a, O)]


def round_trip(sp, d):
    """one word: the digests of a one-field spec_to_grid and of the grid_to_spec of its result"""
    g = sp.spec_to_grid(d.S[5], 1)
    return synth.digest(g) + synth.digest(sp.grid_to_spec(g))


if __name__ == "__main__":            # a child process with an environment of its own (SPDY_HOST_SPIN is read once per process)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child = plan("t30")
    print(round_trip(child, Data(child)))
    child.close()
