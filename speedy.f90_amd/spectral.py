"""Python mirror of the reference's `spectral` module (spectral.f90:8-11) over the C-ABI.

Same public names, argument meaning and result shapes as the Fortran module, plus batched
and device-resident variants.  Arrays are NumPy C-order views of the reference's column-major
arrays (axes reversed):

    grid  vorg(ix,il)          -> float64    [..., il, ix]
    spec  vorm(mx,nx) complex  -> complex128 [..., nx, mx]
    four  (2*mx,il)            -> float64    [..., il, 2*mx]

Leading dimensions are the batch (e.g. the kx levels of a (mx,nx,kx) array).  Host methods
accept/return NumPy arrays; *_dev methods take torch CUDA tensors (device memory stays where
it is; kernels run on torch's current stream unless use_own_stream() was called).
"""
import ctypes

import numpy as np

from ._lib import check, load
from .columns import (MOIST_2D, MOIST_3D, PBL_2D, PBL_3D, RAD_2D, RAD_3D, RAD_SW_2D, SFC_2D, SFC_3, SFC_BOUNDARY,  # noqa: F401
                      SURFACE_DEFAULT, SURFACE_FIELDS, SURFACE_ICE_COUPLING, SURFACE_LAND_COUPLING, SURFACE_SST_ANOMALY,
                      SPPT_FIELDS, SPPT_TABLES, SURFACE_TABLES, ColumnPhysics, ColumnPhysicsOut, DeviceField, MoistOut, PblOut, RadOut,
                      RadSurface, SfcBoundary, SfcOut, Sppt, SurfaceClim, SurfaceModel, _p)
from .columns import (DIAG_DEKE, DIAG_FIELDS, DIAG_NONFINITE, DIAG_REFERENCE, DIAG_REKE, DIAG_TEMP_HIGH, DIAG_TEMP_LOW,  # noqa: F401
                      Diagnostics, DiagnosticsStop, format_diagnostics)

from .letkf import LETKF_FIELDS, LETKF_TABLES, Letkf, Obs  # noqa: F401,E402

RESOLUTIONS = {"t30": (30, 96, 24), "t63": (63, 192, 48)}   # trunc, ix, iy
MAX_PLEV = 32                                               # SPDY_MAX_PLEV
PLEV_COORDS = {"p": 0, "logp": 1}                           # SPDY_PLEV_LINEAR_P, SPDY_PLEV_LOG_P


class SpecSeg(ctypes.Structure):      # spdy_spec_seg (include/spdy.h)
    _fields_ = [("nb", ctypes.c_int), ("d_spec", ctypes.c_void_p)]


class StepOp(ctypes.Structure):       # spdy_step_op
    _fields_ = [("nlev", ctypes.c_int), ("field", ctypes.c_void_p), ("fdt", ctypes.c_void_p)]


class HdiffOp(ctypes.Structure):      # spdy_hdiff_op
    _fields_ = [("nlev", ctypes.c_int), ("field", ctypes.c_void_p), ("fdt_in", ctypes.c_void_p), ("d_dmp", ctypes.c_void_p),
                ("d_dmp1", ctypes.c_void_p), ("fdt_out", ctypes.c_void_p)]


class OutputFields(ctypes.Structure):  # spdy_output_fields
    NAMES = ("u", "v", "t", "q", "phi", "ps")
    _fields_ = [(n, ctypes.c_void_p) for n in NAMES]


class Graph:
    """A captured sequence of device-resident calls (spdy_graph_* in include/spdy.h)."""

    def __init__(self, lib, handle, sp=None):
        self.lib, self.h, self.sp = lib, handle, sp

    def launch(self):
        """Replays on the plan's stream -- after re-pointing it at torch's current stream when the plan follows torch
        (the default), so that the replay is ordered with the surrounding torch ops like every ``*_dev`` call."""
        if self.sp is not None:
            self.sp._sync_stream()
        check(self.lib.spdy_graph_launch(self.h))

    def num_nodes(self):
        """Nodes of the captured graph: one per kernel launch / collective (spdy_graph_num_nodes)."""
        n = ctypes.c_int(0)
        check(self.lib.spdy_graph_num_nodes(self.h, ctypes.byref(n)))
        return n.value

    def close(self):
        if self.h:
            self.lib.spdy_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GraphCapture:
    def __init__(self, sp):
        self.sp, self.graph = sp, Graph(sp.lib, None, sp)

    def __enter__(self):
        check(self.sp.lib.spdy_graph_begin(self.sp.h))
        self.sp._capturing = True
        return self.graph

    def __exit__(self, exc_type, exc, tb):
        h = ctypes.c_void_p()
        self.sp._capturing = False
        rc = self.sp.lib.spdy_graph_end(self.sp.h, ctypes.byref(h))
        if exc_type is None:
            check(rc)
            self.graph.h = h
        elif rc == 0:
            self.sp.lib.spdy_graph_destroy(h)
        return False


class Spectral(ColumnPhysics):
    """One transform plan = the module state `initialize_spectral` builds (spectral.f90:20); its column physics: columns.py."""

    def __init__(self, res="t30", kx=8, max_batch=64, device=0):
        trunc, ix, iy = RESOLUTIONS[res] if isinstance(res, str) else res
        self.lib = load()
        h = ctypes.c_void_p()
        check(self.lib.spdy_plan_create(trunc, ix, iy, kx, max_batch, device, ctypes.byref(h)))
        self.h = h
        self.trunc, self.ix, self.iy, self.il, self.kx = trunc, ix, iy, 2 * iy, kx
        self.nx, self.mx, self.max_batch, self.device = trunc + 2, trunc + 1, max_batch, device
        self.grid_shape, self.spec_shape = (self.il, self.ix), (self.nx, self.mx)
        self.four_shape = (self.il, 2 * self.mx)

    def close(self):
        if getattr(self, "h", None):
            self.lib.spdy_plan_destroy(self.h)
            self.h = None

    __del__ = close

    # ------------------------------------------------------------------ helpers
    def _in(self, a, shape, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape[-len(shape):] != tuple(shape):
            raise ValueError("expected trailing shape %s, got %s" % (shape, a.shape))
        lead = a.shape[:-len(shape)]
        nb = int(np.prod(lead)) if lead else 1
        return a, lead, nb

    def table(self, name):
        n = check(self.lib.spdy_get_table(self.h, name.encode(), None, 0))
        out = np.zeros(n)
        check(self.lib.spdy_get_table(self.h, name.encode(), _p(out), n))
        return out

    @property
    def el2(self):
        """Public table of the reference module (spectral.f90:8)."""
        return self.table("el2").reshape(self.spec_shape)

    # ------------------------------------------------------------------ transforms (host arrays)
    def spec_to_grid(self, vorm, kcos=1):
        """spectral.f90:98 -- kcos: int or per-field sequence."""
        s, lead, nb = self._in(vorm, self.spec_shape, np.complex128)
        g = np.empty(lead + self.grid_shape)
        kc = np.ascontiguousarray(np.broadcast_to(np.asarray(kcos, np.int32), (nb,)))
        check(self.lib.spdy_spec_to_grid_batch(self.h, nb, _p(s), _p(kc), _p(g)))
        return g

    def grid_to_spec(self, vorg):
        """spectral.f90:112"""
        g, lead, nb = self._in(vorg, self.grid_shape, np.float64)
        s = np.empty(lead + self.spec_shape, np.complex128)
        check(self.lib.spdy_grid_to_spec_batch(self.h, nb, _p(g), _p(s)))
        return s

    def legendre_inv(self, s):
        s, lead, nb = self._in(s, self.spec_shape, np.complex128)
        f = np.empty(lead + self.four_shape)
        check(self.lib.spdy_legendre_inv(self.h, nb, _p(s), _p(f)))
        return f

    def legendre_dir(self, f):
        f, lead, nb = self._in(f, self.four_shape, np.float64)
        s = np.empty(lead + self.spec_shape, np.complex128)
        check(self.lib.spdy_legendre_dir(self.h, nb, _p(f), _p(s)))
        return s

    def fourier_inv(self, f, kcos=1):
        f, lead, nb = self._in(f, self.four_shape, np.float64)
        g = np.empty(lead + self.grid_shape)
        check(self.lib.spdy_fourier_inv(self.h, nb, _p(f), int(kcos), _p(g)))
        return g

    def fourier_dir(self, g):
        g, lead, nb = self._in(g, self.grid_shape, np.float64)
        f = np.empty(lead + self.four_shape)
        check(self.lib.spdy_fourier_dir(self.h, nb, _p(g), _p(f)))
        return f

    # ------------------------------------------------------------------ spectral operators
    def laplacian(self, a):
        a, lead, nb = self._in(a, self.spec_shape, np.complex128)
        o = np.empty_like(a)
        check(self.lib.spdy_laplacian(self.h, nb, _p(a), _p(o)))
        return o

    def inverse_laplacian(self, a):
        a, lead, nb = self._in(a, self.spec_shape, np.complex128)
        o = np.empty_like(a)
        check(self.lib.spdy_inverse_laplacian(self.h, nb, _p(a), _p(o)))
        return o

    def trunct(self, a):
        a, lead, nb = self._in(a, self.spec_shape, np.complex128)
        a = a.copy()
        check(self.lib.spdy_trunct(self.h, nb, _p(a)))
        return a

    def grad(self, psi):
        psi, lead, nb = self._in(psi, self.spec_shape, np.complex128)
        dx, dy = np.zeros_like(psi), np.zeros_like(psi)
        check(self.lib.spdy_grad(self.h, nb, _p(psi), _p(dx), _p(dy)))
        return dx, dy

    def vds(self, ucosm, vcosm):
        u, lead, nb = self._in(ucosm, self.spec_shape, np.complex128)
        v, _, _ = self._in(vcosm, self.spec_shape, np.complex128)
        vor, div = np.zeros_like(u), np.zeros_like(u)
        check(self.lib.spdy_vds(self.h, nb, _p(u), _p(v), _p(vor), _p(div)))
        return vor, div

    def uvspec(self, vorm, divm):
        a, lead, nb = self._in(vorm, self.spec_shape, np.complex128)
        b, _, _ = self._in(divm, self.spec_shape, np.complex128)
        u, v = np.zeros_like(a), np.zeros_like(a)
        check(self.lib.spdy_uvspec(self.h, nb, _p(a), _p(b), _p(u), _p(v)))
        return u, v

    def vdspec(self, ug, vg, kcos=2):
        ug, lead, nb = self._in(ug, self.grid_shape, np.float64)
        vg, _, _ = self._in(vg, self.grid_shape, np.float64)
        vor = np.zeros(lead + self.spec_shape, np.complex128)
        div = np.zeros_like(vor)
        check(self.lib.spdy_vdspec(self.h, nb, _p(ug), _p(vg), _p(vor), _p(div), int(kcos)))
        return vor, div

    def uvspec_to_grid(self, vorm, divm, kcos=2):
        """uvspec + spec_to_grid(., kcos) of both results in one call (tendencies.f90:98-100); leading batch dims allowed."""
        vorm, lead, nb = self._in(vorm, self.spec_shape, np.complex128)
        divm, _, _ = self._in(divm, self.spec_shape, np.complex128)
        ug, vg = np.zeros(lead + self.grid_shape), np.zeros(lead + self.grid_shape)
        check(self.lib.spdy_uvspec_to_grid(self.h, nb, _p(vorm), _p(divm), _p(ug), _p(vg), int(kcos)))
        return ug, vg

    def grad_to_grid(self, psi, kcos=2):
        """grad + spec_to_grid(., kcos) of both results in one call (tendencies.f90:121-123)."""
        psi, lead, nb = self._in(psi, self.spec_shape, np.complex128)
        gx, gy = np.zeros(lead + self.grid_shape), np.zeros(lead + self.grid_shape)
        check(self.lib.spdy_grad_to_grid(self.h, nb, _p(psi), _p(gx), _p(gy), int(kcos)))
        return gx, gy

    # ------------------------------------------------------------------ spectral-space tail
    def do_horizontal_diffusion(self, field, fdt_in, dmp, dmp1):
        """horizontal_diffusion.f90:86-105 (2-D or 3-D by the leading dimension)."""
        field, lead, nlev = self._in(field, self.spec_shape, np.complex128)
        fdt_in, _, _ = self._in(fdt_in, self.spec_shape, np.complex128)
        dmp = np.ascontiguousarray(dmp, np.float64)
        dmp1 = np.ascontiguousarray(dmp1, np.float64)
        out = np.empty_like(field)
        check(self.lib.spdy_hdiff(self.h, nlev, _p(field), _p(fdt_in), _p(dmp), _p(dmp1), _p(out)))
        return out

    def initialize_implicit(self, dt):
        """implicit.f90:36"""
        check(self.lib.spdy_implicit_init(self.h, float(dt)))

    def set_sigma(self, hsg):
        """Half levels hsg[kx+1] for a level count the reference defines no set for (geometry.f90:42-48)."""
        hsg = np.ascontiguousarray(hsg, np.float64)
        if hsg.shape != (self.kx + 1,):
            raise ValueError("hsg must have kx+1 entries")
        check(self.lib.spdy_plan_set_sigma(self.h, _p(hsg)))

    def get_geopotential(self, t, phis):
        """geopotential.f90:33 -- t [kx,nx,mx], phis [nx,mx] -> phi [kx,nx,mx]."""
        t = np.ascontiguousarray(t, np.complex128); phis = np.ascontiguousarray(phis, np.complex128)
        if t.shape != (self.kx,) + self.spec_shape or phis.shape != self.spec_shape:
            raise ValueError("get_geopotential expects (kx,nx,mx), (nx,mx)")
        phi = np.empty_like(t)
        check(self.lib.spdy_geopotential(self.h, _p(t), _p(phis), _p(phi)))
        return phi

    def step_field(self, j1, dt, eps, wil, field, fdt):
        """time_stepping.f90:121-167 step_field_2d/3d -- field [2,nlev,nx,mx] (or [2,nx,mx]), fdt [nlev,nx,mx] (or
        [nx,mx]); returns the updated copies (field, fdt)."""
        f = np.array(field, np.complex128, order="C"); d = np.array(fdt, np.complex128, order="C")
        nlev = 1 if d.ndim == 2 else d.shape[0]
        check(self.lib.spdy_step_field(self.h, nlev, int(j1), float(dt), float(eps), float(wil), _p(f), _p(d)))
        return f, d

    def implicit_terms(self, divdt, tdt, psdt):
        """implicit.f90:168 (returns the updated copies)."""
        d = np.array(divdt, np.complex128, order="C")
        t = np.array(tdt, np.complex128, order="C")
        p = np.array(psdt, np.complex128, order="C")
        if d.shape != (self.kx,) + self.spec_shape or t.shape != d.shape or p.shape != self.spec_shape:
            raise ValueError("implicit_terms expects (kx,nx,mx),(kx,nx,mx),(nx,mx)")
        check(self.lib.spdy_implicit_terms(self.h, _p(d), _p(t), _p(p)))
        return d, t, p

    # ------------------------------------------------------------------ device-resident batch (torch tensors)
    # Stream policy of the device-resident (`*_dev`) methods.  Default: follow torch -- before every call the plan is
    # switched to torch's current stream, so kernels are ordered with the torch ops that produce/consume the tensors
    # (torch's legacy default stream maps to the plan's own blocking stream, which HIP orders against the default
    # stream).  use_own_stream(): the plan keeps its own stream (bench.py, graph replay loops); the caller synchronises.
    def use_torch_stream(self):
        self._follow = True
        self._sync_stream()

    def use_own_stream(self):
        self._follow = False
        self._cur_stream = 0
        check(self.lib.spdy_plan_set_stream(self.h, None))

    def _sync_stream(self):
        # (while a capture is open the plan's stream is pinned: spdy_plan_set_stream would fail with SPDY_ERR_STATE)
        # (a closed plan has no stream: the call that follows reports what it was asked on)
        if not getattr(self, "_follow", True) or getattr(self, "_capturing", False) or not self.h:
            return
        import torch
        h = torch.cuda.current_stream().cuda_stream
        if h != getattr(self, "_cur_stream", 0):
            check(self.lib.spdy_plan_set_stream(self.h, ctypes.c_void_p(h) if h else None))
            self._cur_stream = h

    KERNEL_KINDS = ("legendre_inv", "fourier_inv", "fourier_dir", "legendre_dir", "s2g_fused", "g2s_fused")

    def set_fused(self, mode):
        """1 / -1 (default) = fused single-pass kernels (T30, T63) at every batch size, 0 = four-kernel path."""
        check(self.lib.spdy_plan_set_fused(self.h, int(mode)))

    def set_option(self, name, value):
        """Launch-policy switch of this plan (spdy_plan_set_option): "t30_part", "t30_split", "t63_split", "t63_stage",
        "t63_derive" (0 / 1), "t63_np2_from", "wt_min_mb", "physics_fused", "ens_member_qcorh" (0 / 1)."""
        check(self.lib.spdy_plan_set_option(self.h, name.encode(), int(value)))

    def wave_placement(self):
        """(SIMD of waves 0..7 of workgroup 0, number of workgroups that violate the round-robin placement the T63 kernels'
        role assignment relies on) -- spdy_wave_placement."""
        simd, bad = (ctypes.c_int * 8)(), ctypes.c_int(0)
        check(self.lib.spdy_wave_placement(self.h, simd, ctypes.byref(bad)))
        return list(simd), bad.value

    def set_profiling(self, on=True):
        check(self.lib.spdy_plan_set_profiling(self.h, 1 if on else 0))

    def get_profile(self):
        """{kernel kind: (total ms, launches)} measured with HIP events on the launch stream."""
        ms = (ctypes.c_double * 6)()
        cnt = (ctypes.c_int * 6)()
        check(self.lib.spdy_plan_get_profile(self.h, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNEL_KINDS)}

    def synchronize(self):
        check(self.lib.spdy_plan_synchronize(self.h))

    def graph_capture(self):
        self._sync_stream()
        return self._graph_capture()

    def _graph_capture(self):
        """Context manager: record the ``*_dev`` calls made inside it (nothing runs) and return a
        :class:`Graph` whose ``launch()`` replays them as one HIP graph launch on the plan's stream::

            with sp.graph_capture() as g:
                sp.spec_to_grid_dev(spec, grid); sp.grid_to_spec_dev(grid, spec2)
            g.launch(); sp.synchronize()

        The plan must be on its own stream (or another non-default one), not torch's legacy default stream."""
        return _GraphCapture(self)

    @staticmethod
    def _dp(t):
        """device pointer of a tensor (or DeviceField); None stays None (an optional argument that is not given)"""
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def spec_to_grid_dev(self, d_spec, d_grid, kcos=1, d_kcos=None):
        """d_spec: [nb, nx, mx] complex128 (or [nb,nx,mx,2] float64) CUDA tensor; d_grid: [nb, il, ix] float64."""
        self._sync_stream()
        nb = d_grid.shape[0]
        check(self.lib.spdy_spec_to_grid_dev(self.h, nb, self._dp(d_spec), self._dp(d_kcos), int(kcos), self._dp(d_grid)))

    def grid_to_spec_dev(self, d_grid, d_spec):
        self._sync_stream()
        nb = d_grid.shape[0]
        check(self.lib.spdy_grid_to_spec_dev(self.h, nb, self._dp(d_grid), self._dp(d_spec)))

    def uvspec_dev(self, vor, div, u, v):
        self._sync_stream()
        check(self.lib.spdy_uvspec_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(u), self._dp(v)))

    def vdspec_dev(self, ug, vg, vor, div, kcos=2):
        self._sync_stream()
        check(self.lib.spdy_vdspec_dev(self.h, ug.shape[0], self._dp(ug), self._dp(vg), self._dp(vor), self._dp(div), int(kcos)))

    def uvspec_to_grid_dev(self, vor, div, ug, vg, kcos=2):
        """uvspec followed by spec_to_grid(., kcos) of both results (tendencies.f90:98-100), one pass at T30."""
        self._sync_stream()
        check(self.lib.spdy_uvspec_to_grid_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg), int(kcos)))

    def grad_to_grid_dev(self, psi, gx, gy, kcos=2):
        """grad followed by spec_to_grid(., kcos) of both results (tendencies.f90:121-123), one pass at T30."""
        self._sync_stream()
        check(self.lib.spdy_grad_to_grid_dev(self.h, psi.shape[0], self._dp(psi), self._dp(gx), self._dp(gy), int(kcos)))

    def inverse_batch_dev(self, vor, div, ug, vg, spec, grid, kcos_pairs=2, kcos=1, d_kcos=None):
        """uvspec + spec_to_grid(., kcos_pairs) of the (vor, div) pairs and spec_to_grid of `spec` in one launch."""
        self._sync_stream()
        check(self.lib.spdy_inverse_batch_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg), int(kcos_pairs),
                                              spec.shape[0], self._dp(spec), self._dp(d_kcos), int(kcos), self._dp(grid)))

    def inverse_batch_grad_dev(self, vor, div, ug, vg, spec, grid, psi, gx, gy, kcos_pairs=2, kcos=1, d_kcos=None, kcos_grad=2):
        """inverse_batch_dev + grad_to_grid_dev(psi -> gx, gy): everything a step transforms to the grid, one fused launch at T63."""
        self._sync_stream()
        check(self.lib.spdy_inverse_batch_grad_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg),
                                                   int(kcos_pairs), spec.shape[0], self._dp(spec), self._dp(d_kcos), int(kcos), self._dp(grid),
                                                   psi.shape[0], self._dp(psi), self._dp(gx), self._dp(gy), int(kcos_grad)))

    def inverse_batch_segs_dev(self, vor, div, ug, vg, specs, grid, psi=None, gx=None, gy=None, kcos_pairs=2, kcos=1, d_kcos=None, kcos_grad=2):
        """inverse_batch_grad_dev with the plain spectra in up to four separate arrays `specs` (tendencies.f90:89-101 reads
        vor, div, t, tr from four prognostic arrays); their grids are the one stack `grid`.  psi / gx / gy optional."""
        self._sync_stream()
        segs = (SpecSeg * len(specs))(*[SpecSeg(int(x.shape[0]), self._dp(x)) for x in specs])
        ngrad = 0 if psi is None else psi.shape[0]
        check(self.lib.spdy_inverse_batch_segs_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg),
                                                   int(kcos_pairs), len(specs), ctypes.cast(segs, ctypes.c_void_p),
                                                   self._dp(d_kcos), int(kcos), self._dp(grid), ngrad, self._dp(psi if ngrad else None),
                                                   self._dp(gx if ngrad else None), self._dp(gy if ngrad else None), int(kcos_grad)))

    def direct_batch_dev(self, ug, vg, vor, div, grid, spec, kcos=2):
        """vdspec of the (ug, vg) pairs and grid_to_spec of `grid` in one launch (a model step's direct batch)."""
        self._sync_stream()
        check(self.lib.spdy_direct_batch_dev(self.h, ug.shape[0], self._dp(ug), self._dp(vg), self._dp(vor), self._dp(div), int(kcos),
                                             grid.shape[0], self._dp(grid), self._dp(spec)))

    def implicit_terms_dev(self, divdt, tdt, psdt):
        self._sync_stream()
        check(self.lib.spdy_implicit_terms_dev(self.h, self._dp(divdt), self._dp(tdt), self._dp(psdt)))

    def _members(self, name, nmem, *args):
        """The step call spdy_<name>(plan, ...) or, with a member count, its ensemble form spdy_ens_<name>(plan, nmem, ...); args:
        tensors (or None), and numbers already cast."""
        self._sync_stream()
        fn, lead = (getattr(self.lib, "spdy_" + name), ()) if nmem is None else (getattr(self.lib, "spdy_ens_" + name), (int(nmem),))
        check(fn(self.h, *lead, *[x if isinstance(x, (int, float)) else self._dp(x) for x in args]))

    def _spectral_step(self, name, nmem, lead, fields, sdrag, j1, dt, eps, wil, phi):
        self._members(name, nmem, *lead, *fields, float(sdrag), int(j1), float(dt), float(eps), float(wil), phi)

    def grid_tendencies_dev(self, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out):
        """tendencies.f90:105-197 on the gridded prognostics; outputs are the operands of one direct_batch_dev launch."""
        self._members("grid_tendencies_dev", None, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out)

    def tendency_combine_dev(self, pdiv, pspec):
        """In place on the direct batch's outputs: divdt -= laplacian(KE), tdt += ttend, trdt += trtend, psdt(1,1) = 0."""
        self._sync_stream()
        check(self.lib.spdy_tendency_combine_dev(self.h, self._dp(pdiv), self._dp(pspec)))

    def spectral_step_dev(self, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag, j1, dt, eps, wil, phi):
        """Everything after the direct batch in one launch: tendency_combine, spectral_tendencies, implicit_terms, hdiff_step
        and step_fields of ps, vor, div, t, tr (prognostics [2,kx,nx,mx] / ps [2,nx,mx], both time levels)."""
        self._spectral_step("spectral_step_dev", None, (), (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh), sdrag, j1, dt,
                            eps, wil, phi)

    def direct_batch_spectral_step_dev(self, ug, vg, grid, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag, j1, dt,
                                       eps, wil, phi, kcos=2):
        """direct_batch_dev(ug, vg [3kx] -> pvor, pdiv; grid [3kx+1] -> pspec) + spectral_step_dev as one call (at T63 vds is
        applied where the spectral step reads the pairs' spectra: one launch less)."""
        self._spectral_step("direct_batch_spectral_step_dev", None, (ug, vg, grid, int(kcos)),
                            (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh), sdrag, j1, dt, eps, wil, phi)

    # ------------------------------------------------------------------ ensemble time step (layout: ensemble.py)
    def ens_grid_tendencies_dev(self, nmem, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out):
        """grid_tendencies_dev for nmem members in one launch: inputs (nmem, kx) grids each, px, py (nmem); outputs group-major,
        u_out, v_out (3, nmem, kx), plain_out (3, nmem, kx) followed by the nmem level-free fields."""
        self._members("grid_tendencies_dev", nmem, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out)

    def ens_spectral_step_dev(self, nmem, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag, j1, dt, eps, wil, phi):
        """spectral_step_dev for nmem members in one launch: prognostics (2, nmem, kx, nx, mx) / ps (2, nmem, nx, mx), phi
        (nmem, kx, nx, mx), pvor, pdiv, pspec group-major; phis, tcorh, qcorh are shared."""
        self._spectral_step("spectral_step_dev", nmem, (), (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh), sdrag, j1, dt,
                            eps, wil, phi)

    def ens_direct_batch_spectral_step_dev(self, nmem, ug, vg, grid, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag,
                                           j1, dt, eps, wil, phi, kcos=2):
        """direct_batch_spectral_step_dev for nmem members: 3*nmem*kx pairs and 3*nmem*kx + nmem plain fields through one
        direct batch, then ens_spectral_step_dev."""
        self._spectral_step("direct_batch_spectral_step_dev", nmem, (ug, vg, grid, int(kcos)),
                            (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh), sdrag, j1, dt, eps, wil, phi)

    def ens_geopotential_dev(self, nmem, t, phis, phi):
        """geopotential_dev for nmem members: t, phi (nmem, kx, nx, mx), phis shared"""
        self._members("geopotential_dev", nmem, t, phis, phi)

    def output_batch_dev(self, vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out):
        """input_output.f90:184-206 on device-resident state: complex128 [kx,nx,mx] (ps [nx,mx]) in, float32 [kx,il,ix]
        (ps_out [il,ix]) out."""
        self._sync_stream()
        args = (vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out)
        check(self.lib.spdy_output_batch_dev(self.h, *[self._dp(x) for x in args]))

    # ------------------------------------------------------------------ ensemble output (include/spdy.h, "ensemble output")
    def ens_output_workspace(self, nmem):
        """before a capture that contains ens_output_batch_dev"""
        check(self.lib.spdy_ens_output_workspace(self.h, int(nmem)))

    def ens_output_batch_dev(self, nmem, vor, div, t, q, phi, ps, members=None, mean=None, spread=None, use=None):
        """output_batch_dev for the nmem members of an ensemble, and the ensemble mean and spread: time level 1 of the ensemble in,
        complex128 (nmem, kx, nx, mx) (ps (nmem, nx, mx)).  members, mean, spread: None (not wanted) or a dict u, v, t, q, phi, ps
        of float32 tensors -- members (nmem, kx, il, ix), ps (nmem, il, ix); mean and spread (kx, il, ix), ps (il, ix).  use: None
        (all members) or an int32 device tensor of nmem entries, non-zero = the member enters the statistics."""
        self._sync_stream()
        groups = [None if g is None else OutputFields(*[g[n].data_ptr() for n in OutputFields.NAMES]) for g in (members, mean, spread)]
        check(self.lib.spdy_ens_output_batch_dev(self.h, int(nmem), *[self._dp(x) for x in (vor, div, t, q, phi, ps, use)],
                                                 *[None if g is None else ctypes.byref(g) for g in groups]))

    # ------------------------------------------------------------------ pressure-level output (include/spdy.h, "pressure-level output")
    @staticmethod
    def _plev(plev, coord):
        """(nlev, the host array of pressures in Pa and its pointer, the C value of coord): coord "p" (linear in p) or "logp"""
        if coord not in PLEV_COORDS:
            raise ValueError("coord must be one of %s" % (sorted(PLEV_COORDS),))
        p = np.ascontiguousarray(np.atleast_1d(plev), np.float64)
        if p.ndim != 1:
            raise ValueError("plev must be a sequence of pressures in Pa")
        return p.size, p, p.ctypes.data_as(ctypes.c_void_p), PLEV_COORDS[coord]

    @staticmethod
    def _groups(*groups):
        structs = [None if g is None else OutputFields(*[g[n].data_ptr() for n in OutputFields.NAMES]) for g in groups]
        return structs, [None if g is None else ctypes.byref(g) for g in structs]

    def ens_output_pressure_dev(self, nmem, vor, div, t, q, phi, ps, plev, coord="p", members=None, mean=None, spread=None, below=None,
                                use=None):
        """ens_output_batch_dev on pressure levels: plev, a host sequence of nlev pressures in Pa (read now: a captured call keeps
        its values); coord "p" (linear in p, the reference script's) or "logp".  members: u .. phi (nmem, nlev, il, ix), ps (nmem,
        il, ix); mean and spread: (nlev, il, ix), ps (il, ix); below: None or a float32 tensor (nlev, il, ix), the number of members
        in use whose lowest model level lies above the level."""
        nlev, keep, pp, cc = self._plev(plev, coord)
        self._sync_stream()
        structs, refs = self._groups(members, mean, spread)
        check(self.lib.spdy_ens_output_pressure_dev(self.h, int(nmem), *[self._dp(x) for x in (vor, div, t, q, phi, ps, use)], nlev, pp, cc,
                                                    *refs, self._dp(below)))

    def ens_output_pressure_grid_dev(self, nmem, grid, plev, coord="p", members=None, mean=None, spread=None, below=None, use=None):
        """ens_output_pressure_dev's kernel alone on a gridded ensemble: grid, float64, the (5 kx + 1) nmem grids u | v | t | q | phi
        (nmem, kx, il, ix) each | ps (nmem, il, ix) back to back, the model's raw values (q in g/kg, phi in m2/s2, ps as log(p/p0))"""
        nlev, keep, pp, cc = self._plev(plev, coord)
        self._sync_stream()
        structs, refs = self._groups(members, mean, spread)
        check(self.lib.spdy_ens_output_pressure_grid_dev(self.h, int(nmem), self._dp(grid), self._dp(use), nlev, pp, cc, *refs,
                                                         self._dp(below)))

    def output_pressure_dev(self, vor, div, t, q, phi, ps, plev, coord, u_out, v_out, t_out, q_out, phi_out, ps_out):
        """output_batch_dev on pressure levels, the one-member case of ens_output_pressure_dev: float32 [nlev,il,ix] (ps_out
        [il,ix]) out"""
        nlev, keep, pp, cc = self._plev(plev, coord)
        self._sync_stream()
        args = (vor, div, t, q, phi, ps)
        outs = (u_out, v_out, t_out, q_out, phi_out, ps_out)
        check(self.lib.spdy_output_pressure_dev(self.h, *[self._dp(x) for x in args], nlev, pp, cc, *[self._dp(x) for x in outs]))

    def geopotential_dev(self, t, phis, phi):
        self._members("geopotential_dev", None, t, phis, phi)

    def spectral_tendencies_dev(self, div, t, ps, phis, divdt, tdt, psdt, phi):
        """tendencies.f90:242-293 -- div, t, ps: time level j2 of the prognostics; divdt, tdt, psdt in place; phi out."""
        self._sync_stream()
        check(self.lib.spdy_spectral_tendencies_dev(self.h, *[self._dp(x) for x in (div, t, ps, phis, divdt, tdt, psdt, phi)]))

    def hdiff_step_dev(self, vor, div, t, tr, tcorh, qcorh, sdrag, vordt, divdt, tdt, trdt):
        """The diffusion block of step() (time_stepping.f90:62-96) in one launch; tendencies in place."""
        self._sync_stream()
        dp = self._dp
        check(self.lib.spdy_hdiff_step_dev(self.h, dp(vor), dp(div), dp(t), dp(tr), dp(tcorh), dp(qcorh), float(sdrag),
                                           dp(vordt), dp(divdt), dp(tdt), dp(trdt)))

    def step_fields_dev(self, pairs, j1, dt, eps, wil):
        """step_field_2d/3d for several prognostic arrays in one launch: pairs = [(field [2,nlev,nx,mx], fdt [nlev,nx,mx]), ...]."""
        self._sync_stream()
        arr = (StepOp * len(pairs))()
        for o, (f, d) in zip(arr, pairs):
            nlev = 1 if d.dim() == 2 else d.shape[0]
            assert f.numel() == 2 * d.numel()
            o.nlev, o.field, o.fdt = nlev, f.data_ptr(), d.data_ptr()
        check(self.lib.spdy_step_fields_dev(self.h, len(pairs), ctypes.cast(arr, ctypes.c_void_p), int(j1), float(dt), float(eps), float(wil)))

    def hdiff_multi_dev(self, ops):
        """ops: up to 8 tuples (field, fdt_in, dmp_name, dmp1_name, out) -- the diffusion calls of one time step
        (time_stepping.f90:63-96) in one launch."""
        self._sync_stream()
        arr = (HdiffOp * len(ops))()
        for o, (field, fdt_in, dmp_name, dmp1_name, out) in zip(arr, ops):
            o.nlev, o.field, o.fdt_in, o.fdt_out = field.shape[0], field.data_ptr(), fdt_in.data_ptr(), out.data_ptr()
            o.d_dmp, o.d_dmp1 = self._device_table(dmp_name).value, self._device_table(dmp1_name).value
        check(self.lib.spdy_hdiff_multi_dev(self.h, len(ops), ctypes.cast(arr, ctypes.c_void_p)))

    def _device_table(self, name):
        """Device pointer of a damping table of the plan (spdy_device_table)."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_device_table(self.h, name.encode(), ctypes.byref(p)))
        return p

    def hdiff_dev(self, field, fdt_in, dmp_name, dmp1_name, out):
        self._sync_stream()
        check(self.lib.spdy_hdiff_dev(self.h, field.shape[0], self._dp(field), self._dp(fdt_in), self._device_table(dmp_name),
                                      self._device_table(dmp1_name), self._dp(out)))
