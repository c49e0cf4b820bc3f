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
import weakref

import numpy as np

from ._lib import check, load

RESOLUTIONS = {"t30": (30, 96, 24), "t63": (63, 192, 48)}   # trunc, ix, iy


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _out_struct(cls, out):
    """An optional-output struct (MoistOut, RadOut) holding the device pointers of the dict `out` (name -> tensor or None)."""
    o = cls()
    fields = [f[0] for f in cls._fields_]
    for name, t in (out or {}).items():
        if name not in fields:
            raise ValueError("unknown %s field %r" % (cls.__name__, name))
        if t is not None:
            setattr(o, name, t.data_ptr())
    return o


def _nb(tg):
    """states in a device level stack: [nb, kx, il, ix] or one [kx, il, ix]"""
    return tg.shape[0] if tg.dim() == 4 else 1


class MoistOut(ctypes.Structure):
    """spdy_moist_out (include/spdy.h): optional outputs of the moist physics, device pointers or None."""
    _fields_ = [("precnv", ctypes.c_void_p), ("precls", ctypes.c_void_p), ("cbmf", ctypes.c_void_p), ("iptop", ctypes.c_void_p),
                ("icnv", ctypes.c_void_p), ("qsat", ctypes.c_void_p), ("rh", ctypes.c_void_p), ("se", ctypes.c_void_p)]


MOIST_2D = ("precnv", "precls", "cbmf", "iptop", "icnv")   # (ix,il) per state; iptop / icnv int32
MOIST_3D = ("qsat", "rh", "se")                             # (ix,il,kx) per state


class RadSurface(ctypes.Structure):
    """spdy_rad_surface (include/spdy.h): land fraction and surface albedo, device pointers."""
    _fields_ = [("fmask", ctypes.c_void_p), ("albsfc", ctypes.c_void_p)]


class RadOut(ctypes.Structure):
    """spdy_rad_out (include/spdy.h): optional outputs of the radiation, device pointers or None."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr", "slrd", "slr", "olr",
                                                "tt_rsw", "tt_rlw")]


RAD_SW_2D = ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr")   # (ix,il) per state, compute_sw calls; icltop int32
RAD_2D = ("slrd", "slr", "olr")                                    # (ix,il) per state
RAD_3D = ("tt_rsw", "tt_rlw")                                      # (ix,il,kx) per state


class SfcBoundary(ctypes.Structure):
    """spdy_sfc_boundary (include/spdy.h): boundary fields of the surface fluxes, device pointers, all required."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("fmask", "sst", "stl", "soilw", "snowc", "alb_l", "alb_s")]


class SfcOut(ctypes.Structure):
    """spdy_sfc_out (include/spdy.h): optional outputs of the surface fluxes, device pointers or None."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("ustr", "vstr", "shf", "evap", "slru", "hfluxn", "tskin", "u0", "v0", "t0")]


class PblOut(ctypes.Structure):
    """spdy_pbl_out (include/spdy.h): optional outputs of the boundary layer, device pointers or None."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl")]


class ColumnPhysicsOut(ctypes.Structure):
    """spdy_column_physics_out (include/spdy.h): the optional outputs of every block of the chain, and ts / fsfcu."""
    _fields_ = [("moist", MoistOut), ("rad", RadOut), ("sfc", SfcOut), ("pbl", PblOut), ("ts", ctypes.c_void_p),
                ("fsfcu", ctypes.c_void_p)]


SFC_BOUNDARY = tuple(f[0] for f in SfcBoundary._fields_)
SFC_3 = ("ustr", "vstr", "shf", "evap", "slru")            # (ix,il,3) per state: land, sea, weighted
SFC_2D = ("tskin", "u0", "v0", "t0")                       # (ix,il) per state
PBL_2D = ("ut_pbl", "vt_pbl")                              # (ix,il) per state: level kx
PBL_3D = ("tt_pbl", "qt_pbl")                              # (ix,il,kx) per state


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


class DeviceField:
    """Device memory that a plan-side object owns, usable wherever a ``*_dev`` method takes a tensor (data_ptr()).
    ``numpy()`` and ``upload()`` are synchronising copies through a fresh host buffer, meant for tests, outputs and restarts:
    they wait for everything enqueued on the plan's stream, so a run keeps them out of its step loop."""

    def __init__(self, sp, ptr, shape):
        self.sp, self.ptr, self.shape = sp, int(ptr), tuple(shape)

    def data_ptr(self):
        return self.ptr

    def numpy(self):
        """A host copy, after everything enqueued on the plan's stream: allocates, blocks the host."""
        out = np.empty(self.shape)
        check(self.sp.lib.spdy_dev_download(self.sp.h, _p(out), ctypes.c_void_p(self.ptr), out.nbytes))
        return out

    def upload(self, a):
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != self.shape:
            raise ValueError("expected shape %s" % (self.shape,))
        check(self.sp.lib.spdy_dev_upload(self.sp.h, ctypes.c_void_p(self.ptr), _p(a), a.nbytes))


class SurfaceClim(ctypes.Structure):
    """spdy_surface_clim (include/spdy.h): the host fields a surface model is made from."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("fmask", "alb0", "stl12", "snowd12", "soilw12", "sst12", "sice12", "sstan3")]


SURFACE_LAND_COUPLING, SURFACE_ICE_COUPLING, SURFACE_SST_ANOMALY, SURFACE_DEFAULT = 1, 2, 4, 7
SURFACE_TABLES = ("fmask_l", "fmask_s", "rhcapl", "cdland", "rhcaps", "rhcapi", "cdsea", "cdice")
SURFACE_FIELDS = ("stlcl_ob", "snowdcl_ob", "soilwcl_ob", "stl_lm", "stl_am", "snowd_am", "soilw_am", "sstcl_ob", "sicecl_ob",
                  "ticecl_ob", "sstan_ob", "sst_om", "tice_om", "sice_om", "sst_am", "sstan_am", "sice_am", "tice_am", "ssti_om",
                  "snowc", "alb_l", "alb_s", "albsfc", "corh")


class SurfaceModel:
    """The slab land, sea and ice models and the daily forcing on the device (spdy_surface_model_* in include/spdy.h).

    clim: dict of host arrays fmask, alb0 [il, ix]; stl12, snowd12, soilw12, sst12, sice12 [12, il, ix]; sstan3 [3, il, ix] (may
    be absent without SURFACE_SST_ANOMALY).  One step of a run: on the first step of a day forcing_dev(qcorh); the step; the
    host's newdate and, when the day changed, set_date; couple_dev(day, hfluxn, shf, evap, ssrd)."""

    def __init__(self, sp, clim, delt, flags=SURFACE_DEFAULT):
        self.sp, self.lib, self.flags = sp, sp.lib, int(flags)
        shapes = {"fmask": (), "alb0": (), "stl12": (12,), "snowd12": (12,), "soilw12": (12,), "sst12": (12,), "sice12": (12,),
                  "sstan3": (3,)}
        host, c = {}, SurfaceClim()
        for n, lead in shapes.items():
            if clim.get(n) is None:
                continue
            host[n] = np.ascontiguousarray(clim[n], np.float64)
            if host[n].shape != lead + sp.grid_shape:
                raise ValueError("%s must have shape %s" % (n, lead + sp.grid_shape))
            setattr(c, n, host[n].ctypes.data)
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_surface_model_create(sp.h, ctypes.byref(c), float(delt), self.flags, ctypes.byref(h)))
        self.h = h
        # the plan closes its models first; the references of models that are gone are dropped here
        sp._models = [r for r in getattr(sp, "_models", []) if r() is not None and r().h] + [weakref.ref(self)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.spdy_surface_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def table(self, name):
        """A host table of land_model_init / sea_model_init (SURFACE_TABLES), [il, ix]."""
        n = check(self.lib.spdy_surface_model_table(self.h, name.encode(), None, 0))
        out = np.zeros(n)
        check(self.lib.spdy_surface_model_table(self.h, name.encode(), _p(out), n))
        return out.reshape(self.sp.grid_shape)

    def set_date(self, imont1, tmonth, tyear):
        """The date of the interpolations and of the zonal radiation forcing (date.f90:147-151's imont1, tmonth, tyear); the
        upload is ordered on the plan's stream, so a graph replayed after this call uses the new date."""
        self.sp._sync_stream()
        check(self.lib.spdy_surface_model_set_date(self.h, int(imont1), float(tmonth), float(tyear)))

    def set_sst_anomaly(self, sstan3):
        """Replaces the three-month window of SST anomalies [3, il, ix] (obs_ssta's shift)."""
        a = np.ascontiguousarray(sstan3, np.float64)
        if a.shape != (3,) + self.sp.grid_shape:
            raise ValueError("sstan3 must be [3, il, ix]")
        self.sp._sync_stream()
        check(self.lib.spdy_surface_model_set_sst_anomaly(self.h, _p(a)))

    def couple_dev(self, day, hfluxn=None, shf=None, evap=None, ssrd=None):
        """couple_sea_land(day) in one launch: hfluxn [2, il, ix], shf, evap [3, il, ix], ssrd [il, ix] device tensors as
        physics_dev writes them (None allowed with day == 0)."""
        self.sp._sync_stream()
        ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        check(self.lib.spdy_surface_model_couple_dev(self.h, int(day), ptr(hfluxn), ptr(shf), ptr(evap), ptr(ssrd)))

    def forcing_dev(self, qcorh):
        """set_forcing(1) parts 2 and 4: snowc, alb_l, alb_s, albsfc, and qcorh [nx, mx] complex128 (device tensor) written."""
        self.sp._sync_stream()
        check(self.lib.spdy_surface_model_forcing_dev(self.h, ctypes.c_void_p(qcorh.data_ptr())))

    def boundary_struct(self):
        """(SfcBoundary of the model's own device arrays, device pointer of albsfc) for the C calls."""
        b, alb = SfcBoundary(), ctypes.c_void_p()
        check(self.lib.spdy_surface_model_boundary(self.h, ctypes.byref(b), ctypes.byref(alb)))
        return b, alb

    def field(self, name):
        """A field of the model by the reference's name (SURFACE_FIELDS, SURFACE_TABLES, alb0): a DeviceField [il, ix] in the
        model's own device memory."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_surface_model_field(self.h, name.encode(), ctypes.byref(p)))
        return DeviceField(self.sp, p.value, self.sp.grid_shape)

    def boundary(self):
        """(bnd, albsfc) for Spectral.physics_dev: DeviceFields of the model's own arrays (bnd["fmask"] = fmask_l)."""
        names = {"fmask": "fmask_l", "sst": "sst_am", "stl": "stl_am", "soilw": "soilw_am", "snowc": "snowc", "alb_l": "alb_l",
                 "alb_s": "alb_s"}
        return {k: self.field(v) for k, v in names.items()}, self.field("albsfc")


class Spectral:
    """One transform plan = the module state `initialize_spectral` builds (spectral.f90:20)."""

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
            for ref in getattr(self, "_models", []):       # a surface model must go before its plan (include/spdy.h)
                m = ref()
                if m is not None:
                    m.close()
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
        if not getattr(self, "_follow", True) or getattr(self, "_capturing", False):
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
        "t63_derive" (0 / 1), "t63_np2_from", "wt_min_mb"."""
        check(self.lib.spdy_plan_set_option(self.h, name.encode(), int(value)))

    def wave_placement(self):
        """(SIMD of waves 0..7 of workgroup 0, number of workgroups that violate the round-robin placement the T63 kernels'
        role assignment relies on) -- spdy_wave_placement."""
        import ctypes
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
        return ctypes.c_void_p(t.data_ptr())

    def spec_to_grid_dev(self, d_spec, d_grid, kcos=1, d_kcos=None):
        """d_spec: [nb, nx, mx] complex128 (or [nb,nx,mx,2] float64) CUDA tensor; d_grid: [nb, il, ix] float64."""
        self._sync_stream()
        nb = d_grid.shape[0]
        check(self.lib.spdy_spec_to_grid_dev(self.h, nb, self._dp(d_spec), self._dp(d_kcos) if d_kcos is not None else None,
                                             int(kcos), self._dp(d_grid)))

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
                                              spec.shape[0], self._dp(spec), self._dp(d_kcos) if d_kcos is not None else None, int(kcos),
                                              self._dp(grid)))

    def inverse_batch_grad_dev(self, vor, div, ug, vg, spec, grid, psi, gx, gy, kcos_pairs=2, kcos=1, d_kcos=None, kcos_grad=2):
        """inverse_batch_dev + grad_to_grid_dev(psi -> gx, gy): everything a step transforms to the grid, one fused launch at T63."""
        self._sync_stream()
        check(self.lib.spdy_inverse_batch_grad_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg),
                                                   int(kcos_pairs), spec.shape[0], self._dp(spec),
                                                   self._dp(d_kcos) if d_kcos is not None else None, int(kcos), self._dp(grid),
                                                   psi.shape[0], self._dp(psi), self._dp(gx), self._dp(gy), int(kcos_grad)))

    def inverse_batch_segs_dev(self, vor, div, ug, vg, specs, grid, psi=None, gx=None, gy=None, kcos_pairs=2, kcos=1, d_kcos=None, kcos_grad=2):
        """inverse_batch_grad_dev with the plain spectra in up to four separate arrays `specs` (tendencies.f90:89-101 reads
        vor, div, t, tr from four prognostic arrays); their grids are the one stack `grid`.  psi / gx / gy optional."""
        self._sync_stream()
        import ctypes

        class Seg(ctypes.Structure):
            _fields_ = [("nb", ctypes.c_int), ("d_spec", ctypes.c_void_p)]
        segs = (Seg * len(specs))(*[Seg(int(x.shape[0]), self._dp(x)) for x in specs])
        ngrad = 0 if psi is None else psi.shape[0]
        check(self.lib.spdy_inverse_batch_segs_dev(self.h, vor.shape[0], self._dp(vor), self._dp(div), self._dp(ug), self._dp(vg),
                                                   int(kcos_pairs), len(specs), ctypes.cast(segs, ctypes.c_void_p),
                                                   self._dp(d_kcos) if d_kcos is not None else None, int(kcos), self._dp(grid),
                                                   ngrad, self._dp(psi) if ngrad else None, self._dp(gx) if ngrad else None,
                                                   self._dp(gy) if ngrad else None, int(kcos_grad)))

    def direct_batch_dev(self, ug, vg, vor, div, grid, spec, kcos=2):
        """vdspec of the (ug, vg) pairs and grid_to_spec of `grid` in one launch (a model step's direct batch)."""
        self._sync_stream()
        check(self.lib.spdy_direct_batch_dev(self.h, ug.shape[0], self._dp(ug), self._dp(vg), self._dp(vor), self._dp(div), int(kcos),
                                             grid.shape[0], self._dp(grid), self._dp(spec)))

    def implicit_terms_dev(self, divdt, tdt, psdt):
        self._sync_stream()
        check(self.lib.spdy_implicit_terms_dev(self.h, self._dp(divdt), self._dp(tdt), self._dp(psdt)))

    def grid_tendencies_dev(self, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out):
        """tendencies.f90:105-197 on the gridded prognostics; outputs are the operands of one direct_batch_dev launch."""
        self._sync_stream()
        args = (ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out)
        check(self.lib.spdy_grid_tendencies_dev(self.h, *[self._dp(x) for x in args]))

    def tendency_combine_dev(self, pdiv, pspec):
        """In place on the direct batch's outputs: divdt -= laplacian(KE), tdt += ttend, trdt += trtend, psdt(1,1) = 0."""
        self._sync_stream()
        check(self.lib.spdy_tendency_combine_dev(self.h, self._dp(pdiv), self._dp(pspec)))

    def spectral_step_dev(self, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag, j1, dt, eps, wil, phi):
        """Everything after the direct batch in one launch: tendency_combine, spectral_tendencies, implicit_terms, hdiff_step
        and step_fields of ps, vor, div, t, tr (prognostics [2,kx,nx,mx] / ps [2,nx,mx], both time levels)."""
        self._sync_stream()
        args = (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh)
        check(self.lib.spdy_spectral_step_dev(self.h, *[self._dp(x) for x in args], float(sdrag), int(j1), float(dt), float(eps),
                                              float(wil), self._dp(phi)))

    def direct_batch_spectral_step_dev(self, ug, vg, grid, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh, sdrag, j1, dt,
                                       eps, wil, phi, kcos=2):
        """direct_batch_dev(ug, vg [3kx] -> pvor, pdiv; grid [3kx+1] -> pspec) + spectral_step_dev as one call (at T63 vds is
        applied where the spectral step reads the pairs' spectra: one launch less)."""
        self._sync_stream()
        args = (pvor, pdiv, pspec, vor, div, t, tr, ps, phis, tcorh, qcorh)
        check(self.lib.spdy_direct_batch_spectral_step_dev(self.h, self._dp(ug), self._dp(vg), self._dp(grid), int(kcos),
                                                           *[self._dp(x) for x in args], float(sdrag), int(j1), float(dt), float(eps),
                                                           float(wil), self._dp(phi)))

    def output_batch_dev(self, vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out):
        """input_output.f90:184-206 on device-resident state: complex128 [kx,nx,mx] (ps [nx,mx]) in, float32 [kx,il,ix]
        (ps_out [il,ix]) out."""
        self._sync_stream()
        args = (vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out)
        check(self.lib.spdy_output_batch_dev(self.h, *[self._dp(x) for x in args]))

    def geopotential_dev(self, t, phis, phi):
        self._sync_stream()
        check(self.lib.spdy_geopotential_dev(self.h, self._dp(t), self._dp(phis), self._dp(phi)))

    def spectral_tendencies_dev(self, div, t, ps, phis, divdt, tdt, psdt, phi):
        """tendencies.f90:242-293 -- div, t, ps: time level j2 of the prognostics; divdt, tdt, psdt in place; phi out."""
        self._sync_stream()
        check(self.lib.spdy_spectral_tendencies_dev(self.h, *[self._dp(x) for x in (div, t, ps, phis, divdt, tdt, psdt, phi)]))

    def hdiff_step_dev(self, vor, div, t, tr, tcorh, qcorh, sdrag, vordt, divdt, tdt, trdt):
        """The diffusion block of step() (time_stepping.f90:62-96) in one launch; tendencies in place."""
        self._sync_stream()
        dp = lambda x: self._dp(x) if x is not None else None
        check(self.lib.spdy_hdiff_step_dev(self.h, dp(vor), dp(div), dp(t), dp(tr), dp(tcorh), dp(qcorh), float(sdrag),
                                           dp(vordt), dp(divdt), dp(tdt), dp(trdt)))

    def step_fields_dev(self, pairs, j1, dt, eps, wil):
        """step_field_2d/3d for several prognostic arrays in one launch: pairs = [(field [2,nlev,nx,mx], fdt [nlev,nx,mx]), ...]."""
        self._sync_stream()
        class Op(ctypes.Structure):
            _fields_ = [("nlev", ctypes.c_int), ("field", ctypes.c_void_p), ("fdt", ctypes.c_void_p)]
        arr = (Op * len(pairs))()
        for o, (f, d) in zip(arr, pairs):
            nlev = 1 if d.dim() == 2 else d.shape[0]
            assert f.numel() == 2 * d.numel()
            o.nlev, o.field, o.fdt = nlev, f.data_ptr(), d.data_ptr()
        check(self.lib.spdy_step_fields_dev(self.h, len(pairs), ctypes.cast(arr, ctypes.c_void_p), int(j1), float(dt), float(eps), float(wil)))

    def hdiff_multi_dev(self, ops):
        """ops: up to 8 tuples (field, fdt_in, dmp_name, dmp1_name, out) -- the diffusion calls of one time step
        (time_stepping.f90:63-96) in one launch."""
        self._sync_stream()
        class Op(ctypes.Structure):
            _fields_ = [("nlev", ctypes.c_int), ("field", ctypes.c_void_p), ("fdt_in", ctypes.c_void_p),
                        ("d_dmp", ctypes.c_void_p), ("d_dmp1", ctypes.c_void_p), ("fdt_out", ctypes.c_void_p)]
        arr = (Op * len(ops))()
        for o, (field, fdt_in, dmp_name, dmp1_name, out) in zip(arr, ops):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            check(self.lib.spdy_device_table(self.h, dmp_name.encode(), ctypes.byref(a)))
            check(self.lib.spdy_device_table(self.h, dmp1_name.encode(), ctypes.byref(b)))
            o.nlev, o.field, o.fdt_in, o.d_dmp, o.d_dmp1, o.fdt_out = field.shape[0], field.data_ptr(), fdt_in.data_ptr(), a.value, b.value, out.data_ptr()
        check(self.lib.spdy_hdiff_multi_dev(self.h, len(ops), ctypes.cast(arr, ctypes.c_void_p)))

    def hdiff_dev(self, field, fdt_in, dmp_name, dmp1_name, out):
        self._sync_stream()
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.spdy_device_table(self.h, dmp_name.encode(), ctypes.byref(a)))
        check(self.lib.spdy_device_table(self.h, dmp1_name.encode(), ctypes.byref(b)))
        check(self.lib.spdy_hdiff_dev(self.h, field.shape[0], self._dp(field), self._dp(fdt_in), a, b, self._dp(out)))

    # ------------------------------------------------------------------ moist physics (physics.f90:110-138)
    def moist_columns_dev(self, tg, qg, phig, pslg, ttend, qtend, out=None):
        """Precipitation block on nb gridded states: tg, qg, phig, ttend, qtend [nb,kx,il,ix] (or [kx,il,ix]), pslg [nb,il,ix];
        ttend / qtend in place.  out: dict of optional device outputs (MOIST_2D [nb,il,ix], iptop/icnv int32; MOIST_3D like tg)."""
        self._sync_stream()
        o = _out_struct(MoistOut, out)
        check(self.lib.spdy_moist_columns_dev(self.h, _nb(tg), *[self._dp(x) for x in (tg, qg, phig, pslg, ttend, qtend)], ctypes.byref(o)))

    def moist_workspace(self):
        check(self.lib.spdy_moist_workspace(self.h))

    def moist_physics_dev(self, t, q, phi, ps, ttend, qtend, out=None):
        """The same from one state's spectra (time level 1: t, q [kx,nx,mx], phi [kx,nx,mx], ps [nx,mx] complex128): one inverse
        launch into plan workspace, then the column kernel.  ttend / qtend [kx,il,ix] in place."""
        self._sync_stream()
        o = _out_struct(MoistOut, out)
        check(self.lib.spdy_moist_physics_dev(self.h, *[self._dp(x) for x in (t, q, phi, ps, ttend, qtend)], ctypes.byref(o)))

    # ------------------------------------------------------------------ radiation (physics.f90:146-166, :180-186)
    def radiation_set_date(self, tyear):
        """Zonal radiation forcing of the date tyear (fraction of the year; get_zonal_average_fields + solar).  On a device plan
        the upload is ordered on the plan's stream: a graph replayed after this call uses the new date."""
        if self.device >= 0:
            self._sync_stream()
        check(self.lib.spdy_radiation_set_date(self.h, float(tyear)))

    def radiation_state_size(self):
        """Doubles of radiation state per model state (the caller's device buffer holds nb of them)."""
        return check(self.lib.spdy_radiation_state_size(self.h))

    def radiation_down_dev(self, compute_sw, tg, qg, phig, pslg, rh, precnv, precls, iptop, fmask, albsfc, state, out=None):
        """Down half on nb gridded states: tg, qg, phig, rh [nb,kx,il,ix] (or [kx,il,ix]); pslg, precnv, precls, iptop (int32),
        fmask, albsfc [nb,il,ix]; state [nb * radiation_state_size()] float64.  rh .. albsfc are read with compute_sw only and
        may be None otherwise.  out: dict of optional device outputs (RAD_SW_2D, RAD_2D [nb,il,ix]; RAD_3D like tg)."""
        self._sync_stream()
        sfc = RadSurface(self._dp(fmask) if fmask is not None else None, self._dp(albsfc) if albsfc is not None else None)
        ptr = lambda x: None if x is None else self._dp(x)
        check(self.lib.spdy_radiation_down_dev(self.h, _nb(tg), 1 if compute_sw else 0, *[ptr(x) for x in (tg, qg, phig, pslg, rh,
                                               precnv, precls, iptop)], ctypes.byref(sfc), self._dp(state),
                                               ctypes.byref(_out_struct(RadOut, out))))

    def radiation_up_dev(self, tg, pslg, ts, fsfcu, state, ttend, out=None):
        """Up half: ts, fsfcu (= slru(:,:,3)) [nb,il,ix]; ttend [nb,kx,il,ix] in place (+ tt_rsw + tt_rlw)."""
        self._sync_stream()
        check(self.lib.spdy_radiation_up_dev(self.h, _nb(tg), *[self._dp(x) for x in (tg, pslg, ts, fsfcu, state, ttend)],
                                             ctypes.byref(_out_struct(RadOut, out))))

    # ------------------------------------------------------------------ surface fluxes, boundary layer (physics.f90:169-170, :193-205)
    def surface_set_orography(self, phis0):
        """Surface geopotential phis0 [il, ix]: the plan keeps it and forog (set_orog_land_sfc_drag); on a device plan the upload
        is ordered on the plan's stream."""
        if self.device >= 0:
            self._sync_stream()
        a = np.ascontiguousarray(phis0, np.float64)
        if a.shape != self.grid_shape:
            raise ValueError("phis0 must be [il, ix]")
        check(self.lib.spdy_surface_set_orography(self.h, _p(a)))

    def _boundary(self, bnd):
        return SfcBoundary(*[self._dp(bnd[n]) for n in SFC_BOUNDARY])

    def surface_fluxes_dev(self, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd, ts, fsfcu, flux3, out=None):
        """get_surface_fluxes on nb gridded states: ug .. phig [nb,kx,il,ix] (or [kx,il,ix]); pslg, ssrd, slrd and the fields of
        bnd (dict: SFC_BOUNDARY) [nb,il,ix]; writes ts, fsfcu [nb,il,ix] and flux3 [nb,4,il,ix] (ustr3 vstr3 shf3 evap3).  out: dict
        of optional device outputs (SFC_3 [nb,3,il,ix], hfluxn [nb,2,il,ix], SFC_2D [nb,il,ix])."""
        self._sync_stream()
        b = self._boundary(bnd)
        check(self.lib.spdy_surface_fluxes_dev(self.h, _nb(tg), *[self._dp(x) for x in (ug, vg, tg, qg, phig, pslg, ssrd, slrd)],
                                               ctypes.byref(b), self._dp(ts), self._dp(fsfcu), self._dp(flux3),
                                               ctypes.byref(_out_struct(SfcOut, out))))

    def pbl_dev(self, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend, out=None):
        """get_vertical_diffusion_tend, the surface-flux tendencies and the four sums: qg, phig, se, rh, qsat [nb,kx,il,ix] (or
        [kx,il,ix]), pslg, icnv (int32) [nb,il,ix], flux3 [nb,4,il,ix]; utend (level kx only), vtend, ttend, qtend in place.  out:
        dict of optional device outputs (PBL_2D [nb,il,ix], PBL_3D like qg)."""
        self._sync_stream()
        check(self.lib.spdy_pbl_dev(self.h, _nb(qg), *[self._dp(x) for x in (qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend,
                                                                            ttend, qtend)], ctypes.byref(_out_struct(PblOut, out))))

    def column_physics_workspace(self):
        check(self.lib.spdy_column_physics_workspace(self.h))

    def column_physics_dev(self, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, state, utend, vtend, ttend, qtend, out=None):
        """physics.f90:110-205 on nb gridded states: moist block, radiation down, surface fluxes, radiation up, boundary layer, the
        intermediates in plan workspace.  out: dict with optional dicts "moist", "rad", "sfc", "pbl" (as the single calls take
        them) and optional tensors "ts", "fsfcu"."""
        self._sync_stream()
        o = self._column_physics_out(out)
        b = self._boundary(bnd)
        check(self.lib.spdy_column_physics_dev(self.h, _nb(tg), 1 if compute_sw else 0, *[self._dp(x) for x in (ug, vg, tg, qg, phig,
                                               pslg)], ctypes.byref(b), None if albsfc is None else self._dp(albsfc),
                                               self._dp(state), *[self._dp(x) for x in (utend, vtend, ttend, qtend)], ctypes.byref(o)))

    def _column_physics_out(self, out):
        out = out or {}
        return ColumnPhysicsOut(_out_struct(MoistOut, out.get("moist")), _out_struct(RadOut, out.get("rad")),
                                _out_struct(SfcOut, out.get("sfc")), _out_struct(PblOut, out.get("pbl")),
                                None if out.get("ts") is None else self._dp(out["ts"]),
                                None if out.get("fsfcu") is None else self._dp(out["fsfcu"]))

    def physics_workspace(self):
        check(self.lib.spdy_physics_workspace(self.h))

    def physics_dev(self, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, state, utend, vtend, ttend, qtend, out=None):
        """physics.f90:94-205 on one state from its spectra (time level 1: vor, div, t, q, phi [kx,nx,mx], ps [nx,mx] complex128):
        one inverse launch into plan workspace, then the column physics (one launch, or the five calls with the plan option
        "physics_fused" 0).  utend, vtend, ttend, qtend [kx,il,ix] in place; bnd, albsfc, state and out as column_physics_dev."""
        self._sync_stream()
        o = self._column_physics_out(out)
        b = self._boundary(bnd)
        check(self.lib.spdy_physics_dev(self.h, 1 if compute_sw else 0, *[self._dp(x) for x in (vor, div, t, q, phi, ps)],
                                        ctypes.byref(b), None if albsfc is None else self._dp(albsfc), self._dp(state),
                                        *[self._dp(x) for x in (utend, vtend, ttend, qtend)], ctypes.byref(o)))

    def _grid_args(self, ins, names3, ref="tg"):
        """ins (name -> array) as float64 arrays, shapes checked against the level stack ins[ref]: names3 are level stacks, the
        others (ix,il) fields.  Returns (ins, the level stack's shape, its leading (batch) shape, nb)."""
        ins = {k: np.ascontiguousarray(v, np.float64) for k, v in ins.items()}
        grid3 = ins[ref].shape
        if grid3[-3:] != (self.kx,) + self.grid_shape:
            raise ValueError("%s must be [nb,] kx, il, ix" % ref)
        lead = grid3[:-3]
        for k, v in ins.items():
            want = grid3 if k in names3 else lead + self.grid_shape
            if v.shape != want:
                raise ValueError("%s must have shape %s" % (k, want))
        return ins, grid3, lead, int(np.prod(lead)) if lead else 1

    def _sfc_results(self, lead):
        res = {n: np.empty(lead + (3,) + self.grid_shape) for n in SFC_3}
        res["hfluxn"] = np.empty(lead + (2,) + self.grid_shape)
        res.update({n: np.empty(lead + self.grid_shape) for n in SFC_2D + ("ts", "fsfcu")})
        res["flux3"] = np.empty(lead + (4,) + self.grid_shape)
        return res

    def surface_columns(self, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd):
        """NumPy convenience: spdy_surface_fluxes_dev on copies in plan-owned device memory.  bnd: dict of the SFC_BOUNDARY fields.
        Returns a dict with ts, fsfcu, flux3 [nb,4,il,ix] and every optional output."""
        ins = dict(ug=ug, vg=vg, tg=tg, qg=qg, phig=phig, pslg=pslg, ssrd=ssrd, slrd=slrd, **{n: bnd[n] for n in SFC_BOUNDARY})
        ins, _, lead, nb = self._grid_args(ins, ("ug", "vg", "tg", "qg", "phig"))
        res = self._sfc_results(lead)

        def call(d):
            b = SfcBoundary(*[d[n].value for n in SFC_BOUNDARY])
            o = SfcOut(**{n: d[n].value for n in SFC_3 + ("hfluxn",) + SFC_2D})
            check(self.lib.spdy_surface_fluxes_dev(self.h, nb, *[d[n] for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "ssrd", "slrd")],
                                                   ctypes.byref(b), d["ts"], d["fsfcu"], d["flux3"], ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def pbl_columns(self, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend):
        """NumPy convenience: spdy_pbl_dev on copies in plan-owned device memory.  Returns a dict with the updated utend, vtend,
        ttend, qtend and every optional output."""
        names3 = ("qg", "phig", "se", "rh", "qsat", "utend", "vtend", "ttend", "qtend")
        ins = dict(qg=qg, phig=phig, pslg=pslg, se=se, rh=rh, qsat=qsat, utend=utend, vtend=vtend, ttend=ttend, qtend=qtend)
        ins, grid3, lead, nb = self._grid_args(ins, names3, "qg")
        ins["icnv"] = np.ascontiguousarray(icnv, np.int32)
        ins["flux3"] = np.ascontiguousarray(flux3, np.float64)
        if ins["icnv"].shape != lead + self.grid_shape or ins["flux3"].shape != lead + (4,) + self.grid_shape:
            raise ValueError("icnv must be [nb,] il, ix and flux3 [nb,] 4, il, ix")
        res = {n: np.empty(grid3) for n in ("utend", "vtend", "ttend", "qtend") + PBL_3D}
        res.update({n: np.empty(lead + self.grid_shape) for n in PBL_2D})

        def call(d):
            o = PblOut(**{n: d[n].value for n in PBL_2D + PBL_3D})
            check(self.lib.spdy_pbl_dev(self.h, nb, *[d[n] for n in ("qg", "phig", "pslg", "se", "rh", "qsat", "icnv", "flux3", "utend",
                                                                     "vtend", "ttend", "qtend")], ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def column_physics(self, ug, vg, tg, qg, phig, pslg, bnd, albsfc, utend, vtend, ttend, qtend, compute_sw=True, state=None):
        """NumPy convenience: spdy_column_physics_dev on copies in plan-owned device memory.  state: the radiation state to start
        from (as returned under "state"); None starts a fresh one (then compute_sw must be set).  On calls without shortwave the
        plan's workspace holds the ssrd of the last call with it.  Returns a dict with the updated tendencies, every optional
        output of every block (those of the shortwave only with compute_sw) and the updated state."""
        names3 = ("ug", "vg", "tg", "qg", "phig", "utend", "vtend", "ttend", "qtend")
        ins = dict(ug=ug, vg=vg, tg=tg, qg=qg, phig=phig, pslg=pslg, utend=utend, vtend=vtend, ttend=ttend, qtend=qtend,
                   **{n: bnd[n] for n in SFC_BOUNDARY})
        if compute_sw:
            ins["albsfc"] = albsfc
        ins, grid3, lead, nb = self._grid_args(ins, names3)
        nst = self.radiation_state_size() * nb
        if state is None and not compute_sw:
            raise ValueError("the first call on a radiation state must have compute_sw set")
        ins["state"] = np.zeros(nst) if state is None else np.ascontiguousarray(state, np.float64)
        if ins["state"].shape != (nst,):
            raise ValueError("state must hold %d doubles" % nst)
        rad = tuple(n for n in RAD_2D + ("tt_rlw",) + ((RAD_SW_2D + ("tt_rsw",)) if compute_sw else ()) if n != "ssrd")
        res = self._sfc_results(lead)
        del res["flux3"]
        res.update({n: np.empty(grid3) for n in ("utend", "vtend", "ttend", "qtend") + MOIST_3D + PBL_3D})
        res["state"] = np.empty(nst)
        res.update({n: np.empty(lead + self.grid_shape, np.int32 if n in ("iptop", "icnv") else np.float64) for n in MOIST_2D + PBL_2D})
        res.update({n: np.empty(grid3 if n in RAD_3D else lead + self.grid_shape, np.int32 if n == "icltop" else np.float64)
                    for n in rad})

        def call(d):
            o = ColumnPhysicsOut(MoistOut(**{n: d[n].value for n in MOIST_2D + MOIST_3D}), RadOut(**{n: d[n].value for n in rad}),
                                 SfcOut(**{n: d[n].value for n in SFC_3 + ("hfluxn",) + SFC_2D}),
                                 PblOut(**{n: d[n].value for n in PBL_2D + PBL_3D}), d["ts"].value, d["fsfcu"].value)
            b = SfcBoundary(*[d[n].value for n in SFC_BOUNDARY])
            check(self.lib.spdy_column_physics_dev(self.h, nb, 1 if compute_sw else 0, *[d[n] for n in ("ug", "vg", "tg", "qg", "phig",
                                                   "pslg")], ctypes.byref(b), d.get("albsfc"), d["state"],
                                                   *[d[n] for n in ("utend", "vtend", "ttend", "qtend")], ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def radiation_columns(self, tg, qg, phig, pslg, rh, precnv, precls, iptop, fmask, albsfc, ts, fsfcu, ttend, compute_sw=True,
                          state=None):
        """NumPy convenience: both radiation halves on copies in plan-owned device memory.  Shapes as radiation_down_dev (NumPy).
        state: the radiation state to start from (as returned under "state"); None starts a fresh one (then compute_sw must be
        set).  Returns a dict with the updated ttend, every optional output (those of the shortwave only with compute_sw) and the
        updated state."""
        ins = {"tg": tg, "qg": qg, "phig": phig, "pslg": pslg, "ts": ts, "fsfcu": fsfcu, "ttend": ttend}
        if compute_sw:
            ins.update(rh=rh, precnv=precnv, precls=precls, fmask=fmask, albsfc=albsfc)
        ins = {k: np.ascontiguousarray(v, np.float64) for k, v in ins.items()}
        grid3 = ins["tg"].shape
        if grid3[-3:] != (self.kx,) + self.grid_shape:
            raise ValueError("tg must be [nb,] kx, il, ix")
        lead = grid3[:-3]
        nb = int(np.prod(lead)) if lead else 1
        for k, v in ins.items():
            want = grid3 if k in ("tg", "qg", "phig", "rh", "ttend") else lead + self.grid_shape
            if v.shape != want:
                raise ValueError("%s must have shape %s" % (k, want))
        if compute_sw:
            ins["iptop"] = np.ascontiguousarray(iptop, np.int32)
            if ins["iptop"].shape != lead + self.grid_shape:
                raise ValueError("iptop must be [nb,] il, ix")
        nst = self.radiation_state_size() * nb
        if state is None and not compute_sw:
            raise ValueError("the first call on a radiation state must have compute_sw set")
        st = np.zeros(nst) if state is None else np.ascontiguousarray(state, np.float64)
        if st.shape != (nst,):
            raise ValueError("state must hold %d doubles" % nst)
        names = RAD_2D + ("tt_rlw",) + ((RAD_SW_2D + ("tt_rsw",)) if compute_sw else ())
        res = {n: np.empty(grid3 if n in RAD_3D else lead + self.grid_shape, np.int32 if n == "icltop" else np.float64)
               for n in names}
        res.update(ttend=np.empty(grid3), state=np.empty(nst))
        ins["state"] = st

        def call(d):
            o = RadOut(**{n: d[n].value for n in names})
            sfc = RadSurface(d["fmask"].value, d["albsfc"].value) if compute_sw else RadSurface()
            g = lambda k: d.get(k)
            check(self.lib.spdy_radiation_down_dev(self.h, nb, 1 if compute_sw else 0, g("tg"), g("qg"), g("phig"), g("pslg"),
                                                   g("rh"), g("precnv"), g("precls"), g("iptop"), ctypes.byref(sfc), d["state"],
                                                   ctypes.byref(o)))
            check(self.lib.spdy_radiation_up_dev(self.h, nb, d["tg"], d["pslg"], d["ts"], d["fsfcu"], d["state"], d["ttend"],
                                                 ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def moist_columns(self, tg, qg, phig, pslg, ttend, qtend):
        """NumPy convenience: spdy_moist_columns_dev on copies in plan-owned device memory.  Returns a dict with the updated
        ttend, qtend and every optional output (shapes as the inputs; iptop / icnv int32)."""
        ins = [np.ascontiguousarray(a, np.float64) for a in (tg, qg, phig, pslg, ttend, qtend)]
        grid3 = ins[0].shape
        if grid3[-3:] != (self.kx,) + self.grid_shape or any(a.shape != grid3 for a in (ins[1], ins[2], ins[4], ins[5])):
            raise ValueError("tg, qg, phig, ttend, qtend must be [nb,] kx, il, ix")
        lead = grid3[:-3]
        nb = int(np.prod(lead)) if lead else 1
        if ins[3].shape != lead + self.grid_shape:
            raise ValueError("pslg must be [nb,] il, ix")
        res = {"ttend": np.empty(grid3), "qtend": np.empty(grid3)}
        for n in MOIST_2D:
            res[n] = np.empty(lead + self.grid_shape, np.int32 if n in ("iptop", "icnv") else np.float64)
        for n in MOIST_3D:
            res[n] = np.empty(grid3)
        ins = dict(zip(("tg", "qg", "phig", "pslg", "ttend", "qtend"), ins))

        def call(d):
            o = MoistOut(**{n: d[n].value for n in MOIST_2D + MOIST_3D})
            check(self.lib.spdy_moist_columns_dev(self.h, nb, *[d[n] for n in ins], ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def _on_device(self, ins, res, call):
        """Copy the NumPy arrays of ins (name -> array) into plan-owned device memory and allocate a buffer for each array of res
        (name -> array) that ins does not hold; call(d) with d: name -> device pointer; copy every buffer of res back into its
        array and return res.  The buffers are freed whatever happens."""
        d = {}
        try:
            for n, a in list(ins.items()) + [(n, a) for n, a in res.items() if n not in ins]:
                ptr = ctypes.c_void_p()
                check(self.lib.spdy_dev_alloc(self.h, max(a.nbytes, 8), ctypes.byref(ptr)))
                d[n] = ptr
                if n in ins:
                    check(self.lib.spdy_dev_upload(self.h, ptr, _p(a), a.nbytes))
            call(d)
            for n, a in res.items():
                check(self.lib.spdy_dev_download(self.h, _p(a), d[n], a.nbytes))
        finally:
            for ptr in d.values():
                self.lib.spdy_dev_free(self.h, ptr)
        return res
