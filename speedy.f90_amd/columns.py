"""Column physics and the surface models over the C-ABI: the part of the binding that is no mirror of the `spectral` module.

FIELDS names every array of the optional-output, boundary and climatology structs of include/spdy.h once, in the header's member
order, with its shape and dtype.  The ctypes structures, the public name tuples, the output buffers (Spectral.column_outputs) and
the NumPy conveniences are all derived from it.  Arrays are NumPy C-order views of the reference's column-major ones, so a level
stack (ix,il,kx) is [kx, il, ix]; nb states lie back to back along a leading axis.
ColumnPhysics is a mixin of spectral.Spectral: it uses the plan's lib, h, kx, grid_shape, device, _dp and _sync_stream.
"""
import ctypes

import numpy as np

from ._lib import check

# kind of an array = what precedes (il, ix) in one state's shape: the levels, nothing, or a number of planes
LEVELS, FIELD = "kx", "field"


def _table(kind, *names, dtype=np.float64):
    return tuple((n, kind, dtype) for n in names)


_RAD_SW = _table(FIELD, "cloudc", "clstr") + _table(FIELD, "icltop", dtype=np.int32) + _table(FIELD, "ssrd", "ssr", "tsr")
FIELDS = {      # struct of include/spdy.h (without spdy_ and _out) -> ((name, kind, dtype), ...)
    "moist": _table(FIELD, "precnv", "precls", "cbmf") + _table(FIELD, "iptop", "icnv", dtype=np.int32) + _table(LEVELS, "qsat", "rh", "se"),
    "rad_surface": _table(FIELD, "fmask", "albsfc"),
    "rad": _RAD_SW + _table(FIELD, "slrd", "slr", "olr") + _table(LEVELS, "tt_rsw", "tt_rlw"),
    "sfc_boundary": _table(FIELD, "fmask", "sst", "stl", "soilw", "snowc", "alb_l", "alb_s"),
    "sfc": _table(3, "ustr", "vstr", "shf", "evap", "slru") + _table(2, "hfluxn") + _table(FIELD, "tskin", "u0", "v0", "t0"),
    "pbl": _table(FIELD, "ut_pbl", "vt_pbl") + _table(LEVELS, "tt_pbl", "qt_pbl"),
    "column_physics": _table(FIELD, "ts", "fsfcu"),       # after the four blocks
    "surface_clim": _table(FIELD, "fmask", "alb0") + _table(12, "stl12", "snowd12", "soilw12", "sst12", "sice12") + _table(3, "sstan3"),
    "args": _table(LEVELS, "ug", "vg", "tg", "qg", "phig", "utend", "vtend", "ttend", "qtend") + _table(FIELD, "pslg") + _table(4, "flux3"),       # the calls' plain arguments
}
BLOCKS = ("moist", "rad", "sfc", "pbl")
_KIND = {n: (kind, dtype) for t in FIELDS.values() for n, kind, dtype in t}


def dtype_of(name):
    return _KIND[name][1]


def shape_of(name, lead, kx, grid_shape):
    """Shape of the array `name` for a batch of leading shape `lead` (a tuple, () for one state)."""
    kind = _KIND[name][0]
    return tuple(lead) + {LEVELS: (kx,), FIELD: ()}.get(kind, (kind,)) + tuple(grid_shape)


def _names(table, kind=None):
    table = FIELDS[table] if isinstance(table, str) else table
    return tuple(n for n, k, _ in table if kind in (None, k))


def _struct(name, table, nested=()):
    """The ctypes mirror of a struct of include/spdy.h: the nested (name, struct) members, then one pointer per entry of the table."""
    return type(name, (ctypes.Structure,), {"_fields_": list(nested) + [(n, ctypes.c_void_p) for n in _names(table)]})


# the optional outputs are device pointers or None; boundary and climatology fields are all required
MoistOut = _struct("MoistOut", "moist")                    # spdy_moist_out: optional outputs of the moist physics
RadSurface = _struct("RadSurface", "rad_surface")          # spdy_rad_surface: land fraction and surface albedo
RadOut = _struct("RadOut", "rad")                          # spdy_rad_out: optional outputs of the radiation
SfcBoundary = _struct("SfcBoundary", "sfc_boundary")       # spdy_sfc_boundary: boundary fields of the surface fluxes
SfcOut = _struct("SfcOut", "sfc")                          # spdy_sfc_out: optional outputs of the surface fluxes
PblOut = _struct("PblOut", "pbl")                          # spdy_pbl_out: optional outputs of the boundary layer
OUT_STRUCTS = {"moist": MoistOut, "rad": RadOut, "sfc": SfcOut, "pbl": PblOut}
# spdy_column_physics_out: the optional outputs of every block of the chain, and ts / fsfcu
ColumnPhysicsOut = _struct("ColumnPhysicsOut", "column_physics", [(b, OUT_STRUCTS[b]) for b in BLOCKS])
SurfaceClim = _struct("SurfaceClim", "surface_clim")       # spdy_surface_clim: the host fields a surface model is made from

MOIST_2D = _names("moist", FIELD)              # (ix,il) per state; iptop / icnv int32
MOIST_3D = _names("moist", LEVELS)             # (ix,il,kx) per state
RAD_SW_2D = _names(_RAD_SW)                    # (ix,il) per state, compute_sw calls; icltop int32
RAD_2D = _names("rad", FIELD)[len(RAD_SW_2D):]   # (ix,il) per state
RAD_3D = _names("rad", LEVELS)                 # (ix,il,kx) per state
SFC_BOUNDARY = _names("sfc_boundary")
SFC_3 = _names("sfc", 3)                       # (ix,il,3) per state: land, sea, weighted
SFC_2D = _names("sfc", FIELD)                  # (ix,il) per state
PBL_2D = _names("pbl", FIELD)                  # (ix,il) per state: level kx
PBL_3D = _names("pbl", LEVELS)                 # (ix,il,kx) per state
_TEND = ("utend", "vtend", "ttend", "qtend")


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


def _struct_of(cls, d):
    """The struct cls with every member that d (name -> device pointer, as _on_device passes it) holds; the others stay None."""
    return cls(**{n: _struct_of(t, d) if issubclass(t, ctypes.Structure) else d[n].value for n, t in cls._fields_
                  if issubclass(t, ctypes.Structure) or n in d})


def _nb(tg):
    """states in a device level stack: [nb, kx, il, ix] or one [kx, il, ix]"""
    return tg.shape[0] if tg.dim() == 4 else 1


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


SURFACE_LAND_COUPLING, SURFACE_ICE_COUPLING, SURFACE_SST_ANOMALY, SURFACE_DEFAULT = 1, 2, 4, 7
SURFACE_TABLES = ("fmask_l", "fmask_s", "rhcapl", "cdland", "rhcaps", "rhcapi", "cdsea", "cdice")
SURFACE_FIELDS = ("stlcl_ob", "snowdcl_ob", "soilwcl_ob", "stl_lm", "stl_am", "snowd_am", "soilw_am", "sstcl_ob", "sicecl_ob",
                  "ticecl_ob", "sstan_ob", "sst_om", "tice_om", "sice_om", "sst_am", "sstan_am", "sice_am", "tice_am", "ssti_om",
                  "snowc", "alb_l", "alb_s", "albsfc", "corh")


class PlanObject:
    """What the objects made on a plan share (include/spdy.h, "plan"): the handle `h`, its release, and the two-call query of a
    host table.  PREFIX names the C calls.  A handle outlives its plan: once the plan is closed every call but close raises
    SpdyError (SPDY_ERR_STATE), so the objects and their plan may be closed, or collected, in any order."""
    PREFIX = None

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.PREFIX + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _table(self, name):
        """the table as the flat float64 array the library returns"""
        query = getattr(self.lib, self.PREFIX + "_table")
        n = check(query(self.h, name.encode(), None, 0))
        out = np.zeros(n)
        check(query(self.h, name.encode(), _p(out), n))
        return out


class SurfaceModel(PlanObject):
    """The slab land, sea and ice models and the daily forcing on the device (spdy_surface_model_* in include/spdy.h).

    clim: dict of host arrays fmask, alb0 [il, ix]; stl12, snowd12, soilw12, sst12, sice12 [12, il, ix]; sstan3 [3, il, ix] (may
    be absent without SURFACE_SST_ANOMALY).  One step of a run: on the first step of a day forcing_dev(qcorh); the step; the
    host's newdate and, when the day changed, set_date; couple_dev(day, hfluxn, shf, evap, ssrd).

    nmem > 1: the models of an ensemble's members in one object, one launch per call.  What no kernel writes (the constants, the
    climatologies, the date) is held once; every field couple_dev or forcing_dev writes, and fmask_l, is [nmem, il, ix]."""
    PREFIX = "spdy_surface_model"

    def __init__(self, sp, clim, delt, flags=SURFACE_DEFAULT, nmem=1):
        self.sp, self.lib, self.flags, self.nmem = sp, sp.lib, int(flags), int(nmem)
        host, c = {}, SurfaceClim()
        for n in _names("surface_clim"):
            if clim.get(n) is None:
                continue
            host[n] = np.ascontiguousarray(clim[n], np.float64)
            want = shape_of(n, (), sp.kx, sp.grid_shape)
            if host[n].shape != want:
                raise ValueError("%s must have shape %s" % (n, want))
            setattr(c, n, host[n].ctypes.data)
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_ens_surface_model_create(sp.h, self.nmem, ctypes.byref(c), float(delt), self.flags, ctypes.byref(h)))
        self.h = h

    def table(self, name):
        """A host table of land_model_init / sea_model_init (SURFACE_TABLES), [il, ix]."""
        return self._table(name).reshape(self.sp.grid_shape)

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
        physics_dev writes them (None allowed with day == 0); with nmem members [nmem, 2, il, ix] .. [nmem, il, ix], as
        ens_physics_dev writes them."""
        self.sp._sync_stream()
        ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        check(self.lib.spdy_surface_model_couple_dev(self.h, int(day), ptr(hfluxn), ptr(shf), ptr(evap), ptr(ssrd)))

    def forcing_dev(self, qcorh):
        """set_forcing(1) parts 2 and 4: snowc, alb_l, alb_s, albsfc, and qcorh [nx, mx] complex128 (device tensor; with nmem
        members [nmem, nx, mx], one transform call) written."""
        self.sp._sync_stream()
        check(self.lib.spdy_surface_model_forcing_dev(self.h, ctypes.c_void_p(qcorh.data_ptr())))

    def boundary_struct(self):
        """(SfcBoundary of the model's own device arrays, device pointer of albsfc) for the C calls."""
        b, alb = SfcBoundary(), ctypes.c_void_p()
        check(self.lib.spdy_surface_model_boundary(self.h, ctypes.byref(b), ctypes.byref(alb)))
        return b, alb

    def members(self, name=None):
        """How many members hold their own copy of a field: nmem for what a kernel writes and for fmask_l, 1 for a field held
        once; with no name the object's nmem."""
        return check(self.lib.spdy_surface_model_members(self.h, None if name is None else name.encode()))

    def field(self, name):
        """A field of the model by the reference's name (SURFACE_FIELDS, SURFACE_TABLES, alb0): a DeviceField in the model's own
        device memory, [il, ix], or [nmem, il, ix] where a model of nmem > 1 members holds the field per member."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_surface_model_field(self.h, name.encode(), ctypes.byref(p)))
        lead = (self.nmem,) if self.nmem > 1 and self.members(name) > 1 else ()
        return DeviceField(self.sp, p.value, lead + self.sp.grid_shape)

    def boundary(self):
        """(bnd, albsfc) for Spectral.physics_dev: DeviceFields of the model's own arrays (bnd["fmask"] = fmask_l); with nmem
        members the [nmem, il, ix] views Ensemble.step's physics takes."""
        names = {"fmask": "fmask_l", "sst": "sst_am", "stl": "stl_am", "soilw": "soilw_am", "snowc": "snowc", "alb_l": "alb_l",
                 "alb_s": "alb_s"}
        return {k: self.field(v) for k, v in names.items()}, self.field("albsfc")


SPPT_TABLES = ("phi", "f0", "first", "sigma", "mu")
SPPT_FIELDS = ("eta", "spec", "pattern")


class Sppt(PlanObject):
    """The SPPT pattern on the device (spdy_sppt_* in include/spdy.h): gen_sppt of sppt.f90 with a counter-based generator.

    nsteps: steps per day; mu: the taper per level, kx values top down (None = all ones).  One step of a run: advance_dev(), then
    Spectral.physics_sppt_dev(self, ...), which reads the pattern and mu and does not advance.

    nmem > 1 (or seeds given): one pattern per member of an ensemble, member-major, advanced together by the same three launches;
    seeds: one per member (default seed + e), each member drawing what a one-member object with its seed draws.  The step is then
    advance_dev() and Spectral.ens_physics_sppt_dev(nmem, self, ...): Ensemble.step does both when its physics has "sppt"."""
    PREFIX = "spdy_sppt"

    def __init__(self, sp, nsteps, mu=None, seed=0, nmem=1, seeds=None):
        self.sp, self.lib = sp, sp.lib
        if mu is not None:
            mu = np.ascontiguousarray(mu, np.float64)
            if mu.shape != (sp.kx,):
                raise ValueError("mu must hold kx values")
        if seeds is not None and nmem not in (1, len(seeds)):
            raise ValueError("seeds must hold nmem values")
        nmem = int(nmem) if seeds is None else len(seeds)
        if seeds is None:
            seeds = [int(seed) + e for e in range(max(nmem, 0))]
        seeds = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], np.uint64)
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_ens_sppt_create(sp.h, nmem, int(nsteps), None if mu is None else _p(mu), _p(seeds), ctypes.byref(h)))
        self.h, self.nmem = h, nmem

    def table(self, name):
        """A host table (SPPT_TABLES): phi, f0, first as floats, sigma [nx, mx], mu [kx]."""
        out = self._table(name)
        return float(out[0]) if out.size == 1 and name != "mu" else out.reshape((self.sp.nx, self.sp.mx)) if name == "sigma" else out

    def members(self):
        """the number of patterns the object holds"""
        return check(self.lib.spdy_sppt_members(self.h))

    def field(self, name):
        """"eta", "spec" ([kx, nx, mx] complex128, as a DeviceField of [kx, nx, mx, 2] float64) or "pattern" [kx, il, ix]: the
        object's own device memory; the pointers never change.  With nmem > 1 every shape has the members in front: [nmem, kx, ..]."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_sppt_field(self.h, name.encode(), ctypes.byref(p)))
        sp = self.sp
        lead = (self.nmem, sp.kx) if self.nmem > 1 else (sp.kx,)
        return DeviceField(sp, p.value, lead + (sp.grid_shape if name == "pattern" else (sp.nx, sp.mx, 2)))

    def numpy(self, name):
        """A host copy of a field after everything enqueued on the plan's stream: eta and spec as complex128 [kx, nx, mx]
        ([nmem, kx, nx, mx] with nmem > 1)."""
        a = self.field(name).numpy()
        return a if name == "pattern" else a.view(np.complex128)[..., 0]

    def reset(self, seed, member=0):
        """A new seed and draws = 0 for that member only: its next advance is a first one.  Stream-ordered; not during a capture."""
        self.sp._sync_stream()
        check(self.lib.spdy_ens_sppt_reset(self.h, int(member), int(seed)))

    def draws(self, member=0):
        """The member's number of advances since create / reset (downloads the device counter: synchronises the plan's stream)."""
        self.sp._sync_stream()
        n = ctypes.c_longlong()
        check(self.lib.spdy_ens_sppt_draws(self.h, int(member), ctypes.byref(n)))
        return n.value

    def advance_dev(self, eta=None):
        """gen_sppt() for every member: noise (drawn on the device, or eta [kx, nx, mx] / [nmem, kx, nx, mx] complex128 device
        tensor), AR(1) update, the plan's inverse transform, the clip into "pattern"; three launches whatever nmem is; capturable,
        each replay draws new noise."""
        self.sp._sync_stream()
        check(self.lib.spdy_sppt_advance_dev(self.h, None if eta is None else ctypes.c_void_p(eta.data_ptr())))


DIAG_REKE, DIAG_DEKE, DIAG_TEMP_LOW, DIAG_TEMP_HIGH, DIAG_NONFINITE = 1, 2, 4, 8, 16
DIAG_REFERENCE = DIAG_REKE | DIAG_DEKE | DIAG_TEMP_LOW | DIAG_TEMP_HIGH      # what stops the reference (diagnostics.f90:61-62)
DIAG_FIELDS = ("history", "state", "limits")


class DiagnosticsStop(RuntimeError):
    """The state left the accepted range: the reference's `stop 'Model variables out of accepted range'`."""

    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status


class Diagnostics(PlanObject):
    """check_diagnostics on the device (spdy_diagnostics_* in include/spdy.h): per level reke, deke and temp of each checked step
    in a ring of `capacity` rows, the step counter and the sticky first offence, all in device memory.

    One step of a device-resident run: forcing, the step, check_dev on time level 2, couple; status() or raise_if_stopped() once
    per output interval.  check_dev is one launch and capturable: each replay records the next step.

    nmem > 1: the guard of an ensemble's members in one object and one launch.  Every member has its own rows, counter and sticky
    first offence; the limits are shared.  status and read then take the member."""
    PREFIX = "spdy_diagnostics"

    def __init__(self, sp, capacity=64, first_step=0, nmem=1):
        self.sp, self.lib, self.capacity, self.nmem = sp, sp.lib, int(capacity), int(nmem)
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_ens_diagnostics_create(sp.h, self.nmem, self.capacity, int(first_step), ctypes.byref(h)))
        self.h = h

    def set_limits(self, limits=None):
        """reke, deke, temp low, temp high (None = the reference's 500, 500, 180, 320).  Stream-ordered; not during a capture."""
        if limits is not None:
            limits = np.ascontiguousarray(limits, np.float64)
            if limits.shape != (4,):
                raise ValueError("limits must hold four values")
        self.sp._sync_stream()
        check(self.lib.spdy_diagnostics_set_limits(self.h, None if limits is None else _p(limits)))

    def reset(self, next_step=0):
        """A new next step, no offence, an empty history.  Stream-ordered; not during a capture."""
        self.sp._sync_stream()
        check(self.lib.spdy_diagnostics_reset(self.h, int(next_step)))

    def check_dev(self, vor, div, t):
        """One launch on [kx, nx, mx] complex128 device tensors (time level 2 of the prognostics; with nmem members [nmem, kx,
        nx, mx], e.g. ens.vor[1]): the step's row, the range test, the counter."""
        self.sp._sync_stream()
        check(self.lib.spdy_diagnostics_check_dev(self.h, *[ctypes.c_void_p(x.data_ptr()) for x in (vor, div, t)]))

    def status(self, member=0):
        """{"next_step", "bad_step" (-1: nothing tripped), "bad_level", "bad_mask", "bad_row" ([3, kx] or None)} of one member;
        synchronises the plan's stream."""
        self.sp._sync_stream()
        nxt, bad, lev, mask = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
        row = np.zeros((3, self.sp.kx))
        check(self.lib.spdy_ens_diagnostics_status(self.h, int(member), ctypes.byref(nxt), ctypes.byref(bad), ctypes.byref(lev),
                                                   ctypes.byref(mask), _p(row)))
        return {"next_step": nxt.value, "bad_step": bad.value, "bad_level": lev.value, "bad_mask": mask.value,
                "bad_row": row if bad.value >= 0 else None}

    def read(self, step, count=1, member=0):
        """The rows of steps step .. step + count - 1 of one member as [count, 3, kx] (reke | deke | temp); synchronises the
        plan's stream."""
        self.sp._sync_stream()
        rows = np.zeros((int(count), 3, self.sp.kx))
        check(self.lib.spdy_ens_diagnostics_read(self.h, int(member), int(step), int(count), _p(rows)))
        return rows

    def stopped(self):
        """The members' first offending steps, -1 where a member has not tripped: one synchronisation, one download."""
        self.sp._sync_stream()
        bad = (ctypes.c_longlong * self.nmem)()
        check(self.lib.spdy_ens_diagnostics_stopped(self.h, bad))
        return list(bad)

    def use_dev(self, out=None):
        """The members' sticky records as a member mask (include/spdy.h, "member mask"): an int32 device tensor of nmem entries, 1
        where the member has not tripped at any level (stopped() gives -1 there), else 0 -- what Ensemble.analyse, verify and
        output take as `use`.  One launch and no synchronisation; capturable when `out` (such a tensor) is given."""
        import torch
        if out is None:
            out = torch.empty(self.nmem, dtype=torch.int32, device="cuda:%d" % self.sp.device)
        if not torch.is_tensor(out) or out.dtype != torch.int32 or out.numel() != self.nmem or not out.is_contiguous():
            raise ValueError("use_dev: out must be %d contiguous int32 entries" % self.nmem)
        self.sp._sync_stream()
        check(self.lib.spdy_mask_from_diagnostics_dev(self.h, ctypes.c_void_p(out.data_ptr())))
        return out

    def field(self, name):
        """"history" as a DeviceField [capacity, 3, kx] ([capacity, nmem, 3, kx] with nmem > 1 members), "limits" [4]; "state" as
        the device address (per-level records)."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_diagnostics_field(self.h, name.encode(), ctypes.byref(p)))
        if name == "state":
            return p.value
        lead = (self.capacity,) + ((self.nmem,) if self.nmem > 1 else ())
        return DeviceField(self.sp, p.value, lead + (3, self.sp.kx) if name == "history" else (4,))

    def format(self, step, row):
        """The reference's three printed lines (diagnostics.f90:72-74) for one [3, kx] row."""
        return format_diagnostics(self.lib, step, row)

    def raise_if_stopped(self):
        """Raises DiagnosticsStop where the reference would stop: the status holds one of its four comparisons.  The message is
        the reference's three lines and its stop message.  Returns the status otherwise (a non-finite value alone does not stop
        the reference and is left to the caller: status["bad_mask"] & DIAG_NONFINITE).  With nmem > 1 members: the first member
        the reference would have stopped is named in front of its three lines, and the list of every member's status is
        returned otherwise."""
        if self.nmem == 1:
            st = self.status()
            if st["bad_mask"] & DIAG_REFERENCE:
                raise DiagnosticsStop(self.format(st["bad_step"], st["bad_row"]) + "Model variables out of accepted range", st)
            return st
        sts = [self.status(e) if b >= 0 else None for e, b in enumerate(self.stopped())]
        for e, st in enumerate(sts):
            if st is not None and st["bad_mask"] & DIAG_REFERENCE:
                raise DiagnosticsStop(" member %d\n" % e + self.format(st["bad_step"], st["bad_row"])
                                      + "Model variables out of accepted range", dict(st, member=e))
        return [self.status(e) if st is None else st for e, st in enumerate(sts)]


def format_diagnostics(lib, step, row):
    """spdy_diagnostics_format for a [3, kx] row (host only)"""
    row = np.ascontiguousarray(row, np.float64)
    if row.ndim != 2 or row.shape[0] != 3:
        raise ValueError("row must be [3, kx]")
    n = check(lib.spdy_diagnostics_format(row.shape[1], int(step), _p(row), None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    check(lib.spdy_diagnostics_format(row.shape[1], int(step), _p(row), buf, n + 1))
    return buf.value.decode()


class ColumnPhysics:
    """The column-physics calls of a plan (a mixin of spectral.Spectral)."""

    def column_outputs(self, nb, blocks=BLOCKS, names=None):
        """Zero-filled CUDA tensors (torch's current device) for the optional outputs of nb states, the `out` of the ``*_dev`` calls.
        One block ("moist" or ("moist",)): its dict name -> tensor.  Several: a dict block -> such a dict, with all four also "ts"
        and "fsfcu", as column_physics_dev / physics_dev take it.  names: the members wanted (default all)."""
        import torch
        zeros = lambda n: torch.zeros(shape_of(n, (nb,), self.kx, self.grid_shape), dtype=getattr(torch, np.dtype(dtype_of(n)).name),
                                      device="cuda")
        blocks = (blocks,) if isinstance(blocks, str) else tuple(blocks)
        out = {b: {n: zeros(n) for n in _names(b) if names is None or n in names} for b in blocks}
        if len(blocks) == 1:
            return out[blocks[0]]
        if set(blocks) == set(BLOCKS):
            out.update({n: zeros(n) for n in _names("column_physics")})
        return out

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
        sfc = RadSurface(self._dp(fmask), self._dp(albsfc))
        check(self.lib.spdy_radiation_down_dev(self.h, _nb(tg), 1 if compute_sw else 0, *[self._dp(x) for x in (tg, qg, phig, pslg, rh,
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
        them) and optional tensors "ts", "fsfcu" (column_outputs makes one)."""
        self._sync_stream()
        o = self._column_physics_out(out)
        b = self._boundary(bnd)
        check(self.lib.spdy_column_physics_dev(self.h, _nb(tg), 1 if compute_sw else 0, *[self._dp(x) for x in (ug, vg, tg, qg, phig,
                                               pslg)], ctypes.byref(b), self._dp(albsfc),
                                               self._dp(state), *[self._dp(x) for x in (utend, vtend, ttend, qtend)], ctypes.byref(o)))

    def _column_physics_out(self, out):
        out = out or {}
        return ColumnPhysicsOut(*[_out_struct(OUT_STRUCTS[b], out.get(b)) for b in BLOCKS],
                                *[self._dp(out.get(n)) for n in _names("column_physics")])

    def physics_workspace(self):
        check(self.lib.spdy_physics_workspace(self.h))

    def _physics(self, fn, lead, compute_sw, spectra, bnd, albsfc, state, tends, out):
        """The marshalling of the physics-from-spectra calls: the C function, its leading arguments, the shared ones."""
        self._sync_stream()
        o = self._column_physics_out(out)
        b = self._boundary(bnd)
        check(fn(self.h, *lead, 1 if compute_sw else 0, *[self._dp(x) for x in spectra], ctypes.byref(b), self._dp(albsfc),
                 self._dp(state), *[self._dp(x) for x in tends], ctypes.byref(o)))

    def physics_dev(self, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, state, utend, vtend, ttend, qtend, out=None):
        """physics.f90:94-205 on one state from its spectra (time level 1: vor, div, t, q, phi [kx,nx,mx], ps [nx,mx] complex128):
        one inverse launch into plan workspace, then the column physics (one launch, or the five calls with the plan option
        "physics_fused" 0).  utend, vtend, ttend, qtend [kx,il,ix] in place; bnd, albsfc, state and out as column_physics_dev."""
        self._physics(self.lib.spdy_physics_dev, (), compute_sw, (vor, div, t, q, phi, ps), bnd, albsfc, state,
                      (utend, vtend, ttend, qtend), out)

    def ens_physics_workspace(self, nmem):
        check(self.lib.spdy_ens_physics_workspace(self.h, int(nmem)))

    def ens_physics_dev(self, nmem, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, state, utend, vtend, ttend, qtend, out=None):
        """physics_dev for nmem members (ensemble.py's layout): time level 1 of all members, vor, div, t, q, phi [nmem,kx,nx,mx], ps
        [nmem,nx,mx]; ONE inverse launch, then the column physics with nb = nmem.  utend .. qtend [nmem,kx,il,ix] in place; the fields
        of bnd, albsfc, state and out are per member, back to back, as column_physics_dev takes them for nb states."""
        self._physics(self.lib.spdy_ens_physics_dev, (int(nmem),), compute_sw, (vor, div, t, q, phi, ps), bnd, albsfc, state,
                      (utend, vtend, ttend, qtend), out)

    # ------------------------------------------------------------------ SPPT (physics.f90:85-88, :207-222)
    def column_physics_sppt_workspace(self):
        check(self.lib.spdy_column_physics_sppt_workspace(self.h))

    def physics_sppt_workspace(self):
        check(self.lib.spdy_physics_sppt_workspace(self.h))

    def column_physics_sppt_dev(self, pattern, mu, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, state, utend, vtend, ttend,
                                qtend, out=None):
        """column_physics_dev followed by SPPT: pattern [nb,kx,il,ix] (device, clipped), mu kx host values top down (None = 1);
        each tendency becomes (1 + pattern*mu(k))*(tend - tend_dyn) + tend_dyn with tend_dyn its value at entry."""
        self._sync_stream()
        o = self._column_physics_out(out)
        b = self._boundary(bnd)
        if mu is not None:
            mu = np.ascontiguousarray(mu, np.float64)
            if mu.shape != (self.kx,):
                raise ValueError("mu must hold kx values")
        check(self.lib.spdy_column_physics_sppt_dev(self.h, _nb(tg), self._dp(pattern), None if mu is None else _p(mu),
                                                    1 if compute_sw else 0, *[self._dp(x) for x in (ug, vg, tg, qg, phig, pslg)],
                                                    ctypes.byref(b), self._dp(albsfc), self._dp(state),
                                                    *[self._dp(x) for x in (utend, vtend, ttend, qtend)], ctypes.byref(o)))

    def physics_sppt_dev(self, sppt, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, state, utend, vtend, ttend, qtend, out=None):
        """physics_dev followed by SPPT with the current pattern and the mu of sppt (a Sppt of this plan), which is not advanced:
        call sppt.advance_dev() first."""
        self._physics(self.lib.spdy_physics_sppt_dev, (sppt.h,), compute_sw, (vor, div, t, q, phi, ps), bnd, albsfc, state,
                      (utend, vtend, ttend, qtend), out)

    def ens_physics_sppt_workspace(self, nmem):
        check(self.lib.spdy_ens_physics_sppt_workspace(self.h, int(nmem)))

    def ens_physics_sppt_dev(self, nmem, sppt, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, state, utend, vtend, ttend, qtend,
                             out=None):
        """ens_physics_dev followed by SPPT, each member with its own current pattern of sppt (a Sppt of this plan with nmem members)
        and the shared mu; sppt is not advanced: call sppt.advance_dev() first."""
        self._physics(self.lib.spdy_ens_physics_sppt_dev, (int(nmem), sppt.h), compute_sw, (vor, div, t, q, phi, ps), bnd, albsfc, state,
                      (utend, vtend, ttend, qtend), out)

    # ------------------------------------------------------------------ NumPy conveniences: inputs and results by name, shaped by FIELDS
    def _grid_args(self, ins, ref="tg"):
        """ins (name -> array) as contiguous arrays of FIELDS' dtypes, shapes checked against the level stack ins[ref].  Returns
        (ins, the leading (batch) shape, nb)."""
        ins = {k: np.ascontiguousarray(v, dtype_of(k)) for k, v in ins.items()}
        grid3 = ins[ref].shape
        if grid3[-3:] != (self.kx,) + self.grid_shape:
            raise ValueError("%s must be [nb,] kx, il, ix" % ref)
        lead = grid3[:-3]
        for k, v in ins.items():
            want = shape_of(k, lead, self.kx, self.grid_shape)
            if v.shape != want:
                raise ValueError("%s must have shape %s" % (k, want))
        return ins, lead, int(np.prod(lead)) if lead else 1

    def _results(self, names, lead):
        return {n: np.empty(shape_of(n, lead, self.kx, self.grid_shape), dtype_of(n)) for n in names}

    def _radiation_state(self, state, nb, compute_sw):
        """The radiation state of nb model states to start a call from: `state`, or a fresh one (zeros) for None."""
        nst = self.radiation_state_size() * nb
        if state is None and not compute_sw:
            raise ValueError("the first call on a radiation state must have compute_sw set")
        st = np.zeros(nst) if state is None else np.ascontiguousarray(state, np.float64)
        if st.shape != (nst,):
            raise ValueError("state must hold %d doubles" % nst)
        return st

    def moist_columns(self, tg, qg, phig, pslg, ttend, qtend):
        """NumPy convenience: spdy_moist_columns_dev on copies in plan-owned device memory.  Returns a dict with the updated
        ttend, qtend and every optional output (shapes as the inputs; iptop / icnv int32)."""
        ins, lead, nb = self._grid_args(dict(tg=tg, qg=qg, phig=phig, pslg=pslg, ttend=ttend, qtend=qtend))
        res = self._results(("ttend", "qtend") + _names("moist"), lead)

        def call(d):
            check(self.lib.spdy_moist_columns_dev(self.h, nb, *[d[n] for n in ins], ctypes.byref(_struct_of(MoistOut, d))))
        return self._on_device(ins, res, call)

    def radiation_columns(self, tg, qg, phig, pslg, rh, precnv, precls, iptop, fmask, albsfc, ts, fsfcu, ttend, compute_sw=True,
                          state=None):
        """NumPy convenience: both radiation halves on copies in plan-owned device memory.  Shapes as radiation_down_dev (NumPy).
        state: the radiation state to start from (as returned under "state"); None starts a fresh one (then compute_sw must be
        set).  Returns a dict with the updated ttend, every optional output (those of the shortwave only with compute_sw) and the
        updated state."""
        ins = dict(tg=tg, qg=qg, phig=phig, pslg=pslg, ts=ts, fsfcu=fsfcu, ttend=ttend)
        if compute_sw:
            ins.update(rh=rh, precnv=precnv, precls=precls, fmask=fmask, albsfc=albsfc, iptop=iptop)
        ins, lead, nb = self._grid_args(ins)
        ins["state"] = self._radiation_state(state, nb, compute_sw)
        res = self._results(RAD_2D + ("tt_rlw",) + ((RAD_SW_2D + ("tt_rsw",)) if compute_sw else ()) + ("ttend",), lead)
        res["state"] = np.empty_like(ins["state"])

        def call(d):
            o, sfc = _struct_of(RadOut, d), _struct_of(RadSurface, d)
            check(self.lib.spdy_radiation_down_dev(self.h, nb, 1 if compute_sw else 0, *[d.get(n) for n in ("tg", "qg", "phig", "pslg",
                                                   "rh", "precnv", "precls", "iptop")], ctypes.byref(sfc), d["state"], ctypes.byref(o)))
            check(self.lib.spdy_radiation_up_dev(self.h, nb, d["tg"], d["pslg"], d["ts"], d["fsfcu"], d["state"], d["ttend"],
                                                 ctypes.byref(o)))
        return self._on_device(ins, res, call)

    def surface_columns(self, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd):
        """NumPy convenience: spdy_surface_fluxes_dev on copies in plan-owned device memory.  bnd: dict of the SFC_BOUNDARY fields.
        Returns a dict with ts, fsfcu, flux3 [nb,4,il,ix] and every optional output."""
        ins = dict(ug=ug, vg=vg, tg=tg, qg=qg, phig=phig, pslg=pslg, ssrd=ssrd, slrd=slrd, **{n: bnd[n] for n in SFC_BOUNDARY})
        ins, lead, nb = self._grid_args(ins)
        res = self._results(_names("sfc") + ("ts", "fsfcu", "flux3"), lead)

        def call(d):
            check(self.lib.spdy_surface_fluxes_dev(self.h, nb, *[d[n] for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "ssrd", "slrd")],
                                                   ctypes.byref(_struct_of(SfcBoundary, d)), d["ts"], d["fsfcu"], d["flux3"],
                                                   ctypes.byref(_struct_of(SfcOut, d))))
        return self._on_device(ins, res, call)

    def pbl_columns(self, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend):
        """NumPy convenience: spdy_pbl_dev on copies in plan-owned device memory.  Returns a dict with the updated utend, vtend,
        ttend, qtend and every optional output."""
        ins = dict(qg=qg, phig=phig, pslg=pslg, se=se, rh=rh, qsat=qsat, icnv=icnv, flux3=flux3, utend=utend, vtend=vtend,
                   ttend=ttend, qtend=qtend)
        ins, lead, nb = self._grid_args(ins, "qg")
        res = self._results(_TEND + _names("pbl"), lead)

        def call(d):
            check(self.lib.spdy_pbl_dev(self.h, nb, *[d[n] for n in ins], ctypes.byref(_struct_of(PblOut, d))))
        return self._on_device(ins, res, call)

    def column_physics(self, ug, vg, tg, qg, phig, pslg, bnd, albsfc, utend, vtend, ttend, qtend, compute_sw=True, state=None):
        """NumPy convenience: spdy_column_physics_dev on copies in plan-owned device memory.  state: the radiation state to start
        from (as returned under "state"); None starts a fresh one (then compute_sw must be set).  On calls without shortwave the
        plan's workspace holds the ssrd of the last call with it.  Returns a dict with the updated tendencies, every optional
        output of every block (those of the shortwave only with compute_sw) and the updated state."""
        ins = dict(ug=ug, vg=vg, tg=tg, qg=qg, phig=phig, pslg=pslg, utend=utend, vtend=vtend, ttend=ttend, qtend=qtend,
                   **{n: bnd[n] for n in SFC_BOUNDARY})
        if compute_sw:
            ins["albsfc"] = albsfc
        ins, lead, nb = self._grid_args(ins)
        ins["state"] = self._radiation_state(state, nb, compute_sw)
        skip = ("ssrd",) + (() if compute_sw else RAD_SW_2D + ("tt_rsw",))       # ssrd stays in the plan's workspace
        outs = tuple(n for b in BLOCKS for n in _names(b) if b != "rad" or n not in skip) + _names("column_physics")
        res = self._results(_TEND + outs, lead)
        res["state"] = np.empty_like(ins["state"])

        def call(d):
            o = _struct_of(ColumnPhysicsOut, d)
            check(self.lib.spdy_column_physics_dev(self.h, nb, 1 if compute_sw else 0, *[d[n] for n in ("ug", "vg", "tg", "qg", "phig",
                                                   "pslg")], ctypes.byref(_struct_of(SfcBoundary, d)), d.get("albsfc"), d["state"],
                                                   *[d[n] for n in _TEND], ctypes.byref(o)))
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
