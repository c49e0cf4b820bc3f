"""CPU: the lifetime rule of the objects made on a plan (include/spdy.h, the plan section), on a host-only T30 L8 plan.  A surface
model, an SPPT pattern, a diagnostics object and an analysis object each outlive their plan as a dead handle: every entry point
but _destroy returns SPDY_ERR_STATE and names the destroyed plan, _destroy returns SPDY_OK.  The entry points are taken from the
binding's table by prefix, so one that is added later is covered or the test says which arguments it lacks."""
import ctypes

import numpy as np
import pytest

import longrun
import surfmodel as sm
from support import package

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -3, -5
KX, MAX_BATCH, NMEM = 8, 64, 2
PREFIXES = {"surface_model": ("spdy_surface_model_", "spdy_ens_surface_model_"), "sppt": ("spdy_sppt_", "spdy_ens_sppt_"),
            "diagnostics": ("spdy_diagnostics_", "spdy_ens_diagnostics_"), "letkf": ("spdy_letkf_", "spdy_ens_letkf_")}
NO_HANDLE = {"spdy_diagnostics_format"}          # formats a row the caller passes: takes no object
NULL_TEXT = {"surface_model": b"null surface model", "sppt": b"null SPPT pattern", "diagnostics": b"null diagnostics object",
             "letkf": b"null analysis object"}


def entry_points(kind):
    """every call of the kind that the binding declares, but its _create and _destroy forms"""
    names = [n for n in package()._lib.SIGNATURES if n.startswith(PREFIXES[kind]) and n not in NO_HANDLE]
    return sorted(n for n in names if not n.endswith(("_create", "_destroy")))


class Args:
    """host buffers that stay alive for the test, and the arguments after the handle of every entry point: valid on a live plan"""

    def __init__(self):
        self.buf = np.zeros(4096)
        self.q = self.buf.ctypes.data_as(ctypes.c_void_p)      # a non-null "device pointer": no check dereferences one
        self.ll = [ctypes.c_longlong() for _ in range(2)]
        self.i = [ctypes.c_int() for _ in range(2)]
        self.ptr = ctypes.c_void_p()
        self.bnd = package().spectral.SfcBoundary()
        self.obs = (package().letkf.Obs * 1)(package().letkf.Obs(2, 3, 10.0, 20.0, 250.0, 1.0))
        q, ll, i, ref = self.q, self.ll, self.i, ctypes.byref
        self.of = {
            "spdy_surface_model_members": (None,),
            "spdy_surface_model_table": (b"fmask_l", None, 0),
            "spdy_surface_model_set_date": (1, 0.5, 0.04),
            "spdy_surface_model_set_sst_anomaly": (q,),
            "spdy_surface_model_couple_dev": (0, None, None, None, None),
            "spdy_surface_model_forcing_dev": (q,),
            "spdy_surface_model_boundary": (ref(self.bnd), ref(self.ptr)),
            "spdy_surface_model_field": (b"sst_am", ref(self.ptr)),
            "spdy_sppt_members": (),
            "spdy_sppt_reset": (7,),
            "spdy_ens_sppt_reset": (1, 7),
            "spdy_sppt_table": (b"sigma", None, 0),
            "spdy_sppt_field": (b"pattern", ref(self.ptr)),
            "spdy_sppt_draws": (ref(ll[0]),),
            "spdy_ens_sppt_draws": (1, ref(ll[0])),
            "spdy_sppt_advance_dev": (None,),
            "spdy_diagnostics_set_limits": (None,),
            "spdy_diagnostics_reset": (0,),
            "spdy_diagnostics_check_dev": (q, q, q),
            "spdy_diagnostics_status": (ref(ll[0]), ref(ll[1]), ref(i[0]), ref(i[1]), q),
            "spdy_ens_diagnostics_status": (1, ref(ll[0]), ref(ll[1]), ref(i[0]), ref(i[1]), q),
            "spdy_diagnostics_read": (0, 1, q),
            "spdy_ens_diagnostics_read": (1, 0, 1, q),
            "spdy_ens_diagnostics_stopped": (ref(ll[0]),),
            "spdy_diagnostics_field": (b"history", ref(self.ptr)),
            "spdy_letkf_set_localization": (1.0e6, 0.0, 1.0),
            "spdy_letkf_set_obs": (1, ctypes.cast(self.obs, ctypes.c_void_p)),
            "spdy_letkf_set_weight_stride": (2, 2),
            "spdy_letkf_table": (b"unit", None, 0),
            "spdy_letkf_field": (b"hx", ref(self.ptr)),
            "spdy_letkf_analyse_grid_dev": (q,) * 10,
            "spdy_ens_letkf_dev": (q,) * 5,
        }


@pytest.fixture(scope="module")
def clim(oracle_factory):
    s = package()
    sp = s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=-1)
    c = sm.climatology(sm.orography(oracle_factory("t30")), longrun.latitudes(sp.table("sia_half")))
    c = {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + sp.grid_shape) for k, v in c.items()}
    sp.close()
    return c


def make(kind, sp, clim):
    """the object of the kind on sp; members where the kind has them.  The single-member calls of a kind that checks the member
    count before the device (spdy_diagnostics_status, _read) get an object of one member."""
    s = package()
    if kind == "surface_model":
        return {"": s.SurfaceModel(sp, clim, sm.DELT, nmem=NMEM)}
    if kind == "sppt":
        return {"": s.Sppt(sp, 36, nmem=NMEM)}
    if kind == "diagnostics":
        return {"": s.Diagnostics(sp, capacity=4, nmem=NMEM), "single": s.Diagnostics(sp, capacity=4)}
    return {"": s.Letkf(sp, NMEM, 4, 1.0e6)}


def handle_for(objs, name):
    return objs["single" if name in ("spdy_diagnostics_status", "spdy_diagnostics_read") else ""].h


@pytest.mark.parametrize("kind", list(PREFIXES))
def test_every_entry_point_of_a_dead_object_is_refused(kind, clim):
    s = package()
    lib, a = s.load(), Args()
    names = entry_points(kind)
    assert names and not [n for n in names if n not in a.of], "entry points without arguments in this test"
    sp = s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=-1)
    objs = make(kind, sp, clim)
    # the arguments are valid while the plan lives: the call succeeds, or reaches the check of the device, which comes last
    for n in names:
        rc = getattr(lib, n)(handle_for(objs, n), *a.of[n])
        assert rc >= 0 or rc == ERR_NO_DEVICE, (n, rc, lib.spdy_last_error())
    assert lib.spdy_plan_destroy(sp.h) == OK
    sp.h = None
    for n in names:
        rc = getattr(lib, n)(handle_for(objs, n), *a.of[n])
        assert rc == ERR_STATE, (n, rc, lib.spdy_last_error())
        assert b"has been destroyed" in lib.spdy_last_error() and b"plan" in lib.spdy_last_error(), n
    for o in objs.values():
        assert getattr(lib, o.PREFIX + "_destroy")(o.h) == OK
        o.h = None


@pytest.mark.parametrize("kind", list(PREFIXES))
def test_null_handle_keeps_its_code_and_text(kind):
    lib, a = package().load(), Args()
    n = {"surface_model": "spdy_surface_model_field", "sppt": "spdy_sppt_members", "diagnostics": "spdy_diagnostics_reset",
         "letkf": "spdy_letkf_table"}[kind]
    assert getattr(lib, n)(None, *a.of[n]) == ERR_ARG
    assert lib.spdy_last_error() == NULL_TEXT[kind]


def test_dead_pattern_in_the_physics_calls():
    """spdy_physics_sppt_dev and spdy_ens_physics_sppt_dev on a live plan with the pattern of a destroyed one"""
    s = package()
    lib, a = s.load(), Args()
    sp, gone = (s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=-1) for _ in range(2))
    sp.radiation_set_date(0.0)
    sp.surface_set_orography(np.zeros(sp.grid_shape))
    one, two = s.Sppt(gone, 36), s.Sppt(gone, 36, nmem=NMEM)
    gone.close()
    q = a.q
    bnd, out = s.spectral.SfcBoundary(*[q] * 7), s.spectral.ColumnPhysicsOut()
    tail = (1,) + (q,) * 6 + (ctypes.byref(bnd),) + (q,) * 6 + (ctypes.byref(out),)
    assert lib.spdy_physics_sppt_dev(sp.h, one.h, *tail) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    assert lib.spdy_ens_physics_sppt_dev(sp.h, NMEM, two.h, *tail) == ERR_STATE and b"has been destroyed" in lib.spdy_last_error()
    one.close(); two.close(); sp.close()


def test_a_failing_create_leaves_the_plan_usable(clim):
    """creates that fail after the object has joined its plan: the plan serves the next create and is destroyed with SPDY_OK"""
    s = package()
    lib = s.load()
    sp = s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=-1)
    h = ctypes.c_void_p()
    seed = (ctypes.c_ulonglong * 1)(1)
    assert lib.spdy_ens_sppt_create(sp.h, 1, 0, None, seed, ctypes.byref(h)) == ERR_ARG and not h.value          # nsteps refused
    with pytest.raises(s.SpdyError) as e:
        s.SurfaceModel(sp, clim, 0.0)                                                                          # delt refused
    assert e.value.code == ERR_ARG
    small = s.Spectral("t30", kx=KX, max_batch=NMEM * (2 * KX + 1) - 1, device=-1)
    assert lib.spdy_letkf_create(small.h, NMEM, 4, ctypes.byref(h)) == ERR_ARG and b"max_batch" in lib.spdy_last_error()
    for _ in range(3):
        objs = [o for kind in PREFIXES for o in make(kind, sp, clim).values()]
        assert objs[1].table("sigma").shape == (sp.nx, sp.mx)
        for o in objs[::2]:
            o.close()                                    # some before the plan's end, the others after it
    assert lib.spdy_plan_destroy(sp.h) == OK and lib.spdy_plan_destroy(small.h) == OK
    sp.h = small.h = None
    for o in objs:
        o.close()
