"""The surface models on the device (include/spdy.h: spdy_surface_model_*) against the restatement tests/surfmodel.py, on full
grids at T30 L8 and T63 L16: after couple(0), the first forcing and every step of the three date windows (tmonth crossing 0.5, a
month change with obs_ssta, the turn of the year) every field of spdy_surface_model_field, the boundary arrays and albsfc agree
within TOL, and qcorh agrees with the oracle's grid_to_spec of the restated corh.  Each coupling flag at 0 and at 1; a captured
couple_dev replayed across a date change and two runs are bit-equal; the error codes of the header."""
import ctypes

import numpy as np
import pytest

import longrun
import physstep
import support
import surfmodel as sm
import synth
from conftest import TOL

pytestmark = pytest.mark.gpu

ARG, NO_DEVICE, STATE = -1, -3, -5


def shaped(c, shape):
    return {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + shape) for k, v in c.items()}


def setup(tag, start, flags=sm.DEFAULT, sp=None):
    s = support.package()
    sp = sp or support.plan(tag, max_batch=4)
    phis0 = sm.orography(sp)
    sp.surface_set_orography(phis0)
    lat = longrun.latitudes(sp.table("sia_half"))
    c = sm.climatology(phis0, lat, start=start[:2])
    n = phis0.size
    tab = sm.tables(c["fmask"], c["alb0"], sp.table("sia_half"), sp.ix)
    ref = sm.Model(c, tab, flags, ssta=sm.ssta_reader(c["fmask"]))
    dev = s.SurfaceModel(sp, shaped(c, sp.grid_shape), sm.DELT, flags)
    return sp, phis0, ref, dev


def agree(x, ref, what):
    if not np.abs(ref).max() > 0.0:
        assert not np.any(x), what
        return 0.0
    e = synth.relerr(x, ref)
    assert e <= TOL, (what, e)
    return e


class Driver:
    """issues the device calls of one run in the order of include/spdy.h next to surfmodel.run, and compares as it goes"""

    def __init__(self, sp, ref, dev, oracle=None, compare=True):
        import torch
        self.sp, self.ref, self.dev, self.o, self.compare = sp, ref, dev, oracle, compare
        il, ix = sp.grid_shape
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
        self.flux = {"hfluxn": z(2, il, ix), "shf": z(3, il, ix), "evap": z(3, il, ix), "ssrd": z(il, ix)}
        self.qcorh = torch.zeros(sp.spec_shape, dtype=torch.complex128, device="cuda")
        self.day_key, self.worst, self.log = None, 0.0, []

    def load_flux(self, flux):
        import torch
        for k, t in self.flux.items():
            t.copy_(torch.from_numpy(np.ascontiguousarray(flux[k]).reshape(t.shape)))
        torch.cuda.synchronize()

    def couple(self, day):
        self.dev.couple_dev(day, **(self.flux if day else {}))

    def on_step(self, model_step, day, date, flux, shifted):
        if date.key() != self.day_key:                       # the host's newdate: the day changed
            self.dev.set_date(date.imont1, date.tmonth, date.tyear)
            self.day_key = date.key()
        if shifted:
            self.dev.set_sst_anomaly(self.ref.sstan3.reshape((3,) + self.sp.grid_shape))
        if day:
            self.load_flux(flux)
        self.couple(day)
        self.check(sm.FIELDS, "step %d (day %d, %s)" % (model_step, day, date.key()))

    def on_forcing(self, model_step, date):
        import torch
        self.dev.forcing_dev(self.qcorh)
        where = "forcing before step %d" % model_step
        self.check(sm.FORCING, where)
        if not self.compare:
            self.log.append(self.qcorh.cpu().numpy().copy())
            return
        bnd, albsfc = self.dev.boundary()
        want = self.ref.boundary()
        for k, t in bnd.items():
            self.worst = max(self.worst, agree(t.numpy().reshape(-1), want[k], "%s: boundary %s" % (where, k)))
        agree(albsfc.numpy().reshape(-1), want["albsfc"], where + ": albsfc")
        q = self.qcorh.cpu().numpy()
        self.worst = max(self.worst, agree(q, self.o.grid_to_spec(self.ref.f["corh"].reshape(self.sp.grid_shape)), where + ": qcorh"))

    def check(self, names, where):
        for k in names:
            x = self.dev.field(k).numpy().reshape(-1)
            if self.compare:
                self.worst = max(self.worst, agree(x, self.ref.f[k], "%s: %s" % (where, k)))
            else:
                self.log.append(x)


def run_window(tag, wname, flags, oracle, compare=True, driver=Driver):
    start = sm.WINDOWS[wname]
    sp, phis0, ref, dev = setup(tag, start, flags)
    d = driver(sp, ref, dev, oracle, compare)
    n = phis0.size
    sm.run(ref, start, sm.WINDOW_STEPS, phis0.reshape(-1), lambda k: sm.fluxes(k, n), d.on_forcing, d.on_step)
    dev.close()
    sp.close()
    return d, ref


@pytest.mark.parametrize("wname", list(sm.WINDOWS))
@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_windows_match_restatement(tag, wname, oracle_factory):
    d, ref = run_window(tag, wname, sm.DEFAULT, oracle_factory(tag))
    print("[surfmodel %s %s] worst relative error %.2e, freezing-point margin %.2e" % (tag, wname, d.worst, ref.margin))
    assert ref.margin >= physstep.RUN_MARGIN                 # no column near sstcl_ob = sstfr, where sice jumps
    assert all(v.any() for v in ref.branch.values())


@pytest.mark.parametrize("flags", [sm.DEFAULT & ~sm.LAND, sm.DEFAULT & ~sm.ICE, sm.DEFAULT & ~sm.SSTAN, 0])
@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_flags_off(tag, flags, oracle_factory):
    """each coupling flag at 0 (the windows above have them at 1), over the month change where obs_ssta runs"""
    d, ref = run_window(tag, "month", flags, oracle_factory(tag))
    if not flags & sm.LAND:
        assert np.array_equal(ref.f["stl_am"], ref.f["stlcl_ob"])
    if not flags & sm.SSTAN:
        assert not ref.f["sstan_am"].any()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_two_runs_bit_equal(tag):
    a, _ = run_window(tag, "month", sm.DEFAULT, None, compare=False)
    b, _ = run_window(tag, "month", sm.DEFAULT, None, compare=False)
    assert len(a.log) == len(b.log) > 0
    for x, y in zip(a.log, b.log):
        assert np.array_equal(x, y)


class GraphDriver(Driver):
    """couple_dev(day > 0) captured once and replayed for every later step, the date changing between replays"""
    graph = None

    def couple(self, day):
        if not day:
            return Driver.couple(self, day)
        if self.graph is None:
            with self.sp.graph_capture() as g:
                Driver.couple(self, day)
            self.graph = g
            self.nodes = g.num_nodes()
        self.graph.launch()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_captured_couple_across_date_change(tag):
    eager, _ = run_window(tag, "month", sm.DEFAULT, None, compare=False)
    graph, _ = run_window(tag, "month", sm.DEFAULT, None, compare=False, driver=GraphDriver)
    assert graph.nodes == 1                                  # the step graph's node count + 1
    assert len(eager.log) == len(graph.log) > 0
    for x, y in zip(eager.log, graph.log):
        assert np.array_equal(x, y)
    graph.graph.close()


def test_error_codes():
    import torch
    s = support.package()
    start = sm.WINDOWS["month"]
    sp, phis0, ref, dev = setup("t30", start)
    il, ix = sp.grid_shape
    lib, code = sp.lib, lambda e: e.value.code
    q = torch.zeros(sp.spec_shape, dtype=torch.complex128, device="cuda")
    fl = {"hfluxn": torch.zeros(2, il, ix, dtype=torch.float64, device="cuda"), "shf": torch.zeros(3, il, ix, dtype=torch.float64, device="cuda"),
          "evap": torch.zeros(3, il, ix, dtype=torch.float64, device="cuda"), "ssrd": torch.zeros(il, ix, dtype=torch.float64, device="cuda")}
    # before set_date
    for call in (lambda: dev.couple_dev(0), lambda: dev.forcing_dev(q)):
        with pytest.raises(s.SpdyError) as e:
            call()
        assert code(e) == STATE
    d = sm.Date(*start)
    dev.set_date(d.imont1, d.tmonth, d.tyear)
    # before couple(0)
    for call in (lambda: dev.couple_dev(1, **fl), lambda: dev.forcing_dev(q)):
        with pytest.raises(s.SpdyError) as e:
            call()
        assert code(e) == STATE
    dev.couple_dev(0)
    # NULL required pointers
    with pytest.raises(s.SpdyError) as e:
        dev.couple_dev(1, fl["hfluxn"], fl["shf"], None, fl["ssrd"])
    assert code(e) == ARG
    assert lib.spdy_surface_model_forcing_dev(dev.h, None) == ARG
    assert lib.spdy_surface_model_couple_dev(None, 0, None, None, None, None) == ARG
    assert lib.spdy_surface_model_set_sst_anomaly(dev.h, None) == ARG
    assert lib.spdy_surface_model_boundary(dev.h, None, None) == ARG
    assert lib.spdy_surface_model_field(dev.h, b"no_such_field", ctypes.byref(ctypes.c_void_p())) == ARG
    h = ctypes.c_void_p()
    assert lib.spdy_surface_model_create(sp.h, None, sm.DELT, 7, ctypes.byref(h)) == ARG
    with pytest.raises(s.SpdyError) as e:
        dev.set_date(13, 0.5, 0.5)
    assert code(e) == ARG
    # a tyear that is refused leaves the interpolation date as it was
    before = dev.field("stlcl_ob").numpy()
    with pytest.raises(s.SpdyError) as e:
        dev.set_date(7, 0.25, float("nan"))
    assert code(e) == ARG
    dev.couple_dev(1, **fl)
    assert np.array_equal(dev.field("stlcl_ob").numpy(), before)
    # create: an unknown flag bit; no sstan3 under SPDY_SURFACE_SST_ANOMALY (and accepted without that flag)
    c = sm.climatology(phis0, longrun.latitudes(sp.table("sia_half")), start=start[:2])
    with pytest.raises(s.SpdyError) as e:
        s.SurfaceModel(sp, shaped(c, sp.grid_shape), sm.DELT, 8)
    assert code(e) == ARG
    c.pop("sstan3")
    with pytest.raises(s.SpdyError) as e:
        s.SurfaceModel(sp, shaped(c, sp.grid_shape), sm.DELT, sm.DEFAULT)
    assert code(e) == ARG
    s.SurfaceModel(sp, shaped(c, sp.grid_shape), sm.DELT, sm.DEFAULT & ~sm.SSTAN).close()
    # forcing needs the orography; couple(0) cannot be recorded (it must have run before anything relies on it)
    bare = support.plan("t30", max_batch=4)
    c["sstan3"] = np.zeros((3, phis0.size))
    bm = s.SurfaceModel(bare, shaped(c, bare.grid_shape), sm.DELT)
    bm.set_date(d.imont1, d.tmonth, d.tyear)
    with pytest.raises(s.SpdyError) as e:
        with bare.graph_capture():
            bm.couple_dev(0)
    assert code(e) == STATE
    bm.couple_dev(0)
    with pytest.raises(s.SpdyError) as e:
        bm.forcing_dev(q)
    assert code(e) == STATE
    bm.close()
    bare.close()
    # set_date is refused while a capture is open
    sp.use_own_stream()
    with pytest.raises(s.SpdyError) as e:
        with sp.graph_capture():
            dev.set_date(d.imont1, d.tmonth, d.tyear)
    assert code(e) == STATE
    dev.couple_dev(1, **fl)                                  # and the model is usable again
    sp.synchronize()
    # a host-only plan: the tables exist, every device call is refused
    hp = support.plan("t30", max_batch=4, device=-1)
    c = sm.climatology(phis0, longrun.latitudes(hp.table("sia_half")), start=start[:2])
    hm = s.SurfaceModel(hp, shaped(c, hp.grid_shape), sm.DELT)
    assert np.array_equal(hm.table("cdsea"), dev.table("cdsea"))
    for call in (lambda: lib.spdy_surface_model_set_date(hm.h, 1, 0.5, 0.04), lambda: lib.spdy_surface_model_couple_dev(hm.h, 0, None, None, None, None),
                 lambda: lib.spdy_surface_model_forcing_dev(hm.h, ctypes.c_void_p(q.data_ptr()))):
        assert call() == NO_DEVICE
    hm.close()
    hp.close()
    dev.close()
    sp.close()
