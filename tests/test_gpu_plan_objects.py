"""GPU: a plan closed while a surface model, an SPPT pattern, a diagnostics object, an analysis object and a graph that holds a call
of each are alive (include/spdy.h, the plan section).  Every later call on the five handles is refused with SPDY_ERR_STATE before
it touches the device, closing them raises nothing, and a fresh plan transforms as before.  tests/test_plan_objects_cpu.py and the
host check tools/object_lifetime_check.c establish the same on a host-only plan, call by call."""
import numpy as np
import pytest

import longrun
import support
import surfmodel as sm
import synth
from conftest import TOL

pytestmark = pytest.mark.gpu
STATE = -5
KX, MAX_BATCH, NMEM = 8, 64, 2


def test_plan_closed_before_its_objects_and_their_graph(oracle_factory):
    import torch
    s = support.package()
    sp = s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=0)
    # one object of each kind, each where its capturable call is legal
    phis0 = sm.orography(sp)
    sp.surface_set_orography(phis0)
    c = sm.climatology(phis0, longrun.latitudes(sp.table("sia_half")))
    model = s.SurfaceModel(sp, {k: np.ascontiguousarray(v).reshape(v.shape[:-1] + sp.grid_shape) for k, v in c.items()}, sm.DELT,
                           nmem=NMEM)
    model.set_date(1, 0.5, 0.04)
    model.couple_dev(0)
    sppt = s.Sppt(sp, 36, nmem=NMEM)
    diag = s.Diagnostics(sp, capacity=4, nmem=NMEM)
    letkf = s.Letkf(sp, NMEM, 4, 1.0e6)
    letkf.set_obs([s.OBS_T], [3], [10.0], [20.0], [250.0], [1.0])
    z = lambda *shape: torch.zeros(shape, dtype=torch.complex128, device="cuda")
    qcorh = z(NMEM, *sp.spec_shape)
    vor, div, t, q, ps = [z(NMEM, KX, *sp.spec_shape) for _ in range(4)] + [z(NMEM, *sp.spec_shape)]
    calls = (lambda: sppt.advance_dev(), lambda: diag.check_dev(vor, div, t), lambda: model.forcing_dev(qcorh),
             lambda: letkf.analyse_dev(vor, div, t, q, ps))
    for call in calls:                # eagerly first: what a transform allocates at its first call of a size exists before the capture
        call()
    sp.use_own_stream()
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        for call in calls:
            call()
    g.launch()
    sp.synchronize()
    assert diag.status(member=1)["next_step"] == 2 and sppt.draws(member=1) == 2              # the eager call and the replay

    sp.close()                        # the five handles are alive
    for call in calls + (g.launch,):
        with pytest.raises(s.SpdyError) as e:
            call()
        assert e.value.code == STATE, str(e.value)
    for o in (model, sppt, diag, letkf, g):
        o.close()
    torch.cuda.synchronize()

    # the device is in order: a fresh plan against the oracle
    sp = s.Spectral("t30", kx=KX, max_batch=MAX_BATCH, device=0)
    S = synth.spectra(1, sp.trunc, full_rows=True)
    G = sp.spec_to_grid(S, 1)
    assert synth.relerr(G[0], oracle_factory("t30").spec_to_grid(S[0], 1)) <= TOL
    sp.close()


def test_every_named_array_is_its_own():
    """The analysis object, the nature run and the diagnostics object each keep their arrays in one device allocation (two with a
    weight stride).  Every field a name reaches is filled over its full documented shape with values no other field holds, then all
    are read back: each holds what was written to it, so no two arrays overlap, and every address is a multiple of 8.  nmem and
    nobs = max_obs are odd, so the analysis object's int arrays start after an odd number of per-observation doubles."""
    s = support.package()
    kx, nmem, nobs = 5, 3, 5
    sp = s.Spectral("t30", kx=kx, max_batch=64, device=0)
    sp.set_sigma(np.linspace(0.0, 1.0, kx + 1) ** 1.5)
    letkf = s.Letkf(sp, nmem, nobs, 1.0e6, weight_stride=(2, 2))
    letkf.set_obs([s.OBS_T] * nobs, [2] * nobs, 30.0 * np.arange(nobs), 10.0 * np.arange(nobs) - 20.0, [250.0] * nobs, [1.0] * nobs)
    nat = s.Nature(sp, capacity=3)
    diag = s.Diagnostics(sp, capacity=3, nmem=nmem)
    fields = [(o, n, o.field(n)) for o, names in ((letkf, s.letkf.LETKF_FIELDS), (nat, s.nature.NATURE_FIELDS), (diag, s.columns.DIAG_FIELDS))
              for n in names]
    fields = [(o, n, f) for o, n, f in fields if isinstance(f, s.DeviceField)]
    assert len(fields) == len(s.letkf.LETKF_FIELDS) + len(s.nature.NATURE_FIELDS) + 2
    assert letkf.field("hx").shape == (nobs, nmem) and letkf.field("weights").shape[1:] == (kx, nmem, nmem)
    want = []
    for k, (o, n, f) in enumerate(fields):
        assert f.ptr % 8 == 0, (n, hex(f.ptr))
        want.append(1.0e7 * (k + 1) + np.arange(int(np.prod(f.shape)), dtype=np.float64).reshape(f.shape))
        f.upload(want[k])
    for (o, n, f), w in zip(fields, want):
        assert np.array_equal(o.field(n).numpy(), w), n
    for o in (diag, nat, letkf, sp):
        o.close()
