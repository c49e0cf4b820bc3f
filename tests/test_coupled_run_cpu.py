"""The reference side of tests/test_gpu_coupled_run.py meets its conditions, on the CPU: over the start-up steps and the 108
coupled leapfrog steps of both cases no decision of the physics of any column is closer to its threshold than
physstep.RUN_MARGIN, and no column's interpolated sstcl_ob is closer to the freezing point (no column is ever excluded); the run
stays finite, crosses the month boundary with obs_ssta, and the surface model moves the boundary fields the physics read."""
import numpy as np
import pytest

import coupledrun
import longrun
import physstep
import support
import surfmodel as sm


@pytest.mark.parametrize("name", list(longrun.CASES))
def test_coupled_reference_run_conditions(name, oracle_factory):
    sp = support.plan("t30", 36, device=-1)
    cps, log, events = coupledrun.reference_run(sp, oracle_factory("t30"), name)
    assert len(log) == coupledrun.NSTEPS + 2 and sorted(cps) == list(coupledrun.CHECKPOINTS)
    worst = min(log, key=lambda e: e["margin"])
    print("[coupled run '%s'] smallest decision margin %.1e (step %d), freezing-point margin %.1e" % (name, worst["margin"], worst["n"],
                                                                                                   log[-1]["freeze"]))
    assert worst["margin"] >= physstep.RUN_MARGIN, (name, worst)
    assert log[-1]["freeze"] >= physstep.RUN_MARGIN
    for n in cps:
        assert all(np.isfinite(v).all() for k, v in cps[n].items() if k not in ("surf",))
        assert all(np.isfinite(v).all() for v in cps[n]["surf"].values())
    days = [n for n, e in events.items() if e[1]]
    assert days == [36, 72, 108] and sum(e[2] is not None for e in events.values()) == sm.NSTEPS and events[108][0][0] == 2
    a, b = cps[36]["surf"], cps[108]["surf"]
    assert np.abs(a["stl_am"] - b["stl_am"]).max() > 0.1 and np.abs(a["tice_om"] - b["tice_om"]).max() > 1e-3
    assert not np.array_equal(cps[36]["qcorh"], cps[108]["qcorh"])
    sp.close()
