"""GPU: longrun's "rest" and "wind" cases with the whole physics AND the surface coupled, in the order of calls of DESIGN s14: the
start-up steps, then three days (108 leapfrog steps) from 30 January, over the month boundary, as graph replays.  The step reads
the surface model's own arrays (spdy_surface_model_boundary) and writes out.sfc.hfluxn / shf / evap and out.rad.ssrd, which
couple_dev reads as the LAST NODE of the step's graph on steps within a day; on a day's last step the graph without it is
replayed, the host sets the new date and couple_dev is issued eagerly; forcing_dev (albedos and the real qcorh, written into the
array the step reads) precedes the first step of a day.  The reference side is tests/coupledrun.py (its conditions are asserted on
the CPU by tests/test_coupled_run_cpu.py and again here).  At each day's end the prognostics, the radiation state, qcorh and every
field of the surface model agree within TOL.  The test notices what it is for: with couple_dev skipped for one step, or
forcing_dev issued after a day's first step instead of before it, the first checkpoint after the fault fails."""
import pytest

import coupledrun
import longrun
import physstep
import support
from conftest import TOL
from physstep import KX

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(longrun.CASES))
def test_three_day_coupled_run(name, oracle_factory):
    o = oracle_factory("t30")
    sp = support.plan("t30", 4 * KX + 4)
    cps, log, events = coupledrun.reference_run(sp, o, name)
    case, c, _ = coupledrun.setup(sp, o, name)
    assert min(e["margin"] for e in log) >= physstep.RUN_MARGIN and log[-1]["freeze"] >= physstep.RUN_MARGIN
    sp.surface_set_orography(case.phis0)
    sp.physics_workspace()
    sp.use_own_stream()
    ncol = sp.il * sp.ix
    got, nodes = coupledrun.device_run(sp, case, c, events)
    lines, worst = [], ("", 0.0)
    for n in coupledrun.CHECKPOINTS:
        e = coupledrun.errors(got[n], cps[n], ncol)
        top = sorted(e.items(), key=lambda kv: -kv[1])[:6]
        lines.append("step %3d: " % n + " ".join("%s %.1e" % kv for kv in top))
        worst = max([worst] + [("step %d %s" % (n, k), v) for k, v in e.items()], key=lambda x: x[1])
    print("\n[3-day coupled run '%s' vs the reference side, largest relative errors; decision margin %.1e, freezing-point margin %.1e]\n  "
          % (name, min(e["margin"] for e in log), log[-1]["freeze"]) + "\n  ".join(lines))
    print("[graph nodes] step %d, step + couple_dev %d (shortwave %d, %d)" % (nodes[False, False], nodes[False, True], nodes[True, False],
                                                                            nodes[True, True]))
    assert worst[1] <= TOL, (name, worst)
    assert nodes[False, True] == nodes[False, False] + 1 and nodes[True, True] == nodes[True, False] + 1, nodes
    # the test notices what it is for: the first checkpoint after each fault fails
    for fault, cp in (("skip_couple", 36), ("late_forcing", 72)):
        bad, _ = coupledrun.device_run(sp, case, c, events, fault)
        e = coupledrun.errors(bad[cp], cps[cp], ncol)
        print("[fault %s] largest relative error at step %d: %.1e" % (fault, cp, max(e.values())))
        assert max(e.values()) > TOL, (fault, cp)
    sp.close()
