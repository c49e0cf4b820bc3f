"""CPU: the reference side of the two-day run WITH the whole physics (tests/physstep.py: reference_run; the GPU side is
tests/test_gpu_physics_run.py) -- the conditions under which a device run can be held to it column by column: finite, no
decision of any column on any of the 74 steps within RUN_MARGIN of its threshold, every branch of every block taken -- and the
NumPy restatements of the physics on columns that run produced, against the flang-built reference (tests/golden/ref_physrun.npz)."""
import os

import numpy as np
import pytest

import longrun
import moist
import physstep
import support
import surface
import synth
from conftest import ROOT, TOL

PROG = ("vor", "div", "t", "tr", "ps")


@pytest.fixture(scope="module")
def plan():
    return support.plan("t30", 36, device=-1)


def test_shortwave_cadence():
    """speedy.f90:21,35 and shortwave_radiation.f90:67: both start-up steps, then leapfrog steps 1, 4, 7, ..."""
    on = [n for n in range(-1, 73) if physstep.shortwave_step(n)]
    assert on == [-1, 0] + list(range(1, 73, 3))
    assert all(physstep.shortwave_step(n) == (i < 2) for i, n in enumerate(physstep.RESYNC))


def test_hook_reads_time_level_one(plan, oracle_factory):
    """physics.f90:94-104: the physics read time level 1 whatever level the dynamics read.  grids_of on a state whose second
    level is garbage gives what it gives on the state itself, and differs once level 1 is changed."""
    o = oracle_factory("t30")
    st = longrun.rest_state(o, wind=longrun.CASES["wind"])
    bad = {n: (np.stack([v[0], np.full_like(v[1], np.nan)]) if v.ndim > 2 else v) for n, v in st.items()}
    g, gb = physstep.grids_of(o, st), physstep.grids_of(o, bad)
    for n in g:
        assert np.array_equal(g[n], gb[n]), n
    other = dict(st, t=np.stack([st["t"][0] * 1.01, st["t"][1]]))
    assert not np.array_equal(physstep.grids_of(o, other)["tg"], g["tg"])


@pytest.mark.parametrize("name", ["rest", "wind"])
def test_reference_side_of_the_run(name, plan, oracle_factory):
    """Start-up steps + 72 leapfrog steps at delt = 2400 s from the reference's rest state with the whole physics in every step:
    every prognostic finite at every checkpoint; the CONDITION that no decision of any column on any step lies within
    RUN_MARGIN = 1e-11 of its threshold (no column is ever excluded from a comparison); for "wind", every branch of the moist
    block, the surface fluxes and the boundary layer taken by some column on some step, and at step 72 some but not all
    columns convect."""
    o = oracle_factory("t30")
    case = physstep.run_case(plan, o, name)
    cps, log, pre = physstep.reference_run(case)
    assert len(log) == longrun.NSTEPS + 2 and sorted(cps) == list(longrun.CHECKPOINTS) and not pre
    assert [e["sw"] for e in log[:6]] == [True, True, True, False, False, True]
    for n, cp in cps.items():
        for k in PROG + ("rad", "ssrd"):
            assert np.all(np.isfinite(cp[k].real)) and np.all(np.isfinite(cp[k].imag)), (name, n, k)
        assert cp["rad"].shape == (6 * o.kx + 7, o.il * o.ix)
    worst = min(log, key=lambda e: e["margin"])
    print("\n[run with physics '%s'] smallest decision margin of %d steps: %.2e (leapfrog step %d)" % (
        name, len(log), worst["margin"], worst["n"]))
    taken = {}
    for e in log:
        for k, v in list(e["moist"].items()) + list(e["branches"].items()):
            taken[k] = taken.get(k, 0) + v
        if e["n"] in longrun.CHECKPOINTS:
            print("  step %2d: margin %.1e, %d columns convect; moist %s; surface %s" % (
                e["n"], e["margin"], e["convecting"], e["moist"], e["branches"]))
    assert worst["margin"] >= physstep.RUN_MARGIN, (name, worst["n"], worst["margin"])
    if name == "wind":
        names = set(log[0]["moist"]) | set(surface.SFC_BRANCHES) | set(surface.PBL_BRANCHES)
        assert set(surface.SFC_BRANCHES) | set(surface.PBL_BRANCHES) == set(log[0]["branches"])
        never = sorted(k for k in names if not taken.get(k))
        assert not never, never
        assert 1 <= log[-1]["convecting"] <= o.il * o.ix - 1


def test_restatements_on_evolved_columns():
    """surface.chain on columns the run itself made -- the grids of "wind" before leapfrog steps 70 (shortwave) and 72 (none, on
    the radiation state the run holds), stored with every input in tests/golden/ref_physrun.npz -- against the flang-built
    reference's own blocks on the same grids: floats within TOL, integers identical, and the stored sample holds every branch
    the two grids take."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_physrun.npz"))
    kx = 8
    tab = moist.tables(moist.HSG[kx])
    worst = ("", 0.0)
    for n in physstep.PHYSRUN_STEPS:
        p = "s%d_" % n
        c = {k: z[p + "in_" + k] for k in physstep.PHYSRUN_INPUTS}
        zon = {k: z[p + "zon_" + k] for k in physstep.ZON}
        sw = bool(z[p + "sw"])
        assert sw == physstep.shortwave_step(n)
        state = None if sw else {k: z[p + "rs_" + k].copy() for k in physstep.RAD_STATE}
        r, _ = surface.chain(tab, c, zon, z[p + "in_sqcoa"], sw, state)
        assert float(r["margin"].min()) >= physstep.RUN_MARGIN
        got = physstep.chain_outputs(r, c)
        assert set(got) == {k[len(p) + 4:] for k in z.files if k.startswith(p + "out_")}
        for k, g in got.items():
            w = z[p + "out_" + k]
            assert g.shape == w.shape, (n, k)
            if w.dtype.kind == "i":
                assert np.array_equal(g, w), (n, k)
            else:
                e = synth.relerr(g, w)
                worst = max(worst, ("step %d %s" % (n, k), e), key=lambda x: x[1])
                assert e <= TOL, (n, k, e)
        # the sample holds every branch the whole grid took
        br = dict(surface.branch_cols(r), **{"moist_" + k: v for k, v in r["moist"]["branch_cols"].items()})
        names, counts = list(z[p + "branch_names"]), z[p + "branch_counts"]
        assert sorted(names) == sorted(br)
        for k, cnt in zip(names, counts):
            assert (cnt > 0) == bool(br[k].any()), (n, k, int(cnt))
    print("\n[restatements on evolved columns] worst %s %.1e" % worst)
