"""GPU: the column physics ON its thresholds and in regimes outside the ordinary draw (tests/thresholds.py).

The columns constructed exactly on every class-(i) threshold of thresholds.INVENTORY and one ulp to either side run through the
one-launch chain (csrc/spdy_column_chain.hip, "physics_fused" 1), the five-kernel chain ("physics_fused" 0) and the five single
entry points (spdy_moist_columns_dev, spdy_radiation_down_dev / _up_dev, spdy_surface_fluxes_dev, spdy_pbl_dev), a shortwave call
and a call without shortwave on the held state: the three bit-equal, integers identical to the flang-built reference
(tests/golden/ref_thresholds.npz), floats within TOL of it, in the array norm and in EVERY column by the column's own scale
(guards.column_err; thresholds.scales for differences of large terms).  Where the reference is exactly 0 in a column the device is
exactly 0.  The regime states run the whole chain on every column against the restatement in the same way.

The per-column bound is the project's TOL for every output: the reference side alone (restatement against the flang-built
reference, tests/test_thresholds_cpu.py) stays below 4.3e-14 in every column, more than a factor 10 below TOL.  For sfc.shf,
sfc.hfluxn, rad.tt_rlw, pbl.tt_pbl and ttend the operand scale exceeds the array's own maximum in most columns, so for them the array
norm asserted beside it is the binding one.  Only the rows marked `observable` in thresholds.INVENTORY pin the kernel's operator;
the other constructed columns are robustness cases (signed zeros, denormals, ends of tables, exact 0 and 1 after clamps)."""
import os

import numpy as np
import pytest

import moist
import radiation
import support
import surface
import thresholds as th
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _plan(tag, tyear, c, il, ix, sp=None):
    sp = sp or support.plan(tag, 4)
    sp.radiation_set_date(tyear)
    sp.surface_set_orography(c["phis0"].reshape(il, ix))
    zon = radiation.zonal_columns({n: sp.table(n) for n in th.ZON}, 1, il, ix)
    sqcoa = surface.sqcoa_columns(sp.table("coa_half"), 1, il, ix)
    return sp, zon, sqcoa


def _stored(ref, tag, step):
    pre = "%s_c%d_" % (tag, step)
    return {k[len(pre):]: ref[k] for k in ref.files if k.startswith(pre)}


@pytest.mark.parametrize("tag", th.TAGS)
def test_threshold_columns_on_device(tag):
    """Measured on MI355X, worst per-column error per block (t30 / t30k5): against the reference moist 9.4e-15 / 2.4e-15 (precls),
    rad 1.4e-15 / 4.1e-16, sfc 3.9e-16 / 2.1e-15, pbl and tendencies 1.6e-16 / 1.1e-15; every column against the restatement
    moist 1.9e-13 / 3.5e-14 (precls), rad 2.7e-14 / 2.1e-14, sfc 2.8e-15 / 3.8e-15, pbl and tendencies 1.3e-15 / 2.9e-15."""
    ref = np.load(os.path.join(GOLDEN, "ref_thresholds.npz"))
    ix, il, kx = support.grid(tag)
    th.check_threshold_columns(tag, support.plan(tag, 4), moist.tables(moist.HSG[kx]), int(ref[tag + "_seed"]), ref[tag + "_sub"],
                               lambda step: _stored(ref, tag, step))


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_regimes_every_column(tag):
    """The one-launch chain on every column of every regime of thresholds.REGIMES against the restatement: integers identical,
    floats within TOL per column by the column's own scale; near-tie columns are left out (at most 1 % of a regime, asserted).
    Measured on MI355X: no column left out; worst per-column error 3.0e-13 (t30, solstice_dec, moist.precls) and 2.9e-13 (t63k16,
    high_orography, moist.precls); radiation at most 1.1e-13 (clstr), surface 4.2e-14 (evap), tendencies 1.3e-14 (qtend)."""
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    sp = support.plan(tag, 4)
    sp.column_physics_workspace()
    for name, (seed, tyear) in th.REGIMES.items():
        c = th.regime(name, tab, il * ix)
        sp, zon, sqcoa = _plan(tag, tyear, c, il, ix, sp)
        r, keep = th.regime_run(tab, c, zon, sqcoa)
        share = th.check_regime(name, r, keep)
        one = th.chain(sp, kx, il, ix, [(th.dev(c, il, ix), True)], 1)
        got = {n[2:]: v for n, v in one.items() if not n.endswith("state")}
        worst = {}
        th.against(got, th.flat(r, kx), kx, th.scales(tab, c, r), keep, False, "%s %s" % (tag, name), worst)
        print("[regime %s %s] %.3f %% of the columns left out; worst per-column error per block: %s"
              % (tag, name, 100 * share, ", ".join("%s %.1e (%s)" % (b, e, n) for b, (e, n) in sorted(worst.items()))))
    sp.close()
