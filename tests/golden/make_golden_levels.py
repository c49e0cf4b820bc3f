#!/usr/bin/env python3
"""Regenerate tests/golden/ref_levels.npz from the REAL reference at 12 levels -- a level count inside the 9..15 class of the step
kernels (tests/levels.py), where the oracle was a bare restatement before.

Needs oracle/_ref/libspeedy_ref_t30k12.so (oracle/build_ref.sh: the reference with kx = 12; the half levels levels.sigma(12) go
in through the reference's public geometry variables, as for the 16-level build).  Holds the sigma tables and, at dt = 1200 and
4800, tref*, implicit_terms, do_horizontal_diffusion and one call of the reference's adiabatic step(2, 2, dt) with its
get_tendencies (ref_dynstep.npz's recipe) on dynstep.state(., 8000); get_geopotential once.  Sub-lattices of the 3-D arrays.

    python tests/golden/make_golden_levels.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import levels  # noqa: E402
import synth  # noqa: E402

TAG, KX = "t30k12", 12
DTS = (1200.0, 4800.0)
SUB = (slice(None), slice(None, None, 4), slice(None, None, 3))      # the part of a [12, 32, 31] array that is kept
SIGMA_TABLES = ("hsg", "dhs", "fsg", "dhsr", "fsgr")


def geop_inputs(kx, nx, mx):
    return synth.cfield((kx, nx, mx), 5, 300.0), synth.cfield((nx, mx), 6, 1000.0)


def reference():
    """the flang build at 12 levels with levels.sigma(12): half levels in, derived level tables from the C oracle (bit-equal to
    the reference's own at kx = 5, 7, 8: tests/test_oracle_golden.py)"""
    from oracle.pyoracle import Reference
    r = Reference(TAG)
    assert r.kx == KX
    o = levels.oracle("t30", KX)
    r.set_sigma(*[o.table(n) for n in SIGMA_TABLES])
    return r


def make(r):
    import dynstep
    d = {}
    kx, nx, mx = r.kx, r.nx, r.mx
    cut = lambda a: a[SUB]
    d.update(r.sigma())
    T, phis = geop_inputs(kx, nx, mx)
    d["geop"] = cut(r.geopotential(T, phis))
    div, t, ps = synth.tail_inputs(kx, nx, mx)
    for dt in DTS:
        key = "dt%d_" % int(dt)
        r.tail_init(dt)
        d.update({key + k: v for k, v in r.tref_tables().items()})
        d.update(r.corv())
        a, b, c = r.implicit_terms(div, t, ps)
        d[key + "imp_div_out"], d[key + "imp_t_out"], d[key + "imp_ps_out"] = cut(a), cut(b), c
        dm = r.dmp_tables()
        d[key + "hdiff3d"] = cut(r.hdiff(t, div, dm["dmpd"], dm["dmp1d"]))
    st = dynstep.state(r, 8000)
    for dt in DTS:
        key = "dt%d_j22_" % int(dt)
        r.tail_init(dt)
        new, phi = r.step(2, 2, dt, st)
        for n in ("vor", "div", "t", "tr"):
            d[key + n] = new[n][(Ellipsis,) + SUB[1:]]
        d[key + "ps"], d[key + "phi"] = new["ps"], cut(phi)
        for n, a in zip(("vordt", "divdt", "tdt", "psdt", "trdt"), r.get_tendencies(2, st)):
            d[key + n] = a if n == "psdt" else cut(a)
    return d


if __name__ == "__main__":
    from oracle.pyoracle import build
    build()
    out = os.path.join(HERE, "ref_levels.npz")
    np.savez_compressed(out, **make(reference()))
    print("wrote", out, os.path.getsize(out) // 1024, "KiB")
