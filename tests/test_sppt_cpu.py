"""CPU: the SPPT generator's definition (Philox4x32-10 known answers, the uniform mapping at the extreme words), the host tables
of spdy_sppt_create on device-less plans against the restatement (tests/sppt.py), the restatement against the flang-built
reference (tests/golden/ref_sppt.npz: randn, the clips, both AR(1) branches, the transform, on the reference's own uniforms),
and the error codes."""
import ctypes

import numpy as np
import pytest

import sppt
import support
from conftest import TOL, VARIANTS

KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % int(w) for w in sppt.philox4x32_10(counter, key)) == want


def test_uniform_mapping_at_the_extreme_words():
    """r1 in (0, 1], r2 in [0, 1): all-zero words give the smallest values, all-one words the largest; randn is finite at both"""
    lo, hi = sppt.uniforms((0, 0, 0, 0)), sppt.uniforms((0xffffffff,) * 4)
    assert lo[0] == 2.0 ** -53 and lo[1] == 0.0
    assert hi[0] == 1.0 and hi[1] == 1.0 - 2.0 ** -53
    for r1, r2 in (lo, hi, (lo[0], hi[1]), (hi[0], lo[1])):
        assert np.isfinite(sppt.randn(r1, r2))
    assert sppt.FOUR_PI == 12.566370964050293 and sppt.STDDEV == 0.33000001311302185


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_tables_on_a_host_plan(tag):
    import speedy_f90_amd as s
    kx = VARIANTS[tag][3]
    sp = support.plan(tag, max_batch=4, device=-1)
    mu = np.linspace(0.0, 1.0, kx)
    for nsteps, m in ((36, None), (48, mu)):
        pat = s.Sppt(sp, nsteps, m, seed=1)
        ref = sppt.tables(sp.trunc, nsteps)
        for n in ("phi", "f0", "first"):
            assert abs(pat.table(n) - ref[n]) <= TOL * abs(ref[n]), (n, pat.table(n), ref[n])
        sig = pat.table("sigma")
        assert sig.shape == (sp.nx, sp.mx) and sig[0, 0] == pat.table("f0")
        assert np.abs(sig - ref["sigma"]).max() <= TOL * np.abs(ref["sigma"]).max()
        assert np.array_equal(pat.table("mu"), np.ones(kx) if m is None else mu)
        with pytest.raises(s.SpdyError) as e:        # a host-only plan has no device fields
            pat.field("pattern")
        assert e.value.code == -3
        pat.close()
    sp.close()


def test_restatement_against_the_reference(golden, oracle_factory):
    """everything after the uniforms, on the levels the fixture holds"""
    g, o = golden("sppt"), oracle_factory("t30")
    tab = sppt.tables(o.trunc, int(g["nsteps"]))
    worst = max(abs(tab["phi"] - g["phi"]) / g["phi"], np.abs(tab["sigma"] - g["sigma"]).max() / g["sigma"].max())
    ref = sppt.Pattern(o, int(g["nsteps"]))
    for call in range(3):
        u = g["uni%d" % call]
        ref.advance(sppt.randn(u[..., 0, 0], u[..., 0, 1]) + 1j * sppt.randn(u[..., 1, 0], u[..., 1, 1]))
        for got, want in ((ref.spec, g["spec%d" % call]), (ref.pattern, g["grid%d" % call])):
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("\n[sppt restatement vs reference] worst %.1e" % worst)
    assert worst <= TOL


def test_error_codes():
    import speedy_f90_amd as s
    sp = support.plan("t30", max_batch=4, device=-1)
    lib, h = sp.lib, ctypes.c_void_p()
    ARG = -1
    assert lib.spdy_sppt_create(None, 36, None, 1, ctypes.byref(h)) == ARG
    assert lib.spdy_sppt_create(sp.h, 36, None, 1, None) == ARG
    assert lib.spdy_sppt_create(sp.h, 0, None, 1, ctypes.byref(h)) == ARG
    assert lib.spdy_sppt_create(sp.h, -3, None, 1, ctypes.byref(h)) == ARG
    pat = s.Sppt(sp, 36)
    buf = np.zeros(4)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.spdy_sppt_table(None, b"phi", P(buf), 4) == ARG
    assert lib.spdy_sppt_table(pat.h, None, P(buf), 4) == ARG
    assert lib.spdy_sppt_table(pat.h, b"nothing", P(buf), 4) == ARG
    assert lib.spdy_sppt_table(pat.h, b"sigma", P(buf), 4) == ARG             # cap too small
    assert lib.spdy_sppt_table(pat.h, b"phi", P(buf), 0) == ARG
    assert lib.spdy_sppt_table(pat.h, b"sigma", None, 0) == sp.nx * sp.mx     # the size query
    assert lib.spdy_sppt_table(pat.h, b"phi", P(buf), 4) == 1 and buf[0] == pat.table("phi")
    p = ctypes.c_void_p()
    n = ctypes.c_longlong()
    assert lib.spdy_sppt_field(None, b"eta", ctypes.byref(p)) == ARG
    assert lib.spdy_sppt_field(pat.h, None, ctypes.byref(p)) == ARG
    assert lib.spdy_sppt_field(pat.h, b"eta", None) == ARG
    assert lib.spdy_sppt_field(pat.h, b"nothing", ctypes.byref(p)) == ARG
    assert lib.spdy_sppt_draws(None, ctypes.byref(n)) == ARG
    assert lib.spdy_sppt_draws(pat.h, None) == ARG
    assert lib.spdy_sppt_reset(None, 1) == ARG
    assert lib.spdy_sppt_advance_dev(None, None) == ARG
    assert lib.spdy_sppt_destroy(None) == 0
    for rc in (lib.spdy_sppt_advance_dev(pat.h, None), lib.spdy_sppt_reset(pat.h, 1), lib.spdy_sppt_draws(pat.h, ctypes.byref(n))):
        assert rc == -3                                                       # a host-only plan: SPDY_ERR_NO_DEVICE
    assert lib.spdy_physics_sppt_dev(None, pat.h, 1, *([None] * 14)) == ARG
    assert lib.spdy_column_physics_sppt_dev(None, 1, None, None, 1, *([None] * 14)) == ARG
    assert lib.spdy_physics_sppt_workspace(None) == ARG and lib.spdy_column_physics_sppt_workspace(None) == ARG
    assert lib.spdy_physics_sppt_workspace(sp.h) == -3
    with pytest.raises(ValueError):
        s.Sppt(sp, 36, np.ones(3))
    pat.close()
    sp.close()
