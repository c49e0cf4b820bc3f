"""CPU: pin the C restatement (oracle/speedy_oracle.c) to the reference.

1. against the committed golden vectors (reference outputs produced by the flang build of
   /root/reference/source, tests/golden/make_golden.py) -- runs everywhere;
2. against the reference's outputs for extra seeds, whole arrays (tests/golden/ref_live.npz: their digests, recorded
   from the flang build by make_golden.py) -- runs everywhere too.
The restatement is expected to be bit-exact; the assertion bar is 1e-15 relative, bit for bit where a digest pins it.
"""
import os

import numpy as np
import pytest

import dynstep
import synth
from conftest import GOLDEN
from golden.make_golden import tail_inputs

EXACT = 1e-15
TAGS = ("t30", "t63")


def close(x, ref, tol=EXACT):
    assert x.shape == ref.shape
    assert synth.relerr(x, ref) <= tol


def live_golden():
    return np.load(os.path.join(GOLDEN, "ref_live.npz"))


def pinned(x, z, key):
    """x is, bit for bit, the whole array of the reference's output that ref_live.npz holds the digest of under `key`."""
    assert np.all(np.isfinite(x)), key
    assert synth.digest(x) == str(z[key]), key


@pytest.mark.parametrize("tag", TAGS)
def test_tables(tag, golden, oracle_factory):
    g, o = golden(tag), oracle_factory(tag)
    assert list(g["dims"]) == [o.trunc, o.ix, o.iy, o.il, o.kx, o.nx, o.mx]
    for name in ("sia_half", "cosgr", "cosgr2", "hsg", "dhs", "fsg", "dhsr", "fsgr", "work"):
        assert np.array_equal(o.table(name), g["tab_" + name]), name
    assert np.array_equal(o.table("coa_half")[: o.iy], g["tab_coa_half"])
    assert np.array_equal(o.table("ifac")[:6].astype(int), g["tab_ifac"][:6])
    assert np.array_equal(o.table("epsi"), g["tab_epsi"].ravel())
    assert np.array_equal(o.table("el2"), g["tab_el2"].ravel())


def test_known_answers_appendix_f(oracle_factory):
    """SURVEY.md Appendix F known-answer values (flang -O2 oracle run)."""
    o = oracle_factory("t30")
    sia = o.table("sia_half")
    bits = sia.astype(np.float32).view(np.uint32)
    assert np.array_equal(sia, sia.astype(np.float32).astype(np.float64))      # exactly float32 values
    assert bits[0] == 0x3F7FB2AE and bits[11] == 0x3F395CD2 and bits[23] == 0x3D04A2C4
    assert o.table("work")[0] == 0.997858923119484320 and o.table("work")[1] == 0.0654031310475514244
    assert list(o.table("ifac")[:6].astype(int)) == [96, 4, 2, 4, 4, 3]
    assert abs(o.table("wt").sum() - 1.0) < 2e-15
    s = o.grid_to_spec(np.ones((o.il, o.ix)))
    assert s[0, 0].real == 1.41421358031670752
    o63 = oracle_factory("t63")
    assert list(o63.table("ifac")[:6].astype(int)) == [192, 4, 4, 4, 4, 3]
    assert o63.table("sia_half").astype(np.float32).view(np.uint32)[47] == 0x3C855767
    nsh2 = o.table("nsh2").astype(int)
    assert nsh2[0] == 62 and nsh2[-1] == 2 and nsh2.sum() == 1054


@pytest.mark.parametrize("tag", TAGS)
def test_transform_stages(tag, golden, oracle_factory):
    g, o = golden(tag), oracle_factory(tag)
    S, G = g["S"], g["G"]
    for b in range(g["leginv"].shape[0]):
        close(o.legendre_inv(S[b]), g["leginv"][b])
        close(o.fourier_inv(g["leginv"][b], 1), g["finv1"][b])
        close(o.fourier_inv(g["leginv"][b], 2), g["finv2"][b])
        close(o.fourier_dir(G[b]), g["fdir"][b])
        close(o.legendre_dir(g["fdir"][b]), g["legdir"][b])
        close(o.spec_to_grid(S[b], 1), g["s2g1"][b])
        close(o.spec_to_grid(S[b], 2), g["s2g2"][b])
        close(o.grid_to_spec(G[b]), g["g2s"][b])
        # structural facts the reference exhibits
        assert np.all(g["g2s"][b][-1] == 0)                      # row nx stays 0
        assert np.array_equal(g["finv2"][b], g["finv1"][b] * o.table("cosgr")[:, None])
    close(o.grid_to_spec(np.ones((o.il, o.ix))), g["ones_g2s"])


@pytest.mark.parametrize("tag", TAGS)
def test_spectral_operators(tag, golden, oracle_factory):
    g, o = golden(tag), oracle_factory(tag)
    S, G = g["S"], g["G"]
    close(o.laplacian(S[0]), g["lap"])
    close(o.inverse_laplacian(S[0]), g["invlap"])
    close(o.trunct(S[0]), g["trunct"])
    dx, dy = o.grad(S[0]); close(dx, g["grad_dx"]); close(dy, g["grad_dy"])
    a, b = o.vds(S[0], S[1]); close(a, g["vds_vor"]); close(b, g["vds_div"])
    a, b = o.uvspec(S[0], S[1]); close(a, g["uv_u"]); close(b, g["uv_v"])
    a, b = o.vdspec(G[0], G[1], 2); close(a, g["vdspec2_vor"]); close(b, g["vdspec2_div"])
    a, b = o.vdspec(G[0], G[1], 1); close(a, g["vdspec1_vor"]); close(b, g["vdspec1_div"])


@pytest.mark.parametrize("tag", TAGS)
def test_fftpack_vectors(tag, golden, oracle_factory):
    import ctypes
    g, o = golden(tag), oracle_factory(tag)
    work = np.ascontiguousarray(g["tab_work"]); ifac = np.ascontiguousarray(g["tab_ifac"].astype(np.int32))
    for key, fn in (("fft_b", o.lib.orc_rfftb1), ("fft_f", o.lib.orc_rfftf1)):
        c = g["fft_in"].copy(); ch = np.zeros_like(c)
        rc = fn(ctypes.c_int(c.size), c.ctypes.data_as(ctypes.c_void_p), ch.ctypes.data_as(ctypes.c_void_p),
                work.ctypes.data_as(ctypes.c_void_p), ifac.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        close(c, g[key])


@pytest.mark.parametrize("tag", TAGS)
def test_tail(tag, golden, oracle_factory):
    g, o = golden(tag), oracle_factory(tag)
    if "imp_div" in g.files:
        div, t, ps = g["imp_div"], g["imp_t"], g["imp_ps"]
        assert np.array_equal(div, tail_inputs(o.kx, o.nx, o.mx)[0])
    else:
        div, t, ps = tail_inputs(o.kx, o.nx, o.mx)
    for dt in g["dts"]:
        key = "dt%d_" % int(dt)
        o.tail_init(float(dt))
        for name in ("dmp", "dmpd", "dmps", "dmp1", "dmp1d", "dmp1s", "tref", "tref2", "tref3"):
            close(o.table(name), g[key + name].ravel())
        if dt in g["imp_dts"]:
            a, b, c = o.implicit_terms(div, t, ps)
            close(a, g[key + "imp_div_out"]); close(b, g[key + "imp_t_out"]); close(c, g[key + "imp_ps_out"])
        if key + "hdiff2d" in g.files:
            close(o.hdiff(ps, 2 * ps, g[key + "dmps"], g[key + "dmp1s"]), g[key + "hdiff2d"])
        if key + "hdiff3d" in g.files:
            close(o.hdiff(t, div, g[key + "dmp"], g[key + "dmp1"]), g[key + "hdiff3d"])


@pytest.mark.parametrize("tag", TAGS)
def test_against_live_reference(tag, oracle_factory):
    """Extra seeds against the reference's outputs for them (tests/golden/ref_live.npz), whole arrays."""
    z, o = live_golden(), oracle_factory(tag)
    S = synth.spectra(3, o.trunc, first=100, full_rows=True)
    G = synth.grids(3, o.ix, o.il, first=100)
    for b in range(3):
        for kcos in (1, 2):
            pinned(o.spec_to_grid(S[b], kcos), z, "rt_%s_s2g_%d_%d" % (tag, b, kcos))
        pinned(o.grid_to_spec(G[b]), z, "rt_%s_g2s_%d" % (tag, b))
    # round-trip accuracy of the reference itself is only ~5e-5 (first-guess Gaussian latitudes)
    s2 = o.grid_to_spec(o.spec_to_grid(synth.spectra(1, o.trunc)[0], 1))
    err = np.max(np.abs(s2 - synth.spectra(1, o.trunc)[0])[:-1])
    assert 1e-6 < err < 5e-3
    pinned(o.roundtrip_loop(G[:2]), z, "rt_%s_loop" % tag)


EXTRA = ("t30", "t63", "t30k5", "t30k7", "t63k16")


@pytest.mark.parametrize("tag", EXTRA)
def test_other_level_counts_and_geopotential(tag, golden, oracle_factory):
    """ref_extra.npz: flang builds of the reference with kx = 5, 7 (geometry.f90:42-48) and kx = 16 (half levels
    supplied through the reference's public geometry variables), plus get_geopotential (geopotential.f90:33-57),
    coriol (geometry.f90:89) and tcorv/qcorv (horizontal_diffusion.f90:70-82) at every level count."""
    from golden.make_golden import geop_inputs, L16_SUB
    g, o = golden("extra"), oracle_factory(tag)
    cut = (lambda a: a[L16_SUB]) if tag == "t63k16" else (lambda a: a)
    for name in ("hsg", "dhs", "fsg", "dhsr", "fsgr", "coriol", "tcorv", "qcorv"):
        assert np.array_equal(o.table(name), g[tag + "_" + name]), name
    T, phis = geop_inputs(o.kx, o.nx, o.mx)
    assert np.array_equal(cut(o.geopotential(T, phis)), g[tag + "_geop"])
    div, t, ps = tail_inputs(o.kx, o.nx, o.mx)
    for dt in (1200.0, 4800.0):
        key = "%s_dt%d_" % (tag, int(dt))
        if key + "tref" not in g.files:
            continue
        o.tail_init(dt)
        for name in ("tref", "tref2", "tref3"):
            assert np.array_equal(o.table(name), g[key + name]), name
        if key + "imp_div_out" in g.files:
            a, b, c = o.implicit_terms(div, t, ps)
            close(cut(a), g[key + "imp_div_out"]); close(cut(b), g[key + "imp_t_out"]); close(c, g[key + "imp_ps_out"])
            close(cut(o.hdiff(t, div, o.table("dmpd").reshape(o.nx, o.mx), o.table("dmp1d").reshape(o.nx, o.mx))), g[key + "hdiff3d"])


@pytest.mark.parametrize("tag", ("t30k5", "t30k7", "t63k16"))
def test_other_level_counts_live(tag, oracle_factory):
    """implicit_terms and get_geopotential at 5, 7 and 16 levels on another seed, whole arrays (tests/golden/ref_live.npz)."""
    z, o = live_golden(), oracle_factory(tag)
    o.tail_init(2400.0)
    div, t, ps = synth.tail_inputs(o.kx, o.nx, o.mx, seed=1234)
    outs = o.implicit_terms(div, t, ps)
    assert len(outs) == 3
    for i, x in enumerate(outs):
        pinned(x, z, "lev_%s_imp%d" % (tag, i))
    T, phis = synth.cfield((o.kx, o.nx, o.mx), 77, 250.0), synth.cfield((o.nx, o.mx), 78, 500.0)
    pinned(o.geopotential(T, phis), z, "lev_%s_geop" % tag)


@pytest.mark.parametrize("tag", sorted(dynstep.STEP_CASES))
def test_step_field_pinned(tag, oracle_factory):
    """step_field_2d / step_field_3d (time_stepping.f90:126-167): the C oracle against the reference's own two functions,
    compiled by flang from the reference file (oracle/build_ref.sh cuts them into a scratch module) -- golden vectors for
    j1 = 1 (forward step) and j1 = 2 (leapfrog + Robert-Asselin-Williams filter), 8, 5 and 16 levels."""
    z, o = dynstep.step_golden(), oracle_factory(tag)
    wil, rob = z[tag + "_wil_rob"]
    assert wil == float(np.float32(0.53)) and rob == float(np.float32(0.05))      # params.f90:32-33: float32 literals
    F3, D3, F2, D2 = dynstep.step_inputs(o.kx, o.nx, o.mx)
    for j1, dt, eps in ((1, 2400.0, 0.0), (2, 4800.0, rob)):
        key = "%s_j%d_" % (tag, j1)
        sub = dynstep.STEP_CASES[tag] if dynstep.STEP_CASES[tag] else (dynstep.STEP_J1_SUB if j1 == 1 else None)
        cut = (lambda a: a[(Ellipsis,) + sub]) if sub else (lambda a: a)
        f3, d3 = o.step_field(j1, dt, eps, wil, F3, D3)
        f2, d2 = o.step_field(j1, dt, eps, wil, F2, D2)
        for mine, ref in ((cut(f3), z[key + "f3"]), (cut(d3), z[key + "d3"]), (f2, z[key + "f2"]), (d2, z[key + "d2"])):
            assert mine.shape == ref.shape
            close(mine, ref)
        assert np.array_equal(cut(d3), z[key + "d3"]) and np.array_equal(d2, z[key + "d2"])    # trunct is exact


def test_step_field_live(oracle_factory):
    """The same against the flang build's outputs for other steps, full arrays (tests/golden/ref_live.npz)."""
    from golden.make_golden import LIVE_STEP_CASES
    z, o = live_golden(), oracle_factory("t30")
    wil, rob = z["sf_wil_rob"]
    F3, D3, F2, D2 = dynstep.step_inputs(o.kx, o.nx, o.mx)
    for c, (j1, dt, filtered) in enumerate(LIVE_STEP_CASES):
        for dim, (F, D) in ((3, (F3, D3)), (2, (F2, D2))):
            a, b = o.step_field(j1, dt, rob if filtered else 0.0, wil, F, D)
            pinned(a, z, "sf_%d_%dd_field" % (c, dim)); pinned(b, z, "sf_%d_%dd_fdt" % (c, dim))


SPECTEND_CASES = {"t30": None, "t30k5": None, "t63k16": (slice(None), slice(None, None, 5), slice(None, None, 3))}


@pytest.mark.parametrize("tag", sorted(SPECTEND_CASES))
def test_spectral_tendencies_pinned(tag, oracle_factory):
    """get_spectral_tendencies (tendencies.f90:241-293): the C oracle against the reference's own subroutine, compiled by flang
    from the reference file (oracle/build_ref.sh cuts it, and the declaration part of prognostics.f90, into scratch modules) --
    golden vectors at 8, 5 and 16 levels, the inputs placed in time level 1 and in time level 2 of the reference's arrays."""
    from golden.make_golden import spectend_inputs
    z, o = np.load(os.path.join(GOLDEN, "ref_spectend.npz")), oracle_factory(tag)
    o.tail_init(4800.0)
    div, t, ps, phis, divdt, tdt, psdt = spectend_inputs(o.kx, o.nx, o.mx)
    a, b, c, phi = o.spectral_tendencies(div, t, ps, phis, divdt, tdt, psdt)
    for j2 in (1, 2):
        sub = SPECTEND_CASES[tag] or (dynstep.STEP_J1_SUB if j2 == 2 else None)
        cut = (lambda x: x[sub]) if sub else (lambda x: x)
        key = "%s_j%d_" % (tag, j2)
        for mine, name in ((cut(a), "divdt"), (cut(b), "tdt"), (c, "psdt"), (cut(phi), "phi")):
            ref = z[key + name]
            assert mine.shape == ref.shape, (name, mine.shape, ref.shape)
            close(mine, ref)


def test_spectral_tendencies_live(oracle_factory):
    """The same against the flang build's outputs, full arrays and another dt (tests/golden/ref_live.npz)."""
    from golden.make_golden import spectend_inputs
    z, o = live_golden(), oracle_factory("t30")
    for dt in (1200.0, 4800.0):
        o.tail_init(dt)
        outs = o.spectral_tendencies(*spectend_inputs(o.kx, o.nx, o.mx))
        assert len(outs) == 4
        for i, x in enumerate(outs):
            pinned(x, z, "stend_dt%d_%d" % (int(dt), i))


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_dynamics_step_pinned(tag, oracle_factory):
    """The oracle's whole adiabatic time step (tests/dynstep.py: inverse transforms, grid-space dynamical tendencies, direct
    transforms, tendency combination, get_spectral_tendencies, implicit_terms, the diffusion block, step_field) against ONE CALL
    of the reference's own step(j1, j2, dt) -- time_stepping.f90 compiled by flang unchanged, on tendencies.f90 minus its three
    physics lines (oracle/build_ref.sh) -- and its get_tendencies: golden vectors at 8, 5 and 16 levels, BIT FOR BIT."""
    from golden.make_golden import DYNSTEP_CASES, DYN63_SUB, STEP_SUB
    import dynstep
    z, o = np.load(os.path.join(GOLDEN, "ref_dynstep.npz")), oracle_factory(tag)
    sub = DYN63_SUB if tag == "t63k16" else STEP_SUB
    st = dynstep.state(o, 8000)
    for j1, j2, dt in (DYNSTEP_CASES if tag == "t30" else DYNSTEP_CASES[1:]):
        o.tail_init(dt)
        new, out = dynstep.oracle_dynamics_step(o, st, j1, dt, 0.0 if j1 == 1 else dynstep.ROB, j2=j2, before_diffusion=True)
        key = "%s_j%d%d_" % (tag, j1, j2)
        for n in ("vor", "div", "t", "tr"):
            assert np.array_equal(new[n][(Ellipsis,) + sub[1:]], z[key + n]), (key, n)
        assert np.array_equal(new["ps"], z[key + "ps"]) and np.array_equal(out["phi"][sub], z[key + "phi"]), key
        for n in ("vordt", "divdt", "tdt", "psdt", "trdt"):             # get_tendencies: before the diffusion and the leapfrog
            a = out["pre_" + n]
            assert np.array_equal(a if n == "psdt" else a[sub], z[key + n].reshape((a if n == "psdt" else a[sub]).shape)), (key, n)


@pytest.mark.parametrize("case", ["rest", "wind"])
def test_two_day_run_pinned(case, oracle_factory):
    """BASELINE config 1's stand-in: first_step + 72 leapfrog steps (2 days) of the flang-built reference's adiabatic step from
    the reference's own rest state over a seeded orography (tests/longrun.py; tests/golden/ref_run72.npz), against the oracle's
    call-by-call step CHAINED over the same 74 steps: the prognostics after 1, 2, 4, 9, 18, 36 and 72 steps, BIT FOR BIT --
    the restatement does not drift from the reference over a run, it IS the reference's arithmetic."""
    import dynstep
    import longrun
    z, o = np.load(os.path.join(GOLDEN, "ref_run72.npz")), oracle_factory("t30")
    st = longrun.rest_state(o, wind=longrun.CASES[case])
    out = longrun.run(lambda j1, j2, dt, s: dynstep.oracle_dynamics_step(o, s, j1, dt, 0.0 if j1 == 1 else dynstep.ROB, j2=j2)[0],
                      o.tail_init, st)
    assert sorted(out) == list(longrun.CHECKPOINTS)
    for n, state in out.items():
        for k, a in state.items():
            assert np.all(np.isfinite(a.view(float)))
            assert np.array_equal(longrun.cut(k, a), z["%s_%d_%s" % (case, n, k)]), (case, n, k)
    u, v = o.uvspec(out[72]["vor"][0, 0], out[72]["div"][0, 0])       # the run is not a trivial one: m/s at the top level
    assert np.abs(o.spec_to_grid(u, 2)).max() > (10.0 if case == "wind" else 0.5)


def test_dynamics_step_live(oracle_factory):
    """The same against the flang build's outputs: the start-up sequence of first_step and a leapfrog step, chained, full
    arrays, bit for bit (tests/golden/ref_live.npz)."""
    from golden.make_golden import LIVE_DYN_CASES
    import dynstep
    z, o = live_golden(), oracle_factory("t30")
    st_o = dynstep.state(o, 8100)
    for c, (j1, j2, dt) in enumerate(LIVE_DYN_CASES):
        o.tail_init(dt)
        st_o, out = dynstep.oracle_dynamics_step(o, st_o, j1, dt, 0.0 if j1 == 1 else dynstep.ROB, j2=j2)
        for n in ("vor", "div", "t", "tr", "ps"):
            pinned(st_o[n], z, "dyn_%d_%s" % (c, n))
        pinned(out["phi"], z, "dyn_%d_phi" % c)


@pytest.mark.parametrize("tag", ["t30", "t30k5", "t63k16"])
def test_output_fields_pinned(tag, oracle_factory):
    """The gridded snapshot (input_output.f90:183-205: uvspec + five inverse transforms per level, float32 conversions with
    q*1.0e-3, phi/grav, p0*exp(ps)): the C oracle against the reference's own lines, cut out of input_output.f90 as they are and
    compiled by flang (oracle/build_ref.sh) -- golden vectors at 8, 5 and 16 levels.  BIT FOR BIT in float32 for the five linear
    fields; ps_out goes through libm's exp() and is held to one float32 ulp (it is bit-equal on the build image)."""
    from golden.make_golden import OUT_SUB, OUT_SEED
    import dynstep
    z, o = np.load(os.path.join(GOLDEN, "ref_output.npz")), oracle_factory(tag)
    st = dynstep.state(o, OUT_SEED)
    phi = o.geopotential(st["t"][0], st["phis"])
    outs = o.output(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])
    for n, a in zip(("u", "v", "t", "q", "phi"), outs):
        assert np.array_equal(a[OUT_SUB[tag]].view(np.int32), z["%s_%s" % (tag, n)].view(np.int32)), (tag, n)
    ulp = np.abs(outs[5].view(np.int32).astype(np.int64) - z[tag + "_ps"].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()


def test_output_fields_live(oracle_factory):
    """The same against the flang build's outputs at T30 L8 and T63 L8 on another seed, whole arrays (tests/golden/ref_live.npz)."""
    import dynstep
    z = live_golden()
    for tag in ("t30", "t63"):
        o = oracle_factory(tag)
        st = dynstep.state(o, 7100)
        phi = o.geopotential(st["t"][0], st["phis"])
        outs = o.output(st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], phi, st["ps"][0])
        assert len(outs) == 6
        for n, a in zip(("u", "v", "t", "q", "phi", "ps"), outs):
            pinned(a.view(np.int32), z, "out_%s_%s" % (tag, n))


def test_step_restatements_selfconsistent(oracle_factory):
    """Independent NumPy readings of the source lines of step_field, get_spectral_tendencies and the diffusion block against the
    C restatements (kept from the rounds in which those pieces could not be pinned; they are pinned now: tests above)."""
    o = oracle_factory("t30")
    o.tail_init(4800.0)
    kx, nx, mx = o.kx, o.nx, o.mx
    shp = (kx, nx, mx)
    # --- step_field_2d (time_stepping.f90:142-167)
    rob, wil, dt = float(np.float32(0.05)), float(np.float32(0.53)), 4800.0
    F = synth.cfield((2,) + shp, 11); D = synth.cfield(shp, 12, 1e-4)
    trf = o.table("trfilt").reshape(nx, mx)
    for j1, eps in ((1, 0.0), (2, rob)):
        out, fdt = o.step_field(j1, dt, eps, wil, F, D)
        fd = D * trf
        o1, o2 = F[0].copy(), F[1].copy()
        fnew = o1 + dt * fd
        oj = o1 if j1 == 1 else o2
        n1 = oj + wil * eps * (o1 - 2 * oj + fnew)
        oj2 = n1 if j1 == 1 else o2
        n2 = fnew - (1.0 - wil) * eps * (n1 - 2.0 * oj2 + fnew)
        assert synth.relerr(out[0], n1) < 1e-15 and synth.relerr(out[1], n2) < 1e-15 and np.array_equal(fdt, fd)
    # --- diffusion block (time_stepping.f90:62-96) from the pinned do_horizontal_diffusion
    vor, div, t, tr = (synth.cfield(shp, 20 + i) for i in range(4))
    vdt, ddt, tdt, qdt = (synth.cfield(shp, 30 + i, 1e-5) for i in range(4))
    tcorh, qcorh = synth.cfield((nx, mx), 40), synth.cfield((nx, mx), 41)
    sdrag = 1.0 / (float(np.float32(24.0 * 30.0)) * 3600.0)
    T = {n: o.table(n).reshape(nx, mx) for n in ("dmp", "dmpd", "dmps", "dmp1", "dmp1d", "dmp1s")}
    a, b, c, d = o.hdiff_step(vor, div, t, tr, tcorh, qcorh, sdrag, vdt, ddt, tdt, qdt)
    hd = o.hdiff
    ra = hd(vor, vdt, T["dmp"], T["dmp1"]); rb = hd(div, ddt, T["dmpd"], T["dmp1d"])
    ctmp = t + tcorh[None] * o.table("tcorv")[:, None, None]
    rc = hd(ctmp, tdt, T["dmp"], T["dmp1"])
    ra[0, :, 0] -= sdrag * vor[0, :, 0]; rb[0, :, 0] -= sdrag * div[0, :, 0]
    ra = hd(vor, ra, T["dmps"], T["dmp1s"]); rb = hd(div, rb, T["dmps"], T["dmp1s"]); rc = hd(ctmp, rc, T["dmps"], T["dmp1s"])
    rd = hd(tr + qcorh[None] * o.table("qcorv")[:, None, None], qdt, T["dmpd"], T["dmp1d"])
    for x, y in ((a, ra), (b, rb), (c, rc), (d, rd)):
        assert synth.relerr(x, y) < 1e-15
    # --- get_spectral_tendencies (tendencies.f90:242-293)
    ps, phis = synth.cfield((nx, mx), 50, 0.1), synth.cfield((nx, mx), 51, 1000.0)
    psdt = synth.cfield((nx, mx), 52, 1e-6)
    tt = synth.cfield(shp, 53, 300.0)
    A, B, C, phi = o.spectral_tendencies(div, tt, ps, phis, ddt, tdt, psdt)
    dhs, dhsr = o.table("dhs"), o.table("dhsr")
    tref, tref2, tref3 = o.table("tref"), o.table("tref2"), o.table("tref3")
    dmean = sum(div[k] * dhs[k] for k in range(kx))
    rps = psdt - dmean; rps[0, 0] = 0
    sig = np.zeros((kx + 1, nx, mx), complex); dumk = np.zeros_like(sig)
    for k in range(kx - 1):
        sig[k + 1] = sig[k] - dhs[k] * (div[k] - dmean)
    for k in range(1, kx):
        dumk[k] = sig[k] * (tref[k] - tref[k - 1])
    rt = np.stack([tdt[k] - (dumk[k + 1] + dumk[k]) * dhsr[k] + tref3[k] * (sig[k + 1] + sig[k]) - tref2[k] * dmean for k in range(kx)])
    rphi = o.geopotential(tt, phis)
    rgas = float(np.float32(2.0) / np.float32(7.0)) * 1004.0
    rdiv = np.stack([ddt[k] - o.laplacian(rphi[k] + rgas * tref[k] * ps) for k in range(kx)])
    assert np.array_equal(phi, rphi)
    for x, y in ((A, rdiv), (B, rt), (C, rps)):
        assert synth.relerr(x, y) < 1e-14


def _levels12(o, golden_of):
    """the oracle at 12 levels (tests/levels.py) against golden_of(key): the sigma tables, get_geopotential and, at two time steps,
    tref*, implicit_terms, do_horizontal_diffusion and one adiabatic step(2, 2, dt) with its get_tendencies -- BIT FOR BIT"""
    import dynstep
    from golden.make_golden_levels import DTS, SUB, geop_inputs
    cut = lambda a: a[SUB]
    same = lambda a, key: (a.shape == golden_of(key).shape and np.array_equal(a, golden_of(key)), key)
    for name in ("hsg", "dhs", "fsg", "dhsr", "fsgr", "tcorv", "qcorv"):
        assert np.array_equal(o.table(name), golden_of(name)), name
    assert np.all(np.isfinite(o.table("fsgr")))
    T, phis = geop_inputs(o.kx, o.nx, o.mx)
    ok, key = same(cut(o.geopotential(T, phis)), "geop")
    assert ok, key
    div, t, ps = tail_inputs(o.kx, o.nx, o.mx)
    st = dynstep.state(o, 8000)
    for dt in DTS:
        key = "dt%d_" % int(dt)
        o.tail_init(dt)
        for name in ("tref", "tref2", "tref3"):
            assert np.array_equal(o.table(name), golden_of(key + name)), (dt, name)
        a, b, c = o.implicit_terms(div, t, ps)
        h = o.hdiff(t, div, o.table("dmpd").reshape(o.nx, o.mx), o.table("dmp1d").reshape(o.nx, o.mx))
        for x, name in ((cut(a), "imp_div_out"), (cut(b), "imp_t_out"), (c, "imp_ps_out"), (cut(h), "hdiff3d")):
            assert np.all(np.isfinite(x)), (dt, name)
            ok, k = same(x, key + name)
            assert ok, k
        new, out = dynstep.oracle_dynamics_step(o, st, 2, dt, dynstep.ROB, j2=2, before_diffusion=True)
        key += "j22_"
        for n in ("vor", "div", "t", "tr"):
            ok, k = same(new[n][(Ellipsis,) + SUB[1:]], key + n)
            assert ok, k
        assert same(new["ps"], key + "ps")[0] and same(cut(out["phi"]), key + "phi")[0], key
        for n in ("vordt", "divdt", "tdt", "psdt", "trdt"):             # get_tendencies: before the diffusion and the leapfrog
            a = out["pre_" + n]
            ok, k = same(a if n == "psdt" else cut(a), key + n)
            assert ok, k


def test_levels12_pinned():
    """The oracle inside the 9..15 level class of the step kernels: at kx = 12 against the flang build of the reference with
    kx = 12 (oracle/build_ref.sh t30k12; tests/golden/ref_levels.npz, tests/golden/make_golden_levels.py)."""
    import levels
    z = np.load(os.path.join(GOLDEN, "ref_levels.npz"))
    _levels12(levels.oracle("t30", 12), lambda key: z[key])


def test_levels12_live():
    """The same against the flang build itself, where oracle/_ref holds it: nothing between the reference and the oracle."""
    import levels
    from oracle.pyoracle import Reference
    from golden import make_golden_levels as mg
    levels.oracle("t30", 12)                                  # (builds oracle/_ref where the reference's sources are present)
    if not Reference.available(mg.TAG):
        pytest.skip("no flang build of the reference at 12 levels here")
    d = mg.make(mg.reference())
    _levels12(levels.oracle("t30", 12), lambda key: d[key])
    z = np.load(os.path.join(GOLDEN, "ref_levels.npz"))       # and the committed file is what the build gives
    assert sorted(z.files) == sorted(d)
    for k in z.files:
        assert np.array_equal(z[k], d[k]), k
