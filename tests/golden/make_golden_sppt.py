#!/usr/bin/env python3
"""Regenerate tests/golden/ref_sppt.npz from the REAL reference's sppt.f90 (build container only).

sppt.f90 and what it uses (types, params, physical_constants, geometry, fftpack, fourier, legendre, spectral) are compiled by
flang -O2 where they lie ($SPEEDY_REFERENCE/source) into a mktemp directory that is deleted afterwards, at T30 L8.  sppt.f90 gets
its `private` statement turned into `public` and its `call time_seed()` taken out, both in a temporary variant, so that the shim
(written into the same directory by this generator) can read sigma, phi and sppt_spec and replay the noise: it keeps the
generator's state (random_seed(get=)), calls gen_sppt(), puts the state back and draws the same uniforms again in gen_sppt's own
loop order.  Nothing from the reference is committed: the only output is the npz.

Three calls: the first one and two later ones.  Recorded: phi, sigma (one level; the generator asserts that all levels are equal),
and per call the uniforms, sppt_spec and the clipped grid of the levels LEVELS (the levels do not interact, and the uniforms do
not compress: all eight would not fit a committed file).  The generator asserts that tests/sppt.py gives the same from the
uniforms (randn, the clips, both AR(1) branches, the oracle's spec_to_grid) within 1e-12 and prints the worst difference.

    python tests/golden/make_golden_sppt.py
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden_moist as mg  # noqa: E402
import sppt  # noqa: E402

MODS = ("types", "params", "physical_constants", "geometry", "fftpack", "fourier", "legendre", "spectral", "sppt")
VARIANT = "s/^    private$/    public/; s/if (first) call time_seed()/continue/"
NCALLS = 3
LEVELS = (0, 7)                  # 0-based: the top and the bottom level
SHIM = """module sppt_shim
    use iso_c_binding
    use types, only: p
    use params
    implicit none
contains
    subroutine sp_init() bind(C, name="sp_init")
        use geometry, only: initialize_geometry
        use spectral, only: initialize_spectral
        call initialize_geometry
        call initialize_spectral
    end subroutine
    subroutine sp_step(uni, spec, grid, sig, ph) bind(C, name="sp_step")
        use sppt
        real(c_double), intent(out) :: uni(2,2,mx,nx,kx), grid(ix,il,kx), sig(mx,nx,kx), ph
        complex(c_double_complex), intent(out) :: spec(mx,nx,kx)
        integer :: nseed, m, n, k
        integer, allocatable :: st(:)
        real(p) :: r(2)
        call random_seed(size=nseed)
        allocate(st(nseed))
        call random_seed(get=st)
        grid = gen_sppt()
        call random_seed(put=st)
        do m = 1, mx
            do n = 1, nx
                do k = 1, kx
                    call random_number(r)
                    uni(:,1,m,n,k) = r
                    call random_number(r)
                    uni(:,2,m,n,k) = r
                end do
            end do
        end do
        spec = sppt_spec
        sig = sigma
        ph = phi
    end subroutine
end module
"""
P = mg.P


def build(tmp):
    srcs = []
    for m in MODS:
        src = os.path.join(mg.REF, m + ".f90")
        if m == "sppt":
            src = os.path.join(tmp, m + ".f90")
            open(src, "w").write(mg.sed(VARIANT, os.path.join(mg.REF, m + ".f90")))
        srcs.append(src)
    shim = os.path.join(tmp, "sppt_shim.f90")
    open(shim, "w").write(SHIM)
    so = os.path.join(tmp, "libsppt.so")
    subprocess.run([mg.FC, "-O2", "-fPIC", "-shared", "-w", "-Wl,-Bsymbolic", "-o", so] + srcs + [shim], cwd=tmp, check=True)
    return so


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_sppt: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    from oracle.pyoracle import Oracle, build as build_oracle
    build_oracle()
    o = Oracle(30, 96, 24, 8)
    kx, nx, mx, il, ix = o.kx, o.nx, o.mx, o.il, o.ix
    tmp = tempfile.mkdtemp(prefix="spdy_sppt_")
    d, worst = {}, 0.0
    try:
        lib = ctypes.CDLL(build(tmp))
        lib.sp_init()
        ref = sppt.Pattern(o)
        for call in range(NCALLS):
            uni, spec = np.zeros((kx, nx, mx, 2, 2)), np.zeros((kx, nx, mx), np.complex128)
            grid, sig, ph = np.zeros((kx, il, ix)), np.zeros((kx, nx, mx)), ctypes.c_double()
            lib.sp_step(P(uni), P(spec), P(grid), P(sig), ctypes.byref(ph))
            assert (uni[..., 0] > 0).all() and (uni < 1).all()
            eta = sppt.randn(uni[..., 0, 0], uni[..., 0, 1]) + 1j * sppt.randn(uni[..., 1, 0], uni[..., 1, 1])
            ref.advance(eta)

            def close(got, want, what):
                e = float(np.abs(got - want).max() / np.abs(want).max())
                assert e <= 1e-12, "call %d %s: restatement differs by %.2e" % (call, what, e)
                return e
            assert (sig == sig[0]).all()
            worst = max(worst, close(ref.tab["sigma"], sig[0], "sigma"), close(ref.tab["phi"], ph.value, "phi"),
                        close(ref.spec, spec, "sppt_spec"), close(ref.pattern, grid, "grid"))
            assert np.abs(grid).max() <= 1.0
            lv = list(LEVELS)
            d.update({"uni%d" % call: uni[lv], "spec%d" % call: spec[lv], "grid%d" % call: grid[lv]})
            print("call %d: |spec| max %.3e, grid std %.3f, clipped %.2f %%" % (call, np.abs(spec).max(), grid.std(),
                                                                             100.0 * (np.abs(grid) == 1.0).mean()))
        d.update(phi=np.float64(ph.value), sigma=sig[0].copy(), nsteps=np.int64(sppt.NSTEPS), levels=np.array(LEVELS, np.int64))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("restatement within %.1e of the reference" % worst)
    out = os.path.join(HERE, "ref_sppt.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%.2f MB)" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
