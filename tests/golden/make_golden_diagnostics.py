#!/usr/bin/env python3
"""Regenerate tests/golden/ref_diagnostics.npz from the REAL reference's diagnostics.f90 (build container only).

diagnostics.f90 and what it uses (types, params, physical_constants, geometry, fftpack, fourier, legendre, spectral) are compiled
by flang -O2 where they lie ($SPEEDY_REFERENCE/source) into a mktemp directory that is deleted afterwards, at T30 L8.
diagnostics.f90 is compiled in a temporary variant whose local `diag` becomes an intent(out) argument (the sed program VARIANT),
driven by the shim this generator writes into the same directory.  Nothing from the reference is committed: the only output is
the npz.

Input: the state after first_step and NSTEPS leapfrog steps of the reference's own ADIABATIC run (the flang-built T30 L8 library
under oracle/_ref/) from the "wind" start of tests/longrun.py.  Recorded: vor, div, t of the levels LEVELS (the levels do not
interact), the reference's diag for them, and the text the reference prints for the step ISTEP with mod(istep, nstdia) == 0,
captured from a child process's standard output.  The generator asserts that tests/diagnostics.py gives the same: the two sums
within 1e-15 relative, temp bit for bit, the text character for character; it prints the worst difference.  It also runs the
reference in a child process on the same state with the mean temperature of one level raised over 320 K, and checks that the
child prints the three lines and stops with the reference's message, as the restated predicate says it must.

    python tests/golden/make_golden_diagnostics.py
"""
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
import diagnostics  # noqa: E402
import longrun  # noqa: E402

MODS = ("types", "params", "physical_constants", "geometry", "fftpack", "fourier", "legendre", "spectral", "diagnostics")
VARIANT = ("s/subroutine check_diagnostics(vor, div, t, istep)/subroutine check_diagnostics(vor, div, t, istep, diag)/; "
           "s/^        real(p) :: diag(kx,3)/        real(p), intent(out) :: diag(kx,3)/")
NSTEPS = 36                      # one day after first_step
NSTDIA = 180                     # params.f90:60
ISTEP = 2 * NSTDIA               # the printed step
LEVELS = (0, 7)                  # 0-based: the top and the bottom level
SHIM = """module diagnostics_shim
    use iso_c_binding
    use types, only: p
    use params
    implicit none
contains
    subroutine dg_init(nstdia_in) bind(C, name="dg_init")
        use geometry, only: initialize_geometry
        use spectral, only: initialize_spectral
        integer(c_int), value :: nstdia_in
        call initialize_geometry
        call initialize_spectral
        nstdia = nstdia_in
    end subroutine
    subroutine dg_check(vor, div, t, istep, diag) bind(C, name="dg_check")
        use diagnostics, only: check_diagnostics
        complex(c_double_complex), intent(in) :: vor(mx,nx,kx), div(mx,nx,kx), t(mx,nx,kx)
        integer(c_int), value :: istep
        real(c_double), intent(out) :: diag(kx,3)
        call check_diagnostics(vor, div, t, istep, diag)
        flush(6)
    end subroutine
end module
"""
# the child: loads the library, runs one check on the state in a file, writes diag back; what it prints is the reference's
CHILD = """import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
z = np.load(sys.argv[2])
lib.dg_init(ctypes.c_int(int(sys.argv[4])))
a = [np.ascontiguousarray(z[n]) for n in ("vor", "div", "t")]
d = np.zeros((3, a[0].shape[0]))
lib.dg_check(*[x.ctypes.data_as(ctypes.c_void_p) for x in a], ctypes.c_int(int(sys.argv[3])), d.ctypes.data_as(ctypes.c_void_p))
np.save(sys.argv[5], d)
"""


def build(tmp):
    srcs = []
    for m in MODS:
        src = os.path.join(mg.REF, m + ".f90")
        if m == "diagnostics":
            text = mg.sed(VARIANT, src)
            assert "istep, diag)" in text and "intent(out) :: diag(kx,3)" in text, "the diagnostics.f90 variant did not apply"
            src = os.path.join(tmp, m + ".f90")
            open(src, "w").write(text)
        srcs.append(src)
    shim = os.path.join(tmp, "diagnostics_shim.f90")
    open(shim, "w").write(SHIM)
    so = os.path.join(tmp, "libdiag.so")
    subprocess.run([mg.FC, "-O2", "-fPIC", "-shared", "-w", "-Wl,-Bsymbolic", "-o", so] + srcs + [shim], cwd=tmp, check=True)
    return so


def child(tmp, so, state, istep, tag):
    """one check_diagnostics call in a process of its own -> (diag or None if the child stopped, stdout, stderr, exit code)"""
    script, inp, out = os.path.join(tmp, "child.py"), os.path.join(tmp, tag + "_in.npz"), os.path.join(tmp, tag + "_out.npy")
    open(script, "w").write(CHILD)
    np.savez(inp, **state)
    r = subprocess.run([sys.executable, script, so, inp, str(istep), str(NSTDIA), out], capture_output=True, text=True, cwd=tmp)
    return (np.load(out) if os.path.exists(out) else None), r.stdout, r.stderr, r.returncode


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_diagnostics: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    from oracle.pyoracle import Oracle, Reference, build as build_oracle
    build_oracle()
    r = Reference("t30")
    o = Oracle(r.trunc, r.ix, r.iy, r.kx)
    st = longrun.rest_state(o, wind=longrun.CASES["wind"])
    end = longrun.run(lambda j1, j2, dt, s: r.step(j1, j2, dt, s)[0], r.tail_init, st, nsteps=NSTEPS, checkpoints=(NSTEPS,))[NSTEPS]
    state = {n: np.ascontiguousarray(end[n][1]) for n in ("vor", "div", "t")}          # time level 2, as speedy.f90:41 passes it
    elm2 = o.table("elm2")
    tmp = tempfile.mkdtemp(prefix="spdy_diag_")
    try:
        so = build(tmp)
        want = diagnostics.diag(state["vor"], state["div"], state["t"], elm2)
        got, text, err, rc = child(tmp, so, state, ISTEP, "print")
        assert got is not None and rc == 0, (rc, err)
        quiet = child(tmp, so, state, ISTEP + 1, "quiet")
        assert quiet[1] == "" and np.array_equal(quiet[0], got), "a step off the print period must print nothing"
        worst = float(np.abs(got[:2] / want[:2] - 1.0).max())
        assert worst <= 1e-15, "restated sums differ from the reference by %.2e" % worst
        assert np.array_equal(got[2], want[2]), "restated temp is not the reference's bit for bit"
        assert text == diagnostics.lines(ISTEP, got), (text, diagnostics.lines(ISTEP, got))
        assert not diagnostics.stops(got)
        print(text, end="")
        print("restated sums within %.1e of the reference, temp bit-equal, text equal" % worst)
        # the stop: the mean temperature of the bottom level over 320 K
        hot = {n: a.copy() for n, a in state.items()}
        hot["t"][LEVELS[1], 0, 0] = 330.0 / diagnostics.SQRT_HALF
        hwant = diagnostics.diag(hot["vor"], hot["div"], hot["t"], elm2)
        assert diagnostics.stops(hwant) and diagnostics.masks(hwant)[LEVELS[1]] == diagnostics.TEMP_HIGH
        hgot, htext, herr, hrc = child(tmp, so, hot, ISTEP + 1, "hot")
        assert hgot is None, "the reference did not stop where the restated predicate says it must"
        assert diagnostics.STOP in herr + htext, (htext, herr)
        assert htext.startswith(diagnostics.lines(ISTEP + 1, hwant)), (htext, diagnostics.lines(ISTEP + 1, hwant))
        print("the reference stops on temp > 320 with '%s' (exit code %d)" % (diagnostics.STOP, hrc))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lv = list(LEVELS)
    d = {n: a[lv] for n, a in state.items()}
    d.update(diag=got[:, lv], text=np.array(text), istep=np.int64(ISTEP), levels=np.array(LEVELS, np.int64), nsteps=np.int64(NSTEPS))
    # the whole row as printed, so that the text can be checked against it
    d["diag_all"] = got
    out = os.path.join(HERE, "ref_diagnostics.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%.2f MB)" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
