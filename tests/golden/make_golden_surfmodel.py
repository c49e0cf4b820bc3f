#!/usr/bin/env python3
"""Regenerate tests/golden/ref_surfmodel.npz from the REAL reference's surface models and daily forcing (build container only).

The reference's date, interpolation, boundaries, land_model, sea_model, coupler, mod_radcon, auxiliaries, forcing and what they
use (geometry, the spectral transforms, humidity, the radiation modules for radset and get_zonal_average_fields, surface_fluxes
for set_orog_land_sfc_drag, horizontal_diffusion for tcorh / qcorh) are compiled by flang -O2 where they lie
($SPEEDY_REFERENCE/source) into a mktemp directory that is deleted afterwards.  land_model.f90 and sea_model.f90 get their
`private` statement turned into `public`, so that the shim can read their fields.  input_output.f90 is NOT compiled (NetCDF): the
generator writes a stand-in `module input_output` of its own whose load_boundary_file returns the seeded fields of
tests/surfmodel.py from two banks.  tests/golden/surfmodel_shim.f90 (ours) is the bind(C) entry.  Nothing from the reference is
committed: the only output is the npz.

T30.  For each window of surfmodel.WINDOWS the reference runs initialize_coupler, set_forcing(0) and 108 times the main loop's
body (set_forcing(1) on the first step of a day, newdate, couple_sea_land) on surfmodel.fluxes' seeded flux fields.  The generator
asserts that the reference leaves the climatologies as they were given (surfmodel.after_init), that its date is the restated one
on every step, the freezing-point margin and the branch coverage; it keeps the eight tables and, at the steps CHECK, every field
on a column sample that holds every branch, qcorh of the first and the last forcing, and the inputs of every fourth sample column.

    python tests/golden/make_golden_surfmodel.py
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
import longrun  # noqa: E402
import physstep  # noqa: E402
import surfmodel as sm  # noqa: E402

MODS = ("types", "params", "physical_constants", "dynamical_constants", "geometry", "date", "interpolation", "fftpack", "fourier",
        "legendre", "spectral", "input_output", "boundaries", "mod_radcon", "auxiliaries", "humidity", "horizontal_diffusion",
        "shortwave_radiation", "longwave_radiation", "land_model", "surface_fluxes", "sea_model", "coupler", "forcing")
PUBLIC = "s/^    private$/    public/"
NBANK = 14                       # months of the anomaly file the stand-in holds: December before the start year to its end
                                 # and one more (obs_ssta reads month (start year - issty0)*12 + the model's month: sea_model.f90:377)
NUNIFORM, NBRANCH, INSTEP = 12, 2, 4
# the recorded steps (0: after initialize_coupler): every ninth step, and the steps around each midnight
CHECK = tuple(sorted(set(range(0, sm.WINDOW_STEPS + 1, 9)) | {35, 37, 71, 73, 107}))
INPUT_OUTPUT = """module input_output
    use types, only: p
    use params
    implicit none
    real(p) :: bank12(ix,il,12,5), ssta_bank(ix,il,%d)
    integer :: ssta_first = 1
    interface load_boundary_file
        module procedure load_2d
        module procedure load_month
        module procedure load_long
    end interface
contains
    function load_2d(file_name, field_name) result(field)
        character(len=*), intent(in) :: file_name, field_name
        real(p) :: field(ix,il)
        field = 0.0_p                      ! vegh, vegl: no vegetation
    end function
    function load_month(file_name, field_name, month) result(field)
        character(len=*), intent(in) :: file_name, field_name
        integer, intent(in) :: month
        real(p) :: field(ix,il)
        integer :: k
        k = 0
        if (field_name == "stl") k = 1
        if (field_name == "snowd") k = 2
        if (field_name == "swl1") k = 3
        if (field_name == "sst") k = 4
        if (field_name == "icec") k = 5
        if (k == 0) then
            field = 0.0_p                  ! swl2: a dry second layer
        else
            field = bank12(:,:,month,k)
        end if
    end function
    function load_long(file_name, field_name, month, length) result(field)
        character(len=*), intent(in) :: file_name, field_name
        integer, intent(in) :: month, length
        real(p) :: field(ix,il)
        field = ssta_bank(:,:,month - ssta_first + 1)
    end function
end module
""" % NBANK
P = mg.P


def build(tmp):
    srcs = []
    for m in MODS:
        src = os.path.join(mg.REF, m + ".f90")
        if m == "input_output":
            src = os.path.join(tmp, m + ".f90")
            open(src, "w").write(INPUT_OUTPUT)
        elif m in ("land_model", "sea_model"):
            src = os.path.join(tmp, m + ".f90")
            open(src, "w").write(mg.sed(PUBLIC, os.path.join(mg.REF, m + ".f90")))
        srcs.append(src)
    so = os.path.join(tmp, "libsurfmodel.so")
    subprocess.run([mg.FC, "-O2", "-fPIC", "-shared", "-w", "-Wl,-Bsymbolic", "-o", so] + srcs +
                   [os.path.join(HERE, "surfmodel_shim.f90")], cwd=tmp, check=True)
    return so


def sample(ref, tab, c, ncol):
    """columns spread evenly, plus some of every branch and of every class of the init routines' decisions"""
    fl, fs = tab["fmask_l"], tab["fmask_s"]
    masks = dict(ref.branch)
    masks.update(land0=fl == 0.0, land_low=(fl > 0.0) & (fl < sm.THIRD), land_high=(fl >= sm.THIRD) & (fl < 1.0), land1=fl == 1.0,
                 sea_low=(fs > 0.0) & (fs < sm.THIRD), alb_lo=c["alb0"] < sm.f32(0.4), alb_hi=c["alb0"] >= sm.f32(0.4))
    pick = [np.linspace(0, ncol - 1, NUNIFORM).astype(np.int64)]
    for k, mask in sorted(masks.items()):
        idx = np.nonzero(mask)[0]
        assert idx.size, "no column in class %s" % k
        pick.append(idx[np.linspace(0, idx.size - 1, min(NBRANCH, idx.size)).astype(np.int64)])
    return np.unique(np.concatenate(pick)), {k: int(v.sum()) for k, v in masks.items()}


def run(wname, so, tmp, o):
    # module state is per loaded library: one private copy per window
    mine = os.path.join(tmp, "libsurfmodel_%s.so" % wname)
    shutil.copy(so, mine)
    lib = ctypes.CDLL(mine)
    start = sm.WINDOWS[wname]
    phis0 = sm.orography(o)
    il, ix = phis0.shape
    n = il * ix
    c = sm.climatology(phis0, longrun.latitudes(o.table("sia_half")), start=start[:2])
    g = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape((-1, il, ix)))
    b12 = np.stack([g(c[k]) for k in ("stl12", "snowd12", "swl1", "sst12", "sice12")])
    first = (start[0] - sm.ISSTY0) * 12
    raw_ssta = lambda k: sm.sstan_month(k, n)
    sb = np.stack([g(raw_ssta(first + k))[0] for k in range(NBANK)])
    lib.sm_inputs(P(g(c["fmask"])), P(g(c["alb0"])), P(g(phis0)), P(b12), P(sb), ctypes.c_int(NBANK))
    lib.sm_init(*[ctypes.c_int(v) for v in start + (first,)])
    tab = sm.tables(c["fmask"], c["alb0"], o.table("sia_half"), ix)
    ref = sm.Model(c, tab, ssta=sm.ssta_reader(c["fmask"]))
    out, tt, rr = np.zeros((19, il, ix)), np.zeros((8, il, ix)), np.zeros((4, il, ix))
    qq, clim, ymdt = np.zeros((o.nx, o.mx), np.complex128), np.zeros((5, 12, il, ix)), np.zeros(8)
    rec = {"fields": {}, "forcing": {}, "qcorh": {}, "worst": 0.0}

    def get():
        lib.sm_get(P(out), P(tt), P(rr), P(qq), P(clim), P(ymdt))

    def close(x, want, what):
        s = np.abs(x).max()
        e = float(np.abs(x - want).max() / s) if s > 0 else float(np.abs(want).max())
        rec["worst"] = max(rec["worst"], e)
        assert e <= 1e-12, "%s %s: restatement differs by %.2e" % (wname, what, e)

    ms = ctypes.c_int(1)

    def on_step(step, day, date, flux, shifted):
        if day:
            fl = {k: g(v) for k, v in flux.items()}
            lib.sm_step(ctypes.byref(ms), P(fl["hfluxn"]), P(fl["shf"]), P(fl["evap"]), P(g(flux["ssrd"])))
        get()
        assert tuple(ymdt[:6].astype(int)) == (date.year, date.month, date.day, date.hour, date.minute, date.imont1), (step, ymdt)
        assert ymdt[6] == date.tmonth and ymdt[7] == date.tyear, (step, ymdt[6:], date.tmonth, date.tyear)
        for i, k in enumerate(sm.FIELDS):
            close(out[i].reshape(-1), ref.f[k], "step %d %s" % (step, k))
        if step in CHECK:
            rec["fields"][step] = out.reshape(19, n).copy()

    # the reference's set_forcing(1) of a step runs inside that step's sm_step: the restated values are kept until then
    kept = {}

    def on_forcing_keep(step, date):
        kept[step] = ({k: ref.f[k].copy() for k in sm.FORCING}, o.grid_to_spec(ref.f["corh"].reshape(il, ix)))

    def on_step_all(step, day, date, flux, shifted):
        on_step(step, day, date, flux, shifted)
        fstep = step
        if step > 0 and step in kept:              # (set_forcing(0)'s results are those of step 1's set_forcing(1))
            want, q = kept[fstep]
            for i, k in enumerate(sm.FORCING[:4]):
                close(rr[i].reshape(-1), want[k], "forcing of step %d %s" % (fstep, k))
            close(qq, q, "forcing of step %d qcorh" % fstep)
            rec["forcing"][fstep] = rr.reshape(4, n).copy()
            rec["qcorh"][fstep] = qq.copy()
    sm.run(ref, start, sm.WINDOW_STEPS, phis0.reshape(-1), lambda k: sm.fluxes(k, n), on_forcing_keep, on_step_all)
    # what the reference made of the fields it was given; its tables
    get()
    for i, k in enumerate(sm.CLIM12):
        assert np.array_equal(clim[i].reshape(12, n), c[k]), "%s: the reference changed %s" % (wname, k)
    for i, k in enumerate(sm.TABLES):
        close(tt[i].reshape(-1), tab[k], "table " + k)
    assert ref.margin >= physstep.RUN_MARGIN, ref.margin
    assert all(v.any() for v in ref.branch.values()), {k: int(v.sum()) for k, v in ref.branch.items()}
    sub, counts = sample(ref, tab, c, n)
    print("%s: margin %.2e, %d sample columns, classes %s, restatement within %.1e" % (wname, ref.margin, sub.size, counts, rec["worst"]))
    d = {wname + "_sub": sub, wname + "_insub": sub[::INSTEP], wname + "_check": np.array(sorted(rec["fields"]), np.int64),
         wname + "_fields": np.stack([rec["fields"][s][:, sub] for s in sorted(rec["fields"])]),
         wname + "_forcing_steps": np.array(sorted(rec["forcing"]), np.int64),
         wname + "_forcing": np.stack([rec["forcing"][s][:, sub] for s in sorted(rec["forcing"])]),
         wname + "_qcorh_steps": np.array([min(rec["qcorh"]), max(rec["qcorh"])], np.int64),
         wname + "_qcorh": np.stack([rec["qcorh"][min(rec["qcorh"])], rec["qcorh"][max(rec["qcorh"])]]),
         wname + "_tables": np.stack([tt[i].reshape(-1)[sub] for i in range(8)]),
         wname + "_min_margin": np.float64(ref.margin),
         wname + "_class_names": np.array(sorted(counts)), wname + "_class_counts": np.array([counts[k] for k in sorted(counts)], np.int64)}
    ins = sub[::INSTEP]
    for k in ("fmask", "alb0") + sm.CLIM12 + ("sstan3",):
        d["%s_in_%s" % (wname, k)] = np.asarray(c[k])[..., ins]
    d[wname + "_in_phis0"] = phis0.reshape(-1)[ins]
    return d


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_surfmodel: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    from oracle.pyoracle import Oracle, build as build_oracle
    build_oracle()
    o = Oracle(30, 96, 24, 8)
    tmp = tempfile.mkdtemp(prefix="spdy_surfmodel_")
    d = {"seed": np.int64(sm.CLIM_SEED), "field_names": np.array(sm.FIELDS), "forcing_names": np.array(sm.FORCING[:4]),
         "table_names": np.array(sm.TABLES)}
    cwd = os.getcwd()
    try:
        so = build(tmp)
        os.chdir(tmp)                      # initialize_date looks for a namelist.nml: there is none here
        for wname in sm.WINDOWS:
            d.update(run(wname, so, tmp, o))
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    out = os.path.join(HERE, "ref_surfmodel.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%.2f MB)" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
