// Host-side table generation for the spectral transform plan (product code).
//
// Reproduces, value for value, the tables the reference builds once at start-up:
//   geometry.f90:35-89, fftpack.f90:1-67 (rffti1), legendre.f90:23-71,158-237,
//   spectral.f90:20-82, horizontal_diffusion.f90:36-82, implicit.f90:36-165, physics.f90:12-39 and the level
//   constants of convection.f90:55-71 and large_scale_condensation.f90:47-66; radset (longwave_radiation.f90:197-220)
//   and, per date, get_zonal_average_fields + solar (shortwave_radiation.f90:238-329).
// The reference is FP64 in storage only; unsuffixed literals and float() are float32 first
// (SURVEY.md Appendix A).  Those sub-expressions are evaluated in float here too -- an
// "improved" table (exact pi, true Gaussian nodes, double 1/ix) breaks parity at 1e-8.
#pragma once
#include <string>
#include <vector>

namespace spdy {

struct HostTables {
    int trunc = 0, ix = 0, iy = 0, il = 0, kx = 0, nx = 0, mx = 0;
    // geometry
    std::vector<double> sia_half, coa_half, cosgr, cosgr2, hsg, dhs, fsg, dhsr, fsgr;
    std::vector<double> coriol;    // [il] 2*omega*sia (geometry.f90:89), j = 0 southernmost
    double rgas = 0.0, akap = 0.0, grav = 0.0; // physical_constants.f90:18-24 (float32 literals widened)
    // FFT
    std::vector<double> work;      // ix twiddle slots, FFTPACK layout
    int ifac[15] = {0};
    double fwd_scale = 0.0;        // float32(1/ix) widened  (fourier.f90:72)
    double taui = 0.0, sqrt2 = 0.0, hsqt2 = 0.0;   // float32 radix constants widened
    // Legendre
    std::vector<double> epsi, repsi, wt, poly;   // poly[m + mx*(n + nx*j)]
    std::vector<int> nsh2;
    // spectral operators
    std::vector<double> el2, elm2, el4, trfilt, gradx, gradym, gradyp, uvdx, uvdym, uvdyp, vddym, vddyp;
    // horizontal diffusion + implicit
    std::vector<double> dmp, dmpd, dmps, dmp1, dmp1d, dmp1s;
    std::vector<double> tref, tref1, tref2, tref3, xc, xd, xj, dhsx, elz;
    bool implicit_ready = false;
    double implicit_dt = 0.0;
    bool sigma_ready = false;      // hsg..fsgr hold a sigma-level set (geometry.f90:42-60 or set_sigma)
    // geopotential.f90:22-30 (valid when sigma_ready): xgeop1[kx], xgeop2[kx] (xgeop2[0] unused = 0),
    // and the lapse-rate correction factors corf[kx] of :53 (0 for the top and bottom level)
    std::vector<double> xgeop1, xgeop2, corf;
    // horizontal_diffusion.f90:70-82 (valid when sigma_ready): tcorv[kx], qcorv[kx]
    std::vector<double> tcorv, qcorv;
    // physics.f90:12-39 initialize_physics (valid when sigma_ready): sigl[kx], sigh[kx+1] (= sigh(0:kx)), grdsig[kx],
    // grdscp[kx], wvi[2*kx] (column-major wvi(kx,2)); convection.f90 level constants: entr[kx-2] (= entr(2:kx-1), after the
    // normalisation by sentr) and fm0; large_scale_condensation.f90:47-66 per level k (index k-1; 0 at k = 1): rhref, dqmax
    // and pfact = dhs*prg
    std::vector<double> sigl, sigh, grdsig, grdscp, wvi, entr, lsc_rhref, lsc_dqmax, lsc_pfact;
    double fm0 = 0.0;
    // vertical_diffusion.f90:57-77 (valid when sigma_ready): vd_scalars = cshc cvdi fshcq fshcse fvdiq fvdise; vd_rsig[kx] =
    // 1/dhs(k), vd_rsig1[kx] = 1/(1 - sigh(k)) (entry kx unused = 0); and per pair of levels k, k + 1 (index k-1; last 0) the
    // vd_drh0 = rhgrad*(fsg(k+1) - fsg(k)) and vd_fvdiq2 = fvdiq*sigh(k) of :80-81 (k = kx - 1) and :114-115
    std::vector<double> vd_scalars, vd_rsig, vd_rsig1, vd_drh0, vd_fvdiq2;
    // surface_fluxes.f90:300-309 set_orog_land_sfc_drag at the surface geopotential set by set_orography (valid when
    // orog_ready): phis0 and forog (ix, il), j = 0 southernmost
    std::vector<double> phis0, forog;
    bool orog_ready = false;
    // longwave_radiation.f90:197-220 radset: fband(100:400,4) column-major, entry (t - 100) + 301*(jb - 1)
    std::vector<double> fband;
    // shortwave_radiation.f90:238-329 get_zonal_average_fields + solar at the date set by set_date (valid when date_ready): one
    // value per latitude [il] (the reference's (ix,il) fields are constant along i), j = 0 southernmost
    std::vector<double> fsol, ozone, ozupp, zenit, stratz;
    bool date_ready = false;
    double tyear = 0.0;

    // Builds everything except the dt-dependent implicit tables.  Returns "" or an error text.
    std::string build(int trunc, int ix, int iy, int kx);
    // Caller-supplied half levels hsg[kx+1] (e.g. a 16-level set: geometry.f90:42-48 only defines kx = 5, 7, 8);
    // derives dhs, fsg, dhsr, fsgr as geometry.f90:51-60 does and invalidates the implicit tables.
    std::string set_sigma(const double *hsg_in);
    // implicit.f90:36-165 (+ dmp1* of :50-56).  Returns "" or an error text.
    std::string build_implicit(double dt);
    // The zonal radiation forcing of the date tyear (fraction of the year, 0 = 1 Jan 0h).  Returns "" or an error text.
    std::string set_date(double tyear);
    // Keeps the surface geopotential phis0[ix*il] and builds forog from it.  Returns "" or an error text.
    std::string set_orography(const double *phis0_in);
    // Named lookup for spdy_get_table; nullptr if unknown. *count receives the length.
    const double *lookup(const std::string &name, int *count, std::vector<double> &scratch) const;
};

// The constant fields of the slab surface models, (ix, il) each, j = 0 southernmost: land_model.f90:75-87 and :159-180
// (fmask_l, rhcapl, cdland), sea_model.f90:137-150 and :204-250 (fmask_s, rhcaps, rhcapi, cdsea, cdice; l_globe with the
// latitudinal smoothing of dmask).  thrsh = 0.1, flandmin = fseamin = 1./3., the depths and times are float32 values widened.
struct SurfaceTables {
    std::vector<double> fmask_l, fmask_s, rhcapl, cdland, rhcaps, rhcapi, cdsea, cdice;
    // fmask, alb0: (ix, il) as boundaries.f90 holds them; delt: the time step in seconds.  Returns "" or an error text.
    std::string build(const HostTables &t, const double *fmask, const double *alb0, double delt);
    const std::vector<double> *lookup(const std::string &name) const;
};

// The weights and 0-based months of forin5 and forint (interpolation.f90:16-69) for the month imont1 (1 .. 12) and the fraction
// tmonth of it: w5 = wm2 wm1 w0 wp1 wp2 at m5 = imon-2 .. imon+2; wmon at m2 = (imon, imon2); s2 is forint(2, sstan3)'s imon2.
struct SurfaceDateWeights {
    double w5[5], wmon;
    int m5[5], m2[2], s2;
};
std::string surface_date_weights(int imont1, double tmonth, SurfaceDateWeights *w);

// The constants of the SPPT pattern (sppt.f90:28-41, :76-84) for nsteps steps per day: phi = exp(-(24/nsteps)/6.0), f0 and
// sigma (mx, nx) = f0 exp(-0.25 len_decorr**2 el2) over the whole rectangle, sigma(1,1) = f0 included (the reference perturbs the
// global mean too; sigma is the same on every level), first = (1 - phi**2)**(-0.5), the factor of the first AR(1) step, and the
// taper mu[kx].  stddev = 0.33 is a float32 value widened, len_decorr = 500000 and time_decorr = 6 are exact.
struct SpptTables {
    std::vector<double> phi, f0, first, sigma, mu;   // phi, f0, first: one value each
    // mu: kx values or null = all ones.  Returns "" or an error text.
    std::string build(const HostTables &t, int nsteps, const double *mu_in);
    const std::vector<double> *lookup(const std::string &name) const;
};

}  // namespace spdy
