// The surface models on the device: couple_sea_land (coupler.f90:30-38 = couple_land_atm, land_model.f90:184-239, and
// couple_sea_atm, sea_model.f90:253-363 with run_sea_model :387-444) as one launch, and the column part of set_forcing
// (forcing.f90:55-62 and :84-97) as another.  One thread per column; every field is the model's own (csrc/spdy_kernels.hpp:
// SurfField), read and written by its column's thread only.  The date weights are read from model memory (SurfDate), so a
// captured launch picks a new date up on its next replay.
//
// nmem members go through ONE launch of each kernel: blockIdx.y is the member, which enters only as uniform offsets -- of its own
// fields in the model's array (surf_slot, csrc/spdy_kernels.hpp) and of its state in the flux arrays.  Every expression below
// is the single state's, on the same values in the same order.
//
// Unsuffixed literals of the reference are float32 values widened: sstfr = 273.2 - 1.8 is a float32
// difference, anom0 = 20., albsea .. emisfc, sbc, alhc, sd2sc.  sea_coupling_flag is 0 (the reference stops otherwise), so
// hfseacl = 0, beta = 1, sst_om is initialised to 0 and no ocean-model climatology exists.
#include "spdy_columns.hpp"

namespace spdy {
namespace {

constexpr int SURF_BLOCK = 64;

__global__ __launch_bounds__(SURF_BLOCK) void surface_couple_kernel(const SurfCols a)
{
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * SURF_BLOCK + threadIdx.x;
    const long ncol = a.ncol;
    if (i >= ncol) return;
    const int nmem = a.nmem, mem = blockIdx.y;
    double *const f = a.f + i;
    const SurfDate &d = *a.date;
    auto at = [&](int n) -> double & { return f[surf_slot(n, nmem, mem) * ncol]; };               // a field by its name
    const double *const cl = f + surf_slot(SM_NFIELDS, nmem, 0) * ncol;
    auto clim = [&](int n) { return cl[(long)(n - SM_NFIELDS) * ncol]; };                         // a month of a climatology
    const long mo = (long)mem * ncol;
    const double *const hfluxn = a.hfluxn + 2 * mo, *const shf = a.shf + 3 * mo, *const evap = a.evap + 3 * mo, *const ssrd = a.ssrd + mo;
    // interpolation.f90:38-69 and :16-35 at this column
    auto forin5 = [&](int c) {
        return d.w5[0] * clim(c + d.m5[0]) + d.w5[1] * clim(c + d.m5[1]) + d.w5[2] * clim(c + d.m5[2]) + d.w5[3] * clim(c + d.m5[3]) +
               d.w5[4] * clim(c + d.m5[4]);
    };
    auto forint = [&](int c, int m0, int m1) {
        const double x = clim(c + m0);
        return x + d.wmon * (clim(c + m1) - x);
    };
    const double sstfr = F(273.2f - 1.8f);

    // ---- couple_land_atm
    const double stlcl = forin5(SM_STL12);
    const double snowdcl = forint(SM_SNOWD12, d.m2[0], d.m2[1]);
    const double soilwcl = forint(SM_SOILW12, d.m2[0], d.m2[1]);
    at(SM_STLCL_OB) = stlcl;
    at(SM_SNOWDCL_OB) = snowdcl;
    at(SM_SOILWCL_OB) = soilwcl;
    if (a.day == 0) {
        at(SM_STL_LM) = stlcl;
        at(SM_STL_AM) = stlcl;
    } else if (a.flags & SURF_LAND) {
        // run_land_model
        double tanom = at(SM_STL_LM) - stlcl;
        tanom = at(SM_CDLAND) * (tanom + at(SM_RHCAPL) * hfluxn[i]);
        const double stl = tanom + stlcl;
        at(SM_STL_LM) = stl;
        at(SM_STL_AM) = stl;
    } else {
        at(SM_STL_AM) = stlcl;
    }
    at(SM_SNOWD_AM) = snowdcl;
    at(SM_SOILW_AM) = soilwcl;

    // ---- couple_sea_atm: interpolation and the adjustment over sea ice (sea_model.f90:265-305)
    double sstcl = forin5(SM_SST12);
    double sicecl = forint(SM_SICE12, d.m2[0], d.m2[1]);
    double sstan = at(SM_SSTAN_OB);
    if (a.flags & SURF_SSTAN) {
        sstan = forint(SM_SSTAN3, 1, d.s2);
        at(SM_SSTAN_OB) = sstan;
    }
    double ticecl;
    if (sstcl > sstfr) {
        sicecl = 0.5 < sicecl ? 0.5 : sicecl;
        ticecl = sstfr;
        if (sicecl > 0.0) sstcl = sstfr + (sstcl - sstfr) / (1.0 - sicecl);
    } else {
        sicecl = 0.5 > sicecl ? 0.5 : sicecl;
        ticecl = sstfr + (sstcl - sstfr) / sicecl;
        sstcl = sstfr;
    }
    at(SM_SSTCL_OB) = sstcl;
    at(SM_SICECL_OB) = sicecl;
    at(SM_TICECL_OB) = ticecl;

    double sst_om, tice_om, sice_om;
    if (a.day == 0) {
        sst_om = 0.0;                 // sea_coupling_flag <= 0
        tice_om = ticecl;
        sice_om = sicecl;
    } else {
        sst_om = at(SM_SST_OM);
        tice_om = at(SM_TICE_OM);
        sice_om = at(SM_SICE_OM);
        if (a.flags & SURF_ICE) {
            // run_sea_model, with sice_am / tice_am of the previous call
            const double albsea = F(0.07f), albice = F(0.60f), emisfc = F(0.98f), sbc = F(5.67e-8f), alhc = F(2501.0f);
            const double hfl2 = hfluxn[ncol + i];
            const double tice_am = at(SM_TICE_AM), sice_am = at(SM_SICE_AM);
            const double fr2 = sstfr * sstfr, ti2 = tice_am * tice_am;
            const double difice = (albsea - albice) * ssrd[i] + emisfc * sbc * (fr2 * fr2 - ti2 * ti2) + shf[ncol + i] +
                                  evap[ncol + i] * alhc;
            const double hflux_i = hfl2 + difice * (1.0 - sice_am);
            // 1. ocean mixed layer
            double hflux = hfl2 - 0.0 - sicecl * (hflux_i + 1.0 * (sstfr - tice_om));
            double tanom = sst_om - sstcl;
            tanom = at(SM_CDSEA) * (tanom + at(SM_RHCAPS) * hflux);
            sst_om = tanom + sstcl;
            // 2. sea-ice slab
            hflux = hflux_i + 1.0 * (sstfr - tice_om);
            tanom = tice_om - ticecl;
            const double anom0 = F(20.0f);
            const double cdis = at(SM_CDICE) * (anom0 / (anom0 + fabs(tanom)));
            tanom = cdis * (tanom + at(SM_RHCAPI) * hflux);
            tice_om = tanom + ticecl;
            sice_om = sicecl;
        }
    }
    at(SM_SST_OM) = sst_om;
    at(SM_TICE_OM) = tice_om;
    at(SM_SICE_OM) = sice_om;

    // ---- fields for the atmosphere (sea_model.f90:327-362)
    const double sstan_am = (a.flags & SURF_SSTAN) ? sstan : 0.0;
    double sst_am = sstcl + sstan_am;
    const double sice_am = (a.flags & SURF_ICE) ? sice_om : sicecl;
    const double tice_am = (a.flags & SURF_ICE) ? tice_om : ticecl;
    sst_am = sst_am + sice_am * (tice_am - sst_am);
    at(SM_SSTAN_AM) = sstan_am;
    at(SM_SICE_AM) = sice_am;
    at(SM_TICE_AM) = tice_am;
    at(SM_SST_AM) = sst_am;
    at(SM_SSTI_OM) = sst_om + sice_am * (tice_am - sst_om);
}

__global__ __launch_bounds__(SURF_BLOCK) void surface_forcing_kernel(const SurfForcingCols a)
{
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * SURF_BLOCK + threadIdx.x;
    const long ncol = a.ncol;
    if (i >= ncol) return;
    const int nmem = a.nmem, mem = blockIdx.y;
    double *const f = a.f + i;
    auto at = [&](int n) -> double & { return f[surf_slot(n, nmem, mem) * ncol]; };
    // forcing.f90:55-62, mod_radcon.f90:22-24, land_model.f90:43
    const double albsea = F(0.07f), albice = F(0.60f), albsn = F(0.60f), sd2sc = F(60.0f), refrh1 = F(0.7f);
    const double alb0 = at(SM_ALB0), fl = at(SM_FMASK_L), fs = at(SM_FMASK_S);
    const double sc = at(SM_SNOWD_AM) / sd2sc;
    const double snowc = 1.0 < sc ? 1.0 : sc;
    const double alb_l = alb0 + snowc * (albsn - alb0);
    const double alb_s = albsea + at(SM_SICE_AM) * (albice - albsea);
    at(SM_SNOWC) = snowc;
    at(SM_ALB_L) = alb_l;
    at(SM_ALB_S) = alb_s;
    at(SM_ALBSFC) = alb_s + fl * (alb_l - alb_s);
    // forcing.f90:84-97.  qref is get_qsat's sig <= 0 form on psfc/psfc: its denominator ps(1,1) - 0.378 qsat is 1.0 * 1.0 -
    // 0.378 qsat of the sig > 0 form, the same bits
    const double tsfc = fl * at(SM_STL_AM) + fs * at(SM_SST_AM);
    const double tref = tsfc + a.gamlat * a.phis0[i];
    const double psfc = pow(tsfc / tref, a.pexp);
    const double qref = get_qsat(tref, psfc / psfc, 1.0);
    const double qsfc = get_qsat(tsfc, psfc, 1.0);
    at(SM_CORH) = refrh1 * (qref - qsfc);
}

template <class Args>
hipError_t launch(void (*k)(Args), const Args &a, hipStream_t s)
{
    if (a.ncol <= 0 || !a.f || a.nmem < 1 || a.nmem > 65535) return hipErrorInvalidValue;
    const dim3 grd((unsigned)((a.ncol + SURF_BLOCK - 1) / SURF_BLOCK), (unsigned)a.nmem), blk(SURF_BLOCK);
    hipLaunchKernelGGL(k, grd, blk, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_surface_couple(const SurfCols &a, hipStream_t s)
{
    if (!a.date || (a.day != 0 && !(a.hfluxn && a.shf && a.evap && a.ssrd))) return hipErrorInvalidValue;
    return launch(surface_couple_kernel, a, s);
}

hipError_t launch_surface_forcing(const SurfForcingCols &a, hipStream_t s)
{
    if (!a.phis0) return hipErrorInvalidValue;
    return launch(surface_forcing_kernel, a, s);
}

}  // namespace spdy
