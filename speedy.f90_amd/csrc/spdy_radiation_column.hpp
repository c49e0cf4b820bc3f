// Column physics on the device: the radiation schemes of get_physical_tendencies (physics.f90:146-166 and :180-186) --
// clouds and the shortwave fluxes (shortwave_radiation.f90:74-234, :332-410), the downward longwave fluxes
// (longwave_radiation.f90:16-117) and the upward longwave fluxes (:120-194).
//
// The reference has two halves with the surface fluxes between them.  The down half is two launches: radiation_sw_kernel
// (compute_sw calls only: clouds, shortwave, the longwave transmissivities) and radiation_lwdown_kernel (downward longwave);
// together in one kernel they do not fit the register file at KMAX 16 without spilling.  The up half is radiation_up_kernel
// (upward longwave, then the temperature tendency).  What
// the reference keeps in module state between them and across steps (tau2, stratc, flux; the shortwave heating of the last
// shortwave step) is the caller's radiation state: rad_state_fields(kx) fields of ncol doubles per model state.
//
// Layout and launch as every column kernel (csrc/spdy_columns.hpp).  Levels are indexed TOP DOWN here, k = 0 .. kx-1 for the
// reference's level k + 1 (both schemes sweep from the top first); loops are unrolled over KMAX with k < kx predicates, so no
// per-thread array is indexed at run time.  What the reference reads at a level that depends on kx (nl1 = kx - 1, kx) is loaded
// from memory at that runtime address instead.  No contraction, and the reference's association order throughout.
#pragma once
#include <hip/hip_runtime.h>

#include "spdy_columns.hpp"

namespace spdy {
namespace radiation {

// physical_constants.f90:29; mod_radcon.f90:26-27; shortwave_radiation.f90:14-54
__device__ constexpr double kSbc = F(5.67e-8f), kEpslw = F(0.05f), kEmisfc = F(0.98f);

// fband(nint(ta), 1:4) (longwave_radiation.f90:197-220), evaluated in registers bit-equal to the plan's table (spdy_tables.cpp
// make_fband).  Fortran nint rounds half away from zero: round().  The index is clamped to the table's range [100, 400]; rows
// outside [200, 320] repeat the end rows there, so the row is that of clamp(nint(ta), 200, 320).  The clamp acts in double
// before the conversion (a NaN temperature takes row 200), so no temperature gives an undefined conversion.
__device__ inline void fband_row(double ta, double f[4])
{
#pragma clang fp contract(off)
    const double tc = fmin(fmax(ta, 100.0), 400.0);
    int n = static_cast<int>(round(tc));
    n = n < 200 ? 200 : n > 320 ? 320 : n;
    const double eps1 = 1.0 - kEpslw;
    const float d2 = static_cast<float>((n - 247) * (n - 247)), d3 = static_cast<float>((n - 282) * (n - 282));
    const float d4 = static_cast<float>((n - 315) * (n - 315));
    f[1] = static_cast<double>(0.148f - 3.0e-6f * d2) * eps1;
    f[2] = static_cast<double>(0.356f - 5.2e-6f * d3) * eps1;
    f[3] = static_cast<double>(0.314f + 1.0e-5f * d4) * eps1;
    f[0] = eps1 - (f[1] + f[2] + f[3]);
}

// longwave_radiation.f90:38-66: blackbody emission st4a(k,1) -> s1[k], st4a(k,2) -> s2[k].  Both kernels call this on the same
// temperatures, so the upward half recomputes the downward half's values bit for bit instead of storing them.
template <int KMAX, class Table>
__device__ inline void blackbody(const double (&ta)[KMAX], int kx, const Table &wvi2, double (&s1)[KMAX], double (&s2)[KMAX])
{
#pragma clang fp contract(off)
    double half[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        half[k] = 0.0;
        if (k + 1 < KMAX && k < kx - 1) half[k] = ta[k] + wvi2[k] * (ta[k + 1] - ta[k]);
    }
    s2[0] = 0.75 * ta[0] + 0.25 * half[0];
    s2[1] = 0.50 * ta[1] + 0.25 * (half[0] + half[1]);
#pragma unroll
    for (int k = 2; k < KMAX; ++k) {
        if (k < kx - 1) {
            const double g = half[k] - half[k - 1];
            s2[k] = 0.5 * (g > 0.0 ? g : 0.0);                        // 0.5*anis*max(..., 0.0), anis = 1.0
        } else {                                                      // k = kx - 1 (and unused levels)
            const double g = ta[k] - half[k - 1];
            s2[k] = 1.0 * (g > 0.0 ? g : 0.0);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        s1[k] = kSbc * pow(s2[k], 4.0);                               // st4a**4.0: a pow call in the reference's build
        s2[k] = 0.0;
    }
#pragma unroll
    for (int k = 2; k < KMAX; ++k) {
        const double st3a = kSbc * (ta[k] * (ta[k] * ta[k]));          // ta**3.0 = ta*(ta*ta) in the reference's build
        s1[k] = st3a * ta[k];
        s2[k] = 4.0 * st3a * s2[k];
    }
}

// The radiation state of this column: field f at st + f * ncol.  State fields: tau2 (k, jb) at jb * kx + k, stratc at 4 kx,
// tt_rsw at 4 kx + 2, flux at 5 kx + 2, the longwave dfabs at 5 kx + 6, slrd at 6 kx + 6 (rad_state_fields(kx) = 6 kx + 7).
template <class Args>
__device__ inline double *column_state(const Args &a, const Column &c)
{
    return a.state + c.b * a.ncol * rad_state_fields(a.kx) + c.col;
}

// physics.f90:147-162 and shortwave_radiation.f90:74-234, :332-410 (compute_sw calls only): gse, clouds, the shortwave
// fluxes and heating, and the longwave transmissivities and stratospheric terms the longwave halves read from the state.
// For the column gid (< nb * ncol), with the moist block's precnv, precls and iptop of the column; returns ssrd.
template <int KMAX, class Args>
__device__ __forceinline__ double radiation_sw_column(const Args &a, long gid, double precnv, double precls, int iptop)
{
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    const long base = c.base;
    double *const st = column_state(a, c);
    const int j = (int)(c.col / a.ix);                                // latitude row
    auto S = [&](int f) -> double & { return st[(long)f * ncol]; };
    const int f_tau = 0, f_stratc = 4 * kx, f_ttrsw = 4 * kx + 2;
    auto qa_at = [&](long o) { const double q = a.qg[o]; return q > 0.0 ? q : 0.0; };   // qg = max(qg, 0.0), local

    const double psa = exp(a.pslg[gid]);                              // physics.f90:110-111
    const double rps = 1.0 / psa;

    // physics.f90:147: gse from the two lowest levels
    const long o1 = base + (long)(kx - 2) * ncol, o2 = base + (long)(kx - 1) * ncol;
    const double se1 = kCp * a.tg[o1] + a.phig[o1], se2 = kCp * a.tg[o2] + a.phig[o2];
    const double gse = (se1 - se2) / (a.phig[o1] - a.phig[o2]);

    // clouds (shortwave_radiation.f90:332-410)
    const double rhcl1 = F(0.30f), rhcl2 = F(1.00f), qacl = F(0.20f), wpcl = F(0.2f), pmaxcl = F(10.0f);
    const double clsmax = F(0.60f), clsminl = F(0.15f), gse_s0 = F(0.25f), gse_s1 = F(0.40f);
    const double rrcl = 1. / (rhcl2 - rhcl1);
    int icltop = kx + 1;
    double cloudc = 0.0;
    const double rhnl1 = a.rh[o1];
    if (rhnl1 > rhcl1) { cloudc = rhnl1 - rhcl1; icltop = kx - 1; }
#pragma unroll
    for (int k = 2; k < KMAX; ++k)                                    // do k = 3, kx - 2
        if (k <= kx - 3) {
            const long o = base + (long)k * ncol;
            const double drh = a.rh[o] - rhcl1;
            if (drh > cloudc && qa_at(o) > qacl) { cloudc = drh; icltop = k + 1; }
        }
    const double p8 = F(86.4f) * (precnv + precls);
    const double pr1 = pmaxcl < p8 ? pmaxcl : p8;
    const double c1 = cloudc * rrcl;
    const double m = 1.0 < c1 ? 1.0 : c1;
    const double cc = wpcl * sqrt(pr1) + m * m;                        // min(1.0, cloudc*rrcl)**2.0 = m*m in the reference's build
    cloudc = 1.0 < cc ? 1.0 : cc;
    const int ipt = iptop;
    icltop = ipt < icltop ? ipt : icltop;
    const double qcloud = qa_at(o1);                                  // qcloud = qa(:,:,nl1)
    const double clfact = F(1.2f), rgse = 1.0 / (gse_s1 - gse_s0);
    const double g1 = rgse * (gse - gse_s0);
    const double g2 = 1.0 < g1 ? 1.0 : g1;
    const double fstab = 0.0 > g2 ? 0.0 : g2;
    const double cs = clsmax - clfact * cloudc;
    double clstr = fstab * (cs > 0.0 ? cs : 0.0);
    const double cl = clstr > clsminl ? clstr : clsminl;
    const double clstrl = cl * a.rh[o2];
    clstr = clstr + a.fmask[gid] * (clstrl - clstr);

    // get_shortwave_rad_fluxes (shortwave_radiation.f90:74-234)
    const double albcl = F(0.43f), albcls = F(0.50f), abscl1 = F(0.015f), abscl2 = F(0.15f);
    const double absdry = F(0.033f), abswv1 = F(0.022f), abswv2 = F(15.000f);
    const double fband2 = F(0.05f), fband1 = 1.0 - fband2;
    const double *z = a.zonal;
    const int il = a.il;
    const double fsol = z[j], ozone = z[il + j], ozupp = z[2 * il + j], zenit = z[3 * il + j], stratz = z[4 * il + j];
    // 1. tau2(:,:,:,3): albcl*cloudc at icltop (<= kx), then albcls*clstr at kx.  Only icltop and kx hold a value: t3cl, t3kx.
    // (icltop = 2 is never scaled by the flux in 3.3 but still enters 4.2 -- the reference's order, kept.)
    double t3cl = icltop <= kx - 1 ? albcl * cloudc : 0.0;
    double t3kx = albcls * clstr;
    // 2. transmissivities; 3. downward flux, bands 1 and 2 level by level (each dfabs(k) takes band 1, then band 2)
    const double psaz = psa * zenit;
    const double ac = abscl1 * qcloud;
    const double acloud = cloudc * (ac < abscl2 ? ac : abscl2);
    double t1[KMAX], d[KMAX];
    double ftop = fsol, f1 = fsol * fband1, f2 = fsol * fband2;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        t1[k] = d[k] = 0.0;
        if (k < kx) {
            const double qa = qa_at(base + (long)k * ncol);
            if (k == 0) t1[k] = exp(-psaz * a.dhs[0] * absdry);
            else if (k < kx - 1 && k + 1 >= icltop) t1[k] = exp(-psaz * a.dhs[k] * (a.abs1[k] + abswv1 * qa + acloud));
            else t1[k] = exp(-psaz * a.dhs[k] * (a.abs1[k] + abswv1 * qa));
            if (k == 0) {                                             // 3.2: ozone and dry air in the stratosphere
                d[k] = f1;
                f1 = t1[k] * (f1 - ozupp * psa);
                d[k] = d[k] - f1;
            } else if (k == 1) {
                d[k] = f1;
                f1 = t1[k] * (f1 - ozone * psa);
                d[k] = d[k] - f1;
            } else {                                                  // 3.3: absorption and reflection in the troposphere
                double t3 = 0.0;
                if (k == kx - 1) { t3kx = f1 * t3kx; t3 = t3kx; }
                else if (k + 1 == icltop) { t3cl = f1 * t3cl; t3 = t3cl; }
                f1 = f1 - t3;
                d[k] = f1;
                f1 = t1[k] * f1;
                d[k] = d[k] - f1;
            }
            if (k >= 1) {                                             // band 2, k = 2 .. kx
                const double t2 = exp(-psaz * a.dhs[k] * abswv2 * qa);
                d[k] = d[k] + f2;
                f2 = t2 * f2;
                d[k] = d[k] - f2;
            }
        }
    }
    // 4.1 surface; 4.2 upward flux (tau2(k,3) is t3kx at kx, t3cl at icltop <= kx-1, 0 elsewhere)
    const double fsfcd = f1 + f2;
    f1 = f1 * a.albsfc[gid];
    const double fsfc = fsfcd - f1;
#pragma unroll
    for (int k = KMAX - 1; k >= 0; --k)
        if (k < kx) {
            d[k] = d[k] + f1;
            f1 = t1[k] * f1;
            d[k] = d[k] - f1;
            f1 = f1 + (k == kx - 1 ? t3kx : k + 1 == icltop ? t3cl : 0.0);
        }
    ftop = ftop - f1;
    // physics.f90:160-162: tt_rsw, held in the state for the steps without shortwave
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < kx) {
            const double tt = d[k] * rps * a.grdscp[k];
            S(f_ttrsw + k) = tt;
            if (a.tt_rsw) a.tt_rsw[base + (long)k * ncol] = tt;
        }
    if (a.ssrd) a.ssrd[gid] = fsfcd;
    if (a.ssr) a.ssr[gid] = fsfc;
    if (a.tsr) a.tsr[gid] = ftop;
    if (a.cloudc) a.cloudc[gid] = cloudc;
    if (a.clstr) a.clstr[gid] = clstr;
    if (a.icltop) a.icltop[gid] = icltop;

    // 5.1 longwave transmissivities, into the state
    const double ablwin = F(0.3f), ablco2 = F(6.0f), ablwv1 = F(0.7f), ablwv2 = F(50.0f), ablcl1 = F(12.0f), ablcl2 = F(0.6f);
    const double acl = cloudc * ablcl2;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < kx) {
            const double dh = a.dhs[k];
            double tau[4];
            if (k == 0) {
                tau[0] = exp(-psa * dh * ablwin);
                tau[1] = exp(-psa * dh * ablco2);
                tau[2] = 1.0;
                tau[3] = 1.0;
            } else if (k == 1 || k == kx - 1) {                       // do k = 2, kx, kx - 2: levels 2 and kx only
                const double qa = qa_at(base + (long)k * ncol);
                tau[0] = exp(-psa * dh * ablwin);
                tau[1] = exp(-psa * dh * ablco2);
                tau[2] = exp(-psa * dh * ablwv1 * qa);
                tau[3] = exp(-psa * dh * ablwv2 * qa);
            } else {                                                  // cloudy layers 3 .. nl1
                const double qa = qa_at(base + (long)k * ncol);
                const double deltap = psa * dh;
                const double acloud1 = k + 1 < icltop ? acl : ablcl1 * cloudc;
                const double w1 = ablwv1 * qa, w2 = ablwv2 * qa;
                tau[0] = exp(-deltap * (ablwin + acloud1));
                tau[1] = exp(-deltap * ablco2);
                tau[2] = exp(-deltap * (w1 > acl ? w1 : acl));
                tau[3] = exp(-deltap * (w2 > acl ? w2 : acl));
            }
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) S(f_tau + jb * kx + k) = tau[jb];
        }
    // 5.2 stratospheric correction terms
    S(f_stratc) = stratz * psa;
    S(f_stratc + 1) = a.eps1 * psa;
    return fsfcd;
}

// get_downward_longwave_rad_fluxes (longwave_radiation.f90:16-117), level by level from the top, with the transmissivities of
// the state (made by the last radiation_sw_kernel on it)
// For the column gid (< nb * ncol); returns slrd.
template <int KMAX, class Args>
__device__ __forceinline__ double radiation_lwdown_column(const Args &a, long gid)
{
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    double *const st = column_state(a, c);
    auto S = [&](int f) -> double & { return st[(long)f * ncol]; };
    const int f_tau = 0, f_flux = 5 * kx + 2, f_dfabs = 5 * kx + 6, f_slrd = 6 * kx + 6;

    double ta[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) ta[k] = k < kx ? a.tg[c.base + (long)k * ncol] : 0.0;
    double s1[KMAX], s2[KMAX];
    blackbody<KMAX>(ta, kx, a.wvi2, s1, s2);
    double flux[4] = {0.0, 0.0, 0.0, 0.0}, corlw = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < kx) {
            double fb[4];
            fband_row(ta[k], fb);
            double dk = 0.0;
            if (k == 0) {                                             // 3.1 stratosphere, bands 1 and 2
#pragma unroll
                for (int jb = 0; jb < 2; ++jb) {
                    const double emis = 1.0 - S(f_tau + jb * kx + k);
                    const double brad = fb[jb] * (s1[k] + emis * s2[k]);
                    flux[jb] = emis * brad;
                    dk = dk - flux[jb];
                }
            } else {                                                  // 3.2 troposphere, every band
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const double tau = S(f_tau + jb * kx + k);
                    const double emis = 1.0 - tau;
                    const double brad = fb[jb] * (s1[k] + emis * s2[k]);
                    dk = dk + flux[jb];
                    flux[jb] = tau * flux[jb] + emis * brad;
                    dk = dk - flux[jb];
                }
            }
            if (k == kx - 1) {                                        // 3.4 "black" band correction
                corlw = kEpslw * kEmisfc * s1[k];
                dk = dk - corlw;
            }
            S(f_dfabs + k) = dk;
        }
    double fsfcd = 0.0;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        fsfcd = fsfcd + kEmisfc * flux[jb];
        S(f_flux + jb) = flux[jb];
    }
    fsfcd = fsfcd + corlw;
    S(f_slrd) = fsfcd;
    if (a.slrd) a.slrd[gid] = fsfcd;
    return fsfcd;
}

// physics.f90:180-186 for the column gid (< nb * ncol), with the surface call's ts and fsfcu of the column
template <int KMAX, class Args>
__device__ __forceinline__ void radiation_up_column(const Args &a, long gid, double ts, double fsfcu)
{
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    const long base = c.base;
    double *const st = column_state(a, c);
    auto S = [&](int f) { return st[(long)f * ncol]; };
    const int f_tau = 0, f_stratc = 4 * kx, f_ttrsw = 4 * kx + 2, f_flux = 5 * kx + 2, f_dfabs = 5 * kx + 6, f_slrd = 6 * kx + 6;

    const double psa = exp(a.pslg[gid]);
    const double rps = 1.0 / psa;
    double ta[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) ta[k] = k < kx ? a.tg[base + (long)k * ncol] : 0.0;
    double s1[KMAX], s2[KMAX];
    blackbody<KMAX>(ta, kx, a.wvi2, s1, s2);

    // get_upward_longwave_rad_fluxes (longwave_radiation.f90:120-194)
    const double refsfc = 1.0 - kEmisfc;
    const double fsfc = fsfcu - S(f_slrd);
    double fs[4], flux[4];
    fband_row(ts, fs);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) flux[jb] = fs[jb] * fsfcu + refsfc * S(f_flux + jb);
    const double stratc1 = S(f_stratc), stratc2 = S(f_stratc + 1);
    double corlw1 = 0.0, corlw2 = 0.0;
#pragma unroll
    for (int k = KMAX - 1; k >= 0; --k)
        if (k < kx) {
            double dk = S(f_dfabs + k);
            if (k == kx - 1) dk = dk + kEpslw * fsfcu;                 // "black" band correction
            double fb[4];
            fband_row(ta[k], fb);
            const int nbnd = k == 0 ? 2 : 4;                          // 4.2 troposphere: every band; 4.3 stratosphere: 1 and 2
#pragma unroll
            for (int jb = 0; jb < 4; ++jb)
                if (jb < nbnd) {
                    const double tau = S(f_tau + jb * kx + k);
                    const double emis = 1.0 - tau;
                    const double brad = fb[jb] * (s1[k] - emis * s2[k]);
                    dk = dk + flux[jb];
                    flux[jb] = tau * flux[jb] + emis * brad;
                    dk = dk - flux[jb];
                }
            if (k == 1) {                                             // polar night / black band corrections of levels 1, 2
                corlw2 = a.dhs[1] * stratc2 * s1[1];
                dk = dk - corlw2;
            } else if (k == 0) {
                corlw1 = a.dhs[0] * stratc2 * s1[0] + stratc1;
                dk = dk - corlw1;
            }
            // physics.f90:182-186
            const long o = base + (long)k * ncol;
            const double tt = dk * rps * a.grdscp[k];
            if (a.tt_rlw) a.tt_rlw[o] = tt;
            a.ttend[o] = a.ttend[o] + S(f_ttrsw + k) + tt;
        }
    double ftop = corlw1 + corlw2;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) ftop = ftop + flux[jb];
    if (a.slr) a.slr[gid] = fsfc;
    if (a.olr) a.olr[gid] = ftop;
}

}  // namespace radiation
}  // namespace spdy
