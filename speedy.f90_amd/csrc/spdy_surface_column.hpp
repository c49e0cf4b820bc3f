// Column physics on the device: the surface fluxes of get_physical_tendencies (physics.f90:169-170; get_surface_fluxes,
// surface_fluxes.f90:97-295) and its boundary layer (physics.f90:193-205; get_vertical_diffusion_tend,
// vertical_diffusion.f90:57-142, the surface-flux tendencies of the lowest level and the four sums).
//
// Two launches, because the up half of the radiation lies between them in the reference's order of the ttend sums
// ((ttend + tt_rsw) + tt_rlw before + tt_pbl): surface_fluxes_kernel turns the down half's ssrd / slrd into the ts and
// slru(:,:,3) the up half reads and the four averaged fluxes, pbl_kernel reads those after the up half.
//
// SPPT (physics.f90:208-222; sppt_on is .false. in params.f90) follows the boundary layer: csrc/spdy_sppt.hip makes the pattern and
// brackets the five calls, csrc/spdy_column_chain.hip applies it in the one launch.  Out of scope, as in the reference's own
// configuration: the second get_surface_fluxes call (sea_coupling_flag > 0, lfluxland = .false.: the reference's
// sea model stops with "not implemented" for those flags and that path reads ks unset).  Only lfluxland = .true. is built.
//
// Reproduced as they are: fhum0 = 0, so both rel_hum_to_spec_hum branches are dead, q1 = qa(:,:,kx) and rh is never read -- it
// is not an argument here; hfluxn(:,:,2) = .. - slru + shf + alhc*evap (plus); t0 is computed twice and denvvs(:,:,0) uses the
// first; ftemp0*t1 + gtemp0*t2 with ftemp0 = 1, gtemp0 = 0 is still evaluated; x**2.0 = x*x, x**3.0 = x*(x*x), x**4.0 a pow call,
// as the reference's build has them.
//
// Layout and launch as every column kernel (csrc/spdy_columns.hpp).  The surface kernel touches only (ix, il) fields and the
// levels kx - 1, kx, loaded at their runtime address.  pbl_kernel holds the column TOP DOWN, k = 0 .. kx-1 for the reference's
// level k + 1, unrolled over KMAX with k < kx predicates; what the shallow convection reads at kx - 1 and kx is loaded at the
// runtime address, so no per-thread array is indexed at run time.  No contraction, the reference's association order.
#pragma once
#include <hip/hip_runtime.h>

#include "spdy_columns.hpp"

namespace spdy {
namespace surface {

// physical_constants.f90:21-29, mod_radcon.f90:27, surface_fluxes.f90:12-34, vertical_diffusion.f90:19-26
__device__ constexpr double kP0 = F(1.e+5f), kAlhc = F(2501.0f), kSbc = F(5.67e-8f), kEmisfc = F(0.98f);
__device__ constexpr double kFwind0 = F(0.95f), kFtemp0 = F(1.0f), kCdl = F(2.4e-3f), kCds = F(1.0e-3f), kChl = F(1.2e-3f);
__device__ constexpr double kChs = F(0.9e-3f), kVgust = F(5.0f), kCtday = F(1.0e-2f), kDtheta = F(3.0f), kFstab = F(0.67f);
__device__ constexpr double kClambda = F(7.0f), kClambsn = F(7.0f);
__device__ constexpr double kRedshc = F(0.5f), kSegrad = F(0.1f);

// surface_fluxes.f90:158-166, :229-236: the stability correction's potential temperature difference
__device__ inline double stability_dth(double tsfc, double t2)
{
#pragma clang fp contract(off)
    const double astab = 0.5, d = tsfc - t2;
    if (tsfc > t2) return kDtheta < d ? kDtheta : d;                   // min(dtheta, d)
    const double s = astab * d;
    return -kDtheta > s ? -kDtheta : s;                               // max(-dtheta, astab*d)
}

// For the column gid (< nb * ncol), with the down half's ssrd and slrd of the column.  ts, fsfcu and the four averaged fluxes
// come back in registers; a.ts, a.fsfcu and a.flux3 are written where they are set (the C ABI requires them, the chain does not).
template <int KMAX, class Args>
__device__ __forceinline__ SfcHand surface_fluxes_column(const Args &a, long gid, double ssrd, double slrd)
{
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    const long okx = c.base + (long)(kx - 1) * ncol, onl1 = okx - ncol;
    const long col = c.col;

    const double psa = exp(a.pslg[gid]);
    const double ua = a.ug[okx], va = a.vg[okx], ta = a.tg[okx], tb = a.tg[onl1], phi = a.phig[okx];
    const double qg = a.qg[okx];
    const double qa = qg > 0.0 ? qg : 0.0;                            // physics.f90:113
    const double fmask = a.fmask[gid], tsea = a.sst[gid], stl = a.stl[gid], soilw = a.soilw[gid], snowc = a.snowc[gid];
    const double alb_l = a.alb_l[gid], alb_s = a.alb_s[gid];
    const double phi0 = a.phis0[col], forog = a.forog[col], sqcoa = a.sqcoa[col / a.ix];

    const double cp = kCp, rgas = a.rgas;
    const double esbc = kEmisfc * kSbc;
    // 1. extrapolation of wind, temperature and density to the surface
    const double u0 = kFwind0 * ua, v0 = kFwind0 * va;
    const double gtemp0 = 1.0 - kFtemp0, rcp = 1.0 / cp;
    const double dt1 = a.wvi2_kx * (ta - tb);
    double t11 = ta + dt1;
    double t12 = t11 - phi0 * dt1 / (rgas * 288.0 * a.sigl_kx);
    const double t22 = ta + rcp * phi;
    const double t21 = t22 - rcp * phi0;
    if (ta > tb) {
        t11 = kFtemp0 * t11 + gtemp0 * t21;
        t12 = kFtemp0 * t12 + gtemp0 * t22;
    } else {
        t11 = ta;
        t12 = ta;
    }
    const double t0 = t12 + fmask * (t11 - t12);
    const double den0 = (kP0 * psa / (rgas * t0)) * sqrt(u0 * u0 + v0 * v0 + kVgust * kVgust);
    // 2. land: fluxes at the prescribed skin temperature
    double tskin = stl + kCtday * sqcoa * ssrd * (1.0 - alb_l) * psa;
    const double rdth = kFstab / kDtheta;
    const double den1 = den0 * (1.0 + stability_dth(tskin, t21) * rdth);
    const double cdldv = kCdl * den0 * forog;
    const double ustr1 = -cdldv * ua, vstr1 = -cdldv * va;
    const double chlcp = kChl * cp;
    double shf1 = chlcp * den1 * (tskin - t11);
    const double q1 = qa;
    const double qs1 = get_qsat(tskin, psa, 1.0);
    const double dq = soilw * qs1 - q1;
    double evap1 = kChl * den1 * (0.0 > dq ? 0.0 : dq);
    // 3. land: energy balance, skin temperature and fluxes adjusted
    const double tsk3 = tskin * (tskin * tskin);
    const double dslr = 4.0 * esbc * tsk3;
    double slru1 = esbc * tsk3 * tskin;
    double hf1 = ssrd * (1.0 - alb_l) + slrd - (slru1 + shf1 + kAlhc * evap1);
    const double clamb = kClambda + snowc * (kClambsn - kClambda);
    hf1 = hf1 - clamb * (tskin - stl);
    double qs2 = get_qsat(tskin + 1.0, psa, 1.0);
    qs2 = evap1 > 0.0 ? soilw * (qs2 - qs1) : 0.0;
    const double dtskin = hf1 / (clamb + dslr + kChl * den1 * (cp + kAlhc * qs2));
    tskin = tskin + dtskin;
    shf1 = shf1 + chlcp * den1 * dtskin;
    evap1 = evap1 + kChl * den1 * qs2 * dtskin;
    slru1 = slru1 + dslr * dtskin;
    hf1 = clamb * (tskin - stl);
    // 4. sea
    const double den2 = den0 * (1.0 + stability_dth(tsea, t22) * rdth);
    const double cdsdv = kCds * den2;
    const double ustr2 = -cdsdv * ua, vstr2 = -cdsdv * va;
    const double shf2 = kChs * cp * den2 * (tsea - t12);
    const double qss = get_qsat(tsea, psa, 1.0);
    const double evap2 = kChs * den2 * (qss - q1);
    const double slru2 = esbc * pow(tsea, 4.0);
    const double hf2 = ssrd * (1.0 - alb_s) + slrd - slru2 + shf2 + kAlhc * evap2;
    // weighted averages
    const double ustr3 = ustr2 + fmask * (ustr1 - ustr2), vstr3 = vstr2 + fmask * (vstr1 - vstr2);
    const double shf3 = shf2 + fmask * (shf1 - shf2), evap3 = evap2 + fmask * (evap1 - evap2);
    const double slru3 = slru2 + fmask * (slru1 - slru2);

    const double ts = tsea + fmask * (stl - tsea);
    if (a.ts) a.ts[gid] = ts;
    if (a.fsfcu) a.fsfcu[gid] = slru3;
    if (a.flux3) {
        double *const f3 = a.flux3 + c.b * 4 * ncol + col;
        f3[0] = ustr3;
        f3[ncol] = vstr3;
        f3[2L * ncol] = shf3;
        f3[3L * ncol] = evap3;
    }
    const long o3 = c.b * 3 * ncol + col;
    auto put3 = [&](double *p, double x1, double x2, double x3) {
        if (p) { p[o3] = x1; p[o3 + ncol] = x2; p[o3 + 2L * ncol] = x3; }
    };
    put3(a.ustr, ustr1, ustr2, ustr3);
    put3(a.vstr, vstr1, vstr2, vstr3);
    put3(a.shf, shf1, shf2, shf3);
    put3(a.evap, evap1, evap2, evap3);
    put3(a.slru, slru1, slru2, slru3);
    if (a.hfluxn) { a.hfluxn[c.b * 2 * ncol + col] = hf1; a.hfluxn[c.b * 2 * ncol + col + ncol] = hf2; }
    if (a.tskin) a.tskin[gid] = tsea + fmask * (tskin - tsea);
    if (a.u0) a.u0[gid] = u0;
    if (a.v0) a.v0[gid] = v0;
    if (a.t0) a.t0[gid] = t12 + fmask * (t11 - t12);
    return SfcHand{ts, slru3, {ustr3, vstr3, shf3, evap3}};
}

// For the column gid (< nb * ncol), with the moist block's icnv and the surface call's four averaged fluxes of the column
template <int KMAX, class Args>
__device__ __forceinline__ void pbl_column(const Args &a, long gid, int icnv, const double (&flux3)[4])
{
    // the threshold decisions (dmse >= 0, drh >= drh0, se < se0) must see the reference's roundings: no contraction
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    const long base = c.base;
    const long okx = base + (long)(kx - 1) * ncol, onl1 = okx - ncol;

    double se[KMAX], rh[KMAX], qs[KMAX], phi[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        se[k] = rh[k] = qs[k] = phi[k] = 0.0;
        if (k < kx) {
            const long o = base + (long)k * ncol;
            se[k] = a.se[o]; rh[k] = a.rh[o]; qs[k] = a.qsat[o]; phi[k] = a.phig[o];
        }
    }
    double tt[KMAX], qt[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) tt[k] = qt[k] = 0.0;

    // 2. shallow convection (vertical_diffusion.f90:80-108): levels nl1 = kx - 1 and kx at their runtime address
    {
        const double se_kx = a.se[okx], se_nl1 = a.se[onl1], rh_kx = a.rh[okx], rh_nl1 = a.rh[onl1];
        const double qs_kx = a.qsat[okx], qs_nl1 = a.qsat[onl1];
        const double qg = a.qg[okx];
        const double qa_kx = qg > 0.0 ? qg : 0.0;
        const double dmse = se_kx - se_nl1 + kAlhc * (qa_kx - qs_nl1);
        const double drh = rh_kx - rh_nl1;
        double tn = 0.0, tk = 0.0, qn = 0.0, qk = 0.0;             // the (nl1, kx) values, before the level's rsig
        bool tset = false, qset = false;
        if (dmse >= 0.0) {
            const double fcnv = icnv > 0 ? kRedshc : 1.0;
            const double fluxse = fcnv * a.fshcse * dmse;
            tn = fluxse; tk = -fluxse; tset = true;
            if (drh >= 0.0) {
                const double fluxq = fcnv * a.fshcq * qs_kx * drh;
                qn = fluxq; qk = -fluxq; qset = true;
            }
        } else {
            double drh0 = 0.0, fvdiq2 = 0.0;
#pragma unroll
            for (int k = 0; k + 1 < KMAX; ++k)
                if (k == kx - 2) { drh0 = a.drh0[k]; fvdiq2 = a.fvdiq2[k]; }
            if (drh > drh0) {
                const double fluxq = fvdiq2 * qs_nl1 * drh;
                qn = fluxq; qk = -fluxq; qset = true;
            }
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k == kx - 2) {
                if (tset) tt[k] = tn * a.rsig[k];
                if (qset) qt[k] = qn * a.rsig[k];
            } else if (k == kx - 1) {
                if (tset) tt[k] = tk * a.rsig[k];
                if (qset) qt[k] = qk * a.rsig[k];
            }
        }
    }

    // 3. vertical diffusion of moisture above the PBL (:111-129): do k = 3, kx - 2 where sigh(k) > 0.5
#pragma unroll
    for (int k = 2; k + 1 < KMAX; ++k)
        if (k <= kx - 3 && ((a.diffmask >> k) & 1)) {
            const double drh = rh[k + 1] - rh[k];
            if (drh >= a.drh0[k]) {
                const double fluxq = a.fvdiq2[k] * qs[k] * drh;
                qt[k] = qt[k] + fluxq * a.rsig[k];
                qt[k + 1] = qt[k + 1] - fluxq * a.rsig[k + 1];
            }
        }

    // 4. damping of super-adiabatic lapse rate (:132-141).  Level m receives, in the reference's order, - fluxse(k)*rsig1(k) of
    // every firing k < m (k ascending) and then + fluxse(m)*rsig(m): a register triangle, no running sum
    double dn[KMAX], upk[KMAX];                                        // fluxse(k)*rsig1(k), fluxse(k)*rsig(k) of the firing levels
    int fire = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        dn[k] = upk[k] = 0.0;
        if (k + 1 < KMAX && k < kx - 1) {
            const double se0 = se[k + 1] + kSegrad * (phi[k] - phi[k + 1]);
            if (se[k] < se0) {
                const double fluxse = a.fvdise * (se0 - se[k]);
                fire |= 1 << k;
                upk[k] = fluxse * a.rsig[k];
                dn[k] = fluxse * a.rsig1[k];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < KMAX; ++m)
        if (m < kx) {
#pragma unroll
            for (int k = 0; k < m; ++k)
                if ((fire >> k) & 1) tt[m] = tt[m] - dn[k];
            if ((fire >> m) & 1) tt[m] = tt[m] + upk[m];
        }

    // physics.f90:197-205: the surface-flux tendencies of level kx and the four sums
    const double rps = 1.0 / exp(a.pslg[gid]);
    const double ut = 0.0 + flux3[0] * rps * a.grdsig_kx;
    const double vt = 0.0 + flux3[1] * rps * a.grdsig_kx;
    const double dtk = flux3[2] * rps * a.grdscp_kx, dqk = flux3[3] * rps * a.grdsig_kx;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < kx) {
            if (k == kx - 1) { tt[k] = tt[k] + dtk; qt[k] = qt[k] + dqk; }
            const long o = base + (long)k * ncol;
            if (a.tt_pbl) a.tt_pbl[o] = tt[k];
            if (a.qt_pbl) a.qt_pbl[o] = qt[k];
            a.ttend[o] = a.ttend[o] + tt[k];
            a.qtend[o] = a.qtend[o] + qt[k];
        }
    // ut_pbl / vt_pbl are zero above kx: utend / vtend are read and written at level kx only (the reference's + 0.0 at the other
    // levels changes no bit but the sign of a -0.0)
    a.utend[okx] = a.utend[okx] + ut;
    a.vtend[okx] = a.vtend[okx] + vt;
    if (a.ut_pbl) a.ut_pbl[gid] = ut;
    if (a.vt_pbl) a.vt_pbl[gid] = vt;
}

}  // namespace surface
}  // namespace spdy
