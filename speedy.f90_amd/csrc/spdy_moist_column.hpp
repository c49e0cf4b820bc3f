// Column physics on the device: the precipitation block of get_physical_tendencies (physics.f90:110-138) -- thermodynamic
// fields, spec_hum_to_rel_hum (humidity.f90:16-28, get_qsat :46-79), deep convection (convection.f90:26-235) with the
// scaling of its fluxes, and large-scale condensation (large_scale_condensation.f90:32-83).
//
// Layout and launch as every column kernel (csrc/spdy_columns.hpp).  The reference addresses the convection scheme from the
// surface up (kx, kx-1, kx-3 .. 3, itop .. kx-1), so the column is held in registers BOTTOM UP: r = kx - k for the reference's
// level k (r = 0 is the lowest level).  With the level count a runtime value every index the scheme uses is then a compile-time r, the loops are
// unrolled over KMAX with r < kx predicates, and no per-thread array is ever indexed at run time (which would put it in
// scratch).  The per-level tables come in the kernel arguments in the same bottom-up order.
#pragma once
#include <hip/hip_runtime.h>

#include "spdy_columns.hpp"

namespace spdy {

// The block for the column gid (< nb * ncol).  What the later blocks of the chain read per column comes back in registers too.
template <int KMAX, class Args>
__device__ __forceinline__ MoistHand moist_column(const Args &a, long gid)
{
    // the threshold decisions (psa > psmin, mss0 > mss2, dqa < 0, ...) must see the reference's roundings: no contraction
#pragma clang fp contract(off)
    const int kx = a.kx, ncol = a.ncol;
    const Column c(gid, ncol, kx);
    const long base = c.base;          // level k (1-based) of this column at base + (k - 1) * ncol
    auto at = [&](int r) { return base + (long)(kx - 1 - r) * ncol; };

    // physical_constants.f90:22-26, convection.f90:15-20, :46-49, large_scale_condensation.f90:24, :50-52
    const double cp = kCp, alhc = F(2501.0f);
    const double psmin = F(0.8f), rhbl = F(0.9f), rhil = F(0.7f), smf = F(0.8f), fqmax = 5.0;
    const double rdps = 2.0 / (1.0 - psmin), rlhc = 1.0 / alhc;
    const double rtlsc = 1.0 / (F(4.0f) * 3600.0), tfact = alhc / cp;

    // physics.f90:110-120: psg, rps, the clamp of qg, se; then qsat and rh level by level
    const double psa = exp(a.pslg[gid]);
    const double rps = 1.0 / psa;
    double se[KMAX], qa[KMAX], qs[KMAX];
#pragma unroll
    for (int r = 0; r < KMAX; ++r) {
        se[r] = qa[r] = qs[r] = 0.0;
        if (r < kx) {
            const long o = at(r);
            const double tg = a.tg[o], q = a.qg[o];
            qa[r] = q > 0.0 ? q : 0.0;                                 // max(qg, 0.0)
            se[r] = cp * tg + a.phig[o];
            qs[r] = get_qsat(tg, psa, a.fsg[r]);
            if (a.se) a.se[o] = se[r];
            if (a.qsat) a.qsat[o] = qs[r];
            if (a.rh) a.rh[o] = qa[r] / qs[r];
        }
    }

    // convection.f90:158-235 diagnose_convection: rt = kx - itop of the convective top, -1 where there is none (itop = kx + 1)
    int rt = -1;
    double qdif = 0.0;
    if (psa > psmin) {
        const double mse0 = se[0] + alhc * qa[0];
        double mse1 = se[1] + alhc * qa[1];
        mse1 = mse0 < mse1 ? mse0 : mse1;
        const double mssb = se[0] + alhc * qs[0];
        const double mss0 = mse0 > mssb ? mse0 : mssb;
        int rk1 = 0, rk2 = 0;
        double msthr = 0.0;
#pragma unroll
        for (int r = 3; r < KMAX; ++r)                                // do k = kx-3, 3, -1 (empty for kx = 5)
            if (r <= kx - 3) {
                const double mr = se[r] + alhc * qs[r], mr1 = se[r - 1] + alhc * qs[r - 1];
                const double mss2 = mr + a.wvi2[r] * (mr1 - mr);
                if (mss0 > mss2) rk1 = r;
                if (mse1 > mss2) { rk2 = r; msthr = mss2; }
            }
        if (rk1 > 0) {
            const double qthr0 = rhbl * qs[0], qthr1 = rhbl * qs[1];
            const bool lqthr = qa[0] > qthr0 && qa[1] > qthr1;
            if (rk2 > 0) {
                rt = rk1;
                const double d0 = qa[0] - qthr0, d1 = (mse0 - msthr) * rlhc;
                qdif = d0 > d1 ? d0 : d1;
            } else if (lqthr) {
                rt = rk1;
                qdif = qa[0] - qthr0;
            }
        }
    }

    // convection.f90:74-152: mass fluxes of the convective columns
    double dfse[KMAX], dfqa[KMAX];
#pragma unroll
    for (int r = 0; r < KMAX; ++r) dfse[r] = dfqa[r] = 0.0;
    double cbmf = 0.0, precnv = 0.0;
    if (rt > 0) {
        const double q1 = 1.01f * qa[0];
        const double qmax = q1 > qs[0] ? q1 : qs[0];
        double sb = se[1] + a.wvi2[1] * (se[0] - se[1]);
        double qb = qa[1] + a.wvi2[1] * (qa[0] - qa[1]);
        qb = qb < qa[0] ? qb : qa[0];
        const double f1 = (psa - psmin) * rdps;
        const double fpsa = psa * (1.0 < f1 ? 1.0 : f1);
        const double f2 = qdif / (qmax - qb);
        double fmass = a.fm0 * fpsa * (fqmax < f2 ? fqmax : f2);
        cbmf = fmass;
        double fus = fmass * se[0], fuq = fmass * qmax, fds = fmass * sb, fdq = fmass * qb;
        dfse[0] = fds - fus;
        dfqa[0] = fdq - fuq;
#pragma unroll
        for (int r = 1; r + 1 < KMAX; ++r)                            // do k = kx - 1, itop + 1, -1
            if (r < rt) {
                dfse[r] = fus - fds;
                dfqa[r] = fuq - fdq;
                const double enmass = a.entr[r] * psa * cbmf;
                fmass = fmass + enmass;
                fus = fus + enmass * se[r];
                fuq = fuq + enmass * qa[r];
                sb = se[r + 1] + a.wvi2[r + 1] * (se[r] - se[r + 1]);
                qb = qa[r + 1] + a.wvi2[r + 1] * (qa[r] - qa[r + 1]);
                fds = fmass * sb;
                fdq = fmass * qb;
                dfse[r] = dfse[r] + fds - fus;
                dfqa[r] = dfqa[r] + fdq - fuq;
                const double delq = rhil * qs[r] - qa[r];
                if (delq > 0.0) {
                    const double fsq = smf * cbmf * delq;
                    dfqa[r] = dfqa[r] + fsq;
                    dfqa[0] = dfqa[0] - fsq;
                }
            }
#pragma unroll
        for (int r = 1; r < KMAX; ++r)                                // top layer k = itop
            if (r == rt) {
                const double qsatb = qs[r] + a.wvi2[r] * (qs[r - 1] - qs[r]);
                const double pr = fuq - fmass * qsatb;
                precnv = pr > 0.0 ? pr : 0.0;
                dfse[r] = fus - fds + alhc * precnv;
                dfqa[r] = fuq - fdq - precnv;
            }
    }
    // physics.f90:129: icnv = kx - iptop, before the condensation lowers iptop
    const int icnv = rt;
    int itop = rt > 0 ? kx - rt : kx + 1;

    // physics.f90:124-127 (flux scaling, k >= 2), large_scale_condensation.f90:54-80 and physics.f90:134-135, level by level
    // from the top down so that precls sums k = 2 .. kx in the reference's order
    const double psa2 = psa * psa;
    double precls = 0.0;
#pragma unroll
    for (int r = KMAX - 1; r >= 0; --r)
        if (r < kx) {
            const long o = at(r);
            double tt = dfse[r], qt = dfqa[r], dtl = 0.0, dql = 0.0;
            if (r <= kx - 2) {
                tt = tt * rps * a.grdscp[r];
                qt = qt * rps * a.grdsig[r];
                const double dqa = a.rhref[r] * qs[r] - qa[r];
                if (dqa < 0.0) {
                    itop = kx - r < itop ? kx - r : itop;
                    dql = dqa * rtlsc;
                    const double lim = a.dqmax[r] * psa2;
                    dtl = tfact * (-dql < lim ? -dql : lim);
                }
                precls = precls - a.pfact[r] * dql;
            }
            a.ttend[o] = a.ttend[o] + tt + dtl;
            a.qtend[o] = a.qtend[o] + qt + dql;
        }
    precls = precls * psa;

    if (a.precnv) a.precnv[gid] = precnv;
    if (a.precls) a.precls[gid] = precls;
    if (a.cbmf) a.cbmf[gid] = cbmf;
    if (a.iptop) a.iptop[gid] = itop;
    if (a.icnv) a.icnv[gid] = icnv;
    return MoistHand{precnv, precls, itop, icnv};
}

}  // namespace spdy
