// The observation operator H x of the ensemble analysis and the nature run: the bilinear stencil of an
// observation, a member's value on a model level and at a pressure, and the step that couples the members of one observation.
// Device functions only, for every kernel that observes (csrc/spdy_letkf.hip, csrc/spdy_nature.hip): each formula is written here
// and nowhere else, so the kernels differ in their thread layout and in where a row is kept, never in what they compute.  "A
// member" is a field base and a ps base: a member of a gridded ensemble, or the nature run's truth rows.  Each operation is rounded
// once: every function here is compiled without contraction.  No atomics, every sum in a fixed order (stencil points as the host
// lists them, members ascending).
#pragma once

#include "spdy_kernels.hpp"

namespace spdy {

// the four grid points of observation o and their weights, as the host made them (csrc/spdy_api_letkf.hip, stencil)
struct ObsStencil {
    int idx[4];
    double w[4];
};

__device__ __forceinline__ ObsStencil obsop_stencil(const int *sidx, const double *swgt, int o)
{
#pragma clang fp contract(off)
    ObsStencil s;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        s.idx[n] = sidx[4 * (size_t)o + n];
        s.w[n] = swgt[4 * (size_t)o + n];
    }
    return s;
}

// the bilinear sum of four values on the stencil: this association, everywhere
__device__ __forceinline__ double obsop_bilinear(const ObsStencil &s, double z0, double z1, double z2, double z3)
{
#pragma clang fp contract(off)
    return ((s.w[0] * z0 + s.w[1] * z1) + s.w[2] * z2) + s.w[3] * z3;
}

// the field of variable v of a gridded ensemble by selects: a pointer array indexed per lane would go to scratch
__device__ __forceinline__ const double *obsop_field(const double *const (&x)[LETKF_VARS], int v)
{
#pragma clang fp contract(off)
    return v == 0 ? x[0] : v == 1 ? x[1] : v == 2 ? x[2] : v == 3 ? x[3] : x[4];
}

// the member's value on a model level; row: that level of the member's field (ps: its one level)
__device__ __forceinline__ double obsop_level(const double *row, const ObsStencil &s)
{
#pragma clang fp contract(off)
    const double z0 = row[s.idx[0]], z1 = row[s.idx[1]], z2 = row[s.idx[2]], z3 = row[s.idx[3]];
    return obsop_bilinear(s, z0, z1, z2, z3);
}

// The member's value at a pressure (include/spdy.h, "observations at a pressure").  f: the member's field of kl
// levels (ps: 1), pse: its ps, xo = ln(p_o / p0).  The brackets of the target in the four stencil columns come from their four ps
// (one loop of kx trips, csrc/spdy_vinterp.hpp); the two levels each bracket names are loaded by address, all eight loads before
// the first use.  atp false -- an observation on a model level, or of ps -- takes the same path with its bracket replaced by {lev,
// the level's own bits}, so the lanes of a wave do not diverge and h has obsop_level's bits.  ps: the bilinear sum of the stencil's
// ps; out: the target lies outside one of the four columns (never for atp false).  No array is indexed by a bracket.
struct ObsAtPressure {
    double h, ps;
    int out;
};

__device__ __forceinline__ ObsAtPressure obsop_pressure(const double *f, const double *pse, int kl, int ncol, bool atp, int lev, double xo,
                                                        const VLevels &lv, const ObsStencil &s)
{
#pragma clang fp contract(off)
    double ps[4], f0[4], f1[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) ps[n] = pse[s.idx[n]];
    const double l0 = lv.lev[0];
    VBracket b[4];
    vinterp_brackets<true, 4>(lv, ps, xo, b);
    int out = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int k0 = min(atp ? b[n].kb : lev, kl - 1), k1 = min(k0 + 1, kl - 1);
        f0[n] = f[(size_t)k0 * ncol + s.idx[n]];
        f1[n] = f[(size_t)k1 * ncol + s.idx[n]];
        out |= (atp && (xo < vinterp_coord<true>(ps[n], l0) || (b[n].cls & VINTERP_BELOW))) ? 1 : 0;
        b[n].cls = atp ? b[n].cls : VINTERP_LO;                    // a model level: f0's bits
    }
    double z[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) z[n] = vinterp_value(b[n], f0[n], f1[n]);
    return {obsop_bilinear(s, z[0], z[1], z[2], z[3]), obsop_bilinear(s, ps[0], ps[1], ps[2], ps[3]), out};
}

// One observation's row over the members, as the coupling step reads it: hx(e), and with PRESSURE ps(e), the stencil's ps_e, and
// out(e), the member's out-of-column flag.  ObsRow is a row that is kept: FLAG int in LDS, double in memory.  A kernel that forms
// its row while it is summed gives an accessor of its own.
template <class FLAG>
struct ObsRow {
    const double *h, *p;
    const FLAG *f;
    __device__ __forceinline__ double hx(int e) const { return h[e]; }
    __device__ __forceinline__ double ps(int e) const { return p[e]; }
    __device__ __forceinline__ int out(int e) const { return f[e] != 0 ? 1 : 0; }
};

// What couples the members of observation o: hxmean and dep, and with PRESSURE olns of an at-pressure observation, used and reff
// (1 / error^2, 0 where a member in use is out of its column).  The sums take the members in ascending order; MASK (the member
// mask, a.umap): those in use, by a select, divided by their number, so a member not in use may hold anything.  Returns the mean.
template <bool MASK, bool PRESSURE, class ROW>
__device__ __forceinline__ double obsop_couple(const LetkfObserve &a, int o, const ROW &row)
{
#pragma clang fp contract(off)
    const int E = a.nmem, n = MASK ? a.umap[0] : E;
    double sum = 0.0, psum = 0.0;
    int out = 0;
    for (int e = 0; e < E; ++e) {
        const bool u = !MASK || a.umap[LETKF_URANK + e] >= 0;
        const double h = row.hx(e);
        sum = u ? sum + h : sum;
        if constexpr (PRESSURE) {
            psum = u ? psum + row.ps(e) : psum;
            out |= u ? row.out(e) : 0;
        }
    }
    const double mean = sum / n;
    a.hxmean[o] = mean;
    a.dep[o] = a.value[o] - mean;
    if constexpr (PRESSURE) {
        if (a.atp[o] != 0) a.olns[o] = a.lnp[o] - psum / n;
        a.used[o] = out ? 0.0 : 1.0;
        a.reff[o] = out ? 0.0 : a.rinv[o];
    }
    return mean;
}

// y of member e from its hx and the mean: 0.0 for a member not in use
template <bool MASK>
__device__ __forceinline__ double obsop_anomaly(const LetkfObserve &a, int e, double h, double mean)
{
#pragma clang fp contract(off)
    return !MASK || a.umap[LETKF_URANK + e] >= 0 ? h - mean : 0.0;
}

}  // namespace spdy
