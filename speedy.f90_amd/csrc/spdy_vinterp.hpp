// Vertical interpolation of one model column to a target coordinate by np.interp's rule (include/spdy.h, "pressure-level
// output"): the bracket of a target among the kx full levels, and the value on it.  Device functions only, for every kernel that
// needs a column on a pressure: the column itself is never held by the thread -- the bracket is found from the level table
// (wave-uniform, in the kernel-argument struct) and the member's surface pressure, and the two levels it names are then loaded
// by address.  Each operation is rounded once: every function here is compiled without contraction.
#pragma once

#include <hip/hip_runtime.h>

namespace spdy {

constexpr int VINTERP_KMAX = 32;          // SPDY_MAX_KX (include/spdy.h)

// the model levels' table as a kernel argument: fsg[k] (linear in p) or ln fsg[k] (linear in ln p), ascending
struct VLevels {
    int kx;
    double lev[VINTERP_KMAX];
};

// the coordinate of level k.  LOG false: X_k = P * fsg[k] with P the surface pressure in Pa; LOG true: X_k = ln(ps/p0) + ln fsg[k]
template <bool LOG>
__device__ __forceinline__ double vinterp_coord(double a, double lev)
{
#pragma clang fp contract(off)
    return LOG ? a + lev : a * lev;
}

// Where a target x lies in a column.  kb in [0, max(kx - 2, 0)]: the level at which the target's bracket starts, so that kb and
// min(kb + 1, kx - 1) are the two levels to load.  cls, a set of bits (an integer, so that it lives in a vector register like kb:
// a bool per lane would hold a pair of scalar registers each): VINTERP_LO: x <= X_0 (or kx == 1), the value is level kb's = level
// 0's; VINTERP_HI: x >= X_{kx-1}, the value is level kb + 1's = level kx-1's; VINTERP_BELOW: x > X_{kx-1}; VINTERP_NAN: the
// caller's, the value is NaN whatever the levels hold.  With neither LO nor HI, X_kb <= x < X_{kb+1} and w = (x - X_kb) /
// (X_{kb+1} - X_kb).
enum { VINTERP_LO = 1, VINTERP_HI = 2, VINTERP_BELOW = 4, VINTERP_NAN = 8 };
struct VBracket {
    int kb, cls;
    double w;
};

// The brackets of one target in N columns (a[r]: column r's surface pressure in Pa, LOG false, or ln(ps/p0), LOG true).  The trip
// count is kx and k is wave-uniform: one level of the table per trip, a select per column, no branch, and no bound or address that
// depends on a[r] -- a NaN or infinite a[r] leaves kb inside its range (the column's values are the caller's to replace).
template <bool LOG, int N>
__device__ __forceinline__ void vinterp_brackets(const VLevels &lv, const double (&a)[N], double x, VBracket (&b)[N])
{
#pragma clang fp contract(off)
    const int kx = lv.kx;
    const double l0 = lv.lev[0];
    double xlo[N], xhi[N], xl[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        xlo[r] = xhi[r] = xl[r] = vinterp_coord<LOG>(a[r], l0);
        b[r].kb = 0;
        b[r].cls = kx == 1 || x <= xlo[r] ? VINTERP_LO : 0;
    }
#pragma nounroll
    for (int k = 1; k < kx; ++k) {
        const double lk = lv.lev[k];
        const bool inner = k < kx - 1;                     // a bracket may start at k
#pragma unroll
        for (int r = 0; r < N; ++r) {
            xl[r] = vinterp_coord<LOG>(a[r], lk);          // X_k; after the last trip X_{kx-1}
            xhi[r] = b[r].kb == k - 1 ? xl[r] : xhi[r];    // the bracket started at k - 1 so far: X_k ends it
            const bool adv = inner && xl[r] <= x;          // X_k <= x: it starts at k or later
            b[r].kb += adv ? 1 : 0;
            xlo[r] = adv ? xl[r] : xlo[r];
        }
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
        b[r].cls |= (x >= xl[r] ? VINTERP_HI : 0) | (x > xl[r] ? VINTERP_BELOW : 0);
        b[r].w = (x - xlo[r]) / (xhi[r] - xlo[r]);
    }
}

// the value on the target from the two loaded levels f0 = f[kb], f1 = f[min(kb + 1, kx - 1)]: the end level's bits where the
// target is outside the column, f0 + w * (f1 - f0) inside, NaN for a bracket marked VINTERP_NAN
__device__ __forceinline__ double vinterp_value(const VBracket &b, double f0, double f1)
{
#pragma clang fp contract(off)
    const double d = f1 - f0, y = f0 + b.w * d;
    const double v = (b.cls & VINTERP_LO) ? f0 : ((b.cls & VINTERP_HI) ? f1 : y);
    return (b.cls & VINTERP_NAN) ? __longlong_as_double(0x7ff8000000000000LL) : v;
}

}  // namespace spdy
