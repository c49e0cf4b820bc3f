// SPPT on the device (sppt.f90; physics.f90:85-88, :207-222): the noise of gen_sppt with a counter-based generator, the AR(1)
// update in spectral space, the clip of the transformed pattern, and the save / apply kernels that bracket the five calls of
// the column physics.  The inverse transform between the update and the clip is the plan's own (csrc/spdy_api_sppt.hip).
//
// The generator is Philox4x32-10 as include/spdy.h defines it (csrc/spdy_philox.hpp, with the reference's randn): key (seed lo,
// seed hi), counter (coefficient index in storage order inside the member, part, draws lo, draws hi), so a coefficient's noise
// depends on (seed, draws, index) only -- not on the launch geometry, and not on the ensemble the member travels in.
#include "spdy_philox.hpp"

namespace spdy {
namespace {

constexpr int SPPT_BLOCK = 256;

// min(lim, |x|) * sign(1, x) (sppt.f90:66-68, :98)
__device__ inline double sppt_clip(double x, double lim) { return fmin(lim, fabs(x)) * copysign(1.0, x); }

// the member is blockIdx.y: its own {draws, seed}, its own branch, and the generator's index counts inside the member, so member e
// draws what a one-member object with its seed draws and the 32-bit counter word is bounded by mx * nx * kx whatever nmem is
__global__ __launch_bounds__(SPPT_BLOCK) void sppt_noise_kernel(const SpptNoise a)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * SPPT_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const SpptState *const st = a.state + blockIdx.y;
    const unsigned long long draws = st->draws, seed = st->seed;
    const long o = 2 * ((long)blockIdx.y * a.n + i);
    double re, im;
    if (a.eta_in) {
        re = a.eta_in[o]; im = a.eta_in[o + 1];
    } else {
        re = sppt_randn((unsigned)i, 0u, draws, seed); im = sppt_randn((unsigned)i, 1u, draws, seed);
    }
    re = sppt_clip(re, 10.0); im = sppt_clip(im, 10.0);
    a.eta[o] = re; a.eta[o + 1] = im;
    const double sg = a.sigma[i % a.nspec];
    double sr, si;
    if (draws == 0) {                                 // sppt.f90:84, left to right
        const double c = a.first * sg;
        sr = c * re; si = c * im;
    } else {                                          // :89
        sr = a.phi * a.spec[o] + sg * re; si = a.phi * a.spec[o + 1] + sg * im;
    }
    a.spec[o] = sr; a.spec[o + 1] = si;
}

__global__ __launch_bounds__(SPPT_BLOCK) void sppt_clip_kernel(double *pattern, long n, SpptState *state)
{
    const long i = (long)blockIdx.x * SPPT_BLOCK + threadIdx.x;
    // every launch before this one on the stream has read the counter (the noise kernel), every launch after it sees the new one
    if (i == 0) state[blockIdx.y].draws = state[blockIdx.y].draws + 1;
    if (i < n) pattern[(long)blockIdx.y * n + i] = sppt_clip(pattern[(long)blockIdx.y * n + i], 1.0);
}

__global__ __launch_bounds__(COLUMN_BLOCK) void sppt_save_kernel(const SpptCols a)
{
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    const Column c(gid, a.ncol, a.kx);
    double *const st = a.save, *const sq = a.save + (size_t)a.kx * a.g, *const su = a.save + (size_t)2 * a.kx * a.g;
    for (int k = 0; k < a.kx; ++k) {
        const long o = c.base + (long)k * a.ncol;
        st[o] = a.ttend[o]; sq[o] = a.qtend[o];
    }
    const long okx = c.base + (long)(a.kx - 1) * a.ncol;
    su[gid] = a.utend[okx]; su[a.g + gid] = a.vtend[okx];
}

__global__ __launch_bounds__(COLUMN_BLOCK) void sppt_apply_kernel(const SpptCols a)
{
#pragma clang fp contract(off)
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    const Column c(gid, a.ncol, a.kx);
    const double *const st = a.save, *const sq = a.save + (size_t)a.kx * a.g, *const su = a.save + (size_t)2 * a.kx * a.g;
    for (int k = 0; k < a.kx; ++k) {
        const long o = c.base + (long)k * a.ncol;
        const double f = 1 + a.pattern[o] * a.mu[k];
        a.ttend[o] = f * (a.ttend[o] - st[o]) + st[o];
        a.qtend[o] = f * (a.qtend[o] - sq[o]) + sq[o];
        if (k == a.kx - 1) {                          // ut_pbl, vt_pbl are zero above level kx
            const double ud = su[gid], vd = su[a.g + gid];
            a.utend[o] = f * (a.utend[o] - ud) + ud;
            a.vtend[o] = f * (a.vtend[o] - vd) + vd;
        }
    }
}

bool cols_ok(const SpptCols &a)
{
    return a.kx >= 5 && a.kx <= COLUMN_KMAX && a.nb >= 0 && a.ncol > 0 && (size_t)a.nb * a.ncol <= a.g && a.pattern && a.utend &&
           a.vtend && a.ttend && a.qtend && a.save;
}

dim3 column_grid(const SpptCols &a) { return dim3((unsigned)(((long)a.nb * a.ncol + COLUMN_BLOCK - 1) / COLUMN_BLOCK)); }

}  // namespace

hipError_t launch_sppt_noise(const SpptNoise &a, hipStream_t s)
{
    if (a.n <= 0 || a.nspec <= 0 || a.n % a.nspec || a.nmem < 1 || a.nmem > 65535 || !a.state || !a.sigma || !a.eta || !a.spec)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sppt_noise_kernel, dim3((a.n + SPPT_BLOCK - 1) / SPPT_BLOCK, a.nmem), dim3(SPPT_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sppt_clip(double *pattern, long n, int nmem, SpptState *state, hipStream_t s)
{
    if (n <= 0 || nmem < 1 || nmem > 65535 || !pattern || !state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sppt_clip_kernel, dim3((unsigned)((n + SPPT_BLOCK - 1) / SPPT_BLOCK), nmem), dim3(SPPT_BLOCK), 0, s, pattern, n,
                       state);
    return hipGetLastError();
}

hipError_t launch_sppt_save(const SpptCols &a, hipStream_t s)
{
    if (!cols_ok(a)) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    hipLaunchKernelGGL(sppt_save_kernel, column_grid(a), dim3(COLUMN_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sppt_apply(const SpptCols &a, hipStream_t s)
{
    if (!cols_ok(a)) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    hipLaunchKernelGGL(sppt_apply_kernel, column_grid(a), dim3(COLUMN_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdy
