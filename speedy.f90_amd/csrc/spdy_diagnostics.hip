// check_diagnostics on the device (diagnostics.f90:16-75): per level the eddy kinetic energy of the rotational and of the
// divergent flow, reke = sum_{m>=2, n} elm2(m,n) |vor(m,n,k)|^2 and deke likewise (the reference's -Re(inverse_laplacian(x) conjg(x))
// with inverse_laplacian = -x elm2, spectral.f90:91-96: the zonal column m = 1 left out, the whole (mx,nx) rectangle summed), the
// mean temperature temp = sqrt(0.5) Re t(1,1,k), and the reference's range test.  The step number, the history ring and the
// sticky first offence live in device memory (include/spdy.h, "diagnostics"), so ONE captured launch records step s, s + 1, ...
// on successive replays.
//
// Shape: one workgroup per level, DIAG_BLOCK threads.  Thread i of the workgroup owns coefficients i, i + DIAG_BLOCK, ... of its
// level in storage order; the partial sums go down a fixed shuffle tree inside each wave and the wave sums through LDS to thread
// 0, which adds them in wave order.  So a sum depends on the level's values and on elm2 only: no atomics, no other workgroup's
// result, the same bits on every run.  Every term is >= 0, so the order costs rounding only (2 (N - 1) 2^-53 relative at worst).
// Each level keeps its own slice of the state, its own copy of the step counter included, and is written by its workgroup's thread
// 0 alone with ordinary vector stores.  The one thing a workgroup reads of the others is their bad_step, to stop refreshing its
// saved row once any level has tripped at an EARLIER step: what this launch writes there is the current step s, which that test
// (bad_step < s) ignores whether it is seen or not, so the read does not depend on the order the workgroups run in.
//
// nmem members: a (kx, nmem) grid.  Workgroup (k, e) is the single object's workgroup k on member e's slice of the spectra, on
// state[e][.] and on block e of the history row: the same thread-to-coefficient map and reduction tree, so the same bits.  The
// "earlier offence" scan reads the member's own kx levels only: a member that trips freezes its own saved row and no other's.
#include "spdy_kernels.hpp"

namespace spdy {
namespace {

constexpr int DIAG_BLOCK = 1024, DIAG_WAVES = DIAG_BLOCK / 64;
// diagnostics.f90:33: sqrt(0.5) is a default-real expression, the float32 value 0.707106769084930419921875 widened
constexpr double DIAG_SQRT_HALF = 0x1.6a09e6p-1;

__device__ inline double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;                                         // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(DIAG_BLOCK) void diagnostics_kernel(const DiagArgs a)
{
    __shared__ double part[2][DIAG_WAVES];
    const int k = blockIdx.x, mem = blockIdx.y, tid = threadIdx.x;
    DiagLevel *const mine = a.state + (size_t)mem * a.kx, *const me = mine + k;   // the member's levels, this level
    const size_t ms = 2 * (size_t)mem * a.kx * a.nspec;                          // the member's (mx, nx, kx) slice (doubles)
    const long long s = me->next_step;                // read by every thread before the barrier, written by thread 0 after it
    int earlier = 0;                                  // some level's first offence lies before this step: the saved row is final
    for (int j = tid; j < a.kx; j += DIAG_BLOCK) {
        const long long b = mine[j].bad_step;
        earlier |= b >= 0 && b < s;
    }
    double t0 = 0.0, lim[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid == 0) {
        t0 = a.t[ms + 2 * (size_t)k * a.nspec];
        for (int i = 0; i < 4; ++i) lim[i] = a.limits[i];
    }
    const double *const v = a.vor + ms + 2 * (size_t)k * a.nspec, *const d = a.div + ms + 2 * (size_t)k * a.nspec;
    double sv = 0.0, sd = 0.0;
    for (int i = tid; i < a.nspec; i += DIAG_BLOCK) {
        const double e = a.elm2[i], vr = v[2 * i], vi = v[2 * i + 1], dr = d[2 * i], di = d[2 * i + 1];
        const bool eddy = i % a.mx != 0;              // m = 1 of the reference is not read: a select, so no value there can reach the sum
        sv += eddy ? e * (vr * vr + vi * vi) : 0.0;
        sd += eddy ? e * (dr * dr + di * di) : 0.0;
    }
    sv = wave_sum(sv); sd = wave_sum(sd);
    if ((tid & 63) == 0) { part[0][tid >> 6] = sv; part[1][tid >> 6] = sd; }
    const int frozen = __syncthreads_or(earlier);
    if (tid != 0) return;
    double reke = 0.0, deke = 0.0;
    for (int w = 0; w < DIAG_WAVES; ++w) { reke += part[0][w]; deke += part[1][w]; }
    const double temp = DIAG_SQRT_HALF * t0;          // one load, one multiply: bit for bit the reference's
    // diagnostics.f90:61-62 as written: strict, so a NaN trips none of the four
    int mask = (reke > lim[0] ? DIAG_REKE : 0) | (deke > lim[1] ? DIAG_DEKE : 0) | (temp < lim[2] ? DIAG_TEMP_LOW : 0) |
               (temp > lim[3] ? DIAG_TEMP_HIGH : 0);
    if (!(isfinite(reke) && isfinite(deke) && isfinite(temp))) mask |= DIAG_NONFINITE;
    double *const row = a.history + ((size_t)(s % a.capacity) * a.nmem + mem) * 3 * a.kx;
    row[k] = reke; row[a.kx + k] = deke; row[2 * a.kx + k] = temp;
    if (!frozen) {                                    // until a level trips every level's saved row follows the step
        me->row_step = s;
        me->row[0] = reke; me->row[1] = deke; me->row[2] = temp;
    }
    if (mask && me->bad_step < 0) { me->bad_step = s; me->bad_mask = mask; }   // the first offence stays
    me->next_step = s + 1;
}

// The guard's sticky records as a member mask (include/spdy.h, "member mask"): one thread per member reads its kx records.
__global__ __launch_bounds__(64) void diagnostics_use_kernel(const DiagLevel *const state, const int nmem, const int kx, int *const use)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nmem) return;
    int ok = 1;
    for (int k = 0; k < kx; ++k) ok = state[(size_t)e * kx + k].bad_step < 0 ? ok : 0;
    use[e] = ok;
}

}  // namespace

hipError_t launch_diagnostics_use(const DiagLevel *state, int nmem, int kx, int *use, hipStream_t s)
{
    if (!state || !use || nmem < 1 || kx < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diagnostics_use_kernel, dim3((unsigned)((nmem + 63) / 64)), dim3(64), 0, s, state, nmem, kx, use);
    return hipGetLastError();
}

hipError_t launch_diagnostics(const DiagArgs &a, hipStream_t s)
{
    if (a.kx <= 0 || a.mx <= 0 || a.nspec <= 0 || a.nspec % a.mx || a.capacity < 1 || !a.vor || !a.div || !a.t || !a.elm2 ||
        !a.limits || !a.history || !a.state || a.nmem < 1 || a.nmem > 65535)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(diagnostics_kernel, dim3((unsigned)a.kx, (unsigned)a.nmem), dim3(DIAG_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdy
