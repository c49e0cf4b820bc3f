// The nature run on the device (include/spdy.h, "nature run"): the observation values of an analysis object's
// network drawn from the gridded truth with counter-based noise, the advance of the draw counter, and the scores of a gridded
// ensemble against the truth.  The transforms in front of them are the plan's own (csrc/spdy_api_nature.hip).
//
// Everything here is bit-reproducible: no atomics, every sum in a fixed order (members ascending, a fixed tree over a latitude's
// points, latitudes ascending), every loop with a fixed bound.  A row's scores are formed from that row's grids by that row's
// workgroups and thread only, so a non-finite value stays in its row.  No contraction, as in the other column kernels.
#include "spdy_obsop.hpp"
#include "spdy_philox.hpp"

namespace spdy {
namespace {

constexpr int NATURE_BLOCK = 256;        // observations per workgroup of the draw kernel, rows per workgroup of the final sums
constexpr int NATURE_SCORE_BLOCK = 128;  // threads of a (row, latitude) workgroup: two waves, one pass over T30's 96 longitudes

// The draw of the observations [first, last) of the network (the whole network: [0, nobs); include/spdy.h, "observations in time
// slots"): thread o - first forms h as the analysis forms a member's hx (csrc/spdy_obsop.hpp), the truth being the one member --
// row v * kx + k of it on a model level (lev is 0 for ps); PRESSURE, a network that holds an observation at a pressure, by
// obsop_pressure with the truth's ps, clamped to the end level outside the column -- and adds the noise with the counter of o
// itself, so a slot's draw is the whole network's draw on its range.
template <bool PRESSURE>
__global__ __launch_bounds__(NATURE_BLOCK) void nature_slot_draw_kernel(const NatureObs a)
{
#pragma clang fp contract(off)
    const int o = a.first + blockIdx.x * NATURE_BLOCK + threadIdx.x;
    if (o >= a.last) return;
    const int v = a.var[o], lev = a.lev[o];
    const ObsStencil st = obsop_stencil(a.sidx, a.swgt, o);
    const double *const f = a.truth + (size_t)v * a.kx * a.ncol;
    double h;
    if constexpr (!PRESSURE)
        h = obsop_level(f + (size_t)lev * a.ncol, st);
    else
        h = obsop_pressure(f, a.truth + (size_t)4 * a.kx * a.ncol, v < 4 ? a.kx : 1, a.ncol, a.atp[o] != 0, lev, a.lnp[o], a.lv, st).h;
    if (a.noise == 0.0) {
        a.value[o] = h;
        return;
    }
    const double z = sppt_randn((unsigned)o, 0u, a.state[1], a.state[0]);
    a.value[o] = h + (a.noise * a.error[o]) * z;
}

__global__ void nature_count_kernel(unsigned long long *state)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = state[1] + 1;
}

// one workgroup per (latitude j, row f); EMAX bounds the members a thread keeps in registers (two passes: the mean, then the
// squared deviations from it).  MASK (include/spdy.h, "member mask"): a.use is read as it is, n counts its non-zero entries, a member
// not in use is never loaded and is skipped by a select, the sums take the others in ascending order, mbar = sum / n and s2 = sum /
// (n - 1); n = 1 gives s2 = +0, n = 0 NaN in all three.  No run-time branch: MASK = false is the kernel it was.
template <int EMAX, bool MASK>
__global__ __launch_bounds__(NATURE_SCORE_BLOCK) void nature_zonal_kernel(const NatureScore a)
{
#pragma clang fp contract(off)
    __shared__ double wave_sum[NATURE_SCORE_BLOCK / 64][3];
    const int j = blockIdx.x, f = blockIdx.y, E = a.nmem, kx = a.kx, tid = threadIdx.x;
    const size_t ncol = (size_t)a.ix * a.il;
    const int v = f < 4 * kx ? f / kx : 4, k = f < 4 * kx ? f % kx : 0;
    const double *const x = a.x[v] + (size_t)k * ncol + (size_t)j * a.ix;       // member 0 (letkf_at)
    const size_t member = v < 4 ? (size_t)kx * ncol : ncol;
    const double *const truth = a.truth + (size_t)f * ncol + (size_t)j * a.ix;
    double s_m = 0.0, s_mm = 0.0, s_var = 0.0;
    unsigned in_use = 0xffffffffu;           // MASK: bit e = member e is in use; n of them
    int n = E;
    if constexpr (MASK) {
        in_use = 0u;
        n = 0;
        for (int e = 0; e < E; ++e)
            if (a.use[e] != 0) { in_use |= 1u << e; ++n; }
    }
    for (int i = tid; i < a.ix; i += NATURE_SCORE_BLOCK) {
        const double t = truth[i];
        double d[EMAX];
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E && (!MASK || (in_use >> e & 1u))) d[e] = x[e * member + i] - t;
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E && (!MASK || (in_use >> e & 1u))) sum = sum + d[e];
        const double m = sum / n;
        double q = 0.0;
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E && (!MASK || (in_use >> e & 1u))) {
                const double r = d[e] - m;
                q = q + r * r;
            }
        s_m = s_m + m;
        s_mm = s_mm + m * m;
        if constexpr (MASK)
            s_var = s_var + (n >= 2 ? q / (n - 1) : n == 1 ? 0.0 : m);      // n = 0: m is NaN
        else
            s_var = s_var + q / (E - 1);
    }
    // a fixed tree: lanes 32 apart, 16, ... 1, then the waves in ascending order
    for (int off = 32; off > 0; off >>= 1) {
        s_m = s_m + __shfl_down(s_m, off);
        s_mm = s_mm + __shfl_down(s_mm, off);
        s_var = s_var + __shfl_down(s_var, off);
    }
    if ((tid & 63) == 0) {
        wave_sum[tid >> 6][0] = s_m; wave_sum[tid >> 6][1] = s_mm; wave_sum[tid >> 6][2] = s_var;
    }
    __syncthreads();
    if (tid < 3) {
        double s = wave_sum[0][tid];
        for (int w = 1; w < NATURE_SCORE_BLOCK / 64; ++w) s = s + wave_sum[w][tid];
        a.part[((size_t)f * a.il + j) * 3 + tid] = s;
    }
}

__global__ __launch_bounds__(NATURE_BLOCK) void nature_final_kernel(const NatureScore a)
{
#pragma clang fp contract(off)
    const int nrows = 4 * a.kx + 1, f = blockIdx.x * NATURE_BLOCK + threadIdx.x;
    if (f >= nrows) return;
    double m = 0.0, mm = 0.0, var = 0.0;
    for (int j = 0; j < a.il; ++j) {
        const double *const p = a.part + ((size_t)f * a.il + j) * 3;
        const double g = a.gw[j];
        m = m + g * (p[0] / a.ix);
        mm = mm + g * (p[1] / a.ix);
        var = var + g * (p[2] / a.ix);
    }
    a.scores[f] = sqrt(mm);
    a.scores[nrows + f] = m;
    a.scores[2 * nrows + f] = sqrt(var);
}

}  // namespace

hipError_t launch_nature_slot_draw(const NatureObs &a, hipStream_t s)
{
    if (a.first < 0 || a.last < a.first || a.last > a.nobs || a.kx < 1 || a.ncol < 1 || !a.truth || !a.state || !a.value || !(a.noise >= 0.0))
        return hipErrorInvalidValue;
    if (a.atp && (a.kx < 2 || a.kx > VINTERP_KMAX || a.lv.kx != a.kx || !a.lnp)) return hipErrorInvalidValue;
    if (a.last == a.first) return hipSuccess;
    if (!a.var || !a.lev || !a.sidx || !a.swgt || !a.error) return hipErrorInvalidValue;
    const dim3 grid((a.last - a.first + NATURE_BLOCK - 1) / NATURE_BLOCK), block(NATURE_BLOCK);
    if (a.atp)
        hipLaunchKernelGGL(nature_slot_draw_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(nature_slot_draw_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_nature_count(unsigned long long *state, hipStream_t s)
{
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nature_count_kernel, dim3(1), dim3(64), 0, s, state);
    return hipGetLastError();
}

hipError_t launch_nature_score(const NatureScore &a, hipStream_t s)
{
    if (a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.kx < 1 || a.ix < 1 || a.il < 1 || !a.truth || !a.gw || !a.part || !a.scores)
        return hipErrorInvalidValue;
    for (int v = 0; v < LETKF_VARS; ++v)
        if (!a.x[v]) return hipErrorInvalidValue;
    const int nrows = 4 * a.kx + 1;
    const dim3 grid(a.il, nrows), block(NATURE_SCORE_BLOCK);
    if (a.use) {
        if (a.nmem <= 8)
            hipLaunchKernelGGL((nature_zonal_kernel<8, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((nature_zonal_kernel<LETKF_MAX_MEMBERS, true>), grid, block, 0, s, a);
    } else if (a.nmem <= 8)
        hipLaunchKernelGGL((nature_zonal_kernel<8, false>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((nature_zonal_kernel<LETKF_MAX_MEMBERS, false>), grid, block, 0, s, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(nature_final_kernel, dim3((nrows + NATURE_BLOCK - 1) / NATURE_BLOCK), dim3(NATURE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdy
