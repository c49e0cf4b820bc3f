// The ensemble analysis on the device (include/spdy.h, "ensemble analysis"): the observation-space quantities, the
// local ensemble transforms of every grid column and level -- or of a coarse list of columns, with the kernel that interpolates them
// to every column (weight interpolation) -- the kernel that adds the spectral increments to the prognostics, and the two kernels of
// observations in time slots: one keeps what is per member at a slot's time, one finishes it at analysis time.
// What the observation kernels compute is csrc/spdy_obsop.hpp's; here are their thread layouts.  The transforms
// around them are the plan's own (csrc/spdy_api_letkf.hip).
//
// Everything here is bit-reproducible: no atomics, every sum in a fixed order (observations ascending, members ascending), every
// loop with a fixed bound.  The Jacobi sweeps end at the convergence test or after LETKF_SWEEPS; a NaN fails every test, so a
// non-finite input runs the full count and leaves NaN, it does not hang.  No contraction, as in the other column kernels.
#include <type_traits>

#include "spdy_obsop.hpp"

namespace spdy {
namespace {

constexpr int LETKF_BLOCK = 256;     // threads of a column's workgroup: four waves
constexpr int LETKF_CHUNK = 256;     // observations scanned per step: one per thread
constexpr int LETKF_TILE = 16;       // observations in range staged in LDS per accumulation step
constexpr int LETKF_SWEEPS = 16;     // the most Jacobi sweeps (E = 32: 9 to 13 with many observations, up to 16 with fewer than members)
constexpr int LETKF_MAX_KX = 32;
constexpr double LETKF_REARTH = 6.371e6;
constexpr double LETKF_TOL = 0x1p-53;   // a pair with |a_pq| <= tol * sqrt(a_pp a_qq) is not rotated

// the workgroup's LDS, in doubles from the 16-byte aligned base; every offset is even
struct LetkfLds {
    int C, B, V, S, X, ty, rtab, td, lwh, lidx, misc, total;
    __host__ __device__ LetkfLds(int ep, int kx, int nlv)
    {
        int o = 0;
        C = o; o += kx * ep * ep;            // A = (E-1)/rho I + C of every level, later T of the level
        B = o; o += kx * ep;                 // b of every level
        V = o; o += nlv * ep * ep;           // eigenvectors, per level in flight
        S = o; o += nlv * 6 * ep;            // lambda | V^T b / lambda | sqrt((E-1)/lambda) | wbar | (c, s), (p, q) (int) of the pairs
        X = o; o += nlv * LETKF_VARS * ep;   // the members' values of the five variables
        ty = o; o += LETKF_TILE * ep;        // Y of the staged observations
        rtab = o; o += kx * LETKF_TILE;      // r = w / error^2 per level and staged observation
        td = o; o += LETKF_TILE;             // their departures
        lwh = o; o += LETKF_CHUNK;           // horizontal weights of the chunk's observations in range
        lidx = o; o += LETKF_CHUNK / 2;      // their indices (int)
        misc = o; o += (16 + LETKF_MAX_KX) / 2;   // int: wave counts [4], sweep flags [4], rotation marks [4], touched [kx]
        total = o;
    }
};

// Gaspari and Cohn (1999), eq. 4.10; support r < 2.  The inner branch in Horner form; the outer branch, r^5/12 - r^4/2 + 5r^3/8 +
// 5r^2/3 - 5r + 4 - 2/(3r), in its factored form (2 - r)^4 (r^2 + 2r - 1/2) / (12 r): the sum of powers cancels down to its last
// bits where the weight fades out, and a weight wrong by a few 1e-16 there, times 1/error^2, times a thousand observations, moves
// an analysis at the edge of their range by 1e-12; the product has no cancellation and cannot round below zero.
__device__ inline double letkf_gc(double r)
{
#pragma clang fp contract(off)
    if (!(r < 2.0)) return r != r ? r : 0.0;
    if (r <= 1.0) return (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * (r * r) + 1.0;
    const double s = 2.0 - r, s2 = s * s;
    return (s2 * s2) * ((r + 2.0) * r - 0.5) / (12.0 * r);
}

// round-robin pair m of round r among n (even) players: the last player stays, the others turn
__device__ inline void letkf_pair(int m, int r, int n, int &p, int &q)
{
    if (m == 0) { p = n - 1; q = r; return; }
    p = (r + m) % (n - 1);
    q = (r - m + n - 1) % (n - 1);
}

__device__ inline size_t letkf_at(int v, int e, int k, int kx, int ncol, int col)
{
    return v < 4 ? ((size_t)e * kx + k) * ncol + col : (size_t)e * ncol + col;
}

// The observation-space quantities of a model-level network: one thread per observation, the members in a loop.  Every member's
// hx is its own H x_e, formed and stored while the coupling step sums it (the accessor below); y is then written from the stored
// row.  MASK (the member mask, a.umap): the sums take the members in use, y of a member not in use is 0.0.  One body, two
// instantiations, no run-time branch.
struct LetkfLevelRow {
    const double *row0;      // member 0's level of the observed field
    size_t step;             // doubles from a member to the next
    const ObsStencil &s;
    double *hxo;             // the observation's row of hx
    __device__ __forceinline__ double hx(int e) const { return hxo[e] = obsop_level(row0 + e * step, s); }
};

template <bool MASK>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_obs_kernel(const LetkfObserve a)
{
#pragma clang fp contract(off)
    const int o = a.first + blockIdx.x * LETKF_BLOCK + threadIdx.x;
    if (o >= a.last) return;
    const int v = a.var[o], k = a.lev[o], E = a.nmem, kl = v < 4 ? a.kx : 1;      // levels of the field: ps has one, and lev 0
    const ObsStencil st = obsop_stencil(a.sidx, a.swgt, o);
    double *const hx = a.hx + (size_t)o * E;
    const double mean = obsop_couple<MASK, false>(a, o, LetkfLevelRow{obsop_field(a.x, v) + (size_t)k * a.ncol, (size_t)kl * a.ncol, st, hx});
    for (int e = 0; e < E; ++e) a.y[(size_t)o * E + e] = obsop_anomaly<MASK>(a, e, hx[e], mean);
}

// The member mask's table from the caller's use[nmem] (include/spdy.h, "member mask"): one wave, lane e owns member e; the compact
// index of a member in use is the number of members in use below it (ballot and prefix count, no atomics).
__global__ __launch_bounds__(64) void letkf_mask_kernel(const int *const use, const int nmem, int *const umap, double *const nused)
{
    const int e = threadIdx.x;
    const bool u = e < nmem && use[e] != 0;
    const unsigned long long mask = __ballot(u);
    const int rank = __popcll(mask & ((1ull << e) - 1ull)), n = __popcll(mask);
    if (u) umap[1 + rank] = e;
    if (e < nmem) umap[LETKF_URANK + e] = u ? rank : -1;
    if (e == 0) { umap[0] = n; *nused = (double)n; }
}

// The observation-space quantities of a network that holds observations given at a pressure (include/spdy.h, "observations at a
// pressure").  A workgroup owns LETKF_BLOCK / E whole observations.  Thread (observation, member) forms its member's
// value (obsop_pressure: an observation on a model level or of ps takes the same path, so the lanes of a wave do not diverge) and
// leaves hx_e, the stencil's ps_e and its out-of-column flag in LDS; thread (observation) then couples the members.  No atomics,
// every bound a kernel argument.  MASK (the member mask, a.umap): the thread layout is that of nmem and every member's hx is its
// own.  Two instantiations, no run-time branch.
template <bool MASK>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_pobs_kernel(const LetkfObserve a)
{
#pragma clang fp contract(off)
    __shared__ double shx[LETKF_BLOCK], spb[LETKF_BLOCK], smean[LETKF_BLOCK / 2];
    __shared__ int sout[LETKF_BLOCK];
    const int E = a.nmem, tid = threadIdx.x, opb = LETKF_BLOCK / E;
    const int slot = tid / E, e = tid - slot * E, o = a.first + blockIdx.x * opb + slot;
    const bool act = slot < opb && o < a.last;
    double h = 0.0;
    if (act) {
        const int v = a.var[o], kl = v < 4 ? a.kx : 1;             // levels of the field: ps has one
        const ObsAtPressure m = obsop_pressure(obsop_field(a.x, v) + (size_t)e * kl * a.ncol, a.x[4] + (size_t)e * a.ncol, kl, a.ncol,
                                               a.atp[o] != 0, a.lev[o], a.lnp[o], a.lv, obsop_stencil(a.sidx, a.swgt, o));
        h = m.h;
        a.hx[(size_t)o * E + e] = h;
        shx[tid] = h;
        spb[tid] = m.ps;
        sout[tid] = m.out;
    }
    __syncthreads();
    const int o1 = a.first + blockIdx.x * opb + tid;
    if (tid < opb && o1 < a.last) smean[tid] = obsop_couple<MASK, true>(a, o1, ObsRow<int>{shx + tid * E, spb + tid * E, sout + tid * E});
    __syncthreads();
    if (act) a.y[(size_t)o * E + e] = obsop_anomaly<MASK>(a, e, h, smean[slot]);
}

// Observing a time slot (include/spdy.h, "observations in time slots"): what is per member, and nothing that
// couples members.  Thread (observation of the slot, member) in letkf_pobs_kernel's layout, a workgroup owns LETKF_BLOCK / E whole
// observations of [first, last); no LDS, no barrier.  PRESSURE = false (a model-level network): obsop_level, it does not pay for
// brackets.  PRESSURE = true: obsop_pressure, and the stencil's ps_e and the member's out-of-column flag go to slot_ps and
// slot_out, as doubles, in the place of LDS.  No atomics, every bound a kernel argument.
template <bool PRESSURE>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_slot_obs_kernel(const LetkfObserve a)
{
#pragma clang fp contract(off)
    const int E = a.nmem, tid = threadIdx.x, opb = LETKF_BLOCK / E;
    const int slot = tid / E, e = tid - slot * E, o = a.first + blockIdx.x * opb + slot;
    if (slot >= opb || o >= a.last) return;
    const int v = a.var[o], lev = a.lev[o], kl = v < 4 ? a.kx : 1;  // levels of the field: ps has one
    const double *const f = obsop_field(a.x, v) + (size_t)e * kl * a.ncol;
    const ObsStencil st = obsop_stencil(a.sidx, a.swgt, o);
    if constexpr (!PRESSURE) {
        a.hx[(size_t)o * E + e] = obsop_level(f + (size_t)min(lev, kl - 1) * a.ncol, st);
    } else {
        const ObsAtPressure m = obsop_pressure(f, a.x[4] + (size_t)e * a.ncol, kl, a.ncol, a.atp[o] != 0, lev, a.lnp[o], a.lv, st);
        a.hx[(size_t)o * E + e] = m.h;
        a.slot_ps[(size_t)o * E + e] = m.ps;
        a.slot_out[(size_t)o * E + e] = m.out ? 1.0 : 0.0;
    }
}

// The finish of a slot analysis, in the observation kernel's place: one thread per observation couples the members from its row
// of hx (and, PRESSURE, of slot_ps and slot_out) in memory, so a member not in use may hold anything.  y is written row by row.
// Four instantiations, no run-time branch.
template <bool MASK, bool PRESSURE>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_slot_finish_kernel(const LetkfObserve a)
{
#pragma clang fp contract(off)
    const int o = a.first + blockIdx.x * LETKF_BLOCK + threadIdx.x;
    if (o >= a.last) return;
    const int E = a.nmem;
    const double *const hx = a.hx + (size_t)o * E;
    const double mean = obsop_couple<MASK, PRESSURE>(a, o, ObsRow<double>{hx, a.slot_ps + (size_t)o * E, a.slot_out + (size_t)o * E});
    for (int e = 0; e < E; ++e) a.y[(size_t)o * E + e] = obsop_anomaly<MASK>(a, e, hx[e], mean);
}

// LIST = false: one workgroup per grid column, which gets its increments.  LIST = true (weight interpolation): workgroup b solves
// grid column cols[b] and writes T of every level to tw, [b][k][f][e] with e fastest, and no increments.
// ARGS = LetkfMaskedCols (the member mask: MASK; include/spdy.h, "member mask"): E is n = umap[0], read once and the same for the workgroup,
// and everything below -- the diagonal, the padded size, the LDS layout, the pair schedule, the means -- is that of an object of n
// members; compact index e stands for member umap[1 + e] in every load of y and x and every store of dx; the members not in use
// get 0.0.  y, x, dx and tw keep the strides of NM = nmem members, and the launch shape, nlv and the LDS request are those of nmem
// (the layout of a smaller E fits).  n < 2: zero increments, nothing else.  Four instantiations, no run-time branch: those on
// LetkfCols are the kernels they were before the mask existed, instruction for instruction.
__device__ inline const LetkfCols &letkf_cols(const LetkfCols &a) { return a; }
__device__ inline const LetkfCols &letkf_cols(const LetkfMaskedCols &a) { return a.c; }
__device__ inline const int *letkf_umap(const LetkfCols &) { return nullptr; }
__device__ inline const int *letkf_umap(const LetkfMaskedCols &a) { return a.umap; }
__device__ inline double letkf_diag(const LetkfCols &a, int) { return a.diag; }
// (n - 1) / rho as one IEEE division: the bits the host gives an object of n members
__device__ inline double letkf_diag(const LetkfMaskedCols &a, int n) { return (double)(n - 1) / a.rho; }
// ARGS = LetkfAdaptiveCols, LetkfAdaptiveMaskedCols (adaptive inflation: ADAPT; include/spdy.h, "adaptive inflation"): the diagonal
// of level k is (n - 1) / rho[k][col], one IEEE division where C's diagonal is initialised -- the bits of an object whose scalar
// rho is that value; everything else is the plain or the masked kernel.  Four instantiations more, no LDS more.
__device__ inline const LetkfCols &letkf_cols(const LetkfAdaptiveCols &a) { return a.c; }
__device__ inline const LetkfCols &letkf_cols(const LetkfAdaptiveMaskedCols &a) { return a.c; }
__device__ inline const int *letkf_umap(const LetkfAdaptiveCols &) { return nullptr; }
__device__ inline const int *letkf_umap(const LetkfAdaptiveMaskedCols &a) { return a.umap; }
__device__ inline double letkf_diag(const LetkfAdaptiveCols &, int) { return 0.0; }            // not read: the diagonal is per level
__device__ inline double letkf_diag(const LetkfAdaptiveMaskedCols &, int) { return 0.0; }
template <class ARGS> __device__ inline double letkf_diag(const ARGS &a, int n, int k, int ncol, int col)
{
    return (double)(n - 1) / a.rho[(size_t)k * ncol + col];
}

template <bool LIST, class ARGS>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_transform_kernel(const ARGS args)
{
#pragma clang fp contract(off)
    constexpr bool MASK = std::is_same<ARGS, LetkfMaskedCols>::value || std::is_same<ARGS, LetkfAdaptiveMaskedCols>::value;
    constexpr bool ADAPT = std::is_same<ARGS, LetkfAdaptiveCols>::value || std::is_same<ARGS, LetkfAdaptiveMaskedCols>::value;
    const LetkfCols &a = letkf_cols(args);
    const int *const umap = letkf_umap(args);
    extern __shared__ __attribute__((aligned(16))) char letkf_smem[];
    double *const sm = reinterpret_cast<double *>(letkf_smem);
    const int E = MASK ? umap[0] : a.nmem, NM = MASK ? a.nmem : E, ep = (E + 1) & ~1, ee = ep * ep, kx = a.kx, ncol = a.ncol, tid = threadIdx.x;
    const int col = LIST ? a.cols[blockIdx.x] : blockIdx.x;
    const int *const um = MASK ? umap + 1 : nullptr, *const urank = MASK ? umap + LETKF_URANK : nullptr;
    int me0 = 0, me1 = 0;                     // MASK: the members of this thread's two elements of a staged tile of Y
    if constexpr (MASK) {
        if (E < 2) {                          // nothing to analyse: every member's increments are 0.0
            if constexpr (!LIST)
                for (int x = tid; x < (4 * kx + 1) * NM; x += LETKF_BLOCK) {
                    const int f = x / NM, m = x % NM, v = f < 4 * kx ? f / kx : 4, k = f < 4 * kx ? f % kx : 0;
                    a.dx[v][letkf_at(v, m, k, kx, ncol, col)] = 0.0;
                }
            return;
        }
        const int e0 = tid % ep, e1 = (tid + LETKF_BLOCK) % ep;
        me0 = e0 < E ? um[e0] : 0;
        me1 = e1 < E ? um[e1] : 0;
    }
    const double mdiag = MASK ? letkf_diag(args, E) : 0.0;      // unmasked: a.diag is read where it is used, as it always was
    const LetkfLds L(ep, kx, a.nlv);
    double *const C = sm + L.C, *const B = sm + L.B, *const ty = sm + L.ty, *const rtab = sm + L.rtab, *const td = sm + L.td,
                  *const lwh = sm + L.lwh;
    int *const lidx = reinterpret_cast<int *>(sm + L.lidx), *const misc = reinterpret_cast<int *>(sm + L.misc);
    int *const wcount = misc, *const flag = misc + 4, *const rot = misc + 8, *const touched = misc + 16;

    // A = (E - 1) / rho I (an odd E: one decoupled row more), b = 0
    for (int el = tid; el < kx * ee; el += LETKF_BLOCK) {
        const int i = (el % ee) / ep, j = el % ep;
        if constexpr (ADAPT)
            C[el] = i == j ? (i < E ? letkf_diag(args, E, el / ee, ncol, col) : 1.0) : 0.0;
        else
            C[el] = i == j ? (i < E ? (MASK ? mdiag : a.diag) : 1.0) : 0.0;
    }
    for (int el = tid; el < kx * ep; el += LETKF_BLOCK) B[el] = 0.0;
    if (tid < kx) touched[tid] = 0;
    const double cx = a.colunit[col], cy = a.colunit[ncol + col], cz = a.colunit[2 * ncol + col];
    __syncthreads();

    // ---- C and b of every level: the observations in ascending order, chunk by chunk
    for (int base = 0; base < a.nobs; base += LETKF_CHUNK) {
        const int o = base + tid;
        double wh = 0.0;
        if (o < a.nobs) {
            const double dx = cx - a.ounit[3 * (size_t)o], dy = cy - a.ounit[3 * (size_t)o + 1], dz = cz - a.ounit[3 * (size_t)o + 2];
            const double chord = sqrt((dx * dx + dy * dy) + dz * dz);
            const double dist = 2.0 * LETKF_REARTH * asin(fmin(1.0, 0.5 * chord));
            wh = letkf_gc(dist / a.ch);
        }
        // the chunk's observations in range, compacted in ascending order: ballot and prefix counts
        const bool keep = wh != 0.0;
        const unsigned long long mask = __ballot(keep);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int pos = __popcll(mask & ((1ull << lane) - 1ull)), nc = 0;
        for (int w = 0; w < LETKF_BLOCK / 64; ++w) {
            const int c = wcount[w];
            if (w < wave) pos += c;
            nc += c;
        }
        if (keep) { lidx[pos] = o; lwh[pos] = wh; }
        __syncthreads();
        for (int t0 = 0; t0 < nc; t0 += LETKF_TILE) {
            const int nt = min(LETKF_TILE, nc - t0);
            for (int x = tid; x < nt * kx; x += LETKF_BLOCK) {
                const int t = x / kx, k = x % kx, oo = lidx[t0 + t];
                double w = lwh[t0 + t];
                if (a.cv > 0.0) w = w * letkf_gc(fabs(a.lnfsg[k] - a.olns[oo]) / a.cv);
                rtab[k * LETKF_TILE + t] = w * a.rinv[oo];
            }
            for (int x = tid; x < nt * ep; x += LETKF_BLOCK) {
                const int t = x / ep, e = x % ep;
                if constexpr (MASK)       // LETKF_TILE * ep <= 2 LETKF_BLOCK: x is tid or tid + LETKF_BLOCK
                    ty[x] = e < E ? a.y[(size_t)lidx[t0 + t] * NM + (x < LETKF_BLOCK ? me0 : me1)] : 0.0;
                else
                    ty[x] = e < E ? a.y[(size_t)lidx[t0 + t] * E + e] : 0.0;
            }
            if (tid < nt) td[tid] = a.dep[lidx[t0 + tid]];
            __syncthreads();
            for (int el = tid; el < kx * ee; el += LETKF_BLOCK) {
                const int k = el / ee, i = (el % ee) / ep, j = el % ep;
                double acc = C[el];
                for (int t = 0; t < nt; ++t) {
                    const double r = rtab[k * LETKF_TILE + t];
                    if (r != 0.0) acc += r * (ty[t * ep + i] * ty[t * ep + j]);
                }
                C[el] = acc;
            }
            for (int el = tid; el < kx * ep; el += LETKF_BLOCK) {
                const int k = el / ep, i = el % ep;
                double acc = B[el];
                bool any = false;
                for (int t = 0; t < nt; ++t) {
                    const double r = rtab[k * LETKF_TILE + t];
                    if (r != 0.0) { acc += r * (ty[t * ep + i] * td[t]); any = true; }
                }
                B[el] = acc;
                if (any && i == 0) touched[k] = 1;      // tile after tile may: always the same value
            }
            __syncthreads();
        }
    }

    // ---- per level: A = V Lambda V^T by parallel cyclic Jacobi, T, the increments; nlv levels at a time, tpl threads each
    const int nlv = a.nlv, tpl = LETKF_BLOCK / nlv, lv = tid / tpl, lt = tid % tpl, half = ep / 2;
    double *const V = sm + L.V + lv * ee, *const S = sm + L.S + lv * 6 * ep, *const X = sm + L.X + lv * LETKF_VARS * ep;
    double *const lam = S, *const hh = S + ep, *const gf = S + 2 * ep, *const wbar = S + 3 * ep, *const cs = S + 4 * ep;
    int *const pq = reinterpret_cast<int *>(S + 5 * ep);
    // the two phases' work without a division: rows as (pair, column) with 32 lanes per pair, columns as (row, pair) with 16
    // lanes per row -- neighbouring lanes then touch neighbouring words of one row of A, not one word of neighbouring rows
    const int rj = lt & 31, rm = lt >> 5, rstep = tpl >> 5, cm = lt & 15, ci = lt >> 4, cstep = tpl >> 4;
    for (int k0 = 0; k0 < kx; k0 += nlv) {
        const int k = k0 + lv;
        const bool act = k < kx;
        double *const A = C + (act ? k : 0) * ee;
        const double *const Bk = B + (act ? k : 0) * ep;
        if (act)
            for (int el = lt; el < ee; el += tpl) V[el] = el / ep == el % ep ? 1.0 : 0.0;
        if (lt == 0) flag[lv] = act && touched[k];      // a level no observation reaches is diagonal already
        __syncthreads();
        for (int sweep = 0; sweep < LETKF_SWEEPS; ++sweep) {
            bool any = false;
            for (int l = 0; l < nlv; ++l) any = any || flag[l];
            if (!any) break;                            // the same for every thread
            const bool go = flag[lv] != 0;
            if (lt == 0) rot[lv] = 0;
            __syncthreads();
            for (int r = 0; r < ep - 1; ++r) {
                if (go && lt < half) {
                    int p, q;
                    letkf_pair(lt, r, ep, p, q);
                    const double app = A[p * ep + p], aqq = A[q * ep + q], apq = A[p * ep + q];
                    double c = 1.0, s = 0.0;
                    if (!(fabs(apq) <= LETKF_TOL * sqrt(app * aqq))) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        rot[lv] = 1;                    // several lanes may: all write the same value
                    }
                    cs[2 * lt] = c; cs[2 * lt + 1] = s;
                    pq[2 * lt] = p; pq[2 * lt + 1] = q;
                }
                __syncthreads();
                if (go && rj < ep)                      // rows: A <- J^T A
                    for (int m = rm; m < half; m += rstep) {
                        const int p = pq[2 * m], q = pq[2 * m + 1];
                        const double c = cs[2 * m], s = cs[2 * m + 1], x = A[p * ep + rj], y = A[q * ep + rj];
                        A[p * ep + rj] = c * x - s * y;
                        A[q * ep + rj] = s * x + c * y;
                    }
                __syncthreads();
                if (go && cm < half) {                  // columns: A <- A J, V <- V J; the rotated pair's element is zero
                    const int p = pq[2 * cm], q = pq[2 * cm + 1];
                    const double c = cs[2 * cm], s = cs[2 * cm + 1];
                    for (int i = ci; i < ep; i += cstep) {
                        double x = A[i * ep + p], y = A[i * ep + q];
                        double xn = c * x - s * y, yn = s * x + c * y;
                        if (s != 0.0 && i == p) yn = 0.0;
                        if (s != 0.0 && i == q) xn = 0.0;
                        A[i * ep + p] = xn; A[i * ep + q] = yn;
                        x = V[i * ep + p]; y = V[i * ep + q];
                        V[i * ep + p] = c * x - s * y;
                        V[i * ep + q] = s * x + c * y;
                    }
                }
                __syncthreads();
            }
            if (lt == 0 && go) flag[lv] = rot[lv];      // no pair rotated: converged
            __syncthreads();
        }
        // T = V diag(sqrt((E-1)/lambda)) V^T + wbar 1^T - I with wbar = V Lambda^-1 V^T b, into the place of A
        if (act && lt < ep) lam[lt] = A[lt * ep + lt];
        __syncthreads();
        if (act && lt < ep) {
            double vtb = 0.0;
            for (int g = 0; g < ep; ++g) vtb += V[g * ep + lt] * Bk[g];
            hh[lt] = vtb / lam[lt];
            gf[lt] = sqrt((double)(E - 1) / lam[lt]);
        }
        __syncthreads();
        if (act && lt < ep) {
            double w = 0.0;
            for (int i = 0; i < ep; ++i) w += V[lt * ep + i] * hh[i];
            wbar[lt] = w;
        }
        __syncthreads();
        if (act)
            for (int el = lt; el < ee; el += tpl) {
                const int f = el / ep, e = el % ep;
                double acc = 0.0;
                int i = e;                              // the sum starts at i = e: the lanes' rows of V on different banks
                for (int n = 0; n < ep; ++n) {
                    acc += (V[f * ep + i] * gf[i]) * V[e * ep + i];
                    i = i + 1 == ep ? 0 : i + 1;
                }
                const double tfe = (acc + wbar[f]) - (f == e ? 1.0 : 0.0);
                if constexpr (LIST) {
                    if (f < E && e < E) a.tw[(((size_t)blockIdx.x * kx + k) * NM + f) * NM + e] = tfe;
                } else {
                    A[el] = tfe;
                }
            }
        if constexpr (LIST) {
            __syncthreads();
            continue;
        }
        // the increments of u, v, t, q at this level, of ps at the lowest: dx_e = sum_f (x_f - mean) T[f][e]
        const int nvar = act ? (k == kx - 1 ? LETKF_VARS : LETKF_VARS - 1) : 0;
        for (int x = lt; x < nvar * ep; x += tpl) {
            const int v = x / ep, e = x % ep;
            if constexpr (MASK)
                X[x] = e < E ? a.x[v][letkf_at(v, um[e], k, kx, ncol, col)] : 0.0;
            else
                X[x] = e < E ? a.x[v][letkf_at(v, e, k, kx, ncol, col)] : 0.0;
        }
        __syncthreads();
        for (int x = lt; x < nvar * ep; x += tpl) {
            const int v = x / ep, e = x % ep;
            if (e >= E) continue;
            const double *const xv = X + v * ep;
            double sum = 0.0;
            for (int f = 0; f < E; ++f) sum += xv[f];
            const double mean = sum / E;
            double d = 0.0;
            for (int f = 0; f < E; ++f) d += (xv[f] - mean) * A[f * ep + e];
            a.dx[v][letkf_at(v, MASK ? um[e] : e, k, kx, ncol, col)] = d;
        }
        if constexpr (MASK)                    // a member not in use: nobody reads its values, its increments are exactly 0.0
            for (int x = lt; x < nvar * NM; x += tpl) {
                const int v = x / NM, m = x % NM;
                if (urank[m] < 0) a.dx[v][letkf_at(v, m, k, kx, ncol, col)] = 0.0;
            }
        __syncthreads();
    }
}

// Weight interpolation: the increments of every grid column from the transforms of the coarse columns.  An item is one (level, grid
// column), the column fastest; it has lpi lanes (E rounded up to a power of two), lane e forms member e's increments, so a
// workgroup holds 256 / lpi items of neighbouring columns, which mostly share their stencil's coarse columns (L1, L2).  Per f the
// lanes of an item read a row of T of each stencil entry, contiguous along e; the members' values go through LDS (five doubles per
// thread, 10 KB per workgroup whatever E), loaded and stored with the column fastest over the lanes.  A streaming kernel: no
// atomics, every bound a kernel argument, the sums in the order of letkf_transform_kernel's step 4.
// MASK (the member mask, umap): the launch shape, the LDS slots and the strides of T are those of nmem.  Lane e still owns member
// e: a member in use has the compact index c = rank[e] and forms dx from the leading n x n block of each T and the values of the
// members umap[1 + f], f < n ascending, with the means over them; a member not in use reads nothing and gets 0.0, and so does
// every member when n < 2 (the weight buffer is then not read at all).  One body, two instantiations, no run-time branch.
template <bool MASK>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_apply_kernel(const LetkfApply a, const int lpi, const int *const umap)
{
#pragma clang fp contract(off)
    __shared__ double X[LETKF_VARS * LETKF_BLOCK];      // [slot][v][lpi]
    const int NM = a.nmem, E = MASK ? umap[0] : NM, kx = a.kx, ncol = a.ncol, tid = threadIdx.x, ipb = LETKF_BLOCK / lpi;
    const int *const um = MASK ? umap + 1 : nullptr;
    const long nitem = (long)kx * ncol, first = (long)blockIdx.x * ipb;
    {   // the members' values: thread -> (member, slot), the slots' columns contiguous
        const int slot = tid % ipb, f = tid / ipb;
        const long item = first + slot;
        if (item < nitem && f < NM) {
            const int k = (int)(item / ncol), col = (int)(item % ncol), nvar = k == kx - 1 ? LETKF_VARS : LETKF_VARS - 1;
            for (int v = 0; v < nvar; ++v) X[(slot * LETKF_VARS + v) * lpi + f] = a.x[v][letkf_at(v, f, k, kx, ncol, col)];
        }
    }
    __syncthreads();
    const int slot = tid / lpi, e = tid % lpi;
    const long item = first + slot;
    const int c = e < NM ? (MASK ? umap[LETKF_URANK + e] : e) : -1;
    double d[LETKF_VARS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (item < nitem && c >= 0 && (!MASK || E >= 2)) {
        const int k = (int)(item / ncol), col = (int)(item % ncol);
        const bool sfc = k == kx - 1;
        const double *const xs = X + slot * LETKF_VARS * lpi;
        double mean[LETKF_VARS];
        for (int v = 0; v < LETKF_VARS; ++v) {
            double sum = 0.0;
            for (int f = 0; f < E; ++f) sum += xs[v * lpi + (MASK ? um[f] : f)];
            mean[v] = sum / E;
        }
        const double w0 = a.iwgt[4 * (size_t)col], w1 = a.iwgt[4 * (size_t)col + 1], w2 = a.iwgt[4 * (size_t)col + 2],
                     w3 = a.iwgt[4 * (size_t)col + 3];
        const size_t ee = (size_t)NM * NM, lev = (size_t)k * ee + c;
        const double *const t0 = a.tw + (size_t)a.iidx[4 * (size_t)col] * kx * ee + lev,
                     *const t1 = a.tw + (size_t)a.iidx[4 * (size_t)col + 1] * kx * ee + lev,
                     *const t2 = a.tw + (size_t)a.iidx[4 * (size_t)col + 2] * kx * ee + lev,
                     *const t3 = a.tw + (size_t)a.iidx[4 * (size_t)col + 3] * kx * ee + lev;
#pragma unroll 4
        for (int f = 0; f < E; ++f) {
            const size_t r = (size_t)f * NM;
            const int mf = MASK ? um[f] : f;
            double t = w0 * t0[r];            // (1 - a)(1 - b) with a, b < 1: the first term is always present
            if (w1 != 0.0) t += w1 * t1[r];
            if (w2 != 0.0) t += w2 * t2[r];
            if (w3 != 0.0) t += w3 * t3[r];
            for (int v = 0; v < LETKF_VARS - 1; ++v) d[v] += (xs[v * lpi + mf] - mean[v]) * t;
            if (sfc) d[4] += (xs[4 * lpi + mf] - mean[4]) * t;
        }
    }
    __syncthreads();
    X[(slot * LETKF_VARS + 0) * lpi + e] = d[0];
    X[(slot * LETKF_VARS + 1) * lpi + e] = d[1];
    X[(slot * LETKF_VARS + 2) * lpi + e] = d[2];
    X[(slot * LETKF_VARS + 3) * lpi + e] = d[3];
    X[(slot * LETKF_VARS + 4) * lpi + e] = d[4];
    __syncthreads();
    {
        const int slot2 = tid % ipb, f = tid / ipb;
        const long item2 = first + slot2;
        if (item2 < nitem && f < NM) {
            const int k = (int)(item2 / ncol), col = (int)(item2 % ncol), nvar = k == kx - 1 ? LETKF_VARS : LETKF_VARS - 1;
            for (int v = 0; v < nvar; ++v) a.dx[v][letkf_at(v, f, k, kx, ncol, col)] = X[(slot2 * LETKF_VARS + v) * lpi + f];
        }
    }
}

__global__ __launch_bounds__(LETKF_BLOCK) void spec_add_kernel(const LetkfAdd a)
{
    const int op = blockIdx.y;
    const long i = (long)blockIdx.x * LETKF_BLOCK + threadIdx.x;
    if (i >= a.n[op]) return;
    const double d = a.src[op][i];
    if (d != 0.0) a.dst[op][i] = a.dst[op][i] + d;
}

// Relaxation of the raw increments (include/spdy.h, "relaxation"): one lane per grid item, blockIdx.y the item's
// field (variable and level, u | v | t | q | ps), the columns across the lanes, so every member's load is coalesced.  The members'
// values stay in registers under their compact index c < n: every loop over them is unrolled to LETKF_MAX_MEMBERS and leaves at
// c == n, which is the same for the whole launch, so no register index is a run-time one, nothing goes to scratch and no
// predicate has to be kept (a bit per member, tested in every loop, cost 52 spilled SGPRs).  All of an item's x and raw values are
// loaded before the first sum and long before the first store: dx may be x.  MASK (the member mask, a.umap): n and the member of
// each compact index come from the table instead of nmem; a member not in use is not read and gets 0.0, and so does every member
// when n < 2.  One body, two instantiations.  No atomics, the sums in ascending member order.
template <bool MASK>
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_relax_kernel(const LetkfRelax a)
{
#pragma clang fp contract(off)
    const int col = blockIdx.x * LETKF_BLOCK + threadIdx.x;
    if (col >= a.ncol) return;
    const int item = blockIdx.y, kx = a.kx, ncol = a.ncol, E = a.nmem;
    const int v = item < 4 * kx ? item / kx : 4, k = item - v * kx;
    // the variable's fields by selects, as letkf_pobs_kernel does it
    const double *const xv = v == 0 ? a.x[0] : v == 1 ? a.x[1] : v == 2 ? a.x[2] : v == 3 ? a.x[3] : a.x[4];
    const double *const rv = v == 0 ? a.raw[0] : v == 1 ? a.raw[1] : v == 2 ? a.raw[2] : v == 3 ? a.raw[3] : a.raw[4];
    double *const dv = v == 0 ? a.dx[0] : v == 1 ? a.dx[1] : v == 2 ? a.dx[2] : v == 3 ? a.dx[3] : a.dx[4];
    const size_t at = letkf_at(v, 0, k, kx, ncol, col), step = (size_t)(v < 4 ? kx : 1) * ncol;
    const int n = MASK ? a.umap[0] : E;
    if constexpr (MASK) {
        if (n < 2) {
            for (int e = 0; e < E; ++e) dv[at + e * step] = 0.0;
            a.inflation[(size_t)item * ncol + col] = 1.0;
            return;
        }
    }
    // compact index c stands for member m: c itself without a mask, umap[1 + c] with one; both ascending.  Without a mask the
    // lane's own offset walks the members: 32 scalar offsets held from the loads to the stores would not fit the SGPRs
    double x[LETKF_MAX_MEMBERS], d[LETKF_MAX_MEMBERS];
    size_t walk = at;
#pragma unroll
    for (int c = 0; c < LETKF_MAX_MEMBERS; ++c) {
        x[c] = d[c] = 0.0;
        if (c < n) {
            const size_t off = MASK ? at + a.umap[1 + c] * step : walk;
            x[c] = xv[off];
            d[c] = rv[off];
        }
        walk += step;
    }
    double sx = 0.0, sd = 0.0;
#pragma unroll
    for (int c = 0; c < LETKF_MAX_MEMBERS; ++c)
        if (c < n) {
            sx += x[c];
            sd += d[c];
        }
    const double xm = sx / n, dm = sd / n;
    double sb2 = 0.0, sa2 = 0.0;
#pragma unroll
    for (int c = 0; c < LETKF_MAX_MEMBERS; ++c)
        if (c < n) {
            const double b = x[c] - xm, p = b + a.omr * (d[c] - dm);
            sb2 += b * b;
            sa2 += p * p;
            x[c] = b;
            d[c] = p;
        }
    const double sb = sqrt(sb2 / (n - 1)), sa = sqrt(sa2 / (n - 1));
    const double f = sa > 0.0 ? 1.0 + a.rtps * (sb - sa) / sa : 1.0;
    walk = at;
#pragma unroll
    for (int c = 0; c < LETKF_MAX_MEMBERS; ++c) {
        if (c < n) dv[MASK ? at + a.umap[1 + c] * step : walk] = dm + (f * d[c] - x[c]);
        walk += step;
    }
    if constexpr (MASK) {
        // the members not in use keep the 0.0 the analysis wrote for them
        for (int e = 0; e < E; ++e)
            if (a.umap[LETKF_URANK + e] < 0) dv[at + e * step] = 0.0;
    }
    a.inflation[(size_t)item * ncol + col] = f;
}

// The background check and the observation-space statistics (include/spdy.h, "background check and observation statistics";
// DESIGN.md s27), between the observation stage and the transform.  Workgroup g owns group g: its QC_BLOCK = 1024 threads walk the
// network in chunks of QC_BLOCK, thread t looks at observation base + t and takes it if it is of group g, so thread t holds the
// partial sums of the group's observations o = t (mod QC_BLOCK), o ascending; then a halving tree in LDS, s[t] = s[t] + s[t + h]
// for h = 512, 256, ..., 1, five of the ten numbers at a time.  (With 256 threads the walk of 13 728 observations was a chain of 54
// dependent steps per thread, 87 us at E = 4; the sums' order is part of the definition, so the block size is too.)  An observation
// is of one group only: what is written per observation has one writer.  DECIDE: an analysis call -- the test is made (g2 > 0,
// n >= 2), used, reff and the check's record are written, and the departure is kept.  Otherwise the stats-only call: the record and
// the kept departure of the latest checked analysis are read and nothing is decided; used and reff are given back what that
// analysis left (the observation stage of an at-pressure network has just overwritten them).  MASK (the member mask, a.umap): n
// and the members of the spread's sum are the mask's, by a select.  One body, four instantiations, no run-time branch on either.
// No atomics; every bound a kernel argument or a constant.
constexpr int QC_BLOCK = 1024, QC_PASS = QC_STATS / 2;

template <bool MASK, bool DECIDE>
__global__ __launch_bounds__(QC_BLOCK) void letkf_qc_kernel(const LetkfQc a)
{
#pragma clang fp contract(off)
    __shared__ double part[QC_PASS][QC_BLOCK];
    const int g = blockIdx.x, tid = threadIdx.x, E = a.nmem, n = MASK ? a.umap[0] : E;
    const double nm1 = (double)(n - 1);
    const bool test = DECIDE && a.g2 > 0.0 && n >= 2;
    double acc[QC_STATS];
#pragma unroll
    for (int i = 0; i < QC_STATS; ++i) acc[i] = 0.0;
    // the group of the next chunk's observation is asked for before this chunk's is worked on, and everything an observation
    // needs is loaded before the first store: the walk is a chain of one memory latency per chunk, not of three
    const int *const gid = a.group ? a.group : a.var;
    int mine = tid < a.nobs ? gid[tid] : -1;
    for (int base = 0; base < a.nobs; base += QC_BLOCK) {
        const int o = base + tid, onext = o + QC_BLOCK, here = mine;
        mine = onext < a.nobs ? gid[onext] : -1;
        if (here != g) continue;
        const double *const y = a.y + (size_t)o * E;
        const double err = a.err[o], dep = a.dep[o], rinv = a.rinv[o];
        const double kept0 = DECIDE ? (a.incol ? a.incol[o] : 1.0) : a.check[o], kept1 = DECIDE ? 0.0 : a.depb[o];
        double ss = 0.0;
        for (int e = 0; e < E; ++e) {
            const bool u = !MASK || a.umap[LETKF_URANK + e] >= 0;
            const double ye = y[e];
            ss = u ? ss + ye * ye : ss;
        }
        const double s2 = ss / nm1, e2 = err * err;
        double code, depb;
        if constexpr (DECIDE) {
            const bool incol = kept0 != 0.0;
            const bool rej = test && dep * dep > a.g2 * (s2 + e2);
            code = !incol ? 2.0 : rej ? 1.0 : 0.0;
            depb = dep;
            a.check[o] = code;
            a.depb[o] = dep;
        } else {
            code = kept0;
            depb = kept1;
        }
        const bool used = code == 0.0;
        a.used[o] = used ? 1.0 : 0.0;
        a.reff[o] = used ? rinv : 0.0;
        acc[0] += 1.0;
        acc[1] = code == 2.0 ? acc[1] + 1.0 : acc[1];
        acc[2] = code == 1.0 ? acc[2] + 1.0 : acc[2];
        if (used) {
            acc[3] += 1.0;
            acc[4] += dep;
            acc[5] += dep * dep;
            acc[6] += s2;
            acc[7] += e2;
            acc[8] += dep * depb;
            acc[9] += depb;
        }
    }
#pragma unroll
    for (int pass = 0; pass < QC_STATS / QC_PASS; ++pass) {
#pragma unroll
        for (int i = 0; i < QC_PASS; ++i) part[i][tid] = acc[pass * QC_PASS + i];
        __syncthreads();
        for (int h = QC_BLOCK / 2; h >= 1; h >>= 1) {
            if (tid < h) {
#pragma unroll
                for (int i = 0; i < QC_PASS; ++i) part[i][tid] = part[i][tid] + part[i][tid + h];
            }
            __syncthreads();
        }
        if (tid < QC_PASS) a.stats[(size_t)g * QC_STATS + pass * QC_PASS + tid] = part[tid][0];
        __syncthreads();
    }
}

// Adaptive inflation (include/spdy.h, "adaptive inflation"), the estimate's two launches.  The first: s2 of every
// observation, one thread each, the members ascending; y of a member not in use is 0.0 and adds an exact zero, so there is no
// mask form: only n is the mask's.  n < 2: nothing is written.
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_infl_obs_kernel(const LetkfInfl a)
{
#pragma clang fp contract(off)
    const int o = blockIdx.x * LETKF_BLOCK + threadIdx.x, E = a.nmem, n = a.umap ? a.umap[0] : E;
    if (o >= a.nobs || n < 2) return;
    const double *const y = a.y + (size_t)o * E;
    double ss = 0.0;
    for (int e = 0; e < E; ++e) {
        const double ye = y[e];
        ss += ye * ye;
    }
    a.s2[o] = ss / (double)(n - 1);
}

// The second: one workgroup per grid column, at every column whatever the weight stride.  The scan is the transform kernel's, with
// its expressions: chunks of LETKF_CHUNK, the horizontal weight, ballot and prefix compaction in ascending order; the thread that
// keeps an observation stages what the sums need of it in LDS.  Lane k < kx then carries p1, p2, p3 of level k in registers over
// the chunk's compacted observations, ascending, and after the last chunk updates rho[k][col] in place and stores the sums.  No
// atomics; every loop bound a kernel argument or a constant; 10 KB of static LDS.
__global__ __launch_bounds__(LETKF_BLOCK) void letkf_infl_kernel(const LetkfInfl a)
{
#pragma clang fp contract(off)
    __shared__ double lwh[LETKF_CHUNK], lolns[LETKF_CHUNK], lreff[LETKF_CHUNK], ld2[LETKF_CHUNK], ls2[LETKF_CHUNK];
    __shared__ int wcount[LETKF_BLOCK / 64];
    const int n = a.umap ? a.umap[0] : a.nmem;
    if (n < 2) return;                            // the same for every thread of the launch
    const int tid = threadIdx.x, col = blockIdx.x, kx = a.kx, ncol = a.ncol;
    const double cx = a.colunit[col], cy = a.colunit[ncol + col], cz = a.colunit[2 * ncol + col];
    const double lnk = tid < kx ? a.lnfsg[tid] : 0.0;
    double p1 = 0.0, p2 = 0.0, p3 = 0.0;
    for (int base = 0; base < a.nobs; base += LETKF_CHUNK) {
        const int o = base + tid;
        double wh = 0.0;
        if (o < a.nobs) {
            const double dx = cx - a.ounit[3 * (size_t)o], dy = cy - a.ounit[3 * (size_t)o + 1], dz = cz - a.ounit[3 * (size_t)o + 2];
            const double chord = sqrt((dx * dx + dy * dy) + dz * dz);
            const double dist = 2.0 * LETKF_REARTH * asin(fmin(1.0, 0.5 * chord));
            wh = letkf_gc(dist / a.ch);
        }
        const bool keep = wh != 0.0;
        const unsigned long long mask = __ballot(keep);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int pos = __popcll(mask & ((1ull << lane) - 1ull)), nc = 0;
        for (int w = 0; w < LETKF_BLOCK / 64; ++w) {
            const int c = wcount[w];
            if (w < wave) pos += c;
            nc += c;
        }
        if (keep) {
            const double dep = a.dep[o];
            lwh[pos] = wh; lolns[pos] = a.olns[o]; lreff[pos] = a.reff[o]; ld2[pos] = dep * dep; ls2[pos] = a.s2[o];
        }
        __syncthreads();
        if (tid < kx)
            for (int t = 0; t < nc; ++t) {
                double w = lwh[t];
                if (a.cv > 0.0) w = w * letkf_gc(fabs(lnk - lolns[t]) / a.cv);
                const double r = w * lreff[t];
                if (r != 0.0) {
                    p1 += r * ld2[t];
                    p2 += r * ls2[t];
                    p3 += w;
                }
            }
        __syncthreads();
    }
    if (tid >= kx) return;
    const size_t at = (size_t)tid * ncol + col, plane = (size_t)kx * ncol;
    const double rho = a.rho[at];
    double out = rho;
    if (p3 > 0.0 && p2 > 0.0) {
        const double ro = (p1 - p3) / p2;
        const double t = (rho * p2 + p3) / p2;
        const double vo = (2.0 / p3) * (t * t);
        const double g = a.vb / (vo + a.vb);
        const double est = rho + g * (ro - rho);
        // fmin and fmax drop a NaN, so the estimate is tested before the bounds: a non-finite one leaves rho as it is
        if (__builtin_isfinite(est)) out =fmin(fmax(est, a.rho_min), a.rho_max);
    }
    a.rho[at] = out;
    a.parm[at] = p1;
    a.parm[plane + at] = p2;
    a.parm[2 * plane + at] = p3;
}

}  // namespace

size_t letkf_lds_bytes(int nmem, int kx, int nlv) { return sizeof(double) * (size_t)LetkfLds((nmem + 1) & ~1, kx, nlv).total; }

namespace {
// The transform kernel's eight instantiations, named here and nowhere else: [adaptive][masked][list].  launch_letkf_transform picks
// from the table and letkf_prepare walks it, so no form can be launched without its LDS attribute.
#define SPDY_TRANSFORM_FORMS(ARGS)                                                                                     \
    {reinterpret_cast<const void *>(letkf_transform_kernel<false, ARGS>), reinterpret_cast<const void *>(letkf_transform_kernel<true, ARGS>)}
const void *const transform_forms[2][2][2] = {{SPDY_TRANSFORM_FORMS(LetkfCols), SPDY_TRANSFORM_FORMS(LetkfMaskedCols)},
                                              {SPDY_TRANSFORM_FORMS(LetkfAdaptiveCols), SPDY_TRANSFORM_FORMS(LetkfAdaptiveMaskedCols)}};
#undef SPDY_TRANSFORM_FORMS
}  // namespace

// the whole LDS of a compute unit, whatever this object needs: objects of other sizes launch the same kernel
hipError_t letkf_prepare(size_t lds)
{
    constexpr size_t whole = 160 * 1024;
    if (lds > whole) return hipErrorInvalidValue;
    for (const auto &adaptive : transform_forms)
        for (const auto &masked : adaptive)
            for (const void *f : masked)
                if (const hipError_t rc = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)whole)) return rc;
    return hipSuccess;
}

hipError_t launch_letkf_mask(const int *use, int nmem, int *umap, double *nused, hipStream_t s)
{
    if (!use || nmem < 2 || nmem > LETKF_MAX_MEMBERS || !umap || !nused) return hipErrorInvalidValue;
    hipLaunchKernelGGL(letkf_mask_kernel, dim3(1), dim3(64), 0, s, use, nmem, umap, nused);
    return hipGetLastError();
}

namespace {
// The checks of the three launches of the observation stage.  observes: the launch forms hx from the ensemble; couples: it forms
// what couples members; a launch that does one of the two keeps, or reads, the slots' rows.  *empty: nothing to launch.
hipError_t observe_ready(const LetkfObserve &a, bool observes, bool couples, bool *empty)
{
    if (a.first < 0 || a.last < a.first || a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || !a.hx) return hipErrorInvalidValue;
    if (observes) {
        if (a.kx < 1 || a.kx > LETKF_MAX_KX || a.ncol < 1) return hipErrorInvalidValue;
        for (int v = 0; v < LETKF_VARS; ++v)
            if (!a.x[v]) return hipErrorInvalidValue;
        if (a.atp && (a.kx < 2 || a.kx > VINTERP_KMAX || a.lv.kx != a.kx)) return hipErrorInvalidValue;
    }
    if (couples && (!a.hxmean || !a.y || !a.dep)) return hipErrorInvalidValue;
    if (a.atp) {
        if (!a.lnp || (couples && (!a.rinv || !a.olns || !a.used || !a.reff))) return hipErrorInvalidValue;
        if (observes != couples && (!a.slot_ps || !a.slot_out)) return hipErrorInvalidValue;
    }
    *empty = a.last == a.first;
    if (*empty) return hipSuccess;
    if (observes && (!a.var || !a.lev || !a.sidx || !a.swgt)) return hipErrorInvalidValue;
    if (couples && !a.value) return hipErrorInvalidValue;
    return hipSuccess;
}
}  // namespace

hipError_t launch_letkf_observe(const LetkfObserve &a, hipStream_t s)
{
    bool empty = false;
    if (const hipError_t rc = observe_ready(a, true, true, &empty)) return rc;
    if (empty) return hipSuccess;
    const int n = a.last - a.first, opb = LETKF_BLOCK / a.nmem;
    const dim3 each((n + LETKF_BLOCK - 1) / LETKF_BLOCK), whole((n + opb - 1) / opb), block(LETKF_BLOCK);
    if (a.atp) {
        if (a.umap) hipLaunchKernelGGL(letkf_pobs_kernel<true>, whole, block, 0, s, a);
        else hipLaunchKernelGGL(letkf_pobs_kernel<false>, whole, block, 0, s, a);
    } else {
        if (a.umap) hipLaunchKernelGGL(letkf_obs_kernel<true>, each, block, 0, s, a);
        else hipLaunchKernelGGL(letkf_obs_kernel<false>, each, block, 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_letkf_slot_obs(const LetkfObserve &a, hipStream_t s)
{
    bool empty = false;
    if (const hipError_t rc = observe_ready(a, true, false, &empty)) return rc;
    if (empty) return hipSuccess;
    const int opb = LETKF_BLOCK / a.nmem, n = a.last - a.first;
    if (a.atp)
        hipLaunchKernelGGL(letkf_slot_obs_kernel<true>, dim3((n + opb - 1) / opb), dim3(LETKF_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(letkf_slot_obs_kernel<false>, dim3((n + opb - 1) / opb), dim3(LETKF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_letkf_slot_finish(const LetkfObserve &a, hipStream_t s)
{
    bool empty = false;
    if (const hipError_t rc = observe_ready(a, false, true, &empty)) return rc;
    if (empty) return hipSuccess;
    const dim3 grid((a.last - a.first + LETKF_BLOCK - 1) / LETKF_BLOCK), block(LETKF_BLOCK);
    if (a.umap) {
        if (a.atp) hipLaunchKernelGGL((letkf_slot_finish_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((letkf_slot_finish_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (a.atp) hipLaunchKernelGGL((letkf_slot_finish_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((letkf_slot_finish_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

namespace {
// the checks of a transform launch, masked or not; *list: the column-list form
hipError_t transform_ready(const LetkfCols &a, size_t lds, bool *list)
{
    if (a.nobs < 0 || a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.kx < 1 || a.kx > LETKF_MAX_KX || a.ncol < 1 ||
        (a.nlv != 1 && a.nlv != 2 && a.nlv != 4) || lds != letkf_lds_bytes(a.nmem, a.kx, a.nlv) || !(a.ch > 0.0) || !(a.diag > 0.0) ||
        !a.colunit || !a.lnfsg)
        return hipErrorInvalidValue;
    if (a.nobs && (!a.ounit || !a.olns || !a.rinv || !a.y || !a.dep)) return hipErrorInvalidValue;
    *list = a.cols || a.tw || a.nlist;
    if (*list) return !a.cols || !a.tw || a.nlist < 1 || a.nlist > a.ncol ? hipErrorInvalidValue : hipSuccess;
    for (int v = 0; v < LETKF_VARS; ++v)
        if (!a.x[v] || !a.dx[v]) return hipErrorInvalidValue;
    return hipSuccess;
}
}  // namespace

// One launch of the form the route names: field: adaptive inflation's, or NULL and the scalar rho holds (c.diag has it; the masked
// form reads rho itself); umap: the member mask's table, or NULL.  Each form gets the argument struct it is instantiated on.
hipError_t launch_letkf_transform(const LetkfCols &c, double rho, const double *field, const int *umap, size_t lds, hipStream_t s)
{
    bool list = false;
    if (!field && umap && !(rho > 0.0)) return hipErrorInvalidValue;
    if (const hipError_t rc = transform_ready(c, lds, &list)) return rc;
    const LetkfMaskedCols m{c, rho, umap};
    const LetkfAdaptiveCols a{c, field};
    const LetkfAdaptiveMaskedCols am{c, field, umap};
    const void *const arg[2][2] = {{&c, &m}, {&a, &am}};
    void *args[1] = {const_cast<void *>(arg[field != nullptr][umap != nullptr])};
    (void)hipLaunchKernel(transform_forms[field != nullptr][umap != nullptr][list], dim3(list ? c.nlist : c.ncol), dim3(LETKF_BLOCK), args, lds, s);
    return hipGetLastError();
}

// both launches of the estimate; an empty network still gets both (the first with one idle workgroup): the node count is fixed
hipError_t launch_letkf_infl(const LetkfInfl &a, hipStream_t s)
{
    if (a.nobs < 0 || a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.kx < 1 || a.kx > LETKF_MAX_KX || a.ncol < 1 || !(a.ch > 0.0) ||
        !(a.vb >= 0.0) || !(a.rho_min > 0.0) || !(a.rho_max >= a.rho_min) || !a.colunit || !a.lnfsg || !a.s2 || !a.rho || !a.parm)
        return hipErrorInvalidValue;
    if (a.nobs && (!a.ounit || !a.olns || !a.reff || !a.y || !a.dep)) return hipErrorInvalidValue;
    const int nb = a.nobs ? (a.nobs + LETKF_BLOCK - 1) / LETKF_BLOCK : 1;
    hipLaunchKernelGGL(letkf_infl_obs_kernel, dim3(nb), dim3(LETKF_BLOCK), 0, s, a);
    if (const hipError_t rc = hipGetLastError()) return rc;
    hipLaunchKernelGGL(letkf_infl_kernel, dim3(a.ncol), dim3(LETKF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_letkf_apply(const LetkfApply &a, hipStream_t s, const int *umap)
{
    if (a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.kx < 1 || a.kx > LETKF_MAX_KX || a.ncol < 1 || a.nlist < 1 || a.nlist > a.ncol ||
        !a.iidx || !a.iwgt || !a.tw)
        return hipErrorInvalidValue;
    for (int v = 0; v < LETKF_VARS; ++v)
        if (!a.x[v] || !a.dx[v]) return hipErrorInvalidValue;
    int lpi = 2;
    while (lpi < a.nmem) lpi *= 2;
    const long nitem = (long)a.kx * a.ncol, ipb = LETKF_BLOCK / lpi;
    const dim3 grid((unsigned)((nitem + ipb - 1) / ipb)), block(LETKF_BLOCK);
    if (umap)
        hipLaunchKernelGGL(letkf_apply_kernel<true>, grid, block, 0, s, a, lpi, umap);
    else
        hipLaunchKernelGGL(letkf_apply_kernel<false>, grid, block, 0, s, a, lpi, umap);
    return hipGetLastError();
}

hipError_t launch_spec_add(const LetkfAdd &a, hipStream_t s)
{
    if (a.nops < 1 || a.nops > LETKF_VARS) return hipErrorInvalidValue;
    long most = 0;
    for (int i = 0; i < a.nops; ++i) {
        if (a.n[i] < 0 || !a.dst[i] || !a.src[i]) return hipErrorInvalidValue;
        most = a.n[i] > most ? a.n[i] : most;
    }
    if (!most) return hipSuccess;
    hipLaunchKernelGGL(spec_add_kernel, dim3((unsigned)((most + LETKF_BLOCK - 1) / LETKF_BLOCK), a.nops), dim3(LETKF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_letkf_relax(const LetkfRelax &a, hipStream_t s)
{
    if (a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.kx < 1 || a.kx > LETKF_MAX_KX || a.ncol < 1 || !a.inflation || !(a.omr >= 0.0) ||
        !(a.omr <= 1.0) || !(a.rtps >= 0.0) || !(a.rtps <= 1.0))
        return hipErrorInvalidValue;
    for (int v = 0; v < LETKF_VARS; ++v)
        if (!a.x[v] || !a.raw[v] || !a.dx[v]) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.ncol + LETKF_BLOCK - 1) / LETKF_BLOCK), (unsigned)(4 * a.kx + 1));
    if (a.umap)
        hipLaunchKernelGGL(letkf_relax_kernel<true>, grid, dim3(LETKF_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(letkf_relax_kernel<false>, grid, dim3(LETKF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_letkf_qc(const LetkfQc &a, bool decide, hipStream_t s)
{
    if (a.nobs < 0 || a.nmem < 2 || a.nmem > LETKF_MAX_MEMBERS || a.ngroups < 1 || a.ngroups > QC_MAX_GROUPS || !(a.g2 >= 0.0) ||
        !a.stats || !a.check || !a.depb)
        return hipErrorInvalidValue;
    if (a.nobs && (!a.var || !a.y || !a.dep || !a.err || !a.rinv || !a.used || !a.reff)) return hipErrorInvalidValue;
    const dim3 grid(a.ngroups), block(QC_BLOCK);
    if (a.umap) {
        if (decide) hipLaunchKernelGGL((letkf_qc_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((letkf_qc_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (decide) hipLaunchKernelGGL((letkf_qc_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((letkf_qc_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace spdy
