// Column physics on the device: the whole chain of get_physical_tendencies (physics.f90:110-205) in ONE launch.
//
// One thread owns one column through all blocks and no block reads another thread's result, so the five calls of
// spdy_column_physics_dev (six kernels with shortwave) are one kernel with no barrier and no communication: the same device
// functions the single kernels call (csrc/spdy_moist_column.hpp, spdy_radiation_column.hpp, spdy_surface_column.hpp), in the
// same order, so every column sees the same instructions on the same values.
//
// Hand-over between the blocks.  The per-column scalars (precnv, precls, iptop, icnv, ssrd on shortwave calls, slrd, ts, fsfcu,
// the four averaged fluxes) stay in registers: 11 values.  se, rh and qsat (3 kx values) go through memory -- the moist block
// holds its column bottom up and the boundary layer top down with the levels kx - 1 and kx at runtime addresses, so a register
// hand-over would be a KMAX x KMAX select, and pbl_kernel<16> alone is at 242 VGPRs; the thread stores them to the workspace
// field the chain uses and loads them back (program order in one thread, same address: no fence).  ttend / qtend are summed in
// memory block by block as the single kernels do, which keeps the reference's order of the sums.
#include "spdy_moist_column.hpp"
#include "spdy_radiation_column.hpp"
#include "spdy_surface_column.hpp"

namespace spdy {
namespace {

// The chain of one column.  SPPT (physics.f90:85-88, :207-222): the column's entry values of ttend and qtend are stored before the
// first block sums into them and loaded back after the last, those of utend and vtend (level kx, the only one the chain changes)
// stay in registers, and every tendency becomes (1 + pattern * mu(k)) * (tend - tend_dyn) + tend_dyn.
template <int KMAX, bool SPPT, class Args, class Sppt>
__device__ __forceinline__ void chain_column(const Args &a, const Sppt &sp, long gid)
{
    const Column c(gid, a.ncol, a.kx);
    const long okx = c.base + (long)(a.kx - 1) * a.ncol;
    double u_dyn = 0.0, v_dyn = 0.0;
    if constexpr (SPPT) {
        for (int k = 0; k < a.kx; ++k) {
            const long o = c.base + (long)k * a.ncol;
            sp.save_t[o] = a.pbl.ttend[o]; sp.save_q[o] = a.pbl.qtend[o];
        }
        u_dyn = a.pbl.utend[okx]; v_dyn = a.pbl.vtend[okx];
    }
    const MoistHand m = moist_column<KMAX>(a.moist, gid);
    // ssrd is written by shortwave calls only and held in memory for the others (include/spdy.h)
    const double ssrd = a.rad.compute_sw ? radiation::radiation_sw_column<KMAX>(a.rad, gid, m.precnv, m.precls, m.iptop)
                                         : a.rad.ssrd[gid];
    const double slrd = radiation::radiation_lwdown_column<KMAX>(a.rad, gid);
    const SfcHand s = surface::surface_fluxes_column<KMAX>(a.sfc, gid, ssrd, slrd);
    radiation::radiation_up_column<KMAX>(a.rad, gid, s.ts, s.fsfcu);
    surface::pbl_column<KMAX>(a.pbl, gid, m.icnv, s.flux3);
    if constexpr (SPPT) {
#pragma clang fp contract(off)
        for (int k = 0; k < a.kx; ++k) {
            const long o = c.base + (long)k * a.ncol;
            const double f = 1 + sp.pattern[o] * sp.mu[k];
            const double td = sp.save_t[o], qd = sp.save_q[o];
            a.pbl.ttend[o] = f * (a.pbl.ttend[o] - td) + td;
            a.pbl.qtend[o] = f * (a.pbl.qtend[o] - qd) + qd;
            if (k == a.kx - 1) {
                a.pbl.utend[o] = f * (a.pbl.utend[o] - u_dyn) + u_dyn;
                a.pbl.vtend[o] = f * (a.pbl.vtend[o] - v_dyn) + v_dyn;
            }
        }
    }
}

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void column_physics_kernel(const ChainCols)
{
    const auto &a = kernel_args<ChainCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    chain_column<KMAX, false>(a, a, gid);
}

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void column_physics_sppt_kernel(const ChainSpptCols)
{
    const auto &a = kernel_args<ChainSpptCols>();
    const long gid = column_gid();
    if (gid >= (long)a.c.nb * a.c.ncol) return;
    chain_column<KMAX, true>(a.c, a, gid);
}

bool chain_ok(const ChainCols &a)
{
    const MoistCols &m = a.moist;
    const bool same = a.nb == m.nb && a.ncol == m.ncol && a.kx == m.kx && a.rad.nb == m.nb && a.sfc.nb == m.nb && a.pbl.nb == m.nb && a.rad.ncol == m.ncol && a.sfc.ncol == m.ncol &&
                      a.pbl.ncol == m.ncol && a.rad.kx == m.kx && a.sfc.kx == m.kx && a.pbl.kx == m.kx;
    if (!same || a.rad.ix <= 0 || a.rad.il <= 0 || a.sfc.ix <= 0 || m.ncol % a.sfc.ix) return false;
    return m.se && m.rh && m.qsat && a.rad.ssrd;
}

}  // namespace

hipError_t launch_column_chain(const ChainCols &a, hipStream_t s)
{
    if (!chain_ok(a)) return hipErrorInvalidValue;
    return launch_columns(column_physics_kernel<8>, column_physics_kernel<16>, a, s);
}

hipError_t launch_column_chain_sppt(const ChainSpptCols &a, hipStream_t s)
{
    if (!chain_ok(a.c) || !a.pattern || !a.save_t || !a.save_q) return hipErrorInvalidValue;
    const ChainCols &c = a.c;
    if (c.kx < 5 || c.kx > COLUMN_KMAX || c.nb < 0 || c.ncol <= 0) return hipErrorInvalidValue;
    const long n = (long)c.nb * c.ncol;
    if (!n) return hipSuccess;
    const dim3 grd((unsigned)((n + COLUMN_BLOCK - 1) / COLUMN_BLOCK)), blk(COLUMN_BLOCK);
    hipLaunchKernelGGL(c.kx <= 8 ? column_physics_sppt_kernel<8> : column_physics_sppt_kernel<16>, grd, blk, 0, s, a);
    return hipGetLastError();
}

}  // namespace spdy
