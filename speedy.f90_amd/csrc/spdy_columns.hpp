// Launch and addressing layer of the column-physics kernels (csrc/spdy_physics.hip, csrc/spdy_radiation.hip,
// csrc/spdy_surface.hip, csrc/spdy_column_chain.hip), the one device function they share (get_qsat), and what one block of the
// chain hands to a later one per column.
//
// One thread per (state, column): nb * ncol threads in blocks of COLUMN_BLOCK, threads with consecutive longitude in
// consecutive lanes, so every level load and store is one coalesced access per wave.  Each kernel comes as <8> and <16>:
// KMAX is the number of levels its loops are unrolled over (with runtime level < kx predicates), 8 for kx <= 8, else 16.
#pragma once
#include <hip/hip_runtime.h>

#include "spdy_kernels.hpp"

namespace spdy {

constexpr int COLUMN_BLOCK = 64;

// default-real literals and parameters of the reference are float32 values widened to double
__host__ __device__ constexpr double F(float x) { return static_cast<double>(x); }

// physical_constants.f90:22
__device__ constexpr double kCp = F(1004.0f);

// get_qsat (humidity.f90:46-79) for sig > 0: saturation specific humidity [g/kg] at temperature ta, normalised pressure ps and
// sigma sig.  e0 is a double literal, the other constants default reals; the reference's association order, no contraction.
__device__ inline double get_qsat(double ta, double ps, double sig)
{
#pragma clang fp contract(off)
    const double e0 = 6.108e-3, c1 = F(17.269f), c2 = F(21.875f);
    const double t0 = F(273.16f), t1 = F(35.86f), t2 = F(7.66f);
    const double x = ta >= t0 ? c1 * (ta - t0) / (ta - t1) : c2 * (ta - t0) / (ta - t2);
    const double e = e0 * exp(x);
    return 622.0 * e / (sig * ps - 0.378f * e);
}

// This thread's place in the launch: gid = b * ncol + col for state b and column col.  The threads past the last column of the
// last state (gid >= nb * ncol) return at once.
__device__ inline long column_gid() { return (long)blockIdx.x * COLUMN_BLOCK + threadIdx.x; }

// This thread's column: level l (0-based, in the grid's memory order) of a (ix, il, kx) grid of the state at base + l * ncol, a
// (ix, il) field at gid.
struct Column {
    long gid, b, col, base;
    __device__ Column(long g, int ncol, int kx) : gid(g)
    {
        b = g / ncol;
        col = g - b * ncol;
        base = b * ncol * kx + col;
    }
};

// A kernel's by-value argument struct (its ONE argument) where the launch put it: at the start of the kernarg segment, in the
// constant address space.  The schemes are device functions that take their arguments by reference; handed the kernel's own
// parameter they would read a private copy of it, which the compiler splits into scalars that are all loaded at the kernel's
// entry (every level table: hundreds of SGPRs, spilled).  Read in place each table entry is a scalar load where it is used, as
// it is in a kernel that names its parameter directly.  The device functions are templates on the argument type for this.
#define SPDY_KERNARG __attribute__((address_space(4)))
template <class Args>
__device__ __forceinline__ const SPDY_KERNARG Args &kernel_args()
{
    return *(const SPDY_KERNARG Args *)__builtin_amdgcn_kernarg_segment_ptr();
}

// What a block hands to the later blocks of the chain, per column.  The one-launch chain keeps these in registers; the kernels of
// the single blocks store them (where the caller gave a place) and the next kernel loads them.
struct MoistHand { double precnv, precls; int iptop, icnv; };       // iptop after condensation, icnv before it
struct SfcHand { double ts, fsfcu, flux3[4]; };                     // flux3: ustr3 vstr3 shf3 evap3

// The launch of a column kernel whose arguments `a` have nb, ncol and kx: k8 for kx <= 8, k16 for kx <= COLUMN_KMAX.
template <class Args>
hipError_t launch_columns(void (*k8)(Args), void (*k16)(Args), const Args &a, hipStream_t s)
{
    if (a.kx < 5 || a.kx > COLUMN_KMAX || a.nb < 0 || a.ncol <= 0) return hipErrorInvalidValue;
    const long n = (long)a.nb * a.ncol;
    if (!n) return hipSuccess;
    const dim3 grd((unsigned)((n + COLUMN_BLOCK - 1) / COLUMN_BLOCK)), blk(COLUMN_BLOCK);
    hipLaunchKernelGGL(a.kx <= 8 ? k8 : k16, grd, blk, 0, s, a);
    return hipGetLastError();
}

}  // namespace spdy
