// Column physics on the device: the launches of the surface fluxes (physics.f90:169-170) and the boundary layer (:193-205).
// The schemes are the device functions of csrc/spdy_surface_column.hpp, which the one-launch chain
// (csrc/spdy_column_chain.hip) calls too; the kernels here load what the chain hands over in registers.
#include "spdy_surface_column.hpp"

namespace spdy {
namespace {
using namespace surface;

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void surface_fluxes_kernel(const SfcCols)
{
    const auto &a = kernel_args<SfcCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    surface_fluxes_column<KMAX>(a, gid, a.ssrd[gid], a.slrd[gid]);
}

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void pbl_kernel(const PblCols)
{
    const auto &a = kernel_args<PblCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    const Column c(gid, a.ncol, a.kx);
    const double *const f3 = a.flux3 + c.b * 4 * a.ncol + c.col;
    const double flux3[4] = {f3[0], f3[a.ncol], f3[2L * a.ncol], f3[3L * a.ncol]};
    pbl_column<KMAX>(a, gid, a.icnv[gid], flux3);
}

}  // namespace

hipError_t launch_surface_fluxes(const SfcCols &a, hipStream_t s)
{
    if (a.ix <= 0 || a.ncol % a.ix) return hipErrorInvalidValue;
    return launch_columns(surface_fluxes_kernel<8>, surface_fluxes_kernel<16>, a, s);
}

hipError_t launch_pbl(const PblCols &a, hipStream_t s) { return launch_columns(pbl_kernel<8>, pbl_kernel<16>, a, s); }

}  // namespace spdy
