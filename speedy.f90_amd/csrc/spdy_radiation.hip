// Column physics on the device: the launches of the radiation schemes (physics.f90:146-166 and :180-186).  The schemes are the
// device functions of csrc/spdy_radiation_column.hpp, which the one-launch chain (csrc/spdy_column_chain.hip) calls too; the
// kernels here load what the chain hands over in registers.
#include "spdy_radiation_column.hpp"

namespace spdy {
namespace {
using namespace radiation;

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void radiation_sw_kernel(const RadCols)
{
    const auto &a = kernel_args<RadCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    radiation_sw_column<KMAX>(a, gid, a.precnv[gid], a.precls[gid], a.iptop[gid]);
}

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void radiation_lwdown_kernel(const RadCols)
{
    const auto &a = kernel_args<RadCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    radiation_lwdown_column<KMAX>(a, gid);
}

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void radiation_up_kernel(const RadCols)
{
    const auto &a = kernel_args<RadCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    radiation_up_column<KMAX>(a, gid, a.ts[gid], a.fsfcu[gid]);
}

}  // namespace

hipError_t launch_radiation(const RadCols &a, int phase, hipStream_t s)
{
    if (a.ix <= 0 || a.il <= 0) return hipErrorInvalidValue;
    if (phase == 0) return launch_columns(radiation_sw_kernel<8>, radiation_sw_kernel<16>, a, s);
    if (phase == 1) return launch_columns(radiation_lwdown_kernel<8>, radiation_lwdown_kernel<16>, a, s);
    if (phase == 2) return launch_columns(radiation_up_kernel<8>, radiation_up_kernel<16>, a, s);
    return hipErrorInvalidValue;
}

}  // namespace spdy
