// Column physics on the device: the launch of the precipitation block (physics.f90:110-138).  The block itself is the device
// function moist_column (csrc/spdy_moist_column.hpp), which the one-launch chain (csrc/spdy_column_chain.hip) calls too.
#include "spdy_moist_column.hpp"

namespace spdy {
namespace {

template <int KMAX>
__global__ __launch_bounds__(COLUMN_BLOCK) void moist_columns_kernel(const MoistCols)
{
    const auto &a = kernel_args<MoistCols>();
    const long gid = column_gid();
    if (gid >= (long)a.nb * a.ncol) return;
    moist_column<KMAX>(a, gid);
}

}  // namespace

hipError_t launch_moist_columns(const MoistCols &a, hipStream_t s)
{
    return launch_columns(moist_columns_kernel<8>, moist_columns_kernel<16>, a, s);
}

}  // namespace spdy
