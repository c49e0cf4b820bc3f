// Internal: the counter-based generator include/spdy.h defines ("SPPT"), shared by the SPPT pattern (csrc/spdy_sppt.hip) and the
// nature run's observation noise (csrc/spdy_nature.hip).  Philox4x32-10 with key (seed lo, seed hi) and counter (index, part,
// draws lo, draws hi), so a draw depends on (seed, draws, index, part) only -- not on the launch geometry.
// randn is the reference's (sppt.f90:102-116), float32 literals widened: u = sqrt(-2 log r1), v = (2.0f * 6.28318530718f) r2
// (4 pi: the reference's factor), u sin v.  Full-precision log, sqrt and sin, no contraction.
#pragma once
#include "spdy_columns.hpp"

namespace spdy {

struct Philox4 { unsigned w[4]; };

__device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// draw number `part` of index idx (SPPT: a coefficient's real part 0 and imaginary part 1, before the clip)
__device__ inline double sppt_randn(unsigned idx, unsigned part, unsigned long long draws, unsigned long long seed)
{
#pragma clang fp contract(off)
    const Philox4 x = philox4x32_10(idx, part, (unsigned)draws, (unsigned)(draws >> 32), (unsigned)seed, (unsigned)(seed >> 32));
    const double two26 = 67108864.0, twom53 = 1.0 / 9007199254740992.0;
    const double r1 = ((double)(x.w[0] >> 5) * two26 + (double)(x.w[1] >> 6) + 1.0) * twom53;      // (0, 1]
    const double r2 = ((double)(x.w[2] >> 5) * two26 + (double)(x.w[3] >> 6)) * twom53;            // [0, 1)
    const double u = sqrt(F(-2.0f) * log(r1));
    const double v = F(2.0f * 6.28318530718f) * r2;
    return u * sin(v);
}

}  // namespace spdy
