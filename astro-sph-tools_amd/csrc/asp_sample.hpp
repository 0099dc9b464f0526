// asp_sample.hpp -- what the 2-D sampler (asp_sample.hip) and the 3-D sampler
// (asp_sample3d.hip) share: the order-preserving fp64 encoding of the bounding-box atomics,
// the monotone cell expression, the fixed-point scale exponent and the finalising pass.
// Each unit keeps its own descriptor (SDesc / SDesc3); the pieces here only need its
// fixed-point exponents k[2].
#pragma once

#include <hip/hip_runtime.h>

#include "asp_device.hpp"
#include "asp_map_device.hpp"

namespace asp {

constexpr int kSBlock = 256;

// fp64 <-> unsigned with the same order (for atomicMin / atomicMax).
__device__ __forceinline__ unsigned long long enc_ordered(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec_ordered(unsigned long long e) {
    const unsigned long long b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}

// Cell of a coordinate along one axis: min(G - 1, max(0, floor((c - c0) s))), monotone
// non-decreasing in c (a subtraction, a multiplication by s >= 0 and a floor), the same
// expression for the points and for the particles' box edges.  A NaN product (0 * inf when
// the box is degenerate) gives cell 0.
__device__ __forceinline__ int scell(double c, double c0, double s, int G) {
    double f = floor((c - c0) * s);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)(G - 1)) f = (double)(G - 1);
    return (int)f;
}

// Fixed-point exponent: every scaled term stays below 2^50 (f2fix needs < 2^51) and a sum
// of n of them below 2^62, each with a factor 16 to spare for |f| > 1 (a negative h gives
// q < 0, where the cubic's polynomial reaches 11).  It depends on n and max |c| only, so
// the sums do not depend on the order of the particles or of the points.
__device__ __forceinline__ int fix_exponent(long long n, float cm) {
    int k = 0;
    if (cm > 0.0f && n > 0) {
        int es, et;
        frexp((double)n * (double)cm, &es);
        frexp((double)cm, &et);
        k = min(58 - es, 46 - et);
    }
    return k;
}

// Accumulators (cell order) -> fp32 outputs in the caller's order: emit_pixel, the map's
// conversion, accumulate and ratio.  DESC: the unit's descriptor (its k[2]).
template <int NOUT, int ACC, class DESC>
__global__ __launch_bounds__(kSBlock) void k_sfinal(const unsigned long long* __restrict__ acc,
                                                     long long m, const int* __restrict__ perm,
                                                     const DESC* __restrict__ D,
                                                     float* __restrict__ out0,
                                                     float* __restrict__ out1, int flags) {
    const long long j = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (j >= m) return;
    emit_pixel<NOUT, ACC>((long long)perm[j], acc[j], NOUT == 2 ? acc[m + j] : 0ull, D->k[0],
                          D->k[1], out0, out1, flags);
}

}  // namespace asp
