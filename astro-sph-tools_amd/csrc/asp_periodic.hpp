// asp_periodic.hpp -- the periodic-box arithmetic of asp_nearest and asp_halo_profiles, defined
// once: scipy's wrap and periodic distance (fp64, no contraction; include/asp.h has the
// definition), the monotone cell expression both grids use, the validation of a centre and
// the margin every cell-face bound is reduced by.  include/asp_profiles.h promises that a
// (particle, halo) pair is decided by asp_nearest's arithmetic, bit for bit: both units call
// these functions.
#pragma once

#include <hip/hip_runtime.h>

#include "asp_host.hpp"

namespace asp {

// scipy's wrap of a query coordinate into the box: x - floor(x / L) * L, then its two
// corrections for the rounding of that expression.
__device__ __forceinline__ double wrap_box(double x, double L) {
    double w = x - floor(x / L) * L;
    if (w >= L) w = w - L;
    if (w < 0.0) w = w + L;
    return w;
}

// Cell of a coordinate in [0, L] (a wrapped query may equal L): min(G - 1, floor(c G / L)).
// The same expression for centres and queries, monotone in c.  Clamped at both ends in
// fp64: a finite query so large that its wrap loses the box (|x| >~ 2^52 L) still gets a
// cell inside the table.
__device__ __forceinline__ int cell_of(double c, int G, double L) {
    double f = floor(c * (double)G / L);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)(G - 1)) f = (double)(G - 1);
    return (int)f;
}

// scipy's periodic squared distance (wrapped query first): per axis d = w - c folded into
// [-L/2, L/2], then ((dx dx + dy dy) + dz dz).
__device__ __forceinline__ double fold(double d, double L, double halfL) {
    if (d < -halfL) return L + d;
    if (d > halfL) return d - L;
    return d;
}
__device__ __forceinline__ double pdist2(double wx, double wy, double wz, double cx, double cy,
                                         double cz, double L, double halfL) {
    const double dx = fold(wx - cx, L, halfL), dy = fold(wy - cy, L, halfL),
                 dz = fold(wz - cz, L, halfL);
    return (dx * dx + dy * dy) + dz * dz;
}

// The margin every bound built from cell faces gives away, for a grid of cell edge h = L / G.
// Cells come from cell_of(), so cell k of an axis is [k h, (k + 1) h) up to a few ulp of L
// (~2^-50 L); a face position k h, a difference to it and the folded difference the distance
// is built from each add one more rounding of that size.  2^-20 h >= 2^-28 L (G <= 256) is
// far more than all of them together, so a lower bound on a separation reduced by the margin
// is a lower bound on the COMPUTED separation, and a reach widened by it covers every cell
// the computed arithmetic can place a member in.
__device__ __forceinline__ double face_margin(double h) { return h * 0x1p-20; }

// What is wrong with centre j of c (m x 3) in the box [0, L): bit 0: a coordinate >= L,
// bit 1: a negative coordinate, bit 2: a non-finite one.
__device__ __forceinline__ int centre_bits(const double* __restrict__ c, long long j, double L) {
    int bad = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double v = c[3 * j + a];
        if (!__builtin_isfinite(v)) bad |= 4;
        else if (v >= L) bad |= 1;
        else if (v < 0.0) bad |= 2;
    }
    return bad;
}

// The error of the centre_bits() of all centres or-ed together, or ASP_OK.
inline int centre_error(int bits) {
    if (bits & 4)
        return fail(ASP_ERR_INVALID, "a centre coordinate is not finite (centres must lie inside "
                                     "the periodic box [0, box_width))");
    if (bits & 1)
        return fail(ASP_ERR_INVALID, "a centre coordinate is >= box_width: outside the periodic box");
    if (bits & 2)
        return fail(ASP_ERR_INVALID, "a centre coordinate is negative: outside the periodic box");
    return ASP_OK;
}

}  // namespace asp
