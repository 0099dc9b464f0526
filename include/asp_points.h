/*
 * asp_points.h -- SPH sums at arbitrary 3-D points (C-ABI of libasp_hip.so, beside asp.h,
 * whose flags, kernel ids and error codes these functions use).
 */
#ifndef ASP_POINTS_H
#define ASP_POINTS_H

#include "asp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * SPH sums at arbitrary 3-D points -- field values at positions (halo centres, star or
 * black-hole particles, the particles of another snapshot) and the run of a field along
 * sightlines of any direction (LineOfSightFileBase, _LineOfSightBase.py:16-73: a start
 * position and a direction vector per sightline; the bins' centres are the points).
 * asp_sample3d is to asp_project3d what asp_sample2d is to asp_project2d:
 *
 *   out0[k] = sum_p a0[p] * W(r, h_p)  over p with  r2 < (2 h_p)*(2 h_p),
 *   r2 = (dx*dx + dy*dy) + dz*dz,  dx = x_p - px[k],  dy = y_p - py[k],  dz = z_p - pz[k]
 *
 * -- every quantity of the test in fp64, in this order, no fused multiply-add: asp_project3d's
 * contract (the oracle's voxel_pass), so the neighbour set of a point that coincides with a
 * voxel corner is the cube's, bit for bit.  asp_sample3d decides on the fp64 values of its
 * fp32 inputs, asp_sample3d_f64 on the reader's fp64 positions themselves ((n, 3) row-major).
 * Values: fp32 terms from the 2-D sampler's scalar term arithmetic, q = sqrt(fl32(r2)) / h
 * (the fp64 entry rounds h and a to fp32 once), the pair difference formed in fp64 -- no
 * local frame -- accumulated in fp64 per point.  Kernel ids 0, 1, 2; the column kernels
 * (ids 3, 4) have no 3-D form and are ASP_ERR_INVALID, as for asp_project3d.
 * a1 / out1 (both NULL or both non-NULL) give a second sum over the same neighbour sets.
 * px, py, pz: fp64 point coordinates; out0 / out1: m floats.
 *
 * flags: ASP_F_DEVICE_PTRS (every pointer, px / py / pz included, is a device pointer; the
 * work is ordered on `stream`), ASP_F_RATIO (out0 <- out0 / out1, 0 where out1 == 0; needs
 * out1, not with ASP_F_ACCUMULATE), ASP_F_ACCUMULATE (add into the outputs),
 * ASP_F_DETERMINISTIC (int64 fixed point on ONE scale per output, a power of two taken from n
 * and max_p |a_p| W(0, h_p): bitwise reproducible, independent of the order of the particles
 * and of the points, of the batching and of host or device callers; each term is rounded to
 * <= 2^-46 max|a W(0)|, 2^-57 n max|a W(0)| when that is larger; not with ASP_F_RATIO).
 * ASP_F_DEVICE_OUTPUTS: ASP_ERR_INVALID.
 *
 * Sizes: n == 0 gives zeros (the outputs untouched under ASP_F_ACCUMULATE); m == 0 is valid
 * and needs no device; m >= 2^31 is ASP_ERR_UNSUPPORTED; any n runs in one call (batched
 * internally, ASP_MAX_BATCH).  n < 0, m < 0, NULL arrays with non-zero sizes, an unknown or
 * column kernel id, one of a1 / out1 without the other: ASP_ERR_INVALID before any device
 * work, asp_last_error naming the condition.
 *
 * Odd values.  A point with a non-finite coordinate gets 0.  A particle is admitted when
 * 2|h| is > 0 and finite in fp32 and x, y, z are finite in fp32 -- h == 0, a non-finite h, x,
 * y or z, or an h so large that 2h overflows fp32 contribute to no point.  A negative h
 * passes the test ((2h)^2 > 0, as in the oracle): the particle is in the neighbour set of the
 * points inside its ball; its term (q = r / h < 0) is no physical value and only the
 * neighbour counts are specified.  A non-finite a of an admitted particle makes exactly the
 * points inside its ball NaN; under ASP_F_DETERMINISTIC those points are unspecified.
 *
 * Method: the points are sorted into a uniform G x G x G cell grid over
 * their bounding box, keyed (cx G + cy) G + cz; each particle visits the cell rows its box
 * meets -- a lane per particle, or the whole wave when the box meets more than
 * ASP_SAMPLE_WIDE_CELLS cells (default 27) or those cells hold more than
 * ASP_SAMPLE_WIDE_POINTS points (default 16).  Workspace, shared with asp_sample2d: with
 * device pointers and one sum 56 bytes per point (keys and indices in and out, the sorted
 * coordinates, the accumulator), 64 with a second sum, plus 8 bytes per cell; host callers add
 * the staged arrays (24 bytes per point of coordinates, 4 per output, and the particle batch).  Timing: the prep is profile stage 21 (sample_prep);
 * the deposit, the fixed-point scale and the finalising pass are stage 22 (sample_deposit).
 * Environment (read per call; results have identical neighbour sets and stay within the
 * value bar for every setting): ASP_SAMPLE_CELLS (cells per axis, 1 .. 160; default
 * ceil(cbrt(m / 4)) capped at 160), ASP_SAMPLE_WIDE_CELLS, ASP_SAMPLE_WIDE_POINTS,
 * ASP_SAMPLE3D_WALK (the wave's walk: 1, the default, strides over the concatenated spans of
 * 64 cell rows at a time; 0 strides each row's span on its own), ASP_SAMPLE3D_WALK_MIX (m,
 * default 1: within walk 1, a 64-row chunk with at most 1 + m * ceil(points / 64) non-empty
 * rows -- few, long rows -- is strided row by row after all; 0: only a single row is),
 * ASP_SAMPLE_COUNT
 * (diagnostic: asp_last_stats[9] = (particle, point) pairs tested; the other counters are 0).
 */
int asp_sample3d(const float *x, const float *y, const float *z, const float *h,
                 const float *a0, const float *a1, int64_t n,
                 const double *px, const double *py, const double *pz, int64_t m,
                 int32_t kernel_id, int32_t flags, float *out0, float *out1,
                 int32_t device, void *stream);
int asp_sample3d_f64(const double *positions, const double *h, const double *a0,
                     const double *a1, int64_t n,
                     const double *px, const double *py, const double *pz, int64_t m,
                     int32_t kernel_id, int32_t flags, float *out0, float *out1,
                     int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASP_POINTS_H */
