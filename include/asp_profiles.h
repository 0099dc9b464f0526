/*
 * asp_profiles.h -- halo-centred radial profiles and aperture sums in a periodic box (C-ABI
 * of libasp_hip.so, beside asp.h, whose flags and error codes this function uses).
 */
#ifndef ASP_PROFILES_H
#define ASP_PROFILES_H

#include "asp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * For m halo centres with a radius each and nbins radial bins: the number of particles and
 * the sum of up to four particle properties in every (halo, bin), in a periodic box of width
 * L = box_width.  The direction asp_nearest leaves open: haloes overlap (satellites inside
 * hosts, the 3 R200 spheres of neighbours), so a particle belongs to many.
 *
 *   positions  (n, 3) fp64 row-major, any values
 *   props      (nprops, n) fp64, property-major, 0 <= nprops <= 4; NULL when nprops == 0
 *   centres    (m, 3) fp64, every coordinate in [0, L)
 *   radius     (m) fp64, finite and >= 0; NULL: the edges are lengths (the factor below is 1)
 *   edges      (nbins + 1) fp64, finite, edges[0] >= 0, strictly ascending, 1 <= nbins <= 64
 *   count      (m, nbins) int64
 *   sum        (nprops, m, nbins) fp64; NULL when nprops == 0
 *
 * Definition -- fp64 throughout, in this order, no fused multiply-add:
 *   1. the particle is wrapped as asp_nearest wraps a query: w = x - floor(x / L) * L, then
 *      w >= L -> w - L, w < 0 -> w + L;
 *   2. per axis, for centre c: d = w - c, d < -L/2 -> L + d, else d > L/2 -> d - L;
 *   3. d2 = (dx dx + dy dy) + dz dz;
 *   4. t_b = edges[b] * radius[j], T_b = t_b * t_b;
 *   5. particle p is in bin b of halo j iff T_b <= d2 < T_{b+1}.
 * Each (particle, halo) pair has one d2, that of the nearest image: a reach beyond L/2 counts
 * a particle once.  count[j, b] is the exact number of such particles, sum[k, j, b] the fp64
 * sum of props[k, p] over them, in any order.  So: a halo of radius 0 gets zeros; a particle
 * row with a non-finite coordinate belongs to no halo; a non-finite property of a member
 * makes exactly its bins non-finite; a particle exactly on a centre is in bin 0 iff
 * edges[0] == 0.
 *
 * flags: ASP_F_DEVICE_PTRS (every pointer is a device pointer and the work is ordered on
 * `stream`; the call waits for the edges and for the centre check), ASP_F_ACCUMULATE (add
 * into count and sum).  Any other bit: ASP_ERR_INVALID.
 *
 * ASP_ERR_INVALID before any device work, asp_last_error naming the condition: n < 0 or
 * m < 0, nprops outside 0 .. 4, nbins outside 1 .. 64, NULL arrays with non-zero sizes,
 * box_width not finite or <= 0, edges not finite, negative or not strictly ascending (with
 * ASP_F_DEVICE_PTRS the edges are checked after their copy to the host).
 * m * nbins >= 2^31: ASP_ERR_UNSUPPORTED.  A centre outside [0, L) or non-finite, a radius
 * negative or non-finite: ASP_ERR_INVALID, found on the device; the outputs are then
 * unspecified.  m == 0 is valid and needs no device; n == 0 gives zeros (the outputs
 * untouched under ASP_F_ACCUMULATE) and needs no device for host arrays.  Any n runs in one
 * call, in batches of at most 2^30 particles accumulating into the outputs.
 *
 * Method: per batch the particles are wrapped, sorted by the cell of a
 * G x G x G grid over [0, L) and gathered into cell order; every halo gathers from the
 * cells its reach meets (a superset), a lane per light halo, waves over items of a capped
 * number of candidates for the others.  Timing: no stage was added; the prep (centre check,
 * keys, sort, cell starts, gather, candidate count, item scan) is profile stage 19
 * (nearest_prep), the walk stage 20 (nearest_search).  Environment (read per call; the counts
 * are identical and the sums stay within the summation-order bar for every setting):
 * ASP_PROFILE_BATCH (particles per batch, default 2^27), ASP_PROFILE_CELLS (G, 1 .. 256;
 * default floor(cbrt(n / 8)) per batch of n, capped at 256), ASP_PROFILE_LIGHT (haloes with at
 * most this many candidates take the lane class, default 32; 0: none), ASP_PROFILE_ITEM
 * (candidates per wave item, default 1024), ASP_PROFILE_PRUNE (0: no cell row is
 * skipped), ASP_PROFILE_COUNT (diagnostic: asp_last_stats[9] = (particle, halo) pairs tested;
 * the pairs included are the sum of count).
 */
int asp_halo_profiles(const double *positions, const double *props, int32_t nprops, int64_t n,
                      const double *centres, const double *radius, int64_t m,
                      const double *edges, int32_t nbins, double box_width,
                      int64_t *count, double *sum, int32_t flags, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASP_PROFILES_H */
