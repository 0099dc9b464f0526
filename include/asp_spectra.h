/*
 * asp_spectra.h -- sightline spectra: SPH columns deposited in velocity bins (C-ABI of
 * libasp_hip.so, beside asp.h, whose flags, kernel ids and error codes these functions use).
 */
#ifndef ASP_SPECTRA_H
#define ASP_SPECTRA_H

#include "asp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Half-width, in units of b, of the velocity range a particle is deposited over. */
#define ASP_SPECTRA_T 5.0

/*
 * The column density per unit line-of-sight velocity at M sightlines along a box axis -- what
 * an absorption spectrum is made from, out of the fields a sightline object carries
 * (LineOfSightBase, _LineOfSightBase.py:130-189: positions, velocities, masses, temperatures,
 * smoothing lengths).  Each particle's column at the sightline (asp_sample2d's pair term) is
 * spread over velocity bins by a Gaussian of its thermal width, centred on its
 * Hubble-flow-plus-peculiar velocity.
 *
 * Definition.  For sightline s at (px[s], py[s]), particle p and velocity bin k of K = nbins:
 *
 *   N_ps      = a[p] * W(r, h_p)                     the pair term of asp_sample2d, same mask:
 *                                                    r2 = dx*dx + dy*dy < (2 h_p)*(2 h_p), fp64, no FMA
 *   edge_j    = v0 + j*dv                            fp64, j any integer
 *   G_p(j)    = [ erf((edge_{j+1} - vc[p]) / b[p]) - erf((edge_j - vc[p]) / b[p]) ] / (2 dv)
 *   window:   out[s*K + k] = sum_p N_ps * G_p(k),                      k = 0 .. K-1
 *   ring:     out[s*K + k] = sum_p N_ps * sum_{j = k (mod K)} G_p(j)   (the K bins are a periodic ring)
 *
 * vc[p] is the particle's velocity-space coordinate (fp64; the caller forms it, for example
 * H x_los + v_los), b[p] its Doppler parameter.  G is the BIN-AVERAGED Gaussian, so in ring
 * mode sum_k out[s,k] dv is the asp_sample2d column of s, and in window mode as well when the
 * window covers every vc +- T b.  The neighbour sets are asp_sample2d's, bit for bit (kernel ids
 * 0-4; the fp32 entry decides on the fp64 values of its fp32 inputs, the _f64 entry on the
 * reader's fp64 positions, axis 0 / 1 / 2 without cull bits), and N_ps is formed exactly as the
 * sampler forms it: an fp32 term, the pair difference in fp64.  The velocity part is fp64
 * throughout -- the edges, their differences from vc, the scaling by b (one fp64 reciprocal per
 * particle), erf, the bin's difference and its product with N_ps widened to fp64 -- because erf
 * differences in fp32 lose all relative accuracy when dv << b.  Sums are accumulated in fp64 per
 * (sightline, bin) and written as fp32: out0 / out1 hold m * nbins floats, row-major by
 * sightline.  a1 / out1 (both NULL or both non-NULL) give a second sum over the same pairs and
 * bins.
 *
 * Truncation.  Only the bins that meet [vc - T b, vc + T b] are visited, T = ASP_SPECTRA_T = 5
 * (erfc(5) = 1.54e-12 <= 2^-36; the range's ends are moved outwards by 2^-40 of their operands
 * before the bins are taken, so no such bin is lost to rounding).  What is dropped is bounded
 * per (pair, bin) by |N_ps| erfc(T) / (2 dv).  In window mode the visited range is clipped to
 * 0 .. K-1; in ring mode index j goes to j mod K (the mathematical modulus), ranges longer than
 * K included.
 *
 * Admission.  A particle is admitted as asp_sample2d admits it (2|h| > 0 and finite in fp32, u
 * and v finite in fp32) and, in addition, when vc is finite, b is finite and > 0 and
 * T b / dv < 2^24; otherwise it contributes to no bin.  In ring mode a particle whose bin
 * indices reach 2^52 in magnitude (|vc - v0| / dv: edges that are no longer distinct numbers)
 * contributes to no bin either.  A sightline with a non-finite coordinate reads 0 in every bin.
 * A non-finite a of an admitted particle gives unspecified bins on the sightlines inside its
 * disc.
 *
 * flags: ASP_F_DEVICE_PTRS (every pointer is a device pointer; the work is ordered on
 * `stream`), ASP_F_ACCUMULATE (add into the outputs), ASP_F_RATIO (out0 <- out0 / out1 per bin,
 * 0 where out1 == 0: the column-weighted temperature or density of a bin; needs out1, not with
 * ASP_F_ACCUMULATE).  ASP_F_DETERMINISTIC: ASP_ERR_UNSUPPORTED (there are no fixed-point
 * spectra); ASP_F_DEVICE_OUTPUTS: ASP_ERR_INVALID.
 *
 * ASP_ERR_INVALID before any device work, asp_last_error naming the condition: dv not finite or
 * <= 0, v0 not finite, nbins < 1, ring not 0 or 1, and asp_sample2d's own argument errors
 * (n < 0, m < 0, an unknown kernel id, NULL arrays with non-zero sizes -- vc and b included --,
 * one of a1 / out1 without the other, an axis outside 0 .. 2).  m * nbins >= 2^31 and m >= 2^31:
 * ASP_ERR_UNSUPPORTED.  n == 0 gives zeros (the outputs untouched under ASP_F_ACCUMULATE);
 * m == 0 is valid and needs no device; any n runs in one call (batched internally,
 * ASP_MAX_BATCH).
 *
 * Method: asp_sample2d's point grid, particle loader and pair search
 * (both classes: a lane per particle, the wave per particle); the included pairs of a wave step
 * are compacted into LDS and the wave takes them one after the other, its 64 lanes striding
 * over the pair's bins, so one wave-instruction adds 64 neighbouring accumulators with
 * no-return fp64 atomics.  Workspace: asp_sample2d's, plus 8 m nbins bytes per sum (and, for
 * host callers, 4 m nbins per output and 16 bytes per particle of a batch).  Timing: the prep is
 * profile stage 21 (sample_prep); zeroing the accumulators, the deposit and the finalising pass
 * are stage 23 (spectra_deposit).  Environment (read per call): asp_sample2d's ASP_SAMPLE_CELLS,
 * ASP_SAMPLE_WIDE_CELLS, ASP_SAMPLE_WIDE_POINTS; ASP_SPECTRA_WALK (1, the default: the wave
 * walks a pair's bins; 0: the lane that found the pair walks them -- the same sums within the
 * value bar); ASP_SAMPLE_COUNT (diagnostic: asp_last_stats[9] = (particle, sightline) pairs
 * tested, [10] = (pair, bin) adds issued, per sum; the other counters are 0).
 */
int asp_spectra2d(const float *u, const float *v, const float *h, const float *a0, const float *a1,
                  const double *vc, const float *b, int64_t n,
                  const double *px, const double *py, int64_t m,
                  double v0, double dv, int32_t nbins, int32_t ring, int32_t kernel_id,
                  int32_t flags, float *out0, float *out1, int32_t device, void *stream);
int asp_spectra2d_f64(const double *positions, const double *h, const double *a0, const double *a1,
                      const double *vc, const double *b, int64_t n, int32_t axis,
                      const double *px, const double *py, int64_t m,
                      double v0, double dv, int32_t nbins, int32_t ring, int32_t kernel_id,
                      int32_t flags, float *out0, float *out1, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASP_SPECTRA_H */
