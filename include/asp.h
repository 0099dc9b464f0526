/*
 * asp.h -- C-ABI of the MI355X-native SPH particle-to-grid projector (libasp_hip.so).
 *
 * Drop-in boundary for astro_sph_tools' map-rendering path.  Each entry point names
 * the reference interface it replaces (paths under
 * /root/reference/src/astro_sph_tools/).  The Python mirror of the reference API
 * (astro-sph-tools_amd/asp_amd/) binds these with ctypes; INTEGRATION.md shows the
 * binding a maintainer would add to the reference itself.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ or torch types cross this boundary;
 *  - every function returns ASP_OK (0) or a negative ASP_ERR_* code, and sets a
 *    thread-local message readable with asp_last_error();
 *  - inputs are borrowed and never written; outputs are written in full;
 *  - particle inputs are float32 structure-of-arrays, already axis-selected: (u, v) are
 *    the two projected coordinates (X -> (y, z), Y -> (x, z), Z -> (x, y);
 *    _projector.py:38-46, _pixel_calculations.pyx:20-28);
 *  - images are (nx, ny) C-order float32, element [xi * ny + yi] (_projector.py:88,117);
 *  - by default pointers are HOST pointers (the library stages them through HBM);
 *    with ASP_F_DEVICE_PTRS they are device pointers on `device` and the call is
 *    ordered on `stream` (a hipStream_t, NULL = the legacy default stream);
 *  - thread-safe: a per-device workspace cache guarded by a mutex; one call at a time
 *    per device enqueues work, and each call's stream first waits for the previous
 *    call's work (an event), so calls on different streams never share buffers in flight.
 */
#ifndef ASP_H
#define ASP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_API_VERSION 1

/* kernel_id: the SPH kernel W(r, h), support 2h, evaluated at the projected 2-D distance
 * r of a (particle, pixel corner) pair.  Ids 0 and 1 are the reference's semantics (S6):
 * the 3-D-normalised kernel, ~ 1/h^3, so a map has units [A]/L^3.  Ids 3 and 4 are the
 * same two kernels integrated along the line of sight,
 *   W_col(r, h) = (K/h^2) F(q),  F(q) = 2 int_0^sqrt(4-q^2) w(sqrt(q^2 + z^2)) dz,  q = r/h,
 * 2-D-normalised (2 pi int W_col r dr = 1): a map is a column density, [A]/L^2, and its
 * sum times the pixel area is sum A.  The neighbour test r^2 < (2h)^2, the chunk cull and
 * every entry point's arguments are the same for all ids; the column kernels have no 3-D
 * form (asp_project3d returns ASP_ERR_INVALID for them). */
#define ASP_KERNEL_CUBIC_SPLINE 0 /* _kernels.pyx:9-20 quartic_spline_kernel (M4 cubic)  */
#define ASP_KERNEL_WENDLAND_C2 1  /* 21/(16 pi h^3) (1-q/2)^4 (1+2q), build-defined      */
#define ASP_KERNEL_INDICATOR 2    /* W = 1 for every included pair: neighbour counting    */
#define ASP_KERNEL_CUBIC_SPLINE_COLUMN 3 /* column integral of id 0: 3/(2 pi h^2) at q = 0 */
#define ASP_KERNEL_WENDLAND_C2_COLUMN 4  /* column integral of id 1: 7/(4 pi h^2) at q = 0 */

/* flags */
#define ASP_F_DEVICE_PTRS 0x1 /* inputs/outputs are device pointers on `device`            */
#define ASP_F_RATIO 0x2       /* two outputs: out0 <- out0 / out1 (0 where out1 == 0)      */
#define ASP_F_ACCUMULATE 0x4  /* add into out0/out1 instead of overwriting                 */
#define ASP_F_DETERMINISTIC 0x8 /* int64 fixed-point accumulation: bitwise reproducible and
                                 * input-order independent maps; relative precision degrades
                                 * for pixels below ~2^-37 n_t max|A W| of their 64x64 tile
                                 * (DESIGN.md §4).  Default: fp64 accumulation.  Not with
                                 * ASP_F_RATIO (ASP_ERR_INVALID): a ratio of fixed-point
                                 * components is imprecise in kernel-tail pixels.           */
#define ASP_F_DEVICE_OUTPUTS 0x10 /* host (pageable) inputs, device outputs: the reader's
                                   * arrays in, a device map out for the RCCL sum; the
                                   * inputs go through pinned bounce buffers (two 32 MiB
                                   * pieces, CPU copy overlapping the DMA)                 */

/* asp_project2d_f64 axis: cull on axis c's columns (the reference's mixed spellings) */
#define ASP_AXIS_CULL(c) (((c) + 1) << 4)

/* errors */
#define ASP_OK 0
#define ASP_ERR_INVALID -1     /* bad argument (ValueError on the Python side)             */
#define ASP_ERR_HIP -2         /* HIP runtime error                                         */
#define ASP_ERR_NOMEM -3       /* device allocation failed                                  */
#define ASP_ERR_UNSUPPORTED -4 /* valid request this build does not implement               */

/* Library version (ASP_API_VERSION * 10000 + build number). */
int asp_version(void);

/* Message for the last failing call on this thread ("" if none). */
const char *asp_last_error(void);

/* Number of visible HIP devices (0 on a host without a GPU; never fails). */
int asp_device_count(void);

/*
 * 2-D projection: replaces create_image (_projector.py:75-120) together with
 * process_chunk (:13-73), calculate_pixel_value (_pixel_calculations.pyx:9-36) and the
 * kernel (_kernels.pyx:9-20).
 *
 *   out0[xi, yi] = sum_p a0[p] * W(r_p, h_p)   over p passing the reference's cull of
 *                  the chunk_size tile holding (xi, yi) AND r_p^2 < (2 h_p)^2,
 *   r_p^2 = (u_p - X_xi)^2 + (v_p - Y_yi)^2,  X_xi = u_min + xi * (u_max-u_min)/nx,
 *   Y_yi = v_min + yi * (v_max - v_min)/nx   (sic: nx -- reference quirk S2).
 *
 * Neighbour membership is decided with the reference's fp64 arithmetic on the fp64
 * values of the fp32 inputs (bit-exact neighbour sets for those inputs; for raw fp64
 * reader arrays use asp_project2d_f64); values are accumulated in fp32 terms.  a1/out1 (both non-NULL or both
 * NULL) give a second map over the same neighbour sets (mass-weighted maps:
 * a0 = m*T, a1 = m, with ASP_F_RATIO).  n == 0 is valid (all-zero image).
 * chunk_size >= 1 is the reference's tile size; it only changes results for
 * non-square images (quirk S2), exactly as in the reference.
 */
int asp_project2d(const float *u, const float *v, const float *h, const float *a0,
                  const float *a1, int64_t n, double u_min, double u_max, double v_min,
                  double v_max, int32_t nx, int32_t ny, int32_t chunk_size, int32_t kernel_id,
                  int32_t flags, float *out0, float *out1, int32_t device, void *stream);

/*
 * Image rows [row_lo, row_hi) of asp_project2d's map only -- the row-slab (image-plane)
 * decomposition of SURVEY.md §8(e) / H2, the reference's own image chunks
 * (_projector.py:89-111) distributed: out0 / out1 hold (row_hi - row_lo) x ny pixels,
 * element [(xi - row_lo) * ny + yi], each equal to the pixel asp_project2d writes for the
 * whole image (same corners, pitches, chunk cull and decisions; particles whose footprint
 * misses the rows are skipped).  Any 0 <= row_lo < row_hi <= nx (the GPU tiles of the
 * call start at row_lo).  Other arguments as asp_project2d.
 */
int asp_project2d_rows(const float *u, const float *v, const float *h, const float *a0,
                       const float *a1, int64_t n, double u_min, double u_max, double v_min,
                       double v_max, int32_t nx, int32_t ny, int32_t chunk_size, int32_t row_lo,
                       int32_t row_hi, int32_t kernel_id, int32_t flags, float *out0,
                       float *out1, int32_t device, void *stream);

/*
 * Several property maps from ONE binning (the callers render m, m*T, ion masses ... of
 * the same particles: io/data_structures/_SnapshotBase.py:618-906): out_k = the
 * asp_project2d map of props[k] for k < nprops <= 6, every map over the same neighbour
 * sets.  The particles are counted and scattered once; the records carry the first two
 * properties' coefficients and, beside them, those of properties 2..5, which further
 * deposit passes read.  nprops <= 2 is asp_project2d; more need ASP_F_DEVICE_PTRS (device
 * pointers) and fp64 accumulation (no ASP_F_RATIO / ASP_F_DETERMINISTIC: form ratios
 * with asp_ratio).  props / outs are host arrays of nprops device pointers.
 */
int asp_project2d_props(const float *u, const float *v, const float *h,
                        const float *const *props, int32_t nprops, int64_t n, double u_min,
                        double u_max, double v_min, double v_max, int32_t nx, int32_t ny,
                        int32_t chunk_size, int32_t kernel_id, int32_t flags,
                        float *const *outs, int32_t device, void *stream);

/*
 * The same on the reader's float64 arrays (positions (n, 3), h, props[k] float64, all on
 * the device: ASP_F_DEVICE_PTRS), with the exact fp64 decisions of asp_project2d_f64.
 */
int asp_project2d_props_f64(const double *positions, const double *h,
                            const double *const *props, int32_t nprops, int64_t n,
                            int32_t axis, double u_min, double u_max, double v_min,
                            double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                            int32_t kernel_id, int32_t flags, float *const *outs,
                            int32_t device, void *stream);

/*
 * SPH-weighted property maps -- north_star's "mass/rho-weighted scatter" over the SoA
 * (x, y, z, h, m, rho, A): out_k = sum_j (m_j / rho_j) props[k]_j W(r_ij, h_j), the SPH
 * estimate of the field props[k] integrated along the line of sight, with rho the
 * reader's densities (io/data_structures/_SnapshotBase.py:833, get_densities) and m its
 * masses (:618-700).  rho NULL: the mass-weighted sums sum_j m_j props[k]_j W.  Each
 * property's fp32 working copy is fl32(props[k] * (m / rho)), evaluated in fp64 and
 * rounded once on the device; binning, neighbour decisions and the deposit are
 * asp_project2d_props'(_f64) -- so with nprops = 2 and ASP_F_RATIO, out0 is the
 * (m/rho)-weighted mean of props[0] over props[1]'s weights.  Host pointers are accepted
 * for nprops <= 2 (as asp_project2d / asp_project2d_f64); mass / rho live where the
 * properties live.
 */
int asp_project2d_sph(const float *u, const float *v, const float *h, const float *mass,
                      const float *rho, const float *const *props, int32_t nprops, int64_t n,
                      double u_min, double u_max, double v_min, double v_max, int32_t nx,
                      int32_t ny, int32_t chunk_size, int32_t kernel_id, int32_t flags,
                      float *const *outs, int32_t device, void *stream);
int asp_project2d_sph_f64(const double *positions, const double *h, const double *mass,
                          const double *rho, const double *const *props, int32_t nprops,
                          int64_t n, int32_t axis, double u_min, double u_max, double v_min,
                          double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                          int32_t kernel_id, int32_t flags, float *const *outs, int32_t device,
                          void *stream);

/*
 * create_image on the reader's own float64 arrays: the drop-in for create_image
 * (_projector.py:75-120) as it is called, with positions (n, 3) float64 row-major (the
 * reader's get_positions, _SnapshotBase.py:708-722), smoothing lengths and properties
 * float64, and the projection axis (0 = X -> (y, z), 1 = Y -> (x, z), 2 = Z -> (x, y);
 * _projector.py:38-46).  The reference decides the chunk cull (_projector.py:38-46, enum
 * comparison) and the pixel test (_pixel_calculations.pyx:20-28, str().encode()) from
 * the axis separately, so some spellings (a str "x") cull on other columns than they
 * test: axis | ASP_AXIS_CULL(c) reproduces that, culling on axis c's columns.  The library stages float32 working copies in HBM and keeps the
 * float64 arrays resident: every (particle, pixel) decision is the reference's fp64 test
 * on the ORIGINAL fp64 values (bit-exact neighbour sets for any fp64 input, not only
 * fp32-representable ones); values accumulate as in asp_project2d.  Host pointers unless
 * ASP_F_DEVICE_PTRS (then device pointers, ordered on `stream`).  Other arguments and
 * flags as asp_project2d.
 */
int asp_project2d_f64(const double *positions, const double *h, const double *a0,
                      const double *a1, int64_t n, int32_t axis, double u_min, double u_max,
                      double v_min, double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                      int32_t kernel_id, int32_t flags, float *out0, float *out1, int32_t device,
                      void *stream);

/*
 * The kernel_func plugin point (_projector.py:26, 86; _pixel_calculations.pyx:30-33): for
 * an arbitrary user kernel W(r, h) -- Python code that cannot run on the device -- the
 * device produces the neighbour pairs and the host evaluates W on them, in a SESSION that
 * stages and bins the particles once per map:
 *
 *   asp_pairs_begin: stage positions (n, 3) / h (axis, extent, chunk_size as
 *     asp_project2d_f64), bin them and count every GPU tile's pairs: tile_pairs[t] for the
 *     ceil(nx/64) * ceil(ny/64) tiles t = tx * ceil(ny/64) + ty (host array).  *session
 *     receives the handle (NULL on error).  With ASP_F_DEVICE_PTRS positions / h are device
 *     arrays that must stay alive until asp_pairs_end, and the emit outputs are device
 *     pointers too.
 *   asp_pairs_emit: for the tiles tile_lo <= t < tile_hi, every (pixel, particle) pair
 *     create_image includes (the exact decision of asp_project2d_f64): particle[k] (index
 *     into the inputs) and r2[k] = dx*dx + dy*dy in fp64 as the reference forms it
 *     (.pyx:13-14, :20-30), k in [offsets[q], offsets[q+1]) for the q-th pixel of the
 *     range -- pixels tile by tile, (lx * 64 + ly) inside a tile, pixels outside the image
 *     empty; offsets ((tile_hi - tile_lo) * 4096 + 1 entries) start at 0 and end at the
 *     sum of tile_pairs over the range, the size particle / r2 must have.  Order inside a
 *     pixel unspecified.  The session keeps the binned records resident between emits
 *     (images of more than 4096 tiles: per window of tile rows, re-binned when a range
 *     moves to the next window).
 *   asp_pairs_end: release the session (NULL is a no-op).
 * A session is used by one thread at a time; it owns its buffers, so other calls on the
 * device may run between its emits.
 */
int asp_pairs_begin(const double *positions, const double *h, int64_t n, int32_t axis,
                    double u_min, double u_max, double v_min, double v_max, int32_t nx,
                    int32_t ny, int32_t chunk_size, int32_t flags, int32_t device, void *stream,
                    int64_t *tile_pairs, void **session);
int asp_pairs_emit(void *session, int32_t tile_lo, int32_t tile_hi, int64_t *offsets,
                   int32_t *particle, double *r2);
int asp_pairs_end(void *session);

/*
 * 3-D voxel cube (build-defined; SURVEY.md §8(a) "512^3 cube" -- no reference
 * counterpart, it extends create_image's pixel semantics (_pixel_calculations.pyx:11-14,
 * :30-34) to voxels; CPU restatement: oracle/asp_oracle.c oracle_project3d):
 *
 *   out[i, j, k - k_lo] = sum_p a[p] * W(r_p, h_p)  over p with r_p^2 < (2 h_p)^2,
 *   r_p^2 = ((x_p - X_i)^2 + (y_p - Y_j)^2) + (z_p - Z_k)^2   (fp64, bit-exact sets),
 *   X_i = x_min + i * (x_max - x_min)/nx, Y_j and Z_k likewise with ny and nz.
 *
 * Only planes k_lo <= k < k_hi are produced (Z-slab ownership across GPUs); out is
 * (nx, ny, k_hi - k_lo) C-order float32.  At most 16384 bricks of 16x16x32 voxels per
 * call (a whole 512^3 cube fits).  flags: ASP_F_DEVICE_PTRS, ASP_F_ACCUMULATE.
 */
int asp_project3d(const float *x, const float *y, const float *z, const float *h,
                  const float *a, int64_t n, double x_min, double x_max, double y_min,
                  double y_max, double z_min, double z_max, int32_t nx, int32_t ny, int32_t nz,
                  int32_t k_lo, int32_t k_hi, int32_t kernel_id, int32_t flags, float *out,
                  int32_t device, void *stream);

/*
 * Kernel evaluation on the device: replaces quartic_spline_kernel(r, h)
 * (_kernels.pyx:9-20) for kernel_id 0; fp64 in and out, same formula and branch order.
 * Host pointers unless ASP_F_DEVICE_PTRS.
 */
int asp_kernel_eval(int32_t kernel_id, const double *r, const double *h, double *w, int64_t n,
                    int32_t flags, int32_t device, void *stream);

/*
 * Bin assignment (the reference's process_chunk cull, _projector.py:38-48): for every
 * particle, the inclusive range of chunk indices [cx0, cx1] x [cy0, cy1] whose cull it
 * passes (empty when cx0 > cx1 or cy0 > cy1).  Computed on the device in fp64 with the
 * reference's operation order; bit-exact membership.  Host pointers unless
 * ASP_F_DEVICE_PTRS.
 */
int asp_chunk_ranges(const float *u, const float *v, const float *h, int64_t n, double u_min,
                     double u_max, double v_min, double v_max, int32_t nx, int32_t ny,
                     int32_t chunk_size, int32_t *cx0, int32_t *cx1, int32_t *cy0,
                     int32_t *cy1, int32_t flags, int32_t device, void *stream);

/*
 * Neighbour sets of selected pixels (calculate_pixel_value's mask,
 * _pixel_calculations.pyx:30-31, restricted to the chunk cull): for pixel k
 * (id = xi * ny + yi), the ascending particle indices in
 * index[offsets[k] .. offsets[k+1]).  Uses the same device inclusion test as
 * asp_project2d.  *total receives the number of pairs; when it exceeds cap, nothing
 * beyond cap is written and the call returns ASP_OK with *total > cap.
 * Host pointers only (a test/inspection entry point).
 */
int asp_pixel_neighbours(const float *u, const float *v, const float *h, int64_t n,
                         double u_min, double u_max, double v_min, double v_max, int32_t nx,
                         int32_t ny, int32_t chunk_size, const int64_t *pixels, int64_t npix,
                         int64_t *offsets, int32_t *index, int64_t cap, int64_t *total,
                         int32_t device);

/*
 * Weighted-map finalisation: out0[i] <- out1[i] != 0 ? out0[i] / out1[i] : 0 for the n
 * elements (what ASP_F_RATIO does inside asp_project2d; used after a cross-GPU sum of
 * the two component maps).  Device pointers only, ordered on `stream`.
 */
int asp_ratio(float *out0, const float *out1, int64_t n, int32_t device, void *stream);

/* Periodic-box operations: pb_flags of asp_stage_particles, op of asp_periodic. */
#define ASP_PB_WRAP 0x1             /* make_periodic (_periodic_box_manipulations.py:36-48) */
#define ASP_PB_SHIFT_ORIGIN 0x2     /* shift_origin (:54-57): x - origin, then wrapped       */
#define ASP_PB_SHIFT_CENTRE 0x4     /* shift_centre (:63-69): x + (L/2 - centre), wrapped    */
#define ASP_PB_ORIGIN_IS_CENTRE 0x8 /* the box is [-L/2, L/2) instead of [0, L)              */
#define ASP_PB_IMAGES 0x10          /* asp_stage_particles: append periodic images           */
#define ASP_PB_DISPLACEMENT 0x20    /* asp_periodic: calculate_wrapped_displacement (:10-20) */

/*
 * Snapshot -> projector staging.  Replaces the host-side step of
 * create_image that takes the reader's arrays (io/data_structures/_SnapshotBase.py:599-725:
 * positions (n, 3) float64 row-major, smoothing lengths and properties float64) to the
 * float32 structure of arrays asp_project2d consumes, with the axis selection of
 * _projector.py:38-46 (axis 0 = X -> (y, z), 1 = Y -> (x, z), 2 = Z -> (x, y)); the
 * conversion (round to nearest, as NumPy's astype(float32)) runs on the device.
 *   u, v, hf, a0f, a1f: DEVICE float32 outputs on `device` of capacity cap (hf, a0f, a1f
 *   may be NULL, as may their inputs h, a0, a1).  Inputs are host pointers, copied in
 *   chunks with copy and conversion overlapped, unless ASP_F_DEVICE_PTRS.
 * Periodic box, pb_flags: at most one of ASP_PB_WRAP,
 *   ASP_PB_SHIFT_ORIGIN, ASP_PB_SHIFT_CENTRE (centre = the new origin / centre, 3 values;
 *   the reference helpers' fp64 arithmetic on the two projected coordinates), optionally
 *   ASP_PB_ORIGIN_IS_CENTRE, and ASP_PB_IMAGES: every particle inside the box
 *   [lo, lo + L)^2 (lo = 0, or -L/2) whose reach 2|h| (+ a 2^-20 margin) crosses a face
 *   gets a copy one box width over (up to 3 per particle), appended after the n
 *   originals in an unspecified order -- projecting the result over the box gives the
 *   periodic map.  *n_out = n + images; if that exceeds cap the images beyond cap are
 *   dropped and the call returns ASP_ERR_INVALID with *n_out set to the size needed.
 */
int asp_stage_particles(const double *positions, const double *h, const double *a0,
                        const double *a1, int64_t n, int32_t axis, const double *centre,
                        double box_width, int32_t pb_flags, float *u, float *v, float *hf,
                        float *a0f, float *a1f, int64_t cap, int64_t *n_out, int32_t flags,
                        int32_t device, void *stream);

/*
 * The periodic-box helpers of tools/_periodic_box_manipulations.py on the device, fp64,
 * bit-identical to the reference: op = ASP_PB_WRAP (make_periodic / calculate_periodic,
 * :36-48), ASP_PB_SHIFT_ORIGIN (shift_origin :54-57, b = new origin), ASP_PB_SHIFT_CENTRE
 * (shift_centre :63-69, b = new centre), ASP_PB_DISPLACEMENT
 * (calculate_wrapped_displacement :10-20, a = from, b = to).  out[i] for i < n; a and b
 * repeat with periods pa and pb (NumPy broadcasting of a (3,) vector over (N, 3)).
 * Device pointers, ordered on `stream`.
 */
int asp_periodic(int32_t op, const double *a, int64_t pa, const double *b, int64_t pb,
                 int64_t n, double box_width, int32_t origin_is_centre, double *out,
                 int32_t device, void *stream);

/*
 * calculate_wrapped_distance (_periodic_box_manipulations.py:22-34): per row of 3, the
 * length (squared != 0: its square) of the wrapped displacement; from / to repeat with
 * periods pf / pt (elements).  Device pointers, ordered on `stream`.
 */
int asp_wrapped_distance(const double *from, int64_t pf, const double *to, int64_t pt,
                         int64_t rows, double box_width, int32_t squared, double *out,
                         int32_t device, void *stream);

/*
 * Smoothing lengths from the k-th nearest neighbour: replaces
 * the scipy KDTree query of io/SWIFT/_SnapshotSWIFT.py:62-83 (dark matter: h = distance to
 * the k-th nearest particle, the particle itself counted, k = 32 there):
 *   h[i] = sqrt(d2_(k)),  d2 = ((x_i - x_j)^2 + (y_i - y_j)^2) + (z_i - z_j)^2  (fp64),
 * d2_(k) the k-th smallest over all j, j = i included -- scipy's Euclidean distance, so
 * the result is bit-identical to the reference's; +inf when n < k (scipy's value for a
 * missing neighbour).  positions (n, 3) float64 row-major, h float64; 1 <= k <= 64,
 * n < 2^31.  Host pointers unless ASP_F_DEVICE_PTRS (then ordered on `stream`).
 * Non-finite values (scipy refuses such arrays; here the call is defined): a row with a NaN
 * or infinite coordinate is nobody's neighbour and gets h = +inf; every other row gets its
 * k-th smallest finite d2 among the rows with a position, or +inf if fewer than k of its d2
 * are finite (too few such rows, or squares that overflow: coordinates ~1e160 apart) -- the
 * value scipy gives on the finite rows alone.  Exact while the finite coordinates' extent
 * (max - min per axis) is itself finite.  Every thread's work is bounded by n for any input
 * bits: a particle without a finite k-th distance after its window scans the array once.
 * Environment (read per call; results do not depend on it): ASP_KNN_WINDOW, ASP_KNN_FINE,
 * ASP_KNN_F32, ASP_KNN_MASK, ASP_KNN_NEAR, ASP_KNN_FILL, ASP_KNN_UNION, ASP_KNN_SUBMIN
 * (csrc/asp_knn.hip), ASP_KNN_THREAD (the one-lane-per-particle form, a diagnostic: same
 * contract), ASP_KNN_COUNT (diagnostic counters: asp_last_stats).
 */
int asp_knn_smoothing_lengths(const double *positions, int64_t n, int32_t k, double *h,
                              int32_t flags, int32_t device, void *stream);

/*
 * Nearest halo centre of every particle in a periodic box: replaces the scipy query of
 * _scripts/find_nearest_haloes.py:196-221, KDTree(halo_centres[mask], boxsize=L).query(
 * positions), once per minimum-halo-mass cut -- here every cut ("set") in one call.
 *   positions (n, 3) float64 row-major, any finite values; centres (m, 3) float64, every
 *   coordinate in [0, L), L = box_width; member[j] bit s set: centre j belongs to set s
 *   (member NULL: every centre in set 0, nsets = 1); 1 <= nsets <= 8; m < 2^31 and fewer
 *   than 2^31 memberships over all sets (else ASP_ERR_UNSUPPORTED); index int32 and distance
 *   float64, both (nsets, n) set-major.
 * Arithmetic (scipy's, fp64, in this order, no fused multiply-add): per axis the query is
 * wrapped, w = x - floor(x / L) * L, then w >= L -> w - L, w < 0 -> w + L; for a centre c,
 * d = w - c, d < -L/2 -> L + d, else d > L/2 -> d - L; d2 = ((dx dx + dy dy) + dz dz).
 * distance[s, i] = sqrt(min d2 over the centres of set s): bit-identical to scipy's
 * query(...)[0].  index[s, i] = the minimising centre's position in `centres` (not in the
 * subset, so np.take(halo_ids, index) needs no masked copy); exact ties in d2 go to the
 * lowest position (scipy's tie order is unspecified).  An empty set gives index -1 and
 * distance +inf (the values the script writes for a cut without haloes).
 * Differences from scipy: a query row with a non-finite coordinate gives index -1 and
 * distance NaN for that row only (scipy raises for the whole array).  A centre outside
 * [0, L) or non-finite is ASP_ERR_INVALID, as scipy refuses such a tree; asp_last_error
 * names the condition.  box_width not finite or <= 0, nsets outside 1..8, member NULL with
 * nsets > 1, n < 0, m < 0, NULL arrays with non-zero sizes: ASP_ERR_INVALID before any
 * device work.  Any n >= 0 runs in one call (batched internally).
 * Host pointers, staged through the device workspace, unless ASP_F_DEVICE_PTRS (then every
 * pointer is a device pointer and the work is ordered on `stream`; the call still waits
 * for the centre check).  Environment (read per call): ASP_NEAREST_SORT (1, the default,
 * searches the queries in the order of their cell key, 0 in the caller's order; same
 * results), ASP_NEAREST_PRUNE (0 scans every cell of every shell; same results),
 * ASP_NEAREST_COUNT (diagnostic: asp_last_stats[9] = distances evaluated).
 */
int asp_nearest(const double *positions, int64_t n, const double *centres, int64_t m,
                const uint32_t *member, int32_t nsets, double box_width, int32_t *index,
                double *distance, int32_t flags, int32_t device, void *stream);

/*
 * SPH sums at arbitrary points -- sightline columns: calculate_pixel_value
 * (_pixel_calculations.pyx:9-36), the reference's point-wise unit of work, at M arbitrary
 * positions instead of the corners of a pixel grid (the positions and directions of
 * LineOfSightFileBase, _LineOfSightBase.py:16-73, for sightlines along the projection axis).
 * With kernel ids 3 / 4 and ion masses from asp_table_interp the result is the column density
 * at the sightline itself.
 *
 *   out0[k] = sum_p a0[p] * W(r, h_p)  over p with  r2 = dx*dx + dy*dy < (2 h_p)*(2 h_p),
 *   dx = u_p - px[k],  dy = v_p - py[k]
 *
 * -- every quantity of the test in fp64, in the reference's operation order (.pyx:20-31), no
 * fused multiply-add; there is NO chunk cull (that is create_image's).  Neighbour sets are
 * bit-exact: asp_sample2d decides on the fp64 values of its fp32 inputs, asp_sample2d_f64 on
 * the reader's fp64 arrays themselves (positions (n, 3) row-major, axis 0 / 1 / 2 selecting
 * the columns as asp_project2d_f64 does; an axis carrying ASP_AXIS_CULL bits is
 * ASP_ERR_INVALID: there is no cull to redirect).  Values: fp32 terms from the map's own
 * term arithmetic (the fp64 entry rounds h and a to fp32 once, as the map's staging does),
 * the pair difference formed in fp64, accumulated in fp64 per point; kernel ids 0 .. 4.
 * a1 / out1 (both NULL or both non-NULL) give a second sum over the same neighbour sets.
 * px, py: fp64 point coordinates in the projected (u, v) frame; out0 / out1: m floats.
 *
 * flags: ASP_F_DEVICE_PTRS (every pointer, px / py included, is a device pointer; the work
 * is ordered on `stream`), ASP_F_RATIO (out0 <- out0 / out1, 0 where out1 == 0; needs out1,
 * not with ASP_F_ACCUMULATE), ASP_F_ACCUMULATE (add into the outputs), ASP_F_DETERMINISTIC
 * (int64 fixed point on ONE scale per output, a power of two taken from n and
 * max_p |a_p| W(0, h_p): bitwise reproducible, independent of the order of the particles and
 * of the points; each term is rounded to <= 2^-46 max|a W(0)|, 2^-57 n max|a W(0)| when that
 * is larger; not with ASP_F_RATIO).  ASP_F_DEVICE_OUTPUTS: ASP_ERR_INVALID.
 *
 * Sizes: n == 0 gives zeros (the outputs untouched under ASP_F_ACCUMULATE); m == 0 is valid
 * and needs no device; m >= 2^31 is ASP_ERR_UNSUPPORTED; any n runs in one call (batched
 * internally, ASP_MAX_BATCH).  n < 0, m < 0, NULL arrays with non-zero sizes, an unknown
 * kernel id, one of a1 / out1 without the other: ASP_ERR_INVALID before any device work,
 * asp_last_error naming the condition.
 *
 * Odd values.  A point with a non-finite coordinate gets 0 (the reference's result: every
 * comparison is false).  Particles are admitted as asp_project2d's footprint() admits them,
 * on the fp32 working values: 2|h| must be > 0 and finite in fp32 and u, v finite in fp32 --
 * h == 0, a non-finite h, u or v, or an h so large that 2h overflows fp32 contribute to no
 * point.  A negative h passes the reference's test ((2h)^2 > 0), so the particle is in the
 * neighbour set of the points inside its disc, as it is in the map's where the chunk cull
 * lets it through; its term is the scalar form a K / h^3 f(r / h) with q = r / h < 0 -- not a
 * physical value, and one the map's deposit paths do not form alike either.  A non-finite a of an admitted particle makes
 * exactly the points inside its disc NaN (the map's NaN pixels contain those: its
 * edge-continuous forms also reach the rest of the particle's candidate box); under
 * ASP_F_DETERMINISTIC those points are unspecified.
 *
 * Method: the points are sorted into a uniform cell grid over their bounding
 * box; each particle visits the cells its box meets -- a lane per particle, or the whole wave
 * when the box meets more than ASP_SAMPLE_WIDE_CELLS cells (default 16) or those cells hold
 * more than ASP_SAMPLE_WIDE_POINTS points (default 256: many sightlines on one position).  Workspace: 48 bytes
 * per point plus 8 bytes per cell.  Periodic boxes: stage with asp_stage_particles(...,
 * ASP_PB_IMAGES) and pass its fp32 device arrays here.  Environment (read per call; results
 * have identical neighbour sets and stay within the value bar for every setting):
 * ASP_SAMPLE_CELLS (cells per axis, 1 .. 2048; default ceil(sqrt(m / 4)) capped at 2048),
 * ASP_SAMPLE_WIDE_CELLS, ASP_SAMPLE_WIDE_POINTS, ASP_SAMPLE_COUNT (diagnostic: asp_last_stats[9] = (particle, point)
 * pairs tested; the map counters are 0 after a sample call).
 */
int asp_sample2d(const float *u, const float *v, const float *h, const float *a0, const float *a1,
                 int64_t n, const double *px, const double *py, int64_t m, int32_t kernel_id,
                 int32_t flags, float *out0, float *out1, int32_t device, void *stream);
int asp_sample2d_f64(const double *positions, const double *h, const double *a0, const double *a1,
                     int64_t n, int32_t axis, const double *px, const double *py, int64_t m,
                     int32_t kernel_id, int32_t flags, float *out0, float *out1,
                     int32_t device, void *stream);

/*
 * Cross-snapshot ID matching: the numerical core of tools/_ArrayReorder.py -- ArrayReorder
 * (:815-1038) and ArrayMapping (:1042-1171), which line two ID orderings up with argsort /
 * isin / searchsorted over int64 IDs (:1003-1038, :1057-1081).  For source IDs S with the
 * optional filter sf and target IDs T with the optional filter tf (filters: one 0/1 byte
 * per ID, NumPy bool_; NULL = all true):
 *   index[j]          = the i with sf[i], tf[j] and S[i] == T[j]; -1 where there is none;
 *   source_matched[i] = sf[i] and some j with tf[j] has T[j] == S[i]   (may be NULL);
 *   counts[0] = targets with index >= 0, counts[1] = sources matched, counts[2] = duplicates
 *   seen (0 = none).  A duplicate is an ID value carried by >= 2 filtered sources AND >= 1
 *   filtered target: duplicated source IDs that no filtered target asks for, or that a
 *   filter removes, are legal, and so are repeated targets (one-to-many).  With duplicates
 *   the call still returns ASP_OK and index / source_matched are unspecified.
 * IDs are arbitrary 64-bit patterns (uint64 IDs reinterpreted; no value is reserved).
 * mode: which of the reference's two objects the caller builds -- it raises from the counts:
 * ASP_MATCH_MAPPING an IndexError when counts[2] != 0 (:1074-1075), ASP_MATCH_REORDER a
 * ValueError when counts[2] != 0 or counts[0] != counts[1] (:836-838: repeated targets make
 * the two differ).  The outputs are the same in both modes.
 * counts is ALWAYS a host array of 3 words and the call waits for it, as asp_nearest waits
 * for its centre check; the other pointers are host pointers, staged through the device
 * workspace, unless ASP_F_DEVICE_PTRS (device pointers, ordered on `stream`).
 * ASP_ERR_INVALID before any device work, asp_last_error naming the condition: n_source < 0,
 * n_target < 0, NULL arrays with non-zero sizes, NULL counts, a mode outside 0..1.  n_source
 * or n_target >= 2^31: ASP_ERR_UNSUPPORTED (index is int32).  n_target == 0 is valid, needs
 * no device and gives counts {0, 0, 0}; n_source == 0 is valid and gives every index -1.
 * Method: a partitioned hash join; workspace 12 bytes per ID plus 16 bytes
 * per partition.  Without duplicates index is unique, so the outputs are bit-reproducible.
 * Environment (read per call): ASP_MATCH_CHUNK_KEYS = source keys per LDS round and the
 * per-partition target (8..4096, rounded down to a power of two; default 4096, the tuned
 * value; small values let tests reach many partitions and multi-round partitions at small
 * n).  Results are identical for every value.  ASP_MATCH_STOP (diagnostic, for timing the
 * phases from outside: 1 returns after the count and scans, 2 after the scatter; the outputs
 * are then meaningless).
 */
#define ASP_MATCH_MAPPING 0 /* ArrayMapping: targets may repeat                             */
#define ASP_MATCH_REORDER 1 /* ArrayReorder: also targets matched == sources matched        */
int asp_match_ids(const int64_t *source_ids, const uint8_t *source_filter, int64_t n_source,
                  const int64_t *target_ids, const uint8_t *target_filter, int64_t n_target,
                  int32_t mode, int32_t *index, uint8_t *source_matched, int64_t *counts,
                  int32_t flags, int32_t device, void *stream);

/*
 * The row gather that applies asp_match_ids' index: replaces the fancy-index copy per field
 * of _ArrayReorder.py:957 and :1129.  data: n_rows rows of row_bytes bytes (any row_bytes
 * >= 1: scalar fields, (N, 3) positions, int8 flags); out: n_index rows.
 *   out[j] = data[index[j]]  for index[j] >= 0;
 *   for index[j] < 0: fill_row (row_bytes bytes) -- or, with fill_row NULL, out[j] is left
 *   untouched: the reference's call with an output_array and no default_value.
 * An index >= n_rows is ASP_ERR_INVALID (found by the gather's own check, never
 * dereferenced; out is then unspecified).  row_bytes < 1, negative sizes, NULL out / index
 * with n_index > 0, NULL data with n_rows > 0: ASP_ERR_INVALID before any device work.
 * Rows whose size and addresses are multiples of 16, 8 or 4 bytes move as vectors of that
 * width, other rows byte by byte.  Host pointers unless ASP_F_DEVICE_PTRS (then every
 * pointer, fill_row included, is a device pointer and the work is ordered on `stream`; the
 * call waits for the index check).
 */
int asp_take_rows(const void *data, int64_t n_rows, int64_t row_bytes, const int32_t *index,
                  int64_t n_index, const void *fill_row, void *out, int32_t flags,
                  int32_t device, void *stream);

/*
 * Ionisation-table interpolation: replaces the scipy
 * RegularGridInterpolator of data_structures/_IonisationTable.py:44-58 (linear,
 * bounds_error=False, fill_value=-inf; the HM01 tables of
 * io/ionisation_tables/_HM01.py:61-92 are 3-D over (log10 n_H, log10 T, redshift)).
 * table: (n0, n1, n2) float64 C-order on strictly ascending axes g0, g1, g2; points:
 * (n, 3) rows, or (n, 2) rows with `zvalue` inserted at axis `zaxis` (ncol = 2;
 * evaluate_at_redshift, :54-58).  out[i] = the interpolated value, bit-identical to scipy
 * 1.15's linear evaluation (fill outside the table, NaN for NaN input);
 * mode 1: out[i] = (a0[i] * a1[i]) * value, mode 2: (a0[i] * a1[i]) * 10^value -- the ion
 * masses m * X_element * f_ion that feed asp_project2d for an ion column map.  Device
 * pointers, ordered on `stream`.
 */
int asp_table_interp3(const double *table, int32_t n0, int32_t n1, int32_t n2,
                      const double *g0, const double *g1, const double *g2,
                      const double *points, int32_t ncol, int32_t zaxis, double zvalue,
                      int64_t n, double fill, int32_t mode, const double *a0, const double *a1,
                      double *out, int32_t device, void *stream);

/*
 * The same for any number of table axes (IonisationTableBase takes N input dimensions,
 * _IonisationTable.py:31-49): table (shape[0], ..., shape[ndim-1]) float64 C-order, axes[d]
 * a device pointer to axis d (a HOST array of ndim pointers; shape is a host array too),
 * 1 <= ndim <= 6.  points: (n, ndim) rows, or (n, ndim - 1) rows with `zvalue` inserted at
 * axis `zaxis` (for ndim 1 that is ncol 0: out is n copies of table(zvalue), as the
 * reference's evaluate_at_redshift returns; `points` is not read and may be NULL, the data
 * pointer of an (n, 0) array).  order 0: scipy's _evaluate_linear (weights multiplied first, every ndim);
 * order 1: its Cython 2-D fast path (value times w0 times w1), which scipy takes for a
 * writeable native-float64 2-D table.  Bit-identical to scipy 1.15; fill / NaN / mode as
 * asp_table_interp3.
 */
int asp_table_interp(const double *table, int32_t ndim, const int32_t *shape,
                     const double *const *axes, const double *points, int32_t ncol,
                     int32_t zaxis, double zvalue, int64_t n, double fill, int32_t mode,
                     int32_t order, const double *a0, const double *a1, double *out,
                     int32_t device, void *stream);

/*
 * Statistics of the last asp_project2d call on `device` (inspection / roofline):
 * stats[0] = records binned (particle x GPU-tile insertions), stats[1] = work items,
 * stats[2] = wide particles, stats[3] = GPU tile edge (pixels), stats[4] = GPU tiles,
 * stats[5] = records per work item, stats[6] = split tiles, stats[7] = partial slabs,
 * stats[8] = records in the large (gathered) stream; with the environment variable
 * ASP_COUNT_EVALS set (diagnostic: one extra kernel, a host sync), the (pixel, particle)
 * lane-slots the deposit kernels spend: stats[9] total = stats[10] small / mid-size stream
 * + stats[11] gathered large stream + stats[12] wide particles (else 0); stats[13] how the
 * records were scattered (1 the speculative scatter enqueued before the counter read-back
 * was kept, 2 record-placement trials, 3 the speculative scatter found the buffers too
 * small and was relaunched after growing them, 0 one plain launch; the largest code over
 * the passes), stats[14] scatter runs of the placement trials, stats[15] layout reuse: 1 the
 * call reused the previous call's bin layout (same device arrays u, v, h, same grid: no
 * count pass, no scans; its scatter proved the layout exact for the arrays' present
 * contents, and stats[13] is 1), 2 it tried and the scatter rejected the layout (the
 * arrays were rewritten in place: the call then counted as usual), 0 not tried; the
 * environment variable ASP_REUSE_LAYOUT=0 (read per call) switches reuse off, and so do
 * ASP_NO_SPECULATE (reuse is a speculative launch) and ASP_COUNT_EVALS (the diagnostic
 * reads the counted pass's records).  Images of more than 4096
 * tiles and batched calls: the sums over all passes.  After asp_knn_smoothing_lengths
 * (ASP_KNN_COUNT) and asp_nearest (ASP_NEAREST_COUNT) the words describe that call: stats[9]
 * = distances evaluated (asp_nearest: over all queries and sets), the map counters 0
 * (asp_knn_smoothing_lengths: stats[9] the window pass's distances, stats[10] the per-lane
 * cell scans', stats[11] the entries the shared cell pass streamed, stats[12] top-k
 * insertions, and stats[8] the waves whose shared cell pass fell back to the per-lane pass:
 * its box of cells, its list of key ranges or its entries beyond what a wave holds); after
 * asp_sample2d(_f64) with ASP_SAMPLE_COUNT stats[9] = (particle, point) pairs tested;
 * after asp_spectra2d(_f64) with it, stats[10] = (pair, bin) adds issued as well.
 */
int asp_last_stats(int32_t device, int64_t *stats, int32_t nstats);

/*
 * Stage timing with HIP events recorded on the call's stream around every launch
 * (enable != 0 starts and resets, 0 stops).  asp_profile_read returns, per stage, the
 * summed milliseconds and the number of launches since the last reset.  Stages:
 * 0 memset, 1 count, 2 colscan, 3 tilescan, 4 scatter, 5 scale, 6 deposit, 7 merge,
 * 8 wide, 9 ratio; cube (asp_project3d): 10 count, 11 colscan, 12 tilescan, 13 scatter,
 * 14 deposit, 15 merge; 16 gather (2-D gathered deposit of the large-record stream);
 * 17 knn_prep, 18 knn_search (asp_knn_smoothing_lengths); 19 nearest_prep, 20 nearest_search
 * (asp_nearest: the centre check and cell sort; the search, with the query sort when on);
 * 21 sample_prep, 22 sample_deposit (asp_sample2d: point keys, sort and cell offsets; the
 * particle -> point deposit with the fixed-point scale and the finalising pass);
 * 23 spectra_deposit (asp_spectra2d, asp_spectra.h: the (pair, velocity bin) deposit and its
 * finalising pass; its prep is stage 21).
 */
int asp_profile(int32_t device, int32_t enable);
/* As asp_profile(device, 1), but events only around the stages whose bit is set in
 * `stage_mask` (bit k = stage k; 0 stops).  Each event pair costs the stream a few
 * microseconds, so a timed run marks only the kernel it reports (bench.py). */
int asp_profile_stages(int32_t device, uint32_t stage_mask);
int asp_profile_read(int32_t device, double *ms_sum, int64_t *launches, int32_t nstages);

/* Release the cached device workspace of `device` (-1: all devices). */
int asp_release(int32_t device);

#ifdef __cplusplus
}
#endif

#endif /* ASP_H */
