// asp_sample.hip -- SPH sums at arbitrary points (sightline columns): asp_sample2d,
// asp_sample2d_f64.
//
// calculate_pixel_value (_pixel_calculations.pyx:9-36) at M arbitrary points instead of the
// corners of a pixel grid: out[k] = sum_p a[p] W(r, h_p) over the particles with
// r2 = dx dx + dy dy < (2 h_p) (2 h_p), dx = u_p - px[k], dy = v_p - py[k], every quantity of
// the test in fp64 in the reference's operation order (asp.h has the definition).  There is
// no chunk cull: that belongs to create_image.
//
// MI355X layout.  The particles (10^7-10^8) are the stream; the points
// (10^4-10^7, 16 B each in cell order) stay in L2 / Infinity Cache.
//   prep (stage sample_prep, per call): one reduction gives the bounding box of the finite
//     points; a G x G cell grid is laid over it (about kSamplePerCell points per cell,
//     G <= kSampleMaxG; ASP_SAMPLE_CELLS forces G); the points are sorted by row-major cell
//     key (rocPRIM radix sort, the permutation kept), the cell starts come from a count and
//     an exclusive scan, and the fp64 coordinates are gathered into cell order.  Points with
//     a non-finite coordinate get the key past the last cell: nothing visits them, they
//     read 0.  The grid's descriptor stays on the device (no host round trip).
//   deposit (stage sample_deposit, per particle batch; k_sample): one lane per particle.
//     Its box [u - 2|h|, u + 2|h|] x [v - 2|h|, v + 2|h|] (widened by 2^-40 relative, far
//     above the fp64 roundings of the test) gives a cell range through the SAME monotone
//     cell expression the points were keyed with, so no point that can pass is missed; a
//     box that misses the points' bounding box costs nothing more.  Each cell row of the
//     range is one contiguous span of sorted points.  Two classes:
//       narrow (the box meets at most ASP_SAMPLE_WIDE_CELLS cells holding at most
//         ASP_SAMPLE_WIDE_POINTS points): the lane walks its spans;
//       wide: the wave takes the particle (its state broadcast from the owning lane) and the
//         64 lanes stride over each span.
//     Pair test: fp64, exactly the reference's expression -- on gfx950 fp64 multiplies and
//     adds run at the fp32 rate, so the five fp64 operations of the test cost what an fp32
//     test with a band and a fall-back would, without the divergent slow path.  The value:
//     q = sqrt(fl32(r2)) / h and kernel_shape / term_coef, the map's own term arithmetic;
//     the pair difference is formed in fp64, so the term's coordinate error is one fp32
//     rounding of r2 (well inside the maps' 128-pitch local-frame bar).  Terms are added to
//     the point's fp64 (or, ASP_F_DETERMINISTIC, int64 fixed-point) accumulator with global
//     atomics (-munsafe-fp-atomics: the hardware L2 fp64 add).
//   finalise: one pass converts to fp32, applies ratio / accumulate (emit_pixel, the map's)
//     and writes in the caller's point order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/asp.h"
#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map_device.hpp"
#include "asp_prims.hpp"
#include "asp_sample.hpp"

namespace asp {

constexpr int kSampleMaxG = 2048;     // cells per axis at most: a 16 MiB cell-start table
constexpr int kSamplePerCell = 4;     // points per cell the grid aims at
constexpr int kSampleWideCells = 16;  // boxes over more cells go to the wave (ASP_SAMPLE_WIDE_CELLS)
constexpr int kSampleWidePoints = 256;  // ... and boxes holding more points (ASP_SAMPLE_WIDE_POINTS)

// The grid over the points and the call's device-side scalars.
struct SDesc {
    unsigned long long emin[2], emax[2];  // bounding box, order-preserving encodings (atomics)
    double x0, y0, x1, y1;                // the box decoded (k_sdesc); x0 > x1: no finite point
    double sx, sy;                        // cells per unit length, G / (x1 - x0) (0: one cell)
    unsigned cmax[2];                     // max |c| over the particles, fp32 bits (fixed point)
    int k[2];                             // fixed-point scale exponents
    unsigned long long pairs;             // ASP_SAMPLE_COUNT
};

__global__ void k_sinit(SDesc* D) {
    D->emin[0] = D->emin[1] = ~0ull;
    D->emax[0] = D->emax[1] = 0ull;
    D->cmax[0] = D->cmax[1] = 0u;
    D->k[0] = D->k[1] = 0;
    D->pairs = 0ull;
}

// Bounding box of the points whose two coordinates are finite.
__global__ __launch_bounds__(kSBlock) void k_sbbox(const double* __restrict__ px,
                                                    const double* __restrict__ py, long long m,
                                                    SDesc* __restrict__ D) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    unsigned long long lo0 = ~0ull, lo1 = ~0ull, hi0 = 0ull, hi1 = 0ull;
    if (i < m) {
        const double x = px[i], y = py[i];
        if (__builtin_isfinite(x) && __builtin_isfinite(y)) {
            lo0 = hi0 = enc_ordered(x);
            lo1 = hi1 = enc_ordered(y);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo0 = min(lo0, (unsigned long long)__shfl_xor((long long)lo0, o));
        lo1 = min(lo1, (unsigned long long)__shfl_xor((long long)lo1, o));
        hi0 = max(hi0, (unsigned long long)__shfl_xor((long long)hi0, o));
        hi1 = max(hi1, (unsigned long long)__shfl_xor((long long)hi1, o));
    }
    if ((threadIdx.x & 63) == 0 && hi0 != 0ull) {
        atomicMin(&D->emin[0], lo0);
        atomicMin(&D->emin[1], lo1);
        atomicMax(&D->emax[0], hi0);
        atomicMax(&D->emax[1], hi1);
    }
}

__global__ void k_sdesc(SDesc* D, int G) {
    if (D->emax[0] == 0ull) {  // no finite point
        D->x0 = D->y0 = 1.0;
        D->x1 = D->y1 = 0.0;
        D->sx = D->sy = 0.0;
        return;
    }
    D->x0 = dec_ordered(D->emin[0]);
    D->y0 = dec_ordered(D->emin[1]);
    D->x1 = dec_ordered(D->emax[0]);
    D->y1 = dec_ordered(D->emax[1]);
    D->sx = D->x1 > D->x0 ? (double)G / (D->x1 - D->x0) : 0.0;
    D->sy = D->y1 > D->y0 ? (double)G / (D->y1 - D->y0) : 0.0;
}

// Row-major cell key of every point (G * G: a non-finite point), its index, and the cell
// counts.
__global__ __launch_bounds__(kSBlock) void k_skeys(const double* __restrict__ px,
                                                    const double* __restrict__ py, long long m,
                                                    const SDesc* __restrict__ D, int G,
                                                    unsigned* __restrict__ keys, int* __restrict__ idx,
                                                    int* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= m) return;
    const double x = px[i], y = py[i];
    unsigned k = (unsigned)G * (unsigned)G;
    if (__builtin_isfinite(x) && __builtin_isfinite(y))
        k = (unsigned)scell(x, D->x0, D->sx, G) * (unsigned)G + (unsigned)scell(y, D->y0, D->sy, G);
    keys[i] = k;
    idx[i] = (int)i;
    atomicAdd(&cnt[k], 1);
}

// Coordinates into cell order; accumulators zeroed.
template <int NOUT>
__global__ __launch_bounds__(kSBlock) void k_sgather(const double* __restrict__ px,
                                                      const double* __restrict__ py, long long m,
                                                      const int* __restrict__ perm,
                                                      double* __restrict__ sx, double* __restrict__ sy,
                                                      unsigned long long* __restrict__ acc) {
    const long long j = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (j >= m) return;
    const int q = perm[j];
    sx[j] = px[q];
    sy[j] = py[q];
    acc[j] = 0ull;
    if (NOUT == 2) acc[m + j] = 0ull;
}

// The particle arrays of a batch: the fp32 structure of arrays (asp_sample2d), or the
// reader's fp64 arrays with the two position columns of the axis (asp_sample2d_f64).
struct SPart {
    const float *u, *v, *h, *a0, *a1;
    const double *pos, *h64, *a064, *a164;
    int cu, cv;
};

// What the test and the term need of one particle.  The fp32 working values are those
// asp_project2d(_f64) sees (the fp64 entry rounds h and a to nearest, as its staging does),
// and `ok` is footprint()'s admission on them: 2|h| > 0 and finite in fp32, u and v finite in
// fp32.  U, V, H are the values the decision is taken on.
struct SVals {
    double U, V, H;
    float hf, a0, a1;
    bool ok;
};
template <bool F64, int NOUT>
__device__ __forceinline__ SVals sload(const SPart& P, long long p) {
    SVals x;
    if constexpr (F64) {
        x.U = P.pos[3 * p + P.cu];
        x.V = P.pos[3 * p + P.cv];
        x.H = P.h64[p];
        x.hf = (float)x.H;
        x.a0 = (float)P.a064[p];
        x.a1 = NOUT == 2 ? (float)P.a164[p] : 0.0f;
    } else {
        x.U = (double)P.u[p];
        x.V = (double)P.v[p];
        x.hf = P.h[p];
        x.H = (double)x.hf;
        x.a0 = P.a0[p];
        x.a1 = NOUT == 2 ? P.a1[p] : 0.0f;
    }
    const float hd = fabsf(2.0f * x.hf);
    x.ok = hd > 0.0f && __builtin_isfinite(hd) && __builtin_isfinite((float)x.U) &&
           __builtin_isfinite((float)x.V);
    return x;
}

// max |c| over the admitted particles, for the fixed-point scale (finite values only).
template <int KID, int NOUT, bool F64>
__global__ __launch_bounds__(kSBlock) void k_scmax(const SPart P, long long n,
                                                    SDesc* __restrict__ D) {
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    float c0 = 0.0f, c1 = 0.0f;
    if (p < n) {
        const SVals x = sload<F64, NOUT>(P, p);
        if (x.ok) {
            const float t0 = fabsf((float)term_coef<KID>(x.a0, x.hf));
            const float t1 = NOUT == 2 ? fabsf((float)term_coef<KID>(x.a1, x.hf)) : 0.0f;
            c0 = __builtin_isfinite(t0) ? t0 : 0.0f;
            c1 = __builtin_isfinite(t1) ? t1 : 0.0f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        c0 = fmaxf(c0, __shfl_xor(c0, o));
        c1 = fmaxf(c1, __shfl_xor(c1, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (c0 > 0.0f) atomicMax(&D->cmax[0], __float_as_uint(c0));
        if (c1 > 0.0f) atomicMax(&D->cmax[1], __float_as_uint(c1));
    }
}

// The fixed-point exponents (fix_exponent, asp_sample.hpp) from n and max |c|.
__global__ void k_sscale(SDesc* D, long long n) {
    for (int j = 0; j < 2; ++j) D->k[j] = fix_exponent(n, __uint_as_float(D->cmax[j]));
}

// One (particle, point) pair: the reference's test, and the term if it passes.
struct SRec {
    double U, V, T2;   // the decision's values; T2 = (2H)(2H)
    float hinv, s0, s1;
};
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void spair(const SRec& R, const double* __restrict__ sx,
                                      const double* __restrict__ sy, long long m, int j,
                                      unsigned long long* __restrict__ acc) {
    const double dx = R.U - sx[j];  // .pyx:20-28
    const double dy = R.V - sy[j];
    const double r2 = dx * dx + dy * dy;  // .pyx:30 (no contraction: -ffp-contract=off)
    if (r2 < R.T2) {                      // .pyx:31
        const float q = __builtin_amdgcn_sqrtf((float)r2) * R.hinv;
        const float w = kernel_shape<KID>(q);
        acc_add<ACC>(&acc[j], R.s0 * w);
        if constexpr (NOUT == 2) acc_add<ACC>(&acc[m + j], R.s1 * w);
    }
}

template <int KID, int NOUT, int ACC, bool F64>
__global__ __launch_bounds__(kSBlock) void k_sample(const SPart P, long long n,
                                                     const SDesc* __restrict__ D, int G,
                                                     int wide_cells, int wide_points,
                                                     const int* __restrict__ start,
                                                     const double* __restrict__ sx,
                                                     const double* __restrict__ sy, long long m,
                                                     unsigned long long* __restrict__ acc,
                                                     unsigned long long* __restrict__ pairs) {
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    SRec R = {0.0, 0.0, 0.0, 0.0f, 0.0f, 0.0f};
    int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;
    if (p < n) {
        const SVals x = sload<F64, NOUT>(P, p);
        if (x.ok) {
            // |u - px| < 2|H| (1 + 2^-51) for a passing pair; 2^-40 relative to the operands
            // covers that and the roundings of the two edges below many times over
            const double r = 2.0 * fabs(x.H);
            const double rx = r * (1.0 + 0x1p-40) + fabs(x.U) * 0x1p-40;
            const double ry = r * (1.0 + 0x1p-40) + fabs(x.V) * 0x1p-40;
            const double lx = x.U - rx, hx = x.U + rx, ly = x.V - ry, hy = x.V + ry;
            if (hx >= D->x0 && lx <= D->x1 && hy >= D->y0 && ly <= D->y1) {
                cx0 = scell(lx, D->x0, D->sx, G);
                cx1 = scell(hx, D->x0, D->sx, G);
                cy0 = scell(ly, D->y0, D->sy, G);
                cy1 = scell(hy, D->y0, D->sy, G);
                const double t = 2.0 * x.H;
                R.U = x.U;
                R.V = x.V;
                R.T2 = t * t;
                R.hinv = __builtin_amdgcn_rcpf(x.hf);  // value path only, as prep_record
                if constexpr (ACC == kAccFix) {
                    R.s0 = (float)ldexp(term_coef<KID>(x.a0, x.hf), D->k[0]);
                    R.s1 = NOUT == 2 ? (float)ldexp(term_coef<KID>(x.a1, x.hf), D->k[1]) : 0.0f;
                } else {
                    R.s0 = (float)term_coef<KID>(x.a0, x.hf);
                    R.s1 = NOUT == 2 ? (float)term_coef<KID>(x.a1, x.hf) : 0.0f;
                }
            }
        }
    }
    const bool live = cx0 <= cx1;
    bool wide = live && (cx1 - cx0 + 1) * (cy1 - cy0 + 1) > wide_cells;
    int fa = 0, fb = 0;  // the first row's span (often the only one): read once
    if (live && !wide) {  // few cells, but crowded ones: the wave takes those as well
        fa = start[cx0 * G + cy0];
        fb = start[cx0 * G + cy1 + 1];
        int npts = fb - fa;
        for (int cx = cx0 + 1; cx <= cx1; ++cx) npts += start[cx * G + cy1 + 1] - start[cx * G + cy0];
        wide = npts > wide_points;
    }
    unsigned long long tested = 0ull;
    if (live && !wide) {
        for (int cx = cx0; cx <= cx1; ++cx) {
            const int a = cx == cx0 ? fa : start[cx * G + cy0];
            const int b = cx == cx0 ? fb : start[cx * G + cy1 + 1];
            for (int j = a; j < b; ++j) spair<KID, NOUT, ACC>(R, sx, sy, m, j, acc);
            tested += (unsigned long long)(b - a);
        }
    }
    // the wave's wide particles, one after the other, 64 lanes over each span
    unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        SRec Q;
        Q.U = __shfl(R.U, l);
        Q.V = __shfl(R.V, l);
        Q.T2 = __shfl(R.T2, l);
        Q.hinv = __shfl(R.hinv, l);
        Q.s0 = __shfl(R.s0, l);
        Q.s1 = __shfl(R.s1, l);
        const int x0 = __shfl(cx0, l), x1 = __shfl(cx1, l), y0 = __shfl(cy0, l), y1 = __shfl(cy1, l);
        for (int cx = x0; cx <= x1; ++cx) {
            const int a = start[cx * G + y0], b = start[cx * G + y1 + 1];
            for (int j = a + lane; j < b; j += 64) spair<KID, NOUT, ACC>(Q, sx, sy, m, j, acc);
            if (lane == 0) tested += (unsigned long long)(b - a);
        }
    }
    if (pairs) {
        for (int o = 32; o > 0; o >>= 1)
            tested += (unsigned long long)__shfl_xor((long long)tested, o);
        if (lane == 0 && tested) atomicAdd(pairs, tested);
    }
}

// The arguments of the two entry points (one of src32 / src64 is set).
struct SampleArgs {
    const float *u, *v, *h, *a0, *a1;
    const double *pos, *h64, *a064, *a164;
    int axis;
    long long n;
    const double *px, *py;
    long long m;
    int kid, flags;
    float *out0, *out1;
};

static int sample_check(const SampleArgs& A, bool f64) {
    if (A.n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (A.m < 0) return fail(ASP_ERR_INVALID, "m < 0");
    if (A.kid < 0 || A.kid > ASP_KERNEL_WENDLAND_C2_COLUMN)
        return fail(ASP_ERR_INVALID, "unknown kernel_id");
    if (f64 && (A.axis < 0 || A.axis > 2))
        return fail(ASP_ERR_INVALID, "projection axis must be 0 (X), 1 (Y) or 2 (Z); "
                                     "ASP_AXIS_CULL has no meaning without a chunk cull");
    if (A.flags & ASP_F_DEVICE_OUTPUTS)
        return fail(ASP_ERR_INVALID, "ASP_F_DEVICE_OUTPUTS is not supported by asp_sample2d");
    const bool has_a1 = f64 ? A.a164 != nullptr : A.a1 != nullptr;
    if (has_a1 != (A.out1 != nullptr))
        return fail(ASP_ERR_INVALID, "a1 and out1 must both be given or both be NULL");
    if ((A.flags & ASP_F_RATIO) && !A.out1) return fail(ASP_ERR_INVALID, "ASP_F_RATIO needs out1");
    if ((A.flags & ASP_F_RATIO) && (A.flags & ASP_F_ACCUMULATE))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_ACCUMULATE");
    if ((A.flags & ASP_F_RATIO) && (A.flags & ASP_F_DETERMINISTIC))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_DETERMINISTIC "
                                     "(fixed-point components carry no relative precision in "
                                     "kernel-tail points; form ratios from fp64 sums)");
    if (A.m > 0 && (!A.px || !A.py)) return fail(ASP_ERR_INVALID, "NULL point coordinates");
    if (A.m > 0 && !A.out0) return fail(ASP_ERR_INVALID, "out0 is NULL");
    if (A.n > 0) {
        const bool null_in = f64 ? (!A.pos || !A.h64 || !A.a064) : (!A.u || !A.v || !A.h || !A.a0);
        if (null_in) return fail(ASP_ERR_INVALID, "NULL particle array");
    }
    if (A.m > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "m >= 2^31 points per call");
    return ASP_OK;
}

template <bool F64>
static int sample(const SampleArgs& A, int device, hipStream_t stream) {
    ASP_TRY(sample_check(A, F64));
    if (A.m == 0) return ASP_OK;
    const bool dev = A.flags & ASP_F_DEVICE_PTRS;
    const bool acc_flag = A.flags & ASP_F_ACCUMULATE;
    const int nout = A.out1 ? 2 : 1;
    const long long m = A.m, n = A.n;
    if (n == 0 && (acc_flag || !dev)) {  // nothing to add; host outputs need no device
        if (!acc_flag) {
            memset(A.out0, 0, (size_t)m * sizeof(float));
            if (A.out1) memset(A.out1, 0, (size_t)m * sizeof(float));
        }
        return ASP_OK;
    }
    return with_workspace(device, stream, false, [&](Workspace& ws, hipStream_t st) -> int {
        if (ws.prof) ASP_TRY(prof_next(ws));
        stats_clear(ws);
        if (n == 0) {  // device outputs, no particles
            ASP_HIP(hipMemsetAsync(A.out0, 0, (size_t)m * sizeof(float), st));
            if (A.out1) ASP_HIP(hipMemsetAsync(A.out1, 0, (size_t)m * sizeof(float), st));
            stats_publish(ws, device);
            return ASP_OK;
        }
        const bool det = A.flags & ASP_F_DETERMINISTIC;
        const bool count = env_set("ASP_SAMPLE_COUNT");
        Buf* B = ws.sample;

        // ---- prep: the points on the device, keyed, sorted, their cells scanned ----
        StageMark mprep(ws, kSSamplePrep, st);
        const double *dpx = A.px, *dpy = A.py;
        float *d0 = A.out0, *d1 = A.out1;
        const size_t pbytes = (size_t)m * sizeof(double), obytes = (size_t)m * sizeof(float);
        if (!dev) {
            ASP_TRY(to_device(ws, B[kSmpPx], dpx, pbytes, st, Copy::kPlain));
            ASP_TRY(to_device(ws, B[kSmpPy], dpy, pbytes, st, Copy::kPlain));
            ASP_TRY(device_scratch(B[kSmpOut0], d0, obytes));
            if (A.out1) ASP_TRY(device_scratch(B[kSmpOut1], d1, obytes));
            if (acc_flag) {
                ASP_HIP(hipMemcpyAsync(d0, A.out0, obytes, hipMemcpyHostToDevice, st));
                if (d1) ASP_HIP(hipMemcpyAsync(d1, A.out1, obytes, hipMemcpyHostToDevice, st));
            }
        }
        int G = (int)std::ceil(std::sqrt((double)m / kSamplePerCell));
        G = (int)env_int("ASP_SAMPLE_CELLS", std::max(1, std::min(kSampleMaxG, G)), 1, kSampleMaxG);
        const int wide_cells = (int)env_int("ASP_SAMPLE_WIDE_CELLS", kSampleWideCells, 0, INT_MAX);
        const int wide_points = (int)env_int("ASP_SAMPLE_WIDE_POINTS", kSampleWidePoints, 0, INT_MAX);
        const size_t ncell = (size_t)G * G + 1;  // the last: points with a non-finite coordinate
        SDesc* D = nullptr;
        unsigned *kin = nullptr, *kout = nullptr;
        int *iin = nullptr, *iout = nullptr, *cnt = nullptr, *start = nullptr;
        double* sorted = nullptr;
        unsigned long long* acc = nullptr;
        ASP_TRY(device_scratch(B[kSmpDesc], D, sizeof(SDesc)));
        ASP_TRY(device_scratch(B[kSmpKeys], kin, (size_t)m * 2 * sizeof(unsigned)));
        ASP_TRY(device_scratch(B[kSmpIndex], iin, (size_t)m * 2 * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpCellCount], cnt, (ncell + 1) * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpCellStart], start, (ncell + 1) * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpSorted], sorted, 2 * pbytes));
        ASP_TRY(device_scratch(B[kSmpAcc], acc, (size_t)nout * m * sizeof(unsigned long long)));
        kout = kin + m;
        iout = iin + m;
        double *sx = sorted, *sy = sorted + m;
        const unsigned pgrid = (unsigned)((m + kSBlock - 1) / kSBlock);
        hipLaunchKernelGGL(k_sinit, dim3(1), dim3(1), 0, st, D);
        ASP_LAUNCHED();
        hipLaunchKernelGGL(k_sbbox, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, m, D);
        ASP_LAUNCHED();
        hipLaunchKernelGGL(k_sdesc, dim3(1), dim3(1), 0, st, D, G);
        ASP_LAUNCHED();
        ASP_HIP(hipMemsetAsync(cnt, 0, (ncell + 1) * sizeof(int), st));
        hipLaunchKernelGGL(k_skeys, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, m, (const SDesc*)D, G,
                           kin, iin, cnt);
        ASP_LAUNCHED();
        int key_bits = 1;
        while ((1ull << key_bits) <= (unsigned long long)G * G) ++key_bits;
        ASP_TRY(sort_pairs(B[kSmpSortTmp], kin, kout, iin, iout, (size_t)m, key_bits, st));
        ASP_TRY(exclusive_scan_int(B[kSmpScanTmp], cnt, start, ncell + 1, st));
        if (nout == 2)
            hipLaunchKernelGGL(k_sgather<2>, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, m,
                               (const int*)iout, sx, sy, acc);
        else
            hipLaunchKernelGGL(k_sgather<1>, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, m,
                               (const int*)iout, sx, sy, acc);
        ASP_LAUNCHED();
        mprep.done();

        // ---- the particles, batch by batch, into the same accumulators ----
        auto stage = [&](long long a, long long b, SPart& P) -> int {
            const size_t nb = (size_t)(b - a);
            P = SPart{};
            if constexpr (F64) {
                const int cols[3][2] = {{1, 2}, {0, 2}, {0, 1}};  // _projector.py:38-46
                P.cu = cols[A.axis][0];
                P.cv = cols[A.axis][1];
                P.pos = A.pos + 3 * a;
                P.h64 = A.h64 + a;
                P.a064 = A.a064 + a;
                P.a164 = A.a164 ? A.a164 + a : nullptr;
                if (!dev) {
                    ASP_TRY(to_device(ws, B[kSmpPart0], P.pos, nb * 3 * sizeof(double), st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart1], P.h64, nb * sizeof(double), st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart2], P.a064, nb * sizeof(double), st, Copy::kPinned));
                    if (P.a164)
                        ASP_TRY(to_device(ws, B[kSmpPart3], P.a164, nb * sizeof(double), st, Copy::kPinned));
                }
            } else {
                P.u = A.u + a;
                P.v = A.v + a;
                P.h = A.h + a;
                P.a0 = A.a0 + a;
                P.a1 = A.a1 ? A.a1 + a : nullptr;
                if (!dev) {
                    const size_t fb = nb * sizeof(float);
                    ASP_TRY(to_device(ws, B[kSmpPart0], P.u, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart1], P.v, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart2], P.h, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart3], P.a0, fb, st, Copy::kPinned));
                    if (P.a1) ASP_TRY(to_device(ws, B[kSmpPart4], P.a1, fb, st, Copy::kPinned));
                }
            }
            return ASP_OK;
        };
        if (det) {  // the scale needs max |c| over ALL particles before the first term
            ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
                SPart P;
                ASP_TRY(stage(a, b, P));
                const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
                StageMark mk(ws, kSSampleDeposit, st);
                ASP_TRY(dispatch(A.kid, nout, false, [&](auto K, auto NO, auto) -> int {
                    hipLaunchKernelGGL((k_scmax<decltype(K)::value, decltype(NO)::value, F64>), dim3(grid),
                                       dim3(kSBlock), 0, st, P, b - a, D);
                    ASP_LAUNCHED();
                    return ASP_OK;
                }));
                mk.done();
                return ASP_OK;
            }));
            hipLaunchKernelGGL(k_sscale, dim3(1), dim3(1), 0, st, D, n);
            ASP_LAUNCHED();
        }
        unsigned long long* pairs = count ? &D->pairs : nullptr;
        ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
            SPart P;
            ASP_TRY(stage(a, b, P));
            const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
            StageMark mk(ws, kSSampleDeposit, st);
            ASP_TRY(dispatch(A.kid, nout, det, [&](auto K, auto NO, auto AC) -> int {
                hipLaunchKernelGGL((k_sample<decltype(K)::value, decltype(NO)::value,
                                             decltype(AC)::value, F64>),
                                   dim3(grid), dim3(kSBlock), 0, st, P, b - a, (const SDesc*)D, G,
                                   wide_cells, wide_points, (const int*)start, (const double*)sx, (const double*)sy,
                                   m, acc, pairs);
                ASP_LAUNCHED();
                return ASP_OK;
            }));
            mk.done();
            return ASP_OK;
        }));

        // ---- finalise ----
        const int kflags = (acc_flag ? kFlagAccumulate : 0) | ((A.flags & ASP_F_RATIO) ? kFlagRatio : 0);
        StageMark mfin(ws, kSSampleDeposit, st);
        ASP_TRY(dispatch(0, nout, det, [&](auto, auto NO, auto AC) -> int {
            hipLaunchKernelGGL((k_sfinal<decltype(NO)::value, decltype(AC)::value, SDesc>), dim3(pgrid),
                               dim3(kSBlock), 0, st, (const unsigned long long*)acc, m, (const int*)iout,
                               (const SDesc*)D, d0, d1, kflags);
            ASP_LAUNCHED();
            return ASP_OK;
        }));
        mfin.done();
        if (!dev) {
            ASP_TRY(to_host(A.out0, d0, obytes, st));
            if (A.out1) ASP_TRY(to_host(A.out1, d1, obytes, st));
        }
        if (count) {
            unsigned long long e = 0;
            ASP_HIP(hipMemcpyAsync(&e, &D->pairs, sizeof(e), hipMemcpyDeviceToHost, st));
            ASP_HIP(hipStreamSynchronize(st));
            ws.stats[9] = (long long)e;
        }
        if (!dev) ASP_HIP(hipStreamSynchronize(st));
        stats_publish(ws, device);
        return ASP_OK;
    });
}

}  // namespace asp

using namespace asp;

extern "C" int asp_sample2d(const float* u, const float* v, const float* h, const float* a0,
                            const float* a1, int64_t n, const double* px, const double* py,
                            int64_t m, int32_t kernel_id, int32_t flags, float* out0, float* out1,
                            int32_t device, void* stream) {
    t_err.clear();
    SampleArgs A{u, v, h, a0, a1, nullptr, nullptr, nullptr, nullptr, 0, n, px, py, m,
                 kernel_id, flags, out0, out1};
    return sample<false>(A, device, (hipStream_t)stream);
}

extern "C" int asp_sample2d_f64(const double* positions, const double* h, const double* a0,
                                const double* a1, int64_t n, int32_t axis, const double* px,
                                const double* py, int64_t m, int32_t kernel_id, int32_t flags,
                                float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    SampleArgs A{nullptr, nullptr, nullptr, nullptr, nullptr, positions, h, a0, a1, axis, n,
                 px, py, m, kernel_id, flags, out0, out1};
    return sample<true>(A, device, (hipStream_t)stream);
}
