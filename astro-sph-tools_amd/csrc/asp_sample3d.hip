// asp_sample3d.hip -- SPH sums at arbitrary 3-D points (field values at positions,
// sightline profiles): asp_sample3d, asp_sample3d_f64 (include/asp_points.h).
//
// asp_project3d's voxel test at M arbitrary positions instead of the corners of a voxel
// lattice: out[k] = sum_p a[p] W(r, h_p) over the particles with
// r2 = (dx dx + dy dy) + dz dz < (2 h_p) (2 h_p), every quantity of the test in fp64, in
// this order, without contraction.  The method is the 2-D sampler's (asp_sample.hip,
// DESIGN.md §20) with one more axis:
//   prep (stage sample_prep): bounding box of the finite points, a G x G x G cell grid over
//     it (about kPerCell points per cell, G <= kMaxG3: the cell-start table stays at the 2-D
//     sampler's 16 MiB), keys (cx G + cy) G + cz -- the cells of one (cx, cy) ROW are one
//     contiguous span of sorted points -- rocPRIM sort, count + scan for the cell starts,
//     the three fp64 coordinates gathered into cell order.  No host round trip.
//   deposit (stage sample_deposit; k_sample3): one lane per particle.  Its box, widened by
//     2^-40 relative and passed through the points' own cell expression, gives a cell range
//     that is a superset of the cells of every point that can pass.  Two classes:
//       narrow: the lane walks the spans of its rows;
//       wide (more than ASP_SAMPLE_WIDE_CELLS cells or ASP_SAMPLE_WIDE_POINTS points): the
//         wave takes the particle.  A 3-D box meets many short rows, so the wave does not
//         stride row by row (most lanes would idle on a 24-point row): 64 rows at a time,
//         each lane reads one row's span, a wave scan turns the lengths into offsets, and
//         the wave strides over the CONCATENATION of the 64 spans, each lane finding its
//         row by a 6-step search over the offsets held in the lanes' registers.  A chunk of
//         few, long rows (crowded cells: each row fills the wave by itself) is strided row
//         by row instead, the search being pure overhead there (ASP_SAMPLE3D_WALK_MIX).
//         ASP_SAMPLE3D_WALK=0 selects the per-row stride everywhere (the A/B form).
//   finalise: k_sfinal (asp_sample.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/asp_points.h"
#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map_device.hpp"
#include "asp_prims.hpp"
#include "asp_sample.hpp"

namespace asp {

constexpr int kMaxG3 = 160;          // cells per axis at most: 4.1e6 cells, a 16 MiB table
constexpr int kPerCell3 = 4;         // points per cell the grid aims at
constexpr int kWideCells3 = 27;      // boxes over more cells go to the wave (ASP_SAMPLE_WIDE_CELLS)
constexpr int kWidePoints3 = 16;     // ... and boxes holding more points (ASP_SAMPLE_WIDE_POINTS;
                                     // measured: DESIGN.md §21 -- a lane that walks more alone idles 63)
constexpr int kWalkRow = 0;          // wide class: 64 lanes stride one row's span at a time
constexpr int kWalkFlat = 1;         // ... or over the concatenation of 64 rows' spans
// In the flat walk a 64-row chunk with at most 1 + kWalkMix * ceil(points / 64) non-empty rows
// is strided row by row after all (ASP_SAMPLE3D_WALK_MIX; 0: never, but for a single row)
constexpr int kWalkMix = 1;

// The grid over the points and the call's device-side scalars.
struct SDesc3 {
    unsigned long long emin[3], emax[3];  // bounding box, order-preserving encodings (atomics)
    double lo[3], hi[3];                  // the box decoded (k_p3desc); lo[0] > hi[0]: no finite point
    double s[3];                          // cells per unit length, G / (hi - lo) (0: one cell)
    unsigned cmax[2];                     // max |c| over the particles, fp32 bits (fixed point)
    int k[2];                             // fixed-point scale exponents
    unsigned long long pairs;             // ASP_SAMPLE_COUNT
};

__global__ void k_p3init(SDesc3* D) {
    for (int d = 0; d < 3; ++d) {
        D->emin[d] = ~0ull;
        D->emax[d] = 0ull;
    }
    D->cmax[0] = D->cmax[1] = 0u;
    D->k[0] = D->k[1] = 0;
    D->pairs = 0ull;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// Bounding box of the points whose three coordinates are finite.
__global__ __launch_bounds__(kSBlock) void k_p3bbox(const double* __restrict__ px,
                                                     const double* __restrict__ py,
                                                     const double* __restrict__ pz, long long m,
                                                     SDesc3* __restrict__ D) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    if (i < m) {
        const double c[3] = {px[i], py[i], pz[i]};
        if (finite3(c[0], c[1], c[2]))
            for (int d = 0; d < 3; ++d) lo[d] = hi[d] = enc_ordered(c[d]);
    }
    for (int d = 0; d < 3; ++d)
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = min(lo[d], (unsigned long long)__shfl_xor((long long)lo[d], o));
            hi[d] = max(hi[d], (unsigned long long)__shfl_xor((long long)hi[d], o));
        }
    if ((threadIdx.x & 63) == 0 && hi[0] != 0ull)
        for (int d = 0; d < 3; ++d) {
            atomicMin(&D->emin[d], lo[d]);
            atomicMax(&D->emax[d], hi[d]);
        }
}

__global__ void k_p3desc(SDesc3* D, int G) {
    for (int d = 0; d < 3; ++d) {
        if (D->emax[0] == 0ull) {  // no finite point
            D->lo[d] = 1.0;
            D->hi[d] = 0.0;
            D->s[d] = 0.0;
        } else {
            D->lo[d] = dec_ordered(D->emin[d]);
            D->hi[d] = dec_ordered(D->emax[d]);
            D->s[d] = D->hi[d] > D->lo[d] ? (double)G / (D->hi[d] - D->lo[d]) : 0.0;
        }
    }
}

// Cell key (cx G + cy) G + cz of every point (G^3: a non-finite point), its index, and the
// cell counts.
__global__ __launch_bounds__(kSBlock) void k_p3keys(const double* __restrict__ px,
                                                     const double* __restrict__ py,
                                                     const double* __restrict__ pz, long long m,
                                                     const SDesc3* __restrict__ D, int G,
                                                     unsigned* __restrict__ keys,
                                                     int* __restrict__ idx, int* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= m) return;
    const double x = px[i], y = py[i], z = pz[i];
    const unsigned g = (unsigned)G;
    unsigned k = g * g * g;
    if (finite3(x, y, z))
        k = ((unsigned)scell(x, D->lo[0], D->s[0], G) * g + (unsigned)scell(y, D->lo[1], D->s[1], G)) * g +
            (unsigned)scell(z, D->lo[2], D->s[2], G);
    keys[i] = k;
    idx[i] = (int)i;
    atomicAdd(&cnt[k], 1);
}

// Coordinates into cell order; accumulators zeroed.
template <int NOUT>
__global__ __launch_bounds__(kSBlock) void k_p3gather(const double* __restrict__ px,
                                                       const double* __restrict__ py,
                                                       const double* __restrict__ pz, long long m,
                                                       const int* __restrict__ perm,
                                                       double* __restrict__ sx, double* __restrict__ sy,
                                                       double* __restrict__ sz,
                                                       unsigned long long* __restrict__ acc) {
    const long long j = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (j >= m) return;
    const int q = perm[j];
    sx[j] = px[q];
    sy[j] = py[q];
    sz[j] = pz[q];
    acc[j] = 0ull;
    if (NOUT == 2) acc[m + j] = 0ull;
}

// The particle arrays of a batch: the fp32 structure of arrays (asp_sample3d), or the
// reader's fp64 arrays (asp_sample3d_f64).
struct PPart {
    const float *x, *y, *z, *h, *a0, *a1;
    const double *pos, *h64, *a064, *a164;
};

// What the test and the term need of one particle.  The fp32 working values are those
// asp_project3d sees (the fp64 entry rounds h and a to nearest), and `ok` is the admission
// on them: 2|h| > 0 and finite in fp32, x, y, z finite in fp32.  C, H are the values the
// decision is taken on.
struct PVals {
    double C[3], H;
    float hf, a0, a1;
    bool ok;
};
template <bool F64, int NOUT>
__device__ __forceinline__ PVals pload(const PPart& P, long long p) {
    PVals v;
    if constexpr (F64) {
        v.C[0] = P.pos[3 * p];
        v.C[1] = P.pos[3 * p + 1];
        v.C[2] = P.pos[3 * p + 2];
        v.H = P.h64[p];
        v.hf = (float)v.H;
        v.a0 = (float)P.a064[p];
        v.a1 = NOUT == 2 ? (float)P.a164[p] : 0.0f;
    } else {
        v.C[0] = (double)P.x[p];
        v.C[1] = (double)P.y[p];
        v.C[2] = (double)P.z[p];
        v.hf = P.h[p];
        v.H = (double)v.hf;
        v.a0 = P.a0[p];
        v.a1 = NOUT == 2 ? P.a1[p] : 0.0f;
    }
    const float hd = fabsf(2.0f * v.hf);
    v.ok = hd > 0.0f && __builtin_isfinite(hd) && __builtin_isfinite((float)v.C[0]) &&
           __builtin_isfinite((float)v.C[1]) && __builtin_isfinite((float)v.C[2]);
    return v;
}

// max |c| over the admitted particles, for the fixed-point scale (finite values only).
template <int KID, int NOUT, bool F64>
__global__ __launch_bounds__(kSBlock) void k_p3cmax(const PPart P, long long n,
                                                     SDesc3* __restrict__ D) {
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    float c0 = 0.0f, c1 = 0.0f;
    if (p < n) {
        const PVals v = pload<F64, NOUT>(P, p);
        if (v.ok) {
            const float t0 = fabsf((float)term_coef<KID>(v.a0, v.hf));
            const float t1 = NOUT == 2 ? fabsf((float)term_coef<KID>(v.a1, v.hf)) : 0.0f;
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

__global__ void k_p3scale(SDesc3* D, long long n) {
    for (int j = 0; j < 2; ++j) D->k[j] = fix_exponent(n, __uint_as_float(D->cmax[j]));
}

// The sorted points and their accumulators.
struct PPoints {
    const int* start;          // cell starts, G^3 + 2 entries
    const double *sx, *sy, *sz;
    long long m;
    unsigned long long* acc;
};

// One (particle, point) pair: the cube's test (voxel_pass), and the term if it passes.
struct PRec {
    double X, Y, Z, T2;  // the decision's values; T2 = (2H)(2H)
    float hinv, s0, s1;
};
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void ppair(const PRec& R, const PPoints& S, int j) {
    const double dx = R.X - S.sx[j];
    const double dy = R.Y - S.sy[j];
    const double dz = R.Z - S.sz[j];
    const double r2 = (dx * dx + dy * dy) + dz * dz;  // no contraction: -ffp-contract=off
    if (r2 < R.T2) {
        const float q = __builtin_amdgcn_sqrtf((float)r2) * R.hinv;
        const float w = kernel_shape<KID>(q);
        acc_add<ACC>(&S.acc[j], R.s0 * w);
        if constexpr (NOUT == 2) acc_add<ACC>(&S.acc[S.m + j], R.s1 * w);
    }
}

template <int KID, int NOUT, int ACC, bool F64>
__global__ __launch_bounds__(kSBlock) void k_sample3(const PPart P, long long n,
                                                      const SDesc3* __restrict__ D, int G,
                                                      int wide_cells, int wide_points, int walk,
                                                      int mix, const PPoints S,
                                                      unsigned long long* __restrict__ pairs) {
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int* __restrict__ start = S.start;
    PRec R = {0.0, 0.0, 0.0, 0.0, 0.0f, 0.0f, 0.0f};
    int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1, cz0 = 0, cz1 = -1;
    if (p < n) {
        const PVals v = pload<F64, NOUT>(P, p);
        if (v.ok) {
            // |x - px| < 2|H| (1 + 2^-51) for a passing pair; 2^-40 relative to the operands
            // covers that and the roundings of the two edges below many times over
            const double r = 2.0 * fabs(v.H);
            double lo[3], hi[3];
            bool meets = true;
            for (int d = 0; d < 3; ++d) {
                const double rd = r * (1.0 + 0x1p-40) + fabs(v.C[d]) * 0x1p-40;
                lo[d] = v.C[d] - rd;
                hi[d] = v.C[d] + rd;
                meets = meets && hi[d] >= D->lo[d] && lo[d] <= D->hi[d];
            }
            if (meets) {
                cx0 = scell(lo[0], D->lo[0], D->s[0], G);
                cx1 = scell(hi[0], D->lo[0], D->s[0], G);
                cy0 = scell(lo[1], D->lo[1], D->s[1], G);
                cy1 = scell(hi[1], D->lo[1], D->s[1], G);
                cz0 = scell(lo[2], D->lo[2], D->s[2], G);
                cz1 = scell(hi[2], D->lo[2], D->s[2], G);
                const double t = 2.0 * v.H;
                R.X = v.C[0];
                R.Y = v.C[1];
                R.Z = v.C[2];
                R.T2 = t * t;
                R.hinv = __builtin_amdgcn_rcpf(v.hf);  // value path only
                if constexpr (ACC == kAccFix) {
                    R.s0 = (float)ldexp(term_coef<KID>(v.a0, v.hf), D->k[0]);
                    R.s1 = NOUT == 2 ? (float)ldexp(term_coef<KID>(v.a1, v.hf), D->k[1]) : 0.0f;
                } else {
                    R.s0 = (float)term_coef<KID>(v.a0, v.hf);
                    R.s1 = NOUT == 2 ? (float)term_coef<KID>(v.a1, v.hf) : 0.0f;
                }
            }
        }
    }
    const bool live = cx0 <= cx1;
    const int nrow_y = cy1 - cy0 + 1;
    bool wide = live && (cx1 - cx0 + 1) * nrow_y * (cz1 - cz0 + 1) > wide_cells;
    if (live && !wide) {  // few cells, but crowded ones: the wave takes those as well
        int npts = 0;
        for (int cx = cx0; cx <= cx1; ++cx)
            for (int cy = cy0; cy <= cy1; ++cy) {
                const int base = (cx * G + cy) * G;
                npts += start[base + cz1 + 1] - start[base + cz0];
            }
        wide = npts > wide_points;
    }
    unsigned long long tested = 0ull;
    if (live && !wide) {
        for (int cx = cx0; cx <= cx1; ++cx)
            for (int cy = cy0; cy <= cy1; ++cy) {
                const int base = (cx * G + cy) * G;
                const int a = start[base + cz0], b = start[base + cz1 + 1];
                for (int j = a; j < b; ++j) ppair<KID, NOUT, ACC>(R, S, j);
                tested += (unsigned long long)(b - a);
            }
    }
    // the wave's wide particles, one after the other (every lane of the wave gets here)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        PRec Q;
        Q.X = __shfl(R.X, l);
        Q.Y = __shfl(R.Y, l);
        Q.Z = __shfl(R.Z, l);
        Q.T2 = __shfl(R.T2, l);
        Q.hinv = __shfl(R.hinv, l);
        Q.s0 = __shfl(R.s0, l);
        Q.s1 = __shfl(R.s1, l);
        const int x0 = __shfl(cx0, l), x1 = __shfl(cx1, l), y0 = __shfl(cy0, l), y1 = __shfl(cy1, l);
        const int z0 = __shfl(cz0, l), z1 = __shfl(cz1, l);
        const int ny = y1 - y0 + 1, nrows = (x1 - x0 + 1) * ny;
        if (walk == kWalkRow) {
            for (int cx = x0; cx <= x1; ++cx)
                for (int cy = y0; cy <= y1; ++cy) {
                    const int base = (cx * G + cy) * G;
                    const int a = start[base + z0], b = start[base + z1 + 1];
                    for (int j = a + lane; j < b; j += 64) ppair<KID, NOUT, ACC>(Q, S, j);
                    if (lane == 0) tested += (unsigned long long)(b - a);
                }
            continue;
        }
        for (int rb = 0; rb < nrows; rb += 64) {  // 64 rows: lane i holds row rb + i
            const int row = rb + lane;
            int a = 0, len = 0;
            if (row < nrows) {
                const int ix = row / ny;
                const int base = ((x0 + ix) * G + (y0 + row - ix * ny)) * G;
                a = start[base + z0];
                len = start[base + z1 + 1] - a;
            }
            int inc = len;  // inclusive scan of the lengths over the wave
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            const int excl = inc - len;
            const int total = __shfl(inc, 63);
            // few, long rows: each fills the wave on its own and the search below would be
            // pure overhead -- those chunks are strided row by row (non-empty rows only)
            unsigned long long rows = __builtin_amdgcn_ballot_w64(len > 0);
            if (__builtin_popcountll(rows) <= 1 + (long long)mix * ((total + 63) >> 6)) {
                while (rows) {
                    const int i = __builtin_ctzll(rows);
                    rows &= rows - 1ull;
                    const int ai = __shfl(a, i), bi = ai + __shfl(len, i);
                    for (int j = ai + lane; j < bi; j += 64) ppair<KID, NOUT, ACC>(Q, S, j);
                }
                if (lane == 0) tested += (unsigned long long)total;
                continue;
            }
            for (int t0 = 0; t0 < total; t0 += 64) {
                const int t = t0 + lane;
                // the last row whose offset is <= t; t < total, so that row is not empty
                // and t lies inside it (rows past nrows have offset == total)
                int i = 0;
                for (int s = 32; s > 0; s >>= 1) {
                    const int oc = __shfl(excl, i + s);
                    if (oc <= t) i += s;
                }
                const int ai = __shfl(a, i), ei = __shfl(excl, i);
                if (t < total) ppair<KID, NOUT, ACC>(Q, S, ai + (t - ei));
            }
            if (lane == 0) tested += (unsigned long long)total;
        }
    }
    if (pairs) {
        for (int o = 32; o > 0; o >>= 1)
            tested += (unsigned long long)__shfl_xor((long long)tested, o);
        if (lane == 0 && tested) atomicAdd(pairs, tested);
    }
}

// The arguments of the two entry points (the fp32 or the fp64 particle arrays are set).
struct PointArgs {
    const float *x, *y, *z, *h, *a0, *a1;
    const double *pos, *h64, *a064, *a164;
    long long n;
    const double *px, *py, *pz;
    long long m;
    int kid, flags;
    float *out0, *out1;
};

static int points_check(const PointArgs& A, bool f64) {
    if (A.n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (A.m < 0) return fail(ASP_ERR_INVALID, "m < 0");
    if (A.kid == ASP_KERNEL_CUBIC_SPLINE_COLUMN || A.kid == ASP_KERNEL_WENDLAND_C2_COLUMN)
        return fail(ASP_ERR_INVALID, "the column kernels (ids 3, 4) have no 3-D form");
    if (A.kid < 0 || A.kid > ASP_KERNEL_INDICATOR) return fail(ASP_ERR_INVALID, "unknown kernel_id");
    if (A.flags & ASP_F_DEVICE_OUTPUTS)
        return fail(ASP_ERR_INVALID, "ASP_F_DEVICE_OUTPUTS is not supported by asp_sample3d");
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
    if (A.m > 0 && (!A.px || !A.py || !A.pz)) return fail(ASP_ERR_INVALID, "NULL point coordinates");
    if (A.m > 0 && !A.out0) return fail(ASP_ERR_INVALID, "out0 is NULL");
    if (A.n > 0) {
        const bool null_in = f64 ? (!A.pos || !A.h64 || !A.a064) : (!A.x || !A.y || !A.z || !A.h || !A.a0);
        if (null_in) return fail(ASP_ERR_INVALID, "NULL particle array");
    }
    if (A.m > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "m >= 2^31 points per call");
    return ASP_OK;
}

// Kernel ids 0 .. 2 only (dispatch() would instantiate the column kernels as well).
template <class F>
static int dispatch3(int kid, int nout, bool det, F&& f) {
    auto with_kid = [&](auto K) {
        if (nout == 1) return det ? f(K, Int<1>{}, Int<1>{}) : f(K, Int<1>{}, Int<0>{});
        return det ? f(K, Int<2>{}, Int<1>{}) : f(K, Int<2>{}, Int<0>{});
    };
    return kid == 0 ? with_kid(Int<0>{}) : kid == 1 ? with_kid(Int<1>{}) : with_kid(Int<2>{});
}

template <bool F64>
static int sample3(const PointArgs& A, int device, hipStream_t stream) {
    ASP_TRY(points_check(A, F64));
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
        const double *dpx = A.px, *dpy = A.py, *dpz = A.pz;
        float *d0 = A.out0, *d1 = A.out1;
        const size_t pbytes = (size_t)m * sizeof(double), obytes = (size_t)m * sizeof(float);
        if (!dev) {
            ASP_TRY(to_device(ws, B[kSmpPx], dpx, pbytes, st, Copy::kPlain));
            ASP_TRY(to_device(ws, B[kSmpPy], dpy, pbytes, st, Copy::kPlain));
            ASP_TRY(to_device(ws, B[kSmpPz], dpz, pbytes, st, Copy::kPlain));
            ASP_TRY(device_scratch(B[kSmpOut0], d0, obytes));
            if (A.out1) ASP_TRY(device_scratch(B[kSmpOut1], d1, obytes));
            if (acc_flag) {
                ASP_HIP(hipMemcpyAsync(d0, A.out0, obytes, hipMemcpyHostToDevice, st));
                if (d1) ASP_HIP(hipMemcpyAsync(d1, A.out1, obytes, hipMemcpyHostToDevice, st));
            }
        }
        int G = (int)std::ceil(std::cbrt((double)m / kPerCell3));
        G = (int)env_int("ASP_SAMPLE_CELLS", std::max(1, std::min(kMaxG3, G)), 1, kMaxG3);
        const int wide_cells = (int)env_int("ASP_SAMPLE_WIDE_CELLS", kWideCells3, 0, INT_MAX);
        const int wide_points = (int)env_int("ASP_SAMPLE_WIDE_POINTS", kWidePoints3, 0, INT_MAX);
        const int walk = (int)env_int("ASP_SAMPLE3D_WALK", kWalkFlat, kWalkRow, kWalkFlat);
        const int mix = (int)env_int("ASP_SAMPLE3D_WALK_MIX", kWalkMix, 0, 1 << 20);
        const size_t ncell = (size_t)G * G * G + 1;  // the last: points with a non-finite coordinate
        SDesc3* D = nullptr;
        unsigned *kin = nullptr, *kout = nullptr;
        int *iin = nullptr, *iout = nullptr, *cnt = nullptr, *start = nullptr;
        double* sorted = nullptr;
        unsigned long long* acc = nullptr;
        ASP_TRY(device_scratch(B[kSmpDesc], D, sizeof(SDesc3)));
        ASP_TRY(device_scratch(B[kSmpKeys], kin, (size_t)m * 2 * sizeof(unsigned)));
        ASP_TRY(device_scratch(B[kSmpIndex], iin, (size_t)m * 2 * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpCellCount], cnt, (ncell + 1) * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpCellStart], start, (ncell + 1) * sizeof(int)));
        ASP_TRY(device_scratch(B[kSmpSorted3], sorted, 3 * pbytes));
        ASP_TRY(device_scratch(B[kSmpAcc], acc, (size_t)nout * m * sizeof(unsigned long long)));
        kout = kin + m;
        iout = iin + m;
        const PPoints S{start, sorted, sorted + m, sorted + 2 * m, m, acc};
        const unsigned pgrid = (unsigned)((m + kSBlock - 1) / kSBlock);
        hipLaunchKernelGGL(k_p3init, dim3(1), dim3(1), 0, st, D);
        ASP_LAUNCHED();
        hipLaunchKernelGGL(k_p3bbox, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, dpz, m, D);
        ASP_LAUNCHED();
        hipLaunchKernelGGL(k_p3desc, dim3(1), dim3(1), 0, st, D, G);
        ASP_LAUNCHED();
        ASP_HIP(hipMemsetAsync(cnt, 0, (ncell + 1) * sizeof(int), st));
        hipLaunchKernelGGL(k_p3keys, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, dpz, m,
                           (const SDesc3*)D, G, kin, iin, cnt);
        ASP_LAUNCHED();
        int key_bits = 1;
        while ((1ull << key_bits) <= (unsigned long long)G * G * G) ++key_bits;
        ASP_TRY(sort_pairs(B[kSmpSortTmp], kin, kout, iin, iout, (size_t)m, key_bits, st));
        ASP_TRY(exclusive_scan_int(B[kSmpScanTmp], cnt, start, ncell + 1, st));
        if (nout == 2)
            hipLaunchKernelGGL(k_p3gather<2>, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, dpz, m,
                               (const int*)iout, sorted, sorted + m, sorted + 2 * m, acc);
        else
            hipLaunchKernelGGL(k_p3gather<1>, dim3(pgrid), dim3(kSBlock), 0, st, dpx, dpy, dpz, m,
                               (const int*)iout, sorted, sorted + m, sorted + 2 * m, acc);
        ASP_LAUNCHED();
        mprep.done();

        // ---- the particles, batch by batch, into the same accumulators ----
        auto stage = [&](long long a, long long b, PPart& P) -> int {
            const size_t nb = (size_t)(b - a);
            P = PPart{};
            if constexpr (F64) {
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
                P.x = A.x + a;
                P.y = A.y + a;
                P.z = A.z + a;
                P.h = A.h + a;
                P.a0 = A.a0 + a;
                P.a1 = A.a1 ? A.a1 + a : nullptr;
                if (!dev) {
                    const size_t fb = nb * sizeof(float);
                    ASP_TRY(to_device(ws, B[kSmpPart0], P.x, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart1], P.y, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart2], P.z, fb, st, Copy::kPinned));
                    ASP_TRY(to_device(ws, B[kSmpPart3], P.h, fb, st, Copy::kPinned));
                    // the two amplitude arrays share the last slot (sized for both first)
                    float* both = nullptr;
                    ASP_TRY(device_scratch(B[kSmpPart4], both, 2 * fb));
                    ASP_TRY(to_device(ws, B[kSmpPart4], P.a0, fb, st, Copy::kPinned));
                    if (P.a1) ASP_TRY(to_device(ws, B[kSmpPart4], P.a1, fb, st, Copy::kPinned, fb));
                }
            }
            return ASP_OK;
        };
        if (det) {  // the scale needs max |c| over ALL particles before the first term
            ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
                PPart P;
                ASP_TRY(stage(a, b, P));
                const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
                StageMark mk(ws, kSSampleDeposit, st);
                ASP_TRY(dispatch3(A.kid, nout, false, [&](auto K, auto NO, auto) -> int {
                    hipLaunchKernelGGL((k_p3cmax<decltype(K)::value, decltype(NO)::value, F64>), dim3(grid),
                                       dim3(kSBlock), 0, st, P, b - a, D);
                    ASP_LAUNCHED();
                    return ASP_OK;
                }));
                mk.done();
                return ASP_OK;
            }));
            StageMark mscale(ws, kSSampleDeposit, st);
            hipLaunchKernelGGL(k_p3scale, dim3(1), dim3(1), 0, st, D, n);
            ASP_LAUNCHED();
            mscale.done();
        }
        unsigned long long* pairs = count ? &D->pairs : nullptr;
        ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
            PPart P;
            ASP_TRY(stage(a, b, P));
            const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
            StageMark mk(ws, kSSampleDeposit, st);
            ASP_TRY(dispatch3(A.kid, nout, det, [&](auto K, auto NO, auto AC) -> int {
                hipLaunchKernelGGL((k_sample3<decltype(K)::value, decltype(NO)::value,
                                              decltype(AC)::value, F64>),
                                   dim3(grid), dim3(kSBlock), 0, st, P, b - a, (const SDesc3*)D, G,
                                   wide_cells, wide_points, walk, mix, S, pairs);
                ASP_LAUNCHED();
                return ASP_OK;
            }));
            mk.done();
            return ASP_OK;
        }));

        // ---- finalise ----
        const int kflags = (acc_flag ? kFlagAccumulate : 0) | ((A.flags & ASP_F_RATIO) ? kFlagRatio : 0);
        StageMark mfin(ws, kSSampleDeposit, st);
        ASP_TRY(dispatch3(0, nout, det, [&](auto, auto NO, auto AC) -> int {
            hipLaunchKernelGGL((k_sfinal<decltype(NO)::value, decltype(AC)::value, SDesc3>), dim3(pgrid),
                               dim3(kSBlock), 0, st, (const unsigned long long*)acc, m, (const int*)iout,
                               (const SDesc3*)D, d0, d1, kflags);
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

extern "C" int asp_sample3d(const float* x, const float* y, const float* z, const float* h,
                            const float* a0, const float* a1, int64_t n, const double* px,
                            const double* py, const double* pz, int64_t m, int32_t kernel_id,
                            int32_t flags, float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    PointArgs A{x, y, z, h, a0, a1, nullptr, nullptr, nullptr, nullptr, n, px, py, pz, m,
                kernel_id, flags, out0, out1};
    return sample3<false>(A, device, (hipStream_t)stream);
}

extern "C" int asp_sample3d_f64(const double* positions, const double* h, const double* a0,
                                const double* a1, int64_t n, const double* px, const double* py,
                                const double* pz, int64_t m, int32_t kernel_id, int32_t flags,
                                float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    PointArgs A{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, positions, h, a0, a1, n,
                px, py, pz, m, kernel_id, flags, out0, out1};
    return sample3<true>(A, device, (hipStream_t)stream);
}
