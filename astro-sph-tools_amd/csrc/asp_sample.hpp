// asp_sample.hpp -- the point grid of the 2-D sampler (asp_sample.hip, DIM = 2) and of the
// 3-D sampler (asp_sample3d.hip, DIM = 3), written once: the descriptor and its prep kernels,
// the particle loader, the fixed-point scale passes, a particle's record and cell range, the
// pair test, the finalising pass, the argument checks, the prep and the particle staging of a
// call and the samplers' host driver (asp_spectra.hip has its own, over the same prep).  A unit
// keeps what rests on its own measurements: its deposit kernel's walk
// over the cell range, the grid-size rule, the thresholds and the kernel-id range.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map_device.hpp"
#include "asp_prims.hpp"

namespace asp {

constexpr int kSBlock = 256;

// The grid rule and the class thresholds over 2-D points (measured in DESIGN.md §20), for the
// units that walk them: asp_sample.hip and asp_spectra.hip.
constexpr int kSampleMaxG = 2048;     // cells per axis at most: a 16 MiB cell-start table
constexpr int kSamplePerCell = 4;     // points per cell the grid aims at
constexpr int kSampleWideCells = 16;  // boxes over more cells go to the wave (ASP_SAMPLE_WIDE_CELLS)
constexpr int kSampleWidePoints = 256;  // ... and boxes holding more points (ASP_SAMPLE_WIDE_POINTS)

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

// The grid over the points and the call's device-side scalars.
template <int DIM>
struct SDescT {
    unsigned long long emin[DIM], emax[DIM];  // bounding box, order-preserving encodings (atomics)
    double lo[DIM], hi[DIM];                  // the box decoded (k_sdesc); lo[0] > hi[0]: no finite point
    double s[DIM];                            // cells per unit length, G / (hi - lo) (0: one cell)
    unsigned cmax[2];                         // max |c| over the particles, fp32 bits (fixed point)
    int k[2];                                 // fixed-point scale exponents
    unsigned long long pairs;                 // ASP_SAMPLE_COUNT
};

// The DIM coordinate arrays of the points, in the caller's order.
template <int DIM>
struct Coords {
    const double* c[DIM];
};
template <int DIM>
__device__ __forceinline__ bool load_finite(const Coords<DIM>& X, long long i, double* c) {
    bool fin = true;
    for (int d = 0; d < DIM; ++d) {
        c[d] = X.c[d][i];
        fin = fin && __builtin_isfinite(c[d]);
    }
    return fin;
}

template <int DIM>
__global__ void k_sinit(SDescT<DIM>* D) {
    for (int d = 0; d < DIM; ++d) {
        D->emin[d] = ~0ull;
        D->emax[d] = 0ull;
    }
    D->cmax[0] = D->cmax[1] = 0u;
    D->k[0] = D->k[1] = 0;
    D->pairs = 0ull;
}

// Bounding box of the points whose coordinates are all finite.
template <int DIM>
__global__ __launch_bounds__(kSBlock) void k_sbbox(const Coords<DIM> X, long long m,
                                                    SDescT<DIM>* __restrict__ D) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    unsigned long long lo[DIM], hi[DIM];
    double c[DIM];
    const bool fin = i < m && load_finite(X, i, c);
    for (int d = 0; d < DIM; ++d) {
        lo[d] = fin ? enc_ordered(c[d]) : ~0ull;
        hi[d] = fin ? lo[d] : 0ull;
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = min(lo[d], (unsigned long long)__shfl_xor((long long)lo[d], o));
            hi[d] = max(hi[d], (unsigned long long)__shfl_xor((long long)hi[d], o));
        }
    }
    if ((threadIdx.x & 63) == 0 && hi[0] != 0ull)
        for (int d = 0; d < DIM; ++d) {
            atomicMin(&D->emin[d], lo[d]);
            atomicMax(&D->emax[d], hi[d]);
        }
}

template <int DIM>
__global__ void k_sdesc(SDescT<DIM>* D, int G) {
    for (int d = 0; d < DIM; ++d) {
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

// Cell key of every point -- cx G + cy, or (cx G + cy) G + cz: the cells of one row are one
// contiguous span of sorted points; a non-finite point: G^DIM, the same fold from 1 with
// cells 0 -- its index, and the cell counts.
template <int DIM>
__global__ __launch_bounds__(kSBlock) void k_skeys(const Coords<DIM> X, long long m,
                                                    const SDescT<DIM>* __restrict__ D, int G,
                                                    unsigned* __restrict__ keys,
                                                    int* __restrict__ idx, int* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= m) return;
    double c[DIM];
    const bool fin = load_finite(X, i, c);
    unsigned k = fin ? 0u : 1u;
    for (int d = 0; d < DIM; ++d)
        k = k * (unsigned)G + (fin ? (unsigned)scell(c[d], D->lo[d], D->s[d], G) : 0u);
    keys[i] = k;
    idx[i] = (int)i;
    atomicAdd(&cnt[k], 1);
}

// Coordinates into cell order (axis d at sorted + d m); accumulators zeroed.
template <int DIM, int NOUT>
__global__ __launch_bounds__(kSBlock) void k_sgather(const Coords<DIM> X, long long m,
                                                      const int* __restrict__ perm,
                                                      double* __restrict__ sorted,
                                                      unsigned long long* __restrict__ acc) {
    const long long j = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (j >= m) return;
    const int q = perm[j];
    for (int d = 0; d < DIM; ++d) sorted[d * m + j] = X.c[d][q];
    acc[j] = 0ull;
    if (NOUT == 2) acc[m + j] = 0ull;
}

// The particle arrays of a call or of a batch: the fp32 structure of arrays (asp_sample2d,
// asp_sample3d), or the reader's fp64 arrays (the _f64 entries).  The 2-D fp64 entry reads
// the two position columns of its axis (col); the 3-D one reads all three at 3 p + d.
template <int DIM>
struct PartArrays {
    const float *c[DIM], *h, *a0, *a1;
    const double *pos, *h64, *a064, *a164;
};
template <int DIM>
struct Part : PartArrays<DIM> {};
template <>
struct Part<2> : PartArrays<2> {
    int col[2];
};

// What the test and the term need of one particle.  The fp32 working values are those
// asp_project2d(_f64) / asp_project3d see (the fp64 entries round h and a to nearest, as
// their staging does), and `ok` is footprint()'s admission on them: 2|h| > 0 and finite in
// fp32, every coordinate finite in fp32.  C, H are the values the decision is taken on.
template <int DIM>
struct SVals {
    double C[DIM], H;
    float hf, a0, a1;
    bool ok;
};
template <int DIM, bool F64, int NOUT>
__device__ __forceinline__ SVals<DIM> sload(const Part<DIM>& P, long long p) {
    SVals<DIM> x;
    if constexpr (F64) {
        for (int d = 0; d < DIM; ++d) {
            if constexpr (DIM == 2) x.C[d] = P.pos[3 * p + P.col[d]];
            else x.C[d] = P.pos[3 * p + d];
        }
        x.H = P.h64[p];
        x.hf = (float)x.H;
        x.a0 = (float)P.a064[p];
        x.a1 = NOUT == 2 ? (float)P.a164[p] : 0.0f;
    } else {
        for (int d = 0; d < DIM; ++d) x.C[d] = (double)P.c[d][p];
        x.hf = P.h[p];
        x.H = (double)x.hf;
        x.a0 = P.a0[p];
        x.a1 = NOUT == 2 ? P.a1[p] : 0.0f;
    }
    const float hd = fabsf(2.0f * x.hf);
    x.ok = hd > 0.0f && __builtin_isfinite(hd);
    for (int d = 0; d < DIM; ++d) x.ok = x.ok && __builtin_isfinite((float)x.C[d]);
    return x;
}

// max |c| over the admitted particles, for the fixed-point scale (finite values only).
template <int DIM, int KID, int NOUT, bool F64>
__global__ __launch_bounds__(kSBlock) void k_scmax(const Part<DIM> P, long long n,
                                                    SDescT<DIM>* __restrict__ D) {
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    float c0 = 0.0f, c1 = 0.0f;
    if (p < n) {
        const SVals<DIM> x = sload<DIM, F64, NOUT>(P, p);
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

// The fixed-point exponents from n and max |c|.
template <int DIM>
__global__ void k_sscale(SDescT<DIM>* D, long long n) {
    for (int j = 0; j < 2; ++j) D->k[j] = fix_exponent(n, __uint_as_float(D->cmax[j]));
}

// The sorted points and their accumulators.
template <int DIM>
struct Points {
    const int* start;    // cell starts, G^DIM + 2 entries
    const double* s[DIM];  // coordinates in cell order
    long long m;
    unsigned long long* acc;
};

// One particle as the pair test needs it, and the cells its box meets.
template <int DIM>
struct Rec {
    double C[DIM], T2;  // the decision's values; T2 = (2H)(2H)
    float hinv, s0, s1;
};
struct Span {
    int lo, hi;  // cells lo .. hi of one axis
};
template <int DIM>
struct Particle {
    Span c[DIM];  // c[0].lo > c[0].hi: nothing to visit
    Rec<DIM> R;
};

// A particle's box against the bounding box of the finite points (none: lo > hi, no box meets).
template <int DIM>
__device__ __forceinline__ bool box_meets(const double* lo, const double* hi, const SDescT<DIM>* D) {
    for (int d = 0; d < DIM; ++d)
        if (!(hi[d] >= D->lo[d] && lo[d] <= D->hi[d])) return false;
    return true;
}

// Particle p's record and cell range: its box C +- 2|H|, widened by 2^-40 relative (far
// above the fp64 roundings of the test), through the points' own cell expression -- a
// superset of the cells of every point that can pass.  A particle that is not admitted, or
// whose box misses the points' bounding box, gets the empty range.
template <int DIM, int KID, int NOUT, int ACC, bool F64>
__device__ __forceinline__ Particle<DIM> particle_record(const Part<DIM>& P, long long p, long long n,
                                                         const SDescT<DIM>* D, int G) {
    Particle<DIM> A = {};
    Rec<DIM>& R = A.R;
    for (int d = 0; d < DIM; ++d) A.c[d].hi = -1;
    if (p < n) {
        const SVals<DIM> x = sload<DIM, F64, NOUT>(P, p);
        if (x.ok) {
            // |u - px| < 2|H| (1 + 2^-51) for a passing pair; 2^-40 relative to the operands
            // covers that and the roundings of the two edges below many times over
            const double r = 2.0 * fabs(x.H);
            double lo[DIM], hi[DIM];
            for (int d = 0; d < DIM; ++d) {
                const double rd = r * (1.0 + 0x1p-40) + fabs(x.C[d]) * 0x1p-40;
                lo[d] = x.C[d] - rd;
                hi[d] = x.C[d] + rd;
            }
            if (box_meets(lo, hi, D)) {
                // (axis by axis in straight-line code: as a loop, scell's (double)(G - 1) is
                // hoisted before the unrolling and k_sample needs one SGPR more)
                auto cells = [&](int d) {
                    A.c[d].lo = scell(lo[d], D->lo[d], D->s[d], G);
                    A.c[d].hi = scell(hi[d], D->lo[d], D->s[d], G);
                    R.C[d] = x.C[d];
                };
                cells(0);
                cells(1);
                if constexpr (DIM == 3) cells(2);
                const double t = 2.0 * x.H;
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
    return A;
}

// Lane l's record and cell range, for the whole wave.
template <int DIM>
__device__ __forceinline__ Rec<DIM> from_lane(const Rec<DIM>& R, int l) {
    Rec<DIM> Q;
    for (int d = 0; d < DIM; ++d) Q.C[d] = __shfl(R.C[d], l);
    Q.T2 = __shfl(R.T2, l);
    Q.hinv = __shfl(R.hinv, l);
    Q.s0 = __shfl(R.s0, l);
    Q.s1 = __shfl(R.s1, l);
    return Q;
}
__device__ __forceinline__ Span from_lane(const Span& c, int l) {
    return {__shfl(c.lo, l), __shfl(c.hi, l)};
}

// One (particle, point) pair: the reference's test (.pyx:20-31; the cube's voxel_pass), and
// the term if it passes.  r2 is summed left to right, dx dx + dy dy (+ dz dz), without
// contraction (-ffp-contract=off).
template <int DIM, int KID>
__device__ __forceinline__ bool pair_shape(const Rec<DIM>& R, const Points<DIM>& S, int j, float& w) {
    double dd[DIM];
    for (int d = 0; d < DIM; ++d) dd[d] = R.C[d] - S.s[d][j];
    double r2 = dd[0] * dd[0];
    for (int d = 1; d < DIM; ++d) r2 = r2 + dd[d] * dd[d];
    if (!(r2 < R.T2)) return false;
    const float q = __builtin_amdgcn_sqrtf((float)r2) * R.hinv;
    w = kernel_shape<KID>(q);
    return true;
}
// ... its terms s w added to the point's accumulators (the samplers' deposit).
template <int DIM, int KID, int NOUT, int ACC>
__device__ __forceinline__ void pair(const Rec<DIM>& R, const Points<DIM>& S, int j) {
    float w;
    if (pair_shape<DIM, KID>(R, S, j, w)) {
        acc_add<ACC>(&S.acc[j], R.s0 * w);
        if constexpr (NOUT == 2) acc_add<ACC>(&S.acc[S.m + j], R.s1 * w);
    }
}

// The end of a deposit kernel: the wave's pairs tested into the call's counter
// (ASP_SAMPLE_COUNT; pairs is NULL without it).
__device__ __forceinline__ void count_pairs(unsigned long long tested, int lane, unsigned long long* pairs) {
    if (pairs) {
        for (int o = 32; o > 0; o >>= 1)
            tested += (unsigned long long)__shfl_xor((long long)tested, o);
        if (lane == 0 && tested) atomicAdd(pairs, tested);
    }
}

// Accumulators (cell order) -> fp32 outputs in the caller's order: emit_pixel, the map's
// conversion, accumulate and ratio.
template <int DIM, int NOUT, int ACC>
__global__ __launch_bounds__(kSBlock) void k_sfinal(const unsigned long long* __restrict__ acc,
                                                     long long m, const int* __restrict__ perm,
                                                     const SDescT<DIM>* __restrict__ D,
                                                     float* __restrict__ out0,
                                                     float* __restrict__ out1, int flags) {
    const long long j = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (j >= m) return;
    emit_pixel<NOUT, ACC>((long long)perm[j], acc[j], NOUT == 2 ? acc[m + j] : 0ull, D->k[0],
                          D->k[1], out0, out1, flags);
}

// ---- host side ----

// The arguments of an entry point (the fp32 or the fp64 particle arrays are set).
template <int DIM>
struct SampleArgs {
    PartArrays<DIM> src;
    int axis;  // asp_sample2d_f64 only
    long long n;
    Coords<DIM> pt;
    long long m;
    int kid, flags;
    float *out0, *out1;
};

// TR, a unit's traits: name (the fp32 entry point's, for messages), check_kernel(kid),
// cells(m) (G from m) and kMaxG, Knobs / knobs() (the unit's environment knobs, read once per
// call), dispatch(kid, nout, det, f) over the unit's kernel ids, and
// deposit<F64>(kid, nout, det, grid, st, P, nb, D, G, knobs, S, pairs), which launches the
// unit's deposit kernel for one batch.
template <int DIM, class TR>
int sample_check(const SampleArgs<DIM>& A, bool f64) {
    const PartArrays<DIM>& X = A.src;
    if (A.n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (A.m < 0) return fail(ASP_ERR_INVALID, "m < 0");
    ASP_TRY(TR::check_kernel(A.kid));
    if (DIM == 2 && f64 && (A.axis < 0 || A.axis > 2))
        return fail(ASP_ERR_INVALID, "projection axis must be 0 (X), 1 (Y) or 2 (Z); "
                                     "ASP_AXIS_CULL has no meaning without a chunk cull");
    if (A.flags & ASP_F_DEVICE_OUTPUTS)
        return fail(ASP_ERR_INVALID, std::string("ASP_F_DEVICE_OUTPUTS is not supported by ") + TR::name);
    const bool has_a1 = f64 ? X.a164 != nullptr : X.a1 != nullptr;
    if (has_a1 != (A.out1 != nullptr))
        return fail(ASP_ERR_INVALID, "a1 and out1 must both be given or both be NULL");
    if ((A.flags & ASP_F_RATIO) && !A.out1) return fail(ASP_ERR_INVALID, "ASP_F_RATIO needs out1");
    if ((A.flags & ASP_F_RATIO) && (A.flags & ASP_F_ACCUMULATE))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_ACCUMULATE");
    if ((A.flags & ASP_F_RATIO) && (A.flags & ASP_F_DETERMINISTIC))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_DETERMINISTIC "
                                     "(fixed-point components carry no relative precision in "
                                     "kernel-tail points; form ratios from fp64 sums)");
    bool null_pt = false, null_in = f64 ? (!X.pos || !X.h64 || !X.a064) : (!X.h || !X.a0);
    for (int d = 0; d < DIM; ++d) {
        null_pt = null_pt || !A.pt.c[d];
        null_in = null_in || (!f64 && !X.c[d]);
    }
    if (A.m > 0 && null_pt) return fail(ASP_ERR_INVALID, "NULL point coordinates");
    if (A.m > 0 && !A.out0) return fail(ASP_ERR_INVALID, "out0 is NULL");
    if (A.n > 0 && null_in) return fail(ASP_ERR_INVALID, "NULL particle array");
    if (A.m > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "m >= 2^31 points per call");
    return ASP_OK;
}

// The particle arrays [a, b) of a call as the deposit kernel reads them: the caller's device
// arrays, or a host caller's batch staged through the kSmpPart slots -- the fp64 arrays one
// slot each; the fp32 coordinates, then h, then both amplitudes sharing the last.
template <int DIM, bool F64>
int stage_batch(Workspace& ws, const SampleArgs<DIM>& A, long long a, long long b, hipStream_t st,
                Part<DIM>& P) {
    const bool dev = A.flags & ASP_F_DEVICE_PTRS;
    Buf* B = ws.sample;
    const size_t nb = (size_t)(b - a);
    P = Part<DIM>{};
    if constexpr (F64) {
        if constexpr (DIM == 2) {
            const int cols[3][2] = {{1, 2}, {0, 2}, {0, 1}};  // _projector.py:38-46
            P.col[0] = cols[A.axis][0];
            P.col[1] = cols[A.axis][1];
        }
        P.pos = A.src.pos + 3 * a;
        P.h64 = A.src.h64 + a;
        P.a064 = A.src.a064 + a;
        P.a164 = A.src.a164 ? A.src.a164 + a : nullptr;
        const double** arr[4] = {&P.pos, &P.h64, &P.a064, &P.a164};
        for (int i = 0; i < 4; ++i)
            if (!dev && *arr[i])
                ASP_TRY(to_device(ws, B[kSmpPart0 + i], *arr[i], nb * (i ? 1 : 3) * sizeof(double),
                                  st, Copy::kPinned));
    } else {
        const float** arr[DIM + 3];  // array i goes to slot min(i, DIM + 1), a1 behind a0
        for (int d = 0; d < DIM; ++d) {
            P.c[d] = A.src.c[d] + a;
            arr[d] = &P.c[d];
        }
        P.h = A.src.h + a;
        P.a0 = A.src.a0 + a;
        P.a1 = A.src.a1 ? A.src.a1 + a : nullptr;
        arr[DIM] = &P.h;
        arr[DIM + 1] = &P.a0;
        arr[DIM + 2] = &P.a1;
        const size_t fb = nb * sizeof(float);
        float* both = nullptr;  // the last slot is sized for both amplitudes first
        if (!dev) ASP_TRY(device_scratch(B[kSmpPart0 + DIM + 1], both, 2 * fb));
        for (int i = 0; i < DIM + 3; ++i)
            if (!dev && *arr[i])
                ASP_TRY(to_device(ws, B[kSmpPart0 + std::min(i, DIM + 1)], *arr[i], fb, st,
                                  Copy::kPinned, i == DIM + 2 ? fb : 0));
    }
    return ASP_OK;
}

// What the prep leaves for the deposit and the finalising pass: the descriptor, the cells per
// axis, the sorted points and their accumulators, the permutation (cell order -> the caller's
// order), the grid of a pass over the points and the device outputs.
template <int DIM>
struct SGrid {
    SDescT<DIM>* D;
    int G;
    Points<DIM> S;
    const int* perm;
    unsigned pgrid;
    float *d0, *d1;
};

// The prep of a call (stage sample_prep): the points on the device, keyed, sorted, their cells
// scanned; `width` accumulators per point and sum (the samplers: 1, zeroed here; a unit with
// more zeroes them itself) and as many output values.
template <int DIM, class TR>
int sample_prep(Workspace& ws, hipStream_t st, const SampleArgs<DIM>& A, size_t width, SGrid<DIM>& g) {
    using Desc = SDescT<DIM>;
    const bool dev = A.flags & ASP_F_DEVICE_PTRS;
    const bool acc_flag = A.flags & ASP_F_ACCUMULATE;
    const int nout = A.out1 ? 2 : 1;
    const long long m = A.m;
    const size_t pbytes = (size_t)m * sizeof(double), obytes = (size_t)m * width * sizeof(float);
    Buf* B = ws.sample;
    StageMark mprep(ws, kSSamplePrep, st);
    Coords<DIM> X = A.pt;
    float *d0 = A.out0, *d1 = A.out1;
    if (!dev) {
        const int slot[3] = {kSmpPx, kSmpPy, kSmpPz};
        for (int d = 0; d < DIM; ++d)
            ASP_TRY(to_device(ws, B[slot[d]], X.c[d], pbytes, st, Copy::kPlain));
        ASP_TRY(device_scratch(B[kSmpOut0], d0, obytes));
        if (A.out1) ASP_TRY(device_scratch(B[kSmpOut1], d1, obytes));
        if (acc_flag) {
            ASP_HIP(hipMemcpyAsync(d0, A.out0, obytes, hipMemcpyHostToDevice, st));
            if (d1) ASP_HIP(hipMemcpyAsync(d1, A.out1, obytes, hipMemcpyHostToDevice, st));
        }
    }
    const int G = (int)env_int("ASP_SAMPLE_CELLS", std::max(1, std::min(TR::kMaxG, TR::cells(m))), 1,
                               TR::kMaxG);
    size_t ncell = 1;  // G^DIM cells and one more: points with a non-finite coordinate
    for (int d = 0; d < DIM; ++d) ncell *= (size_t)G;
    int key_bits = 1;
    while ((1ull << key_bits) <= ncell) ++key_bits;
    ++ncell;
    Desc* D = nullptr;
    unsigned* kin = nullptr;
    int *iin = nullptr, *cnt = nullptr, *start = nullptr;
    double* sorted = nullptr;
    unsigned long long* acc = nullptr;
    ASP_TRY(device_scratch(B[kSmpDesc], D, sizeof(Desc)));
    ASP_TRY(device_scratch(B[kSmpKeys], kin, (size_t)m * 2 * sizeof(unsigned)));
    ASP_TRY(device_scratch(B[kSmpIndex], iin, (size_t)m * 2 * sizeof(int)));
    ASP_TRY(device_scratch(B[kSmpCellCount], cnt, (ncell + 1) * sizeof(int)));
    ASP_TRY(device_scratch(B[kSmpCellStart], start, (ncell + 1) * sizeof(int)));
    ASP_TRY(device_scratch(B[kSmpSorted], sorted, DIM * pbytes));
    ASP_TRY(device_scratch(B[kSmpAcc], acc, (size_t)nout * m * width * sizeof(unsigned long long)));
    unsigned* kout = kin + m;
    const int* iout = iin + m;
    Points<DIM> S{start, {}, m, acc};
    for (int d = 0; d < DIM; ++d) S.s[d] = sorted + d * m;
    const unsigned pgrid = (unsigned)((m + kSBlock - 1) / kSBlock);
    hipLaunchKernelGGL(k_sinit<DIM>, dim3(1), dim3(1), 0, st, D);
    ASP_LAUNCHED();
    hipLaunchKernelGGL(k_sbbox<DIM>, dim3(pgrid), dim3(kSBlock), 0, st, X, m, D);
    ASP_LAUNCHED();
    hipLaunchKernelGGL(k_sdesc<DIM>, dim3(1), dim3(1), 0, st, D, G);
    ASP_LAUNCHED();
    ASP_HIP(hipMemsetAsync(cnt, 0, (ncell + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_skeys<DIM>, dim3(pgrid), dim3(kSBlock), 0, st, X, m, (const Desc*)D, G, kin,
                       iin, cnt);
    ASP_LAUNCHED();
    ASP_TRY(sort_pairs(B[kSmpSortTmp], kin, kout, iin, iin + m, (size_t)m, key_bits, st));
    ASP_TRY(exclusive_scan_int(B[kSmpScanTmp], cnt, start, ncell + 1, st));
    hipLaunchKernelGGL((nout == 2 ? k_sgather<DIM, 2> : k_sgather<DIM, 1>), dim3(pgrid), dim3(kSBlock),
                       0, st, X, m, iout, sorted, acc);
    ASP_LAUNCHED();
    mprep.done();
    g = SGrid<DIM>{D, G, S, iout, pgrid, d0, d1};
    return ASP_OK;
}

// One call: the points staged, keyed and sorted (stage sample_prep); the particles, batch by
// batch, through the unit's deposit kernel into the points' accumulators (stage
// sample_deposit); the accumulators converted and written in the caller's order.
template <int DIM, bool F64, class TR>
int sample_driver(const SampleArgs<DIM>& A, int device, hipStream_t stream) {
    using Desc = SDescT<DIM>;
    ASP_TRY((sample_check<DIM, TR>(A, F64)));
    if (A.m == 0) return ASP_OK;
    const bool dev = A.flags & ASP_F_DEVICE_PTRS;
    const bool acc_flag = A.flags & ASP_F_ACCUMULATE;
    const int nout = A.out1 ? 2 : 1;
    const long long m = A.m, n = A.n;
    const size_t obytes = (size_t)m * sizeof(float);
    if (n == 0 && (acc_flag || !dev)) {  // nothing to add; host outputs need no device
        if (!acc_flag) {
            memset(A.out0, 0, obytes);
            if (A.out1) memset(A.out1, 0, obytes);
        }
        return ASP_OK;
    }
    return with_workspace(device, stream, false, [&](Workspace& ws, hipStream_t st) -> int {
        if (ws.prof) ASP_TRY(prof_next(ws));
        stats_clear(ws);
        if (n == 0) {  // device outputs, no particles
            ASP_HIP(hipMemsetAsync(A.out0, 0, obytes, st));
            if (A.out1) ASP_HIP(hipMemsetAsync(A.out1, 0, obytes, st));
            stats_publish(ws, device);
            return ASP_OK;
        }
        const bool det = A.flags & ASP_F_DETERMINISTIC;
        const bool count = env_set("ASP_SAMPLE_COUNT");

        // ---- prep: the points on the device, keyed, sorted, their cells scanned ----
        SGrid<DIM> g;
        ASP_TRY((sample_prep<DIM, TR>(ws, st, A, 1, g)));
        Desc* const D = g.D;
        const int G = g.G;
        const Points<DIM>& S = g.S;
        const typename TR::Knobs knobs = TR::knobs();

        // ---- the particles, batch by batch, into the same accumulators ----
        auto stage = [&](long long a, long long b, Part<DIM>& P) -> int {
            return stage_batch<DIM, F64>(ws, A, a, b, st, P);
        };
        if (det) {  // the scale needs max |c| over ALL particles before the first term
            ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
                Part<DIM> P;
                ASP_TRY(stage(a, b, P));
                const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
                StageMark mk(ws, kSSampleDeposit, st);
                ASP_TRY(TR::dispatch(A.kid, nout, false, [&](auto K, auto NO, auto) -> int {
                    hipLaunchKernelGGL((k_scmax<DIM, decltype(K)::value, decltype(NO)::value, F64>),
                                       dim3(grid), dim3(kSBlock), 0, st, P, b - a, D);
                    ASP_LAUNCHED();
                    return ASP_OK;
                }));
                mk.done();
                return ASP_OK;
            }));
            StageMark mscale(ws, kSSampleDeposit, st);
            hipLaunchKernelGGL(k_sscale<DIM>, dim3(1), dim3(1), 0, st, D, n);
            ASP_LAUNCHED();
            mscale.done();
        }
        unsigned long long* pairs = count ? &D->pairs : nullptr;
        ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
            Part<DIM> P;
            ASP_TRY(stage(a, b, P));
            const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
            StageMark mk(ws, kSSampleDeposit, st);
            ASP_TRY(TR::template deposit<F64>(A.kid, nout, det, grid, st, P, b - a, (const Desc*)D, G, knobs,
                                              S, pairs));
            mk.done();
            return ASP_OK;
        }));

        // ---- finalise ----
        const int kflags = (acc_flag ? kFlagAccumulate : 0) | ((A.flags & ASP_F_RATIO) ? kFlagRatio : 0);
        StageMark mfin(ws, kSSampleDeposit, st);
        ASP_TRY(TR::dispatch(0, nout, det, [&](auto, auto NO, auto AC) -> int {
            hipLaunchKernelGGL((k_sfinal<DIM, decltype(NO)::value, decltype(AC)::value>), dim3(g.pgrid),
                               dim3(kSBlock), 0, st, (const unsigned long long*)S.acc, m, g.perm,
                               (const Desc*)D, g.d0, g.d1, kflags);
            ASP_LAUNCHED();
            return ASP_OK;
        }));
        mfin.done();
        if (!dev) {
            ASP_TRY(to_host(A.out0, g.d0, obytes, st));
            if (A.out1) ASP_TRY(to_host(A.out1, g.d1, obytes, st));
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
