// asp_map_device.hpp -- device code that more than one kernel group of the 2-D map uses
// (asp_map_bin.hip, asp_map_deposit.hip, asp_pairs.hip): the clipped tile boxes, the
// prepared record, the tile prologue and pixel write-out, the packed-fp32 kernel shape.
// Only __device__ functions and constants; no host code.
#pragma once

#include <hip/hip_runtime.h>

#include "asp_device.hpp"

namespace asp {

// A record's candidate box clipped to tile (tx, ty), tile-local, one byte per bound:
// x0 | x1 << 8 | y0 << 16 | y1 << 24.
__device__ __forceinline__ unsigned tile_box(const Box& b, int tx, int ty) {
    int X0 = tx * kTile, Y0 = ty * kTile;
    unsigned x0 = max(b.x0, X0) - X0, x1 = min(b.x1, X0 + kTile - 1) - X0;
    unsigned y0 = max(b.y0, Y0) - Y0, y1 = min(b.y1, Y0 + kTile - 1) - Y0;
    return x0 | (x1 << 8) | (y0 << 16) | (y1 << 24);
}

__device__ __forceinline__ bool box_large(unsigned bp, const Grid& g) {
    int bw = (int)((bp >> 8) & 255u) - (int)(bp & 255u) + 1;
    int bh = (int)(bp >> 24) - (int)((bp >> 16) & 255u) + 1;
    return (bw >= g.gather_min && bh >= g.gather_min) || bw * bh >= g.gather_area;
}

// LDS tile: NOUT maps of 64 rows x kRow words (fp64 or int64), pixel (lx, ly) of the tile
// at word lx * kRow + ly.
__device__ __forceinline__ int pix(int lx, int ly) { return lx * kRow + ly; }

__device__ __forceinline__ Prep bcast_prep(const Prep& P, int l) {
    Prep Q;
    Q.u = bcast(P.u, l);
    Q.v = bcast(P.v, l);
    Q.h = bcast(P.h, l);
    Q.lo = bcast(P.lo, l);
    Q.hi = bcast(P.hi, l);
    Q.hinv = bcast(P.hinv, l);
    Q.s0 = bcast(P.s0, l);
    Q.s1 = bcast(P.s1, l);
    Q.thr = bcast(P.thr, l);
    Q.band = bcast(P.band, l);
    Q.p = bcast(P.p, l);
    Q.b.x0 = bcast(P.b.x0, l);
    Q.b.x1 = bcast(P.b.x1, l);
    Q.b.y0 = bcast(P.b.y0, l);
    Q.b.y1 = bcast(P.b.y1, l);
    return Q;
}

__device__ __forceinline__ bool clip(Box& b, int X0, int Y0, int TW, int TH) {
    b.x0 = max(b.x0, X0);
    b.x1 = min(b.x1, X0 + TW - 1);
    b.y0 = max(b.y0, Y0);
    b.y1 = min(b.y1, Y0 + TH - 1);
    return b.x0 <= b.x1 && b.y0 <= b.y1;
}

// A prepared record {u, v, h, c0}, {c1, p, band, box} -> the pair loop's state.  Only
// (2h)^2 and 1/h are recomputed (the same fp32 operations as the scatter's), and in
// fixed-point mode the tile's power-of-two scale applied (ldexp: exact).
template <int ACC>
__device__ __forceinline__ void rec_prep(const float4& r0, const float4& r1, int X0, int Y0,
                                         int2 kk, Prep& P) {
    P.u = r0.x;
    P.v = r0.y;
    P.h = r0.z;
    P.p = __float_as_int(r1.y);
    set_band(P, rec_thr(r0.z), r1.z);
    P.hinv = __builtin_amdgcn_rcpf(r0.z);
    if constexpr (ACC == kAccFix) {
        P.s0 = ldexpf(r0.w, kk.x);
        P.s1 = ldexpf(r1.x, kk.y);
    } else {
        P.s0 = r0.w;
        P.s1 = r1.x;
    }
    unsigned bp = __float_as_uint(r1.w);
    P.b.x0 = X0 + (int)(bp & 255u);
    P.b.x1 = X0 + (int)((bp >> 8) & 255u);
    P.b.y0 = Y0 + (int)((bp >> 16) & 255u);
    P.b.y1 = Y0 + (int)(bp >> 24);
}

__device__ __forceinline__ void load_rec(const float4* recs, long long i, float4& r0, float4& r1) {
    r0 = recs[2 * i];
    r1 = recs[2 * i + 1];
}

// asp_project2d_props, pass 1 / 2: the record's coefficients of properties (2, 3) / (4, 5)
// replace those of (0, 1) (EXT kernels; the binning, band and box are the record's own).
__device__ __forceinline__ void ext_coef(Prep& P, const float4& e, int pass) {
    P.s0 = pass == 1 ? e.x : e.z;
    P.s1 = pass == 1 ? e.y : e.w;
}

constexpr int kTilePix = kTile * kTile;
constexpr int kFlagAccumulate = 1;
constexpr int kFlagRatio = 2;  // fused ratio: out0 <- map0 / map1

// Corner offset tables: xt[k] = fl32(k * pitch_x), yt[k] = fl32(k * pitch_y) for k < 64 --
// the corner k pixels from a record's box origin, in the frame of the record's (u, v)
// (fl32 of the exact offset from the box origin's corner; the error budget is DESIGN.md
// §3's).  The gathers use them from the tile origin.
__device__ __forceinline__ void corner_tables(const Grid& g, int X0, int Y0, float* xt,
                                              float* yt) {
    (void)X0;
    (void)Y0;
    if (threadIdx.x < kTile)
        xt[threadIdx.x] = (float)((double)threadIdx.x * g.psx);
    else if (threadIdx.x < 2 * kTile)
        yt[threadIdx.x - kTile] = (float)((double)(threadIdx.x - kTile) * g.psy_pix);
}

// Tile prologue: zero accumulators, corner tables.
template <int NOUT, int NT>
__device__ __forceinline__ void tile_prologue(const Grid& g, int X0, int Y0,
                                              unsigned long long* acc, float* xt, float* yt) {
    for (int i = threadIdx.x; i < NOUT * kTileWords; i += NT) acc[i] = 0ull;
    corner_tables(g, X0, Y0, xt, yt);
    __syncthreads();
}

// Convert a pixel's sums and write it (plain store: the tile has one owner).
template <int NOUT, int ACC>
__device__ __forceinline__ void emit_pixel(long long o, unsigned long long s0,
                                           unsigned long long s1, int k0, int k1, float* out0,
                                           float* out1, int flags) {
    float v0 = acc_value<ACC>(s0, k0);
    float v1 = NOUT == 2 ? acc_value<ACC>(s1, k1) : 0.0f;
    if (flags & kFlagAccumulate) {
        v0 += out0[o];
        if (NOUT == 2) v1 += out1[o];
    }
    if (NOUT == 2) {
        out1[o] = v1;
        out0[o] = (flags & kFlagRatio) ? (v1 != 0.0f ? v0 / v1 : 0.0f) : v0;
    } else {
        out0[o] = v0;
    }
}

// Power-of-two scale exponent so that n * cmax * 2^k <= 2^kScaleBits.
__device__ __forceinline__ int scale_exp(long long n, float cmax) {
    if (!(cmax > 0.0f) || n <= 0 || !__builtin_isfinite(cmax)) return 0;
    int e;
    frexp((double)n * (double)cmax, &e);  // n*cmax < 2^e
    return kScaleBits - e;
}

typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2v fma2(f2v a, f2v b, f2v c) {  // v_pk_fma_f32
    return __builtin_elementwise_fma(a, b, c);
}

// Kernel shape on two pairs at once (packed fp32).  Only pairs with fp32 r2 < (2h)^2 use
// the result, so q < 2 up to rounding and the Wendland clamp is not needed there (a q a
// few ulp over 2 gives a term ~1e-28 of the peak).
template <int KID>
__device__ __forceinline__ f2v kernel_shape2(f2v q) {
    if constexpr (kColumn<KID>) {  // (the clamp keeps the table index in range for any q)
        const f2v qh = pk_half_clamp(q);
        const f2v t = f2v{1.0f, 1.0f} - qh;
        return column_shape2<KID>(qh, t, t * t);
    } else if constexpr (KID == 0) {
        f2v q2 = q * q;
        f2v a = fma2(q2, fma2(q, f2v{0.75f, 0.75f}, f2v{-1.5f, -1.5f}), f2v{1.0f, 1.0f});
        f2v t = f2v{2.0f, 2.0f} - q;
        f2v b = (t * t) * (t * 0.25f);
        return f2v{q.x < 1.0f ? a.x : b.x, q.y < 1.0f ? a.y : b.y};
    } else if constexpr (KID == 1) {
        f2v t = fma2(q, f2v{-0.5f, -0.5f}, f2v{1.0f, 1.0f});
        f2v t2 = t * t;
        return (t2 * t2) * fma2(q, f2v{2.0f, 2.0f}, f2v{1.0f, 1.0f});
    } else {
        return f2v{1.0f, 1.0f};
    }
}

__device__ __forceinline__ f2v sqrt2(f2v x) {
    return f2v{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
}

}  // namespace asp
