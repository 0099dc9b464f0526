// asp_map_deposit.hip -- the deposit kernels of the 2-D map and their launchers: K4
// deposit, K4g gather, K5 merge, K6 wide, K7 ratio and the ASP_COUNT_EVALS diagnostic (the
// pipeline's overview is in asp_project2d.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map.hpp"
#include "asp_map_device.hpp"
#include "asp_wave.hpp"

namespace asp {

// ----------------------------------------------------------------------------------
// Deposit building blocks (the LDS tile, the prepared record, the tile prologue and
// emit_pixel: asp_map_device.hpp).
// ----------------------------------------------------------------------------------
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void accumulate(const Prep& P, float r2, unsigned long long* acc0,
                                           unsigned long long* acc1, int k) {
    float q = __builtin_amdgcn_sqrtf(r2) * P.hinv;  // v_sqrt_f32, 1 ulp
    float w = kernel_shape<KID>(q);
    acc_add<ACC>(&acc0[k], P.s0 * w);
    if constexpr (NOUT == 2) acc_add<ACC>(&acc1[k], P.s1 * w);
}

// One wave sweeps the (clipped) box of one wave-uniform record: lanes along y (the
// contiguous image axis), so the LDS atomics of a wave hit distinct consecutive words.
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void sweep(const Grid& g, const Src64& s, const Prep& P, int X0, int Y0,
                                      const float* xt, const float* yt,
                                      unsigned long long* acc0, unsigned long long* acc1,
                                      int lane) {
    int bh = P.b.y1 - P.b.y0 + 1;
    if (bh <= 64) {
        int rps = 64 / bh;
        int r = lane / bh, c = lane - r * bh;
        if (r < rps) {
            int yi = P.b.y0 + c;
            float Y = yt[c];
            for (int xi = P.b.x0 + r; xi <= P.b.x1; xi += rps) {
                float r2;
                if (decide(g, s, P, xi, yi, xt[xi - P.b.x0], Y, r2))
                    accumulate<KID, NOUT, ACC>(P, r2, acc0, acc1, pix(xi - X0, yi - Y0));
            }
        }
    } else {
        for (int xi = P.b.x0; xi <= P.b.x1; ++xi) {
            float X = xt[xi - P.b.x0];
            for (int c = lane; c < bh; c += 64) {
                int yi = P.b.y0 + c;
                float r2;
                if (decide(g, s, P, xi, yi, X, yt[c], r2))
                    accumulate<KID, NOUT, ACC>(P, r2, acc0, acc1, pix(xi - X0, yi - Y0));
            }
        }
    }
}

// Lane-per-record deposit of a box of at most S x S pixels: dy^2 per column in
// registers, an unrolled S x S pass decides every pair whose fp32 r2 is outside the error
// band and accumulates it; band pairs (~0.1 %) only set a bit, resolved afterwards in
// fp64 -- keeping the rare slow path out of the unrolled body.
template <int KID, int NOUT, int ACC, int S>
__device__ __forceinline__ void small_box(const Grid& g, const Src64& s, const Prep& P, int bw,
                                          int bh, int X0, int Y0, const float* xt,
                                          const float* yt, unsigned long long* acc0,
                                          unsigned long long* acc1) {
    const int base = pix(P.b.x0 - X0, P.b.y0 - Y0);  // LDS word of pixel (0, 0)
    float dy2[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        float dy = P.v - yt[min(j, bh - 1)];
        dy2[j] = dy * dy;
    }
    unsigned amb = 0u;
#pragma unroll
    for (int ii = 0; ii < S; ++ii) {
        if (ii < bw) {
            float dx = P.u - xt[ii];
            float dx2 = dx * dx;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (j < bh) {
                    float r2 = dx2 + dy2[j];
                    bool a = r2 >= P.lo && r2 <= P.hi;
                    amb |= a ? (1u << (ii * S + j)) : 0u;
                    if (r2 < P.lo)
                        accumulate<KID, NOUT, ACC>(P, r2, acc0, acc1, base + ii * kRow + j);
                }
            }
        }
    }
    while (amb) {
        int bit = __builtin_ctz(amb);
        amb &= amb - 1u;
        int ii = bit / S, j = bit - (bit / S) * S;
        int xi = P.b.x0 + ii, yi = P.b.y0 + j;
        if (exact_pair(g, s, P.p, xi, yi)) {
            float dx = P.u - xt[ii], dy = P.v - yt[j];
            accumulate<KID, NOUT, ACC>(P, dx * dx + dy * dy, acc0, acc1, pix(xi - X0, yi - Y0));
        }
    }
}

// Lane-per-record deposit of a box of at most 3 x 3 pixel corners (pixel-scale h), the
// common case: the nine fp32 r2 and kernel values are computed branch-free in packed
// fp32, and every pair with r2 < (2h)^2 is added.  Valid only when no pair lies in the
// error band (min |r2 - thr| > band): returns false for such a record WITHOUT touching the
// tile; the caller defers it to the exact path (small_box).  The three corner offsets per
// axis come from registers (Corner3: the corner tables' first entries, the same fp32
// values), not LDS: a table read here made every batch wait (lgkmcnt) for the previous
// batch's LDS atomics, which complete in order ahead of it.
struct Corner3 {
    float x[3], y[3];
};
__device__ __forceinline__ Corner3 corner3(const Grid& g) {  // = xt[0..2], yt[0..2]
    Corner3 c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.x[k] = (float)((double)k * g.psx);
        c.y[k] = (float)((double)k * g.psy_pix);
    }
    return c;
}
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ bool small3_fast(const Prep& P, int bw, int bh, int X0, int Y0,
                                            const Corner3& cc,
                                            unsigned long long* acc0, unsigned long long* acc1) {
    constexpr float kFar = 1e18f;  // outside the box: r2 ~ 1e36, far from any threshold
    float dx2[3];
    f2v dy2;
    float dyc2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float d = P.u - cc.x[i];
        d = i < bw ? d : kFar;
        dx2[i] = d * d;
    }
    {
        float d0 = P.v - cc.y[0];
        float d1 = P.v - cc.y[1];
        float d2 = P.v - cc.y[2];
        d1 = bh > 1 ? d1 : kFar;
        d2 = bh > 2 ? d2 : kFar;
        f2v d = f2v{d0, d1};
        dy2 = d * d;
        dyc2 = d2 * d2;
    }
    f2v r2[3];
    float r2c[3];
    float m = __builtin_inff();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r2[i] = dy2 + dx2[i];
        r2c[i] = dx2[i] + dyc2;
        f2v e = r2[i] - P.thr;
        m = fminf(m, fminf(fminf(fabsf(e.x), fabsf(e.y)), fabsf(r2c[i] - P.thr)));
    }
    if (!(m > P.band)) return false;  // a pair in the band (or NaN): exact path
    const int base = pix(P.b.x0 - X0, P.b.y0 - Y0);
    const f2v hv = f2v{P.hinv, P.hinv};
    // column j = 2 of rows 0, 1 as one packed pair, row 2 with a dummy partner
    f2v wc01 = kernel_shape2<KID>(sqrt2(f2v{r2c[0], r2c[1]}) * hv);
    f2v wc2 = kernel_shape2<KID>(sqrt2(f2v{r2c[2], 0.0f}) * hv);
    const float wc[3] = {wc01.x, wc01.y, wc2.x};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f2v w = kernel_shape2<KID>(sqrt2(r2[i]) * hv);
        f2v t0 = w * P.s0, t1 = w * P.s1;
        f2v c = f2v{wc[i], wc[i]} * f2v{P.s0, P.s1};
        const int k = base + i * kRow;
        if (r2[i].x < P.thr) {
            acc_add<ACC>(&acc0[k], t0.x);
            if constexpr (NOUT == 2) acc_add<ACC>(&acc1[k], t1.x);
        }
        if (r2[i].y < P.thr) {
            acc_add<ACC>(&acc0[k + 1], t0.y);
            if constexpr (NOUT == 2) acc_add<ACC>(&acc1[k + 1], t1.y);
        }
        if (r2c[i] < P.thr) {
            acc_add<ACC>(&acc0[k + 2], c.x);
            if constexpr (NOUT == 2) acc_add<ACC>(&acc1[k + 2], c.y);
        }
    }
    return true;
}

// Per-wave list of records deferred to the exact path (a pair in the error band).
constexpr int kDeferCap = 128;

// Exact body for deferred records: lanes 0 .. cnt-1 take list entries first .. first+cnt-1
// (record indices within the item), reload and re-prepare them and decide every pair
// with the error-band / fp64 logic of small_box.  Wave-level: no block barrier.
template <int KID, int NOUT, int ACC, int EXT>
__device__ __forceinline__ void deferred(const Grid& g, const Src64& s,
                                         const float4* __restrict__ recs,
                                         const float4* __restrict__ ext, int pass, long long start,
                                         const int* dlist, int first, int cnt, int X0, int Y0,
                                         int2 kk, const float* xt, const float* yt,
                                         unsigned long long* acc0, unsigned long long* acc1,
                                         int lane) {
    wave_sync();
    int idx = lane < cnt ? dlist[first + lane] : -1;
    __builtin_amdgcn_wave_barrier();
    if (idx < 0) return;
    float4 r0, r1;
    load_rec(recs, start + idx, r0, r1);
    Prep P;
    rec_prep<ACC>(r0, r1, X0, Y0, kk, P);
    if constexpr (EXT) ext_coef(P, ext[start + idx], pass);
    small_box<KID, NOUT, ACC, 4>(g, s, P, P.b.x1 - P.b.x0 + 1, P.b.y1 - P.b.y0 + 1, X0, Y0, xt,
                                 yt, acc0, acc1);
}

// ----------------------------------------------------------------------------------
// Gather form for mid and large boxes (K4g, K6).  A sweep costs an LDS atomic per pair
// and a pass per 64 box pixels; here every thread OWNS 8 pixels of the tile and sums
// their terms in registers.  Wave w owns the 16 x 32 region rows 16 (w / 2) .., columns
// 32 (w % 2) .., as 2 x 4 blocks of 8 x 8 pixels; lane l owns pixel (l / 8, l % 8) of
// each block (block j: block row j / 4, block column j % 4).  Each wave streams the
// item's records itself, 64 at a time (lane i prepares record i into a GEntry held in
// VGPRs), ballots which of them meet its region and walks those: v_readlane puts the
// entry's fields in SGPRs, the blocks the box meets are found with scalar compares, and
// only those blocks' pixels are evaluated -- one pixel per lane per block, so an entry
// costs ~ its box area / 64 wave instructions-per-pixel, whatever its size.  No LDS list,
// no block barrier, no atomics.  Sums: fp32 partials over <= 64 entries folded into fp64
// totals the thread owns in LDS (kAccF64), or exact int64 fixed point in registers
// (kAccFix).
// ----------------------------------------------------------------------------------
constexpr int kGatherThreads = 64;  // one wave per workgroup: one region of the tile
constexpr int kGatherRegions = 8;   // 16 x 32-pixel regions per tile
constexpr int kGatherPix = 8 * kGatherThreads;
static_assert(kGatherRegions * kGatherPix == kTile * kTile, "8 regions x 512 pixels cover the tile");
constexpr int kKernelIndicator = ASP_KERNEL_INDICATOR;
struct GEntry {
    float u, v, lo, hi, hinv, s0, s1;  // tile frame; s0, s1 with the shape's scale folded in
    int p;
    unsigned box;  // tile-local x0 | x1 << 8 | y0 << 16 | y1 << 24 (kNoBox: nothing)
};
constexpr unsigned kNoBox = 0x00ff00ffu;  // x0 = 255 > x1 = 0: meets no region

// One thread's 8 pixels: fp32 partials in registers folded into fp64 totals that the
// thread owns in LDS (kAccF64; word j * 64 + lane: conflict-free), or exact int64
// fixed-point sums in registers (kAccFix).
template <int NOUT, int ACC>
struct GAcc {
    unsigned long long a0[8], a1[8];  // kAccFix sums
    f2 p0[4], p1[4];                  // kAccF64 fp32 partials, pixels (2k, 2k + 1)
    double* t0;
    double* t1;
    __device__ __forceinline__ void init(double* tot) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a0[j] = 0;
            a1[j] = 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p0[k] = (f2){0.0f, 0.0f};
            p1[k] = (f2){0.0f, 0.0f};
        }
        t0 = tot + threadIdx.x;
        t1 = tot + kGatherPix + threadIdx.x;
        if constexpr (ACC != kAccFix) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                t0[j * kGatherThreads] = 0.0;
                if (NOUT == 2) t1[j * kGatherThreads] = 0.0;
            }
        }
    }
    // pixel j += w * (s0, s1)
    __device__ __forceinline__ void add(int j, float w, float s0, float s1) {
        if constexpr (ACC == kAccFix) {
            a0[j] += f2fix(s0 * w);
            if (NOUT == 2) a1[j] += f2fix(s1 * w);
        } else {
            p0[j >> 1][j & 1] = fmaf(s0, w, p0[j >> 1][j & 1]);
            if (NOUT == 2) p1[j >> 1][j & 1] = fmaf(s1, w, p1[j >> 1][j & 1]);
        }
    }
    // pixels 2k, 2k + 1 += w.xy * (s0, s1)  (one v_pk_fma_f32 per map)
    __device__ __forceinline__ void add2(int k, f2 w, float s0, float s1) {
        if constexpr (ACC == kAccFix) {
            add(2 * k, w.x, s0, s1);
            add(2 * k + 1, w.y, s0, s1);
        } else {
            p0[k] = __builtin_elementwise_fma(w, (f2){s0, s0}, p0[k]);
            if (NOUT == 2) p1[k] = __builtin_elementwise_fma(w, (f2){s1, s1}, p1[k]);
        }
    }
    __device__ __forceinline__ void fold() {
        if constexpr (ACC != kAccFix) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                t0[j * kGatherThreads] += (double)p0[j >> 1][j & 1];
                if (NOUT == 2) t1[j * kGatherThreads] += (double)p1[j >> 1][j & 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                p0[k] = (f2){0.0f, 0.0f};
                p1[k] = (f2){0.0f, 0.0f};
            }
        }
    }
    // the accumulator word of pixel j (as the LDS tile / slabs hold it)
    __device__ __forceinline__ unsigned long long word0(int j) const {
        if constexpr (ACC == kAccFix) return a0[j];
        else return (unsigned long long)__double_as_longlong(t0[j * kGatherThreads]);
    }
    __device__ __forceinline__ unsigned long long word1(int j) const {
        if constexpr (ACC == kAccFix) return a1[j];
        else return (unsigned long long)__double_as_longlong(t1[j * kGatherThreads]);
    }
};

// LDS of K4g / K6: the fp64 totals, one word per pixel and map (none in fixed point).
template <int NOUT, int ACC>
constexpr size_t gather_lds() {
    return ACC == kAccFix ? 8 : (size_t)NOUT * kGatherPix * 8;
}

// This thread's pixels: pixel j at row r0 + 8 (j / 4) + lr, column c0 + 8 (j % 4) + lc.
struct GOwn {
    int r0, c0;  // the wave's region (uniform)
    int lr, lc;  // the lane's place in each 8 x 8 block
    __device__ __forceinline__ int row(int j) const { return r0 + 8 * (j >> 2) + lr; }
    __device__ __forceinline__ int col(int j) const { return c0 + 8 * (j & 3) + lc; }
};
__device__ __forceinline__ GOwn gather_owner(int w) {  // w: the region (uniform)
    const int lane = threadIdx.x;
    GOwn o;
    o.r0 = (w >> 1) * 16;
    o.c0 = (w & 1) * 32;
    o.lr = lane >> 3;
    o.lc = lane & 7;
    return o;
}

// Tile-local corner offsets fl32(k * pitch): the values of the corner tables (K4), here
// computed where they are needed (a gather workgroup has no tables).
__device__ __forceinline__ float corner_off_x(const Grid& g, int k) { return (float)((double)k * g.psx); }
__device__ __forceinline__ float corner_off_y(const Grid& g, int k) { return (float)((double)k * g.psy_pix); }

// The corner coordinates of the thread's pixels: 2 rows, 4 columns; and (wave-uniform) the
// corner span of each of the region's 8 x 16 half block rows: rows xl[r]..xh[r] of block
// row r, columns yl[k]..yh[k] of column half k.
struct GCorner {
    float X[2], Y[4];
    float xl[2], xh[2], yl[2], yh[2];
};
__device__ __forceinline__ GCorner gather_corners(const Grid& g, const GOwn& o) {
    GCorner c;
    c.X[0] = corner_off_x(g, o.row(0));
    c.X[1] = corner_off_x(g, o.row(4));
#pragma unroll
    for (int k = 0; k < 4; ++k) c.Y[k] = corner_off_y(g, o.col(k));
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        c.xl[r] = corner_off_x(g, o.r0 + 8 * r);
        c.xh[r] = corner_off_x(g, o.r0 + 8 * r + 7);
        c.yl[r] = corner_off_y(g, o.c0 + 16 * r);
        c.yh[r] = corner_off_y(g, o.c0 + 16 * r + 15);
    }
    return c;
}

// The region's half block rows the entry's DISC can reach (bit 2 r + k: block row r,
// column half k), from the distance between (u, v) and each half row's corner rectangle
// (closest point by clamping).  Conservative: a skipped half row has every pixel at
// fp32 distance^2 >= lim = (2h)^2 (1 + 2^-8) from the particle -- far outside any rounding
// of the pair distance -- so the edge form (§3) gives each of them exactly 0 and skipping
// them changes no sum.  Computed per lane for its own entry before the walk (vectorised
// over the 64 entries), so the walk tests bits instead of box bounds.
__device__ __forceinline__ unsigned edge_mask(const GCorner& c, float u, float v, float thr) {
    float dx2[2], dy2[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float dx = u - fminf(fmaxf(u, c.xl[r]), c.xh[r]);
        const float dy = v - fminf(fmaxf(v, c.yl[r]), c.yh[r]);
        dx2[r] = dx * dx;
        dy2[r] = dy * dy;
    }
    const float lim = thr * (1.0f + 0x1p-8f);
    unsigned m = 0u;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) m |= (dx2[r] + dy2[k] < lim) ? 1u << (2 * r + k) : 0u;
    return m;
}

__device__ __forceinline__ GEntry make_gentry(const Prep& P, int X0, int Y0, float scale) {
    GEntry e;
    e.u = P.u; e.v = P.v; e.lo = P.lo; e.hi = P.hi; e.hinv = P.hinv;
    e.s0 = P.s0 * scale; e.s1 = P.s1 * scale; e.p = P.p;
    e.box = (unsigned)(P.b.x0 - X0) | ((unsigned)(P.b.x1 - X0) << 8) |
            ((unsigned)(P.b.y0 - Y0) << 16) | ((unsigned)(P.b.y1 - Y0) << 24);
    return e;
}

__device__ __forceinline__ bool meets_region(unsigned box, const GOwn& o) {
    return (int)(box & 255u) <= o.r0 + 15 && (int)((box >> 8) & 255u) >= o.r0 &&
           (int)((box >> 16) & 255u) <= o.c0 + 31 && (int)(box >> 24) >= o.c0;
}

// Lane l's entry, wave-uniform (SGPRs).
__device__ __forceinline__ GEntry lane_entry(const GEntry& e, int l) {
    GEntry E;
    E.u = bcast(e.u, l); E.v = bcast(e.v, l); E.lo = bcast(e.lo, l); E.hi = bcast(e.hi, l);
    E.hinv = bcast(e.hinv, l); E.s0 = bcast(e.s0, l); E.s1 = bcast(e.s1, l);
    E.p = bcast(e.p, l); E.box = (unsigned)bcast((int)e.box, l);
    return E;
}

// Which of the wave's 8 blocks the box meets (bit j; uniform).
__device__ __forceinline__ unsigned block_hits(unsigned box, const GOwn& o) {
    const int x0 = box & 255u, x1 = (box >> 8) & 255u;
    const int y0 = (box >> 16) & 255u, y1 = box >> 24;
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int br = o.r0 + 8 * (j >> 2), bc = o.c0 + 8 * (j & 3);
        if (x0 <= br + 7 && x1 >= br && y0 <= bc + 7 && y1 >= bc) m |= 1u << j;
    }
    return m;
}

// Edge-continuous kernels (cubic / Wendland) on a square grid without a mixed cull take no
// decision at all (gather_entry_masked below): W by edge_shape for every pixel of every
// 8 x 16 half block row the entry's disc reaches.  A pixel the reference excludes has
// exact r >= 2h, so its fp32 t = 1 - q/2 lies inside the entry's dead zone (edge_dead2,
// asp_device.hpp) and its term is exactly 0; one it includes inside the dead zone loses a
// term below tau^3 W(0).

// One (uniform) entry, every other case: the box's own rows and columns (non-square grids
// and mixed culls clip the box to the chunk ranges), the error band and the fp64
// decision -- the indicator kernel's neighbour sets are the reference's exactly.
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void gather_entry(const Grid& g, const Src64& s, const GEntry& E,
                                             int X0, int Y0, const GOwn& o, const GCorner& c,
                                             GAcc<NOUT, ACC>& ga) {
    const unsigned m = block_hits(E.box, o);
    const int x0 = E.box & 255u, x1 = (E.box >> 8) & 255u;
    const int y0 = (E.box >> 16) & 255u, y1 = E.box >> 24;
    unsigned in = 0u, amb = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (m & (1u << j)) {
            const float dx = E.u - c.X[j >> 2], dy = E.v - c.Y[j & 3];
            const float r2 = dx * dx + dy * dy;
            const bool inb = (unsigned)(o.row(j) - x0) <= (unsigned)(x1 - x0) &&
                             (unsigned)(o.col(j) - y0) <= (unsigned)(y1 - y0);
            in |= (inb && r2 < E.lo) ? (1u << j) : 0u;
            amb |= (inb && r2 >= E.lo && r2 <= E.hi) ? (1u << j) : 0u;
        }
    }
    for (unsigned a = amb; a; a &= a - 1u) {  // the reference's fp64 decision, one call site
        const int j = __builtin_ctz(a);
        if (exact_pair(g, s, E.p, X0 + o.row(j), Y0 + o.col(j))) in |= 1u << j;
    }
    const float sc = 1.0f / kShapeScale<KID>;  // s0, s1 carry the edge form's scale
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (in & (1u << j)) {  // (the same r2 as above: same operations)
            const float dx = E.u - c.X[j >> 2], dy = E.v - c.Y[j & 3];
            const float r2 = dx * dx + dy * dy;
            const float wk = kernel_shape<KID>(__builtin_amdgcn_sqrtf(r2) * E.hinv) * sc;
            ga.add(j, wk, E.s0, E.s1);
        }
    }
}

// One (uniform) entry of the edge path given its half-row mask bm (edge_mask).
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void gather_entry_masked(float u, float vs, float hinv, float s0,
                                                    float s1, float nt2, unsigned bm,
                                                    const GCorner& c, GAcc<NOUT, ACC>& ga) {
    const f2 hv = {-hinv, -hinv};
    const f2 dead = {nt2, nt2};  // the entry's dead zone at q = 2 (edge_dead2)
    const f2 vv = {vs, vs};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (bm & (3u << (2 * r))) {
            const float dxs = (u - c.X[r]) * hinv;
            const f2 dx2 = {dxs * dxs, dxs * dxs};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (bm & (1u << (2 * r + k))) {
                    const f2 dys = __builtin_elementwise_fma(hv, (f2){c.Y[2 * k], c.Y[2 * k + 1]}, vv);
                    const f2 r2 = __builtin_elementwise_fma(dys, dys, dx2);
                    f2 q;
                    q.x = __builtin_amdgcn_sqrtf(r2.x);
                    q.y = __builtin_amdgcn_sqrtf(r2.y);
                    ga.add2(2 * r + k, edge_shape2<KID, true>(q, dead), s0, s1);
                }
            }
        }
    }
}

// The wave's walk over its lanes' entries: those whose box meets the wave's region.
template <int KID, int NOUT, int ACC>
__device__ __forceinline__ void gather_walk(const Grid& g, const Src64& s, const GEntry& mine,
                                            int X0, int Y0, const GOwn& o, const GCorner& c,
                                            GAcc<NOUT, ACC>& ga) {
    if (KID != kKernelIndicator && !g.nonsquare && !g.mixed) {  // uniform
        // edge path: each lane finds the half rows its entry's disc reaches, and precomputes
        // v / h; the walk then reads 6 words per entry and tests mask bits
        const unsigned em = mine.box == kNoBox ? 0u : edge_mask(c, mine.u, mine.v, mine.hi);
        const float vs = mine.v * mine.hinv;
        // the entry's dead zone (-tau^2, edge_dead2) rides in the mask word, the mask in its
        // low 4 mantissa bits (2^-19 of tau^2, far inside tau's own 2^-20 margin): the walk
        // reads one word per entry for both
        const unsigned emd = em | (__float_as_uint(edge_dead2(mine.lo, mine.hi)) & ~15u);
        unsigned long long m = __ballot(em != 0u);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const unsigned w = (unsigned)bcast((int)emd, l);
            gather_entry_masked<KID, NOUT, ACC>(bcast(mine.u, l), bcast(vs, l), bcast(mine.hinv, l),
                                                bcast(mine.s0, l), bcast(mine.s1, l),
                                                __uint_as_float(w), w & 15u, c, ga);
        }
    } else {
        unsigned long long m = __ballot(meets_region(mine.box, o));
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            gather_entry<KID, NOUT, ACC>(g, s, lane_entry(mine, l), X0, Y0, o, c, ga);
        }
    }
    ga.fold();
}

// Write the thread's 8 pixels: partial slab (split tiles) or the map.
template <int NOUT, int ACC>
__device__ __forceinline__ void gather_emit(const Grid& g, const GAcc<NOUT, ACC>& ga,
                                            const GOwn& o, int X0, int Y0, int slab,
                                            unsigned long long* slabs, int k0, int k1,
                                            float* out0, float* out1, int flags) {
    if (slab >= 0) {  // unpadded slab layout
        unsigned long long* dst = slabs + (long long)slab * NOUT * kTilePix;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = o.row(j) * kTile + o.col(j);
            dst[k] = ga.word0(j);
            if (NOUT == 2) dst[kTilePix + k] = ga.word1(j);
        }
        return;
    }
    const int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (o.row(j) >= TW || o.col(j) >= TH) continue;
        const long long off = (long long)(X0 + o.row(j)) * g.ny + (Y0 + o.col(j));
        emit_pixel<NOUT, ACC>(off, ga.word0(j), NOUT == 2 ? ga.word1(j) : 0ull, k0, k1, out0,
                              out1, flags);
    }
}

// ----------------------------------------------------------------------------------
// Bank-balanced record order for K4 (ASP_DEP_ORDER).  A ds_add_f64 is served in four
// contiguous 16-lane groups, and lanes of a group whose 8-B words share a bank pair (word
// index mod 16) take one LDS pass each (measured: tools/microbench/lds.hip `dep`,
// profiles/deposit_order/).  The lane-per-record body adds the same constant i * kRow + j
// to every lane's base word, so lanes that are conflict-free at the base word are so for
// all 18 adds.  Each wave therefore takes a contiguous pool of kPool records of the item,
// loads only their box words, and orders the pool "by level": first one record of every
// bank pair that has any, then the second ones, ... -- 16 consecutive positions hold
// distinct bank pairs wherever a level is full.  Lane l of batch j takes the record at
// position 64 j + l and loads it by index (the pool's lines are in L2 from the key loads).
// ----------------------------------------------------------------------------------
constexpr int kPoolBatches = 2;
constexpr int kPool = 64 * kPoolBatches;  // <= 256: pool indices are bytes
static_assert(kRow % 16 == 1, "bank pair of pix(x, y) is (x + y) mod 16");
struct OrderLds {  // per wave
    int cnt[16];               // records per bank pair
    unsigned lvl[64];          // level r: positions before it << 16 | bank pairs present
    unsigned char tab[kPool];  // position -> pool index, [lane][batch]
};

// key[j]: packed box word of pool record 64 j + lane; the first n records are live.
// Returns the pool indices this lane takes in batches 0 .. kPoolBatches-1, one byte each
// (meaningful for positions 64 j + lane < n only).
__device__ __forceinline__ unsigned order_pool(const unsigned (&key)[kPoolBatches], int n,
                                               OrderLds& w, int lane) {
    if (lane < 16) w.cnt[lane] = 0;
    wave_sync();
    int bank[kPoolBatches], r[kPoolBatches];  // bank pair; rank among the pool's records of it
    bool big = false;
#pragma unroll
    for (int j = 0; j < kPoolBatches; ++j) {
        bank[j] = (int)(((key[j] & 255u) + ((key[j] >> 16) & 255u)) & 15u);
        r[j] = j * 64 + lane < n ? atomicAdd(&w.cnt[bank[j]], 1) : 0;
        big |= r[j] >= 64;
    }
    wave_sync();
    const int c = w.cnt[lane & 15];
    {   // lane r: level r starts at T = sum_b min(cnt[b], r) and holds the banks with cnt > r
        int T = 0;
        unsigned m = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int cb = __builtin_amdgcn_readlane(c, b);
            T += min(cb, lane);
            m |= cb > lane ? 1u << b : 0u;
        }
        w.lvl[lane] = (unsigned)T << 16 | m;
    }
    wave_sync();
    int pos[kPoolBatches];
    if (__ballot(big)) {  // a bank pair with more than 64 records: the same sums per record
#pragma unroll
        for (int j = 0; j < kPoolBatches; ++j) {
            int p = 0;
            for (int b = 0; b < 16; ++b) {
                const int cb = __builtin_amdgcn_readlane(c, b);
                p += min(cb, r[j]) + (b < bank[j] && cb > r[j] ? 1 : 0);
            }
            pos[j] = p;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPoolBatches; ++j) {
            const unsigned e = w.lvl[r[j]];
            pos[j] = (int)(e >> 16) + __popc(e & ((1u << bank[j]) - 1u));
        }
    }
#pragma unroll
    for (int j = 0; j < kPoolBatches; ++j)
        if (j * 64 + lane < n)
            w.tab[(pos[j] & 63) * kPoolBatches + (pos[j] >> 6)] = (unsigned char)(j * 64 + lane);
    wave_sync();
    unsigned idx = 0u;
#pragma unroll
    for (int j = 0; j < kPoolBatches; ++j) idx |= (unsigned)w.tab[lane * kPoolBatches + j] << (8 * j);
    wave_sync();
    return idx;
}

// Which records take which path in K4 (clipped box w x h pixels).
__device__ __forceinline__ bool is_small(int bw, int bh) { return bw <= 4 && bh <= 4; }

// ----------------------------------------------------------------------------------
// K4: deposit one work item (a run of records of one tile) into LDS, then write the
// tile (single-item tiles) or its partial slab (split tiles).
// ----------------------------------------------------------------------------------
template <int NOUT>
constexpr size_t deposit_lds() {
    return (size_t)NOUT * kTileWords * 8 + 2 * kTile * 4;
}

template <int KID, int NOUT, int ACC, int EXT = 0>
__global__ __launch_bounds__(kDepBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_deposit(
    Grid g, Src64 s, const float4* __restrict__ recs, const Item* __restrict__ items,
    const int* __restrict__ order, const int2* __restrict__ tile_k,
    unsigned long long* __restrict__ slabs, float* __restrict__ out0, float* __restrict__ out1,
    int flags, const float4* __restrict__ ext, int pass, const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];
    unsigned long long* acc0 = acc;
    unsigned long long* acc1 = acc + kTileWords;
    float* xt = (float*)(acc + NOUT * kTileWords);
    float* yt = xt + kTile;
    __shared__ int defer_lds[kDepBlock / 64][kDeferCap];
    // Two maps only: with one map a record has 9 adds, not 18, and ordering it costs more
    // than its conflicts (10^7 -> 2048^2 surface map: deposit 0.106 -> 0.127 ms ordered).
    constexpr bool kOrdered = ASP_DEP_ORDER && NOUT == 2;
    __shared__ OrderLds order_lds[kOrdered ? kDepBlock / 64 : 1];
    const Item it = items[order[blockIdx.x]];  // largest items first (k_tilescan)
    if (it.mode != 0) return;  // the large stream's (K4g)
    int tx = it.tile / g.nty, ty = it.tile - (it.tile / g.nty) * g.nty;
    int X0 = tx * kTile, Y0 = ty * kTile;
    int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
    if (it.count == 0) {  // empty tile: the map is 0 there
        if (flags & kFlagAccumulate) return;
        for (int k = threadIdx.x; k < kTilePix; k += kDepBlock) {
            int lx = k >> kTileShift, ly = k & (kTile - 1);
            if (lx >= TW || ly >= TH) continue;
            long long o = (long long)(X0 + lx) * g.ny + (Y0 + ly);
            out0[o] = 0.0f;
            if (NOUT == 2) out1[o] = 0.0f;
        }
        return;
    }
    const int2 kk = ACC == kAccFix ? tile_k[it.tile] : make_int2(0, 0);
    tile_prologue<NOUT, kDepBlock>(g, X0, Y0, acc, xt, yt);
    const int lane = threadIdx.x & 63;
    const Corner3 c3 = corner3(g);
    int* dlist = defer_lds[threadIdx.x >> 6];
    int ndef = 0;  // wave-uniform
    // One batch: record i (index within the item; r0, r1 its halves) of every thread.
    auto batch = [&](int i, const float4& r0, const float4& r1, const float4& e) {
        Prep P;
        P.b = Box{0, -1, 0, -1};
        bool live = i < it.count;
        if (live) {
            rec_prep<ACC>(r0, r1, X0, Y0, kk, P);
            if constexpr (EXT) ext_coef(P, e, pass);
        }
        live = live && P.b.x0 <= P.b.x1;  // (an empty box deposits nothing)
        const int bw = P.b.x1 - P.b.x0 + 1, bh = P.b.y1 - P.b.y0 + 1;
        const bool small = live && is_small(bw, bh);
        bool amb = false;
        if (small) {
            // lane-per-record.  Boxes of <= 3 x 3 corners (pixel-scale h) take the packed
            // body; 4-wide boxes and records with a pair in the error band are deferred to
            // the exact body, a full wave of them at a time
            if (bw <= 3 && bh <= 3)
                amb = !small3_fast<KID, NOUT, ACC>(P, bw, bh, X0, Y0, c3, acc0, acc1);
            else
                amb = true;
        }
        {
            unsigned long long am = __ballot(amb);
            if (am) {
                if (amb) dlist[ndef + __popcll(am & ((1ull << lane) - 1ull))] = i;
                ndef += __popcll(am);
                if (ndef >= 64) {  // a full wave of deferred records
                    ndef -= 64;
                    deferred<KID, NOUT, ACC, EXT>(g, s, recs, ext, pass, it.start, dlist, ndef,
                                                  64, X0, Y0, kk, xt, yt, acc0, acc1, lane);
                }
            }
        }
        unsigned long long mid = __ballot(live && !small);
        while (mid) {
            int l = __builtin_ctzll(mid);
            mid &= mid - 1;
            Prep Q = bcast_prep(P, l);
            sweep<KID, NOUT, ACC>(g, s, Q, X0, Y0, xt, yt, acc0, acc1, lane);
        }
    };
    const int last = it.count - 1;
    // Software pipeline: batch i + 2 is issued before batch i deposits.  The loads are
    // unconditional (index clamped to the item's last record; lanes past the end ignore
    // theirs), so every iteration issues the same two loads and the compiler's wait
    // before batch i leaves the batch just issued in flight (vmcnt(2); the register
    // rotation makes it wait for batch i + 1 too).  Loads under a branch made it
    // vmcnt(0), i.e. one full memory latency per batch: deposit 1.26 -> 1.22 ms (cfg 3).
    float4 r0, r1, q0, q1, re, qe;  // (re, qe, ne: the EXT coefficients, pass > 0)
    auto load_ext = [&](long long i, float4& e) {
        if constexpr (EXT) e = ext[i];
        else e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    if constexpr (kOrdered) {
        // Wave w takes the pools (k * waves + w) of kPool records, k = 0, 1, ...; pool k + 1 is
        // ordered (order_pool; its keys were issued a pool ago) and pool k + 2's keys are issued
        // before pool k deposits, and every batch is loaded by index two batches ahead.  The
        // loop starts at an empty pool -1 (dead lanes) so that it is entered with the loads in
        // the order every iteration leaves them in -- keys, then records: the waits for the keys
        // and before each batch stay counted vmcnt that leave the later loads in flight (keys
        // issued last in a prologue, or pool -1 peeled off, made them vmcnt(0)).
        OrderLds& ol = order_lds[threadIdx.x >> 6];
        constexpr int kWaves = kDepBlock / 64;
        auto pstart = [&](int k) { return (max(k, 0) * kWaves + (int)(threadIdx.x >> 6)) * kPool; };
        auto pcount = [&](int k) { return k < 0 ? 0 : max(0, min(kPool, it.count - pstart(k))); };
        auto load_keys = [&](int k, unsigned (&key)[kPoolBatches]) {  // the packed box words
#pragma unroll
            for (int j = 0; j < kPoolBatches; ++j)
                key[j] = __float_as_uint(
                    ((const float*)recs)[(it.start + min(pstart(k) + j * 64 + lane, last)) * 8 + 7]);
        };
        unsigned key[kPoolBatches];
        load_keys(0, key);
        asm volatile("" ::: "memory");  // keys first
        load_rec(recs, it.start + min(pstart(0), last), r0, r1);
        load_ext(it.start + min(pstart(0), last), re);
        load_rec(recs, it.start + min(pstart(0) + 1, last), q0, q1);
        load_ext(it.start + min(pstart(0) + 1, last), qe);
        unsigned cidx = 0u;
#pragma nounroll
        for (int k = -1; k * (kWaves * kPool) < it.count; ++k) {
            const int n = pcount(k), nn = pcount(k + 1);
            const unsigned nidx = nn > 0 ? order_pool(key, nn, ol, lane) : 0u;
            load_keys(k + 2, key);
#pragma unroll
            for (int j = 0; j < kPoolBatches; ++j) {
                constexpr int kAhead = 2;  // batches
                const int ni = j + kAhead < kPoolBatches
                    ? pstart(k) + (int)(cidx >> (8 * ((j + kAhead) % kPoolBatches)) & 255u)
                    : pstart(k + 1) + (int)(nidx >> (8 * ((j + kAhead) % kPoolBatches)) & 255u);
                float4 n0, n1, ne;
                load_rec(recs, it.start + min(ni, last), n0, n1);
                load_ext(it.start + min(ni, last), ne);
                // (positions past the pool's end are dead lanes: index it.count)
                batch(j * 64 + lane < n ? pstart(k) + (int)(cidx >> (8 * j) & 255u) : it.count, r0, r1,
                      re);
                r0 = q0;
                r1 = q1;
                re = qe;
                q0 = n0;
                q1 = n1;
                qe = ne;
            }
            cidx = nidx;
        }
        static_assert(kPoolBatches >= 2, "a batch is loaded two batches ahead: at most one pool");
    } else {
        load_rec(recs, it.start + min((int)threadIdx.x, last), r0, r1);
        load_ext(it.start + min((int)threadIdx.x, last), re);
        load_rec(recs, it.start + min((int)threadIdx.x + kDepBlock, last), q0, q1);
        load_ext(it.start + min((int)threadIdx.x + kDepBlock, last), qe);
        for (int base = 0; base < it.count; base += kDepBlock) {
            float4 n0, n1, ne;
            load_rec(recs, it.start + min(base + (int)threadIdx.x + 2 * kDepBlock, last), n0, n1);
            load_ext(it.start + min(base + (int)threadIdx.x + 2 * kDepBlock, last), ne);
            batch(base + threadIdx.x, r0, r1, re);
            r0 = q0;
            r1 = q1;
            re = qe;
            q0 = n0;
            q1 = n1;
            qe = ne;
        }
    }
    if (ndef > 0)
        deferred<KID, NOUT, ACC, EXT>(g, s, recs, ext, pass, it.start, dlist, 0, ndef, X0, Y0, kk,
                                      xt, yt, acc0, acc1, lane);
    __syncthreads();
    if (it.slab >= 0) {  // split tile: partial sums, merged by K5 (slab layout unpadded)
        unsigned long long* dst = slabs + (long long)it.slab * NOUT * kTilePix;
        for (int k = threadIdx.x; k < kTilePix; k += kDepBlock) {
            const int w = pix(k >> kTileShift, k & (kTile - 1));
            dst[k] = acc0[w];
            if (NOUT == 2) dst[kTilePix + k] = acc1[w];
        }
        return;
    }
    for (int k = threadIdx.x; k < kTilePix; k += kDepBlock) {
        int lx2 = k >> kTileShift, ly = k & (kTile - 1);
        if (lx2 >= TW || ly >= TH) continue;
        long long o = (long long)(X0 + lx2) * g.ny + (Y0 + ly);
        const int w = pix(lx2, ly);
        emit_pixel<NOUT, ACC>(o, acc0[w], NOUT == 2 ? acc1[w] : 0ull, kk.x, kk.y, out0, out1,
                              flags);
    }
}

// ----------------------------------------------------------------------------------
// K4g: deposit one work item of the LARGE stream (records whose clipped box is at least
// gather_min pixels on both axes, or gather_area pixels) in the gather form: every wave streams the item's
// records 64 at a time (coalesced 32-B loads, the next 64 in flight) and walks those that
// meet its region (gather_walk).  The tile (or its partial slab) is written straight
// from the registers.
// ----------------------------------------------------------------------------------
template <int KID, int NOUT, int ACC, int EXT = 0>
__global__ __launch_bounds__(kGatherThreads) void k_gather(
    Grid g, Src64 s, const float4* __restrict__ recs, const Item* __restrict__ items,
    const int* __restrict__ order, const int2* __restrict__ tile_k,
    unsigned long long* __restrict__ slabs, float* __restrict__ out0, float* __restrict__ out1,
    int flags, const float4* __restrict__ ext, int pass, const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    extern __shared__ __attribute__((aligned(16))) double tot[];
    const Item it = items[order[blockIdx.x / kGatherRegions]];  // largest first
    if (it.mode != 1) return;
    const int tx = it.tile / g.nty, ty = it.tile - (it.tile / g.nty) * g.nty;
    const int X0 = tx * kTile, Y0 = ty * kTile;
    const int2 kk = ACC == kAccFix ? tile_k[it.tile] : make_int2(0, 0);
    const int lane = threadIdx.x;
    // unconditional loads (index clamped to the item's last record), so no wait or copy
    // of the next batch is forced inside the walk
    const int last = it.count - 1;
    float4 r0, r1, e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    load_rec(recs, it.start + min(lane, last), r0, r1);
    if constexpr (EXT) e = ext[it.start + min(lane, last)];
    const GOwn o = gather_owner(blockIdx.x % kGatherRegions);
    GAcc<NOUT, ACC> ga;
    ga.init(tot);
    const GCorner cc = gather_corners(g, o);
    for (int base = 0; base < it.count; base += 64) {
        GEntry mine;
        mine.box = kNoBox;
        if (base + lane < it.count) {
            Prep P;
            rec_prep<ACC>(r0, r1, X0, Y0, kk, P);
            if constexpr (EXT) ext_coef(P, e, pass);
            P.u += corner_off_x(g, P.b.x0 - X0);  // box-origin frame -> tile frame
            P.v += corner_off_y(g, P.b.y0 - Y0);
            mine = make_gentry(P, X0, Y0, kShapeScale<KID>);
        }
        // the next 64 records load while this batch is walked
        load_rec(recs, it.start + min(base + 64 + lane, last), r0, r1);
        if constexpr (EXT) e = ext[it.start + min(base + 64 + lane, last)];
        gather_walk<KID, NOUT, ACC>(g, s, mine, X0, Y0, o, cc, ga);
    }
    gather_emit<NOUT, ACC>(g, ga, o, X0, Y0, it.slab, slabs, kk.x, kk.y, out0, out1, flags);
}

// ----------------------------------------------------------------------------------
// K5: split tiles -- sum of the item slabs in slab order (deterministic), convert, write.
// Grid (merges, kTilePix / kBlock): each workgroup one 4-row strip of a tile, one pixel
// per thread; the slab loop issues kMergeBatch independent loads per map before summing.
// ----------------------------------------------------------------------------------
constexpr int kMergeBatch = 8;
template <int NOUT, int ACC>
__global__ __launch_bounds__(kBlock) void k_merge(Grid g, const Merge* __restrict__ merges,
                                                  const unsigned long long* __restrict__ slabs,
                                                  const int2* __restrict__ tile_k,
                                                  float* __restrict__ out0,
                                                  float* __restrict__ out1, int flags,
                                                  const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    const Merge m = merges[blockIdx.x];
    int tx = m.tile / g.nty, ty = m.tile - (m.tile / g.nty) * g.nty;
    int X0 = tx * kTile, Y0 = ty * kTile;
    int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
    const int k = blockIdx.y * kBlock + threadIdx.x;
    int lx = k >> kTileShift, ly = k & (kTile - 1);
    if (lx >= TW || ly >= TH) return;
    const int2 kk = ACC == kAccFix ? tile_k[m.tile] : make_int2(0, 0);
    const unsigned long long* src = slabs + (long long)m.slab0 * NOUT * kTilePix + k;
    unsigned long long s0 = 0, s1 = 0;  // +0.0 in fp64 as well
    int j = 0;
    for (; j + kMergeBatch <= m.nslab; j += kMergeBatch) {
        unsigned long long b0[kMergeBatch], b1[kMergeBatch];
#pragma unroll
        for (int q = 0; q < kMergeBatch; ++q) {
            const unsigned long long* p = src + (long long)(j + q) * NOUT * kTilePix;
            b0[q] = p[0];
            b1[q] = NOUT == 2 ? p[kTilePix] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < kMergeBatch; ++q) {  // fixed slab order: deterministic
            s0 = acc_sum<ACC>(s0, b0[q]);
            if (NOUT == 2) s1 = acc_sum<ACC>(s1, b1[q]);
        }
    }
    for (; j < m.nslab; ++j) {
        const unsigned long long* p = src + (long long)j * NOUT * kTilePix;
        s0 = acc_sum<ACC>(s0, p[0]);
        if (NOUT == 2) s1 = acc_sum<ACC>(s1, p[kTilePix]);
    }
    long long o = (long long)(X0 + lx) * g.ny + (Y0 + ly);
    emit_pixel<NOUT, ACC>(o, s0, s1, kk.x, kk.y, out0, out1, flags);
}

// ----------------------------------------------------------------------------------
// K6: wide particles (footprint over > wide_tiles tiles): they are never binned.  One
// workgroup per tile; every wave streams the wide list 64 particles at a time, prepares
// them (prep_record + clip to the tile) and gathers those meeting its region as K4g does;
// fixed point with the wide particles' own bound.  Adds onto the tile K4/K4g/K5 wrote.
// ----------------------------------------------------------------------------------
template <int KID, int NOUT, int ACC>
__global__ __launch_bounds__(kGatherThreads) void k_wide(
    Grid g, Src64 s, const float* __restrict__ u, const float* __restrict__ v,
    const float* __restrict__ h, const float* __restrict__ a0, const float* __restrict__ a1,
    const int* __restrict__ wide_list, int n_wide, const int* __restrict__ ctr,
    float* __restrict__ out0, float* __restrict__ out1, const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    extern __shared__ __attribute__((aligned(16))) double tot[];
    const int t = blockIdx.x / kGatherRegions;
    const int tx = t / g.nty, ty = t - (t / g.nty) * g.nty;
    const int X0 = tx * kTile, Y0 = ty * kTile;
    const int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
    const int k0 = ACC == kAccFix ? scale_exp(n_wide, __uint_as_float((unsigned)ctr[cWideMax0])) : 0;
    const int k1 = (ACC == kAccFix && NOUT == 2)
                       ? scale_exp(n_wide, __uint_as_float((unsigned)ctr[cWideMax1])) : 0;
    const int lane = threadIdx.x;
    const GOwn o = gather_owner(blockIdx.x % kGatherRegions);
    GAcc<NOUT, ACC> ga;
    ga.init(tot);
    const GCorner cc = gather_corners(g, o);
    bool any = false;  // wave-uniform
    for (int c = 0; c < n_wide; c += 64) {
        GEntry mine;
        mine.box = kNoBox;
        const int k = c + lane;
        if (k < n_wide) {
            const int p = wide_list[k];
            Prep P;
            if (prep_record<KID, ACC>(g, s, p, u[p], v[p], h[p], a0[p], NOUT == 2 ? a1[p] : 0.0f,
                                      k0, k1, P) &&
                clip(P.b, X0, Y0, TW, TH)) {
                P.u = (float)(src_u(s, p, P.u) - corner_x(g, X0));  // tile-local frame
                P.v = (float)(src_v(s, p, P.v) - corner_y(g, Y0));
                // the band of THIS frame (|P.u| <= 64 pitches + 2h, offsets < 64 pitches), as
                // K4g's: prep_record's g.mg band is the absolute frame's, and through
                // edge_dead2 it would put |corner| / 2h into the dead zone
                set_band(P, rec_thr(P.h), rec_band(g.mgl, P.h));
                mine = make_gentry(P, X0, Y0, kShapeScale<KID>);
            }
        }
        any = any || __ballot(mine.box != kNoBox) != 0ull;
        gather_walk<KID, NOUT, ACC>(g, s, mine, X0, Y0, o, cc, ga);
    }
    if (!any) return;
    gather_emit<NOUT, ACC>(g, ga, o, X0, Y0, -1, nullptr, k0, k1, out0, out1, kFlagAccumulate);
}

// ----------------------------------------------------------------------------------
// Diagnostic (bench.py's compute roofline, ASP_COUNT_EVALS=1): the (pixel, particle)
// lane-slots the deposit kernels spend, from the binned records, without evaluating any:
//   K4 small / mid stream: 9 per packed <= 3 x 3 box (every slot of the packed body), the
//      box area for 4 x 4 boxes, 64 per pass of a wave sweep;
//   K4g / K6 gather form: 128 per met 8 x 16 half block row (edge kernels) or 64 per met
//      8 x 8 block (decided path) -- as gather_entry_edge / gather_entry spend them.
// evals[0] += small / mid, evals[1] += gather (records), evals[2] += wide particles.
// ----------------------------------------------------------------------------------
__device__ __forceinline__ long long gather_slots(const Grid& g, int kid, unsigned box, float u,
                                                  float v, float hi) {
    const int x0 = box & 255u, x1 = (box >> 8) & 255u, y0 = (box >> 16) & 255u, y1 = box >> 24;
    const bool edge = kid != kKernelIndicator && !g.nonsquare && !g.mixed;
    long long c = 0;
    for (int w = 0; w < kGatherRegions; ++w) {
        const int r0 = (w >> 1) * 16, c0 = (w & 1) * 32;
        if (edge) {  // the half rows edge_mask lets through (u, v: tile frame)
            GOwn o;
            o.r0 = r0;
            o.c0 = c0;
            o.lr = o.lc = 0;
            c += 128LL * __builtin_popcount(edge_mask(gather_corners(g, o), u, v, hi));
            continue;
        }
        for (int r = 0; r < 2; ++r) {
            const int br = r0 + 8 * r;
            if (!(x0 <= br + 7 && x1 >= br)) continue;
            {
                for (int k = 0; k < 4; ++k) {
                    const int bc = c0 + 8 * k;
                    if (y0 <= bc + 7 && y1 >= bc) c += 64;
                }
            }
        }
    }
    return c;
}

__global__ __launch_bounds__(kBlock) void k_evals(Grid g, int kid, Src64 s,
                                                  const float4* __restrict__ recs,
                                                  const Item* __restrict__ items, int n_items,
                                                  const float* __restrict__ u,
                                                  const float* __restrict__ v,
                                                  const float* __restrict__ h,
                                                  const int* __restrict__ wide_list, int n_wide,
                                                  unsigned long long* __restrict__ evals) {
    long long c0 = 0, c1 = 0, c2 = 0;
    if ((int)blockIdx.x < n_items) {
        const Item it = items[blockIdx.x];
        const int tx = it.tile / g.nty, ty = it.tile - (it.tile / g.nty) * g.nty;
        const int X0 = tx * kTile, Y0 = ty * kTile;
        for (int i = threadIdx.x; i < it.count; i += kBlock) {
            float4 r0, r1;
            load_rec(recs, it.start + i, r0, r1);
            Prep P;
            rec_prep<kAccF64>(r0, r1, X0, Y0, make_int2(0, 0), P);
            const int bw = P.b.x1 - P.b.x0 + 1, bh = P.b.y1 - P.b.y0 + 1;
            if (bw <= 0) continue;  // an empty box
            if (it.mode == 1) {
                c1 += gather_slots(g, kid, __float_as_uint(r1.w),
                                   P.u + corner_off_x(g, P.b.x0 - X0),
                                   P.v + corner_off_y(g, P.b.y0 - Y0), P.hi);
            } else if (bw <= 3 && bh <= 3) {
                c0 += 9;
            } else if (is_small(bw, bh)) {
                c0 += bw * bh;
            } else {
                const int passes = bh <= 64 ? (bw + 64 / bh - 1) / (64 / bh) : bw * ((bh + 63) / 64);
                c0 += 64LL * passes;
            }
        }
    } else {  // one workgroup per tile: the wide particles the tile's K6 gathers
        const int t = blockIdx.x - n_items;
        const int tx = t / g.nty, ty = t - (t / g.nty) * g.nty;
        const int X0 = tx * kTile, Y0 = ty * kTile;
        const int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
        for (int i = threadIdx.x; i < n_wide; i += kBlock) {
            const int p = wide_list[i];
            Prep P;
            if (prep_record<2>(g, s, p, u[p], v[p], h[p], 0.0f, 0.0f, 0, 0, P) &&
                clip(P.b, X0, Y0, TW, TH)) {
                const unsigned box = (unsigned)(P.b.x0 - X0) | ((unsigned)(P.b.x1 - X0) << 8) |
                                     ((unsigned)(P.b.y0 - Y0) << 16) | ((unsigned)(P.b.y1 - Y0) << 24);
                set_band(P, rec_thr(P.h), rec_band(g.mgl, P.h));  // the tile frame's, as K6
                c2 += gather_slots(g, kid, box, (float)(src_u(s, p, P.u) - corner_x(g, X0)),
                                   (float)(src_v(s, p, P.v) - corner_y(g, Y0)), P.hi);
            }
        }
    }
    if (c0) atomicAdd(&evals[0], (unsigned long long)c0);
    if (c1) atomicAdd(&evals[1], (unsigned long long)c1);
    if (c2) atomicAdd(&evals[2], (unsigned long long)c2);
}

// K7: out0 <- out0 / out1 (0 where out1 == 0).
__global__ __launch_bounds__(kBlock) void k_ratio(float* __restrict__ out0,
                                                  const float* __restrict__ out1, long long m,
                                                  const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long stride = (long long)gridDim.x * kBlock;
    for (; i < m; i += stride) {
        float d = out1[i];
        out0[i] = d != 0.0f ? out0[i] / d : 0.0f;
    }
}

// K4 / K4g / K5 / K6: the records in ws deposited into o0 (, o1).  EXT = 0: the records'
// own two coefficients (a0 / a1: the properties' fp32 arrays, which the wide particles read
// directly).  EXT = 1 (asp_project2d_props, pass = 1, 2): properties (2 pass, 2 pass + 1)
// from the ext coefficients the pass-0 scatter wrote beside each record.
template <int KID, int NOUT, int ACC, int EXT>
static int run_deposit(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, const float* u,
                       const float* v, const float* h, const float* a0, const float* a1, float* o0,
                       float* o1, int dflags, hipStream_t st, int pass, const int* guard) {
    const float4* recs = (const float4*)ws.recs.p;
    const float4* ext = EXT ? (const float4*)ws.ext.p : nullptr;
    const Item* items = (const Item*)ws.items.p;
    const int* iorder = (const int*)ws.iorder.p;
    const int2* tile_k = (const int2*)ws.tile_k.p;
    unsigned long long* slabs = (unsigned long long*)ws.slabs.p;
    {
        StageMark m(ws, kSDeposit, st);
        const size_t lds = deposit_lds<NOUT>();
        ASP_TRY(allow_dyn_lds((const void*)k_deposit<KID, NOUT, ACC, EXT>, lds));
        hipLaunchKernelGGL((k_deposit<KID, NOUT, ACC, EXT>), dim3(pl.n_items), dim3(kDepBlock), lds,
                           st, g, s, recs, items, iorder, tile_k, slabs, o0, o1, dflags, ext, pass,
                           guard);
        ASP_LAUNCHED();
        m.done();
    }
    if (pl.n_large > 0) {
        StageMark m(ws, kSGather, st);
        hipLaunchKernelGGL((k_gather<KID, NOUT, ACC, EXT>), dim3(pl.n_items * kGatherRegions),
                           dim3(kGatherThreads), (gather_lds<NOUT, ACC>()), st, g, s, recs, items,
                           iorder, tile_k, slabs, o0, o1, dflags, ext, pass, guard);
        ASP_LAUNCHED();
        m.done();
    }
    if (pl.n_merges > 0) {
        StageMark m(ws, kSMerge, st);
        hipLaunchKernelGGL((k_merge<NOUT, ACC>), dim3(pl.n_merges, kTilePix / kBlock), dim3(kBlock),
                           0, st, g, (const Merge*)ws.merges.p, (const unsigned long long*)slabs,
                           tile_k, o0, o1, dflags, guard);
        ASP_LAUNCHED();
        m.done();
    }
    if (pl.n_wide > 0) {
        StageMark m(ws, kSWide, st);
        hipLaunchKernelGGL((k_wide<KID, NOUT, ACC>), dim3(g.ntiles * kGatherRegions),
                           dim3(kGatherThreads), (gather_lds<NOUT, ACC>()), st, g, s, u, v, h, a0,
                           a1, (const int*)ws.wide.p, pl.n_wide, (const int*)ws.counters.p, o0, o1,
                           guard);
        ASP_LAUNCHED();
        m.done();
    }
    return ASP_OK;
}

int launch_deposit(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid, int nout,
                   bool det, const float* u, const float* v, const float* h, const float* a0,
                   const float* a1, float* o0, float* o1, int dflags, hipStream_t st,
                   const int* guard) {
    return dispatch(kid, nout, det, [&](auto K, auto N, auto A) {
        return run_deposit<K(), N(), A(), 0>(g, s, ws, pl, u, v, h, a0, a1, o0, o1, dflags, st, 0,
                                             guard);
    });
}

int launch_deposit_props(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid,
                         int nout, const float* u, const float* v, const float* h,
                         const float* a0, const float* a1, float* o0, float* o1, int dflags,
                         hipStream_t st, int pass) {
    return dispatch_kid(kid, [&](auto K) {
        auto go = [&](auto N) {
            return run_deposit<K(), N(), kAccF64, 1>(g, s, ws, pl, u, v, h, a0, a1, o0, o1, dflags,
                                                     st, pass, nullptr);
        };
        return nout == 2 ? go(Int<2>{}) : go(Int<1>{});
    });
}

int launch_ratio(float* o0, const float* o1, long long npix, hipStream_t st, const int* guard) {
    hipLaunchKernelGGL(k_ratio, dim3(stream_blocks(npix)), dim3(kBlock), 0, st, o0, o1, npix,
                       guard);
    ASP_LAUNCHED();
    return ASP_OK;
}

int launch_evals(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid,
                 const float* u, const float* v, const float* h, unsigned long long* evals,
                 hipStream_t st) {
    hipLaunchKernelGGL(k_evals, dim3((unsigned)(pl.n_items + (pl.n_wide ? g.ntiles : 0))),
                       dim3(kBlock), 0, st, g, kid, s, (const float4*)ws.recs.p,
                       (const Item*)ws.items.p, pl.n_items, u, v, h, (const int*)ws.wide.p,
                       pl.n_wide, evals);
    ASP_LAUNCHED();
    return ASP_OK;
}

}  // namespace asp
