// asp_profiles.hip -- halo-centred radial profiles and aperture sums in a periodic box.
//
// For m halo centres with a radius each and nbins radial bins: the number of particles and
// the sum of up to four particle properties in every (halo, bin).  The arithmetic of a
// (particle, halo) pair is asp_nearest's (scipy's periodic distance, fp64, no contraction;
// include/asp_profiles.h has the definition), so a pair is in or out exactly as a NumPy
// restatement of the definition says.
//
// MI355X layout.  The particles are binned, the haloes gather:
//   prep (per batch of particles): every particle is wrapped once and keyed by its cell of
//     a G x G x G grid over [0, L) (asp_nearest's monotone cell expression; a row with a
//     non-finite coordinate gets key G^3, a cell no halo visits); the (key, index) pairs
//     are radix-sorted, the first particle of every cell is found from the sorted keys, and
//     the wrapped coordinates and the properties are gathered into cell order as fp64 SoA.
//     The key is (cx G + cy) G + cz, so the cells of one (cx, cy) row that a halo's reach
//     meets are one contiguous span of particles, or two when the reach wraps in z.
//   work: a halo's candidate cells are the box [c - R, c + R] per axis, R = edges[nbins] *
//     radius, widened by a margin (axis_range); cell indices are taken modulo G and a box G
//     cells or more wide visits every cell of the axis once.  k_pcand counts each halo's
//     candidates from the cell-start table; a halo with at most `light` candidates is walked
//     by one lane (k_walk_lane), every other becomes ceil(candidates / cap) items, laid out
//     by one exclusive scan, and persistent waves take items (k_walk_wave).  No host round
//     trip per halo or per batch.
//   walk (wave class): the item's thresholds T_b sit in LDS; the wave takes 32 rows at a
//     time, lays their (up to 64) spans end to end with a wave scan and strides over the
//     concatenation -- coalesced fp64 loads, d2, a branch-free search of the thresholds --
//     adding into a per-wave LDS table (64-bit integer adds for the counts, fp64 LDS adds
//     for the sums); at the end of the item one global atomic per non-empty accumulator.
//   rejection: a row of cells whose (x, y) gap to the centre alone exceeds T_nbins is
//     skipped, strictly (row_span has the argument); ASP_PROFILE_PRUNE=0 visits every row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/asp_profiles.h"
#include "asp_host.hpp"
#include "asp_periodic.hpp"
#include "asp_prims.hpp"
#include "asp_wave.hpp"

namespace asp {
namespace {

constexpr int kPBlock = 256;
constexpr int kPWaves = kPBlock / 64;
constexpr int kMaxBins = 64;
constexpr int kMaxProps = 4;
constexpr int kPMaxG = 256;              // cells per axis at most (24-bit cell keys)
constexpr int kPPerCell = 8;             // particles per cell the grid aims at (DESIGN.md §22 sweep)
constexpr long long kPBatch = 1LL << 27; // particles per batch (ASP_PROFILE_BATCH, <= 2^30)
constexpr int kPLight = 32;              // candidates up to which a halo takes the lane class
constexpr int kPItemCap = 1024;          // candidates per wave item (DESIGN.md §22 sweep)
constexpr int kPMaxItems = 1024;         // items per halo at most (the share grows instead)
constexpr int kPWalkBlocks = 2048;       // persistent workgroups of the wave class
constexpr int kRowsPerChunk = 32;        // rows laid end to end at a time (two spans each)

struct PGrid {
    int G, prune;
    double L, halfL, h;
};

// A halo's candidate cells: per axis w cells from (unwrapped) cell lo; w == G: every cell.
struct HBox {
    int lox, wx, loy, wy, loz, wz;
    double cx, cy, cz;
};

struct Span {
    int s0, n0, s1, n1;
};

__device__ __forceinline__ int modg(int v, int G) {
    v %= G;
    return v < 0 ? v + G : v;
}

// The cells of one axis that can hold a member of a halo at c with reach R (>= 0, may be
// +inf).  A member's folded difference on the axis is below t_nbins (1 + 2^-50) in absolute
// value, so its nearest image u lies in [c - R, c + R] up to a few ulp of L; cells come from
// cell_of(), monotone in the coordinate, so cell k is [k h, (k + 1) h) up to a few ulp of L
// (~2^-50 L), and the image's cell index is floor(u G / L), the particle's own cell modulo G
// (a wrapped coordinate equal to L sits in cell G - 1, the upper face of the box: a box
// that reaches it from either side includes that cell).  The box is widened by
// face_margin(h), far more than those roundings and the rounding of c -+ R
// (asp_periodic.hpp), so the cell set is a superset.  A reach of L or more (or a non-finite
// one) takes every cell.
__device__ __forceinline__ void axis_range(double c, double R, const PGrid& g, int& lo, int& w) {
    const double reach = R + face_margin(g.h);
    lo = 0;
    w = g.G;
    if (!(reach < g.L)) return;
    const double a = floor((c - reach) * (double)g.G / g.L);  // in [-G - 1, G]
    const double b = floor((c + reach) * (double)g.G / g.L);  // in [0, 2 G + 1]
    const int ia = (int)a, n = (int)b - ia + 1;
    if (n >= g.G) return;
    lo = ia;
    w = n;
}

__device__ __forceinline__ HBox halo_box(const double* __restrict__ centres, long long j, double R,
                                         const PGrid& g) {
    HBox b;
    b.cx = centres[3 * j];
    b.cy = centres[3 * j + 1];
    b.cz = centres[3 * j + 2];
    axis_range(b.cx, R, g, b.lox, b.wx);
    axis_range(b.cy, R, g, b.loy, b.wy);
    axis_range(b.cz, R, g, b.loz, b.wz);
    return b;
}

// max(0, gap - eps)^2 of the centre to cell lo + k of an axis, or 0 where no bound holds.
// The bound needs the folded difference to be the direct one: a box of w < G cells with
// w h <= L / 2 holds the centre and the cell, so |u - c| <= L / 2 for every image u in the
// cell and the fold leaves it alone.  eps = face_margin(h) covers the cell faces' and the
// difference's roundings (asp_periodic.hpp).
__device__ __forceinline__ double gap2(double c, int lo, int w, int k, const PGrid& g) {
    if (w >= g.G || (double)w * g.h > g.halfL) return 0.0;
    const double f0 = (double)(lo + k) * g.h, f1 = (double)(lo + k + 1) * g.h;
    const double gap = fmax(f0 - c, c - f1) - face_margin(g.h);
    return gap > 0.0 ? gap * gap : 0.0;
}

// Row r = kx wy + ky of a halo's box: the particles of its z-run of cells, one span or two.
// Pruning: a row is empty for the halo when the (x, y) gaps alone put every particle of it
// STRICTLY beyond T_nbins -- the computed d2 of a particle is at least its computed
// dx dx + dy dy, which is at least the reduced gaps' squares.
__device__ __forceinline__ Span row_span(const HBox& b, const PGrid& g, const int* __restrict__ start,
                                         int r, double Tout) {
    Span s = {0, 0, 0, 0};
    const int kx = r / b.wy, ky = r - kx * b.wy;
    if (g.prune && gap2(b.cx, b.lox, b.wx, kx, g) + gap2(b.cy, b.loy, b.wy, ky, g) > Tout) return s;
    const int G = g.G;
    const int base = (modg(b.lox + kx, G) * G + modg(b.loy + ky, G)) * G;
    if (b.wz >= G) {
        s.s0 = start[base];
        s.n0 = start[base + G] - s.s0;
        return s;
    }
    const int zl = modg(b.loz, G), ze = zl + b.wz;
    s.s0 = start[base + zl];
    if (ze <= G) {
        s.n0 = start[base + ze] - s.s0;
    } else {
        s.n0 = start[base + G] - s.s0;
        s.s1 = start[base];
        s.n1 = start[base + ze - G] - s.s1;
    }
    return s;
}

// word |= the centre_bits() of every centre; bit 3: a negative radius, 4: a non-finite one.
__global__ __launch_bounds__(kPBlock) void k_pcheck(const double* __restrict__ c,
                                                     const double* __restrict__ radius, long long m,
                                                     double L, int* __restrict__ word) {
    const long long j = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (j >= m) return;
    int bad = centre_bits(c, j, L);
    if (radius) {
        const double r = radius[j];
        if (!__builtin_isfinite(r)) bad |= 16;
        else if (r < 0.0) bad |= 8;
    }
    if (bad) atomicOr(word, bad);
}

__global__ __launch_bounds__(kPBlock) void k_pkeys(const double* __restrict__ pos, long long n, int G,
                                                    double L, unsigned* __restrict__ keys,
                                                    int* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (i >= n) return;
    const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    unsigned k = (unsigned)G * G * G;
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))
        k = ((unsigned)cell_of(wrap_box(x, L), G, L) * G + cell_of(wrap_box(y, L), G, L)) * G +
            cell_of(wrap_box(z, L), G, L);
    keys[i] = k;
    idx[i] = (int)i;
}

// start[c] = the first sorted position with key >= c, for c in [0, ncell + 1] (keys are in
// [0, ncell]; start[ncell + 1] = n).  Thread i fills the cells between keys i - 1 and i.
__global__ __launch_bounds__(kPBlock) void k_pstart(const unsigned* __restrict__ keys, long long n,
                                                     int ncell, int* __restrict__ start) {
    const long long i = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (i > n) return;
    const int prev = i == 0 ? -1 : (int)keys[i - 1];
    const int cur = i == n ? ncell + 1 : (int)keys[i];
    for (int c = prev + 1; c <= cur; ++c) start[c] = (int)i;
}

// Cell order: wrapped coordinates (x, y, z planes of `stride` doubles), then the properties.
__global__ __launch_bounds__(kPBlock) void k_pgather(const double* __restrict__ pos,
                                                      const double* __restrict__ props, int nprops,
                                                      long long pstride,
                                                      const int* __restrict__ order, long long n,
                                                      double L, double* __restrict__ sorted,
                                                      long long stride) {
    const long long i = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (i >= n) return;
    const long long p = order[i];
    sorted[i] = wrap_box(pos[3 * p], L);
    sorted[stride + i] = wrap_box(pos[3 * p + 1], L);
    sorted[2 * stride + i] = wrap_box(pos[3 * p + 2], L);
    for (int k = 0; k < nprops; ++k) sorted[(3 + k) * stride + i] = props[k * pstride + p];
}

// Candidates of every halo, and its number of wave items (0: the lane class, or nothing).
__global__ __launch_bounds__(kPBlock) void k_pcand(const double* __restrict__ centres,
                                                    const double* __restrict__ radius, long long m,
                                                    double eout, PGrid g,
                                                    const int* __restrict__ start, int light, int cap,
                                                    int max_items, int* __restrict__ cand,
                                                    int* __restrict__ items) {
    const long long j = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (j > m) return;
    if (j == m) {  // (the scan's last element: the total)
        items[j] = 0;
        return;
    }
    const double t = eout * (radius ? radius[j] : 1.0), Tout = t * t;
    const HBox b = halo_box(centres, j, t, g);
    const int nrows = b.wx * b.wy;
    int c = 0;
    for (int r = 0; r < nrows; ++r) {
        const Span s = row_span(b, g, start, r, Tout);
        c += s.n0 + s.n1;
    }
    cand[j] = c;
    items[j] = c <= light ? 0 : min((c + cap - 1) / cap, max_items);
}

// ASP_PROFILE_COUNT: the pairs tested are the candidates of every halo, of either class.
__global__ __launch_bounds__(kPBlock) void k_ptested(const int* __restrict__ cand, long long m,
                                                      unsigned long long* __restrict__ ctr) {
    const long long j = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (j < m && cand[j]) atomicAdd(ctr, (unsigned long long)cand[j]);
}

struct Walk {
    const double* centres;
    const double* radius;
    const double* edges;
    const double* sorted;  // x, y, z, props planes
    long long stride;      // of a plane
    const int* start;
    const int* cand;
    const int* items;      // per halo
    const int* istart;     // their exclusive scan (m + 1)
    unsigned long long* count;
    double* sum;
    long long m;
    int nbins, top;        // top: the largest power of two <= nbins + 1
    PGrid g;
};

// The lane class: one lane walks all of a light halo's candidates; thresholds are formed on
// the fly from the edges (the same two products as the table of the wave class).
template <int NP>
__global__ __launch_bounds__(kPBlock) void k_walk_lane(const Walk W) {
    const long long j = (long long)blockIdx.x * kPBlock + threadIdx.x;
    if (j >= W.m) return;
    const int C = W.cand[j];
    if (C == 0 || W.items[j] != 0) return;
    const int nbins = W.nbins;
    const double rad = W.radius ? W.radius[j] : 1.0;
    const double t0 = W.edges[0] * rad, T0 = t0 * t0;
    const double t1 = W.edges[nbins] * rad, Tout = t1 * t1;
    const HBox b = halo_box(W.centres, j, t1, W.g);
    const double* __restrict__ sx = W.sorted;
    const double* __restrict__ sy = sx + W.stride;
    const double* __restrict__ sz = sy + W.stride;
    const int nrows = b.wx * b.wy;
    for (int r = 0; r < nrows; ++r) {
        const Span s = row_span(b, W.g, W.start, r, Tout);
        for (int half = 0; half < 2; ++half) {
            const int p0 = half ? s.s1 : s.s0, p1 = p0 + (half ? s.n1 : s.n0);
            for (int p = p0; p < p1; ++p) {
                const double d2 = pdist2(sx[p], sy[p], sz[p], b.cx, b.cy, b.cz, W.g.L, W.g.halfL);
                if (!(d2 >= T0 && d2 < Tout)) continue;
                int pos = 0;  // the number of thresholds <= d2: 1 .. nbins here
                for (int step = W.top; step; step >>= 1) {
                    const int q = pos + step;
                    if (q <= nbins) {
                        const double t = W.edges[q - 1] * rad;
                        if (t * t <= d2) pos = q;
                    }
                }
                const long long o = j * nbins + (pos - 1);
                atomicAdd(&W.count[o], 1ull);
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    atomicAdd(&W.sum[(long long)k * W.m * nbins + o], sz[(1 + k) * W.stride + p]);
            }
        }
    }
}

// The wave class: persistent waves over the items.
template <int NP>
__global__ __launch_bounds__(kPBlock) void k_walk_wave(const Walk W) {
    __shared__ double sT[kPWaves][128];  // T_0 .. T_nbins, then +inf
    __shared__ unsigned long long sCnt[kPWaves][kMaxBins];
    __shared__ double sSum[kPWaves][NP ? NP : 1][kMaxBins];
    __shared__ int sPre[kPWaves][65];    // exclusive scan of the chunk's span lengths, and the total
    __shared__ int sSeg[kPWaves][64];    // the spans' first particles
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = gridDim.x * kPWaves;
    const int nbins = W.nbins;
    const int m = (int)W.m;
    const int total = W.istart[m];
    const double* __restrict__ sx = W.sorted;
    const double* __restrict__ sy = sx + W.stride;
    const double* __restrict__ sz = sy + W.stride;
    const double L = W.g.L, halfL = W.g.halfL;
    for (int item = blockIdx.x * kPWaves + wv; item < total; item += nwaves) {
        // the item's halo: the largest j with istart[j] <= item
        int lo = 0, hi = m;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (W.istart[mid] <= item) lo = mid;
            else hi = mid;
        }
        // The halo's number as a lane value: what follows from it (the box, the centre, the
        // item's range) then lives in vector registers -- held as wave-uniform scalars it
        // overflowed the scalar file (SGPR spills).  Every lane holds the same values.
        const int j = __shfl(lo, 0);
        const int nit = W.istart[j + 1] - W.istart[j], C = W.cand[j];
        const int share = (C + nit - 1) / nit;
        // (an item past the halo's last candidate is empty: the share is rounded up)
        const int a = (item - W.istart[j]) * share, e_end = min(C, a + share);
        const double rad = W.radius ? W.radius[j] : 1.0;
        for (int q = lane; q < 128; q += 64) {
            double T = INFINITY;
            if (q <= nbins) {
                const double t = W.edges[q] * rad;
                T = t * t;
            }
            sT[wv][q] = T;
        }
        if (lane < nbins) {
            sCnt[wv][lane] = 0ull;
#pragma nounroll
            for (int k = 0; k < NP; ++k) sSum[wv][k][lane] = 0.0;
        }
        wave_sync();
        const double T0 = sT[wv][0], Tout = sT[wv][nbins];
        const double tout = W.edges[nbins] * rad;
        const HBox b = halo_box(W.centres, j, tout, W.g);
        const int nrows = b.wx * b.wy;
        int off = 0;  // candidates of the rows before the chunk
        for (int r0 = 0; r0 < nrows && off < e_end; r0 += kRowsPerChunk) {
            const int r = r0 + (lane >> 1);
            Span s = {0, 0, 0, 0};
            if (r < nrows) s = row_span(b, W.g, W.start, r, Tout);
            const int first = (lane & 1) ? s.s1 : s.s0, len = (lane & 1) ? s.n1 : s.n0;
            // (written out: wave_incl_scan() here changes the kernel's register assignment,
            // and that form was not timed -- DESIGN.md §23)
            int incl = len;
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            const int tot = __shfl(incl, 63);
            if (off + tot > a) {
                wave_sync();  // (the previous chunk's readers are done)
                sPre[wv][lane] = incl - len;
                sSeg[wv][lane] = first;
                if (lane == 63) sPre[wv][64] = tot;
                wave_sync();
                const int e1 = min(e_end - off, tot);
                int seg = 0;
                for (int e = max(a - off, 0) + lane; e < e1; e += 64) {
                    while (e >= sPre[wv][seg + 1]) ++seg;  // e < tot = sPre[64]: seg <= 63
                    const int p = sSeg[wv][seg] + (e - sPre[wv][seg]);
                    const double d2 = pdist2(sx[p], sy[p], sz[p], b.cx, b.cy, b.cz, L, halfL);
                    if (!(d2 >= T0 && d2 < Tout)) continue;
                    int pos = 0;  // the number of thresholds <= d2 (the table ends in +inf)
                    for (int step = W.top; step; step >>= 1)
                        if (sT[wv][pos + step - 1] <= d2) pos += step;
                    atomicAdd(&sCnt[wv][pos - 1], 1ull);
#pragma nounroll
                    for (int k = 0; k < NP; ++k)
                        atomicAdd(&sSum[wv][k][pos - 1], sz[(1 + k) * W.stride + p]);
                }
            }
            off += tot;
        }
        wave_sync();
        unsigned long long c = 0ull;
        if (lane < nbins) c = sCnt[wv][lane];
        if (c) {
            const long long o = (long long)j * nbins + lane;
            atomicAdd(&W.count[o], c);
#pragma nounroll
            for (int k = 0; k < NP; ++k)
                atomicAdd(&W.sum[(long long)k * W.m * nbins + o], sSum[wv][k][lane]);
        }
        wave_sync();  // (the table is zeroed for the next item)
    }
}

template <int NP>
int launch_walks(const Walk& W, unsigned lane_grid, unsigned wave_grid, hipStream_t st) {
    hipLaunchKernelGGL(k_walk_lane<NP>, dim3(lane_grid), dim3(kPBlock), 0, st, W);
    ASP_LAUNCHED();
    hipLaunchKernelGGL(k_walk_wave<NP>, dim3(wave_grid), dim3(kPBlock), 0, st, W);
    ASP_LAUNCHED();
    return ASP_OK;
}

int check_edges(const double* e, int nbins) {
    for (int b = 0; b <= nbins; ++b) {
        if (!std::isfinite(e[b])) return fail(ASP_ERR_INVALID, "an edge is not finite");
        if (b == 0 && e[0] < 0.0) return fail(ASP_ERR_INVALID, "edges[0] is negative");
        if (b > 0 && !(e[b] > e[b - 1]))
            return fail(ASP_ERR_INVALID, "edges are not strictly ascending");
    }
    return ASP_OK;
}

int profiles(const double* pos, const double* props, int nprops, long long n, const double* centres,
             const double* radius, long long m, const double* edges, int nbins, double L,
             long long* count, double* sum, int flags, int device, hipStream_t st) {
    if (flags & ~(ASP_F_DEVICE_PTRS | ASP_F_ACCUMULATE))
        return fail(ASP_ERR_INVALID, "asp_halo_profiles takes ASP_F_DEVICE_PTRS and ASP_F_ACCUMULATE only");
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (m < 0) return fail(ASP_ERR_INVALID, "m < 0");
    if (nprops < 0 || nprops > kMaxProps) return fail(ASP_ERR_INVALID, "nprops must be in [0, 4]");
    if (nbins < 1 || nbins > kMaxBins) return fail(ASP_ERR_INVALID, "nbins must be in [1, 64]");
    if (!(L > 0.0) || !std::isfinite(L))
        return fail(ASP_ERR_INVALID, "box_width must be finite and > 0");
    if (!edges) return fail(ASP_ERR_INVALID, "NULL edges");
    if (n > 0 && !pos) return fail(ASP_ERR_INVALID, "NULL positions");
    if (n > 0 && nprops > 0 && !props) return fail(ASP_ERR_INVALID, "NULL props with nprops > 0");
    if (m > 0 && !centres) return fail(ASP_ERR_INVALID, "NULL centres");
    if (m > 0 && !count) return fail(ASP_ERR_INVALID, "NULL count");
    if (m > 0 && nprops > 0 && !sum) return fail(ASP_ERR_INVALID, "NULL sum with nprops > 0");
    const bool dev = flags & ASP_F_DEVICE_PTRS, acc = flags & ASP_F_ACCUMULATE;
    double he[kMaxBins + 1];
    if (!dev) {
        std::memcpy(he, edges, (size_t)(nbins + 1) * sizeof(double));
        ASP_TRY(check_edges(he, nbins));
    }
    if (m >= (1LL << 31) || m * nbins >= (1LL << 31))
        return fail(ASP_ERR_UNSUPPORTED, "m * nbins >= 2^31 accumulators per call");
    if (m == 0) return ASP_OK;
    const size_t nacc = (size_t)m * nbins;
    if (n == 0 && !dev) {
        if (!acc) {
            std::memset(count, 0, nacc * sizeof(long long));
            if (nprops) std::memset(sum, 0, nacc * nprops * sizeof(double));
        }
        return ASP_OK;
    }
    return with_workspace(device, st, false, [&](Workspace& ws, hipStream_t st) -> int {
        if (ws.prof) ASP_TRY(prof_next(ws));
        stats_clear(ws);
        Buf* B = ws.profiles;

        // ---- the haloes: edges on the host, everything on the device, checked ----
        StageMark mprep(ws, kSNearestPrep, st);
        const double *dc = centres, *dr = radius, *de = edges;
        if (dev) {
            ASP_HIP(hipMemcpyAsync(he, edges, (size_t)(nbins + 1) * sizeof(double),
                                   hipMemcpyDeviceToHost, st));
            ASP_HIP(hipStreamSynchronize(st));
            ASP_TRY(check_edges(he, nbins));
        } else {
            ASP_TRY(to_device(ws, B[kProfCentres], dc, (size_t)m * 3 * sizeof(double), st, Copy::kPlain));
            if (radius)
                ASP_TRY(to_device(ws, B[kProfRadius], dr, (size_t)m * sizeof(double), st, Copy::kPlain));
            ASP_TRY(to_device(ws, B[kProfEdges], de, (size_t)(nbins + 1) * sizeof(double), st,
                              Copy::kPlain));
        }
        const unsigned hgrid = (unsigned)((m + 1 + kPBlock - 1) / kPBlock);  // m + 1 threads
        int bad = 0;
        {
            ASP_TRY(ensure(B[kProfCheck], sizeof(int)));
            int* word = (int*)B[kProfCheck].p;
            ASP_HIP(hipMemsetAsync(word, 0, sizeof(int), st));
            hipLaunchKernelGGL(k_pcheck, dim3(hgrid), dim3(kPBlock), 0, st, dc, dr, m, L, word);
            ASP_LAUNCHED();
            ASP_HIP(hipMemcpyAsync(&bad, word, sizeof(int), hipMemcpyDeviceToHost, st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        ASP_TRY(centre_error(bad));
        if (bad & 16) return fail(ASP_ERR_INVALID, "a radius is not finite");
        if (bad & 8) return fail(ASP_ERR_INVALID, "a radius is negative");

        // ---- the accumulators ----
        long long* dcount = count;
        double* dsum = sum;
        if (!dev) {
            ASP_TRY(device_scratch(B[kProfCount], dcount, nacc * sizeof(long long)));
            if (nprops) ASP_TRY(device_scratch(B[kProfSum], dsum, nacc * nprops * sizeof(double)));
            if (acc) {
                ASP_HIP(hipMemcpyAsync(dcount, count, nacc * sizeof(long long), hipMemcpyHostToDevice, st));
                if (nprops)
                    ASP_HIP(hipMemcpyAsync(dsum, sum, nacc * nprops * sizeof(double),
                                           hipMemcpyHostToDevice, st));
            }
        }
        if (!acc) {
            ASP_HIP(hipMemsetAsync(dcount, 0, nacc * sizeof(long long), st));
            if (nprops) ASP_HIP(hipMemsetAsync(dsum, 0, nacc * nprops * sizeof(double), st));
        }
        mprep.done();

        // ---- the knobs (read per call) ----
        const long long NB = std::min(std::max(n, 1LL),
                                      (long long)env_int("ASP_PROFILE_BATCH", kPBatch, 1, 1LL << 30));
        const int light = (int)env_int("ASP_PROFILE_LIGHT", kPLight, 0, INT_MAX);
        const int cap = (int)env_int("ASP_PROFILE_ITEM", kPItemCap, 1, 1 << 30);
        const int prune = env_int("ASP_PROFILE_PRUNE", 1) != 0;
        const int gforce = (int)env_int("ASP_PROFILE_CELLS", 0, 0, kPMaxG);
        const int max_items = (int)std::max(1LL, std::min((long long)kPMaxItems, 0x7fffffffLL / (m + 1)));
        DiagCounter tested;
        ASP_TRY(tested.begin("ASP_PROFILE_COUNT", B[kProfCounters], st));
        unsigned long long* const ctr = tested.p;

        // ---- the batches ----
        ASP_TRY(ensure(B[kProfCand], (size_t)(m + 1) * sizeof(int)));
        ASP_TRY(ensure(B[kProfItems], (size_t)(m + 1) * 2 * sizeof(int)));
        int* cand = (int*)B[kProfCand].p;
        int* items = (int*)B[kProfItems].p;
        int* istart = items + (m + 1);
        ASP_TRY(ensure(B[kProfKeys], (size_t)NB * 2 * sizeof(unsigned)));
        ASP_TRY(ensure(B[kProfIndex], (size_t)NB * 2 * sizeof(int)));
        ASP_TRY(ensure(B[kProfSorted], (size_t)NB * (3 + nprops) * sizeof(double)));
        unsigned* kin = (unsigned*)B[kProfKeys].p;
        unsigned* kout = kin + NB;
        int* iin = (int*)B[kProfIndex].p;
        int* iout = iin + NB;
        double* sorted = (double*)B[kProfSorted].p;
        if (!dev && n > 0) {
            ASP_TRY(ensure(B[kProfPos], (size_t)NB * 3 * sizeof(double)));
            if (nprops) ASP_TRY(ensure(B[kProfProps], (size_t)NB * nprops * sizeof(double)));
        }
        int top = 1;
        while (top * 2 <= nbins + 1) top *= 2;
        for (long long a = 0; a < n; a += NB) {
            const long long nb = std::min(NB, n - a);
            const double* dpos = pos + 3 * a;
            const double* dprops = props ? props + a : nullptr;
            long long pstride = n;
            if (!dev) {
                ASP_TRY(to_device(ws, B[kProfPos], dpos, (size_t)nb * 3 * sizeof(double), st, Copy::kPlain));
                if (nprops) {
                    double* staged = (double*)B[kProfProps].p;
                    for (int k = 0; k < nprops; ++k)
                        ASP_HIP(hipMemcpyAsync(staged + (size_t)k * NB, props + (size_t)k * n + a,
                                               (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
                    dprops = staged;
                    pstride = NB;
                }
            }
            StageMark mbatch(ws, kSNearestPrep, st);
            PGrid g;
            g.G = gforce ? gforce
                         : std::max(1, std::min(kPMaxG, (int)std::floor(std::cbrt((double)nb / kPPerCell))));
            g.prune = prune;
            g.L = L;
            g.halfL = 0.5 * L;
            g.h = L / (double)g.G;
            const int ncell = g.G * g.G * g.G;  // and cell `ncell`: the non-finite rows
            int key_bits = 1;
            while ((1LL << key_bits) <= ncell) ++key_bits;
            ASP_TRY(ensure(B[kProfCellStart], (size_t)(ncell + 2) * sizeof(int)));
            int* start = (int*)B[kProfCellStart].p;
            const unsigned pgrid = (unsigned)((nb + kPBlock - 1) / kPBlock);
            hipLaunchKernelGGL(k_pkeys, dim3(pgrid), dim3(kPBlock), 0, st, dpos, nb, g.G, L, kin, iin);
            ASP_LAUNCHED();
            ASP_TRY(sort_pairs(B[kProfSortTmp], kin, kout, iin, iout, (size_t)nb, key_bits, st));
            hipLaunchKernelGGL(k_pstart, dim3((unsigned)((nb + 1 + kPBlock - 1) / kPBlock)), dim3(kPBlock), 0,
                               st, (const unsigned*)kout, nb, ncell, start);
            ASP_LAUNCHED();
            hipLaunchKernelGGL(k_pgather, dim3(pgrid), dim3(kPBlock), 0, st, dpos, dprops, nprops, pstride,
                               (const int*)iout, nb, L, sorted, nb);
            ASP_LAUNCHED();
            hipLaunchKernelGGL(k_pcand, dim3(hgrid), dim3(kPBlock), 0, st, dc, dr, m, he[nbins], g,
                               (const int*)start, light, cap, max_items, cand, items);
            ASP_LAUNCHED();
            ASP_TRY(exclusive_scan_int(B[kProfScanTmp], (const int*)items, istart, (size_t)(m + 1), st));
            if (ctr) {
                hipLaunchKernelGGL(k_ptested, dim3(hgrid), dim3(kPBlock), 0, st, (const int*)cand, m, ctr);
                ASP_LAUNCHED();
            }
            mbatch.done();

            StageMark mwalk(ws, kSNearestSearch, st);
            Walk W;
            W.centres = dc;
            W.radius = dr;
            W.edges = de;
            W.sorted = sorted;
            W.stride = nb;
            W.start = start;
            W.cand = cand;
            W.items = items;
            W.istart = istart;
            W.count = (unsigned long long*)dcount;
            W.sum = dsum;
            W.m = m;
            W.nbins = nbins;
            W.top = top;
            W.g = g;
            const unsigned lgrid = (unsigned)((m + kPBlock - 1) / kPBlock);
            const unsigned wgrid = (unsigned)std::min<long long>(
                kPWalkBlocks, (m * (long long)max_items + kPWaves - 1) / kPWaves);
            switch (nprops) {
                case 0: ASP_TRY(launch_walks<0>(W, lgrid, wgrid, st)); break;
                case 1: ASP_TRY(launch_walks<1>(W, lgrid, wgrid, st)); break;
                case 2: ASP_TRY(launch_walks<2>(W, lgrid, wgrid, st)); break;
                case 3: ASP_TRY(launch_walks<3>(W, lgrid, wgrid, st)); break;
                default: ASP_TRY(launch_walks<4>(W, lgrid, wgrid, st)); break;
            }
            mwalk.done();
        }
        if (!dev) {
            ASP_TRY(to_host(count, dcount, nacc * sizeof(long long), st));
            if (nprops) ASP_TRY(to_host(sum, dsum, nacc * nprops * sizeof(double), st));
        }
        ASP_TRY(tested.end(ws, st));
        if (!dev) ASP_HIP(hipStreamSynchronize(st));
        stats_publish(ws, device);
        return ASP_OK;
    });
}

}  // namespace
}  // namespace asp

using namespace asp;

extern "C" int asp_halo_profiles(const double* positions, const double* props, int32_t nprops,
                                 int64_t n, const double* centres, const double* radius, int64_t m,
                                 const double* edges, int32_t nbins, double box_width,
                                 int64_t* count, double* sum, int32_t flags, int32_t device,
                                 void* stream) {
    t_err.clear();
    return profiles(positions, props, nprops, n, centres, radius, m, edges, nbins, box_width,
                    (long long*)count, sum, flags, device, (hipStream_t)stream);
}
