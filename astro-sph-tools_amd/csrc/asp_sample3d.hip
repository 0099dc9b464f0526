// asp_sample3d.hip -- SPH sums at arbitrary 3-D points (field values at positions,
// sightline profiles): asp_sample3d, asp_sample3d_f64 (include/asp_points.h).
//
// asp_project3d's voxel test at M arbitrary positions instead of the corners of a voxel
// lattice: out[k] = sum_p a[p] W(r, h_p) over the particles with
// r2 = (dx dx + dy dy) + dz dz < (2 h_p) (2 h_p), every quantity of the test in fp64, in
// this order, without contraction.  The method is the 2-D sampler's (asp_sample.hip,
// DESIGN.md §20) with one more axis; all but the deposit kernel's walk is
// the same code (asp_sample.hpp):
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
//   finalise: k_sfinal.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/asp_points.h"
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

template <int KID, int NOUT, int ACC, bool F64>
__global__ __launch_bounds__(kSBlock) void k_sample3(const Part<3> P, long long n,
                                                      const SDescT<3>* __restrict__ D, int G,
                                                      int wide_cells, int wide_points, int walk,
                                                      int mix, const Points<3> S,
                                                      unsigned long long* __restrict__ pairs) {
    const int* __restrict__ start = S.start;
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const auto [c, R] = particle_record<3, KID, NOUT, ACC, F64>(P, p, n, D, G);
    const int cx0 = c[0].lo, cx1 = c[0].hi, cy0 = c[1].lo, cy1 = c[1].hi, cz0 = c[2].lo, cz1 = c[2].hi;
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
                for (int j = a; j < b; ++j) pair<3, KID, NOUT, ACC>(R, S, j);
                tested += (unsigned long long)(b - a);
            }
    }
    // the wave's wide particles, one after the other (every lane of the wave gets here)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const Rec<3> Q = from_lane(R, l);
        const Span qx = from_lane(c[0], l), qy = from_lane(c[1], l), qz = from_lane(c[2], l);
        const int x0 = qx.lo, x1 = qx.hi, y0 = qy.lo, y1 = qy.hi, z0 = qz.lo, z1 = qz.hi;
        const int ny = y1 - y0 + 1, nrows = (x1 - x0 + 1) * ny;
        if (walk == kWalkRow) {
            for (int cx = x0; cx <= x1; ++cx)
                for (int cy = y0; cy <= y1; ++cy) {
                    const int base = (cx * G + cy) * G;
                    const int a = start[base + z0], b = start[base + z1 + 1];
                    for (int j = a + lane; j < b; j += 64) pair<3, KID, NOUT, ACC>(Q, S, j);
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
            // inclusive scan of the lengths over the wave (written out: wave_incl_scan() here
            // changes the kernel's register assignment, and that form was not timed --
            // DESIGN.md §23)
            int inc = len;
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
                    for (int j = ai + lane; j < bi; j += 64) pair<3, KID, NOUT, ACC>(Q, S, j);
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
                if (t < total) pair<3, KID, NOUT, ACC>(Q, S, ai + (t - ei));
            }
            if (lane == 0) tested += (unsigned long long)total;
        }
    }
    count_pairs(tested, lane, pairs);
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

// What the driver (sample_driver, asp_sample.hpp) needs of this unit.
struct Sample3 {
    static constexpr const char* name = "asp_sample3d";
    static constexpr int kMaxG = kMaxG3;
    static int cells(long long m) { return (int)std::ceil(std::cbrt((double)m / kPerCell3)); }
    static int check_kernel(int kid) {
        if (kid == ASP_KERNEL_CUBIC_SPLINE_COLUMN || kid == ASP_KERNEL_WENDLAND_C2_COLUMN)
            return fail(ASP_ERR_INVALID, "the column kernels (ids 3, 4) have no 3-D form");
        if (kid < 0 || kid > ASP_KERNEL_INDICATOR) return fail(ASP_ERR_INVALID, "unknown kernel_id");
        return ASP_OK;
    }
    struct Knobs {
        int wide_cells, wide_points, walk, mix;
    };
    static Knobs knobs() {
        return {(int)env_int("ASP_SAMPLE_WIDE_CELLS", kWideCells3, 0, INT_MAX),
                (int)env_int("ASP_SAMPLE_WIDE_POINTS", kWidePoints3, 0, INT_MAX),
                (int)env_int("ASP_SAMPLE3D_WALK", kWalkFlat, kWalkRow, kWalkFlat),
                (int)env_int("ASP_SAMPLE3D_WALK_MIX", kWalkMix, 0, 1 << 20)};
    }
    template <class F>
    static int dispatch(int kid, int nout, bool det, F&& f) {
        return dispatch3(kid, nout, det, f);
    }
    template <bool F64>
    static int deposit(int kid, int nout, bool det, unsigned grid, hipStream_t st, const Part<3>& P,
                       long long nb, const SDescT<3>* D, int G, const Knobs& K, const Points<3>& S,
                       unsigned long long* pairs) {
        return dispatch3(kid, nout, det, [&](auto KI, auto NO, auto AC) -> int {
            hipLaunchKernelGGL((k_sample3<decltype(KI)::value, decltype(NO)::value, decltype(AC)::value, F64>),
                               dim3(grid), dim3(kSBlock), 0, st, P, nb, D, G, K.wide_cells, K.wide_points,
                               K.walk, K.mix, S, pairs);
            ASP_LAUNCHED();
            return ASP_OK;
        });
    }
};

}  // namespace asp

using namespace asp;

extern "C" int asp_sample3d(const float* x, const float* y, const float* z, const float* h,
                            const float* a0, const float* a1, int64_t n, const double* px,
                            const double* py, const double* pz, int64_t m, int32_t kernel_id,
                            int32_t flags, float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    const SampleArgs<3> A{{{x, y, z}, h, a0, a1, nullptr, nullptr, nullptr, nullptr}, 0, n, {{px, py, pz}},
                          m, kernel_id, flags, out0, out1};
    return sample_driver<3, false, Sample3>(A, device, (hipStream_t)stream);
}

extern "C" int asp_sample3d_f64(const double* positions, const double* h, const double* a0,
                                const double* a1, int64_t n, const double* px, const double* py,
                                const double* pz, int64_t m, int32_t kernel_id, int32_t flags,
                                float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    const SampleArgs<3> A{{{nullptr, nullptr, nullptr}, nullptr, nullptr, nullptr, positions, h, a0, a1}, 0,
                          n, {{px, py, pz}}, m, kernel_id, flags, out0, out1};
    return sample_driver<3, true, Sample3>(A, device, (hipStream_t)stream);
}
