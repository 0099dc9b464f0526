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
// This unit holds k_sample's walk and the 2-D grid rule; the rest is asp_sample.hpp, shared
// with the 3-D sampler (asp_sample3d.hip) and, with the 2-D thresholds, with the spectra
// (asp_spectra.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/asp.h"
#include "asp_sample.hpp"

namespace asp {

template <int KID, int NOUT, int ACC, bool F64>
__global__ __launch_bounds__(kSBlock) void k_sample(const Part<2> P, long long n,
                                                     const SDescT<2>* __restrict__ D, int G,
                                                     int wide_cells, int wide_points,
                                                     const int* __restrict__ start,
                                                     const double* __restrict__ sx,
                                                     const double* __restrict__ sy, long long m,
                                                     unsigned long long* __restrict__ acc,
                                                     unsigned long long* __restrict__ pairs) {
    // (the sorted points as separate arguments, for __restrict__: as one struct argument
    // every instantiation needs 6-12 more SGPRs)
    const Points<2> S{start, {sx, sy}, m, acc};
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const auto [c, R] = particle_record<2, KID, NOUT, ACC, F64>(P, p, n, D, G);
    const int cx0 = c[0].lo, cx1 = c[0].hi, cy0 = c[1].lo, cy1 = c[1].hi;
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
            for (int j = a; j < b; ++j) pair<2, KID, NOUT, ACC>(R, S, j);
            tested += (unsigned long long)(b - a);
        }
    }
    // the wave's wide particles, one after the other, 64 lanes over each span
    unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const Rec<2> Q = from_lane(R, l);
        const Span qx = from_lane(c[0], l), qy = from_lane(c[1], l);
        for (int cx = qx.lo; cx <= qx.hi; ++cx) {
            const int a = start[cx * G + qy.lo], b = start[cx * G + qy.hi + 1];
            for (int j = a + lane; j < b; j += 64) pair<2, KID, NOUT, ACC>(Q, S, j);
            if (lane == 0) tested += (unsigned long long)(b - a);
        }
    }
    count_pairs(tested, lane, pairs);
}

// What the driver (sample_driver, asp_sample.hpp) needs of this unit.
struct Sample2 {
    static constexpr const char* name = "asp_sample2d";
    static constexpr int kMaxG = kSampleMaxG;
    static int cells(long long m) { return (int)std::ceil(std::sqrt((double)m / kSamplePerCell)); }
    static int check_kernel(int kid) {
        if (kid < 0 || kid > ASP_KERNEL_WENDLAND_C2_COLUMN) return fail(ASP_ERR_INVALID, "unknown kernel_id");
        return ASP_OK;
    }
    struct Knobs {
        int wide_cells, wide_points;
    };
    static Knobs knobs() {
        return {(int)env_int("ASP_SAMPLE_WIDE_CELLS", kSampleWideCells, 0, INT_MAX),
                (int)env_int("ASP_SAMPLE_WIDE_POINTS", kSampleWidePoints, 0, INT_MAX)};
    }
    template <class F>
    static int dispatch(int kid, int nout, bool det, F&& f) {
        return asp::dispatch(kid, nout, det, f);
    }
    template <bool F64>
    static int deposit(int kid, int nout, bool det, unsigned grid, hipStream_t st, const Part<2>& P,
                       long long nb, const SDescT<2>* D, int G, const Knobs& K, const Points<2>& S,
                       unsigned long long* pairs) {
        return asp::dispatch(kid, nout, det, [&](auto KI, auto NO, auto AC) -> int {
            hipLaunchKernelGGL((k_sample<decltype(KI)::value, decltype(NO)::value, decltype(AC)::value, F64>),
                               dim3(grid), dim3(kSBlock), 0, st, P, nb, D, G, K.wide_cells, K.wide_points,
                               S.start, S.s[0], S.s[1], S.m, S.acc, pairs);
            ASP_LAUNCHED();
            return ASP_OK;
        });
    }
};

}  // namespace asp

using namespace asp;

extern "C" int asp_sample2d(const float* u, const float* v, const float* h, const float* a0,
                            const float* a1, int64_t n, const double* px, const double* py,
                            int64_t m, int32_t kernel_id, int32_t flags, float* out0, float* out1,
                            int32_t device, void* stream) {
    t_err.clear();
    const SampleArgs<2> A{{{u, v}, h, a0, a1, nullptr, nullptr, nullptr, nullptr}, 0, n, {{px, py}}, m,
                          kernel_id, flags, out0, out1};
    return sample_driver<2, false, Sample2>(A, device, (hipStream_t)stream);
}

extern "C" int asp_sample2d_f64(const double* positions, const double* h, const double* a0,
                                const double* a1, int64_t n, int32_t axis, const double* px,
                                const double* py, int64_t m, int32_t kernel_id, int32_t flags,
                                float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    const SampleArgs<2> A{{{nullptr, nullptr}, nullptr, nullptr, nullptr, positions, h, a0, a1}, axis, n,
                          {{px, py}}, m, kernel_id, flags, out0, out1};
    return sample_driver<2, true, Sample2>(A, device, (hipStream_t)stream);
}
