// asp_spectra.hip -- sightline spectra: SPH columns deposited in velocity bins
// (asp_spectra2d, asp_spectra2d_f64; include/asp_spectra.h has the definition).
//
// Every included (particle, sightline) pair of asp_sample2d spreads its column N_ps over the
// velocity bins of the sightline's row with the bin-averaged Gaussian of the particle's
// Doppler width.  MI355X layout:
//   prep (stage sample_prep): the 2-D sampler's, unchanged -- sample_prep<2> of asp_sample.hpp.
//   deposit (stage spectra_deposit; k_spectra): pairs are found as k_sample finds them, a lane
//     per particle or the wave per particle.  An included pair owns a contiguous run of
//     accumulators in ONE row, so the lane that found it does not walk them: the pairs a wave
//     step includes are compacted into LDS (ballot + lane count), and the wave takes them one
//     after the other, its 64 lanes striding over the pair's bins -- one wave-instruction adds
//     64 neighbouring 8-byte words.  Each lane evaluates erf at its bin's lower edge only; the
//     upper edge is the next lane's value (the last lane's: the next 64 edges' first, computed
//     one step ahead).  ASP_SPECTRA_WALK=0 is the other form, for comparison: the lane that
//     found the pair walks its bins.
//     Velocity arithmetic is fp64 throughout (erf differences lose all relative accuracy in
//     fp32 when dv << b); adds are no-return global fp64 atomics (-munsafe-fp-atomics).
//   finalise (same stage; k_spfinal): emit_pixel per accumulator -- conversion, accumulate and
//     ratio -- with the rows back in the caller's order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/asp_spectra.h"
#include "asp_sample.hpp"
#include "asp_wave.hpp"

namespace asp {

// Half-width of the visited bins in units of b: erfc(5) = 1.54e-12 <= 2^-36.
constexpr double kSpecT = ASP_SPECTRA_T;

// The velocity axis of a call.
struct VelBins {
    double v0, dv, half_inv_dv;  // edge_j = v0 + j dv; 1 / (2 dv)
    int K, ring;
};
// The velocity arrays of a call or of a batch (b as fp32 or as fp64, by entry point).
struct Vel {
    const double* vc;
    const float* b;
    const double* b64;
};
// A particle's run of bins: edges base + i, i = 0 .. len, into bins k0 + i (ring: mod K);
// len == 0: not admitted, or no bin of the window is met.
struct VRec {
    double vc, binv, base;
    int len, k0;
};

template <bool F64>
__device__ __forceinline__ VRec vel_record(const Vel& V, long long p, const VelBins& W) {
    VRec r = {};
    const double vc = V.vc[p];
    double b;
    if constexpr (F64) b = V.b64[p];
    else b = (double)V.b[p];
    const double hw = kSpecT * b;
    if (!(__builtin_isfinite(vc) && __builtin_isfinite(b) && b > 0.0 && hw / W.dv < 0x1p24)) return r;
    // the bins that meet [vc - T b, vc + T b]; the ends moved outwards by 2^-40 of the operands,
    // far above the roundings of the two expressions
    const double pad = 0x1p-40 * (fabs(vc) + fabs(W.v0) + hw);
    double jlo = floor((((vc - hw) - pad) - W.v0) / W.dv);
    double jhi = floor((((vc + hw) + pad) - W.v0) / W.dv);
    if (W.ring) {
        // (beyond 2^52 the edges v0 + j dv are no longer distinct numbers)
        if (!(fabs(jlo) < 0x1p52 && fabs(jhi) < 0x1p52)) return r;
        const double k0 = jlo - (double)W.K * floor(jlo / (double)W.K);  // exact: |jlo| < 2^52
        r.k0 = min(max((int)k0, 0), W.K - 1);
    } else {
        jlo = fmax(jlo, 0.0);
        jhi = fmin(jhi, (double)(W.K - 1));
        if (!(jlo <= jhi)) return r;
        r.k0 = (int)jlo;
    }
    r.vc = vc;
    r.binv = 1.0 / b;
    r.base = jlo;
    r.len = (int)(jhi - jlo) + 1;  // <= 2 (2^24 + 1) + 1 (ring) or K (window)
    return r;
}

__device__ __forceinline__ VRec from_lane(const VRec& r, int l) {
    return {__shfl(r.vc, l), __shfl(r.binv, l), __shfl(r.base, l), __shfl(r.len, l), __shfl(r.k0, l)};
}

// erf at edge i of a run, (edge - vc) / b with edge = v0 + (base + i) dv in fp64.
__device__ __forceinline__ double edge_erf(const VelBins& W, double vc, double binv, double base, int i) {
    return erf(((W.v0 + (base + (double)i) * W.dv) - vc) * binv);
}

// One pair's run, the wave's 64 lanes over its bins.  WRAP: the run passes the ring's end.
template <int NOUT, bool WRAP>
__device__ __forceinline__ void wave_run(const VelBins& W, double n0, double n1, double vc, double binv,
                                         double base, int len, int k0, int lane, double* row0,
                                         double* row1) {
    double e = edge_erf(W, vc, binv, base, lane);
    for (int i0 = 0; i0 < len; i0 += 64) {
        const bool more = i0 + 64 <= len;  // edge i0 + 64 exists: the last lane's upper edge
        const double en = more ? edge_erf(W, vc, binv, base, i0 + 64 + lane) : 0.0;
        double up = __shfl_down(e, 1);
        const double first = __shfl(en, 0);
        if (lane == 63) up = first;
        const int i = i0 + lane;
        if (i < len) {
            const double g = (up - e) * W.half_inv_dv;
            int k = k0 + i;
            if constexpr (WRAP) k %= W.K;
            atomicAdd(row0 + k, n0 * g);
            if constexpr (NOUT == 2) atomicAdd(row1 + k, n1 * g);
        }
        e = en;
    }
}

// ... and the other form (ASP_SPECTRA_WALK=0): the lane walks the run of its own pair.
template <int NOUT>
__device__ __forceinline__ void lane_run(const VelBins& W, double n0, double n1, const VRec& v,
                                         double* row0, double* row1) {
    double e = edge_erf(W, v.vc, v.binv, v.base, 0);
    int k = v.k0;
    for (int i = 0; i < v.len; ++i) {
        const double up = edge_erf(W, v.vc, v.binv, v.base, i + 1);
        const double g = (up - e) * W.half_inv_dv;
        atomicAdd(row0 + k, n0 * g);
        if constexpr (NOUT == 2) atomicAdd(row1 + k, n1 * g);
        e = up;
        if (++k == W.K) k = 0;  // (window runs end at K - 1)
    }
}

// The included pairs of one wave step, in LDS.
struct PairQueue {
    double vc[64], binv[64], base[64];
    float n0[64], n1[64];
    int row[64], len[64], k0[64];
};

// One wave step: lane `in` holds an included pair (terms t0 / t1, point j, run v).  The
// wave's included pairs go through the queue and are deposited one after the other (walk), or
// every lane deposits its own.  Called by the whole wave.
template <int NOUT>
__device__ __forceinline__ void deposit_step(bool in, float t0, float t1, int j, const VRec& v,
                                             PairQueue& Q, int lane, int walk, const VelBins& W,
                                             double* acc, long long mk) {
    if (!walk) {
        if (in) {
            double* row = acc + (long long)j * W.K;
            lane_run<NOUT>(W, (double)t0, (double)t1, v, row, row + mk);
        }
        return;
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
    if (!mask) return;
    if (in) {
        const int s = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        Q.vc[s] = v.vc;
        Q.binv[s] = v.binv;
        Q.base[s] = v.base;
        Q.n0[s] = t0;
        Q.n1[s] = t1;
        Q.row[s] = j;
        Q.len[s] = v.len;
        Q.k0[s] = v.k0;
    }
    wave_sync();
    const int cnt = __builtin_popcountll(mask);
    for (int s = 0; s < cnt; ++s) {
        const int len = Q.len[s], k0 = Q.k0[s];
        double* row = acc + (long long)Q.row[s] * W.K;
        const double n0 = (double)Q.n0[s], n1 = NOUT == 2 ? (double)Q.n1[s] : 0.0;
        if (k0 + len > W.K)
            wave_run<NOUT, true>(W, n0, n1, Q.vc[s], Q.binv[s], Q.base[s], len, k0, lane, row, row + mk);
        else
            wave_run<NOUT, false>(W, n0, n1, Q.vc[s], Q.binv[s], Q.base[s], len, k0, lane, row, row + mk);
    }
    wave_sync();  // the queue is rewritten by the next step
}

template <int KID, int NOUT, bool F64>
__global__ __launch_bounds__(kSBlock) void k_spectra(const Part<2> P, const Vel V, long long n,
                                                      const SDescT<2>* __restrict__ D, int G,
                                                      int wide_cells, int wide_points,
                                                      const int* __restrict__ start,
                                                      const double* __restrict__ sx,
                                                      const double* __restrict__ sy, long long m,
                                                      double* __restrict__ acc, const VelBins W,
                                                      int walk, unsigned long long* __restrict__ counters) {
    __shared__ PairQueue queues[kSBlock / 64];
    PairQueue& Q = queues[threadIdx.x >> 6];
    const Points<2> S{start, {sx, sy}, m, nullptr};
    const long long mk = m * W.K;  // the second sum's accumulators follow the first's
    const long long p = (long long)blockIdx.x * kSBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const auto [c, R] = particle_record<2, KID, NOUT, kAccF64, F64>(P, p, n, D, G);
    const int cx0 = c[0].lo, cx1 = c[0].hi, cy0 = c[1].lo, cy1 = c[1].hi;
    VRec v = {};
    if (cx0 <= cx1) v = vel_record<F64>(V, p, W);
    const bool live = v.len > 0;
    bool wide = live && (cx1 - cx0 + 1) * (cy1 - cy0 + 1) > wide_cells;
    int j = 0, je = 0, cx = cx0;
    if (live && !wide) {  // few cells, but crowded ones: the wave takes those as well
        j = start[cx0 * G + cy0];
        je = start[cx0 * G + cy1 + 1];
        int npts = je - j;
        for (int x = cx0 + 1; x <= cx1; ++x) npts += start[x * G + cy1 + 1] - start[x * G + cy0];
        wide = npts > wide_points;
    }
    unsigned long long tested = 0ull, adds = 0ull;
    // narrow particles: every lane steps through its own spans, one candidate per wave step
    bool have = live && !wide;
    for (;;) {
        while (have && j >= je) {  // the next row's span
            if (++cx > cx1) {
                have = false;
            } else {
                j = start[cx * G + cy0];
                je = start[cx * G + cy1 + 1];
            }
        }
        if (!__builtin_amdgcn_ballot_w64(have)) break;
        float w = 0.0f;
        const bool in = have && pair_shape<2, KID>(R, S, j, w);
        deposit_step<NOUT>(in, R.s0 * w, R.s1 * w, j, v, Q, lane, walk, W, acc, mk);
        if (have) {
            ++j;
            ++tested;
        }
        if (in) adds += (unsigned long long)v.len;
    }
    // the wave's wide particles, one after the other, 64 lanes over each span
    unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const Rec<2> Qr = from_lane(R, l);
        const VRec qv = from_lane(v, l);
        const Span qx = from_lane(c[0], l), qy = from_lane(c[1], l);
        for (int x = qx.lo; x <= qx.hi; ++x) {
            const int a = start[x * G + qy.lo], b = start[x * G + qy.hi + 1];
            for (int j0 = a; j0 < b; j0 += 64) {
                const int jj = j0 + lane;
                float w = 0.0f;
                const bool in = jj < b && pair_shape<2, KID>(Qr, S, jj, w);
                deposit_step<NOUT>(in, Qr.s0 * w, Qr.s1 * w, jj, qv, Q, lane, walk, W, acc, mk);
                if (in) adds += (unsigned long long)qv.len;
            }
            if (lane == 0) tested += (unsigned long long)(b - a);
        }
    }
    count_pairs(tested, lane, counters);
    count_pairs(adds, lane, counters ? counters + 1 : nullptr);
}

// Accumulators (rows in cell order) -> fp32 outputs, rows in the caller's order: emit_pixel,
// as k_sfinal, per (sightline, bin).
template <int NOUT>
__global__ __launch_bounds__(kSBlock) void k_spfinal(const unsigned long long* __restrict__ acc,
                                                      long long m, int K, const int* __restrict__ perm,
                                                      float* __restrict__ out0,
                                                      float* __restrict__ out1, int flags) {
    const long long i = (long long)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= m * K) return;
    const long long j = i / K;
    const int k = (int)(i - j * K);
    emit_pixel<NOUT, kAccF64>((long long)perm[j] * K + k, acc[i], NOUT == 2 ? acc[m * K + i] : 0ull, 0, 0,
                              out0, out1, flags);
}

// The 2-D sampler's grid rule, thresholds and kernel ids (sample_check, sample_prep).
struct Spectra2 {
    static constexpr const char* name = "asp_spectra2d";
    static constexpr int kMaxG = kSampleMaxG;
    static int cells(long long m) { return (int)std::ceil(std::sqrt((double)m / kSamplePerCell)); }
    static int check_kernel(int kid) {
        if (kid < 0 || kid > ASP_KERNEL_WENDLAND_C2_COLUMN) return fail(ASP_ERR_INVALID, "unknown kernel_id");
        return ASP_OK;
    }
};

struct SpectraArgs {
    SampleArgs<2> A;
    Vel vel;
    double v0, dv;
    int nbins, ring;
};

template <bool F64>
int spectra_driver(const SpectraArgs& X, int device, hipStream_t stream) {
    const SampleArgs<2>& A = X.A;
    if (!(std::isfinite(X.dv) && X.dv > 0.0)) return fail(ASP_ERR_INVALID, "dv must be finite and > 0");
    if (!std::isfinite(X.v0)) return fail(ASP_ERR_INVALID, "v0 must be finite");
    if (X.nbins < 1) return fail(ASP_ERR_INVALID, "nbins < 1");
    if (X.ring != 0 && X.ring != 1) return fail(ASP_ERR_INVALID, "ring must be 0 or 1");
    ASP_TRY((sample_check<2, Spectra2>(A, F64)));
    if (A.flags & ASP_F_DETERMINISTIC)
        return fail(ASP_ERR_UNSUPPORTED, "ASP_F_DETERMINISTIC is not supported by asp_spectra2d");
    if (A.n > 0 && (!X.vel.vc || !(F64 ? (const void*)X.vel.b64 : (const void*)X.vel.b)))
        return fail(ASP_ERR_INVALID, "NULL particle array");
    if (A.m * (long long)X.nbins > 0x7fffffffLL)
        return fail(ASP_ERR_UNSUPPORTED, "m * nbins >= 2^31 accumulators per call");
    if (A.m == 0) return ASP_OK;
    const bool dev = A.flags & ASP_F_DEVICE_PTRS;
    const bool acc_flag = A.flags & ASP_F_ACCUMULATE;
    const int nout = A.out1 ? 2 : 1;
    const long long m = A.m, n = A.n, K = X.nbins;
    const size_t obytes = (size_t)(m * K) * sizeof(float);
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
        SGrid<2> g;
        ASP_TRY((sample_prep<2, Spectra2>(ws, st, A, (size_t)K, g)));
        const int wide_cells = (int)env_int("ASP_SAMPLE_WIDE_CELLS", kSampleWideCells, 0, INT_MAX);
        const int wide_points = (int)env_int("ASP_SAMPLE_WIDE_POINTS", kSampleWidePoints, 0, INT_MAX);
        const int walk = env_int("ASP_SPECTRA_WALK", 1) != 0;
        const VelBins W{X.v0, X.dv, 0.5 / X.dv, X.nbins, X.ring};
        double* acc = (double*)g.S.acc;
        unsigned long long* counters = nullptr;  // ASP_SAMPLE_COUNT: pairs tested, (pair, bin) adds
        if (env_set("ASP_SAMPLE_COUNT")) {
            ASP_TRY(device_scratch(ws.aux[kAuxCounters], counters, 2 * sizeof(*counters)));
            ASP_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(*counters), st));
        }
        StageMark mzero(ws, kSSpectraDeposit, st);
        ASP_HIP(hipMemsetAsync(acc, 0, (size_t)nout * m * K * sizeof(double), st));
        mzero.done();

        // ---- the particles, batch by batch, into the same accumulators ----
        ASP_TRY(for_batches(n, [&](long long a, long long b, int) -> int {
            Part<2> P;
            ASP_TRY((stage_batch<2, F64>(ws, A, a, b, st, P)));
            Vel V{X.vel.vc + a, F64 ? nullptr : X.vel.b + a, F64 ? X.vel.b64 + a : nullptr};
            if (!dev) {
                const size_t nb = (size_t)(b - a);
                ASP_TRY(to_device(ws, ws.sample[kSmpVc], V.vc, nb * sizeof(double), st, Copy::kPinned));
                if constexpr (F64)
                    ASP_TRY(to_device(ws, ws.sample[kSmpB], V.b64, nb * sizeof(double), st, Copy::kPinned));
                else
                    ASP_TRY(to_device(ws, ws.sample[kSmpB], V.b, nb * sizeof(float), st, Copy::kPinned));
            }
            const unsigned grid = (unsigned)((b - a + kSBlock - 1) / kSBlock);
            StageMark mk(ws, kSSpectraDeposit, st);
            ASP_TRY(asp::dispatch(A.kid, nout, false, [&](auto KI, auto NO, auto) -> int {
                hipLaunchKernelGGL((k_spectra<decltype(KI)::value, decltype(NO)::value, F64>), dim3(grid),
                                   dim3(kSBlock), 0, st, P, V, b - a, (const SDescT<2>*)g.D, g.G, wide_cells,
                                   wide_points, g.S.start, g.S.s[0], g.S.s[1], m, acc, W, walk, counters);
                ASP_LAUNCHED();
                return ASP_OK;
            }));
            mk.done();
            return ASP_OK;
        }));

        // ---- finalise ----
        const int kflags = (acc_flag ? kFlagAccumulate : 0) | ((A.flags & ASP_F_RATIO) ? kFlagRatio : 0);
        const unsigned fgrid = (unsigned)((m * K + kSBlock - 1) / kSBlock);
        StageMark mfin(ws, kSSpectraDeposit, st);
        hipLaunchKernelGGL((nout == 2 ? k_spfinal<2> : k_spfinal<1>), dim3(fgrid), dim3(kSBlock), 0, st,
                           (const unsigned long long*)g.S.acc, m, (int)K, g.perm, g.d0, g.d1, kflags);
        ASP_LAUNCHED();
        mfin.done();
        if (!dev) {
            ASP_TRY(to_host(A.out0, g.d0, obytes, st));
            if (A.out1) ASP_TRY(to_host(A.out1, g.d1, obytes, st));
        }
        if (counters) {
            unsigned long long e[2] = {0, 0};
            ASP_HIP(hipMemcpyAsync(e, counters, sizeof(e), hipMemcpyDeviceToHost, st));
            ASP_HIP(hipStreamSynchronize(st));
            ws.stats[9] = (long long)e[0];
            ws.stats[10] = (long long)e[1];
        }
        if (!dev) ASP_HIP(hipStreamSynchronize(st));
        stats_publish(ws, device);
        return ASP_OK;
    });
}

}  // namespace asp

using namespace asp;

extern "C" int asp_spectra2d(const float* u, const float* v, const float* h, const float* a0,
                             const float* a1, const double* vc, const float* b, int64_t n,
                             const double* px, const double* py, int64_t m, double v0, double dv,
                             int32_t nbins, int32_t ring, int32_t kernel_id, int32_t flags, float* out0,
                             float* out1, int32_t device, void* stream) {
    t_err.clear();
    const SpectraArgs X{{{{u, v}, h, a0, a1, nullptr, nullptr, nullptr, nullptr}, 0, n, {{px, py}}, m,
                         kernel_id, flags, out0, out1},
                        {vc, b, nullptr}, v0, dv, nbins, ring};
    return spectra_driver<false>(X, device, (hipStream_t)stream);
}

extern "C" int asp_spectra2d_f64(const double* positions, const double* h, const double* a0,
                                 const double* a1, const double* vc, const double* b, int64_t n,
                                 int32_t axis, const double* px, const double* py, int64_t m, double v0,
                                 double dv, int32_t nbins, int32_t ring, int32_t kernel_id, int32_t flags,
                                 float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    const SpectraArgs X{{{{nullptr, nullptr}, nullptr, nullptr, nullptr, positions, h, a0, a1}, axis, n,
                         {{px, py}}, m, kernel_id, flags, out0, out1},
                        {vc, nullptr, b}, v0, dv, nbins, ring};
    return spectra_driver<true>(X, device, (hipStream_t)stream);
}
