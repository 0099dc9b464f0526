// asp_map_bin.hip -- the binning kernels of the 2-D map and their launchers: K1 count,
// K3 scatter, K3b tile scale (the pipeline's overview is in asp_project2d.hip; the scans
// K2a / K2b between count and scatter are asp_binning.hpp's, launched by the driver).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map.hpp"
#include "asp_map_device.hpp"

namespace asp {

// Vector of U floats (one 4 U-byte load per lane).
template <int U>
using vecf = float __attribute__((ext_vector_type(U)));

// Load U CONSECUTIVE particles per lane with one U-wide load per array when the arrays
// are 4 U-byte aligned (`al`); h = 0 past the end, which has no footprint.
template <int U>
__device__ __forceinline__ void load_vec(const float* __restrict__ a, long long p, long long p1,
                                         bool al, float* out) {
    if (al && p + U <= p1) {
        vecf<U> x = *(const vecf<U>*)(a + p);
#pragma unroll
        for (int k = 0; k < U; ++k) out[k] = x[k];
    } else {
#pragma unroll
        for (int k = 0; k < U; ++k) out[k] = p + k < p1 ? a[p + k] : 0.0f;
    }
}
template <int U>
__device__ __forceinline__ bool aligned_vec(const void* a, const void* b, const void* c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & (4 * U - 1)) == 0;
}

template <int U>
__device__ __forceinline__ void load_batch(const float* __restrict__ u, const float* __restrict__ v,
                                           const float* __restrict__ h, long long base,
                                           long long p1, bool al, float* pu, float* pv,
                                           float* ph) {
    long long p = base + (long long)threadIdx.x * U;
    load_vec<U>(u, p, p1, al, pu);
    load_vec<U>(v, p, p1, al, pv);
    load_vec<U>(h, p, p1, al, ph);
}

// Histogram column of a (particle, tile) insertion: t (small / mid-size stream) or
// t + ntiles (large stream, gathered by K4g).  `maybe`: the unclipped box is large.
__device__ __forceinline__ int column(const Grid& g, const Box& b, bool maybe, int tx, int ty) {
    const int t = tx * g.nty + ty;
    return maybe && box_large(tile_box(b, tx, ty), g) ? t + g.ntiles : t;
}
__device__ __forceinline__ bool maybe_large(const Grid& g, const Box& b) {
    const int bw = b.x1 - b.x0 + 1, bh = b.y1 - b.y0 + 1;  // unclipped: an upper bound
    return (bw >= g.gather_min && bh >= g.gather_min) || (long long)bw * bh >= g.gather_area;
}

// ----------------------------------------------------------------------------------
// K1: count insertions per (block, tile)
// ----------------------------------------------------------------------------------
template <bool CULL>
__global__ __launch_bounds__(kCountBlock) void k_count(const float* __restrict__ u,
                                                       const float* __restrict__ v,
                                                       const float* __restrict__ h,
                                                       long long n, long long nblk, Grid g,
                                                       Src64 s, int* __restrict__ hist,
                                                       int* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) int lh[];  // 2 * ntiles columns
    for (int t = threadIdx.x; t < 2 * g.ntiles; t += kCountBlock) lh[t] = 0;
    __syncthreads();
    int nwide = 0;
    const long long p0 = (long long)blockIdx.x * kBatch, stride = nblk * kBatch;
    // Software pipeline: the next batch's loads are in flight while this batch is binned.
    float pu[kCountUnroll], pv[kCountUnroll], ph[kCountUnroll];
    const bool al = aligned_vec<kCountUnroll>(u, v, h);
    load_batch<kCountUnroll>(u, v, h, p0, n, al, pu, pv, ph);
    for (long long base = p0; base < n; base += stride) {
        float nu[kCountUnroll], nv[kCountUnroll], nh[kCountUnroll];
        load_batch<kCountUnroll>(u, v, h, base + stride, n, al, nu, nv, nh);
#pragma unroll
        for (int k = 0; k < kCountUnroll; ++k) {
            Box b;
            const int p = (int)(base + (long long)threadIdx.x * kCountUnroll + k);
            if (!footprint<CULL>(g, s, p, pu[k], pv[k], ph[k], b)) continue;
            int tx0 = b.x0 >> kTileShift, tx1 = b.x1 >> kTileShift;
            int ty0 = b.y0 >> kTileShift, ty1 = b.y1 >> kTileShift;
            if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > g.wide_tiles) {
                ++nwide;
                continue;
            }
            const bool mb = maybe_large(g, b);
            if (tx1 - tx0 <= 1 && ty1 - ty0 <= 1) {
                // at most 2 x 2 tiles (every pixel-scale particle): straight-line, so a wave
                // pays for the second column / row only when one of its lanes needs it
                atomicAdd(&lh[column(g, b, mb, tx0, ty0)], 1);
                if (tx1 > tx0) atomicAdd(&lh[column(g, b, mb, tx1, ty0)], 1);
                if (ty1 > ty0) {
                    atomicAdd(&lh[column(g, b, mb, tx0, ty1)], 1);
                    if (tx1 > tx0) atomicAdd(&lh[column(g, b, mb, tx1, ty1)], 1);
                }
            } else {
                for (int tx = tx0; tx <= tx1; ++tx)
                    for (int ty = ty0; ty <= ty1; ++ty) atomicAdd(&lh[column(g, b, mb, tx, ty)], 1);
            }
        }
#pragma unroll
        for (int k = 0; k < kCountUnroll; ++k) {
            pu[k] = nu[k];
            pv[k] = nv[k];
            ph[k] = nh[k];
        }
    }
    if (nwide) atomicAdd(&ctr[cWideCount], nwide);
    __syncthreads();
    int* row = hist + (long long)blockIdx.x * 2 * g.ntiles;
    for (int t = threadIdx.x; t < 2 * g.ntiles; t += kCountBlock) row[t] = lh[t];
}

// Record stores of the scatter: plain stores (non-temporal ones measured 2x slower, the
// L2 merges the 32-B halves of a line).
__device__ __forceinline__ void rec_store(float4* dst, float4 v) {
    // one global_store_dwordx4 per half record: the empty asm keeps the vectorizer from
    // regrouping two halves as dwordx3 + unaligned dwordx4 + dword
    *dst = v;
    asm volatile("" ::: "memory");
}

template <int NOUT>
__device__ __forceinline__ void load_props(const float* __restrict__ a0,
                                           const float* __restrict__ a1, long long base,
                                           long long p1, bool al, float* pa0, float* pa1) {
    long long p = base + (long long)threadIdx.x * kUnroll;
    load_vec<kUnroll>(a0, p, p1, al, pa0);
    if constexpr (NOUT == 2) {
        load_vec<kUnroll>(a1, p, p1, al, pa1);
    } else {
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) pa1[k] = 0.0f;
    }
}

// ----------------------------------------------------------------------------------
// K3: scatter records into their tiles' runs.  Same particle partition as K1.
// The PREPARED record (32 B, both map counts): {u, v, h, c0}, {c1, p, band, box} --
// c = a * norm(h) the fp32 term coefficients, p the particle index (the fp64 re-decision
// reads the caller's arrays there), band the error band of §3, box the candidate box
// clipped to the tile (4 tile-local bytes).  The deposit's per-record set-up is done
// here, where the store-bound scatter has VALU to spare.  Also the per-(block, tile) max
// |c| (fp32 bits) of the records it inserted, the fixed-point bound of K3b.
// ----------------------------------------------------------------------------------
// SRC: where the record frame's exact coordinates come from -- 0: the fp32 arrays (fp32
// callers), 1: the resident fp64 arrays, loaded with the batch (s.u64 != null), 2: decided
// per particle (src_u: the chunk-cull kernels).  0 and 1 keep loads out of the per-particle
// branches (the fp32 kernels carry no fp64 load path at all).
// PROBE: 1 for the placement trials' launches (the same code under its own name, so that
// profiles of the steady state show them apart).
// Per-wave staging of the paired record stores: first halves at [lane], second halves at
// [72 + lane] (8 float4 apart: neither the b128 writes nor the b128 reads conflict).
constexpr int kStageF4 = 136;

template <int KID, int NOUT, int ACC, bool CULL, int SRC, int PROBE, int NX = 0>
__global__ __launch_bounds__(kScatterBlock) void k_scatter(
    const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ h,
    const float* __restrict__ a0, const float* __restrict__ a1, long long n, long long nblk,
    Grid g, Src64 s, const int* __restrict__ hist, const long long* __restrict__ tile_start,
    const int* __restrict__ tile_total, float4* __restrict__ recs, unsigned* __restrict__ cmx,
    int* __restrict__ wide_list, int* __restrict__ ctr, int grp, long long rec_cap,
    int wide_cap, int verify, XArgs xa) {
    // Speculative launch (enqueued before the host has read the counters): the record and
    // wide-list buffers were sized by an earlier call; if this call needs more, every
    // workgroup leaves at once and the host relaunches after growing them.
    if (ctr[cRecs] > rec_cap || ctr[cWideCount] > wide_cap) {
        if (verify && threadIdx.x == 0) atomicOr(&ctr[cLayoutBad], 1);
        return;
    }
    // No record is stored outside the buffer, whatever the cursors say: with a reused
    // layout (verify) they are the previous call's, and this call's particles may differ.
    // One unsigned compare: a cursor that wrapped below zero is outside as well.
    const unsigned slot_cap = (unsigned)min(rec_cap, (long long)0x7fffffff);
    // absolute record cursors: the small / mid-size stream, then the large one
    extern __shared__ __attribute__((aligned(16))) int cur[];
    // per-wave staging for the paired record stores: 64 records x 32 B (second halves
    // 8 float4 further on, so neither the b128 writes nor the b128 reads conflict)
    float4* stage = (float4*)(cur + 2 * g.ntiles);
    unsigned* cm = (unsigned*)(stage + (kScatterBlock / 64) * kStageF4);
    // this workgroup takes over count workgroups grp * sb ..: its cursors start at the
    // prefix row of the first of them
    const long long sb = blockIdx.x;
    const int* row = hist + sb * grp * 2 * g.ntiles;
    for (int t = threadIdx.x; t < 2 * g.ntiles; t += kScatterBlock)
        cur[t] = (int)tile_start[t] + row[t];  // n_recs < 2^31 (checked on the host)
    if constexpr (ACC == kAccFix)
        for (int t = threadIdx.x; t < g.ntiles * NOUT; t += kScatterBlock) cm[t] = 0u;
    __syncthreads();
    // the batches of count workgroups sb * grp .. (< nblk), in order: batch q * nblk +
    // sb * grp + r for r < gcnt, q = 0, 1, ...  The loop steps (q, r) and carries the batch's
    // first particle index c: a division by gcnt per batch made the compiler emit two
    // 64-bit divisions per iteration (SALU was 147 instructions per wave and iteration,
    // round 6).  One batch per iteration: 2 and 4 batches measured slower (1.794 / 1.918 vs
    // 1.756 ms, round 5, DESIGN_LOG.md §18) -- the scatter is bound by its stores, not by
    // load latency.  Lane particle k of the batch at c: c + k * kScatterBlock + threadIdx.x
    // (coalesced dword loads).  Every load is unconditional -- index clamped to the last
    // particle, h = 0 past the end (no footprint) -- so the compiler can count the loads in
    // flight: with load_vec's vector-or-scalar branches it put s_waitcnt vmcnt(0) right after
    // issuing the NEXT batch's loads.
    const long long gcnt = min((long long)grp, nblk - sb * grp);
    auto base_of = [&](long long q, long long r) { return (q * nblk + sb * grp + r) * kBatch; };
    constexpr int kLane = kUnroll;
    auto pidx = [&](long long b, int k) {
        return b + (long long)k * kScatterBlock + threadIdx.x;
    };
    auto ld = [&](const float* __restrict__ a, long long c, float* out) {
#pragma unroll
        for (int k = 0; k < kLane; ++k) out[k] = a[min(pidx(c, k), n - 1)];
    };
    // Software pipeline: issue the next iteration's loads BEFORE this one's record stores.
    float pu[kLane], pv[kLane], ph[kLane], pa0[kLane], pa1[kLane];
    double pU[kLane], pV[kLane];  // SRC 1: the exact coordinates
    // SRC 1: the fp64 coordinates of the lane's particles (index clamped to the array:
    // unconditional loads; lanes past the end are never binned)
    auto load_src = [&](long long c, double* dU, double* dV) {
        if constexpr (SRC == 1) {
#pragma unroll
            for (int k = 0; k < kLane; ++k) {
                const long long q = min(pidx(c, k), n - 1) * s.stride;
                dU[k] = s.u64[q];
                dV[k] = s.v64[q];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kLane; ++k) dU[k] = dV[k] = 0.0;
        }
    };
    auto load_all = [&](long long c, float* du, float* dv, float* dh, float* d0, float* d1) {
        ld(u, c, du);
        ld(v, c, dv);
        ld(h, c, dh);
        ld(a0, c, d0);
        if constexpr (NOUT == 2) ld(a1, c, d1);
        else
#pragma unroll
            for (int k = 0; k < kLane; ++k) d1[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < kLane; ++k) dh[k] = pidx(c, k) < n ? dh[k] : 0.0f;
    };
    int first_slot[kLane];
    // the prepared fields of every particle's first record (the paired store's payload)
    float first_c0[kLane], first_c1[kLane], first_band[kLane], first_lu[kLane],
        first_lv[kLane];
    unsigned first_box[kLane];
#pragma unroll
    for (int k = 0; k < kLane; ++k) {
        first_slot[k] = -1;
        first_c0[k] = first_c1[k] = first_band[k] = first_lu[k] = first_lv[k] = 0.0f;
        first_box[k] = 0u;
    }
    // NX: properties 2..5, loaded with the batch (software-pipelined like the others)
    float px[NX ? 4 : 1][kLane];
    auto load_x = [&](long long c, float (&dst)[NX ? 4 : 1][kLane]) {
        if constexpr (NX) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ld(xa.a[j], c, dst[j]);
        }
    };
    long long bq = 0, br = 0;
    auto step_batch = [&]() {
        const bool wrap = br + 1 == gcnt;
        bq += wrap ? 1 : 0;
        br = wrap ? 0 : br + 1;
        return base_of(bq, br);
    };
    long long c = base_of(0, 0);  // the current batch's first particle
    load_all(c, pu, pv, ph, pa0, pa1);
    load_src(c, pU, pV);
    load_x(c, px);
    while (c < n) {
        const long long cn = step_batch();  // the next batch to load
        float nu[kLane], nv[kLane], nh[kLane], na0[kLane], na1[kLane];
        load_all(cn, nu, nv, nh, na0, na1);
        double nU[kLane], nV[kLane];
        load_src(cn, nU, nV);
        float nx_[NX ? 4 : 1][kLane];
        load_x(cn, nx_);
#pragma unroll
        for (int k = 0; k < kLane; ++k) {
            const int p = (int)pidx(c, k);
            Box b;
            if (!footprint<CULL>(g, s, p, pu[k], pv[k], ph[k], b)) continue;
            // the fixed-point bound is taken over the same fp32 coefficients the deposit
            // scales
            const float cf0 = (float)term_coef<KID>(pa0[k], ph[k]);
            const float cf1 = NOUT == 2 ? (float)term_coef<KID>(pa1[k], ph[k]) : 0.0f;
            float4 cx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (NX)
                cx = make_float4((float)term_coef<KID>(px[0][k], ph[k]),
                                 (float)term_coef<KID>(px[1][k], ph[k]),
                                 (float)term_coef<KID>(px[2][k], ph[k]),
                                 (float)term_coef<KID>(px[3][k], ph[k]));
            unsigned c0 = 0u, c1 = 0u;
            if constexpr (ACC == kAccFix) {
                c0 = __float_as_uint(fabsf(cf0));
                c1 = __float_as_uint(fabsf(cf1));
            }
            int tx0 = b.x0 >> kTileShift, tx1 = b.x1 >> kTileShift;
            int ty0 = b.y0 >> kTileShift, ty1 = b.y1 >> kTileShift;
            if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > g.wide_tiles) {
                const int w = atomicAdd(&ctr[cWideCursor], 1);
                if ((unsigned)w < (unsigned)wide_cap) wide_list[w] = p;
                if constexpr (ACC == kAccFix) {
                    atomicMax((unsigned*)&ctr[cWideMax0], c0);
                    if (NOUT == 2) atomicMax((unsigned*)&ctr[cWideMax1], c1);
                }
                continue;
            }
            const float band = rec_band(g.mgl, ph[k]);  // decided in the box-origin frame
            // coordinates relative to the record's box origin, from the exact inputs: the
            // deposit's pair arithmetic then carries 2^-24 of the pair distance, not of |u|
            // 
            const double U = SRC == 0 ? (double)pu[k] : SRC == 1 ? pU[k] : src_u(s, p, pu[k]);
            const double V = SRC == 0 ? (double)pv[k] : SRC == 1 ? pV[k] : src_v(s, p, pv[k]);
            first_c0[k] = cf0;
            first_c1[k] = cf1;
            first_band[k] = band;
            first_lu[k] = (float)(U - corner_x(g, max(b.x0, tx0 * kTile)));
            first_lv[k] = (float)(V - corner_y(g, max(b.y0, ty0 * kTile)));
            const bool mb = maybe_large(g, b);
            auto insert = [&](int tx, int ty, bool first) {
                const int t = tx * g.nty + ty;
                const unsigned bp = tile_box(b, tx, ty);
                const int col = mb && box_large(bp, g) ? t + g.ntiles : t;
                int slot = atomicAdd(&cur[col], 1);
                // (props passes never verify: they scatter after the read-back, ext sized from
                // the counters, and slot_cap is then no bound; a props pass that reused a
                // layout would have to pass ext's capacity here)
                if constexpr (NX) {
                    if ((unsigned)slot < slot_cap) rec_store(&xa.ext[slot], cx);
                }
                if constexpr (ACC == kAccFix) {
                    atomicMax(&cm[t * NOUT], c0);
                    if (NOUT == 2) atomicMax(&cm[t * NOUT + 1], c1);
                }
                if (first) {
                    first_slot[k] = slot;  // written by the paired store below
                    first_box[k] = bp;
                } else if ((unsigned)slot < slot_cap) {
                    rec_store(&recs[2 * (long long)slot],
                              make_float4((float)(U - corner_x(g, max(b.x0, tx * kTile))),
                                          (float)(V - corner_y(g, max(b.y0, ty * kTile))),
                                          ph[k], cf0));
                    rec_store(&recs[2 * (long long)slot + 1],
                              make_float4(cf1, __int_as_float(p), band, __uint_as_float(bp)));
                }
            };
            if (tx1 - tx0 <= 1 && ty1 - ty0 <= 1) {  // at most 2 x 2 tiles: straight-line
                insert(tx0, ty0, true);
                if (tx1 > tx0) insert(tx1, ty0, false);
                if (ty1 > ty0) {
                    insert(tx0, ty1, false);
                    if (tx1 > tx0) insert(tx1, ty1, false);
                }
            } else {
                for (int tx = tx0; tx <= tx1; ++tx)
                    for (int ty = ty0; ty <= ty1; ++ty) insert(tx, ty, tx == tx0 && ty == ty0);
            }
        }
        // Paired store of every particle's first record: lanes 2j and 2j+1 write the two
        // 16-B halves of record j, so one store instruction covers 32 whole 32-B records
        // (32 lines) instead of 64 half records (64 lines).
        float4* st = stage + (threadIdx.x >> 6) * kStageF4;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < kLane; ++k) {
            const int p = (int)pidx(c, k);
            st[lane] = make_float4(first_lu[k], first_lv[k], ph[k], first_c0[k]);
            st[72 + lane] = make_float4(first_c1[k], __int_as_float(p), first_band[k],
                                        __uint_as_float(first_box[k]));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                int src = half * 32 + (lane >> 1);
                int slot = __shfl(first_slot[k], src);
                float4 val = st[(lane & 1) * 72 + src];
                if ((unsigned)slot < slot_cap)
                    rec_store(&recs[2 * (long long)slot + (lane & 1)], val);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            first_slot[k] = -1;
        }
#pragma unroll
        for (int k = 0; k < kLane; ++k) {
            pu[k] = nu[k];
            pv[k] = nv[k];
            ph[k] = nh[k];
            pa0[k] = na0[k];
            pa1[k] = na1[k];
            pU[k] = nU[k];
            pV[k] = nV[k];
        }
        if constexpr (NX)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < kLane; ++k) px[j][k] = nx_[j][k];
        c = cn;
    }
    __syncthreads();
    if constexpr (ACC == kAccFix) {
        unsigned* out = cmx + (long long)blockIdx.x * g.ntiles * NOUT;  // per scatter block
        for (int t = threadIdx.x; t < g.ntiles * NOUT; t += kScatterBlock) out[t] = cm[t];
    }
    // The proof of a reused layout: every column's cursor stands where this workgroup's
    // run must end -- where the next scatter workgroup's begins (the prefix row of its
    // first count workgroup), or at the end of the tile's run for the last one.  Equal for
    // every (scatter workgroup, column), and the wide count equal (checked behind the
    // kernel), the layout is the one a count pass over THESE particles makes.
    if (verify) {
        const bool last = sb + 1 == gridDim.x;
        const int* next = hist + (sb + 1) * grp * 2 * g.ntiles;
        int bad = 0;
        for (int t = threadIdx.x; t < 2 * g.ntiles; t += kScatterBlock) {
            const int end = (int)tile_start[t] + (last ? tile_total[t] : next[t]);
            bad |= cur[t] != end;
        }
        if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&ctr[cLayoutBad], 1);
    }
}

// ----------------------------------------------------------------------------------
// K3b: per tile, max over blocks of cmx -> fixed-point exponents tile_k[t] = {k0, k1}.
// ----------------------------------------------------------------------------------
template <int NOUT>
__global__ __launch_bounds__(kBlock) void k_tilescale(const unsigned* __restrict__ cmx, int nblk,
                                                      int ntiles, const int* __restrict__ tile_total,
                                                      int2* __restrict__ tile_k,
                                                      const int* __restrict__ guard) {
    if (layout_rejected(guard)) return;
    __shared__ unsigned part[4][64][NOUT];
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int t = blockIdx.x * 64 + lane;
    int b0 = (int)((long long)nblk * w / 4), b1 = (int)((long long)nblk * (w + 1) / 4);
    unsigned m[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) m[o] = 0u;
    if (t < ntiles)
        for (int b = b0; b < b1; ++b)
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
                m[o] = max(m[o], cmx[((long long)b * ntiles + t) * NOUT + o]);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) part[w][lane][o] = m[o];
    __syncthreads();
    if (w == 0 && t < ntiles) {
        int k[2] = {0, 0};
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            unsigned mm = max(max(part[0][lane][o], part[1][lane][o]),
                              max(part[2][lane][o], part[3][lane][o]));
            k[o] = scale_exp((long long)tile_total[t] + tile_total[t + ntiles],
                             __uint_as_float(mm));
        }
        tile_k[t] = make_int2(k[0], k[1]);
    }
}

static inline size_t scatter_lds_base(const Grid& g) {
    return (size_t)2 * g.ntiles * sizeof(int) + (size_t)(kScatterBlock / 64) * kStageF4 * sizeof(float4);
}
static inline size_t scatter_lds(const Grid& g, int nout, bool det) {
    return scatter_lds_base(g) + (det ? (size_t)g.ntiles * nout * sizeof(unsigned) : 0);
}

int launch_count(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, const float* u,
                 const float* v, const float* h, hipStream_t st) {
    StageMark m(ws, kSCount, st);
    hipLaunchKernelGGL(g.nonsquare || g.mixed ? k_count<true> : k_count<false>,
                       dim3((unsigned)pl.nblk), dim3(kCountBlock),
                       (size_t)2 * g.ntiles * sizeof(int), st, u, v, h, pl.n, pl.nblk, g, s,
                       (int*)ws.hist.p, (int*)ws.counters.p);
    ASP_LAUNCHED();
    m.done();
    return ASP_OK;
}

// K3 on stream st.
template <int KID, int NOUT, int ACC, bool CULL, int SRC, int PROBE, int NX>
static int scatter_variant(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl,
                           const float* u, const float* v, const float* h, const float* a0,
                           const float* a1, long long rec_cap, int wide_cap, hipStream_t st,
                           bool verify, const XArgs& xa) {
    int* dc = (int*)ws.counters.p;
    const size_t lds = scatter_lds(g, NOUT, ACC == kAccFix);
    hipLaunchKernelGGL((k_scatter<KID, NOUT, ACC, CULL, SRC, PROBE, NX>), dim3((unsigned)pl.nblk_s),
                       dim3(kScatterBlock), lds, st, u, v, h, a0,
                       a1, pl.n, pl.nblk, g, s, (const int*)ws.hist.p,
                       (const long long*)ws.tile_start.p, (const int*)ws.tile_total.p,
                       (float4*)ws.recs.p, (unsigned*)ws.cmx.p, (int*)ws.wide.p, dc, pl.grp,
                       rec_cap, wide_cap, verify ? 1 : 0, xa);
    ASP_LAUNCHED();
    return ASP_OK;
}

int launch_scatter(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid, int nout,
                   bool det, const float* u, const float* v, const float* h, const float* a0,
                   const float* a1, long long rec_cap, int wide_cap, hipStream_t st, bool probe,
                   const XArgs* xa, bool verify) {
    StageMark m(ws, kSScatter, st);
    const XArgs none{};
    ASP_TRY(dispatch(kid, nout, det, [&](auto K, auto N, auto A) {
        // (CULL, SRC) from the grid and the source arrays, for the given (PROBE, NX)
        auto launch = [&](auto P, auto X) {
            auto go = [&](auto C, auto S) {
                constexpr int nx = decltype(X)::value;
                return scatter_variant<K(), N(), A(), decltype(C)::value, decltype(S)::value,
                                       decltype(P)::value, nx>(g, s, ws, pl, u, v, h, a0, a1,
                                                               rec_cap, wide_cap, st, verify,
                                                               nx ? *xa : none);
            };
            return g.nonsquare || g.mixed ? go(std::true_type{}, Int<2>{})
                   : s.u64                ? go(std::false_type{}, Int<1>{})
                                          : go(std::false_type{}, Int<0>{});
        };
        if constexpr (N() == 2 && A() == kAccF64) {
            if (xa) return launch(Int<0>{}, Int<1>{});
        }
        return probe ? launch(Int<1>{}, Int<0>{}) : launch(Int<0>{}, Int<0>{});
    }));
    m.done();
    return ASP_OK;
}

int launch_tilescale(const Grid& g, Workspace& ws, const Plan& pl, int nout, hipStream_t st,
                     const int* guard) {
    StageMark m(ws, kSScale, st);
    const dim3 grid((g.ntiles + 63) / 64);
    const unsigned* cmx = (const unsigned*)ws.cmx.p;
    const int* tile_total = (const int*)ws.tile_total.p;
    if (nout == 1)
        hipLaunchKernelGGL((k_tilescale<1>), grid, dim3(kBlock), 0, st, cmx, (int)pl.nblk_s,
                           g.ntiles, tile_total, (int2*)ws.tile_k.p, guard);
    else
        hipLaunchKernelGGL((k_tilescale<2>), grid, dim3(kBlock), 0, st, cmx, (int)pl.nblk_s,
                           g.ntiles, tile_total, (int2*)ws.tile_k.p, guard);
    ASP_LAUNCHED();
    m.done();
    return ASP_OK;
}

}  // namespace asp
