// asp_pairs.hip -- the kernel_func plug-in of the 2-D map: K8 pairs and the session behind
// asp_pairs_begin / _emit / _end.  The binning is the map's own (project2d_device with
// bin_only; the pipeline's overview is in asp_project2d.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/asp.h"
#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map.hpp"
#include "asp_map_device.hpp"
#include "asp_wave.hpp"

namespace asp {

// ----------------------------------------------------------------------------------
// K8 pairs (the kernel_func plugin: _projector.py:26, 86; _pixel_calculations.pyx:30-33),
// one workgroup per GPU tile of a binned window, on the records the session keeps
// resident.  Every included (pixel, particle) pair -- the deposit's exact decision -- is
//   MODE 0: counted per pixel (int32 pixcnt[tile][lx * 64 + ly], int64 tile totals);
//   MODE 1: written as the particle index and the reference's fp64 r^2 = dx^2 + dy^2
//           (dx = U - X, .pyx:13-14, :20-30) at its pixel's slot range, the pixel offsets
//           being the tile base + an exclusive scan of that tile's pixcnt (also written
//           out for the host).  Order within a pixel unspecified.
// The counts come from the same records and decisions as the pairs, so a pixel's slots
// always suffice; a pair that would not fit (a broken invariant) is dropped and counted in
// *overflow, which the host turns into an error.
// ----------------------------------------------------------------------------------
constexpr int kPairsBlock = 256;
template <int MODE>
__global__ __launch_bounds__(kPairsBlock) void k_pairs(
    Grid g, Src64 s, const float4* __restrict__ recs, const long long* __restrict__ tile_start,
    const int* __restrict__ tile_total, const int* __restrict__ wide_list, int n_wide,
    const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ h,
    int t0, int* __restrict__ pixcnt, long long* __restrict__ tile_pairs,
    const long long* __restrict__ tile_base, long long* __restrict__ offsets,
    int* __restrict__ particle, double* __restrict__ r2out, int* __restrict__ overflow) {
    __shared__ int cur[kTilePix];
    __shared__ float xt[kTile], yt[kTile];
    __shared__ long long wsum[kPairsBlock / 64];
    __shared__ long long soff[MODE == 1 ? kTilePix + 1 : 1];  // MODE 1: the pixel offsets
    const int t = t0 + blockIdx.x;
    const int tx = t / g.nty, ty = t - (t / g.nty) * g.nty;
    const int X0 = tx * kTile, Y0 = ty * kTile;
    const int TW = min(kTile, g.nx - X0), TH = min(kTile, g.ny - Y0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int kPer = kTilePix / kPairsBlock;  // 16 consecutive pixels per thread
    long long* off = offsets + (long long)blockIdx.x * kTilePix;  // MODE 1
    if constexpr (MODE == 1) {
        // exclusive scan of the tile's pixel counts + the tile's base: the pixel offsets
        const int* c = pixcnt + (long long)t * kTilePix + threadIdx.x * kPer;
        long long loc[kPer], run = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            loc[k] = run;
            run += c[k];
        }
        const long long x = wave_incl_scan(run, lane);
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        long long base = tile_base[blockIdx.x] + x - run;
        for (int k = 0; k < wv; ++k) base += wsum[k];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            soff[threadIdx.x * kPer + k] = base + loc[k];
            off[threadIdx.x * kPer + k] = base + loc[k];
        }
        if (threadIdx.x == kPairsBlock - 1) {  // = the next tile's base
            soff[kTilePix] = base + run;
            off[kTilePix] = base + run;
        }
    }
    for (int k = threadIdx.x; k < kTilePix; k += kPairsBlock) cur[k] = 0;
    corner_tables(g, X0, Y0, xt, yt);
    __syncthreads();
    auto emit_box = [&](const Prep& P) {  // P in its box-origin frame
        for (int xi = P.b.x0; xi <= P.b.x1; ++xi)
            for (int yi = P.b.y0; yi <= P.b.y1; ++yi) {
                float r2f;
                if (!decide(g, s, P, xi, yi, xt[xi - P.b.x0], yt[yi - P.b.y0], r2f)) continue;
                const int lp = (xi - X0) * kTile + (yi - Y0);
                const int k = atomicAdd(&cur[lp], 1);
                if constexpr (MODE == 1) {
                    const long long slot = soff[lp] + k;
                    if (slot >= soff[lp + 1]) {
                        atomicAdd(overflow, 1);
                        continue;
                    }
                    const Vals x = src_values(g, s, P.p);
                    const double dx = x.U - corner_x(g, xi), dy = x.V - corner_y(g, yi);
                    particle[slot] = P.p;
                    r2out[slot] = dx * dx + dy * dy;
                }
            }
    };
    for (int stream = 0; stream < 2; ++stream) {
        const long long st0 = tile_start[t + stream * g.ntiles];
        const int cnt = tile_total[t + stream * g.ntiles];
        for (int i = threadIdx.x; i < cnt; i += kPairsBlock) {
            float4 r0, r1;
            load_rec(recs, st0 + i, r0, r1);
            Prep P;
            rec_prep<kAccF64>(r0, r1, X0, Y0, make_int2(0, 0), P);
            emit_box(P);
        }
    }
    for (int i = threadIdx.x; i < n_wide; i += kPairsBlock) {
        const int p = wide_list[i];
        Prep P;
        if (!prep_record<2>(g, s, p, u[p], v[p], h[p], 0.0f, 0.0f, 0, 0, P) ||
            !clip(P.b, X0, Y0, TW, TH))
            continue;
        P.u = (float)(src_u(s, p, P.u) - corner_x(g, P.b.x0));  // box-origin frame
        P.v = (float)(src_v(s, p, P.v) - corner_y(g, P.b.y0));
        emit_box(P);
    }
    if constexpr (MODE == 0) {
        __syncthreads();
        long long tot = 0;
        for (int k = threadIdx.x; k < kTilePix; k += kPairsBlock) {
            pixcnt[(long long)t * kTilePix + k] = cur[k];
            tot += cur[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        if (lane == 0) wsum[wv] = tot;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long a = 0;
            for (int k = 0; k < kPairsBlock / 64; ++k) a += wsum[k];
            tile_pairs[t] = a;
        }
    }
}

// The kernel_func plug-in session (asp_pairs_begin / _emit / _end): the particles are
// staged and binned ONCE per create_image call, window by window (window_grid); the
// records of the current window stay resident in the session's own workspace between the
// emits, so a map needing many host batches costs one binning per window, not one per
// batch.
struct PairsSession {
    Workspace ws;  // the session's own buffers (a call on the device cannot evict them)
    Grid full;
    Src64 s{};
    const float* f[3] = {nullptr, nullptr, nullptr};  // fp32 working copies u, v, h
    long long n = 0;
    int device = 0;
    int flags = 0;
    hipStream_t st = nullptr;
    int wtx0 = -1, wtx1 = -1;  // tile rows binned now
    int n_wide = 0;
    std::vector<long long> tile_pairs;  // per GPU tile of the whole image
};

static inline int pairs_window_of(const PairsSession& S, int t) {  // first tile row of t's window
    const int tx = t / S.full.nty, wr = window_rows(S.full);
    return (tx / wr) * wr;
}

// Bin the window holding tile rows [tx0, ..) and count its pixels' pairs (MODE 0).
static int pairs_bin(PairsSession& S, int tx0) {
    Workspace& ws = S.ws;
    const int wr = window_rows(S.full);
    const int tx1 = std::min(tx0 + wr, S.full.ntx);
    if (S.wtx0 == tx0) return ASP_OK;
    const Grid g = window_grid(S.full, tx0, tx1);
    S.wtx0 = -1;
    Buf& pixcnt = ws.pairs[kPairsPixCount];
    Buf& totals = ws.pairs[kPairsTileTotals];
    ASP_TRY(ensure(pixcnt, (size_t)g.ntiles * kTilePix * sizeof(int)));
    ASP_TRY(ensure(totals, (size_t)g.ntiles * sizeof(long long)));
    if (S.n == 0) {  // nothing binned: zero pixel counts and tile totals
        ASP_HIP(hipMemsetAsync(pixcnt.p, 0, (size_t)g.ntiles * kTilePix * sizeof(int), S.st));
        ASP_HIP(hipMemsetAsync(totals.p, 0, (size_t)g.ntiles * sizeof(long long), S.st));
        S.n_wide = 0;
    } else {
        int nw = 0;
        const int rc = project2d_device(ws, g, S.s, S.f[0], S.f[1], S.f[2], S.f[2], nullptr, S.n,
                                        ASP_KERNEL_INDICATOR, 0, nullptr, nullptr, S.st, &nw);
        if (rc == kRetSplit)
            return fail(ASP_ERR_UNSUPPORTED, "kernel_func plug-in: >= 2^31 records in one window");
        ASP_TRY(rc);
        S.n_wide = nw;
        hipLaunchKernelGGL(k_pairs<0>, dim3((unsigned)g.ntiles), dim3(kPairsBlock), 0, S.st, g,
                           S.s, (const float4*)ws.recs.p, (const long long*)ws.tile_start.p,
                           (const int*)ws.tile_total.p, (const int*)ws.wide.p, nw, S.f[0], S.f[1],
                           S.f[2], 0, (int*)pixcnt.p, (long long*)totals.p,
                           (const long long*)nullptr, (long long*)nullptr, (int*)nullptr,
                           (double*)nullptr, (int*)nullptr);
        ASP_LAUNCHED();
    }
    S.wtx0 = tx0;
    S.wtx1 = tx1;
    return ASP_OK;
}

static int pairs_begin(const double* pos, const double* h, long long n, int axis,
                       const MapArgs& m, long long* tile_pairs, PairsSession** out) {
    const int flags = m.flags, device = m.device;
    *out = nullptr;
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (n > 0x7fffffffLL)
        return fail(ASP_ERR_UNSUPPORTED, "kernel_func plug-in: n >= 2^31 particles per call");
    if (n > 0 && (!pos || !h)) return fail(ASP_ERR_INVALID, "NULL particle array");
    if (!tile_pairs) return fail(ASP_ERR_INVALID, "NULL tile_pairs");
    int cull_axis = 0;
    ASP_TRY(decode_axis(axis, cull_axis));
    Grid g;
    ASP_TRY(setup_grid(m, g));
    g.mixed = cull_axis != axis;
    ASP_TRY(set_device(device));
    PairsSession* S = new (std::nothrow) PairsSession();
    if (!S) return fail(ASP_ERR_NOMEM, "session");
    S->full = g;
    S->n = n;
    S->device = device;
    S->flags = flags;
    S->st = (hipStream_t)m.stream;
    Workspace& ws = S->ws;
    auto bail = [&](int rc) {
        (void)hipStreamSynchronize(S->st);
        ws_teardown(ws);
        delete S;
        return rc;
    };
    const bool dev = flags & ASP_F_DEVICE_PTRS;
    const double *dpos = pos, *dh64 = h;
    if (!dev && n > 0) {
        int rc = to_device(ws, ws.in64[0], dpos, (size_t)n * 3 * sizeof(double), S->st, Copy::kPinned);
        if (rc == ASP_OK)
            rc = to_device(ws, ws.in64[1], dh64, (size_t)n * sizeof(double), S->st, Copy::kPinned);
        if (rc != ASP_OK) return bail(rc);
    }
    for (int k = 0; k < 3; ++k) {
        const int rc = ensure(ws.in[k], (size_t)n * sizeof(float));
        if (rc != ASP_OK) return bail(rc);
    }
    float* f[3] = {(float*)ws.in[0].p, (float*)ws.in[1].p, (float*)ws.in[2].p};
    if (n > 0) {
        const int rc = stage_device(dpos, dh64, nullptr, nullptr, n, axis, f[0], f[1], f[2],
                                    nullptr, nullptr, S->st);
        if (rc != ASP_OK) return bail(rc);
    }
    S->s = src64_from_positions(dpos, dh64, axis, cull_axis, f);
    for (int k = 0; k < 3; ++k) S->f[k] = f[k];
    // every window once: its per-tile pair totals (the last window stays binned)
    S->tile_pairs.assign((size_t)g.ntiles, 0);
    const int wr = window_rows(g);
    for (int tx0 = 0; tx0 < g.ntx; tx0 += wr) {
        int rc = pairs_bin(*S, tx0);
        const Grid w = window_grid(g, tx0, std::min(tx0 + wr, g.ntx));
        if (rc == ASP_OK)
            rc = hipMemcpyAsync(S->tile_pairs.data() + (size_t)tx0 * g.nty,
                                ws.pairs[kPairsTileTotals].p, (size_t)w.ntiles * sizeof(long long),
                                hipMemcpyDeviceToHost, S->st) == hipSuccess
                     ? ASP_OK : fail(ASP_ERR_HIP, "tile totals");
        if (rc == ASP_OK)
            rc = hipStreamSynchronize(S->st) == hipSuccess ? ASP_OK : fail(ASP_ERR_HIP, "sync");
        if (rc != ASP_OK) return bail(rc);
    }
    std::copy(S->tile_pairs.begin(), S->tile_pairs.end(), tile_pairs);
    *out = S;
    return ASP_OK;
}

// Pairs of the GPU tiles [t0, t1) (global row-major tile ids), pixels tile by tile and
// lx * 64 + ly inside a tile: offsets ((t1 - t0) * 4096 + 1, from 0), particle, r2.
static int pairs_emit(PairsSession& S, int t0, int t1, long long* offsets, int* particle,
                      double* r2) {
    if (t0 < 0 || t1 > S.full.ntiles || t0 > t1) return fail(ASP_ERR_INVALID, "bad tile range");
    if (!offsets) return fail(ASP_ERR_INVALID, "NULL offsets");
    // per-call scratch: the staged outputs of a host caller, the tiles' slot bases, the
    // overflow flag
    enum { kOffsets, kParticle, kR2, kTileBase, kOverflow };
    static_assert(kOverflow < kAuxCounters, "scratch slots 0 .. 4");
    Workspace& ws = S.ws;
    ASP_HIP(hipSetDevice(S.device));
    const bool dev = S.flags & ASP_F_DEVICE_PTRS;
    const long long npx = (long long)(t1 - t0) * kTilePix;
    long long total = 0;
    for (int t = t0; t < t1; ++t) total += S.tile_pairs[t];
    if (total > 0 && (!particle || !r2)) return fail(ASP_ERR_INVALID, "NULL pair outputs");
    long long* doff = offsets;
    int* dpart = particle;
    double* dr2 = r2;
    if (!dev) {
        ASP_TRY(device_scratch(ws.aux[kOffsets], doff, (size_t)(npx + 1) * sizeof(long long)));
        ASP_TRY(device_scratch(ws.aux[kParticle], dpart, (size_t)std::max(total, 1LL) * sizeof(int)));
        ASP_TRY(device_scratch(ws.aux[kR2], dr2, (size_t)std::max(total, 1LL) * sizeof(double)));
    }
    ASP_TRY(ensure(ws.aux[kTileBase], (size_t)(t1 - t0 + 1) * sizeof(long long)));
    ASP_TRY(ensure(ws.aux[kOverflow], sizeof(int)));
    int* dovf = (int*)ws.aux[kOverflow].p;
    ASP_HIP(hipMemsetAsync(dovf, 0, sizeof(int), S.st));
    if (npx == 0 || S.n == 0) {
        // no tiles, or no particles (nothing was binned: no records for k_pairs to read):
        // every pixel's range is empty
        if (!dev) std::fill(offsets, offsets + npx + 1, 0LL);
        else ASP_HIP(hipMemsetAsync(offsets, 0, (size_t)(npx + 1) * sizeof(long long), S.st));
        ASP_HIP(hipStreamSynchronize(S.st));
        return ASP_OK;
    }
    // window by window (the session re-bins only when the range moves to another window)
    long long done = 0;
    for (int a = t0; a < t1;) {
        const int tx0 = pairs_window_of(S, a);
        ASP_TRY(pairs_bin(S, tx0));
        const int wt0 = tx0 * S.full.nty;                          // window's first tile
        const int b = std::min(t1, S.wtx1 * S.full.nty);
        std::vector<long long> base((size_t)(b - a));
        for (int t = a; t < b; ++t) {
            base[t - a] = done;
            done += S.tile_pairs[t];
        }
        long long* dbase = (long long*)ws.aux[kTileBase].p;
        ASP_HIP(hipMemcpyAsync(dbase, base.data(), base.size() * sizeof(long long),
                               hipMemcpyHostToDevice, S.st));
        const Grid g = window_grid(S.full, S.wtx0, S.wtx1);
        hipLaunchKernelGGL(k_pairs<1>, dim3((unsigned)(b - a)), dim3(kPairsBlock), 0, S.st, g,
                           S.s, (const float4*)ws.recs.p, (const long long*)ws.tile_start.p,
                           (const int*)ws.tile_total.p, (const int*)ws.wide.p, S.n_wide, S.f[0],
                           S.f[1], S.f[2], a - wt0, (int*)ws.pairs[kPairsPixCount].p,
                           (long long*)nullptr,
                           (const long long*)dbase, doff + (long long)(a - t0) * kTilePix, dpart,
                           dr2, dovf);
        ASP_LAUNCHED();
        ASP_HIP(hipStreamSynchronize(S.st));  // dbase is reused by the next window's launch
        a = b;
    }
    int ovf = 0;
    ASP_HIP(hipMemcpyAsync(&ovf, dovf, sizeof(int), hipMemcpyDeviceToHost, S.st));
    if (!dev) {
        ASP_TRY(to_host(offsets, doff, (size_t)(npx + 1) * sizeof(long long), S.st));
        if (total > 0) {
            ASP_TRY(to_host(particle, dpart, (size_t)total * sizeof(int), S.st));
            ASP_TRY(to_host(r2, dr2, (size_t)total * sizeof(double), S.st));
        }
    }
    ASP_HIP(hipStreamSynchronize(S.st));
    if (ovf) return fail(ASP_ERR_INVALID, "pair slots overflowed (counts and pairs disagree)");
    return ASP_OK;
}

static int pairs_end(PairsSession* S) {
    if (!S) return ASP_OK;
    (void)hipSetDevice(S->device);
    (void)hipStreamSynchronize(S->st);
    ws_teardown(S->ws);  // buffers, pinned memory, the side stream and its events
    delete S;
    return ASP_OK;
}

}  // namespace asp

using namespace asp;

extern "C" {

int asp_pairs_begin(const double* positions, const double* h, int64_t n, int32_t axis,
                    double u_min, double u_max, double v_min, double v_max, int32_t nx,
                    int32_t ny, int32_t chunk_size, int32_t flags, int32_t device, void* stream,
                    int64_t* tile_pairs, void** session) {
    t_err.clear();
    if (!session) return fail(ASP_ERR_INVALID, "NULL session");
    PairsSession* S = nullptr;
    const int rc = pairs_begin(positions, h, n, axis,
                               MapArgs{u_min, u_max, v_min, v_max, nx, ny, chunk_size,
                                       ASP_KERNEL_INDICATOR, flags, nullptr, nullptr, device, stream},
                               (long long*)tile_pairs, &S);
    *session = S;
    return rc;
}

int asp_pairs_emit(void* session, int32_t tile_lo, int32_t tile_hi, int64_t* offsets,
                   int32_t* particle, double* r2) {
    t_err.clear();
    if (!session) return fail(ASP_ERR_INVALID, "NULL session");
    return pairs_emit(*(PairsSession*)session, tile_lo, tile_hi, (long long*)offsets, particle, r2);
}

int asp_pairs_end(void* session) {
    t_err.clear();
    return pairs_end((PairsSession*)session);
}

}  // extern "C"
