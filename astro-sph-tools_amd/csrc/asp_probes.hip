// asp_probes.hip -- the parity probes of the 2-D map: the reference's kernel values
// (asp_kernel_eval), chunk ranges (asp_chunk_ranges) and per-pixel neighbour lists
// (asp_pixel_neighbours), each on the projector's own decision code (asp_device.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/asp.h"
#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map.hpp"

namespace asp {

// ----------------------------------------------------------------------------------
// Auxiliary entry points: kernel evaluation, chunk ranges, neighbour lists.
// ----------------------------------------------------------------------------------
// Column-integrated kernels in closed form (fp64).  w(r) is a polynomial in r on each
// piece, and with R = sqrt(q^2 + Z^2)
//   J_n(Z) = int_0^Z r^n dz = (Z R^n + n q^2 J_{n-2}(Z)) / (n + 1),  J_0 = Z,
//   q^2 J_{-1} = q^2 log((Z + R) / q)  (0 at q = 0),
// so int_0^Z w dz = sum_n c[n] J_n(Z).
template <int N>
__device__ double column_piece(const double (&c)[N], double q, double Z) {
    const double q2 = q * q, R = sqrt(q2 + Z * Z);
    double J[N];
    J[0] = Z;
    J[1] = 0.5 * (Z * R + (q > 0.0 ? q2 * log((Z + R) / q) : 0.0));
    double Rn = R;
    for (int k = 2; k < N; ++k) {
        Rn *= R;
        J[k] = (Z * Rn + k * q2 * J[k - 2]) / (k + 1.0);
    }
    double s = 0.0;
    for (int k = 0; k < N; ++k) s += c[k] * J[k];
    return s;
}
// F(q) = 2 int_0^sqrt(4 - q^2) w(sqrt(q^2 + z^2)) dz for 0 <= q < 2.
__device__ double column_F(int kid, double q) {
    const double Zm = sqrt(fmax(4.0 - q * q, 0.0));
    if (kid == ASP_KERNEL_WENDLAND_C2_COLUMN) {  // (1 - r/2)^4 (1 + 2r) by powers of r
        const double c[6] = {1.0, 0.0, -2.5, 2.5, -15.0 / 16.0, 0.125};
        return 2.0 * column_piece(c, q, Zm);
    }
    const double out[4] = {2.0, -3.0, 1.5, -0.25};  // (2 - r)^3 / 4
    double F = column_piece(out, q, Zm);
    if (q < 1.0) {  // the inner polynomial replaces the outer one on [0, sqrt(1 - q^2)]
        const double in[4] = {1.0, 0.0, -1.5, 0.75};
        const double Z1 = sqrt(1.0 - q * q);
        F += column_piece(in, q, Z1) - column_piece(out, q, Z1);
    }
    return 2.0 * F;
}

__global__ void k_kernel_eval(int kid, const double* __restrict__ r, const double* __restrict__ h,
                              double* __restrict__ w, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double q = r[i] / h[i];
    double res = 0.0;
    if (kid == ASP_KERNEL_CUBIC_SPLINE_COLUMN || kid == ASP_KERNEL_WENDLAND_C2_COLUMN) {
        // as ids 0 and 1: inside the support or exactly 0 (h == 0 makes q infinite or NaN:
        // 0).  The integral is even in q, so a negative h is evaluated at |q|.
        const double K = kid == ASP_KERNEL_CUBIC_SPLINE_COLUMN ? 1.0 / M_PI : 21.0 / (16.0 * M_PI);
        if (fabs(q) < 2.0) res = K * column_F(kid, fabs(q)) / (h[i] * h[i]);
    } else if (kid == ASP_KERNEL_CUBIC_SPLINE) {  // _kernels.pyx:13-19, same branch order
        if (q < 1.0)
            res = (1 - 1.5 * pow(q, 2.0) + 0.75 * pow(q, 3.0)) / (M_PI * pow(h[i], 3.0));
        else if (q < 2.0)
            res = (0.25 * pow((2 - q), 3.0)) / (M_PI * pow(h[i], 3.0));
    } else if (kid == ASP_KERNEL_WENDLAND_C2) {
        if (q < 2.0) {
            double t = 1.0 - 0.5 * q;
            res = 21.0 / (16.0 * M_PI * pow(h[i], 3.0)) * pow(t, 4.0) * (1.0 + 2.0 * q);
        }
    } else {
        res = 1.0;
    }
    w[i] = res;
}

__global__ void k_chunk_ranges(Grid g, const float* __restrict__ u, const float* __restrict__ v,
                               const float* __restrict__ h, long long n, int* cx0, int* cx1,
                               int* cy0, int* cy1) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int a, b, c, d;
    chunk_range((double)u[i], (double)h[i], g.x_min, g.psx, g.nx, g.cs, a, b);
    chunk_range((double)v[i], (double)h[i], g.y_min, g.psy_cull, g.ny, g.cs, c, d);
    cx0[i] = a;
    cx1[i] = b;
    cy0[i] = c;
    cy1[i] = d;
}

// Neighbour lists: one workgroup per pixel, particles in ascending order.  The decision
// is the deposit's (footprint box, then decide()), so this lists exactly the pairs the
// deposit accumulates.  pass 0 counts, pass 1 writes at offsets[pixel].
__global__ __launch_bounds__(kBlock) void k_neighbours(Grid g, Src64 s, const float* __restrict__ u,
                                                       const float* __restrict__ v,
                                                       const float* __restrict__ h, long long n,
                                                       const long long* __restrict__ pixels,
                                                       long long* __restrict__ counts,
                                                       const long long* __restrict__ offsets,
                                                       int* __restrict__ index, long long cap,
                                                       int pass) {
    __shared__ int wsum[kBlock / 64];
    __shared__ long long run;
    long long px = pixels[blockIdx.x];
    int xi = (int)(px / g.ny), yi = (int)(px - (px / g.ny) * g.ny);
    float X = (float)corner_x(g, xi), Y = (float)corner_y(g, yi);
    if (threadIdx.x == 0) run = pass ? offsets[blockIdx.x] : 0;
    __syncthreads();
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (long long base = 0; base < n; base += kBlock) {
        long long p = base + threadIdx.x;
        bool in = false;
        if (p < n) {
            Prep P;
            if (prep_record<2>(g, s, (int)p, u[p], v[p], h[p], 0.0f, 0.0f, 0, 0, P) &&
                xi >= P.b.x0 && xi <= P.b.x1 && yi >= P.b.y0 && yi <= P.b.y1) {
                float r2;
                in = decide(g, s, P, xi, yi, X, Y, r2);
            }
        }
        unsigned long long m = __ballot(in);
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int before = 0, tot = 0;
        for (int k = 0; k < kBlock / 64; ++k) {
            if (k < wv) before += wsum[k];
            tot += wsum[k];
        }
        if (pass && in) {
            long long slot = run + before + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < cap) index[slot] = (int)p;
        }
        __syncthreads();
        if (threadIdx.x == 0) run += tot;
        __syncthreads();
    }
    if (!pass && threadIdx.x == 0) counts[blockIdx.x] = run;
}

}  // namespace asp

using namespace asp;

extern "C" {

int asp_kernel_eval(int32_t kernel_id, const double* r, const double* h, double* w, int64_t n,
                    int32_t flags, int32_t device, void* stream) {
    enum { kR, kH, kW };  // per-call scratch of a host caller: staged r, h and the values
    t_err.clear();
    if (kernel_id < 0 || kernel_id > ASP_KERNEL_WENDLAND_C2_COLUMN)
        return fail(ASP_ERR_INVALID, "unknown kernel_id");
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (n == 0) return ASP_OK;
    return with_workspace(device, (hipStream_t)stream, false, [&](Workspace& ws, hipStream_t st) -> int {
        const double *dr = r, *dh = h;
        double* dw = w;
        bool dev = flags & ASP_F_DEVICE_PTRS;
        if (!dev) {
            ASP_TRY(to_device(ws, ws.aux[kR], dr, n * sizeof(double), st, Copy::kPlain));
            ASP_TRY(to_device(ws, ws.aux[kH], dh, n * sizeof(double), st, Copy::kPlain));
            ASP_TRY(device_scratch(ws.aux[kW], dw, n * sizeof(double)));
        }
        hipLaunchKernelGGL(k_kernel_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           (int)kernel_id, dr, dh, dw, (long long)n);
        ASP_LAUNCHED();
        if (!dev) {
            ASP_TRY(to_host(w, dw, n * sizeof(double), st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        return ASP_OK;
    });
}

int asp_chunk_ranges(const float* u, const float* v, const float* h, int64_t n, double u_min,
                     double u_max, double v_min, double v_max, int32_t nx, int32_t ny,
                     int32_t chunk_size, int32_t* cx0, int32_t* cx1, int32_t* cy0, int32_t* cy1,
                     int32_t flags, int32_t device, void* stream) {
    t_err.clear();
    Grid g;
    if (!make_grid(u_min, u_max, v_min, v_max, nx, ny, chunk_size, g))
        return fail(ASP_ERR_INVALID, "invalid grid");
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (n == 0) return ASP_OK;
    return with_workspace(device, (hipStream_t)stream, false, [&](Workspace& ws, hipStream_t st) -> int {
        bool dev = flags & ASP_F_DEVICE_PTRS;
        const float *du = u, *dv = v, *dh = h;
        int* o[4] = {cx0, cx1, cy0, cy1};
        if (!dev) {
            const float** src[3] = {&du, &dv, &dh};
            for (int k = 0; k < 3; ++k)
                ASP_TRY(to_device(ws, ws.in[k], *src[k], n * sizeof(float), st, Copy::kPlain));
            for (int k = 0; k < 4; ++k) ASP_TRY(device_scratch(ws.aux[k], o[k], n * sizeof(int)));
        }
        hipLaunchKernelGGL(k_chunk_ranges, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g,
                           du, dv, dh, (long long)n, o[0], o[1], o[2], o[3]);
        ASP_LAUNCHED();
        if (!dev) {
            int* dst[4] = {cx0, cx1, cy0, cy1};
            for (int k = 0; k < 4; ++k)
                ASP_TRY(to_host(dst[k], o[k], n * sizeof(int), st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        return ASP_OK;
    });
}

int asp_pixel_neighbours(const float* u, const float* v, const float* h, int64_t n,
                         double u_min, double u_max, double v_min, double v_max, int32_t nx,
                         int32_t ny, int32_t chunk_size, const int64_t* pixels, int64_t npix,
                         int64_t* offsets, int32_t* index, int64_t cap, int64_t* total,
                         int32_t device) {
    // per-call scratch: the staged pixel ids, their counts and offsets, the index lists
    enum { kPixels, kCounts, kOffsets, kIndex };
    t_err.clear();
    Grid g;
    if (!make_grid(u_min, u_max, v_min, v_max, nx, ny, chunk_size, g))
        return fail(ASP_ERR_INVALID, "invalid grid");
    if (n < 0 || npix < 0 || cap < 0) return fail(ASP_ERR_INVALID, "negative size");
    for (int64_t k = 0; k < npix; ++k)
        if (pixels[k] < 0 || pixels[k] >= (int64_t)nx * ny)
            return fail(ASP_ERR_INVALID, "pixel id out of range");
    offsets[0] = 0;
    if (total) *total = 0;
    if (npix == 0) return ASP_OK;
    if (n == 0) {
        for (int64_t k = 0; k < npix; ++k) offsets[k + 1] = 0;
        return ASP_OK;
    }
    return with_workspace(device, nullptr, false, [&](Workspace& ws, hipStream_t st) -> int {
        const float* d[3] = {u, v, h};
        for (int k = 0; k < 3; ++k)
            ASP_TRY(to_device(ws, ws.in[k], d[k], n * sizeof(float), st, Copy::kPlain));
        const long long* dpix = (const long long*)pixels;
        long long* dcnt = nullptr;
        ASP_TRY(to_device(ws, ws.aux[kPixels], dpix, npix * sizeof(long long), st, Copy::kPlain));
        ASP_TRY(device_scratch(ws.aux[kCounts], dcnt, npix * sizeof(long long)));
        ASP_TRY(ensure(ws.aux[kOffsets], (npix + 1) * sizeof(long long)));
        const Src64 s{nullptr, nullptr, nullptr, nullptr, nullptr, 0, d[0], d[1], d[2]};
        hipLaunchKernelGGL(k_neighbours, dim3((unsigned)npix), dim3(kBlock), 0, st, g, s, d[0], d[1],
                           d[2], (long long)n, dpix, dcnt, (const long long*)nullptr, (int*)nullptr,
                           0LL, 0);
        ASP_LAUNCHED();
        std::vector<long long> cnt(npix);
        ASP_TRY(to_host(cnt.data(), dcnt, npix * sizeof(long long), st));
        ASP_HIP(hipStreamSynchronize(st));
        for (int64_t k = 0; k < npix; ++k) offsets[k + 1] = offsets[k] + cnt[k];
        long long tot = offsets[npix];
        if (total) *total = tot;
        long long wcap = std::min<long long>(cap, tot);
        if (wcap > 0) {
            int* dindex = nullptr;
            const long long* doff = (const long long*)offsets;
            ASP_TRY(device_scratch(ws.aux[kIndex], dindex, wcap * sizeof(int)));
            ASP_TRY(to_device(ws, ws.aux[kOffsets], doff, npix * sizeof(long long), st, Copy::kPlain));
            hipLaunchKernelGGL(k_neighbours, dim3((unsigned)npix), dim3(kBlock), 0, st, g, s, d[0], d[1],
                               d[2], (long long)n, dpix, dcnt, doff, dindex, wcap, 1);
            ASP_LAUNCHED();
            ASP_TRY(to_host(index, dindex, wcap * sizeof(int), st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        return ASP_OK;
    });
}

}  // extern "C"
