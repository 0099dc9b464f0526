// Microbenchmark: LDS accumulation primitives on gfx950 (random addresses in a 64x64x2
// fp32 tile, the deposit kernel's access pattern).  Build & run:
//   hipcc -O3 --offload-arch=gfx950 -munsafe-fp-atomics -o /tmp/mb tools/microbench/lds.hip
//   /tmp/mb        the primitives;   /tmp/mb dep   the deposit-shaped arrangements (below)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

constexpr int N = 8192;  // 2 x 64 x 64 floats
constexpr int ITERS = 4096;

__device__ __forceinline__ uint32_t hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16; return x;
}

template <int MODE>
__global__ __launch_bounds__(256) void k(float* out, int span) {
    __shared__ float lds[N];
    __shared__ unsigned long long lds64[N / 2];
    __shared__ unsigned long long hi64[MODE >= 10 ? N / 2 : 1];  // the two-word fixed point
    for (int i = threadIdx.x; i < N; i += 256) lds[i] = 0.f;
    for (int i = threadIdx.x; i < N / 2; i += 256) lds64[i] = 0;
    for (int i = threadIdx.x; i < (MODE >= 10 ? N / 2 : 1); i += 256) hi64[i] = 0;
    __syncthreads();
    uint32_t s = hash(blockIdx.x * 256 + threadIdx.x);
    float val = 1.0f + (threadIdx.x & 7);
    unsigned mask = (unsigned)span - 1u;  // span is a power of two
    for (int it = 0; it < ITERS; ++it) {
        s = s * 1664525u + 1013904223u;   // LCG: 2 VALU ops
        int a = (int)((s >> 7) & mask);
        if constexpr (MODE == 0) atomicAdd(&lds[a], val);                      // ds_add_f32
        else if constexpr (MODE == 1) atomicAdd((unsigned*)&lds[a], (unsigned)val);  // ds_add_u32
        else if constexpr (MODE == 2) lds[a] = val;                            // ds_write_b32
        else if constexpr (MODE == 3) atomicAdd(&lds64[a >> 1], (unsigned long long)val);  // ds_add_u64
        else if constexpr (MODE == 4) { float t = lds[a]; lds[a] = t + val; }  // racy RMW
        else if constexpr (MODE == 5) {  // ds_add_rtn_u32 (cursor-style, result used)
            unsigned r = atomicAdd((unsigned*)&lds[a], 1u);
            val += (float)(r & 1u);
        }
        else if constexpr (MODE == 6) atomicAdd((double*)&lds64[a >> 1], (double)val);  // ds_add_f64
        else if constexpr (MODE == 7) atomicMax((unsigned*)&lds[a], (unsigned)val);    // ds_max_u32
        else if constexpr (MODE == 8) {  // ds_add_f64, lanes of each 32-lane half on distinct banks
            int w = ((a >> 1) & ~31) | (threadIdx.x & 31);
            atomicAdd((double*)&lds64[w & (N / 2 - 1)], (double)val);
        } else if constexpr (MODE == 9) {  // ds_add_f64, the deposit's column-only bank mapping:
            int w = ((a >> 1) & ~63) | ((threadIdx.x * 37 + (a >> 7)) & 63);  // random column
            atomicAdd((double*)&lds64[w & (N / 2 - 1)], (double)val);
        } else if constexpr (MODE == 10) {  // two-word fixed point: hi and lo ds_add_u64 each
            // (verdict r05 item 3): t = val * 2^k, hi = floor(t), lo = frac(t) * 2^32
            const double t = (double)val * 0x1p20;
            const double fh = floor(t);
            const unsigned long long hi = (unsigned long long)(long long)fh;
            const unsigned long long lo = (unsigned long long)((t - fh) * 0x1p32);
            atomicAdd(&lds64[a >> 1], lo);
            atomicAdd(&hi64[a >> 1], hi);
        } else if constexpr (MODE == 11) {  // the same words, the conversion omitted
            atomicAdd(&lds64[a >> 1], (unsigned long long)val);
            atomicAdd(&hi64[a >> 1], (unsigned long long)s);
        }
    }
    __syncthreads();
    float acc = 0.f;
    for (int i = threadIdx.x; i < N; i += 256)
        acc += lds[i] + (float)lds64[i / 2] + (MODE >= 10 ? (float)hi64[(i / 2) % (MODE >= 10 ? N / 2 : 1)] : 0.f);
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <int MODE>
float run(float* d, int blocks, int span) {
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, d, span);
    hipEventRecord(a);
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, d, span);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    return ms / 3;
}

// ----------------------------------------------------------------------------------
// Deposit-shaped modes (`lds dep`): k_deposit's small-box inner loop replayed on a synthetic
// record stream -- 32-B records in global memory, 512-thread workgroups, two 64 x 65-word
// fp64 maps in LDS, per record up to 9 slots x 2 maps of ds_add_f64 at base + i * 65 + j
// (slot mask in the record, ~79 % set as in the headline map) -- with the lane <-> record
// arrangement as the variable.  The cost of arranging (key loads, the in-wave sort, the
// ds_bpermute or the permuted reload) is inside the timed loop.
//   ARR 0  production: lane t takes record base + t (block-strided batches)
//   ARR 1  (a) one 64-record batch sorted in the wave, 8 dwords moved with ds_bpermute
//   ARR 2  (b) pool of 128 = two register sets, ds_bpermute from both + select
//   ARR 3  (c) pool of 64 NB records per wave by index: either sorted by bank and dealt over
//          the 16-lane groups, or in level order: all first records of every bank, then
//          all second ones, ... (the "cell" order compacted: no spare groups)
// BINS = 16 or 32: how many bank classes the sort distinguishes (word index mod BINS).
// The data patterns (record generation) place chosen bank classes on chosen lanes of the
// production order, to read the conflict grouping of ds_add_f64 from the rates.
// ----------------------------------------------------------------------------------
constexpr int kRow = 65, kTileW = 64 * kRow;
constexpr int DB = 512;  // workgroup (8 waves), two per CU
struct WaveLds {
    int cnt[32];
    unsigned lvl[64];
    unsigned char tab[256];
};

__global__ void gen(float4* recs, long long n, int pattern) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h = hash((uint32_t)i * 2654435761u + 12345u);
    int lane = (int)(i & 63);
    int x0 = (int)(h % 62u), y0 = (int)((h >> 8) % 62u);
    int M = 0, t = 0;
    if (pattern == 1) { M = 16; t = lane & 15; }
    if (pattern == 2) { M = 16; t = (lane >> 1) & 15; }
    if (pattern == 3) { M = 16; t = lane >> 2; }
    if (pattern == 4) { M = 32; t = lane & 31; }
    if (pattern == 5) { M = 32; t = lane >> 1; }
    if (M) y0 = ((t - x0) & (M - 1)) + (M == 16 ? 16 * (int)((h >> 20) % 3u) : 0);  // <= 47
    unsigned m = 0;
    for (int s = 0; s < 9; ++s) m |= ((hash((uint32_t)i * 9u + s) & 255u) < 202u ? 1u : 0u) << s;
    unsigned box = (unsigned)x0 | (unsigned)(x0 + 2) << 8 | (unsigned)y0 << 16 | (unsigned)(y0 + 2) << 24;
    recs[2 * i] = make_float4(0.25f, 0.5f, 0.75f, 1.0f + (h & 7));
    recs[2 * i + 1] = make_float4(0.5f, __uint_as_float(m), 0.0f, __uint_as_float(box));
}

// LDS written by one lane, read by another of the wave.  A wave's DS operations execute in
// order, so only the compiler has to keep them in order: FENCE 0 = wave barrier alone (the
// accesses may alias, which already orders them), 1 = with wavefront-scope fences, which
// cost an lgkmcnt(0) -- a drain of the wave's queued tile adds -- each.
#ifndef FENCE
#define FENCE 0
#endif
__device__ __forceinline__ void wsync() {
    if (FENCE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (FENCE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Order a pool of NB x 64 records (record j * 64 + lane has box word key[j]; the first n
// are live) by bank class.  Returns, packed one byte per batch, which pool record this
// lane takes in batch 0 .. NB-1.  LEVEL: position = records of lower rank-within-bank,
// then banks in order (16 consecutive positions hold distinct banks while the level is
// full); else plain sorted order dealt round-robin over the 4 NB 16-lane groups (full
// pools only).
template <int NB, int BINS, bool LEVEL>
__device__ __forceinline__ unsigned order_pool(const unsigned (&key)[NB], int n, WaveLds& w,
                                               int lane) {
    if (lane < BINS) w.cnt[lane] = 0;
    wsync();
    int bank[NB], r[NB];
    bool big = false;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        bank[j] = (int)(((key[j] & 255u) + ((key[j] >> 16) & 255u)) & (BINS - 1));  // 65 = 1 mod 32
        r[j] = j * 64 + lane < n ? atomicAdd(&w.cnt[bank[j]], 1) : 0;
        big |= r[j] >= 64;
    }
    wsync();
    const int c = w.cnt[lane & (BINS - 1)];
    int pos[NB];
    if constexpr (LEVEL) {
        int T = 0;
        unsigned m = 0;
#pragma unroll
        for (int b = 0; b < BINS; ++b) {
            const int cb = __builtin_amdgcn_readlane(c, b);
            T += min(cb, lane);
            m |= cb > lane ? 1u << b : 0u;
        }
        // T <= 256: 9 bits; the mask is BINS bits -> two words when BINS = 32
        w.lvl[lane] = BINS == 16 ? ((unsigned)T << 16 | m) : m;
        if (BINS == 32) ((unsigned short*)w.tab)[lane] = (unsigned short)T;  // tab is free here
        wsync();
        if (__ballot(big)) {  // a bank with more than 64 records: per-record sums
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                int p = 0;
#pragma unroll
                for (int b = 0; b < BINS; ++b) {
                    const int cb = __builtin_amdgcn_readlane(c, b);
                    p += min(cb, r[j]) + (b < bank[j] && cb > r[j] ? 1 : 0);
                }
                pos[j] = p;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const unsigned e = w.lvl[r[j]];
                const unsigned below = (1u << bank[j]) - 1u;
                if (BINS == 16) pos[j] = (int)(e >> 16) + __popc(e & 0xffffu & below);
                else pos[j] = (int)((unsigned short*)w.tab)[r[j]] + __popc(e & below);
            }
        }
        wsync();
    } else {
        int pre = 0;
#pragma unroll
        for (int b = 0; b < BINS; ++b) {
            const int cb = __builtin_amdgcn_readlane(c, b);
            pre += b < lane ? cb : 0;
        }
        if (lane < BINS) w.lvl[lane] = (unsigned)pre;
        wsync();
        constexpr int G = 4 * NB;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int p = (int)w.lvl[bank[j]] + r[j];
            pos[j] = (p % G) * 16 + p / G;
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
        if (j * 64 + lane < n) w.tab[(pos[j] & 63) * NB + (pos[j] >> 6)] = (unsigned char)(j * 64 + lane);
    wsync();
    unsigned idx;
    if (NB == 4) idx = ((const unsigned*)w.tab)[lane];
    else if (NB == 2) idx = ((const unsigned short*)w.tab)[lane];
    else idx = w.tab[lane];
    wsync();
    return idx;
}

__device__ __forceinline__ float4 bperm4(const float4& v, int src) {
    float4 o;
    o.x = __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v.x)));
    o.y = __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v.y)));
    o.z = __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v.z)));
    o.w = __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v.w)));
    return o;
}
__device__ __forceinline__ float4 sel4(bool c, const float4& a, const float4& b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// (c) variants: NB >= 2 batches per pool (a batch is loaded two batches ahead); SORT 0 = none (a fixed bijection, for the ablation),
// 1 = sorted + dealt, 2 = level order; RELOAD 0 = coalesced (ablation: the order is
// computed and ignored), 1 = each lane loads its record's two halves, 2 = paired: lanes
// 2t, 2t + 1 load the two halves of one record with one instruction, then swap (DPP).
template <int ARR, int BINS, bool ADDS, int NB = 4, int SORT = 2, int RELOAD = 1>
__global__ __launch_bounds__(DB) __attribute__((amdgpu_waves_per_eu(4))) void dep(
    const float4* __restrict__ recs, int count, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];
    __shared__ WaveLds wl[DB / 64];
    unsigned long long* acc0 = acc;
    unsigned long long* acc1 = acc + kTileW;
    for (int i = threadIdx.x; i < 2 * kTileW; i += DB) acc[i] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveLds& w = wl[wave];
    const long long start = (long long)blockIdx.x * count;
    const int last = count - 1;
    float sink = 0.0f;
    auto load = [&](int i, float4& r0, float4& r1) {
        r0 = recs[2 * (start + min(i, last))];
        r1 = recs[2 * (start + min(i, last)) + 1];
    };
    auto body = [&](const float4& r0, const float4& r1, bool live) {
        const unsigned bp = __float_as_uint(r1.w);
        const int base = (int)(bp & 255u) * kRow + (int)((bp >> 16) & 255u);
        const unsigned m = live ? __float_as_uint(r1.y) : 0u;
        if constexpr (!ADDS) {
            sink += r0.w * (float)(m + base) + r0.x + r0.y + r0.z + r1.x + r1.z;
            return;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (m >> (i * 3 + j) & 1u) {
                    const float wij = r0.x * (float)(i + 1) + r0.y * (float)j + r0.z + r1.z;
                    atomicAdd((double*)&acc0[base + i * kRow + j], (double)(r0.w * wij));
                    atomicAdd((double*)&acc1[base + i * kRow + j], (double)(r1.x * wij));
                }
    };
    if constexpr (ARR == 0 || ARR == 1) {
        float4 r0, r1, q0, q1;
        load(threadIdx.x, r0, r1);
        load(threadIdx.x + DB, q0, q1);
        for (int base = 0; base < count; base += DB) {
            float4 n0, n1;
            load(base + threadIdx.x + 2 * DB, n0, n1);
            if constexpr (ARR == 1) {
                const unsigned key[1] = {__float_as_uint(r1.w)};
                const int src = (int)order_pool<1, BINS, true>(key, 64, w, lane);
                body(bperm4(r0, src), bperm4(r1, src), base + threadIdx.x < count);
            } else {
                body(r0, r1, base + threadIdx.x < count);
            }
            r0 = q0; r1 = q1; q0 = n0; q1 = n1;
        }
    } else if constexpr (ARR == 2) {
        float4 a0, a1, b0, b1;
        load(threadIdx.x, a0, a1);
        load(threadIdx.x + DB, b0, b1);
        for (int base = 0; base < count; base += 2 * DB) {
            float4 na0, na1, nb0, nb1;
            load(base + threadIdx.x + 2 * DB, na0, na1);
            load(base + threadIdx.x + 3 * DB, nb0, nb1);
            const unsigned key[2] = {__float_as_uint(a1.w), __float_as_uint(b1.w)};
            const unsigned idx = order_pool<2, BINS, true>(key, 128, w, lane);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int src = (int)(idx >> (8 * jj) & 255u);
                const float4 x0 = sel4(src < 64, bperm4(a0, src & 63), bperm4(b0, src & 63));
                const float4 x1 = sel4(src < 64, bperm4(a1, src & 63), bperm4(b1, src & 63));
                body(x0, x1, true);
            }
            a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
        }
    } else {
        constexpr int PW = 64 * NB, STRIDE = (DB / 64) * PW;
        auto pstart = [&](int k) { return (max(k, 0) * (DB / 64) + wave) * PW; };
        auto pn = [&](int k) { return k < 0 ? 0 : max(0, min(PW, count - pstart(k))); };
        auto loadkeys = [&](int k, unsigned (&key)[NB]) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
                key[j] = __float_as_uint(
                    ((const float*)recs)[(start + min(pstart(k) + j * 64 + lane, last)) * 8 + 7]);
        };
        auto order = [&](const unsigned (&key)[NB], int n) {
            unsigned idx = 0;
            if constexpr (SORT == 0) {
#pragma unroll
                for (int j = 0; j < NB; ++j) idx |= (((j * 64 + lane) * 97 + 13) & (PW - 1)) << (8 * j);
                idx += key[0] & 0u;
            } else {
                idx = order_pool<NB, BINS, SORT == 2>(key, n, w, lane);
            }
            if constexpr (RELOAD == 0) {
                idx &= 0u;
#pragma unroll
                for (int j = 0; j < NB; ++j) idx |= (unsigned)(j * 64 + lane) << (8 * j);
            }
            return idx;
        };
        auto swap1 = [&](float x) {  // lane ^ 1 (quad_perm [1, 0, 3, 2])
            return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xf, 0xf, true));
        };
        // record i of this lane (pool-relative index pi): issue / finish
        auto rload = [&](int ps, int pi, float4& l0, float4& l1) {
            if constexpr (RELOAD == 2) {
                const int pj = __builtin_amdgcn_mov_dpp(pi, 0xB1, 0xf, 0xf, true);
                const bool odd = lane & 1;
                const long long ra = start + min(ps + (odd ? pj : pi), last);  // the even lane's
                const long long rb = start + min(ps + (odd ? pi : pj), last);  // the odd lane's
                l0 = recs[2 * ra + (lane & 1)];
                l1 = recs[2 * rb + (lane & 1)];
            } else {
                load(ps + pi, l0, l1);
            }
        };
        auto rfinish = [&](float4& l0, float4& l1) {
            if constexpr (RELOAD == 2) {
                const bool odd = lane & 1;
                const float4 give = sel4(odd, l0, l1);  // even gives B.r0, odd gives A.r1
                const float4 got = make_float4(swap1(give.x), swap1(give.y), swap1(give.z), swap1(give.w));
                const float4 x0 = sel4(odd, got, l0), x1 = sel4(odd, l1, got);
                l0 = x0;
                l1 = x1;
            }
        };
        // The loop starts at an empty pool -1 (dead lanes), so that the loop is entered with
        // the loads in the order every iteration leaves them in -- keys first, then record
        // loads -- and the wait for the keys stays a counted vmcnt that leaves the record
        // loads in flight (a prologue that issued the keys last made it vmcnt(0)).
        unsigned key[NB];
        loadkeys(0, key);
        asm volatile("" ::: "memory");  // keys first
        unsigned cidx = 0u;
        float4 a0, a1, b0, b1;
        rload(pstart(0), 0, a0, a1);
        rload(pstart(0), 1, b0, b1);
#pragma nounroll  // (peeling pool -1 off would undo that)
        for (int k = -1; k * STRIDE < count; ++k) {
            // pool k + 1's order (its keys were issued a pool ago), then pool k + 2's keys
            const unsigned nidx = order(key, pn(k + 1));
            loadkeys(k + 2, key);
            const int n = pn(k);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                float4 n0, n1;  // two batches ahead
                if (j + 2 < NB) rload(pstart(k), (int)(cidx >> (8 * (j + 2)) & 255u), n0, n1);
                else rload(pstart(k + 1), (int)(nidx >> (8 * (j + 2 - NB)) & 255u), n0, n1);
                rfinish(a0, a1);
                body(a0, a1, j * 64 + lane < n);
                a0 = b0; a1 = b1; b0 = n0; b1 = n1;
            }
            cidx = nidx;
        }
    }
    __syncthreads();
    float s = sink;
    for (int i = threadIdx.x; i < 2 * kTileW; i += DB) s += (float)__longlong_as_double((long long)acc[i]);
    out[blockIdx.x * DB + threadIdx.x] = s;
}

template <int ARR, int BINS, bool ADDS, int NB = 4, int SORT = 2, int RELOAD = 1>
void run_dep(const char* name, const float4* recs, int blocks, int count, float* out) {
    const size_t lds = 2 * kTileW * 8;
    auto kern = dep<ARR, BINS, ADDS, NB, SORT, RELOAD>;
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(DB), lds, 0, recs, count, out);
    hipEventRecord(a);
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(kern, dim3(blocks), dim3(DB), lds, 0, recs, count, out);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    ms /= 3;
    hipError_t e = hipGetLastError();
    double nrec = (double)blocks * count;
    printf("  %-44s %8.3f ms  %6.2f clk/record/CU@2.4GHz  %6.0f GB/s%s\n", name, ms,
           ms * 1e-3 * 2.4e9 * 256 / nrec, nrec * 32 / (ms * 1e-3) / 1e9,
           e == hipSuccess ? "" : "  [HIP ERROR]");
}

int main_dep() {
    const int blocks = 2048, count = 16384;  // 3.4e7 records, 1.07 GB
    const long long n = (long long)blocks * count;
    float4* recs; float* out;
    if (hipMalloc(&recs, n * 32) != hipSuccess || hipMalloc(&out, blocks * DB * sizeof(float)) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 1;
    }
    const char* pat[] = {"random", "class16 = lane & 15", "class16 = (lane >> 1) & 15", "class16 = lane >> 2",
                         "class32 = lane & 31", "class32 = lane >> 1"};
    for (int p = 0; p < 6; ++p) {
        hipLaunchKernelGGL(gen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, recs, n, p);
        hipDeviceSynchronize();
        printf("records: %s\n", pat[p]);
        run_dep<0, 16, true>("production order", recs, blocks, count, out);
        if (p != 0) continue;
        run_dep<0, 16, false>("production order, no adds (record stream)", recs, blocks, count, out);
        run_dep<1, 16, true>("(a) batch of 64, bpermute, 16 classes", recs, blocks, count, out);
        run_dep<1, 32, true>("(a) batch of 64, bpermute, 32 classes", recs, blocks, count, out);
        run_dep<2, 16, true>("(b) pool 128, bpermute, 16 classes", recs, blocks, count, out);
        run_dep<2, 32, true>("(b) pool 128, bpermute, 32 classes", recs, blocks, count, out);
        run_dep<3, 16, true, 4, 1>("(c) pool 256 by index, sorted+dealt, 16", recs, blocks, count, out);
        run_dep<3, 16, true, 4, 2>("(c) pool 256 by index, level order, 16", recs, blocks, count, out);
        run_dep<3, 32, true, 4, 2>("(c) pool 256 by index, level order, 32", recs, blocks, count, out);
        run_dep<3, 16, true, 2, 2>("(c) pool 128 by index, level order, 16", recs, blocks, count, out);
        run_dep<3, 16, true, 4, 2, 2>("(c) pool 256, level order, paired reload", recs, blocks, count, out);
        run_dep<3, 16, true, 2, 2, 2>("(c) pool 128, level order, paired reload", recs, blocks, count, out);
        printf(" ablations (no adds = record stream + arranging; wrong lanes where noted)\n");
        run_dep<3, 16, false, 4, 2, 1>("(c) 256 level, no adds", recs, blocks, count, out);
        run_dep<3, 16, false, 4, 2, 2>("(c) 256 level paired, no adds", recs, blocks, count, out);
        run_dep<3, 16, false, 4, 2, 0>("(c) 256 keys+sort, coalesced reload, no adds", recs, blocks, count, out);
        run_dep<3, 16, false, 4, 0, 1>("(c) 256 keys, no sort, permuted reload, no adds", recs, blocks, count, out);
        run_dep<3, 16, false, 4, 0, 2>("(c) 256 keys, no sort, paired reload, no adds", recs, blocks, count, out);
        run_dep<3, 16, false, 4, 0, 0>("(c) 256 keys only, coalesced reload, no adds", recs, blocks, count, out);
        run_dep<3, 16, true, 4, 2, 0>("(c) 256 keys+sort, coalesced reload (random lanes)", recs, blocks, count, out);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 'd') return main_dep();
    int blocks = 256 * 8;
    float* d; hipMalloc(&d, blocks * 256 * sizeof(float));
    const char* names[] = {"ds_add_f32", "ds_add_u32", "ds_write_b32", "ds_add_u64", "racy_rmw",
                           "ds_add_rtn_u32", "ds_add_f64", "ds_max_u32", "ds_add_f64 distinct",
                           "ds_add_f64 random col", "2x ds_add_u64 (2-word fix)",
                           "2x ds_add_u64 (no cvt)"};
    for (int span : {8192, 256}) {
        float t[12];
        t[0] = run<0>(d, blocks, span); t[1] = run<1>(d, blocks, span); t[2] = run<2>(d, blocks, span);
        t[3] = run<3>(d, blocks, span); t[4] = run<4>(d, blocks, span); t[5] = run<5>(d, blocks, span);
        t[6] = run<6>(d, blocks, span); t[7] = run<7>(d, blocks, span);
        t[8] = run<8>(d, blocks, span); t[9] = run<9>(d, blocks, span);
        t[10] = run<10>(d, blocks, span); t[11] = run<11>(d, blocks, span);
        double ops = (double)blocks * 256 * ITERS;
        for (int m = 0; m < 12; ++m)
            printf("span %5d %-24s %8.3f ms  %7.2f G lane-ops/s  %6.2f lane-ops/clk/CU@2.4GHz\n", span, names[m], t[m],
                   ops / t[m] / 1e6, ops / (t[m] * 1e-3) / 256 / 2.4e9);
    }
    return 0;
}
